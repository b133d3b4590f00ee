// What the fused ResBlock1 pairs share.  All four (respair_x3.hip, respair_bf16.hip, respair_f32.hip, respair_f32w.hip): the run geometry
// (pair_run) and the host-side fill (pair_fill_common); the bf16 pairs their descriptor and checks, the fp32 pairs theirs; all but the
// minimal-filtering pair (whose lanes own two outputs) the epilogue, once:
//   out = pair_out_value(alpha, beta, acc, b2[co], x, out)   for the workgroup's outputs n0 + [0, TT) of all 32*CH channels.
// The MFMA accumulator gives a lane ONE output sample and 16 channels; moved like that every residual / accumulate-into load and every store
// is a 4-byte lane access (the direct form, any T).  With 16-byte aligned rows (staged: T % 4 == 0, aligned tensors) each wave passes its
// 32 x 32 tiles through a PRIVATE LDS patch of `stage` (>= PAIR_EPI_FLOATS floats, free once the last tap's barrier is behind every wave; no
// block barrier: only the wave's own writes precede its reads) and comes back with 4 consecutive samples of one channel per lane - 16-byte
// accesses, whole 128-B lines per 8 lanes.  Same arithmetic per element in both forms (see conv_epilogue_staged, conv1d_dev.h).
#pragma once
#include "conv1d_staged.h"
#include "dma_ring.h"

#define PAIR_EP 36                                   // floats per staged channel row (32 + 4)
#define PAIR_EPI_FLOATS (4 * 32 * PAIR_EP)           // four wave-private patches
#define PAIR_T 128                                   // intermediate positions per workgroup of the x3 / bf16 pairs (4 waves x 32)
#define PAIR_XW (PAIR_T + CONV_HALO)                 // window rows: conv1's halo (k-1)*dil <= CONV_HALO

struct PairDev {
    const float* x; float* out; int64_t bstride; int T;
    int k, dil;
    const bf16_t* w1; const bf16_t* w2; int64_t w_plane;      // [planes][k][C][C] each, ci contiguous (w_plane: unused by the one-plane form)
    const float* b1; const float* b2;
    float slope, alpha, beta;
    int staged;               // 16-B (staged) epilogue: T % 4 == 0 and 16-B aligned tensors
    const int* row_len; int len_mul;      // row lengths (vb_hifigan_forward_lens): device [B], row b's clip ends at row_len[b] * len_mul; null = T (pair_valid_len)
};
// the fp32 pairs (respair_f32.hip; respair_f32w.hip, whose kernel size is a template parameter and whose epilogue is always the staged one)
struct PairF32Dev {
    const float* x; float* out; int64_t bstride; int T;
    int k, dil;
    const float* w1; const float* w2;      // [k][C ci][C co] fp32 each; respair_f32w: minimal-filtering pseudo-taps [P][C ci][C co] (pack.py:pack_conv_mf)
    const float* b1; const float* b2;
    float slope, alpha, beta;
    int staged;
    const int* row_len; int len_mul;      // as PairDev
#ifdef VB_EXPERIMENTS
    int x_nt;          // window DMA with the non-temporal policy (VB_CONV_XNT, see conv1d_f32g.hip)
#endif
};
// One workgroup's run of `run` intermediate positions (PAIR_T; 128 in respair_f32, M in respair_f32w): outputs n0 + [0, TT), intermediate
// positions m0 + [0, run), window samples x0 + [0, xw_used); the DMA-fed windows start on the quad start_al = x0 - aoff
struct PairRun { int h1, h2, TT, n0, m0, x0, xw_used, start_al, aoff; };
__device__ __forceinline__ PairRun pair_run(int run, int k, int dil) {
    PairRun r;
    r.h2 = (k - 1) / 2; r.h1 = (k - 1) * dil / 2;
    r.TT = pair_run_outputs(run, k);
    r.n0 = blockIdx.x * r.TT;
    r.m0 = r.n0 - r.h2;
    r.x0 = r.m0 - r.h1;
    r.xw_used = run + (k - 1) * dil;
    r.start_al = r.x0 & ~3;
    r.aoff = r.x0 - r.start_al;
    return r;
}
// Where conv2's zero padding of the ACTIVATED intermediate starts for row b: the row's own length when the call carries row lengths - the
// clip alone ends there, and the tail of x behind it is zero like the clip-alone call's padding - else T.  The ONE place of a pair kernel
// that reads it is the intermediate mask; window loads and epilogues keep p.T, the row pitch and padded length.
template <class Dev>
__device__ __forceinline__ int pair_valid_len(const Dev& p, int b) { return p.row_len ? p.row_len[b] * p.len_mul : p.T; }
// b1, LeakyReLU, zero outside [0, T) (conv2 pads the ACTIVATED intermediate) and the operand rounding over the conv1 accumulators of channel
// chunk i: this lane's intermediate position (row of hT, `pitch` bf16 each) and 4 x 4 channels from c0 on, NPL planes `plane` apart
template <int NPL>
__device__ __forceinline__ void pair_store_intermediate(const f32x16& acc, const float* b1, float slope, bool inr, bf16_t* row, int plane) {
    const int g = (threadIdx.x & 63) >> 5;
#pragma unroll
    for (int rg = 0; rg < 4; ++rg) {
        const int c = 8 * rg + 4 * g;
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            v[e] = acc[rg * 4 + e] + b1[c + e];
            v[e] = v[e] > 0.f ? v[e] : v[e] * slope;
            if (!inr) v[e] = 0.f;
        }
        bf16_planes_store<NPL>(v, row + c, plane);
    }
}

// ---- host side, after a launcher's own argument checks (`who` prefixes the message): the x / out check, the descriptor, the grid for runs of
// `run` intermediate positions and the profiler's flops (two convolutions of `taps` multiplications per output; the recomputed halo of conv1
// is not counted) and activation bytes
template <class Dev> struct PairLaunchT { Dev d; dim3 grid; double flops, act_bytes; };
template <class Args, class Dev>
static inline int pair_fill_common(const Args& a, const char* who, int run, double taps, PairLaunchT<Dev>& L) {
    if (a.x == a.out) VB_FAIL(VB_E_INVALID, "%s: x and out must be distinct buffers (neighbouring workgroups re-read the halo)", who);
    Dev& d = L.d;
    d.x = a.x; d.out = a.out; d.bstride = (int64_t)a.C * a.T; d.T = a.T; d.k = a.k; d.dil = a.dil;
    d.w1 = a.w1; d.w2 = a.w2; d.b1 = a.b1; d.b2 = a.b2;
    d.slope = a.slope; d.alpha = a.alpha; d.beta = a.beta;
    d.row_len = a.row_len; d.len_mul = a.len_mul;
    d.staged = (a.T % 4 == 0 && aligned16(a.x) && aligned16(a.out) && !vb_tune().conv_direct_epi) ? 1 : 0;
    L.grid = dim3(cdiv(a.T, pair_run_outputs(run, a.k)), 1, a.B);
    L.flops = 2.0 * 2.0 * a.B * (double)a.C * a.C * taps * (double)a.T;
    L.act_bytes = 4.0 * a.B * (double)a.C * a.T * (2.0 + (a.beta != 0.f ? 1.0 : 0.0));
    return VB_OK;
}
// the bf16 pairs: the argument checks of launch_respair / launch_respair_bf16
using PairLaunch = PairLaunchT<PairDev>;
static inline int pair_fill(const RespairArgs& a, const char* who, PairLaunch& L) {
    if (a.C != 32 && a.C != 64) VB_FAIL(VB_E_INVALID, "%s: C=%d (32 or 64)", who, a.C);
    if (a.k < 1 || (a.k & 1) == 0 || (a.k - 1) * a.dil > CONV_HALO || a.k > 33) VB_FAIL(VB_E_INVALID, "%s: k=%d dil=%d", who, a.k, a.dil);
    VB_TRY(pair_fill_common(a, who, PAIR_T, a.k, L));
    L.d.w_plane = (int64_t)a.k * a.C * a.C;
    return VB_OK;
}

template <int CH>
__device__ __forceinline__ void pair_epilogue(f32x16 (&acc)[CH], float* stage, int staged, const float* xb, float* ob, int T, int n0, int TT,
                                              const float* b2, float alpha, float beta) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = lane >> 5, l31 = lane & 31;
    if (staged) {
        float* patch = stage + wave * (32 * PAIR_EP);
        const int rr = lane >> 3, t4 = (lane & 7) * 4;
        const int nl = 32 * wave + t4;
        const int n = n0 + nl;
        const bool nok = nl < TT && n < T;
#pragma unroll
        for (int i = 0; i < CH; ++i) {
#pragma unroll
            for (int r = 0; r < 16; ++r) patch[(4 * g + 8 * (r >> 2) + (r & 3)) * PAIR_EP + l31] = acc[i][r];
            __builtin_amdgcn_s_waitcnt(0xc07f);
            float4 v[4], rv[4], ov[4];
            float bv[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int co = i * 32 + rr + 8 * k;
                v[k] = *reinterpret_cast<const float4*>(patch + (rr + 8 * k) * PAIR_EP + t4);
                const int64_t oi = (int64_t)co * T + (nok ? n : 0);
                rv[k] = nok ? *reinterpret_cast<const float4*>(xb + oi) : make_float4(0.f, 0.f, 0.f, 0.f);
                ov[k] = (nok && beta != 0.f) ? *reinterpret_cast<const float4*>(ob + oi) : make_float4(0.f, 0.f, 0.f, 0.f);
                bv[k] = b2[co];
            }
            __builtin_amdgcn_s_waitcnt(0xc07f);
            if (nok) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int co = i * 32 + rr + 8 * k;
                    const float a4[4] = {v[k].x, v[k].y, v[k].z, v[k].w}, r4[4] = {rv[k].x, rv[k].y, rv[k].z, rv[k].w};
                    const float o4[4] = {ov[k].x, ov[k].y, ov[k].z, ov[k].w};
                    float q[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) q[e] = pair_out_value(alpha, beta, a4[e], bv[k], r4[e], o4[e]);
                    *reinterpret_cast<float4*>(ob + (int64_t)co * T + n) = make_float4(q[0], q[1], q[2], q[3]);
                }
            }
        }
    } else {
        const int nl = 32 * wave + l31;
        const int n = n0 + nl;
        const bool nok = nl < TT && n < T;
#pragma unroll
        for (int i = 0; i < CH; ++i) {
            float rv[16], ov[16], bv[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = i * 32 + 4 * g + 8 * (r >> 2) + (r & 3);
                rv[r] = nok ? xb[(int64_t)co * T + n] : 0.f;
                ov[r] = (nok && beta != 0.f) ? ob[(int64_t)co * T + n] : 0.f;
                bv[r] = b2[co];
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = i * 32 + 4 * g + 8 * (r >> 2) + (r & 3);
                if (!nok) continue;
                ob[(int64_t)co * T + n] = pair_out_value(alpha, beta, acc[i][r], bv[r], rv[r], ov[r]);
            }
        }
    }
}
