// The epilogue of the split-bf16 / bf16 fused ResBlock1 pairs (respair_x3.hip, respair_bf16.hip), once:
//   out = pair_out_value(alpha, beta, acc, b2[co], x, out)   for the workgroup's outputs n0 + [0, TT) of all 32*CH channels.
// The MFMA accumulator gives a lane ONE output sample and 16 channels; moved like that every residual / accumulate-into load and every store
// is a 4-byte lane access (the direct form, any T).  With 16-byte aligned rows (staged: T % 4 == 0, aligned tensors) each wave passes its
// 32 x 32 tiles through a PRIVATE LDS patch of `stage` (>= PAIR_EPI_FLOATS floats, free once the last tap's barrier is behind every wave; no
// block barrier: only the wave's own writes precede its reads) and comes back with 4 consecutive samples of one channel per lane - 16-byte
// accesses, whole 128-B lines per 8 lanes.  Same arithmetic per element in both forms (see conv_epilogue_staged, conv1d_dev.h).
#pragma once
#include "dma_ring.h"

#define PAIR_EP 36                                   // floats per staged channel row (32 + 4)
#define PAIR_EPI_FLOATS (4 * 32 * PAIR_EP)           // four wave-private patches

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
