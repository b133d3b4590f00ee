// Split-bf16 ("bf16x3") implicit-GEMM Conv1d / polyphase ConvTranspose1d (gfx950): conv1d_f32_kernel's implicit GEMM, fused staging and
// epilogue, but every fp32 operand is split on the fly into a bf16 hi/lo pair and each product runs as hi*hi + lo*hi + hi*lo on
// v_mfma_f32_32x32x16_bf16 with fp32 accumulation.  Operand error 2^-17 (fp32-class results, ~3e-5 max relative vs
// the exact-f32 kernel) at 3 bf16 MFMAs per 16-deep k-step: 5.3x the f32-MFMA rate of gfx950 (157 TF vs 2.5 PF/3).
// The activation window is transposed while staging: LDS holds xT[plane][t][ci] (ci contiguous, pitch 80 B so the
// 16-B fragment reads of 16 consecutive t hit 16 distinct slots); weights are pre-packed [plane][tap][co][ci].
// Geometry and weight staging: conv1d_staged.h (shared with conv1d_bf16_kernel, whose window staging is this kernel's as a template).
#include "kernels.h"
#include "conv1d_staged.h"

#define CK3 32
#define CKP3 40      // bf16 elements per LDS row (32 + 8 pad)

// ABL (tuning only): 1 = window staged once, 2 = weights staged once, 3 = no MFMA, 4 = no epilogue
// ABL == 5 is not an ablation but the XT input mode: the window comes from pre-activated, transposed split planes (xt_planes_kernel)
// by DMA (global_load_lds) - no register staging, no per-tile transform/split; LDS rows are 64 B, XOR-swizzled instead of padded.
template <int WM, int WN, int TM, int TN, int ABL = 0>
__global__ void __launch_bounds__(256) conv1d_x3_kernel(const ConvDev p) {
    constexpr int CO_TILE = WM * TM * 32;
    constexpr int T_TILE = WN * TN * 32;
    constexpr int XW = T_TILE + CONV_HALO;
    __shared__ __attribute__((aligned(16))) bf16_t xT[2][XW * CKP3];
    __shared__ __attribute__((aligned(16))) bf16_t wl[2][2][CO_TILE * CKP3];     // [buf][plane]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 5, l31 = lane & 31;
    const int wm = wave / WN, wn = wave % WN;
    ConvTile t;
    if (!conv_tile(p, T_TILE, CO_TILE, t)) return;
    const int b = t.b, ph = t.ph, n0 = t.n0, co0 = t.co0, in_off = t.in_off, out_off = t.out_off, out_stride = t.out_stride, n_count = t.n_count;
    const int xw_used = t.xw_used, T_eff = t.T_eff, xb = t.xb;
    const float* xbase = t.xbase;
    const bf16_t* wbase = p.wp + (int64_t)b * p.wp_bstride + (int64_t)ph * p.ntaps * p.Co * p.Ci_pad;
    const int cpg = p.gn_groups > 0 ? (p.Ci / p.gn_groups) : 1;
    StagedWeights<2, CK3, CKP3, CO_TILE, false> wts;

    f32x16 acc[TM][TN];
    conv_zero_acc(acc);

    // Window staging in two halves, the two-plane form of conv1d_staged.h's StagedWindow, written out here over local copies of the tile's
    // scalars: through the helper, or with the tile read through the struct, every instance spills about ten more SGPRs and the 64co x 128t
    // one runs 6 % slower (profiles/r09_conv_staged_asm.txt, r09_conv_staged_bench.txt).  xload() issues ALL global loads of a chunk (raw
    // values + the per-channel affine of the fused norm), xstore() later applies the pointwise transform, splits to bf16 hi / lo and writes
    // xT[plane][t][ci].  A wave owns 8 CONSECUTIVE channels of the 32-channel chunk and a lane one window position per pass: coalesced
    // loads along t, one 16-byte LDS write per plane and position.
    constexpr int NIT = XW / 64;
    float raw[8][NIT];
    float nsc[8], nsh[8];
    auto xload = [&](int c0) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int ci = c0 + 8 * wave + e;
            const bool cok = ci < p.Ci;
            nsc[e] = 1.f; nsh[e] = 0.f;
            if (cok && (p.in_act == ACT_GN_SWISH || p.in_act == ACT_GN)) {
                const int grp = ci / cpg;
                const float rs = p.gn_rstd[b * p.gn_groups + grp] * p.gn_gamma[ci];
                nsc[e] = rs;
                nsh[e] = p.gn_beta[ci] - p.gn_mean[b * p.gn_groups + grp] * rs;
            }
            const float* xrow = xbase + (int64_t)(cok ? ci : 0) * p.T_in;
#pragma unroll
            for (int it = 0; it < NIT; ++it) {
                const int idx = n0 + in_off + lane + 64 * it;
                const bool ok = cok && (lane + 64 * it) < xw_used && idx >= 0 && idx < T_eff;
                raw[e][it] = ok ? xrow[p.upsample2 ? (idx >> 1) : idx * p.in_stride + p.in_phase] : 0.f;
            }
        }
    };
    auto xstore = [&](int c0) {
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int wpos = lane + 64 * it;
            if (wpos >= xw_used) continue;
            const int idx = n0 + in_off + wpos;
            const bool inr = idx >= 0 && idx < T_eff;
            bf16x8 hi, lo;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                float v = raw[e][it];
                if (inr && (c0 + 8 * wave + e) < p.Ci) {         // zero padding stays zero: the conv pads the ACTIVATED tensor
                    if (p.in_act == ACT_LRELU) {
                        v = v > 0.f ? v : v * p.in_slope;
                    } else if (p.in_act == ACT_GN_SWISH || p.in_act == ACT_GN) {
                        v = v * nsc[e] + nsh[e];
                        if (p.in_act == ACT_GN_SWISH) v = v / (1.f + __expf(-v));
                    }
                } else {
                    v = 0.f;
                }
                hi[e] = f2bf(v);
                lo[e] = f2bf(v - bf2f(hi[e]));
            }
            *reinterpret_cast<bf16x8*>(&xT[0][wpos * CKP3 + 8 * wave]) = hi;
            *reinterpret_cast<bf16x8*>(&xT[1][wpos * CKP3 + 8 * wave]) = lo;
        }
    };

    const int nchunks = (p.Ci + CK3 - 1) / CK3;
    // XT mode: DMA of one chunk's window = xw_used rows x 64 B per plane, in 1-KB pieces of 16 rows; lane -> (row, 16-B slot),
    // the slot holds source chunk slot ^ ((row >> 2) & 3)
    auto xt_issue = [&](int c0) {
        typedef __attribute__((address_space(3))) void* lds_p;
        typedef const __attribute__((address_space(1))) void* glb_p;
        const int P = (xw_used + 15) >> 4;
        for (int q = wave; q < 2 * P; q += 4) {
            const int pl = q >= P, pr = q - pl * P;
            const int row = pr * 16 + (lane >> 2);
            const int c = (lane & 3) ^ ((row >> 2) & 3);
            const bf16_t* src = p.xt + pl * p.xt_plane + ((int64_t)xb * p.xt_Tp + (n0 + in_off + XT_HEAD + row)) * p.Ci + c0 + c * 8;
            __builtin_amdgcn_global_load_lds((glb_p)src, (lds_p)(&xT[pl][pr * 16 * 32]), 16, 0, 0);
        }
    };
    if constexpr (ABL != 5) xload(0);
    for (int ch = 0; ch < nchunks; ++ch) {
        const int c0 = ch * CK3;
        if constexpr (ABL == 5) {
            xt_issue(c0);                       // every wave is past the previous chunk's last tap (barrier below)
            wts.load(p, wbase, co0, c0, 0); wts.store(&wl[0][0][0]);
            __builtin_amdgcn_s_waitcnt(0x0f70);     // vmcnt(0): the window landed
        } else {
        if (ABL != 1 || ch == 0) xstore(c0);
        if (ABL != 2 || ch == 0) { wts.load(p, wbase, co0, c0, 0); wts.store(&wl[0][0][0]); }
        }
        __syncthreads();
        if (ABL != 1 && ABL != 5 && ch + 1 < nchunks) xload(c0 + CK3);
        for (int j = 0; j < p.ntaps; ++j) {
            const int buf = (ABL == 2) ? 0 : (j & 1);
            if (ABL != 2 && j + 1 < p.ntaps) wts.load(p, wbase, co0, c0, j + 1);
            const int xoff = j * p.dil;
#pragma unroll
            for (int ks = 0; ks < CK3 / 16; ++ks) {
                const int kofs = ks * 16 + g * 8;
                bf16x8 ah[TM], al[TM], bh[TN], bl[TN];
#pragma unroll
                for (int i = 0; i < TM; ++i) {
                    const int o = ((wm * TM + i) * 32 + l31) * CKP3 + kofs;
                    ah[i] = *reinterpret_cast<const bf16x8*>(&wl[buf][0][o]);
                    al[i] = *reinterpret_cast<const bf16x8*>(&wl[buf][1][o]);
                }
#pragma unroll
                for (int jn = 0; jn < TN; ++jn) {
                    const int row = (wn * TN + jn) * 32 + l31 + xoff;
                    const int o = (ABL == 5) ? row * 32 + (((kofs >> 3) ^ ((row >> 2) & 3)) << 3) : row * CKP3 + kofs;
                    bh[jn] = *reinterpret_cast<const bf16x8*>(&xT[0][o]);
                    bl[jn] = *reinterpret_cast<const bf16x8*>(&xT[1][o]);
                }
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int jn = 0; jn < TN; ++jn) {
                        if constexpr (ABL == 3) {
                            acc[i][jn][0] += (float)ah[i][0] * (float)bh[jn][0] + (float)al[i][1] * (float)bl[jn][1];
                        } else {
                            acc[i][jn] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bh[jn], acc[i][jn], 0, 0, 0);
                            acc[i][jn] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[i], bh[jn], acc[i][jn], 0, 0, 0);
                            acc[i][jn] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bl[jn], acc[i][jn], 0, 0, 0);
                        }
                    }
            }
            if (ABL != 2 && j + 1 < p.ntaps) wts.store(&wl[buf ^ 1][0][0]);
            __syncthreads();
        }
    }
    if constexpr (ABL == 4) {
        float sink = 0.f;
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int jn = 0; jn < TN; ++jn) sink += acc[i][jn][0] + acc[i][jn][7];
        if (sink == 12345.678f) p.out[0] = sink;
    } else {
        // (the loop's last __syncthreads() is behind every wave: xT is free and holds the four wave-private staging patches)
        static_assert(sizeof(xT) >= 4 * 32 * CE_PITCH * sizeof(float), "staging patches must fit in the window buffer");
        if (p.stage_epi) conv_epilogue_staged<WM, WN, TM, TN>(p, acc, b, n0, co0, n_count, reinterpret_cast<float*>(&xT[0][0]));
        else conv_epilogue<WM, WN, TM, TN>(p, acc, b, n0, co0, n_count, out_stride, out_off);
    }
}

// One workgroup of a 128co x 256t tile per CU would take 92 KB of LDS; the 128co x 128t tile (71 KB) runs two per CU.
int launch_conv1d_x3(const ConvDev& d, ConvTileId tile, int n_count, int B, bool xt, hipStream_t st) {
    if (d.Ci_pad % CK3) VB_FAIL(VB_E_INVALID, "conv1d: split weights need Ci_pad %% %d == 0", CK3);
    if (xt && d.Co <= 64) VB_FAIL(VB_E_INVALID, "conv1d: XT input is built for Co > 64 (wide layers)");
    conv_tile_dispatch(tile, [&](auto wm, auto wn, auto tm, auto tn) {
        constexpr int WM = decltype(wm)::value, WN = decltype(wn)::value, TM = decltype(tm)::value, TN = decltype(tn)::value;
        dim3 grid(cdiv(n_count, WN * TN * 32), cdiv(d.Co, WM * TM * 32), B * d.phases);
        if constexpr (WM * TM == 4) {          // (XT instances exist for the wide tiles only)
            if (xt) { hipLaunchKernelGGL((conv1d_x3_kernel<WM, WN, TM, TN, 5>), grid, dim3(256), 0, st, d); return; }
        }
#ifdef VB_EXPERIMENTS      // ablation instances exist in the experiments build only (tools/conv_bench.py)
        const int abl = vb_tune().conv_ablate;
        if (abl == 1) hipLaunchKernelGGL((conv1d_x3_kernel<WM, WN, TM, TN, 1>), grid, dim3(256), 0, st, d);
        else if (abl == 2) hipLaunchKernelGGL((conv1d_x3_kernel<WM, WN, TM, TN, 2>), grid, dim3(256), 0, st, d);
        else if (abl == 3) hipLaunchKernelGGL((conv1d_x3_kernel<WM, WN, TM, TN, 3>), grid, dim3(256), 0, st, d);
        else if (abl == 4) hipLaunchKernelGGL((conv1d_x3_kernel<WM, WN, TM, TN, 4>), grid, dim3(256), 0, st, d);
        else
#endif
        hipLaunchKernelGGL((conv1d_x3_kernel<WM, WN, TM, TN, 0>), grid, dim3(256), 0, st, d);
    });
    return VB_OK;
}
