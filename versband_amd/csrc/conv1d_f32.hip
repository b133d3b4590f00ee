// fp32 implicit-GEMM Conv1d on the f32 MFMA (v_mfma_f32_32x32x2_f32, exact fp32) for the
// VAE decoder, the HiFi-GAN generator and the DiT stem (gfx950).
//
//   out[b][co][t] = beta*out + alpha*( act_out( acc_scale*sum_{ci,j} W[j][ci][co] * act_in(x[b][ci][t + j*dil - pad]) )
//                                      + bias[co] + res[b][co][t] )
//
//  * activations are [B][C][T] (T contiguous); weights are pre-packed [phase][tap][Ci][Co]
//    (Co contiguous) so both MFMA operands are read from LDS with unit lane stride
//    (A = W[ci][co..co+31], B = x[ci][t..t+31]) - conflict free without swizzles.
//  * per 16-channel chunk the input window (tile + (k-1)*dil halo) is staged ONCE and
//    re-used by all k taps; the pointwise input transform (LeakyReLU, or GroupNorm+swish
//    from precomputed statistics), zero padding and nearest x2 upsampling are applied
//    while staging, so no activated/upsampled tensor ever goes to HBM.
//  * ConvTranspose1d runs as `stride` polyphase sub-convolutions in one launch
//    (grid.z = batch x phase), each with ceil(k/stride) taps.
//  * per-batch "weights" (w_bstride) let the VAE's single-head attention (q^T k and P v)
//    run on the same kernel.
// This file: the register-staged exact-fp32 kernel, which takes every shape, and the one-output-channel kernel.  The descriptor, the route
// among all conv kernels and launch_conv1d are in conv1d.hip.
#include "kernels.h"
#include "conv1d_staged.h"

template <int WM, int WN, int TM, int TN>
__global__ void __launch_bounds__(256) conv1d_f32_kernel(const ConvDev p) {
    constexpr int CO_TILE = WM * TM * 32;
    constexpr int T_TILE = WN * TN * 32;
    constexpr int XW = T_TILE + CONV_HALO;
    __shared__ float xw[CONV_CK * XW];
    __shared__ float wl[2][CONV_CK * CO_TILE];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 5, l31 = lane & 31;
    const int wm = wave / WN, wn = wave % WN;
    ConvTile t;
    if (!conv_tile(p, T_TILE, CO_TILE, t)) return;
    const int b = t.b, n0 = t.n0, co0 = t.co0, in_off = t.in_off, xw_used = t.xw_used, T_eff = t.T_eff;
    const float* xbase = t.xbase;
    const float* wbase = p.w + (int64_t)b * p.w_bstride + (int64_t)t.ph * p.ntaps * p.Ci * p.Co;
    const int cpg = p.gn_groups > 0 ? (p.Ci / p.gn_groups) : 1;

    f32x16 acc[TM][TN];
    conv_zero_acc(acc);

    constexpr int WPT = CONV_CK * CO_TILE / 256;   // weight elements per thread per tap tile
    float wreg[WPT];
    auto wload = [&](int c0, int j) {
#pragma unroll
        for (int i = 0; i < WPT; ++i) {
            int id = tid + i * 256;
            int ci = id / CO_TILE, col = id - ci * CO_TILE;
            int cig = c0 + ci, cog = co0 + col;
            wreg[i] = (cig < p.Ci && cog < p.Co) ? wbase[((int64_t)j * p.Ci + cig) * p.Co + cog] : 0.f;
        }
    };
    auto wstore = [&](int buf) {
#pragma unroll
        for (int i = 0; i < WPT; ++i) wl[buf][tid + i * 256] = wreg[i];
    };

    const int nchunks = (p.Ci + CONV_CK - 1) / CONV_CK;
    for (int ch = 0; ch < nchunks; ++ch) {
        const int c0 = ch * CONV_CK;
        // ---- stage the activated input window of this channel chunk
        for (int ci = wave; ci < CONV_CK; ci += 4) {
            const int cig = c0 + ci;
            const bool cok = cig < p.Ci;
            float gm = 0.f, gr = 1.f, gg = 1.f, gb = 0.f;
            if (cok && (p.in_act == ACT_GN_SWISH || p.in_act == ACT_GN)) {
                const int grp = cig / cpg;
                gm = p.gn_mean[b * p.gn_groups + grp]; gr = p.gn_rstd[b * p.gn_groups + grp];
                gg = p.gn_gamma[cig]; gb = p.gn_beta[cig];
            }
            const float* xrow = xbase + (int64_t)(cok ? cig : 0) * p.T_in;
            for (int wpos = lane; wpos < xw_used; wpos += 64) {
                const int idx = n0 + in_off + wpos;
                float v = 0.f;
                if (cok && idx >= 0 && idx < T_eff) {
                    v = xrow[p.upsample2 ? (idx >> 1) : idx * p.in_stride + p.in_phase];
                    if (p.in_act == ACT_LRELU) {
                        v = v > 0.f ? v : v * p.in_slope;
                    } else if (p.in_act == ACT_GN_SWISH || p.in_act == ACT_GN) {
                        v = (v - gm) * gr * gg + gb;
                        if (p.in_act == ACT_GN_SWISH) v = v / (1.f + __expf(-v));
                    }
                }
                xw[ci * XW + wpos] = v;
            }
        }
        wload(c0, 0);
        wstore(0);
        __syncthreads();
        for (int j = 0; j < p.ntaps; ++j) {
            const int buf = j & 1;
            if (j + 1 < p.ntaps) wload(c0, j + 1);
            const int xoff = j * p.dil;
#pragma unroll
            for (int kk = 0; kk < CONV_CK / 2; ++kk) {
                const int ci = 2 * kk + g;
                float a[TM], bb[TN];
#pragma unroll
                for (int i = 0; i < TM; ++i) a[i] = wl[buf][ci * CO_TILE + (wm * TM + i) * 32 + l31];
#pragma unroll
                for (int jn = 0; jn < TN; ++jn) bb[jn] = xw[ci * XW + (wn * TN + jn) * 32 + l31 + xoff];
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int jn = 0; jn < TN; ++jn)
                        acc[i][jn] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], bb[jn], acc[i][jn], 0, 0, 0);
            }
            if (j + 1 < p.ntaps) wstore(buf ^ 1);
            __syncthreads();
        }
    }

    conv_epilogue<WM, WN, TM, TN>(p, acc, b, n0, co0, t.n_count, t.out_stride, t.out_off);
}

template <int WM, int WN, int TM, int TN>
static void launch_cfg(const ConvDev& d, int n_count, int B, hipStream_t st) {
    dim3 grid(cdiv(n_count, WN * TN * 32), cdiv(d.Co, WM * TM * 32), B * d.phases);
    hipLaunchKernelGGL((conv1d_f32_kernel<WM, WN, TM, TN>), grid, dim3(256), 0, st, d);
}
// (no 128co x 64t tile here: the kernel is the fallback of shapes nothing else takes)
// the tile of a launch (output channels x positions): launch_conv1d_f32 switches on it, vb_conv1d_plan reports it
void conv1d_f32_tile(const ConvDev& d, int* co, int* t) {
    if (d.Co > 64) { *co = 128; *t = 128; } else if (d.Co > 32) { *co = 64; *t = 128; } else { *co = 32; *t = 256; }
}
void launch_conv1d_f32(const ConvDev& d, int n_count, int B, hipStream_t st) {
    int co, t;
    conv1d_f32_tile(d, &co, &t);
    if (co == 128) launch_cfg<2, 2, 2, 2>(d, n_count, B, st);
    else if (co == 64) launch_cfg<2, 2, 1, 2>(d, n_count, B, st);
    else launch_cfg<1, 4, 1, 2>(d, n_count, B, st);
}

// ---------------------------------------------------------------------------------------------------------
// One output channel (HiFi-GAN conv_post: 32 -> 1 channels, k = 7, tanh; vocoder/hifigan/modules/hifigan.py:139-141).  On the MFMA kernels a
// 32-row tile computes one useful row: 860 us for 0.86 GFLOP at 8 clips.  Here a thread owns two output samples and runs the SAME fmaf
// chain the f32 MFMA does (16-channel chunks -> taps -> channels; v_mfma_f32_32x32x2_f32 is a k-ordered fmaf chain, bit for bit), on the
// activated window staged once per chunk in LDS: bit-identical to conv1d_f32_kernel, exact fp32 in both vocoder precisions.
// ---------------------------------------------------------------------------------------------------------
#define C1_TT 512
__global__ void __launch_bounds__(256) conv1d_co1_kernel(const ConvDev p) {
    __shared__ float xs[CONV_CK][C1_TT + CONV_HALO];
    const int tid = threadIdx.x;
    const int b = blockIdx.y, n0 = blockIdx.x * C1_TT;
    const int halo = (p.ntaps - 1) * p.dil, xw = C1_TT + halo;
    const float* xb = p.x + (int64_t)b * p.x_bstride;
    float acc[2] = {0.f, 0.f};
    for (int c0 = 0; c0 < p.Ci; c0 += CONV_CK) {
        for (int i = tid; i < CONV_CK * xw; i += 256) {
            const int ci = i / xw, wpos = i - ci * xw;
            const int idx = n0 - p.pad + wpos;
            float v = 0.f;
            if (c0 + ci < p.Ci && idx >= 0 && idx < p.T_in) {
                v = xb[(int64_t)(c0 + ci) * p.T_in + idx];
                if (p.in_act == ACT_LRELU) v = v > 0.f ? v : v * p.in_slope;
            }
            xs[ci][wpos] = v;
        }
        __syncthreads();
        for (int j = 0; j < p.ntaps; ++j) {
            const float* wj = p.w + (int64_t)j * p.Ci + c0;
#pragma unroll
            for (int ci = 0; ci < CONV_CK; ++ci) {
                const float wv = (c0 + ci < p.Ci) ? wj[ci] : 0.f;
                acc[0] = fmaf(wv, xs[ci][2 * tid + j * p.dil], acc[0]);
                acc[1] = fmaf(wv, xs[ci][2 * tid + 1 + j * p.dil], acc[1]);
            }
        }
        __syncthreads();
    }
    const float bias = p.bias ? p.bias[0] : 0.f;
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const int n = n0 + 2 * tid + e;
        if (n >= p.T_out) continue;
        const int64_t oi = (int64_t)b * p.out_bstride + n;
        const float res = p.res ? p.res[(int64_t)b * p.res_bstride + n] : 0.f;
        const float old = p.beta != 0.f ? p.out[oi] : 0.f;
        p.out[oi] = conv_out_value(p, acc[e], bias, res, old);
    }
}
void conv1d_co1_tile(int* co, int* t) { *co = 1; *t = C1_TT; }
void launch_conv1d_co1(const ConvDev& d, int B, hipStream_t st) {
    hipLaunchKernelGGL(conv1d_co1_kernel, dim3(cdiv(d.T_out, C1_TT), B), dim3(256), 0, st, d);
}
