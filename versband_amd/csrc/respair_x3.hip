// Fused HiFi-GAN ResBlock1 "pair" for the narrow, long stages of the generator (gfx950):
//
//   out[b][c][t] = beta*out + alpha*( x + b2 + conv2_{k,dil=1}( lrelu( b1 + conv1_{k,dil=d}( lrelu(x) ) ) ) )
//
// (vocoder/hifigan/modules/hifigan.py ResBlock1.forward: xt = lrelu(x); xt = c1(xt); xt = lrelu(xt); xt = c2(xt); x = xt + x)
//
// At C = 64 / 32 channels and T = 240k / 481k samples per clip the two convolutions of a pair are HBM-bound as separate
// launches: x is read, the intermediate written, read again, the residual read and the result written - 5 tensor passes.
// Here one workgroup produces TT = 128-(k-1) output samples of ALL channels and keeps the intermediate in LDS: 2 passes.
//   * window of x (TT + (k-1)(d+1) samples) -> LeakyReLU -> bf16 hi/lo split -> LDS xT[plane][t][ci]  (per 32-ci chunk)
//   * conv1 as split-bf16 ("bf16x3") MFMA implicit GEMM over exactly 128 intermediate positions (one 32-wide MFMA column
//     tile per wave), + b1, LeakyReLU, zero outside [0,T) (conv2 pads the ACTIVATED intermediate), split -> LDS hT
//   * conv2 over hT, + b2 + residual x, alpha/beta accumulation into the MRF sum, coalesced stores (a lane owns one t).
// Same operand precision as conv1d_x3_kernel (operand error 2^-17, fp32 accumulate).
#include "kernels.h"
#include "respair_dev.h"

#define RP_P 40             // bf16 elements per LDS row of a 32-channel chunk (32 + 8 pad: conflict-free 16-B fragment reads)

template <int CH>      // C = 32*CH channels
__global__ void __launch_bounds__(256) respair_x3_kernel(const PairDev p) {
    constexpr int C = 32 * CH;
    // xT (one ci chunk of the activated window, conv1 only) and hT (activated intermediate, all chunks, conv2 only) share
    // storage: hT is written after the barrier that ends conv1's last tap.  41 KB + weights instead of 72 KB: 3 workgroups
    // per CU at 32 channels, 2 at 64 - these kernels are a chain of short phases and live off co-resident workgroups.
    constexpr int XT_EL = 2 * PAIR_XW * RP_P, HT_EL = CH * 2 * PAIR_T * RP_P;
    __shared__ __attribute__((aligned(16))) bf16_t xh[XT_EL > HT_EL ? XT_EL : HT_EL];
    bf16_t (*xT)[PAIR_XW * RP_P] = reinterpret_cast<bf16_t (*)[PAIR_XW * RP_P]>(xh);
    bf16_t (*hT)[2][PAIR_T * RP_P] = reinterpret_cast<bf16_t (*)[2][PAIR_T * RP_P]>(xh);
    __shared__ __attribute__((aligned(16))) bf16_t wl[2][2][C * RP_P];             // [buf][plane] one (tap, ci chunk) of weights

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 5, l31 = lane & 31;
    const int b = blockIdx.z;
    const PairRun r = pair_run(PAIR_T, p.k, p.dil);
    const int TT = r.TT, n0 = r.n0, m0 = r.m0, x0 = r.x0, xw_used = r.xw_used;
    const float* xb = p.x + (int64_t)b * p.bstride;

    // weight tile of one (tap, ci chunk): C rows x 32 ci x 2 planes = C*8 pieces of 16 B
    constexpr int WPT = C * 8 / 256;
    uint4 wreg[WPT];
    auto wload = [&](const bf16_t* wsrc, int c0, int j) {
#pragma unroll
        for (int i = 0; i < WPT; ++i) {
            const int id = tid + i * 256;
            const int pl = id / (C * 4), rem = id - pl * (C * 4);
            const int co = rem >> 2, pc = rem & 3;
            wreg[i] = *reinterpret_cast<const uint4*>(wsrc + pl * p.w_plane + ((int64_t)j * C + co) * C + c0 + pc * 8);
        }
    };
    auto wstore = [&](int buf) {
#pragma unroll
        for (int i = 0; i < WPT; ++i) {
            const int id = tid + i * 256;
            const int pl = id / (C * 4), rem = id - pl * (C * 4);
            const int co = rem >> 2, pc = rem & 3;
            *reinterpret_cast<uint4*>(&wl[buf][pl][co * RP_P + pc * 8]) = wreg[i];
        }
    };
    // activation window staging in two halves (loads of the next chunk fly while the taps of this one are multiplied)
    // (a wave owns 8 CONSECUTIVE channels of the chunk, a lane one window position per pass: coalesced loads along t, ONE 16-byte
    //  LDS write per plane and position - four bank-conflicted 4-byte writes of channel pairs before round 3)
    constexpr int NIT = PAIR_XW / 64;
    float raw[8][NIT];
    auto xload = [&](int c0) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float* xrow = xb + (int64_t)(c0 + 8 * wave + e) * p.T;
#pragma unroll
            for (int it = 0; it < NIT; ++it) {
                const int wpos = lane + 64 * it;
                const int idx = x0 + wpos;
                const bool ok = wpos < xw_used && idx >= 0 && idx < p.T;
                raw[e][it] = ok ? xrow[idx] : 0.f;
            }
        }
    };
    auto xstore = [&]() {
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int wpos = lane + 64 * it;
            if (wpos >= xw_used) continue;
            float v[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float t = raw[e][it];                   // out-of-range samples were loaded as 0 and lrelu(0) = 0
                v[e] = t > 0.f ? t : t * p.slope;
            }
            bf16_planes_store<2>(v, &xT[0][wpos * RP_P + 8 * wave], PAIR_XW * RP_P);
        }
    };

    // two accumulator sets (hi*hi terms / cross terms): consecutive MFMAs never wait for each other's result
    f32x16 acc[CH], acx[CH];
    auto zero_acc = [&]() {
#pragma unroll
        for (int i = 0; i < CH; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) { acc[i][r] = 0.f; acx[i][r] = 0.f; }
    };
    auto fold_acc = [&]() {
#pragma unroll
        for (int i = 0; i < CH; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][r] += acx[i][r];
    };
    // all taps of one ci chunk: B fragments from `src` rows (32*wave + l31 + j*step), A fragments from the weight tile
    auto taps = [&](const bf16_t* wsrc, int c0, const bf16_t* s0, const bf16_t* s1, int step) {
        for (int j = 0; j < p.k; ++j) {
            const int buf = j & 1;
            if (j + 1 < p.k) wload(wsrc, c0, j + 1);
            const int row = 32 * wave + l31 + j * step;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const int kofs = ks * 16 + g * 8;
                const bf16x8 bh = *reinterpret_cast<const bf16x8*>(s0 + row * RP_P + kofs);
                const bf16x8 bl = *reinterpret_cast<const bf16x8*>(s1 + row * RP_P + kofs);
#pragma unroll
                for (int i = 0; i < CH; ++i) {
                    const int o = (i * 32 + l31) * RP_P + kofs;
                    const bf16x8 ah = *reinterpret_cast<const bf16x8*>(&wl[buf][0][o]);
                    const bf16x8 al = *reinterpret_cast<const bf16x8*>(&wl[buf][1][o]);
                    acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc[i], 0, 0, 0);
                    acx[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, acx[i], 0, 0, 0);
                    acx[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acx[i], 0, 0, 0);
                }
            }
            if (j + 1 < p.k) wstore(buf ^ 1);
            __syncthreads();
        }
    };

    // ---- conv1 (dilated) over the activated window -> intermediate positions m0 + [0,128)
    zero_acc();
    xload(0);
#pragma unroll 1
    for (int ch = 0; ch < CH; ++ch) {
        xstore();
        wload(p.w1, ch * 32, 0);
        wstore(0);
        __syncthreads();
        if (ch + 1 < CH) xload((ch + 1) * 32);
        taps(p.w1, ch * 32, &xT[0][0], &xT[1][0], p.dil);
    }
    fold_acc();
    {   // + b1, LeakyReLU, zero outside [0,T), split, to hT[chunk][plane][t][c]
        const int m = m0 + 32 * wave + l31;
        const int Tv = pair_valid_len(p, b);
#pragma unroll
        for (int i = 0; i < CH; ++i)
            pair_store_intermediate<2>(acc[i], p.b1 + i * 32, p.slope, m >= 0 && m < Tv, &hT[i][0][(32 * wave + l31) * RP_P], PAIR_T * RP_P);
    }
    // ---- conv2 (dil 1) over the intermediate -> outputs n0 + [0,TT)
    zero_acc();
#pragma unroll 1
    for (int ch = 0; ch < CH; ++ch) {
        wload(p.w2, ch * 32, 0);
        wstore(0);             // wl[0]'s last readers passed the barrier that ends taps()
        __syncthreads();       // (ch == 0: also publishes hT)
        taps(p.w2, ch * 32, &hT[ch][0][0], &hT[ch][1][0], 1);
    }
    fold_acc();
    // ---- epilogue (respair_dev.h; xh is free: conv2's last barrier is behind every wave)
    static_assert(sizeof(xh) >= PAIR_EPI_FLOATS * sizeof(float), "staging patches must fit");
    pair_epilogue<CH>(acc, reinterpret_cast<float*>(xh), p.staged, xb, p.out + (int64_t)b * p.bstride, p.T, n0, TT, p.b2, p.alpha, p.beta);
}


int launch_respair(const RespairArgs& a, hipStream_t st) {
    PairLaunch L;
    VB_TRY(pair_fill(a, "respair", L));
    ProfScope prof(3, L.flops, L.act_bytes + 2.0 * 4.0 * a.k * a.C * a.C, st);
    // (a persistent variant with both convolutions' weights resident in LDS and the next window prefetched was measured slower,
    //  460 / 900 / 1100 us against 440 / 620 / 830 us for k = 3 / 7 / 11: one workgroup per CU cannot hide its own phase latencies)
    if (a.C == 32) hipLaunchKernelGGL(respair_x3_kernel<1>, L.grid, dim3(256), 0, st, L.d);
    else hipLaunchKernelGGL(respair_x3_kernel<2>, L.grid, dim3(256), 0, st, L.d);
    VB_CHECK_LAUNCH();
    return VB_OK;
}
