// Fused HiFi-GAN ResBlock1 "pair" in single-pass bf16 (gfx950), the one-plane form of respair_x3.hip:
//
//   out[b][c][t] = beta*out + alpha*( x + b2 + conv2_{k,dil=1}( bf16( lrelu( b1 + conv1_{k,dil=d}( bf16( lrelu(x) ) ) ) ) ) )
//
// Arithmetic, exactly: both convolutions multiply round-to-nearest bf16 weights (one plane [k][C][C], ci contiguous) by round-to-nearest
// bf16 activations and accumulate in fp32 (v_mfma_f32_32x32x16_bf16; a bf16 x bf16 product is exact in fp32); the intermediate
// lrelu(b1 + conv1(...)) is rounded to bf16 ONCE, into LDS, where conv2 pads it with zeros outside [0, T).  Against two
// conv1d_bf16_kernel launches only the accumulation order may differ (it does not: chunk -> tap -> k-step in both).
//
// Same window rules as the x3 pair (one workgroup = 128 intermediate positions of ALL channels, TT = 128 - (k-1) outputs, odd k,
// (k-1)*dil <= 64).  What the missing lo plane changes: a tap of a 32-channel chunk is 2 MFMAs per wave at C = 32 (6 in the x3 pair) - a
// block barrier and a register-staged weight tile per tap would cost more than the tap.  So all C input channels are one chunk (rows of
// C + 8 bf16: 80 / 144 bytes, conflict-free 16-byte fragment reads) and the weights move in groups of 128 / C taps: 8 (C = 32) or 16
// (C = 64) MFMAs per wave between two barriers, one ds_read_b128 of the window per C / 32 MFMAs plus one of the weights per MFMA - under
// the two reads per MFMA one wave per SIMD can issue before the LDS array saturates.  Occupancy, from the build's metadata: C = 32 takes
// 35 KB of LDS and 88 registers, C = 64 63 KB and 118 - four / two workgroups per CU, which __launch_bounds__(256, 4 / CH) holds the
// compiler to.
#include "kernels.h"
#include "respair_dev.h"


template <int CH>      // C = 32*CH channels
__global__ void __launch_bounds__(256, 4 / CH) respair_bf16_kernel(const PairDev p) {
    constexpr int C = 32 * CH;
    constexpr int P = C + 8;                 // bf16 elements per LDS row
    constexpr int G = 128 / C;               // taps per weight group
    constexpr int XH_EL = PAIR_XW * P, WL_EL = G * C * P;
    // xT (the activated window, conv1 only) and hT (the activated intermediate, conv2 only) share the first XH_EL elements: hT is written
    // after the barrier that ends conv1's last tap group.  The epilogue's staging patches reuse the whole array.
    __shared__ __attribute__((aligned(16))) bf16_t smem[XH_EL + 2 * WL_EL];
    bf16_t* xh = smem;
    bf16_t* wl = smem + XH_EL;               // [buf][tap in group][co][ci]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 5, l31 = lane & 31;
    const int b = blockIdx.z;
    const PairRun r = pair_run(PAIR_T, p.k, p.dil);
    const int TT = r.TT, n0 = r.n0, m0 = r.m0, x0 = r.x0, xw_used = r.xw_used;
    const float* xb = p.x + (int64_t)b * p.bstride;
    const int ngroups = (p.k + G - 1) / G;

    // weight tile of one tap group: G x C rows x C ci = G*C*C/8 pieces of 16 B (taps past k: zero, never multiplied)
    constexpr int WPT = G * C * C / 8 / 256;
    uint4 wreg[WPT];
    auto wload = [&](const bf16_t* wsrc, int jg) {
#pragma unroll
        for (int i = 0; i < WPT; ++i) {
            const int id = tid + i * 256;
            const int t = id / (C * C / 8), rem = id - t * (C * C / 8);
            const int co = rem / (C / 8), pc = rem - co * (C / 8);
            const int j = jg * G + t;
            wreg[i] = j < p.k ? *reinterpret_cast<const uint4*>(wsrc + ((int64_t)j * C + co) * C + pc * 8) : make_uint4(0, 0, 0, 0);
        }
    };
    auto wstore = [&](int buf) {
#pragma unroll
        for (int i = 0; i < WPT; ++i) {
            const int id = tid + i * 256;
            const int t = id / (C * C / 8), rem = id - t * (C * C / 8);
            const int co = rem / (C / 8), pc = rem - co * (C / 8);
            *reinterpret_cast<uint4*>(&wl[buf * WL_EL + (t * C + co) * P + pc * 8]) = wreg[i];
        }
    };

    f32x16 acc[CH];
    auto zero_acc = [&]() {
#pragma unroll
        for (int i = 0; i < CH; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
    };
    // all taps of one convolution: B fragments from rows (32*wave + l31 + j*step) of xh, A fragments from the weight group in LDS.
    // On entry group 0 sits in wl[0] and a barrier has published it; on exit every wave is past its last read of xh and wl.
    auto taps = [&](const bf16_t* wsrc, int step) {
        for (int jg = 0; jg < ngroups; ++jg) {
            const int buf = jg & 1;
            if (jg + 1 < ngroups) wload(wsrc, jg + 1);
#pragma unroll
            for (int t = 0; t < G; ++t) {
                const int j = jg * G + t;
                if (j >= p.k) break;
                const int row = 32 * wave + l31 + j * step;
#pragma unroll
                for (int ks = 0; ks < C / 16; ++ks) {
                    const int kofs = ks * 16 + g * 8;
                    const bf16x8 bv = *reinterpret_cast<const bf16x8*>(&xh[row * P + kofs]);
#pragma unroll
                    for (int i = 0; i < CH; ++i) {
                        const bf16x8 av = *reinterpret_cast<const bf16x8*>(&wl[buf * WL_EL + (t * C + i * 32 + l31) * P + kofs]);
                        acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, bv, acc[i], 0, 0, 0);
                    }
                }
            }
            if (jg + 1 < ngroups) wstore(buf ^ 1);
            __syncthreads();
        }
    };

    // ---- window of x -> LeakyReLU -> bf16 -> xT[t][ci]: a wave owns C/4 CONSECUTIVE channels, a lane one window position per pass
    // (coalesced loads along t, 16-byte LDS writes)
    {
        constexpr int NIT = PAIR_XW / 64, CPW = C / 4;
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int wpos = lane + 64 * it;
            const int idx = x0 + wpos;
            const bool ok = wpos < xw_used && idx >= 0 && idx < p.T;
            float raw[CPW];
#pragma unroll
            for (int e = 0; e < CPW; ++e) raw[e] = ok ? xb[(int64_t)(CPW * wave + e) * p.T + idx] : 0.f;
            if (wpos >= xw_used) continue;
#pragma unroll
            for (int h = 0; h < CPW / 8; ++h) {
                float v[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float t = raw[8 * h + e];               // out-of-range samples were loaded as 0 and lrelu(0) = 0
                    v[e] = t > 0.f ? t : t * p.slope;
                }
                bf16_planes_store<1>(v, &xh[wpos * P + CPW * wave + 8 * h], 0);
            }
        }
    }
    wload(p.w1, 0);
    wstore(0);
    __syncthreads();
    // ---- conv1 (dilated) over the activated window -> intermediate positions m0 + [0,128)
    zero_acc();
    taps(p.w1, p.dil);
    {   // + b1, LeakyReLU, zero outside [0,T), bf16, to hT[t][c] (xT's storage: conv1's last barrier is behind every wave)
        const int m = m0 + 32 * wave + l31;
        const int Tv = pair_valid_len(p, b);
#pragma unroll
        for (int i = 0; i < CH; ++i)
            pair_store_intermediate<1>(acc[i], p.b1 + i * 32, p.slope, m >= 0 && m < Tv, &xh[(32 * wave + l31) * P + i * 32], 0);
    }
    // ---- conv2 (dil 1) over the intermediate -> outputs n0 + [0,TT).  Rows 128 .. 127 + (k-1) of xh are read as well (stale window
    // values, inside the array): they only reach the output columns nl >= TT, which the epilogue drops.
    wload(p.w2, 0);
    wstore(0);
    __syncthreads();           // publishes hT and the first weight group
    zero_acc();
    taps(p.w2, 1);
    // ---- epilogue (respair_dev.h; smem is free: conv2's last barrier is behind every wave)
    static_assert(sizeof(smem) >= PAIR_EPI_FLOATS * sizeof(float), "staging patches must fit");
    pair_epilogue<CH>(acc, reinterpret_cast<float*>(smem), p.staged, xb, p.out + (int64_t)b * p.bstride, p.T, n0, TT, p.b2, p.alpha, p.beta);
}

int launch_respair_bf16(const RespairArgs& a, hipStream_t st) {
    PairLaunch L;
    VB_TRY(pair_fill(a, "respair_bf16", L));
    if (!aligned16(a.w1) || !aligned16(a.w2)) VB_FAIL(VB_E_INVALID, "respair_bf16: weights are not 16-byte aligned");
    ProfScope prof(3, L.flops, L.act_bytes + 2.0 * 2.0 * a.k * a.C * a.C, st);
    if (a.C == 32) hipLaunchKernelGGL(respair_bf16_kernel<1>, L.grid, dim3(256), 0, st, L.d);
    else hipLaunchKernelGGL(respair_bf16_kernel<2>, L.grid, dim3(256), 0, st, L.d);
    VB_CHECK_LAUNCH();
    return VB_OK;
}
