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
#include "respair_epi.h"

#define RB_T 128            // intermediate positions per workgroup (4 waves x 32)
#define RB_HALO 64          // max (k-1)*dil of conv1
#define RB_XW (RB_T + RB_HALO)

struct PairBf16Dev {
    const float* x; float* out; int64_t bstride; int T;
    int k, dil;
    const bf16_t* w1; const bf16_t* w2;      // [k][C][C] each, ci contiguous
    const float* b1; const float* b2;
    float slope, alpha, beta;
    int staged;               // 16-B (staged) epilogue: T % 4 == 0 and 16-B aligned tensors
};

template <int CH>      // C = 32*CH channels
__global__ void __launch_bounds__(256, 4 / CH) respair_bf16_kernel(const PairBf16Dev p) {
    constexpr int C = 32 * CH;
    constexpr int P = C + 8;                 // bf16 elements per LDS row
    constexpr int G = 128 / C;               // taps per weight group
    constexpr int XH_EL = RB_XW * P, WL_EL = G * C * P;
    // xT (the activated window, conv1 only) and hT (the activated intermediate, conv2 only) share the first XH_EL elements: hT is written
    // after the barrier that ends conv1's last tap group.  The epilogue's staging patches reuse the whole array.
    __shared__ __attribute__((aligned(16))) bf16_t smem[XH_EL + 2 * WL_EL];
    bf16_t* xh = smem;
    bf16_t* wl = smem + XH_EL;               // [buf][tap in group][co][ci]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 5, l31 = lane & 31;
    const int b = blockIdx.z;
    const int h2 = (p.k - 1) / 2, h1 = (p.k - 1) * p.dil / 2;
    const int TT = (RB_T - (p.k - 1)) & ~3;          // outputs per workgroup (a multiple of 4: the epilogue moves 16-B quads)
    const int n0 = blockIdx.x * TT;                  // first output sample
    const int m0 = n0 - h2;                          // first intermediate position
    const int x0 = m0 - h1;                          // first window sample
    const int xw_used = RB_T + (p.k - 1) * p.dil;
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
        constexpr int NIT = RB_XW / 64, CPW = C / 4;
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
                bf16x8 v;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float t = raw[8 * h + e];               // out-of-range samples were loaded as 0 and lrelu(0) = 0
                    v[e] = f2bf(t > 0.f ? t : t * p.slope);
                }
                *reinterpret_cast<bf16x8*>(&xh[wpos * P + CPW * wave + 8 * h]) = v;
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
        const bool inr = m >= 0 && m < p.T;
#pragma unroll
        for (int i = 0; i < CH; ++i)
#pragma unroll
            for (int rg = 0; rg < 4; ++rg) {
                const int c = i * 32 + 8 * rg + 4 * g;
                bf16x4 hv;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float v = acc[i][rg * 4 + e] + p.b1[c + e];
                    v = v > 0.f ? v : v * p.slope;
                    if (!inr) v = 0.f;
                    hv[e] = f2bf(v);
                }
                *reinterpret_cast<bf16x4*>(&xh[(32 * wave + l31) * P + c]) = hv;
            }
    }
    // ---- conv2 (dil 1) over the intermediate -> outputs n0 + [0,TT).  Rows 128 .. 127 + (k-1) of xh are read as well (stale window
    // values, inside the array): they only reach the output columns nl >= TT, which the epilogue drops.
    wload(p.w2, 0);
    wstore(0);
    __syncthreads();           // publishes hT and the first weight group
    zero_acc();
    taps(p.w2, 1);
    // ---- epilogue (respair_epi.h; smem is free: conv2's last barrier is behind every wave)
    static_assert(sizeof(smem) >= PAIR_EPI_FLOATS * sizeof(float), "staging patches must fit");
    pair_epilogue<CH>(acc, reinterpret_cast<float*>(smem), p.staged, xb, p.out + (int64_t)b * p.bstride, p.T, n0, TT, p.b2, p.alpha, p.beta);
}

int launch_respair_bf16(const RespairArgs& a, hipStream_t st) {
    if (a.C != 32 && a.C != 64) VB_FAIL(VB_E_INVALID, "respair_bf16: C=%d (32 or 64)", a.C);
    if (a.k < 1 || (a.k & 1) == 0 || (a.k - 1) * a.dil > RB_HALO || a.k > 33) VB_FAIL(VB_E_INVALID, "respair_bf16: k=%d dil=%d", a.k, a.dil);
    if (a.x == a.out) VB_FAIL(VB_E_INVALID, "respair_bf16: x and out must be distinct buffers (neighbouring workgroups re-read the halo)");
    if (!aligned16(a.w1) || !aligned16(a.w2)) VB_FAIL(VB_E_INVALID, "respair_bf16: weights are not 16-byte aligned");
    PairBf16Dev d;
    d.x = a.x; d.out = a.out; d.bstride = (int64_t)a.C * a.T; d.T = a.T; d.k = a.k; d.dil = a.dil;
    d.w1 = a.w1; d.w2 = a.w2; d.b1 = a.b1; d.b2 = a.b2;
    d.slope = a.slope; d.alpha = a.alpha; d.beta = a.beta;
    const int TT = (RB_T - (a.k - 1)) & ~3;
    d.staged = (a.T % 4 == 0 && aligned16(a.x) && aligned16(a.out) && !vb_tune().conv_direct_epi) ? 1 : 0;
    dim3 grid(cdiv(a.T, TT), 1, a.B);
    // two convolutions' worth of flops (the recomputed halo of conv1 is not counted)
    ProfScope prof(3, 2.0 * 2.0 * a.B * (double)a.C * a.C * a.k * (double)a.T,
                   4.0 * a.B * (double)a.C * a.T * (2.0 + (a.beta != 0.f ? 1.0 : 0.0)) + 2.0 * 2.0 * a.k * a.C * a.C, st);
    if (a.C == 32) hipLaunchKernelGGL(respair_bf16_kernel<1>, grid, dim3(256), 0, st, d);
    else hipLaunchKernelGGL(respair_bf16_kernel<2>, grid, dim3(256), 0, st, d);
    VB_CHECK_LAUNCH();
    return VB_OK;
}
