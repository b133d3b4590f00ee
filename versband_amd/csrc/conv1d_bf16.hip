// Single-pass bf16 implicit-GEMM Conv1d / polyphase ConvTranspose1d (gfx950): the "bf16" precision of the conv nets.
//
// Arithmetic, exactly:  every product is  RN_bf16(W) * RN_bf16(act_in(x))  - the weights arrive rounded (plane 0 of the split packing,
// pack.py:pack_conv_bf16), the activations are rounded after the fused input transform (LeakyReLU / GroupNorm affine (+ swish) / nearest x2 /
// in_stride, zero padding of the ACTIVATED tensor), exactly where conv1d_x3_kernel splits - and the sum is accumulated in fp32 by
// v_mfma_f32_32x32x16_bf16.  A bf16 x bf16 product is exact in fp32, so the only freedom against that definition is the accumulation order
// (64-channel chunks -> taps -> 16-deep k-steps).  Same ConvDev, same staging, same two epilogues (conv1d_dev.h) as conv1d_x3_kernel.
//
// Design: what changes when the lo plane goes.  conv1d_x3_kernel reads, per 16-deep k-step of a 2 x 2 register tile, 8 fragments
// (ds_read_b128) for 12 MFMAs and passes a block barrier every 24 MFMAs (one tap of a 32-channel chunk).  With one plane the same loop would
// read 4 fragments for 4 MFMAs and meet a barrier every 8 MFMAs (256 matrix-pipe cycles): the barrier and the register-staged weight tile
// behind it, not the LDS, would set the pace.  The LDS side: a ds_read_b128 takes 4 LDS cycles per wave instruction, and one wave per SIMD can
// issue two of them per v_mfma_f32_32x32x16_bf16 (32 cycles) before the array (256 B/clk/CU) saturates at a third - one read per MFMA, as a
// 2 x 2 tile gives, is half of that, so a larger register tile (2 x 4: 0.75 reads per MFMA, 128 accumulator registers) buys nothing
// the matrix pipe can use and costs the second workgroup per CU (registers).  So the tile stays and the CHUNK deepens: 64 input
// channels per chunk in one plane fill the LDS the two 32-channel planes filled (144-byte rows: 64 + 8 pad, consecutive rows 36 banks
// apart - the 16 rows of a ds_read_b128 lane group hit 16 distinct 16-byte slots), 16 MFMAs run between two barriers and there are half
// as many barriers, weight tiles and window stagings per unit of K.  A last chunk of 32 channels (Ci_pad is a multiple of 32, not 64)
// runs two k-steps instead of four.
#include "kernels.h"
#include "conv1d_dev.h"

#define BK 64                // input channels per chunk
#define BKP 72               // bf16 elements per LDS row (64 + 8 pad)
#define BHALO 64             // max (taps - 1) * dil: launch_conv1d's halo check

template <int WM, int WN, int TM, int TN>
__global__ void __launch_bounds__(256, 2) conv1d_bf16_kernel(const ConvDev p) {
    constexpr int CO_TILE = WM * TM * 32;
    constexpr int T_TILE = WN * TN * 32;
    constexpr int XW = T_TILE + BHALO;
    __shared__ __attribute__((aligned(16))) bf16_t xT[XW * BKP];               // activated window, transposed: [t][ci]
    __shared__ __attribute__((aligned(16))) bf16_t wl[2][CO_TILE * BKP];       // [buf] one (tap, chunk) of weights: [co][ci]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 5, l31 = lane & 31;
    const int wm = wave / WN, wn = wave % WN;
    const int z = blockIdx.z;
    const int b = z / p.phases, ph = z - b * p.phases;
    const int n0 = blockIdx.x * T_TILE;
    const int co0 = blockIdx.y * CO_TILE;

    // polyphase geometry (phases == 1 -> in_off = -pad, out index = n)
    int in_off, out_off, out_stride, n_count;
    if (p.phases == 1) {
        in_off = -p.pad; out_off = 0; out_stride = 1; n_count = p.T_out;
    } else {
        const int u = p.phases;
        const int d = p.tr_pad - ph;
        const int q0 = d > 0 ? (d + u - 1) / u : 0;
        in_off = q0 - (p.ntaps - 1);
        out_off = q0 * u + ph - p.tr_pad;
        out_stride = u;
        n_count = (p.T_out - out_off + u - 1) / u;
    }
    if (n0 >= n_count) return;

    const int halo = (p.ntaps - 1) * p.dil;
    const int xw_used = T_TILE + halo;
    const int T_eff = p.upsample2 ? 2 * p.T_in : (p.T_in - p.in_phase + p.in_stride - 1) / p.in_stride;
    const int xb = p.x_bmod > 0 ? (b % p.x_bmod) : b;
    const float* xbase = p.x + (int64_t)xb * p.x_bstride;
    const bf16_t* wbase = p.wp + (int64_t)b * p.wp_bstride + (int64_t)ph * p.ntaps * p.Co * p.Ci_pad;
    const int cpg = p.gn_groups > 0 ? (p.Ci / p.gn_groups) : 1;

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    // weight tile of one (tap, chunk): CO_TILE rows x 64 ci = CO_TILE*8 pieces of 16 B; rows past Co and channels past Ci_pad are zero
    constexpr int WPT = CO_TILE * 8 / 256;
    uint4 wreg[WPT];
    auto wload = [&](int c0, int j) {
#pragma unroll
        for (int i = 0; i < WPT; ++i) {
            const int id = tid + i * 256;
            const int co = id >> 3, pc = id & 7;
            const int cog = co0 + co, ci = c0 + pc * 8;
            wreg[i] = (cog < p.Co && ci < p.Ci_pad) ? *reinterpret_cast<const uint4*>(wbase + ((int64_t)j * p.Co + cog) * p.Ci_pad + ci)
                                                    : make_uint4(0, 0, 0, 0);
        }
    };
    auto wstore = [&](int buf) {
#pragma unroll
        for (int i = 0; i < WPT; ++i) {
            const int id = tid + i * 256;
            *reinterpret_cast<uint4*>(&wl[buf][(id >> 3) * BKP + (id & 7) * 8]) = wreg[i];
        }
    };

    // activation window staging in two halves, as in conv1d_x3_kernel: xload() issues all global loads of a chunk (a wave owns 16
    // CONSECUTIVE channels, a lane one window position per pass: coalesced along t), xstore() applies the input transform, rounds to bf16
    // and writes the transposed image (two 16-byte LDS writes per position).  The loads of chunk ch+1 fly while chunk ch is multiplied.
    constexpr int NIT = XW / 64;
    constexpr int CPW = BK / 4;              // channels per wave
    float raw[CPW][NIT];
    float nsc[CPW], nsh[CPW];
    auto xload = [&](int c0) {
#pragma unroll
        for (int e = 0; e < CPW; ++e) {
            const int ci = c0 + CPW * wave + e;
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
#pragma unroll
            for (int h = 0; h < CPW / 8; ++h) {
                bf16x8 v;
#pragma unroll
                for (int e8 = 0; e8 < 8; ++e8) {
                    const int e = 8 * h + e8;
                    float t = raw[e][it];
                    if (inr && (c0 + CPW * wave + e) < p.Ci) {       // zero padding stays zero: the conv pads the ACTIVATED tensor
                        if (p.in_act == ACT_LRELU) {
                            t = t > 0.f ? t : t * p.in_slope;
                        } else if (p.in_act == ACT_GN_SWISH || p.in_act == ACT_GN) {
                            t = t * nsc[e] + nsh[e];
                            if (p.in_act == ACT_GN_SWISH) t = t / (1.f + __expf(-t));
                        }
                    } else {
                        t = 0.f;
                    }
                    v[e8] = f2bf(t);
                }
                *reinterpret_cast<bf16x8*>(&xT[wpos * BKP + CPW * wave + 8 * h]) = v;
            }
        }
    };

    const int nchunks = (p.Ci_pad + BK - 1) / BK;
    xload(0);
    for (int ch = 0; ch < nchunks; ++ch) {
        const int c0 = ch * BK;
        const int nks = (p.Ci_pad - c0 >= BK) ? BK / 16 : 2;        // k-steps of this chunk (Ci_pad % 32 == 0)
        xstore(c0);
        wload(c0, 0); wstore(0);
        __syncthreads();
        if (ch + 1 < nchunks) xload(c0 + BK);
        for (int j = 0; j < p.ntaps; ++j) {
            const int buf = j & 1;
            if (j + 1 < p.ntaps) wload(c0, j + 1);
            const int xoff = j * p.dil;
#pragma unroll
            for (int ks = 0; ks < BK / 16; ++ks) {
                if (ks >= nks) break;
                const int kofs = ks * 16 + g * 8;
                bf16x8 a[TM], bb[TN];
#pragma unroll
                for (int i = 0; i < TM; ++i) a[i] = *reinterpret_cast<const bf16x8*>(&wl[buf][((wm * TM + i) * 32 + l31) * BKP + kofs]);
#pragma unroll
                for (int jn = 0; jn < TN; ++jn) bb[jn] = *reinterpret_cast<const bf16x8*>(&xT[((wn * TN + jn) * 32 + l31 + xoff) * BKP + kofs]);
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int jn = 0; jn < TN; ++jn) acc[i][jn] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i], bb[jn], acc[i][jn], 0, 0, 0);
            }
            if (j + 1 < p.ntaps) wstore(buf ^ 1);
            __syncthreads();
        }
    }
    // (the loop's last __syncthreads() is behind every wave: xT is free and holds the four wave-private staging patches)
    static_assert(sizeof(xT) >= 4 * 32 * CE_PITCH * sizeof(float), "staging patches must fit in the window buffer");
    if (p.stage_epi) conv_epilogue_staged<WM, WN, TM, TN>(p, acc, b, n0, co0, n_count, reinterpret_cast<float*>(&xT[0]));
    else conv_epilogue<WM, WN, TM, TN>(p, acc, b, n0, co0, n_count, out_stride, out_off);
}

template <int WM, int WN, int TM, int TN>
static void launch_cfg_bf16(const ConvDev& d, int n_count, int B, hipStream_t st) {
    dim3 grid(cdiv(n_count, WN * TN * 32), cdiv(d.Co, WM * TM * 32), B * d.phases);
    hipLaunchKernelGGL((conv1d_bf16_kernel<WM, WN, TM, TN>), grid, dim3(256), 0, st, d);
}

// Tiles as launch_conv1d picks them for conv1d_x3_kernel: 128co x 128t (63 KB of LDS), or 128co x 64t (54 KB) when the grid of the
// larger tile fills under 70 % of its last round; 64co x 128t and 32co x 256t (45 / 54 KB) for the narrow layers.  Every instance is held
// to 256 registers (__launch_bounds__(256, 2)): two workgroups per CU, as the x3 instances have - a workgroup's staging and barriers
// run in the shadow of the other's MFMAs.
int launch_conv1d_bf16(const ConvDev& d, int n_count, int B, hipStream_t st) {
    if (!d.wp || d.Ci_pad != (d.Ci + 31) / 32 * 32) VB_FAIL(VB_E_INVALID, "conv1d: bf16 weights need Ci_pad = Ci rounded up to 32 (Ci %d, Ci_pad %d)", d.Ci, d.Ci_pad);
    if (!aligned16(d.wp)) VB_FAIL(VB_E_INVALID, "conv1d: bf16 weights are not 16-byte aligned");
    if ((d.ntaps - 1) * d.dil > BHALO) VB_FAIL(VB_E_INVALID, "conv1d: halo %d exceeds %d", (d.ntaps - 1) * d.dil, BHALO);
    const int64_t blocks = (int64_t)cdiv(n_count, 256) * cdiv(d.Co, 128) * B * d.phases;
    const double eff = (double)blocks / (double)(cdiv(blocks, 256) * 256);
    if (d.Co > 64 && eff < 0.7) launch_cfg_bf16<2, 2, 2, 1>(d, n_count, B, st);
    else if (d.Co > 64) launch_cfg_bf16<2, 2, 2, 2>(d, n_count, B, st);
    else if (d.Co > 32) launch_cfg_bf16<2, 2, 1, 2>(d, n_count, B, st);
    else launch_cfg_bf16<1, 4, 1, 2>(d, n_count, B, st);
    return VB_OK;
}
