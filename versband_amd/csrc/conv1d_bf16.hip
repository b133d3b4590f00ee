// Single-pass bf16 implicit-GEMM Conv1d / polyphase ConvTranspose1d (gfx950): the "bf16" precision of the conv nets.
//
// Arithmetic, exactly:  every product is  RN_bf16(W) * RN_bf16(act_in(x))  - the weights arrive rounded (plane 0 of the split packing,
// pack.py:pack_conv_bf16), the activations are rounded after the fused input transform (LeakyReLU / GroupNorm affine (+ swish) / nearest x2 /
// in_stride, zero padding of the ACTIVATED tensor), exactly where conv1d_x3_kernel splits - and the sum is accumulated in fp32 by
// v_mfma_f32_32x32x16_bf16.  A bf16 x bf16 product is exact in fp32, so the only freedom against that definition is the accumulation order
// (64-channel chunks -> taps -> 16-deep k-steps).  Same ConvDev, same staging (conv1d_staged.h), same two epilogues (conv1d_dev.h) as conv1d_x3_kernel.
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
#include "conv1d_staged.h"

#define BK 64                // input channels per chunk
#define BKP 72               // bf16 elements per LDS row (64 + 8 pad)

template <int WM, int WN, int TM, int TN>
__global__ void __launch_bounds__(256, 2) conv1d_bf16_kernel(const ConvDev p) {
    constexpr int CO_TILE = WM * TM * 32;
    constexpr int T_TILE = WN * TN * 32;
    constexpr int XW = T_TILE + CONV_HALO;
    __shared__ __attribute__((aligned(16))) bf16_t xT[XW * BKP];               // activated window, transposed: [t][ci]
    __shared__ __attribute__((aligned(16))) bf16_t wl[2][CO_TILE * BKP];       // [buf] one (tap, chunk) of weights: [co][ci]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 5, l31 = lane & 31;
    const int wm = wave / WN, wn = wave % WN;
    ConvTile t;
    if (!conv_tile(p, T_TILE, CO_TILE, t)) return;
    const bf16_t* wbase = p.wp + (int64_t)t.b * p.wp_bstride + (int64_t)t.ph * p.ntaps * p.Co * p.Ci_pad;
    StagedWindow<1, BK / 4, XW, BKP> win;            // a wave owns 16 consecutive channels: two 16-byte LDS writes per position
    win.setup(p, wave, lane);
    StagedWeights<1, BK, BKP, CO_TILE, true> wts;    // (a 64-channel chunk can overrun Ci_pad, a multiple of 32)

    f32x16 acc[TM][TN];
    conv_zero_acc(acc);

    const int nchunks = (p.Ci_pad + BK - 1) / BK;
    win.load(p, t, 0);
    for (int ch = 0; ch < nchunks; ++ch) {
        const int c0 = ch * BK;
        const int nks = (p.Ci_pad - c0 >= BK) ? BK / 16 : 2;        // k-steps of this chunk (Ci_pad % 32 == 0)
        win.store(p, t, c0, xT);
        wts.load(p, wbase, t.co0, c0, 0); wts.store(wl[0]);
        __syncthreads();
        if (ch + 1 < nchunks) win.load(p, t, c0 + BK);
        for (int j = 0; j < p.ntaps; ++j) {
            const int buf = j & 1;
            if (j + 1 < p.ntaps) wts.load(p, wbase, t.co0, c0, j + 1);
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
            if (j + 1 < p.ntaps) wts.store(wl[buf ^ 1]);
            __syncthreads();
        }
    }
    // (the loop's last __syncthreads() is behind every wave: xT is free and holds the four wave-private staging patches)
    static_assert(sizeof(xT) >= 4 * 32 * CE_PITCH * sizeof(float), "staging patches must fit in the window buffer");
    if (p.stage_epi) conv_epilogue_staged<WM, WN, TM, TN>(p, acc, t.b, t.n0, t.co0, t.n_count, reinterpret_cast<float*>(&xT[0]));
    else conv_epilogue<WM, WN, TM, TN>(p, acc, t.b, t.n0, t.co0, t.n_count, t.out_stride, t.out_off);
}

// Tiles as conv1d_x3_kernel takes them (conv_staged_tile): 128co x 128t (63 KB of LDS), 128co x 64t (54 KB), 64co x 128t and 32co x 256t
// (45 / 54 KB).  Every instance is held to 256 registers (__launch_bounds__(256, 2)): two workgroups per CU, as the x3 instances have - a
// workgroup's staging and barriers run in the shadow of the other's MFMAs.
int launch_conv1d_bf16(const ConvDev& d, ConvTileId tile, int n_count, int B, hipStream_t st) {
    if (!d.wp || d.Ci_pad != (d.Ci + 31) / 32 * 32) VB_FAIL(VB_E_INVALID, "conv1d: bf16 weights need Ci_pad = Ci rounded up to 32 (Ci %d, Ci_pad %d)", d.Ci, d.Ci_pad);
    if (!aligned16(d.wp)) VB_FAIL(VB_E_INVALID, "conv1d: bf16 weights are not 16-byte aligned");
    conv_tile_dispatch(tile, [&](auto wm, auto wn, auto tm, auto tn) {
        constexpr int WM = decltype(wm)::value, WN = decltype(wn)::value, TM = decltype(tm)::value, TN = decltype(tn)::value;
        dim3 grid(cdiv(n_count, WN * TN * 32), cdiv(d.Co, WM * TM * 32), B * d.phases);
        hipLaunchKernelGGL((conv1d_bf16_kernel<WM, WN, TM, TN>), grid, dim3(256), 0, st, d);
    });
    return VB_OK;
}
