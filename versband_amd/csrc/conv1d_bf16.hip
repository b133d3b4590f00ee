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
//
// XT input mode (XT = true, the analogue of conv1d_x3_kernel's): the 64-channel window chunk is not activated and rounded while staging but
// DMA'd (global_load_lds, 16 B per lane) from the ONE pre-activated, rounded, transposed plane [B][Tp][Ci] that xt_planes_kernel<1> wrote -
// the activation of a wide layer's input then runs once, not once per output-channel tile.  A DMA image is lane-linear, so the window rows
// are 128 B without padding (8 rows per 1-KB wave instruction) and the 16-byte slot of a row is XOR-swizzled with (row >> 1) & 7 instead, the
// swizzle of the GEMM kernels' 64-deep tiles (gemm_tile.h: 16 consecutive rows of a fragment read hit 16 distinct 16-byte slots of the 256-B
// bank line): the DMA lane applies it to the SOURCE chunk it fetches, the fragment read to the chunk it wants.  Weight staging, the k-loop
// and both epilogues are the register-staged form's; layers the conv-as-GEMM route does not take (Ci % 64 != 0, transposed output,
// VB_CONV_GEMM_OFF=1) run here.
#include "kernels.h"
#include "conv1d_staged.h"

#define BK 64                // input channels per chunk
#define BKP 72               // bf16 elements per LDS row (64 + 8 pad)

template <int WM, int WN, int TM, int TN, bool XT = false>
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

    // XT mode: DMA of one chunk's window = xw_used rows x 128 B, in 1-KB pieces of 8 rows (rounded up: the plane has XT_TAIL zero rows behind
    // the clip and XW is a multiple of 8); lane -> (row, 16-byte slot), the slot holds source chunk slot ^ ((row >> 1) & 7).  A last chunk of
    // 32 channels fetches its four chunks twice (slots 4..7 of such a row are never read: two k-steps) instead of reading past the row.
    auto xt_issue = [&](int c0) {
        typedef __attribute__((address_space(3))) void* lds_p;
        typedef const __attribute__((address_space(1))) void* glb_p;
        const int P = (t.xw_used + 7) >> 3;
        for (int q = wave; q < P; q += 4) {
            const int row = q * 8 + (lane >> 3);
            int c = (lane & 7) ^ ((row >> 1) & 7);
            if (c0 + c * 8 >= p.Ci) c &= 3;
            const bf16_t* src = p.xt + ((int64_t)t.xb * p.xt_Tp + (t.n0 + t.in_off + XT_HEAD + row)) * p.Ci + c0 + c * 8;
            __builtin_amdgcn_global_load_lds((glb_p)src, (lds_p)(&xT[q * 8 * BK]), 16, 0, 0);
        }
    };

    const int nchunks = (p.Ci_pad + BK - 1) / BK;
    if constexpr (!XT) win.load(p, t, 0);
    for (int ch = 0; ch < nchunks; ++ch) {
        const int c0 = ch * BK;
        const int nks = (p.Ci_pad - c0 >= BK) ? BK / 16 : 2;        // k-steps of this chunk (Ci_pad % 32 == 0)
        if constexpr (XT) {
            xt_issue(c0);                           // every wave is past the previous chunk's last tap (barrier below)
            wts.load(p, wbase, t.co0, c0, 0); wts.store(wl[0]);
            __builtin_amdgcn_s_waitcnt(0x0f70);     // vmcnt(0): the window landed
        } else {
            win.store(p, t, c0, xT);
            wts.load(p, wbase, t.co0, c0, 0); wts.store(wl[0]);
        }
        __syncthreads();
        if (!XT && ch + 1 < nchunks) win.load(p, t, c0 + BK);
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
                for (int jn = 0; jn < TN; ++jn) {
                    const int row = (wn * TN + jn) * 32 + l31 + xoff;
                    const int o = XT ? row * BK + (((kofs >> 3) ^ ((row >> 1) & 7)) << 3) : row * BKP + kofs;
                    bb[jn] = *reinterpret_cast<const bf16x8*>(&xT[o]);
                }
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
int launch_conv1d_bf16(const ConvDev& d, ConvTileId tile, int n_count, int B, bool xt, hipStream_t st) {
    if (!d.wp || d.Ci_pad != (d.Ci + 31) / 32 * 32) VB_FAIL(VB_E_INVALID, "conv1d: bf16 weights need Ci_pad = Ci rounded up to 32 (Ci %d, Ci_pad %d)", d.Ci, d.Ci_pad);
    if (!aligned16(d.wp)) VB_FAIL(VB_E_INVALID, "conv1d: bf16 weights are not 16-byte aligned");
    if (xt && (d.Co <= 64 || d.Ci % 32 || !aligned16(d.xt))) VB_FAIL(VB_E_INVALID, "conv1d: XT input is built for Co > 64 (wide layers), Ci %% 32 == 0, a 16-byte aligned plane");
    conv_tile_dispatch(tile, [&](auto wm, auto wn, auto tm, auto tn) {
        constexpr int WM = decltype(wm)::value, WN = decltype(wn)::value, TM = decltype(tm)::value, TN = decltype(tn)::value;
        dim3 grid(cdiv(n_count, WN * TN * 32), cdiv(d.Co, WM * TM * 32), B * d.phases);
        if constexpr (WM * TM == 4) {          // (XT instances exist for the wide tiles only)
            if (xt) { hipLaunchKernelGGL((conv1d_bf16_kernel<WM, WN, TM, TN, true>), grid, dim3(256), 0, st, d); return; }
        }
        hipLaunchKernelGGL((conv1d_bf16_kernel<WM, WN, TM, TN>), grid, dim3(256), 0, st, d);
    });
    return VB_OK;
}
