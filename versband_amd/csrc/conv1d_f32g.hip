// DMA-fed exact-fp32 Conv1d / ConvTranspose1d (v_mfma_f32_32x32x2_f32) - its own translation unit because it is built with
// -mllvm -amdgpu-mfma-vgpr-form (accumulators stay in VGPRs: the asm-pipelined loop below otherwise gets its accumulators copied between
// VGPRs and AGPRs around every ring step); see versband_amd/build.py.
#include <stdlib.h>
#include <type_traits>

#include "conv1d_staged.h"
#include "dma_ring.h"
#include "lds_asm.h"
#include "ring_window.h"
#include "ring_step.h"

// ---------------------------------------------------------------------------------------------------------
// DMA-fed exact-fp32 kernel (round 4).  conv1d_f32_kernel (conv1d_f32.hip) multiplies at 80-93 % of the f32 MFMA rate PER TAP (measured at 8
// clips: +54 us per tap at 32 channels = 146 TF/s, +114 at 64, +125 at 128) but every layer pays 650-800 us before its first tap and
// after its last one: the window of every 16-channel chunk goes global -> registers -> transform -> LDS with nothing in flight, weights
// go through registers once per tap, and the epilogue moves 4-byte lane accesses - the vocoder's 72 ResBlock convolutions spend as long
// there as in their MFMAs (profiles/r04_open_fp32voc_kernel_stats.csv).  This kernel keeps the arithmetic - same 16-channel chunks,
// chunk -> tap -> channel-pair order, one v_mfma_f32_32x32x2_f32 per pair: BIT-IDENTICAL results - and changes how operands arrive:
//   * the raw window of a chunk is DMA'd (global_load_lds, 16 B per lane) into a two-stage LDS ring one chunk ahead; LeakyReLU (in place)
//     and zero padding by the lanes that own the quads (ring_window.h: the feed all four fp32 ring kernels share); GroupNorm + swish inputs
//     are pre-activated by gn_apply_kernel (the builder emits it in fp32 mode: the old kernel redid norm + swish + expf once per
//     output-channel tile, 12x on the 1536-channel layers);
//   * weight tiles [16 ci][CO_TILE] stream through a 4-stage ring, three tiles in flight, counted vmcnt + one raw s_barrier per tap; a
//     tap's fragments go through the pipeline all four fp32 ring kernels share (ring_step.h);
//   * the [b][co][t] result leaves through the staged 16-byte epilogue of the split-bf16 kernel (conv_epilogue_staged);
//   * workgroups are numbered so that one XCD keeps a (time tile, clip) unit for ALL its output-channel tiles: the window is fetched
//     into one L2, the (small) weights into all of them.
// Conditions: conv1d_f32g_eligible below (launch_conv1d falls back to conv1d_f32_kernel otherwise).
// ---------------------------------------------------------------------------------------------------------
// NSW = weight-tile ring stages (4: three tiles in flight; 3: two - 49 KB of LDS with the 96-sample tile, three workgroups per CU)
// ABL (experiments build, timing only - results are wrong): 1 = no fragment reads, 2 = no DMA, 4 = no barrier, 8 = no MFMAs, 16 = no epilogue
// NT = taps per phase as a template parameter (0: runtime loop)
// the kernel's geometry, read by the kernel and by its launcher
template <int WM, int WN, int TM, int TN, bool UPS, int NSW>
struct F32gGeo {
    static constexpr int CO_TILE = WM * TM * 32, T_TILE = WN * TN * 32;
    static constexpr int XP = (T_TILE + 64 + 63) / 64 * 64;      // window pitch (positions): tile + halo (<= 60) + alignment slack (<= 3)
    static constexpr int NP = XP / 64;
    static constexpr int XST = CONV_CK * XP, WT = CONV_CK * CO_TILE;       // floats per window stage / weight tile
    static constexpr int NWI = CO_TILE / 16;                     // 1-KB DMA pieces per weight tile
    static constexpr int WPW = NWI >= 4 ? NWI / 4 : 1;           // ... per wave (narrow tiles: the waves repeat each other's pieces)
    static constexpr int XPW = UPS ? 4 * NP : NP;                // window pieces per wave and chunk (16-B lanes: 4 rows of 64 positions per piece)
    static constexpr int BYTES = (2 * XST + NSW * WT) * (int)sizeof(float);      // two window stages, NSW weight stages
    static_assert(NSW == 3 || NSW == 4, "wait_tile counts at most two tiles ahead");
    static_assert(BYTES >= 4 * 32 * CE_PITCH * sizeof(float), "staging patches must fit in the rings (contiguous)");
};
template <int WM, int WN, int TM, int TN, bool UPS, int NSW, int ABL = 0, int NT = 0>
__global__ void __launch_bounds__(256, 3) conv1d_f32g_kernel(const ConvDev p) {      // three waves per SIMD: <= 168 VGPRs (the unrolled-tap instances of the 128 x 128 tile came out at 171)
    using G = F32gGeo<WM, WN, TM, TN, UPS, NSW>;
    constexpr int CO_TILE = G::CO_TILE, T_TILE = G::T_TILE, XP = G::XP, NP = G::NP, XST = G::XST, WT = G::WT, NWI = G::NWI, WPW = G::WPW, XPW = G::XPW;
    extern __shared__ __attribute__((aligned(16))) float g_lds[];
    float* lx = g_lds;
    float* lw = g_lds + 2 * XST;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 5, l31 = lane & 31;
    const int wm = wave / WN, wn = wave % WN;
    // block -> (channel tile, unit = (time tile, clip, phase)): conv1d_dev.h, beside the numbering.  (The decode stays in its own block
    // with the results assigned, not const-initialised: hipcc allocates the runtime-tap instances of the wide tiles differently otherwise.)
    int b, ph, n0, co0;
    {
        int ct, u;
        if (!conv_xcd_unit(p, ct, u)) return;
        const int z = u / p.g_nt;
        n0 = (u - z * p.g_nt) * T_TILE;
        b = z / p.phases; ph = z - b * p.phases;
        co0 = ct * CO_TILE;
    }
    const ConvPhase pp = conv_phase(p, ph);
    const int in_off = pp.in_off, out_off = pp.out_off, out_stride = pp.out_stride, n_count = pp.n_count;
    if (n0 >= n_count) return;

    const int start = n0 + in_off;
    const int start_al = UPS ? start : (start & ~3);      // 16-B pieces start on a quad of the row (rows are 16-B aligned)
    const int aoff = start - start_al;
    const float* xbase = p.x + (int64_t)b * p.x_bstride;
    const float* wbase = p.w + (int64_t)b * p.w_bstride + (int64_t)ph * p.ntaps * p.Ci * p.Co;      // (w_bstride: per-clip operands, VAE attention)
    float slope = p.in_act == ACT_LRELU ? p.in_slope : 1.f;            // max(v, 1 v) = v: no branch in the fragment path
    vgpr_pin(slope);

    // ---- window DMA and the in-place pass (zero padding + LeakyReLU) over what landed: ring_window.h
    RingWindow<XPW, NP, UPS> win;
    win.setup(wave, lane, start_al, p.T_in);
    auto issue_x = [&](int ch) {
        if constexpr (ABL & 2) return;
        bool nt = false;
#ifdef VB_EXPERIMENTS
        nt = p.x_nt;
#endif
        win.issue(xbase + (int64_t)ch * CONV_CK * p.T_in, lx + (ch & 1) * XST, nt);
    };
    const bool act = p.in_act == ACT_LRELU;
    auto fix_x = [&](int ch) { win.fix(lx + (ch & 1) * XST, act, slope); };
    // ---- weight DMA: tile (chunk, tap) = 16 rows of CO_TILE floats, 1-KB pieces of 256 / CO_TILE rows
    constexpr int RPI = 256 / CO_TILE, LPR = CO_TILE / 4;
    int wsrc[WPW];
#pragma unroll
    for (int i = 0; i < WPW; ++i) {
        const int ii = (wave * WPW + i) % NWI;
        const int row = ii * RPI + lane / LPR;
        int cog = co0 + (lane % LPR) * 4;
        if (cog >= p.Co) cog = 0;                           // channels beyond Co: any valid quad, the rows are never stored
        wsrc[i] = row * p.Co + cog;
    }
    auto issue_w = [&](int ch, int j, int slot) {
        if constexpr (ABL & 2) return;
        const float* src = wbase + ((int64_t)j * p.Ci + ch * CONV_CK) * p.Co;
        float* dst = lw + slot * WT;
#pragma unroll
        for (int i = 0; i < WPW; ++i) {
            const int ii = (wave * WPW + i) % NWI;
            __builtin_amdgcn_global_load_lds((glb_ptr_t)(src + wsrc[i]), (lds_ptr_t)(dst + ii * 256), 16, 0, 0);
        }
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int nchunks = p.Ci / CONV_CK;
    const int total = nchunks * p.ntaps;
    // prologue: window of chunk 0, then the first NSW - 1 weight tiles (issue order = retirement order)
    issue_x(0);
    int nch = 0, nj = 0;                 // tile t + NSW - 1
#pragma unroll
    for (int t = 0; t < NSW - 1; ++t) {
        if (t < total) issue_w(nch, nj, t);
        if (++nj == p.ntaps) { nj = 0; ++nch; }
    }
    float da[TM], dbv[TN];               // held-back operands of a step's last channel pair
#pragma unroll
    for (int i = 0; i < TM; ++i) da[i] = 0.f;
#pragma unroll
    for (int jn = 0; jn < TN; ++jn) dbv[jn] = 0.f;
    // one ring step's multiplications: the fragment pipeline of ring_step.h, TM A fragments and TN B reads per channel pair
    auto multiply = [&](const unsigned xaddr, const unsigned waddr) {
        auto mfma = [&](const float (&a)[TM], const float (&bb)[TN]) {
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int jn = 0; jn < TN; ++jn) {
                    if constexpr (ABL & 8) acc[i][jn][0] += a[i] * bb[jn];
                    else acc[i][jn] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], bb[jn], acc[i][jn], 0, 0, 0);
                }
        };
        ring_step_pairs<CONV_CK / 2, TM, TN, (ABL & 1) != 0>(
            [](auto) { return std::integral_constant<int, TN>{}; },
            [&](auto kc, auto ic, float& v) { lds_rd32<(2 * decltype(kc)::value * CO_TILE + decltype(ic)::value * 32) * 4>(v, waddr); },
            [&](auto kc, auto jc, float& v) { lds_rd32<(2 * decltype(kc)::value * XP + decltype(jc)::value * 32) * 4>(v, xaddr); },
            [&]() {
                // the LAST channel pair of the previous step was held back (operands in registers): its MFMAs are queued here, behind the
                // barrier, the DMA issue and the first two fragment requests of this step - 256 matrix-pipe cycles that cover the first LDS
                // round trip (same box: 810 -> 798 us on the 128 x 128 tile; at three workgroups per CU most of it was hidden already).
                // Same accumulation order (they still precede this step's first pair); the first step queues zeros.
                __builtin_amdgcn_sched_barrier(0);
                mfma(da, dbv);
                __builtin_amdgcn_sched_barrier(0);
            },
            [&](auto kc, const float (&a)[TM], const float (&bb)[TN]) {
                if constexpr (decltype(kc)::value + 1 < CONV_CK / 2) mfma(a, bb);
                else {
#pragma unroll
                    for (int i = 0; i < TM; ++i) da[i] = a[i];
#pragma unroll
                    for (int jn = 0; jn < TN; ++jn) dbv[jn] = bb[jn];
                }
            });
    };
    if constexpr (NT > 0) {
        // ---- the tap count is a template parameter (3 / 7 / 11: the generator's ResBlock layers; the launcher checks p.ntaps == NT): the
        // taps of a chunk are unrolled, every wait count is an immediate and a step's control flow is the ring-slot update alone.  The
        // runtime-tap loop below spends ~50 scalar instructions and ~10 branches per step on it, and scalar work between a barrier and
        // the step's first MFMA costs matrix-pipe time (tools/probe/f32_loop_probe: 151 -> 142 TF/s for ~50 dependent scalar
        // instructions per 32 MFMAs).  Same tiles in the same order: bit-identical.
        static_assert(NT >= NSW - 1, "a step issues the tile NSW - 1 ahead: it lies in this chunk or the next one");
        // (the same bound keeps the J == 0 wait below right: min(AH, NT) * WPW equals the runtime loop's (ahead_all - lag) form only while
        //  NT >= NSW - 2, i.e. lag <= 0 - an NT = 1 / 2 instance on the 4-stage ring would bring back the round-5 tail race)
        static_assert(NT >= NSW - 2, "unrolled-tap wait count assumes no lag between the window and its first weight tile");
        const unsigned xa0 = lds_u32(lx + aoff + wn * TN * 32 + l31 + g * XP);
        const unsigned wa0 = lds_u32(lw + wm * TM * 32 + l31 + g * CO_TILE);
        const int dil4 = p.dil * 4;
        int slot = 0, nslot = NSW - 1;
        for (int ch = 0; ch < nchunks; ++ch) {
            const unsigned xa_ch = xa0 + (ch & 1) * (XST * 4);
            auto chunk = [&](auto lastc) {
                constexpr bool LAST = decltype(lastc)::value;
                static_for<0, NT>([&](auto jc) {
                    constexpr int J = decltype(jc)::value;
                    constexpr int AH = LAST ? (NT - 1 - J < NSW - 2 ? NT - 1 - J : NSW - 2) : NSW - 2;      // younger weight tiles that may fly
                    if constexpr (J == 0) {
                        wait_vmcnt<(AH < NT ? AH : NT) * WPW>();
                        if (act || win.xoob) { fix_x(ch); LDS_WAIT(0); }
                    } else {
                        wait_vmcnt<AH * WPW + ((!LAST && J <= NSW - 2) ? XPW : 0)>();
                    }
                    if constexpr (!(ABL & 4)) __builtin_amdgcn_s_barrier();
                    if constexpr (J == 0 && !LAST) issue_x(ch + 1);
                    if constexpr (J + NSW - 1 < NT) issue_w(ch, J + NSW - 1, nslot);
                    else if constexpr (!LAST) issue_w(ch + 1, J + NSW - 1 - NT, nslot);
                    multiply(xa_ch + J * dil4, wa0 + slot * (WT * 4));
                    if (++slot == NSW) slot = 0;
                    if (++nslot == NSW) nslot = 0;
                });
            };
            if (ch + 1 == nchunks) chunk(std::true_type{}); else chunk(std::false_type{});
        }
    } else {
    int ch = 0, j = 0;                   // tile t = (ch, j)
    int slot = 0, nslot = NSW - 1;
    for (int t = 0; t < total; ++t) {
        const int ahead_all = min(total - 1, t + NSW - 2) - t;
        if (j == 0) {
            // the chunk's window must have landed: it was issued at step t - ntaps in front of tile (t - ntaps + NSW - 1), so of the
            // ahead_all tiles younger than tile t only those from that one on may fly: ahead_all - (NSW - 2 - ntaps) of them when the
            // chunk has fewer taps than the ring runs ahead.  (Round 5: this read min(ahead_all, ntaps), which near the END of a 1-tap
            // layer on the 4-stage ring - no weight tile left to issue behind the window - let the window's last piece fly: rare wrong
            // tiles beside a second GPU process, profiles/r05_conv_tail_race.txt.)
            const int lag = NSW - 2 - p.ntaps;
#ifdef VB_EXPERIMENTS
            if (p.old_tail_wait) wait_tile<WPW, XPW>(ch == 0 ? ahead_all : min(ahead_all, p.ntaps), false);      // the round-4 count (tools/flake_conv.py)
            else
#endif
            wait_tile<WPW, XPW>(ch == 0 || lag <= 0 ? ahead_all : max(ahead_all - lag, 0), false);
            if (act || win.xoob) { fix_x(ch); LDS_WAIT(0); }
        } else {
            // window ch + 1 was issued at this chunk's first tap, in front of tile (t - j + NSW - 1): younger than tile t while j <= NSW - 2
            wait_tile<WPW, XPW>(ahead_all, ch + 1 < nchunks && j <= NSW - 2);
        }
        if constexpr (!(ABL & 4)) __builtin_amdgcn_s_barrier();    // tile t (and the window) landed everywhere; everyone finished tile t - 1
        if (j == 0 && ch + 1 < nchunks) issue_x(ch + 1);
        if (t + NSW - 1 < total) issue_w(nch, nj, nslot);
        multiply(lds_u32(lx + (ch & 1) * XST + aoff + j * p.dil + wn * TN * 32 + l31 + g * XP),
                 lds_u32(lw + slot * WT + wm * TM * 32 + l31 + g * CO_TILE));
        if (++j == p.ntaps) { j = 0; ++ch; }
        if (++nj == p.ntaps) { nj = 0; ++nch; }
        if (++slot == NSW) slot = 0;
        if (++nslot == NSW) nslot = 0;
    }
    }
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int jn = 0; jn < TN; ++jn)
            acc[i][jn] = __builtin_amdgcn_mfma_f32_32x32x2f32(da[i], dbv[jn], acc[i][jn], 0, 0, 0);       // the last step's held-back pair
    __syncthreads();                     // the window ring is free: it holds the four wave-private staging patches now
    if constexpr (ABL & 16) {
        float sum = 0.f;
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int jn = 0; jn < TN; ++jn)
#pragma unroll
                for (int r = 0; r < 16; ++r) sum += acc[i][jn][r];
        if (sum == 1.2345e-33f) p.out[0] = sum;
        return;
    }
    if (p.stage_epi) conv_epilogue_staged<WM, WN, TM, TN>(p, acc, b, n0, co0, n_count, lx);
    else conv_epilogue<WM, WN, TM, TN>(p, acc, b, n0, co0, n_count, out_stride, out_off);
}

template <int WM, int WN, int TM, int TN, bool UPS, int NSW = 4, int ABL = 0, int NT = 0>
static void launch_cfg_g(ConvDev& d, int n_count, int B, hipStream_t st) {
    using G = F32gGeo<WM, WN, TM, TN, UPS, NSW>;
    constexpr int CO_TILE = G::CO_TILE, T_TILE = G::T_TILE, BYTES = G::BYTES;
    const int grid = conv_xcd_grid(d, n_count, T_TILE, CO_TILE, B);
    static OnceFlags once;
    vb_set_max_lds_once(once, (const void*)conv1d_f32g_kernel<WM, WN, TM, TN, UPS, NSW, ABL, NT>, BYTES);
    int bytes = BYTES;
#ifdef VB_EXPERIMENTS
    if (const char* e = getenv("VB_F32G_LDSPAD")) bytes += atoi(e);      // unused LDS: fewer workgroups per CU (tools/flake_conv.py; <= 64 KB in all)
    if (getenv("VB_F32G_NOSTAGE")) d.stage_epi = 0;
    d.old_tail_wait = getenv("VB_F32G_OLDWAIT") ? 1 : 0;
    d.x_nt = getenv("VB_CONV_XNT") ? 1 : 0;
#endif
    hipLaunchKernelGGL((conv1d_f32g_kernel<WM, WN, TM, TN, UPS, NSW, ABL, NT>), dim3(grid), dim3(256), bytes, st, d);
}
// Tile choice for wide layers (Co > 64).  Every configuration walks chunks, taps and channel pairs in the same order - the choice never
// changes a bit of the result - so it is free to follow the launch's size: the busiest CU's load (workgroups on it x tile area) over a
// per-tile efficiency (MFMAs between two barriers: 32 / 24 / 16 / 8 per wave).  8 clips: the vocoder's 128 / 256-channel layers take
// 128 x 128, the 1536 / 768-channel VAE layers 128 x 96 (768 workgroups = one round at three per CU); one or two clips: the VAE layers make
// 48-96 workgroups of those tiles for 256 CUs and take 64 x 128 or 64 x 64 instead (one clip: fp32 conv class 14.6 -> 12.1 ms per pass).
static int g_pick_tile(int n_count, int Co, int B, int phases) {
#ifdef VB_EXPERIMENTS
    if (const char* e = getenv("VB_F32G_PICK")) return atoi(e);       // force a tile configuration (tools/flake_hunt_vae.py)
#endif
    struct Cand { int id, co, t; double eff; };
    static const Cand cands[4] = {{0, 128, 128, 1.00}, {1, 128, 96, 0.95}, {2, 64, 128, 0.85}, {3, 64, 64, 0.70}};
    int best = 0;
    double best_cost = 1e30;
    for (const Cand& c : cands) {
        const int64_t wgs = (int64_t)cdiv(n_count, c.t) * cdiv(Co, c.co) * B * phases;
        const double cost = (double)cdiv(wgs, 256) * c.co * c.t / c.eff;
        if (cost < best_cost * 0.999) { best_cost = cost; best = c.id; }
    }
    return best;
}

// the ResBlock tap counts run the loop with its taps unrolled (template parameter NT); VB_CONV_F32_RT_TAPS=1 keeps the runtime-tap loop
// (the bit-identity test and the A/B)
template <int WM, int WN, int TM, int TN, int NSW>
static void launch_cfg_g_taps(ConvDev& d, int n_count, int B, hipStream_t st) {
    const int nt = vb_tune().conv_f32_rt_taps ? 0 : d.ntaps;
    if (nt == 3) launch_cfg_g<WM, WN, TM, TN, false, NSW, 0, 3>(d, n_count, B, st);
    else if (nt == 7) launch_cfg_g<WM, WN, TM, TN, false, NSW, 0, 7>(d, n_count, B, st);
    else if (nt == 11) launch_cfg_g<WM, WN, TM, TN, false, NSW, 0, 11>(d, n_count, B, st);
    else launch_cfg_g<WM, WN, TM, TN, false, NSW>(d, n_count, B, st);
}
#ifdef VB_EXPERIMENTS
// VB_F32G_ABL (read per launch: tools/conv_f32_ablate.py flips it between launches): the timing-only ablation instances of one wide
// tile (3-stage ring, runtime-tap loop).  Returns whether it launched.
static int f32g_abl() { const char* e = getenv("VB_F32G_ABL"); return e ? atoi(e) : 0; }
template <int WM, int WN, int TM, int TN>
static bool launch_cfg_g_abl(int abl, ConvDev& d, int n_count, int B, hipStream_t st) {
    switch (abl) {
        case 1: launch_cfg_g<WM, WN, TM, TN, false, 3, 1>(d, n_count, B, st); return true;
        case 2: launch_cfg_g<WM, WN, TM, TN, false, 3, 2>(d, n_count, B, st); return true;
        case 4: launch_cfg_g<WM, WN, TM, TN, false, 3, 4>(d, n_count, B, st); return true;
        case 8: launch_cfg_g<WM, WN, TM, TN, false, 3, 8>(d, n_count, B, st); return true;
        case 16: launch_cfg_g<WM, WN, TM, TN, false, 3, 16>(d, n_count, B, st); return true;
        case 3: launch_cfg_g<WM, WN, TM, TN, false, 3, 3>(d, n_count, B, st); return true;
        case 7: launch_cfg_g<WM, WN, TM, TN, false, 3, 7>(d, n_count, B, st); return true;
        case 6: launch_cfg_g<WM, WN, TM, TN, false, 3, 6>(d, n_count, B, st); return true;
        default: return false;
    }
}
#endif
// The kernel's launch conditions: fp32 weights, shared or per clip, 16-byte aligned (tiles and clip strides); an input the window DMA can
// fetch - as 16-byte pieces of aligned rows, or upsampled as 4-byte pieces (UPS; wide single-phase layers only: the 128-channel tiles);
// halo <= 60 (window pitch = tile + 64 with <= 3 positions of alignment slack).
bool conv1d_f32g_eligible(const ConvArgs& a, const ConvDev& d) {
    return !a.wp && a.w_bstride % 4 == 0 && aligned16(a.w) && conv_dma_input(a, d, !a.upsample2) && (d.ntaps - 1) * d.dil <= 60 &&
           (!a.upsample2 || (a.Co > 64 && d.phases == 1));
}
// picks the tile and launches; the caller (launch_conv1d) has checked conv1d_f32g_eligible
// the upsampled form's tile: 128 x 96 where its rounds of 256 workgroups cover fewer positions than 128 x 128's
static bool g_ups_96(int n_count, int Co, int B) {
    const int64_t w128 = (int64_t)cdiv(n_count, 128) * cdiv(Co, 128) * B, w96 = (int64_t)cdiv(n_count, 96) * cdiv(Co, 128) * B;
    return cdiv(w96, 256) * 96 < cdiv(w128, 256) * 128;
}
// the tile launch_conv1d_f32g takes (output channels x positions), from the same pickers: what vb_conv1d_plan reports
void conv1d_f32g_tile(const ConvDev& d, int n_count, int B, int upsample2, int* co, int* t) {
    static const int wide[4][2] = {{128, 128}, {128, 96}, {64, 128}, {64, 64}};
    if (upsample2) { *co = 128; *t = g_ups_96(n_count, d.Co, B) ? 96 : 128; }
    else if (d.Co > 64) { const int id = g_pick_tile(n_count, d.Co, B, d.phases) & 3; *co = wide[id][0]; *t = wide[id][1]; }
    else if (d.Co > 32) { *co = 64; *t = 128; }
    else { *co = 32; *t = 256; }
}
void launch_conv1d_f32g(ConvDev& d, int n_count, int B, int upsample2, hipStream_t st) {
    int tile_co, tile_t;
    conv1d_f32g_tile(d, n_count, B, upsample2, &tile_co, &tile_t);
    if (upsample2) {
        if (tile_t == 96) launch_cfg_g<4, 1, 1, 3, true, 3>(d, n_count, B, st);
        else launch_cfg_g<2, 2, 2, 2, true, 3>(d, n_count, B, st);
    } else if (d.Co > 64) {
#ifdef VB_EXPERIMENTS
        if (const char* e = getenv("VB_F32G_TILE")) {       // tile shapes measured and not adopted
            if (atoi(e) == 2) { launch_cfg_g_taps<2, 2, 1, 2, 3>(d, n_count, B, st); return; }      // 64 x 128, 3 stages: 36.5 KB, four workgroups per CU
            if (atoi(e) == 3) { launch_cfg_g_taps<1, 4, 2, 1, 3>(d, n_count, B, st); return; }      // 64 x 128 as 1 x 4 waves of 2 x 1 tiles
        }
#endif
        switch (g_pick_tile(n_count, d.Co, B, d.phases)) {
            case 1:
#ifdef VB_EXPERIMENTS
                if (f32g_abl() == 100) { launch_cfg_g_taps<2, 2, 2, 2, 3>(d, n_count, B, st); return; }      // the 128 x 128 tile on this launch
                if (launch_cfg_g_abl<4, 1, 1, 3>(f32g_abl(), d, n_count, B, st)) return;
#endif
                launch_cfg_g_taps<4, 1, 1, 3, 3>(d, n_count, B, st); break;
            case 2: launch_cfg_g<2, 2, 1, 2, false, 4>(d, n_count, B, st); break;
            case 3: launch_cfg_g<2, 2, 1, 1, false, 3>(d, n_count, B, st); break;
#ifdef VB_EXPERIMENTS
            case 4: launch_cfg_g<2, 2, 1, 2, false, 3>(d, n_count, B, st); break;      // (VB_F32G_PICK only) 64 x 128 on a 3-stage weight ring
            case 5: launch_cfg_g<1, 4, 1, 2, false, 4>(d, n_count, B, st); break;      // (VB_F32G_PICK only) 32 x 256
#endif
            default:
#ifdef VB_EXPERIMENTS
                if (launch_cfg_g_abl<2, 2, 2, 2>(f32g_abl(), d, n_count, B, st)) return;
#endif
                launch_cfg_g_taps<2, 2, 2, 2, 3>(d, n_count, B, st);     // 3-stage ring: 49 KB, three workgroups per CU (31.3 -> 30.4 ms per pass against 4 stages / two)
        }
    } else if (tile_co == 64) launch_cfg_g<2, 2, 1, 2, false>(d, n_count, B, st);
    else launch_cfg_g<1, 4, 1, 2, false>(d, n_count, B, st);
}
