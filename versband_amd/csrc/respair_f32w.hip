// Fused HiFi-GAN ResBlock1 pair in fp32 with F(2,3) minimal filtering, 32 channels (gfx950; round 6).
//
//   out[b][c][t] = beta*out + alpha*( x + b2 + conv2_{k,1}( lrelu( b1 + conv1_{k,d}( lrelu(x) ) ) ) )      (vocoder/hifigan/modules/hifigan.py:27-64)
//
// respair_f32.hip's idea - one workgroup produces a run of output samples of ALL channels, the intermediate never leaves LDS - with
// conv1d_f32w.hip's arithmetic: every 3-tap group of a filter is 4 pseudo-taps for 2 neighbouring outputs of a dilation class (mf_taps.h), the
// four product sums m0..m3 are four MFMA accumulators, y0 = (m0 + m1) + m2 and y1 = (m1 - m2) - m3 are formed once per convolution.  Same chunk ->
// pseudo-tap -> channel-pair order as conv1d_f32w_kernel and the same epilogue arithmetic - but NOT the same bits as two conv1d_f32w launches: the
// even and the odd output of a pair are different sums, and the intermediate run of a workgroup starts (k - 1) / 2 positions in front of its outputs,
// so a position can be the even member here and the odd one there (one ulp on ~1/3 of the elements; both equally close to float64, tests/test_gpu_kernels.py).
// A clip's bits depend on its positions only, never on the batch.
//
// Shape, C = 32.  4 waves, all along time: wave w owns MFMA columns v = 0..31 = 2 x 32 positions.  conv1 (dilation d): column v = (q, r), r < d, owns the
// intermediate positions 2dq + r and 2dq + r + d of the wave's 2 VW, VW = (32 / d) d; the workgroup's intermediate run is M = 8 VW (256 at d = 1, 240 at
// d = 3 / 5).  conv2 (dilation 1): column v owns outputs 2v, 2v + 1 of the wave's 64; the workgroup stores TT = (M - (k - 1)) & ~3 outputs.
// LDS: window ring 2 x [16 ci][320] (both 16-channel chunks of x are requested up front), the intermediate h[32][272] aliases it, weight ring of 3 tiles
// [TPS pseudo-taps][16 ci][32 co] (TPS = 4: 32 MFMAs per ring step and wave; k = 3 has 4 pseudo-taps in all and runs TPS = 2) = 64 KB, two workgroups
// per CU.  The whole schedule - 2 convolutions x 2 chunks x ceil(P / TPS) ring steps - is unrolled: every wait count, tap offset and tile index is an
// immediate.  Ring / counted vmcnt as in respair_f32_kernel; window feed: ring_window.h; fragment pipeline: ring_step.h; run
// geometry and host-side fill: respair_dev.h.
// C = 64: the waves are 2 (time) x 2 (channel halves) - a wave computes 32 of the 64 output channels of its 64 positions in BOTH convolutions, so the
// accumulators stay 4 x 16 registers; runs of M = 4 VW = 128 / 120 intermediate positions, window pitch 192, h[64][144] = 37 KB, tiles of TPS = 2 pseudo-taps
// [2][16][64] = 8 KB: 61 KB, two workgroups per CU; the four 16-channel windows go through the two-stage ring (chunk c + 1 is requested at chunk c's first step).
#include <stdlib.h>
#include <type_traits>

#include "respair_dev.h"
#include "lds_asm.h"
#include "ring_window.h"
#include "ring_step.h"
#include "mf_taps.h"

#define PW_GK 16
#define PW_EP 68             // staged epilogue patch pitch (64 positions + 4)

// the kernel's geometry, read by the kernel and by its launcher
template <int TPS, int C>
struct PairWGeo {
    static constexpr int NSW = 3;
    static constexpr int WC = C / 32, WTW = 4 / WC;            // waves along the channels / along time
    static constexpr int XP = WTW * 64 + 64;                   // window pitch: the run + halo (<= 60) + alignment slack (<= 3)
    static constexpr int HP = WTW * 64 + 16;                   // intermediate pitch: the run + (k - 1 <= 16)
    static constexpr int XST = PW_GK * XP;                     // floats per window stage
    static constexpr int WT = TPS * PW_GK * C;                 // floats per weight tile [TPS][16 ci][C co]
    static constexpr int PPT = PW_GK * C / 256, NPIECE = WT / 256;      // 1-KB DMA pieces per pseudo-tap / per weight tile
    static_assert(NPIECE % 4 == 0, "every wave issues the same number of pieces");
    static constexpr int WPW = NPIECE / 4;
    static constexpr int NP = XP / 64, XPW = NP;               // window pieces per wave and chunk (16 rows x XP / 256 floats / 4 waves)
    static constexpr int XH0 = 2 * XST > C * HP ? 2 * XST : C * HP;      // window ring, intermediate and epilogue patches share storage
    static constexpr int XH = XH0 > 4 * 32 * PW_EP ? XH0 : 4 * 32 * PW_EP;
    static constexpr int BYTES = (XH + NSW * WT) * (int)sizeof(float);
    // intermediate positions per workgroup at dilation dil (VW columns in use per wave)
    __host__ __device__ static constexpr int run(int dil) { return WTW * 2 * ((32 / dil) * dil); }
};
template <int K, int TPS, int C>
__global__ void __launch_bounds__(256, 2) respair_f32w_kernel(const PairF32Dev p) {
    using G = PairWGeo<TPS, C>;
    constexpr int NSW = G::NSW, WC = G::WC, WTW = G::WTW, XP = G::XP, HP = G::HP, XST = G::XST, WT = G::WT, PPT = G::PPT, WPW = G::WPW, NP = G::NP, XPW = G::XPW;
    constexpr int XH = G::XH;
    constexpr int NCH = C / PW_GK;                      // 16-channel chunks per convolution
    constexpr int P = mf_ntaps(K);
    constexpr int KNS = (P + TPS - 1) / TPS;            // ring steps per 16-channel chunk
    constexpr int NT = 2 * NCH * KNS;                   // conv1 chunks, then conv2 chunks
    static_assert(NT >= NSW, "ring");
    extern __shared__ __attribute__((aligned(16))) float pw_lds[];
    float* lx = pw_lds;                                 // window ring; then h[c][HP]; then the epilogue patches
    float* lw = pw_lds + XH;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wt = wave % WTW, wc = wave / WTW;          // this wave's time slot and channel half
    const int g = lane >> 5, l31 = lane & 31;
    const int b = blockIdx.z;
    const int dil = p.dil;
    const int VW = (32 / dil) * dil;
    const PairRun r = pair_run(G::run(dil), K, dil);     // respair_dev.h
    const int TT = r.TT, n0 = r.n0, m0 = r.m0, start_al = r.start_al, aoff = r.aoff;
    const float* xb = p.x + (int64_t)b * p.bstride;
    float slope = p.slope;
    vgpr_pin(slope);

    // ---- window DMA: chunk c -> stage c & 1, chunks 0 and 1 now; LeakyReLU + zero padding in place over what landed: ring_window.h
    RingWindow<XPW, NP> win;
    win.setup(wave, lane, start_al, p.T);
    auto issue_x = [&](int ch) { win.issue(xb + (int64_t)ch * PW_GK * p.T, lx + (ch & 1) * XST); };
    issue_x(0);
    issue_x(1);
    auto fix_x = [&](int ch) { win.fix(lx + (ch & 1) * XST, std::true_type{}, slope); };
    // ---- weight DMA: tile t = (conv, chunk, step): pseudo-taps [s TPS, s TPS + TPS) of 16 input channels; a piece = 256 consecutive floats of the
    // pseudo-tap's [16 ci][C co] block
    auto issue_w = [&](auto tc) {
        constexpr int T_ = decltype(tc)::value;
        constexpr int CONV = T_ / (NCH * KNS), CH = (T_ / KNS) % NCH, S = T_ % KNS, SLOT = T_ % NSW;
        const float* wsrc = CONV ? p.w2 : p.w1;
        float* dst = lw + SLOT * WT;
#pragma unroll
        for (int i = 0; i < WPW; ++i) {
            const int piece = wave * WPW + i;
            const int tap = piece / PPT, sub = piece - tap * PPT;
            int j = S * TPS + tap;
            if (j > P - 1) j = P - 1;                  // pseudo-taps beyond P: a valid block, never multiplied
            const float* src = wsrc + ((int64_t)j * C + CH * PW_GK) * C + sub * 256 + lane * 4;
            __builtin_amdgcn_global_load_lds((glb_ptr_t)src, (lds_ptr_t)(dst + piece * 256), 16, 0, 0);
        }
    };
    issue_w(std::integral_constant<int, 0>{});
    issue_w(std::integral_constant<int, 1>{});

    f32x16 acc[4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[a][r] = 0.f;

    // column v -> the even position inside the wave's range (conv1: dilation classes; conv2: 2 v)
    const int vcol = l31 < VW ? l31 : 0;
    const int vq = vcol / dil;
    const int bpos = 2 * dil * vq + (vcol - vq * dil);
    const unsigned wa0 = lds_u32(lw + g * C + wc * 32 + l31);
    const unsigned xa0 = lds_u32(lx + g * XP + aoff + wt * 2 * VW + bpos);
    const unsigned ha0 = lds_u32(lx + g * HP + wt * 64 + 2 * l31);
    const int dil4 = dil * 4;

    // + b1, LeakyReLU, zero outside [0, T) (conv2 pads the ACTIVATED intermediate) -> h[c][m]; the window ring is dead by then
    auto middle = [&]() {
#pragma clang fp contract(off)
        const int mrel = wt * 2 * VW + bpos;
        const int ma = m0 + mrel;
        const int Tv = pair_valid_len(p, b);
        const bool ok0 = l31 < VW && ma >= 0 && ma < Tv, ok1 = l31 < VW && ma + dil >= 0 && ma + dil < Tv;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int c = wc * 32 + 8 * (r >> 2) + 4 * g + (r & 3);
            const float bb = p.b1[c];
            float y0 = (acc[0][r] + acc[1][r]) + acc[2][r];
            float y1 = (acc[1][r] - acc[2][r]) - acc[3][r];
            y0 = y0 + bb; y1 = y1 + bb;
            y0 = y0 > 0.f ? y0 : y0 * p.slope;
            y1 = y1 > 0.f ? y1 : y1 * p.slope;
            if (l31 < VW) {
                lx[c * HP + mrel] = ok0 ? y0 : 0.f;
                lx[c * HP + mrel + dil] = ok1 ? y1 : 0.f;
            }
#pragma unroll
            for (int a = 0; a < 4; ++a) acc[a][r] = 0.f;
        }
        __builtin_amdgcn_s_waitcnt(0xc07f);
        __builtin_amdgcn_s_barrier();
    };

    // ---- the unrolled schedule.  Issue order: windows 0, 1, tiles 0, 1; then per step [window c + 1 at conv1 chunk c's first step, c >= 1], tile t + 2.
    // In front of step t the loads younger than tile t are: the window step t - 1 issued (if it did) and tile t + 1.
    static_for<0, NT>([&](auto tc) {
        constexpr int T_ = decltype(tc)::value;
        constexpr int CONV = T_ / (NCH * KNS), CH = (T_ / KNS) % NCH, S = T_ % KNS, SLOT = T_ % NSW;
        constexpr int TP_ = T_ > 0 ? T_ - 1 : 0;        // the previous step: did it request a window?
        constexpr bool PREV_WIN = T_ > 0 && (TP_ / (NCH * KNS)) == 0 && (TP_ % KNS) == 0 && ((TP_ / KNS) % NCH) >= 1 && ((TP_ / KNS) % NCH) + 1 < NCH;
        constexpr int AHEAD = (NT - 1 - T_) < (NSW - 2) ? (NT - 1 - T_) : (NSW - 2);       // younger weight tiles that may fly
        wait_vmcnt<AHEAD * WPW + (PREV_WIN ? XPW : 0)>();
        if constexpr (CONV == 0 && S == 0) { fix_x(CH); LDS_WAIT(0); }
        __builtin_amdgcn_s_barrier();          // tile T_ (and its window) landed everywhere; everyone finished step T_ - 1
        if constexpr (CONV == 0 && S == 0 && CH >= 1 && CH + 1 < NCH) issue_x(CH + 1);      // -> the stage chunk CH - 1 has left
        if constexpr (T_ + NSW - 1 < NT) issue_w(std::integral_constant<int, T_ + NSW - 1>{});
        if constexpr (CONV == 1 && CH == 0 && S == 0) middle();
        constexpr int J0 = S * TPS;
        constexpr int NTAP = (P - J0) < TPS ? (P - J0) : TPS;
        constexpr int NM = NTAP * 8;
        const unsigned waddr = wa0 + SLOT * (WT * 4);
        const unsigned baddr = CONV ? ha0 + CH * (PW_GK * HP * 4) : xa0 + (CH & 1) * (XST * 4);
        auto tap = [](auto mc) { return std::integral_constant<int, J0 + decltype(mc)::value / 8>{}; };      // pair m's pseudo-tap
        ring_step_pairs<NM, 1, 2>(
            [&](auto mc) { return std::integral_constant<int, mf_reads(mf_tap(K, decltype(tap(mc))::value))>{}; },
            [&](auto mc, auto, float& v) { constexpr int MM = decltype(mc)::value; lds_rd32<((MM / 8 * PW_GK + 2 * (MM % 8)) * C) * 4>(v, waddr); },
            [&](auto mc, auto jc, float& v) {
                constexpr int KK = decltype(mc)::value % 8;
                constexpr MfTap MT = mf_tap(K, decltype(tap(mc))::value);
                constexpr int O = decltype(jc)::value ? MT.ob : MT.oa;
                if constexpr (CONV) lds_rd32<(2 * KK * HP + O) * 4>(v, baddr);
                else lds_rd32<(2 * KK * XP) * 4>(v, baddr + O * dil4);
            },
            []() {},
            [&](auto mc, const float (&fa)[1], const float (&x)[2]) {
                constexpr MfTap MT = mf_tap(K, decltype(tap(mc))::value);
                acc[MT.acc] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[0], mf_operand<MT.op>(x), acc[MT.acc], 0, 0, 0);
            });
    });
    __syncthreads();                     // h is dead: its storage holds the four wave-private staging patches now

    // ---- epilogue: y0 / y1, staged through a wave-private patch [32 co][64 positions], + b2 + residual x, alpha / beta, 16-byte stores
    {
#pragma clang fp contract(off)
        float* patch = lx + wave * (32 * PW_EP);
        float* ob = p.out + (int64_t)b * p.bstride;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float y0 = (acc[0][r] + acc[1][r]) + acc[2][r];
            const float y1 = (acc[1][r] - acc[2][r]) - acc[3][r];
            float* row = patch + (4 * g + 8 * (r >> 2) + (r & 3)) * PW_EP + 2 * l31;
            row[0] = y0; row[1] = y1;
        }
        __builtin_amdgcn_s_waitcnt(0xc07f);
        const int rr = lane >> 4, t4 = (lane & 15) * 4;
        const int nl = wt * 64 + t4;
        const int n = n0 + nl;
        const bool nok = nl < TT && n < p.T;
#pragma unroll
        for (int kh = 0; kh < 2; ++kh) {
            float4 v[4], rv[4], ov[4];
            float bv[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int cl = rr + 4 * (kh * 4 + q), co = wc * 32 + cl;
                v[q] = *reinterpret_cast<const float4*>(patch + cl * PW_EP + t4);
                const int64_t oi = (int64_t)co * p.T + (nok ? n : 0);
                rv[q] = nok ? *reinterpret_cast<const float4*>(xb + oi) : make_float4(0.f, 0.f, 0.f, 0.f);
                ov[q] = (nok && p.beta != 0.f) ? *reinterpret_cast<const float4*>(ob + oi) : make_float4(0.f, 0.f, 0.f, 0.f);
                bv[q] = p.b2[co];
            }
            if (nok) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int co = wc * 32 + rr + 4 * (kh * 4 + q);
                    float4 o;
                    o.x = pair_out_value(p.alpha, p.beta, v[q].x, bv[q], rv[q].x, ov[q].x); o.y = pair_out_value(p.alpha, p.beta, v[q].y, bv[q], rv[q].y, ov[q].y);
                    o.z = pair_out_value(p.alpha, p.beta, v[q].z, bv[q], rv[q].z, ov[q].z); o.w = pair_out_value(p.alpha, p.beta, v[q].w, bv[q], rv[q].w, ov[q].w);
                    *reinterpret_cast<float4*>(ob + (int64_t)co * p.T + n) = o;
                }
            }
        }
    }
}

template <int K, int TPS, int C>
static void launch_pair_w(const PairF32Dev& d, dim3 grid, hipStream_t st) {
    constexpr int BYTES = PairWGeo<TPS, C>::BYTES;
    static OnceFlags once;
    vb_set_max_lds_once(once, (const void*)respair_f32w_kernel<K, TPS, C>, BYTES);
    hipLaunchKernelGGL((respair_f32w_kernel<K, TPS, C>), grid, dim3(256), BYTES, st, d);
}

bool respair_f32w_supported(const RespairF32Args& a) {
    return (a.C == 32 || a.C == 64) && (a.k == 3 || a.k == 7 || a.k == 11) && a.dil >= 1 && a.dil <= 8 && (a.k - 1) * a.dil <= 60 && a.T % 4 == 0 &&
           aligned16(a.x) && aligned16(a.out) && aligned16(a.w1) && aligned16(a.w2);
}

int respair_f32w_run(int C, int dil) { return C == 32 ? PairWGeo<4, 32>::run(dil) : PairWGeo<2, 64>::run(dil); }
// a.w1 / a.w2 are the minimal-filtering pseudo-tap weights of the two convolutions ([P][C][C], pack.py:pack_conv_mf)
int launch_respair_f32w(const RespairF32Args& a, hipStream_t st) {
    if (!respair_f32w_supported(a)) VB_FAIL(VB_E_INVALID, "respair_f32w: C=%d k=%d dil=%d T=%d (C 32 / 64, k 3/7/11, (k-1) dil <= 60, T %% 4 == 0, 16-B aligned)", a.C, a.k, a.dil, a.T);
    // runs of M = 8 VW (C = 32) / 4 VW (C = 64) intermediate positions; executed flops: pseudo-taps / 2 products per output, two convolutions
    PairLaunchT<PairF32Dev> L{};
    VB_TRY(pair_fill_common(a, "respair_f32w", respair_f32w_run(a.C, a.dil), 0.5 * mf_ntaps(a.k), L));      // respair_dev.h
    const PairF32Dev& d = L.d;
    ProfScope prof(3, L.flops, L.act_bytes + 2.0 * 4.0 * mf_ntaps(a.k) * a.C * a.C, st);
    if (a.C == 32) {
        if (a.k == 3) launch_pair_w<3, 2, 32>(d, L.grid, st);
        else if (a.k == 7) launch_pair_w<7, 4, 32>(d, L.grid, st);
        else launch_pair_w<11, 4, 32>(d, L.grid, st);
    } else {
        if (a.k == 3) launch_pair_w<3, 2, 64>(d, L.grid, st);
        else if (a.k == 7) launch_pair_w<7, 2, 64>(d, L.grid, st);
        else launch_pair_w<11, 2, 64>(d, L.grid, st);
    }
    VB_CHECK_LAUNCH();
    return VB_OK;
}
