// The fragment pipeline of one ring step of the fp32 LDS-DMA ring kernels (conv1d_f32g / conv1d_f32w / respair_f32 / respair_f32w), defined
// once, beside their window feed (ring_window.h).  Each kernel keeps its own schedule - which tile is requested where, every counted vmcnt
// wait and barrier - and its own weight-tile DMA: the shared forms of that DMA cost instances spills or VALU address arithmetic between the
// MFMAs (docs/history.md, "fp32 ring kernels: one fragment pipeline").
#pragma once
#include "dma_ring.h"
#include "lds_asm.h"

// ---- fragment pipeline of one ring step: NM channel pairs, each NA A fragments (weights) and nb(m) B reads (window / intermediate; one, or
// the two an F(2,3) operand is formed from, mf_taps.h).  Fragments come by inline-asm ds_read_b32 with exact lgkmcnt waits (lds_asm.h: with
// LDS-DMA in flight hipcc only ever waits lgkmcnt(0), which exposed one LDS round trip per two pairs) and are requested TWO pairs ahead of
// their multiplication into THREE rotating register sets, so that a request never lands in registers an MFMA in flight still reads: in front
// of pair m exactly the reads of pair m + 1 may still fly.
//   nb(mc)              -> integral_constant: B reads of pair m (<= NBX)
//   read_a(mc, ic, dst), read_b(mc, jc, dst): one lds_rd32 with the caller's compile-time offset
//   first()             what is queued behind the first two requests (the convolutions: the previous step's held-back pair)
//   mul(mc, a, b)       pair m's multiplications from a[NA], b[nb] - or, for a step's last pair, holding them back for the next step
// NOREAD (experiments build, timing only): no reads, lane-derived operands.
template <int NM, int NA, int NBX, bool NOREAD = false, class NB, class RdA, class RdB, class First, class Mul>
__device__ __forceinline__ void ring_step_pairs(NB nb, RdA read_a, RdB read_b, First first, Mul mul) {
    float a[3][NA], b[3][NBX];
    if constexpr (NOREAD) {
        const int lane = threadIdx.x & 63;
#pragma unroll
        for (int s3 = 0; s3 < 3; ++s3) {
#pragma unroll
            for (int i = 0; i < NA; ++i) a[s3][i] = (float)lane;
#pragma unroll
            for (int j = 0; j < NBX; ++j) b[s3][j] = (float)(lane + s3);
        }
    }
    auto request = [&](auto mc) {
        constexpr int S = decltype(mc)::value % 3;
        if constexpr (NOREAD) return;
        static_for<0, NA>([&](auto ic) { read_a(mc, ic, a[S][decltype(ic)::value]); });
        static_for<0, decltype(nb(mc))::value>([&](auto jc) { read_b(mc, jc, b[S][decltype(jc)::value]); });
    };
    request(std::integral_constant<int, 0>{});
    request(std::integral_constant<int, 1>{});
    first();
    static_for<0, NM>([&](auto mc) {
        constexpr int M = decltype(mc)::value, S = M % 3;
        if constexpr (M + 1 < NM) LDS_WAIT(NA + decltype(nb(std::integral_constant<int, M + 1>{}))::value); else LDS_WAIT(0);
#pragma unroll
        for (int i = 0; i < NA; ++i) lds_pin(a[S][i]);
        static_for<0, decltype(nb(mc))::value>([&](auto jc) { lds_pin(b[S][decltype(jc)::value]); });
        if constexpr (M + 2 < NM) request(std::integral_constant<int, M + 2>{});
        mul(mc, a[S], b[S]);
    });
}
