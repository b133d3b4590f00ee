// The activation-window feed of the fp32 LDS-DMA ring kernels (conv1d_f32g / conv1d_f32w / respair_f32 / respair_f32w), defined once:
// which global quads a lane fetches, the DMA that brings a 16-channel chunk into a window stage, and the in-place pass over what landed.
//
// A window stage is [16 ci][NP * 64 positions] floats and starts at position start_al of the clip.  The four waves share a chunk's pieces,
// XPW per wave; piece ii = wave * XPW + i of the
//   16-byte form  is 1 KB = four rows of 64 positions: lane -> quad q = ii * 4 + (lane >> 4), row ci = q / NP, positions
//                 (q - ci * NP) * 64 + (lane & 15) * 4 .. + 3 (rows and start_al are 16-byte aligned, T_in % 4 == 0: a quad never straddles a clip end);
//   UPS form      (conv1d_f32g_kernel's nearest-neighbour upsampled input, T_eff = 2 T_in) is 256 B = one row of 64 positions, a lane
//                 fetches position idx of the upsampled row from idx >> 1 as 4 bytes.
// Positions outside [0, T_eff) are fetched from the row's start (any valid address) and remembered in the lane's bit mask xoob.
//
// fix(): once per chunk, by the lanes that DMA'd the quads, after the wave's own DMA has landed (the caller's counted vmcnt wait) and in
// front of the barrier that publishes the chunk: zeros over the out-of-range quads (padding) and LeakyReLU IN PLACE - not on the B fragments
// inside the MFMA loop: v_mul + 2 v_max per fragment were 6 VALU instructions per 4 MFMAs, and VALU instructions issued between a SIMD's
// MFMAs cost matrix-pipe time (tools/probe/f32_loop_probe: 149 -> 136 TF/s with them; here 36 VALU + 6 LDS instructions per thread and
// chunk replace 48 per tap).  Same operation on the same values: bit-identical.  The LDS accesses come from inline asm: an ordinary one
// makes hipcc drain the DMA ring with vmcnt(0) in front of it (lds_asm.h); the wave has waited for exactly these pieces itself.  The caller
// waits LDS_WAIT(0) behind fix() before its barrier.
#pragma once
#include "dma_ring.h"
#include "lds_asm.h"

template <int XPW, int NP, bool UPS = false>
struct RingWindow {
    int wave, lane;
    int xsrc[XPW];           // piece i: this lane's source offset inside the clip's chunk 0
    unsigned xoob;           // bit i: piece i of this lane lies outside [0, T_eff)

    __device__ __forceinline__ void setup(int wave_, int lane_, int start_al, int T_in) {
        wave = wave_; lane = lane_; xoob = 0;
        const int T_eff = UPS ? 2 * T_in : T_in;
#pragma unroll
        for (int i = 0; i < XPW; ++i) {
            const int ii = wave * XPW + i;
            int ci, pos;
            if constexpr (UPS) { ci = ii / NP; pos = (ii - ci * NP) * 64 + lane; }
            else { const int q = ii * 4 + (lane >> 4); ci = q / NP; pos = (q - ci * NP) * 64 + (lane & 15) * 4; }
            const int idx = start_al + pos;
            const bool ok = idx >= 0 && idx < T_eff;
            xsrc[i] = ci * T_in + (ok ? (UPS ? (idx >> 1) : idx) : 0);
            xoob |= ok ? 0u : (1u << i);
        }
    }
    // chunk (src = its first row in the clip) -> window stage dst.  nt (experiments build only, VB_CONV_XNT=1): the window - read by one or
    // two workgroups - with the non-temporal policy, so that it does not displace the weights every workgroup re-reads from L2 (A/B of
    // round 5, profiles/r05_conv_window_nt.txt)
    __device__ __forceinline__ void issue(const float* src, float* dst, [[maybe_unused]] bool nt = false) const {
#pragma unroll
        for (int i = 0; i < XPW; ++i) {
            const int ii = wave * XPW + i;
#ifdef VB_EXPERIMENTS
            if (nt) {
                if constexpr (UPS) __builtin_amdgcn_global_load_lds((glb_ptr_t)(src + xsrc[i]), (lds_ptr_t)(dst + ii * 64), 4, 0, 2);
                else __builtin_amdgcn_global_load_lds((glb_ptr_t)(src + xsrc[i]), (lds_ptr_t)(dst + ii * 256), 16, 0, 2);
                continue;
            }
#endif
            if constexpr (UPS) __builtin_amdgcn_global_load_lds((glb_ptr_t)(src + xsrc[i]), (lds_ptr_t)(dst + ii * 64), 4, 0, 0);
            else __builtin_amdgcn_global_load_lds((glb_ptr_t)(src + xsrc[i]), (lds_ptr_t)(dst + ii * 256), 16, 0, 0);
        }
    }
    // the in-place pass over this lane's own quads of a landed stage (see the head of the file).  act: a bool decides at run time, and a
    // launch without activation only writes zeros over out-of-range quads; std::true_type (the fused pairs, which always activate) leaves
    // no branch behind
    template <class Act>
    __device__ __forceinline__ void fix(const float* stage, Act act, float slope) const {
        if constexpr (UPS) {
            const unsigned a0 = lds_u32(stage + wave * XPW * 64 + lane);
            float v[XPW];
            if (act) {
                static_for<0, XPW>([&](auto ic) { constexpr int I = decltype(ic)::value; lds_rd32<I * 256>(v[I], a0); });
                LDS_WAIT(0);
            }
            static_for<0, XPW>([&](auto ic) {
                constexpr int I = decltype(ic)::value;
                const bool oob = (xoob >> I) & 1;
                if (act) { lds_pin(v[I]); lds_wr32<I * 256>(a0, oob ? 0.f : fmaxf(v[I], v[I] * slope)); }
                else if (oob) lds_wr32<I * 256>(a0, 0.f);
            });
        } else {
            const unsigned a0 = lds_u32(stage + wave * XPW * 256 + lane * 4);
            lds_u32x4 v[XPW];
            const lds_u32x4 zero = {0u, 0u, 0u, 0u};
            if (act) {
                static_for<0, XPW>([&](auto ic) { constexpr int I = decltype(ic)::value; lds_rd128<I * 1024>(v[I], a0); });
                LDS_WAIT(0);
            }
            static_for<0, XPW>([&](auto ic) {
                constexpr int I = decltype(ic)::value;
                const bool oob = (xoob >> I) & 1;
                if (act) { lds_pin(v[I]); lds_wr128<I * 1024>(a0, oob ? zero : lds_lrelu128_apply(v[I], slope)); }
                else if (oob) lds_wr128<I * 1024>(a0, zero);
            });
        }
    }
};
