// What the kernels that DMA their tiles into LDS rings (global_load_lds + counted vmcnt) share: the compile-time loop, the counted waits,
// the pointer types of the DMA builtin and the fused pairs' outputs per workgroup and output element.  No inline assembly (that is lds_asm.h); the fp32 conv
// kernels' window feed and fragment pipeline, which need both, are ring_window.h and ring_step.h.
#pragma once
#include <type_traits>

// f(integral_constant<int, i>) for i in [I, N): the index is a constant expression in the body (wait counts, LDS offsets, template arguments)
template <int I, int N, class F> __device__ __forceinline__ void static_for(F&& f) {
    if constexpr (I < N) { f(std::integral_constant<int, I>{}); static_for<I + 1, N>(f); }
}

// operands of __builtin_amdgcn_global_load_lds
typedef __attribute__((address_space(3))) void* lds_ptr_t;
typedef const __attribute__((address_space(1))) void* glb_ptr_t;

// at most N of this wave's younger vector-memory operations (DMA pieces included) may still be in flight
template <int N> __device__ __forceinline__ void wait_vmcnt() {
    static_assert(N >= 0 && N < 64, "vmcnt is 6 bits");
    // s_waitcnt simm16 (gfx9): vmcnt[3:0] | expcnt[6:4] | lgkmcnt[11:8] | vmcnt_hi[15:14]; only vmcnt is counted here
    __builtin_amdgcn_s_waitcnt(0x0f70 | (N & 15) | ((N >> 4) << 14));
}
// counted wait in front of ring step t: `ahead` (<= 2) younger weight tiles of WPW pieces per wave (+ one window chunk of XPW when xin) may fly
template <int WPW, int XPW> __device__ __forceinline__ void wait_tile(int ahead, bool xin) {
    if (xin) {
        if (ahead >= 2) wait_vmcnt<2 * WPW + XPW>();
        else if (ahead == 1) wait_vmcnt<WPW + XPW>();
        else wait_vmcnt<XPW>();
    } else {
        if (ahead >= 2) wait_vmcnt<2 * WPW>();
        else if (ahead == 1) wait_vmcnt<WPW>();
        else wait_vmcnt<0>();
    }
}

// Outputs per workgroup of the fused ResBlock pairs (all four: respair_x3 / respair_bf16 / respair_f32 / respair_f32w): a run of `run`
// intermediate positions less conv2's halo, a multiple of 4 (the epilogue moves 16-byte quads).  Kernel and launcher (the grid) both call it.
__host__ __device__ constexpr int pair_run_outputs(int run, int k) { return (run - (k - 1)) & ~3; }

// One output element of the fused ResBlock pairs (respair_x3 / respair_f32 / respair_f32w): conv_out_value (conv1d_dev.h) with acc_scale = 1
// and no output activation - the same pinned arithmetic, so that a pair and the two unfused launches round alike.
__device__ __forceinline__ float pair_out_value(float alpha, float beta, float acc, float bias, float res, float old) {
#pragma clang fp contract(off)
    float val = acc + bias;
    val = val + res;
    return fmaf(val, alpha, beta * old);
}
