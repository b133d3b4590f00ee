// What the register-staged implicit-GEMM kernels share (conv1d_f32.hip, conv1d_x3.hip, conv1d_bf16.hip; the fused pairs take the halo limit
// and the rounding step through respair_dev.h), once: the tile geometry, the two-half window staging, the bf16-MFMA kernels' weight tile
// staging and, host side, the tile table.  conv1d_f32_kernel stages its own window (its GroupNorm form rounds differently) and so does
// conv1d_x3_kernel (StagedWindow<2, 8, ..> is its staging; through the helper it spills more SGPRs and one tile runs 6 % slower).
#pragma once
#include <type_traits>

#include "conv1d_dev.h"

constexpr int CONV_HALO = 64;      // max (taps - 1) * dil of every register-staged kernel: conv1d_fill checks it, the pair launchers too

// ---- geometry --------------------------------------------------------------
// One polyphase sub-convolution (phases == 1: in_off = -pad, out index = n): output n of phase ph is out[out_off + n * out_stride] and reads
// the input from n + in_off on; n_count outputs.  (conv1d_f32g_kernel calls this with its own XCD numbering.)
struct ConvPhase { int in_off, out_off, out_stride, n_count; };
__device__ __forceinline__ ConvPhase conv_phase(const ConvDev& p, int ph) {
    if (p.phases == 1) return {-p.pad, 0, 1, p.T_out};
    const int u = p.phases;
    const int d = p.tr_pad - ph;
    const int q0 = d > 0 ? (d + u - 1) / u : 0;
    const int out_off = q0 * u + ph - p.tr_pad;
    return {q0 - (p.ntaps - 1), out_off, u, (p.T_out - out_off + u - 1) / u};
}
// A workgroup's tile (grid: time tiles x channel tiles x (clip, phase)): xw_used window positions of T_eff (after upsample2 / in_stride)
// input positions, read from clip xb (x_bmod folds clips) at xbase.
struct ConvTile : ConvPhase {
    int b, ph, n0, co0, xw_used, T_eff, xb;
    const float* xbase;
};
// false: the tile lies behind the phase's last output (the workgroup returns)
__device__ __forceinline__ bool conv_tile(const ConvDev& p, int t_tile, int co_tile, ConvTile& g) {
    const int z = blockIdx.z;
    g.b = z / p.phases; g.ph = z - g.b * p.phases;
    g.n0 = blockIdx.x * t_tile;
    g.co0 = blockIdx.y * co_tile;
    static_cast<ConvPhase&>(g) = conv_phase(p, g.ph);
    if (g.n0 >= g.n_count) return false;
    g.xw_used = t_tile + (p.ntaps - 1) * p.dil;
    g.T_eff = p.upsample2 ? 2 * p.T_in : (p.T_in - p.in_phase + p.in_stride - 1) / p.in_stride;
    if (p.row_len) g.T_eff = p.row_len[g.b] * p.len_mul;        // row lengths: the one bound of the window's zero padding
    g.xb = p.x_bmod > 0 ? (g.b % p.x_bmod) : g.b;
    g.xbase = p.x + (int64_t)g.xb * p.x_bstride;
    return true;
}
template <int TM, int TN>
__device__ __forceinline__ void conv_zero_acc(f32x16 (&acc)[TM][TN]) {
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
}

// ---- activation window -----------------------------------------------------
// The fused input transform of one value: LeakyReLU, or the GroupNorm affine folded to t * nsc + nsh (+ swish)
__device__ __forceinline__ float conv_in_act(const ConvDev& p, float t, float nsc, float nsh) {
    if (p.in_act == ACT_LRELU) {
        t = t > 0.f ? t : t * p.in_slope;
    } else if (p.in_act == ACT_GN_SWISH || p.in_act == ACT_GN) {
        t = t * nsc + nsh;
        if (p.in_act == ACT_GN_SWISH) t = t / (1.f + __expf(-t));
    }
    return t;
}
// N (4 / 8) consecutive channels of one position -> bf16, one N*2-byte store per plane: plane 0 the round-to-nearest value and, NPL == 2,
// plane 1 (`plane` elements on) its rounding residual.  Every operand of the split-bf16 / bf16 conv kernels and pairs is rounded here.
template <int NPL, int N>
__device__ __forceinline__ void bf16_planes_store(const float (&v)[N], bf16_t* dst, int plane) {
    typedef __bf16 vec_t __attribute__((ext_vector_type(N)));
    vec_t hi, lo;
#pragma unroll
    for (int e = 0; e < N; ++e) {
        hi[e] = f2bf(v[e]);
        if constexpr (NPL == 2) lo[e] = f2bf(v[e] - bf2f(hi[e]));
    }
    *reinterpret_cast<vec_t*>(dst) = hi;
    if constexpr (NPL == 2) *reinterpret_cast<vec_t*>(dst + plane) = lo;
}
// Window staging in two halves (async-STAGE): load() issues ALL global loads of a chunk into registers (raw values + the per-channel affine
// of the fused norm), store() later applies the pointwise transform, rounds (NPL == 2: splits to hi / lo) and writes the transposed image
// xT[plane][t][ci] (XW rows of PITCH bf16).  The loads of chunk ch+1 are in flight while the taps of chunk ch are multiplied.  A wave owns
// CPW CONSECUTIVE channels of the 4 * CPW-channel chunk and a lane one window position per pass: the global loads stay coalesced along t
// (one channel row per instruction) and the transposed image takes one 16-byte LDS write per plane, position and channel octet.
template <int NPL, int CPW, int XW, int PITCH>
struct StagedWindow {
    static constexpr int NIT = XW / 64;
    int lane, wave, cpg;
    float raw[CPW][NIT];
    float nsc[CPW], nsh[CPW];

    __device__ __forceinline__ void setup(const ConvDev& p, int wave_, int lane_) {
        lane = lane_; wave = wave_;
        cpg = p.gn_groups > 0 ? (p.Ci / p.gn_groups) : 1;
    }
    __device__ __forceinline__ void load(const ConvDev& p, const ConvTile& g, int c0) {
#pragma unroll
        for (int e = 0; e < CPW; ++e) {
            const int ci = c0 + CPW * wave + e;
            const bool cok = ci < p.Ci;
            nsc[e] = 1.f; nsh[e] = 0.f;
            if (cok && (p.in_act == ACT_GN_SWISH || p.in_act == ACT_GN)) {
                const int grp = ci / cpg;
                const float rs = p.gn_rstd[g.b * p.gn_groups + grp] * p.gn_gamma[ci];
                nsc[e] = rs;
                nsh[e] = p.gn_beta[ci] - p.gn_mean[g.b * p.gn_groups + grp] * rs;
            }
            const float* xrow = g.xbase + (int64_t)(cok ? ci : 0) * p.T_in;
#pragma unroll
            for (int it = 0; it < NIT; ++it) {
                const int idx = g.n0 + g.in_off + lane + 64 * it;
                const bool ok = cok && (lane + 64 * it) < g.xw_used && idx >= 0 && idx < g.T_eff;
                raw[e][it] = ok ? xrow[p.upsample2 ? (idx >> 1) : idx * p.in_stride + p.in_phase] : 0.f;
            }
        }
    }
    __device__ __forceinline__ void store(const ConvDev& p, const ConvTile& g, int c0, bf16_t* xT) {
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int wpos = lane + 64 * it;
            if (wpos >= g.xw_used) continue;
            const int idx = g.n0 + g.in_off + wpos;
            const bool inr = idx >= 0 && idx < g.T_eff;
#pragma unroll
            for (int h = 0; h < CPW / 8; ++h) {
                float v[8];
#pragma unroll
                for (int e8 = 0; e8 < 8; ++e8) {
                    const int e = 8 * h + e8;
                    float t = raw[e][it];
                    if (inr && (c0 + CPW * wave + e) < p.Ci) t = conv_in_act(p, t, nsc[e], nsh[e]);
                    else t = 0.f;                            // zero padding stays zero: the conv pads the ACTIVATED tensor
                    v[e8] = t;
                }
                bf16_planes_store<NPL>(v, xT + wpos * PITCH + CPW * wave + 8 * h, XW * PITCH);
            }
        }
    }
};

// ---- weight tile -----------------------------------------------------------
// One (tap, chunk) of the packed weights [plane][tap][Co][Ci_pad]: ROWS output channels x DEPTH input channels x NPL planes, as 16-byte pieces
// through registers (load() early, store() behind the MFMAs that read the other buffer) into wl[plane][co][PITCH].  Rows past Co are zero
// and, where a chunk can overrun the padded row (GUARD_CI: chunks deeper than the 32-channel pad), so are channels past Ci_pad.
template <int NPL, int DEPTH, int PITCH, int ROWS, bool GUARD_CI>
struct StagedWeights {
    static constexpr int PPR = DEPTH / 8;                       // pieces per row
    static constexpr int WPT = ROWS * PPR * NPL / 256;       // pieces per thread
    uint4 wreg[WPT];

    __device__ __forceinline__ void load(const ConvDev& p, const bf16_t* wbase, int co0, int c0, int j) {
#pragma unroll
        for (int i = 0; i < WPT; ++i) {
            const int id = threadIdx.x + i * 256;
            const int pl = NPL == 1 ? 0 : id / (ROWS * PPR), rem = id - pl * (ROWS * PPR);
            const int cog = co0 + rem / PPR, ci = c0 + (rem % PPR) * 8;
            bool ok = cog < p.Co;
            if constexpr (GUARD_CI) ok = ok && ci < p.Ci_pad;
            wreg[i] = ok ? *reinterpret_cast<const uint4*>(wbase + pl * p.wp_plane + ((int64_t)j * p.Co + cog) * p.Ci_pad + ci) : make_uint4(0, 0, 0, 0);
        }
    }
    __device__ __forceinline__ void store(bf16_t* wl) const {
#pragma unroll
        for (int i = 0; i < WPT; ++i) {
            const int id = threadIdx.x + i * 256;
            const int pl = NPL == 1 ? 0 : id / (ROWS * PPR), rem = id - pl * (ROWS * PPR);
            *reinterpret_cast<uint4*>(&wl[pl * (ROWS * PITCH) + (rem / PPR) * PITCH + (rem % PPR) * 8]) = wreg[i];
        }
    }
};

// ---- host side: the tile table ----------------------------------------------
// 128co x 128t, or 128co x 64t when the grid of 128co x 256t-sized granules fills under 70 % of its last round of 256 workgroups (every VAE
// level at B = 8 makes 288: two rounds at 56 % - the smaller tile halves the granule); 64co x 128t and 32co x 256t for the narrow layers.
static inline ConvTileId conv_staged_tile(int Co, int n_count, int B, int phases) {
    if (Co <= 32) return CONV_TILE_32x256;
    if (Co <= 64) return CONV_TILE_64x128;
    const int64_t blocks = (int64_t)cdiv(n_count, 256) * cdiv(Co, 128) * B * phases;
    const double eff = (double)blocks / (double)(cdiv(blocks, 256) * 256);
    return eff < 0.7 ? CONV_TILE_128x64 : CONV_TILE_128x128;
}
// f(WM, WN, TM, TN) with the tile's wave grid and register tile as std::integral_constants
template <class F>
static inline void conv_tile_dispatch(ConvTileId tile, F&& f) {
    using one = std::integral_constant<int, 1>; using two = std::integral_constant<int, 2>; using four = std::integral_constant<int, 4>;
    switch (tile) {
        case CONV_TILE_128x128: f(two(), two(), two(), two()); break;
        case CONV_TILE_128x64: f(two(), two(), two(), one()); break;
        case CONV_TILE_64x128: f(two(), two(), one(), two()); break;
        case CONV_TILE_32x256: f(one(), four(), one(), two()); break;
    }
}
