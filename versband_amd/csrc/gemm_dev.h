// What the bf16 GEMM kernels share (gemm_bf16.hip, band_ffn.hip, gemm_bf16_pk.hip): device-side descriptor, P16 column layout, epilogues.
// The main loops' shared pieces (tile walk, LDS tile image, DMA feed, MFMA step) are in gemm_tile.h.
#pragma once
#include <stdlib.h>
#include <string.h>
#include <type_traits>

#include "kernels.h"
#include "dma_ring.h"

#define BM 128
#define BN 128
#define BK 64
#define NTHREADS 256

struct GemmDev {
    const bf16_t* A; int64_t a_plane; int lda; const int* a_rows; int a_koff_group;
    const bf16_t* B; int64_t b_plane; int ldb; int64_t b_group_stride;
    int M, N, K, nseg, ngroups; const int* group_off; int c_noff_group;
    const float* bias; int64_t bias_group_stride;
    bf16_t* out; int64_t out_plane; int out_np; int ldc;
    float* out32; int ldc32;
    const float* gate; int gate_ld; int T;
    const int* rows_out; const float* row_scale; const float* y32_in; int n_tiles;
    const float* row_scale2; int scale_split;
    int grp_rows, grp_tiles, grp_xcd;   // uniform groups (per-clip operands): rows per group, row tiles per group (0 = off); XCD-affine tile order
    const float* add32; int dup_rows;   // EPI_F32: + add32[m][n]; second copy of the row at m + dup_rows
    int conv_ci, conv_ktap, conv_dil, conv_agrp, conv_arow0; int64_t conv_btap; const float* res32;   // conv-as-GEMM mode (EPI_F32_CT), see GemmArgs
    int ncc, rpx;                   // 128x128 kernel, wide N: column tiles are visited in chunks of ncc (0 = off) over the rpx row tiles of an XCD
    bf16_t* q; int64_t q_plane; bf16_t* k; int64_t k_plane; bf16_t* vt; int64_t vt_plane; int qkv_np;
    const float* rope_cos; const float* rope_sin; int H, hd, Tpad, D;
    float rT, rhd, rD;              // reciprocals for fdiv(): the epilogues decompose row -> (clip, t) and column -> (head, d)
    int no_vt16;                    // QKV P16: keep the V third on the row-per-lane layout (VB_QKV_VT16_OFF: bit-identity switch)
    int epi_old;                    // gated-residual staged epilogue: request the residual after the staging, as rounds 1-3a did (VB_BAND_EPI_OLD)
    unsigned long long* trace;      // tuning only (vbdbg_gemm_trace): per block {t_start, t_loop_end, t_end, hw ids}
    int abl;                        // tuning only (VB_GEMM_ABLATE): 6 = QKV without the V^T stores, 7 = without the q/k stores, 8 = without the RoPE table loads
};

// x / d for 0 <= x < 2^21 without the ~40-instruction integer division: (x + 0.5) / d is at least 0.5/d away
// from every integer, far more than the fp32 rounding of the product.  rinv = 1.0f / d.
__device__ __forceinline__ int fdiv(int x, float rinv) { return (int)(((float)x + 0.5f) * rinv); }

__device__ __forceinline__ void store4p(bf16_t* base, int64_t plane, int np, int64_t idx, const float v[4]) {
    bf16x4 hi;
#pragma unroll
    for (int i = 0; i < 4; ++i) hi[i] = f2bf(v[i]);
    *reinterpret_cast<bf16x4*>(base + idx) = hi;
    if (np == 2) {
        bf16x4 lo;
#pragma unroll
        for (int i = 0; i < 4; ++i) lo[i] = f2bf(v[i] - bf2f(hi[i]));
        *reinterpret_cast<bf16x4*>(base + plane + idx) = lo;
    }
}
__device__ __forceinline__ void store1p(bf16_t* base, int64_t plane, int np, int64_t idx, float v) {
    bf16_t hi = f2bf(v);
    base[idx] = hi;
    if (np == 2) base[plane + idx] = f2bf(v - bf2f(hi));
}

// "P16" column layout: the MFMA accumulator of a 32 x 32 tile gives lane (row, fk) the columns q*8 + fk*4 + e (four separate quads).  When
// LDS row c' of the weight tile is filled with weight row pi(c') = ((c'>>2)&1)*16 + (c'>>3)*4 + (c'&3) instead of c' (a permutation of
// the SOURCE rows of the tile DMA: nothing else moves, the fragment reads stay conflict-free), the same accumulator holds the 16
// CONSECUTIVE output columns fk*16 .. fk*16+15 of the lane's row: bf16 results leave as 16-byte stores (two per tile instead of four
// 8-byte ones), RoPE table entries arrive as 16-byte loads, and every row gets 64 contiguous bytes per tile.  Same values, same
// arithmetic - only which lane holds what.
__device__ __forceinline__ int p16_src_row(int r) { const int c = r & 31; return (r & ~31) + ((c >> 2) & 1) * 16 + (c >> 3) * 4 + (c & 3); }
__device__ __forceinline__ void store8p(bf16_t* base, int64_t plane, int np, int64_t idx, const float v[8]) {
    bf16x8 hi;
#pragma unroll
    for (int i = 0; i < 8; ++i) hi[i] = f2bf(v[i]);
    *reinterpret_cast<bf16x8*>(base + idx) = hi;
    if (np == 2) {
        bf16x8 lo;
#pragma unroll
        for (int i = 0; i < 8; ++i) lo[i] = f2bf(v[i] - bf2f(hi[i]));
        *reinterpret_cast<bf16x8*>(base + plane + idx) = lo;
    }
}
// QKV + RoPE epilogue of one wave in the P16 layout (same arithmetic as epi_store<EPI_QKV_ROPE>, element for element)
template <int TM, int TN>
__device__ __forceinline__ void wave_epilogue_qkv_p16(const struct GemmDev& p, f32x16 (&acc)[TM][TN], int row_base, int rows_end, int n_base,
                                                      int frow, int fk);

// Epilogue in two halves.  epi_load<EPI>() issues every global LOAD an output quad needs (bias, residual + gate,
// RoPE table entries, partial expert sum); epi_store<EPI>() does the math and the stores.  The kernels call epi_load
// for all quads of a 32-row slab first and only then epi_store: vmcnt retires loads and stores in order, so a load
// issued behind a store also waits for that store's round trip - interleaved they serialise one memory round trip per
// quad (measured 1.4x on the residual GEMMs).
struct EpiPre { float4 a, b; };

template <int EPI>
__device__ __forceinline__ void epi_load(const GemmDev& p, int g, int m, int tok, int n, EpiPre& e) {
    e.a = make_float4(0.f, 0.f, 0.f, 0.f); e.b = e.a;
    if constexpr (EPI == EPI_PLANES || EPI == EPI_F32 || EPI == EPI_GELU_PLANES || EPI == EPI_HEADS_T || EPI == EPI_F32_CT) {
        if (p.bias) e.a = *reinterpret_cast<const float4*>(p.bias + g * p.bias_group_stride + n);
        if constexpr (EPI == EPI_F32) {
            if (p.add32) e.b = *reinterpret_cast<const float4*>(p.add32 + (int64_t)m * p.ldc32 + g * p.c_noff_group + n);
        }
        if constexpr (EPI == EPI_F32_CT) {
            if (p.res32) {
                const int b = fdiv(m, p.rT), t = m - b * p.T;
                const float* rp = p.res32 + ((int64_t)b * p.N + n) * p.T + t;
                e.b = make_float4(rp[0], rp[p.T], rp[2 * (int64_t)p.T], rp[3 * (int64_t)p.T]);
            }
        }
    } else if constexpr (EPI == EPI_RESID_GATE) {
        const int col = g * p.c_noff_group + n;
        e.a = *reinterpret_cast<const float4*>(p.out32 + (int64_t)m * p.ldc32 + col);
        e.b = *reinterpret_cast<const float4*>(p.gate + (int64_t)fdiv(m, p.rT) * p.gate_ld + col);
    } else if constexpr (EPI == EPI_SCATTER_ADD_PLANES) {
        e.a = *reinterpret_cast<const float4*>(p.y32_in + (int64_t)tok * p.ldc32 + n);
    } else if constexpr (EPI == EPI_QKV_ROPE) {
        if (n < 2 * p.D && p.abl != 8) {
            const int nn = n - fdiv(n, p.rD) * p.D, t = m - fdiv(m, p.rT) * p.T;
            const int jd = (nn - fdiv(nn, p.rhd) * p.hd) >> 1;
            const float2 cs = *reinterpret_cast<const float2*>(p.rope_cos + (int64_t)t * (p.hd / 2) + jd);
            const float2 sn = *reinterpret_cast<const float2*>(p.rope_sin + (int64_t)t * (p.hd / 2) + jd);
            e.a = make_float4(cs.x, cs.y, sn.x, sn.y);
        }
    }
}

template <int EPI>
__device__ __forceinline__ void epi_store(const GemmDev& p, int g, int m, int tok, float scale, int n, float v[4], const EpiPre& e) {
    // m: global row (slot) index, n: column within the group's [0,N), 4 consecutive columns, all < N
    // The arithmetic is pinned (no implicit contraction, explicit fmaf): the launcher picks the tile configuration from the
    // problem size, and a clip's result must not depend on the batch it rides in - every kernel variant has to round alike.
#pragma clang fp contract(off)
    if constexpr (EPI == EPI_PLANES || EPI == EPI_F32 || EPI == EPI_GELU_PLANES || EPI == EPI_HEADS_T || EPI == EPI_F32_CT) {
        v[0] += e.a.x; v[1] += e.a.y; v[2] += e.a.z; v[3] += e.a.w;
    }
    if constexpr (EPI == EPI_PLANES) {
        store4p(p.out, p.out_plane, p.out_np, (int64_t)m * p.ldc + g * p.c_noff_group + n, v);
    } else if constexpr (EPI == EPI_GELU_PLANES) {
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = 0.5f * v[i] * (1.0f + erff(v[i] * 0.70710678118654752440f));
        store4p(p.out, p.out_plane, p.out_np, (int64_t)m * p.ldc + g * p.c_noff_group + n, v);
    } else if constexpr (EPI == EPI_F32) {
        if (p.add32) { v[0] += e.b.x; v[1] += e.b.y; v[2] += e.b.z; v[3] += e.b.w; }
        *reinterpret_cast<float4*>(p.out32 + (int64_t)m * p.ldc32 + g * p.c_noff_group + n) = make_float4(v[0], v[1], v[2], v[3]);
        if (p.dup_rows > 0) *reinterpret_cast<float4*>(p.out32 + (int64_t)(m + p.dup_rows) * p.ldc32 + g * p.c_noff_group + n) = make_float4(v[0], v[1], v[2], v[3]);
    } else if constexpr (EPI == EPI_F32_CT) {
        const int b = fdiv(m, p.rT), t = m - b * p.T;
        if (p.res32) { v[0] += e.b.x; v[1] += e.b.y; v[2] += e.b.z; v[3] += e.b.w; }
#pragma unroll
        for (int i = 0; i < 4; ++i) p.out32[((int64_t)b * p.N + n + i) * p.T + t] = v[i];
    } else if constexpr (EPI == EPI_RESID_GATE) {
        const int col = g * p.c_noff_group + n;
        float4 h;
        h.x = fmaf(e.b.x, v[0], e.a.x); h.y = fmaf(e.b.y, v[1], e.a.y); h.z = fmaf(e.b.z, v[2], e.a.z); h.w = fmaf(e.b.w, v[3], e.a.w);
        *reinterpret_cast<float4*>(p.out32 + (int64_t)m * p.ldc32 + col) = h;
    } else if constexpr (EPI == EPI_SWIGLU) {
        float o0 = silu_f(v[0]) * v[1], o1 = silu_f(v[2]) * v[3];
        if (p.row_scale2) { o0 *= scale; o1 *= scale; }      // routed gate weight folded into the hidden row (same two roundings as the P16 path)
        int64_t idx = (int64_t)m * p.ldc + g * p.c_noff_group + (n >> 1);
        bf16_t h0 = f2bf(o0), h1 = f2bf(o1);
        typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
        bf16x2 hv; hv[0] = h0; hv[1] = h1;
        *reinterpret_cast<bf16x2*>(p.out + idx) = hv;
        if (p.out_np == 2) {
            bf16x2 lv; lv[0] = f2bf(o0 - bf2f(h0)); lv[1] = f2bf(o1 - bf2f(h1));
            *reinterpret_cast<bf16x2*>(p.out + p.out_plane + idx) = lv;
        }
    } else if constexpr (EPI == EPI_GEGLU) {
        // T5DenseGatedActDense: gelu_new(wi_0 x) * (wi_1 x), NewGELUActivation = 0.5 x (1 + tanh(sqrt(2/pi) (x + 0.044715 x^3)))
        float o[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const float x = v[2 * i];
            const float inner = 0.7978845608028654f * (x + 0.044715f * (x * x * x));
            o[i] = (0.5f * x * (1.0f + tanhf(inner))) * v[2 * i + 1];
        }
        int64_t idx = (int64_t)m * p.ldc + g * p.c_noff_group + (n >> 1);
        bf16_t h0 = f2bf(o[0]), h1 = f2bf(o[1]);
        typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
        bf16x2 hv; hv[0] = h0; hv[1] = h1;
        *reinterpret_cast<bf16x2*>(p.out + idx) = hv;
        if (p.out_np == 2) {
            bf16x2 lv; lv[0] = f2bf(o[0] - bf2f(h0)); lv[1] = f2bf(o[1] - bf2f(h1));
            *reinterpret_cast<bf16x2*>(p.out + p.out_plane + idx) = lv;
        }
    } else if constexpr (EPI == EPI_SCATTER_F32) {
        *reinterpret_cast<float4*>(p.out32 + (int64_t)tok * p.ldc32 + n) = make_float4(scale * v[0], scale * v[1], scale * v[2], scale * v[3]);
    } else if constexpr (EPI == EPI_SCATTER_ADD_PLANES) {
        float o[4] = {fmaf(scale, v[0], e.a.x), fmaf(scale, v[1], e.a.y), fmaf(scale, v[2], e.a.z), fmaf(scale, v[3], e.a.w)};
        store4p(p.out, p.out_plane, p.out_np, (int64_t)tok * p.ldc + n, o);
    } else if constexpr (EPI == EPI_HEADS_T) {
        int b = fdiv(m, p.rT), t = m - b * p.T;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            int nn = n + i;
            int h = fdiv(nn, p.rhd), d = nn - h * p.hd;
            store1p(p.out, p.out_plane, p.out_np, ((int64_t)(b * p.H + h) * p.hd + d) * p.Tpad + t, v[i]);
        }
    } else if constexpr (EPI == EPI_QKV_ROPE) {
        int sec = fdiv(n, p.rD);         // uniform over the 4 columns (D % 4 == 0)
        int nn = n - sec * p.D;
        int b = fdiv(m, p.rT), t = m - b * p.T;
        if (sec < 2) {
            const float c0 = e.a.x, c1 = e.a.y, s0 = e.a.z, s1 = e.a.w;
            float o[4] = {fmaf(v[0], c0, -(v[1] * s0)), fmaf(v[0], s0, v[1] * c0), fmaf(v[2], c1, -(v[3] * s1)), fmaf(v[2], s1, v[3] * c1)};
            if (p.abl == 7) return;
            if (sec == 0) store4p(p.q, p.q_plane, p.qkv_np, (int64_t)m * p.D + nn, o);
            else store4p(p.k, p.k_plane, p.qkv_np, (int64_t)m * p.D + nn, o);
        } else {
            if (p.abl == 6) return;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                int c = nn + i;
                int h = fdiv(c, p.rhd), d = c - h * p.hd;
                store1p(p.vt, p.vt_plane, p.qkv_np, ((int64_t)(b * p.H + h) * p.hd + d) * p.Tpad + t, v[i]);
            }
        }
    }
}

// the whole epilogue of one wave: rows slab by slab (i), loads of a slab first, then math + stores
template <int EPI, int TM = 2, int TN = 2>
__device__ __forceinline__ void wave_epilogue(const GemmDev& p, int g, f32x16 (&acc)[TM][TN], int row_base, int rows_end, int n_base,
                                              int frow, int fk) {
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        const int slot = row_base + i * 32 + frow;
        if (slot >= rows_end) continue;
        int tok = slot; float scale = 1.f;
        if constexpr (EPI == EPI_SCATTER_F32 || EPI == EPI_SCATTER_ADD_PLANES) {
            tok = p.rows_out[slot];
            scale = p.row_scale[tok];
        }
        if constexpr (EPI == EPI_SWIGLU) {
            if (p.row_scale2) scale = (slot < p.scale_split ? p.row_scale : p.row_scale2)[p.a_rows[slot]];
        }
        EpiPre pre[TN][4];
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int n = n_base + j * 32 + q * 8 + fk * 4;
                if (n < p.N) epi_load<EPI>(p, g, slot, tok, n, pre[j][q]);
            }
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int n = n_base + j * 32 + q * 8 + fk * 4;
                if (n >= p.N) continue;     // N % 4 == 0 is required
                float v[4] = {acc[i][j][q * 4 + 0], acc[i][j][q * 4 + 1], acc[i][j][q * 4 + 2], acc[i][j][q * 4 + 3]};
                epi_store<EPI>(p, g, slot, tok, scale, n, v, pre[j][q]);
            }
    }
}

template <int TM, int TN>
__device__ __forceinline__ void wave_epilogue_qkv_p16(const GemmDev& p, f32x16 (&acc)[TM][TN], int row_base, int rows_end, int n_base,
                                                      int frow, int fk) {
#pragma clang fp contract(off)
    const int hd2 = p.hd >> 1;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        const int m = row_base + i * 32 + frow;
        if (m >= rows_end) continue;
        const int b = fdiv(m, p.rT), t = m - b * p.T;
        // loads of the slab first (RoPE table: 8 pairs = two 16-byte loads each for cos and sin), then math + stores
        float4 cs[TN][2], sn[TN][2];
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int n = n_base + j * 32 + fk * 16;
            if (n < 2 * p.D) {
                const int nn = n - fdiv(n, p.rD) * p.D;
                const int jd = (nn - fdiv(nn, p.rhd) * p.hd) >> 1;
                const float* cp = p.rope_cos + (int64_t)t * hd2 + jd;
                const float* sp = p.rope_sin + (int64_t)t * hd2 + jd;
                cs[j][0] = *reinterpret_cast<const float4*>(cp); cs[j][1] = *reinterpret_cast<const float4*>(cp + 4);
                sn[j][0] = *reinterpret_cast<const float4*>(sp); sn[j][1] = *reinterpret_cast<const float4*>(sp + 4);
            }
        }
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int n = n_base + j * 32 + fk * 16;
            if (n >= p.N) continue;                          // N % 16 == 0 is required on this path
            const int sec = fdiv(n, p.rD);
            const int nn = n - sec * p.D;
            if (sec < 2) {
                const float c8[8] = {cs[j][0].x, cs[j][0].y, cs[j][0].z, cs[j][0].w, cs[j][1].x, cs[j][1].y, cs[j][1].z, cs[j][1].w};
                const float s8[8] = {sn[j][0].x, sn[j][0].y, sn[j][0].z, sn[j][0].w, sn[j][1].x, sn[j][1].y, sn[j][1].z, sn[j][1].w};
                float o[16];
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float v0 = acc[i][j][2 * e], v1 = acc[i][j][2 * e + 1];
                    o[2 * e] = fmaf(v0, c8[e], -(v1 * s8[e]));
                    o[2 * e + 1] = fmaf(v0, s8[e], v1 * c8[e]);
                }
                bf16_t* dst = sec == 0 ? p.q : p.k;
                const int64_t pl = sec == 0 ? p.q_plane : p.k_plane;
                store8p(dst, pl, p.qkv_np, (int64_t)m * p.D + nn, o);
                store8p(dst, pl, p.qkv_np, (int64_t)m * p.D + nn + 8, o + 8);
            } else {
                const int h = fdiv(nn, p.rhd), d0 = nn - h * p.hd;          // 16 | hd: the 16 columns stay inside one head
                const int64_t base = ((int64_t)(b * p.H + h) * p.hd + d0) * p.Tpad + t;
#pragma unroll
                for (int e = 0; e < 16; ++e) store1p(p.vt, p.vt_plane, p.qkv_np, base + (int64_t)e * p.Tpad, acc[i][j][e]);
            }
        }
    }
}

// V third of the QKV projection with the MFMA operands' roles exchanged (the workgroup reads the weight tile as its "row" operand and the
// token tile - source rows permuted - as its "column" operand): a lane then owns ONE head-dim column d and 16 CONSECUTIVE tokens per
// 32 x 32 tile, i.e. 32 contiguous bytes of the per-head V^T image [d][t] the attention kernel reads - two 16-byte stores where the
// row-per-lane layout needed sixteen 2-byte ones.  Same products, same k order: bit-identical.  Needs T % 16 == 0.
template <int TM, int TN>
__device__ __forceinline__ void wave_epilogue_vt_p16(const GemmDev& p, f32x16 (&acc)[TM][TN], int d_base, int tok_base, int rows_end, int frow, int fk) {
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        const int n = d_base + i * 32 + frow;             // output column of the projection (this lane's weight row)
        if (n >= p.N) continue;
        const int nn = n - 2 * p.D;
        const int h = fdiv(nn, p.rhd), d = nn - h * p.hd;
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int m0 = tok_base + j * 32 + 16 * fk;
            if (m0 >= rows_end) continue;
            const int b = fdiv(m0, p.rT), t = m0 - b * p.T;
            const int64_t base = ((int64_t)(b * p.H + h) * p.hd + d) * p.Tpad + t;
            float o[16];
#pragma unroll
            for (int e = 0; e < 16; ++e) o[e] = acc[i][j][e];
            if (m0 + 15 < rows_end) {
                store8p(p.vt, p.vt_plane, p.qkv_np, base, o);
                store8p(p.vt, p.vt_plane, p.qkv_np, base + 8, o + 8);
            } else {
#pragma unroll
                for (int e = 0; e < 16; ++e)
                    if (m0 + e < rows_end) store1p(p.vt, p.vt_plane, p.qkv_np, base + e, o[e]);
            }
        }
    }
}

// SwiGLU epilogue of one wave in the P16 layout: 16 consecutive (w1, w3)-interleaved columns = 8 hidden values = one 16-byte store
template <int TM, int TN>
__device__ __forceinline__ void wave_epilogue_swiglu_p16(const GemmDev& p, int g, f32x16 (&acc)[TM][TN], int row_base, int rows_end, int n_base,
                                                         int frow, int fk) {
#pragma clang fp contract(off)
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        const int m = row_base + i * 32 + frow;
        if (m >= rows_end) continue;
        float gs = 1.f;
        if (p.row_scale2) gs = (m < p.scale_split ? p.row_scale : p.row_scale2)[p.a_rows[m]];     // routed gate weight of this slot's token
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int n = n_base + j * 32 + fk * 16;
            if (n >= p.N) continue;                          // N % 16 == 0 is required on this path
            float o[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                o[e] = silu_f(acc[i][j][2 * e]) * acc[i][j][2 * e + 1];
                if (p.row_scale2) o[e] *= gs;
            }
            store8p(p.out, p.out_plane, p.out_np, (int64_t)m * p.ldc + g * p.c_noff_group + (n >> 1), o);
        }
    }
}

// Block-wide epilogue staged through LDS (which is free once the k-loop is over).  The MFMA accumulator layout gives a lane
// one output ROW and 4 consecutive columns, so direct stores put 8-16 B pieces of 32 different rows in every instruction.
// Here a slab of 64 rows x BN columns goes to LDS as fp32 and is read back row-major: a lane still owns 4 consecutive
// columns of one row (the epi_load / epi_store contract) but a wave now covers whole 128-B lines - residual / bias loads and
// all stores are full-line transactions.  The V third of the QKV projection is staged TRANSPOSED instead and written as
// 4 consecutive tokens of one (head, d) row: the per-head V^T image the attention kernel reads, in 8-B pieces of 128-B runs.
// Needs 64 * (BN + 4) * 4 bytes of LDS (BN * 68 * 4 for the transposed variant).
// (NWC wave columns x 2 wave rows, NT threads: 2 x 2 / 256 for the 4-wave kernels, 4 x 2 / 512 for the 8-wave kernel)
// HOIST (gated-residual epilogue of the fused band-expert kernel): the residual and gate values of a whole slab are requested BEFORE the
// slab goes through LDS, not after the second barrier in two passes: one exposed HBM round trip per slab, overlapped with the staging,
// instead of two behind it (same loads, same arithmetic, other issue order): band experts 63.2 -> 55.8 us at 12032 tokens (same box).
template <int EPI, int TM, int TN, int NWC = 2, int NT = NTHREADS, bool HOIST = false>
__device__ __forceinline__ void staged_epilogue(const GemmDev& p, int g, f32x16 (&acc)[TM][TN], float* stg, int row0, int rows_end,
                                                int n0, int tid, int wr, int wc, int frow, int fk) {
    static_assert(NT == 128 * NWC, "two wave rows of NWC waves");
    static_assert(!HOIST || EPI == EPI_RESID_GATE, "hoisted loads: gated-residual epilogue only");
    constexpr int BNB = NWC * 32 * TN;
    constexpr int PITCH = BNB + 4;               // floats; +4 keeps the 16-B column writes of 8 consecutive rows on distinct banks
    constexpr int QPR = BNB / 4;                 // quads per row
    constexpr int QPT = 64 * QPR / NT;           // quads per thread per slab
    bool vsec = false;
    if constexpr (EPI == EPI_QKV_ROPE) vsec = n0 >= 2 * p.D && (p.D % BNB) == 0 && (p.T & 3) == 0 && (p.Tpad & 3) == 0;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        EpiPre preH[HOIST ? QPT : 1];
        if constexpr (HOIST) {
#pragma unroll
            for (int k = 0; k < QPT; ++k) {
                const int idx = tid + k * NT;
                const int lr = idx / QPR, cq = idx - lr * QPR;
                int slot = row0 + (lr >> 5) * 32 * TM + i * 32 + (lr & 31);
                int n = n0 + cq * 4;
                if (slot >= rows_end || n >= p.N) { slot = row0; n = n0; }      // (clamped, not branched: the stores below skip it)
                epi_load<EPI>(p, g, slot, slot, n, preH[k]);
            }
        }
        __builtin_amdgcn_s_waitcnt(0xc07f);      // lgkmcnt(0): own LDS reads done (loop fragments / previous slab)
        __builtin_amdgcn_s_barrier();
        if constexpr (EPI == EPI_QKV_ROPE) {
            if (vsec) {
                constexpr int PT = 64 + 4;       // transposed image [col][row]
#pragma unroll
                for (int j = 0; j < TN; ++j)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int col = wc * 32 * TN + j * 32 + (r >> 2) * 8 + fk * 4 + (r & 3);
                        stg[col * PT + wr * 32 + frow] = acc[i][j][r];
                    }
                __builtin_amdgcn_s_waitcnt(0xc07f);
                __builtin_amdgcn_s_barrier();
                constexpr int IPT = BNB * 16 / NT;
#pragma unroll
                for (int k = 0; k < IPT; ++k) {
                    const int idx = tid + k * NT;
                    const int rq = idx & 15, c = idx >> 4;
                    const int lr = rq * 4;
                    const int slot = row0 + (lr >> 5) * 32 * TM + i * 32 + (lr & 31);
                    const int n = n0 + c;
                    if (slot >= rows_end || n >= p.N) continue;
                    const float4 vv = *reinterpret_cast<const float4*>(stg + c * PT + lr);
                    float v[4] = {vv.x, vv.y, vv.z, vv.w};
                    const int nn = n - 2 * p.D;
                    const int h = fdiv(nn, p.rhd), d = nn - h * p.hd;
                    const int b = fdiv(slot, p.rT), t = slot - b * p.T;
                    const int64_t base = ((int64_t)(b * p.H + h) * p.hd + d) * p.Tpad;
                    if (slot + 3 < rows_end && t + 3 < p.T) {
                        store4p(p.vt, p.vt_plane, p.qkv_np, base + t, v);
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const int m = slot + e;
                            if (m >= rows_end) break;
                            const int bb = fdiv(m, p.rT), tt = m - bb * p.T;
                            store1p(p.vt, p.vt_plane, p.qkv_np, ((int64_t)(bb * p.H + h) * p.hd + d) * p.Tpad + tt, v[e]);
                        }
                    }
                }
                continue;
            }
        }
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int col = wc * 32 * TN + j * 32 + q * 8 + fk * 4;
                *reinterpret_cast<float4*>(stg + (wr * 32 + frow) * PITCH + col) =
                    make_float4(acc[i][j][q * 4 + 0], acc[i][j][q * 4 + 1], acc[i][j][q * 4 + 2], acc[i][j][q * 4 + 3]);
            }
        __builtin_amdgcn_s_waitcnt(0xc07f);
        __builtin_amdgcn_s_barrier();
        // (in passes of at most 8 quads per thread: loads of a pass are issued before its stores; bounds the live registers)
        constexpr int QC = QPT > 8 ? QPT / 2 : QPT;
        static_assert(QPT % QC == 0, "quads per thread must split evenly");
#pragma unroll
        for (int kb = 0; kb < QPT; kb += QC) {
        EpiPre pre[QC];
        int slot_[QC], tok_[QC]; float scale_[QC];
#pragma unroll
        for (int kk = 0; kk < QC; ++kk) {
            const int k = kk, idx = tid + (kb + kk) * NT;
            const int lr = idx / QPR, cq = idx - lr * QPR;
            const int slot = row0 + (lr >> 5) * 32 * TM + i * 32 + (lr & 31);
            const int n = n0 + cq * 4;
            slot_[k] = (slot < rows_end && n < p.N) ? slot : -1;
            tok_[k] = slot; scale_[k] = 1.f;
            if (slot_[k] >= 0) {
                if constexpr (EPI == EPI_SCATTER_F32 || EPI == EPI_SCATTER_ADD_PLANES) {
                    tok_[k] = p.rows_out[slot];
                    scale_[k] = p.row_scale[tok_[k]];
                }
                if constexpr (EPI == EPI_SWIGLU) {
                    if (p.row_scale2) scale_[k] = (slot < p.scale_split ? p.row_scale : p.row_scale2)[p.a_rows[slot]];
                }
                if constexpr (HOIST) pre[k] = preH[kb + kk];
                else epi_load<EPI>(p, g, slot, tok_[k], n, pre[k]);
            }
        }
#pragma unroll
        for (int kk = 0; kk < QC; ++kk) {
            const int k = kk;
            if (slot_[k] < 0) continue;
            const int idx = tid + (kb + kk) * NT;
            const int lr = idx / QPR, cq = idx - lr * QPR;
            const float4 vv = *reinterpret_cast<const float4*>(stg + lr * PITCH + cq * 4);
            float v[4] = {vv.x, vv.y, vv.z, vv.w};
            epi_store<EPI>(p, g, slot_[k], tok_[k], scale_[k], n0 + cq * 4, v, pre[k]);
        }
        }
    }
}

// which epilogues of the 128x128 kernel go through LDS (staged_epilogue) instead of storing from the MFMA layout
#ifndef VB_STAGED_MASK
#define VB_STAGED_MASK 0x91       /* measured per epilogue: PLANES, SWIGLU, GELU_PLANES gain; QKV_ROPE and the fp32 ones do not */
#endif
#define STAGED_EPI(E) (((VB_STAGED_MASK) >> (E)) & 1)

extern unsigned long long* g_gemm_trace;      // tuning only (vbdbg_gemm_trace, gemm_bf16.hip): the launchers copy it into GemmDev::trace
#ifdef VB_EXPERIMENTS
// gemm_bf16_pk.hip: the persistent 8-wave kernel (experiments build only); launch_gemm routes to these
#define PK_MAX_GROUPS 16                      // capacity of the kernel's row-group table
void launch_gemm_pk(int epi, const GemmDev& d, hipStream_t st);            // epi: EPI_QKV_ROPE or EPI_SWIGLU
void launch_gemm_pk_f32(const GemmDev& d, hipStream_t st, int code);       // VB_GEMM_PK_F32 = 1 + ablation code, 100 = traced
#endif
