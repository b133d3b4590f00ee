// Memory-bound and tiny kernels of the DiT, T5 and the sampler's tabulation (gfx950): norms, casts, the pooled-caption mean, stem helpers,
// the FinalLayer input for the GEMM route, the adaLN tabulation operand, the acoustic gate logits and proj_in as a GEMM.
// All are wave64-shaped: one wave per row with float4 lanes where rows are 768 wide.
// (The sampler's update and bookkeeping: sampler_step.hip; router and bucketing: routing.hip; conv-net glue: net_glue.hip.)
#include "kernels.h"


// ---------------------------------------------------------------------------
// RMSNorm * w, then adaLN modulate, written as bf16 planes (feeds the MFMA GEMMs)
//   RMSNorm  flag_large_dit_moe.py:52-77 ; modulate :80-81
// ---------------------------------------------------------------------------
// (round 3: the row stays in registers between the two passes - the second pass re-read it from L2 - and a wave walks TWO rows with all
//  their loads issued up front; same arithmetic in the same order, bit-identical)
template <int NQ>     // D = 256 * NQ (NQ float4 per lane and row); NQ = 0: generic D % 4 == 0 (re-reads the row)
__global__ void __launch_bounds__(256) rmsnorm_mod_kernel(const float* __restrict__ h, const float* __restrict__ w,
                                                         const float* shift, const float* scale, int mod_ld, int rows, int D,
                                                         int T, float eps, Planes out) {
#pragma clang fp contract(off)      // both forms must round alike: no implicit fma
    const int lane = threadIdx.x & 63;
    if constexpr (NQ == 0) {
        const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
        if (row >= rows) return;
        const float* x = h + (int64_t)row * D;
        float ss = 0.f;
        for (int k = lane * 4; k < D; k += 256) {
            float4 v = *reinterpret_cast<const float4*>(x + k);
            ss += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
        }
        ss = wave_sum(ss);
        const float r = rsqrtf(ss / (float)D + eps);
        const int b = row / T;
        for (int k = lane * 4; k < D; k += 256) {
            float4 v = *reinterpret_cast<const float4*>(x + k);
            float4 ww = *reinterpret_cast<const float4*>(w + k);
            float o[4] = {v.x * r * ww.x, v.y * r * ww.y, v.z * r * ww.z, v.w * r * ww.w};
            if (scale) {
                float4 sc = *reinterpret_cast<const float4*>(scale + (int64_t)b * mod_ld + k);
                float4 sh = *reinterpret_cast<const float4*>(shift + (int64_t)b * mod_ld + k);
                o[0] = o[0] * (1.f + sc.x) + sh.x; o[1] = o[1] * (1.f + sc.y) + sh.y;
                o[2] = o[2] * (1.f + sc.z) + sh.z; o[3] = o[3] * (1.f + sc.w) + sh.w;
            }
            bf16x4 hi;
#pragma unroll
            for (int i = 0; i < 4; ++i) hi[i] = f2bf(o[i]);
            *reinterpret_cast<bf16x4*>(out.p + (int64_t)row * D + k) = hi;
            if (out.np == 2) {
                bf16x4 lo;
#pragma unroll
                for (int i = 0; i < 4; ++i) lo[i] = f2bf(o[i] - bf2f(hi[i]));
                *reinterpret_cast<bf16x4*>(out.p + out.plane + (int64_t)row * D + k) = lo;
            }
        }
    } else {
        const int row0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * 2;
        if (row0 >= rows) return;
        float4 v[2][NQ];
#pragma unroll
        for (int rr = 0; rr < 2; ++rr) {
            const float* x = h + (int64_t)min(row0 + rr, rows - 1) * D;
#pragma unroll
            for (int i = 0; i < NQ; ++i) v[rr][i] = *reinterpret_cast<const float4*>(x + lane * 4 + 256 * i);
        }
        float4 ww[NQ];
#pragma unroll
        for (int i = 0; i < NQ; ++i) ww[i] = *reinterpret_cast<const float4*>(w + lane * 4 + 256 * i);
#pragma unroll
        for (int rr = 0; rr < 2; ++rr) {
            const int row = row0 + rr;
            if (row >= rows) break;
            float ss = 0.f;
#pragma unroll
            for (int i = 0; i < NQ; ++i) ss += v[rr][i].x * v[rr][i].x + v[rr][i].y * v[rr][i].y + v[rr][i].z * v[rr][i].z + v[rr][i].w * v[rr][i].w;
            ss = wave_sum(ss);
            const float r = rsqrtf(ss / (float)D + eps);
            const int b = row / T;
#pragma unroll
            for (int i = 0; i < NQ; ++i) {
                const int k = lane * 4 + 256 * i;
                float o[4] = {v[rr][i].x * r * ww[i].x, v[rr][i].y * r * ww[i].y, v[rr][i].z * r * ww[i].z, v[rr][i].w * r * ww[i].w};
                if (scale) {
                    float4 sc = *reinterpret_cast<const float4*>(scale + (int64_t)b * mod_ld + k);
                    float4 sh = *reinterpret_cast<const float4*>(shift + (int64_t)b * mod_ld + k);
                    o[0] = o[0] * (1.f + sc.x) + sh.x; o[1] = o[1] * (1.f + sc.y) + sh.y;
                    o[2] = o[2] * (1.f + sc.z) + sh.z; o[3] = o[3] * (1.f + sc.w) + sh.w;
                }
                bf16x4 hi;
#pragma unroll
                for (int e = 0; e < 4; ++e) hi[e] = f2bf(o[e]);
                *reinterpret_cast<bf16x4*>(out.p + (int64_t)row * D + k) = hi;
                if (out.np == 2) {
                    bf16x4 lo;
#pragma unroll
                    for (int e = 0; e < 4; ++e) lo[e] = f2bf(o[e] - bf2f(hi[e]));
                    *reinterpret_cast<bf16x4*>(out.p + out.plane + (int64_t)row * D + k) = lo;
                }
            }
        }
    }
}
int launch_rmsnorm_mod(const float* h, const float* w, const float* shift, const float* scale, int mod_ld, int rows, int D,
                       int T, float eps, Planes out, hipStream_t st) {
    if (D % 4) VB_FAIL(VB_E_INVALID, "rmsnorm: D%%4");
    const int Tq = T > 0 ? T : 1;
    if (D == 768 && !vb_tune().rmsnorm_generic) hipLaunchKernelGGL(rmsnorm_mod_kernel<3>, dim3(cdiv(rows, 8)), dim3(256), 0, st, h, w, shift, scale, mod_ld, rows, D, Tq, eps, out);
    else if (D == 1024 && !vb_tune().rmsnorm_generic) hipLaunchKernelGGL(rmsnorm_mod_kernel<4>, dim3(cdiv(rows, 8)), dim3(256), 0, st, h, w, shift, scale, mod_ld, rows, D, Tq, eps, out);
    else hipLaunchKernelGGL(rmsnorm_mod_kernel<0>, dim3(cdiv(rows, 4)), dim3(256), 0, st, h, w, shift, scale, mod_ld, rows, D, Tq, eps, out);
    VB_CHECK_LAUNCH();
    return VB_OK;
}

// ---------------------------------------------------------------------------
// LayerNorm (optional affine) -> fp32 and/or planes
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) layernorm_kernel(const float* __restrict__ x, const float* w, const float* bvec, int rows,
                                                       int D, float eps, float* out32, Planes outp) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    const float* xr = x + (int64_t)row * D;
    float s = 0.f;
    for (int k = lane; k < D; k += 64) s += xr[k];
    const float mean = wave_sum(s) / (float)D;
    float vs = 0.f;
    for (int k = lane; k < D; k += 64) { float d = xr[k] - mean; vs += d * d; }
    const float r = rsqrtf(wave_sum(vs) / (float)D + eps);
    for (int k = lane; k < D; k += 64) {
        float o = (xr[k] - mean) * r;
        if (w) o = o * w[k] + bvec[k];
        if (out32) out32[(int64_t)row * D + k] = o;
        if (outp.p) {
            bf16_t hi = f2bf(o);
            outp.p[(int64_t)row * D + k] = hi;
            if (outp.np == 2) outp.p[outp.plane + (int64_t)row * D + k] = f2bf(o - bf2f(hi));
        }
    }
}
int launch_layernorm(const float* x, const float* w, const float* b, int rows, int D, float eps, float* out32, Planes outp,
                     hipStream_t st) {
    hipLaunchKernelGGL(layernorm_kernel, dim3(cdiv(rows, 4)), dim3(256), 0, st, x, w, b, rows, D, eps, out32, outp);
    VB_CHECK_LAUNCH();
    return VB_OK;
}

// ---------------------------------------------------------------------------
// casts
// ---------------------------------------------------------------------------
__global__ void cast_planes_kernel(const float* __restrict__ x, int64_t n, Planes out) {
    int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x * 4;
    for (; i < n; i += stride) {
        if (i + 3 < n) {
            float4 v = *reinterpret_cast<const float4*>(x + i);
            float o[4] = {v.x, v.y, v.z, v.w};
            bf16x4 hi, lo;
#pragma unroll
            for (int k = 0; k < 4; ++k) { hi[k] = f2bf(o[k]); lo[k] = f2bf(o[k] - bf2f(hi[k])); }
            *reinterpret_cast<bf16x4*>(out.p + i) = hi;
            if (out.np == 2) *reinterpret_cast<bf16x4*>(out.p + out.plane + i) = lo;
        } else {
            for (int64_t j = i; j < n; ++j) {
                bf16_t hi = f2bf(x[j]);
                out.p[j] = hi;
                if (out.np == 2) out.p[out.plane + j] = f2bf(x[j] - bf2f(hi));
            }
        }
    }
}
int launch_cast_planes(const float* x, int64_t n, Planes out, hipStream_t st) {
    int blocks = (int)((n / 4 + 255) / 256);
    if (blocks > 4096) blocks = 4096;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(cast_planes_kernel, dim3(blocks), dim3(256), 0, st, x, n, out);
    VB_CHECK_LAUNCH();
    return VB_OK;
}
__global__ void planes_to_f32_kernel(Planes in, int64_t n, float* out) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) {
        float v = bf2f(in.p[i]);
        if (in.np == 2) v += bf2f(in.p[in.plane + i]);
        out[i] = v;
    }
}
int launch_planes_to_f32(Planes in, int64_t n, float* out, hipStream_t st) {
    int blocks = (int)((n + 255) / 256);
    if (blocks > 4096) blocks = 4096;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(planes_to_f32_kernel, dim3(blocks), dim3(256), 0, st, in, n, out);
    VB_CHECK_LAUNCH();
    return VB_OK;
}
__global__ void fill_f32_kernel(float* p, int64_t n, float v) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) p[i] = v;
}
int launch_fill_f32(float* p, int64_t n, float v, hipStream_t st) {
    int blocks = (int)((n + 255) / 256);
    if (blocks > 4096) blocks = 4096;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(fill_f32_kernel, dim3(blocks), dim3(256), 0, st, p, n, v);
    VB_CHECK_LAUNCH();
    return VB_OK;
}

// mean over L rows: [B][L][D] -> [B][D]   (pooled caption, vocal2music_moe.py:410-412)
__global__ void mean_rows_kernel(const float* __restrict__ x, int B, int L, int D, float* out) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * D) return;
    int b = i / D, d = i - b * D;
    float s = 0.f;
    for (int l = 0; l < L; ++l) s += x[((int64_t)b * L + l) * D + d];
    out[i] = s / (float)L;
}
int launch_mean_rows(const float* x, int B, int L, int D, float* out, hipStream_t st) {
    hipLaunchKernelGGL(mean_rows_kernel, dim3(cdiv(B * D, 256)), dim3(256), 0, st, x, B, L, D, out);
    VB_CHECK_LAUNCH();
    return VB_OK;
}

// ---------------------------------------------------------------------------
// stem helpers (vocal2music_moe.py:388-393)
// ---------------------------------------------------------------------------
// out[b][d][t] = table[idx[b][t]][d]; with row lengths (len: device [B], counted in units of len_mul positions) 0 for t >= len_mul * len[b],
// and idx is not read there: the k5p2 convolutions behind it then see the zero padding of the clip alone
__global__ void embed_t_kernel(const int64_t* __restrict__ idx, const float* __restrict__ table, int B, int T, int D, int vocab, float* out,
                               const int* __restrict__ len, int len_mul) {
    __shared__ float tile[64][65];
    const int b = blockIdx.z, t0 = blockIdx.x * 64, d0 = blockIdx.y * 64;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;   // 256 threads: 64 x 4
    const int tend = len ? len_mul * len[b] : T;
    for (int i = ty; i < 64; i += 4) {
        int t = t0 + i;
        if (t >= tend) tile[i][tx] = 0.f;
        else if (t < T && d0 + tx < D) {
            //  the host range-checks index tensors once per identity; the read itself is clamped so that a buffer refilled behind
            // that cache (raw pointer writes, DLPack aliases) can never index outside the table
            int64_t ix = idx[(int64_t)b * T + t];
            ix = ix < 0 ? 0 : (ix >= vocab ? vocab - 1 : ix);
            tile[i][tx] = table[ix * D + d0 + tx];
        }
    }
    __syncthreads();
    for (int i = ty; i < 64; i += 4) {
        int d = d0 + i, t = t0 + tx;
        if (d < D && t < T) out[((int64_t)b * D + d) * T + t] = tile[tx][i];
    }
}
int launch_embed_t(const int64_t* idx, const float* table, int B, int T, int D, int vocab, float* out, hipStream_t st, const int* len, int len_mul) {
    hipLaunchKernelGGL(embed_t_kernel, dim3(cdiv(T, 64), cdiv(D, 64), B), dim3(256), 0, st, idx, table, B, T, D, vocab, out, len, len_mul);
    VB_CHECK_LAUNCH();
    return VB_OK;
}
// out[b][c][t] = (a[2t]+a[2t+1])/2 + (b[2t]+b[2t+1])/2    (AvgPool1d(2) of both branches, then sum)
__global__ void pool_add_kernel(const float* __restrict__ a, const float* __restrict__ bb, int64_t rows, int T_in, float* out) {
    const int To = T_in / 2;
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * To) return;
    int64_t r = i / To; int t = (int)(i - r * To);
    const float* pa = a + r * T_in + 2 * t;
    const float* pb = bb + r * T_in + 2 * t;
    out[i] = (pa[0] + pa[1]) * 0.5f + (pb[0] + pb[1]) * 0.5f;
}
int launch_pool_add(const float* a, const float* b, int B, int C, int T_in, float* out, hipStream_t st) {
    int64_t n = (int64_t)B * C * (T_in / 2);
    hipLaunchKernelGGL(pool_add_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a, b, (int64_t)B * C, T_in, out);
    VB_CHECK_LAUNCH();
    return VB_OK;
}
// [B][C][T_in] -> [B][T_out][C]; rows t >= T_in repeat the last input row (length fix-up :397-401)
__global__ void transpose_bct_btc_kernel(const float* __restrict__ in, int C, int T_in, int T_out, float* out) {
    __shared__ float tile[64][65];
    const int b = blockIdx.z, t0 = blockIdx.x * 64, c0 = blockIdx.y * 64;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    for (int i = ty; i < 64; i += 4) {
        int c = c0 + i, t = t0 + tx;
        int ts = t < T_in ? t : T_in - 1;
        if (c < C && t < T_out) tile[i][tx] = in[((int64_t)b * C + c) * T_in + ts];
    }
    __syncthreads();
    for (int i = ty; i < 64; i += 4) {
        int t = t0 + i, c = c0 + tx;
        if (t < T_out && c < C) out[((int64_t)b * T_out + t) * C + c] = tile[tx][i];
    }
}
int launch_transpose_bct_btc(const float* in, int B, int C, int T_in, int T_out, float* out, hipStream_t st) {
    hipLaunchKernelGGL(transpose_bct_btc_kernel, dim3(cdiv(T_out, 64), cdiv(C, 64), B), dim3(256), 0, st, in, C, T_in, T_out, out);
    VB_CHECK_LAUNCH();
    return VB_OK;
}

// ---------------------------------------------------------------------------
// proj_in (Conv1d C -> D, k taps; vocal2music_moe.py:395) as a GEMM: the latent window of every token as one K-contiguous row
//   A[plane][m = b*T + t][k = tap*32 + ci] = split-bf16( x[b][ci][t + tap - pad] )   (zero outside the clip, for ci >= C and for k >= taps*32)
// With row lengths (len: device [B]) the clip of row b ends at len[b]: taps at or beyond it are zero and x is not read there.
// and the split conv weights [2][taps][D][32] re-laid as B[plane][D][KP].  One thread = one 16-byte group of 8 consecutive k.
// ---------------------------------------------------------------------------
__global__ void im2col_latent_kernel(const float* __restrict__ x, int B, int C, int T, int taps, int pad, int KP, bf16_t* __restrict__ out,
                                     int64_t plane, const int* __restrict__ len) {
    const int gpr = KP >> 3;
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (int64_t)B * T * gpr) return;
    const int m = (int)(idx / gpr), gi = (int)(idx - (int64_t)m * gpr);
    const int b = m / T, t = m - b * T;
    const int k0 = gi * 8, tap = k0 >> 5, ci0 = k0 & 31;
    const int ts = t + tap - pad;
    const int tend = len ? len[b] : T;
    bf16x8 hi, lo;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int ci = ci0 + e;
        const float v = (tap < taps && ci < C && ts >= 0 && ts < tend) ? x[((int64_t)b * C + ci) * T + ts] : 0.f;
        hi[e] = f2bf(v);
        lo[e] = f2bf(v - bf2f(hi[e]));
    }
    *reinterpret_cast<bf16x8*>(out + (int64_t)m * KP + k0) = hi;
    *reinterpret_cast<bf16x8*>(out + plane + (int64_t)m * KP + k0) = lo;
}
int launch_im2col_latent(const float* x, int B, int C, int T, int taps, int pad, int KP, bf16_t* out, int64_t plane, hipStream_t st, const int* len) {
    if (KP % 8 || C > 32 || taps * 32 > KP) VB_FAIL(VB_E_INVALID, "im2col_latent: C=%d taps=%d KP=%d", C, taps, KP);
    const int64_t n = (int64_t)B * T * (KP / 8);
    hipLaunchKernelGGL(im2col_latent_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, x, B, C, T, taps, pad, KP, out, plane, len);
    VB_CHECK_LAUNCH();
    return VB_OK;
}
// the same mask for the proj_in routes that are a general convolution kernel: out[b][c][t] = t < len[b] * len_mul ? x[b][c][t] : 0 (a select:
// x's padding, NaN included, is not read into the copy).  len_mul: samples of x per unit of len (the VAE encoder's mel frames per latent token)
__global__ void mask_latent_kernel(const float* __restrict__ x, int B, int C, int T, const int* __restrict__ len, int len_mul,
                                   float* __restrict__ out) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (int64_t)B * C * T) return;
    const int t = (int)(idx % T), b = (int)(idx / ((int64_t)C * T));
    out[idx] = t < len[b] * len_mul ? x[idx] : 0.f;
}
int launch_mask_latent(const float* x, int B, int C, int T, const int* len, float* out, hipStream_t st, int len_mul) {
    if (len_mul < 1) VB_FAIL(VB_E_INVALID, "mask_latent: len_mul = %d (>= 1)", len_mul);
    hipLaunchKernelGGL(mask_latent_kernel, dim3(cdiv((int64_t)B * C * T, 256)), dim3(256), 0, st, x, B, C, T, len, len_mul, out);
    VB_CHECK_LAUNCH();
    return VB_OK;
}
// the row lengths of a call, by value in the argument block (nothing of the caller's host array outlives the call, and a captured graph
// holds its own copy), into the workspace table the kernels above and the attention read
__global__ void lens_table_kernel(const LensPlan lp, int* __restrict__ out) {
    if ((int)threadIdx.x < lp.B) out[threadIdx.x] = lp.len[threadIdx.x];
}
int launch_lens_table(const LensPlan& lp, int* out, hipStream_t st) {
    hipLaunchKernelGGL(lens_table_kernel, dim3(1), dim3(64), 0, st, lp, out);
    VB_CHECK_LAUNCH();
    return VB_OK;
}
// row lengths in a conv net: the tails out[b][c][len[b] * tmul .. Tp) of an activation buffer [B][C][Tp] back to zero after the op that wrote
// it, so that the next convolution reads behind row b's end what the clip-alone call's zero padding supplies.  grid = (pieces of the
// longest tail, C, B): a workgroup of a full row, or behind a shorter tail's end, leaves at once.  VEC: Tp, every short row's tail start and
// the base are 16-byte multiples (the host checked) - one float4 per lane; otherwise one float.
template <bool VEC>
__global__ void __launch_bounds__(256) tail_zero_kernel(float* __restrict__ out, const int* __restrict__ len, int C, int Tp, int tmul) {
    const int b = blockIdx.z, c = blockIdx.y;
    const int start = len[b] * tmul;
    const int i = (blockIdx.x * 256 + threadIdx.x) * (VEC ? 4 : 1);
    if (start + i >= Tp) return;
    float* p = out + ((int64_t)b * C + c) * Tp + start + i;
    if constexpr (VEC) *reinterpret_cast<float4*>(p) = make_float4(0.f, 0.f, 0.f, 0.f);
    else *p = 0.f;
}
int launch_tail_zero(float* out, const LensPlan& lp, const int* len, int B, int C, int T, int tmul, hipStream_t st) {
    if (lp.B != B || C < 1 || C > 65535 || tmul < 1) VB_FAIL(VB_E_INVALID, "tail_zero: %d lengths for B=%d, C=%d, tmul=%d", lp.B, B, C, tmul);
    const int Tp = T * tmul;
    int tail = 0;
    bool vec = Tp % 4 == 0 && aligned16(out);
    for (int b = 0; b < B; ++b) {
        if (lp.len[b] >= T) continue;
        if ((T - lp.len[b]) * tmul > tail) tail = (T - lp.len[b]) * tmul;
        vec = vec && (lp.len[b] * tmul) % 4 == 0;
    }
    if (tail == 0) return VB_OK;
    const dim3 grid(cdiv(tail, vec ? 1024 : 256), C, B);
    if (vec) hipLaunchKernelGGL(tail_zero_kernel<true>, grid, dim3(256), 0, st, out, len, C, Tp, tmul);
    else hipLaunchKernelGGL(tail_zero_kernel<false>, grid, dim3(256), 0, st, out, len, C, Tp, tmul);
    VB_CHECK_LAUNCH();
    return VB_OK;
}
__global__ void conv_w_to_gemm_kernel(const bf16_t* __restrict__ w3, int64_t w3_plane, int taps, int D, int KP, bf16_t* __restrict__ out) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;      // (plane, co, k)
    if (idx >= (int64_t)2 * D * KP) return;
    const int k = (int)(idx % KP), co = (int)((idx / KP) % D), pl = (int)(idx / ((int64_t)KP * D));
    const int tap = k >> 5, ci = k & 31;
    out[idx] = tap < taps ? w3[pl * w3_plane + ((int64_t)tap * D + co) * 32 + ci] : f2bf(0.f);
}
int launch_conv_w_to_gemm(const bf16_t* w3, int64_t w3_plane, int taps, int D, int KP, bf16_t* out, hipStream_t st) {
    const int64_t n = (int64_t)2 * D * KP;
    hipLaunchKernelGGL(conv_w_to_gemm_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, w3, w3_plane, taps, D, KP, out);
    VB_CHECK_LAUNCH();
    return VB_OK;
}

// out[n][e] = x[n] . W[e] + b[e]   (acoustic gate logits, precompute)
__global__ void __launch_bounds__(256) rows_dot_kernel(const float* __restrict__ x, const float* __restrict__ W,
                                                      const float* __restrict__ bias, int N, int D, int E, float* out) {
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (n >= N) return;
    for (int e = 0; e < E; ++e) {
        float acc = 0.f;
        for (int k = lane * 4; k < D; k += 256) {
            float4 xv = *reinterpret_cast<const float4*>(x + (int64_t)n * D + k);
            float4 wv = *reinterpret_cast<const float4*>(W + (int64_t)e * D + k);
            acc += xv.x * wv.x + xv.y * wv.y + xv.z * wv.z + xv.w * wv.w;
        }
        acc = wave_sum(acc);
        if (lane == 0) out[(int64_t)n * E + e] = acc + bias[e];
    }
}
int launch_rows_dot(const float* x, const float* W, const float* bias, int N, int D, int E, float* out, hipStream_t st) {
    hipLaunchKernelGGL(rows_dot_kernel, dim3(cdiv(N, 4)), dim3(256), 0, st, x, W, bias, N, D, E, out);
    VB_CHECK_LAUNCH();
    return VB_OK;
}

// FinalLayer input: LayerNorm without affine (eps) then adaLN modulate, as split-bf16 planes; one wave per row, the row
// (D <= 1024) lives in registers between the two reductions
__global__ void __launch_bounds__(256) layernorm_mod_planes_kernel(const float* __restrict__ h, const float* __restrict__ shift,
                                                                  const float* __restrict__ scale, int mod_ld, int rows, int D, int T,
                                                                  float eps, Planes out) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    const float* x = h + (int64_t)row * D;
    float4 v[4];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int k = lane * 4 + i * 256;
        v[i] = k < D ? *reinterpret_cast<const float4*>(x + k) : make_float4(0.f, 0.f, 0.f, 0.f);
        s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
    }
    const float mean = wave_sum(s) / (float)D;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int k = lane * 4 + i * 256;
        if (k < D) {
            const float d0 = v[i].x - mean, d1 = v[i].y - mean, d2 = v[i].z - mean, d3 = v[i].w - mean;
            q += (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
        }
    }
    const float rs = rsqrtf(wave_sum(q) / (float)D + eps);
    const int b = row / T;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int k = lane * 4 + i * 256;
        if (k >= D) continue;
        const float4 sc = *reinterpret_cast<const float4*>(scale + (int64_t)b * mod_ld + k);
        const float4 sh = *reinterpret_cast<const float4*>(shift + (int64_t)b * mod_ld + k);
        const float o[4] = {(v[i].x - mean) * rs * (1.f + sc.x) + sh.x, (v[i].y - mean) * rs * (1.f + sc.y) + sh.y,
                            (v[i].z - mean) * rs * (1.f + sc.z) + sh.z, (v[i].w - mean) * rs * (1.f + sc.w) + sh.w};
        bf16x4 hi, lo;
#pragma unroll
        for (int e = 0; e < 4; ++e) { hi[e] = f2bf(o[e]); lo[e] = f2bf(o[e] - bf2f(hi[e])); }
        *reinterpret_cast<bf16x4*>(out.p + (int64_t)row * D + k) = hi;
        if (out.np == 2) *reinterpret_cast<bf16x4*>(out.p + out.plane + (int64_t)row * D + k) = lo;
    }
}
int launch_layernorm_mod_planes(const float* h, const float* shift, const float* scale, int mod_ld, int rows, int D, int T, float eps,
                                Planes out, hipStream_t st) {
    if (D % 4 || D > 1024) VB_FAIL(VB_E_INVALID, "layernorm_mod_planes: D=%d", D);
    hipLaunchKernelGGL(layernorm_mod_planes_kernel, dim3(cdiv(rows, 4)), dim3(256), 0, st, h, shift, scale, mod_ld, rows, D, T > 0 ? T : 1, eps, out);
    VB_CHECK_LAUNCH();
    return VB_OK;
}

// A operand of the adaLN tabulation GEMM: row (step, sample) = silu(temb[step] + cemb[sample]) as split-bf16 planes
__global__ void __launch_bounds__(256) silu_sum_planes_kernel(const float* __restrict__ temb, const float* __restrict__ cemb, int rows,
                                                             int D, int nsample, bf16_t* out, int64_t plane) {
    const int64_t total = (int64_t)rows * (D / 4);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int r = (int)(i / (D / 4)), k = (int)(i - (int64_t)r * (D / 4)) * 4;
        const int step = r / nsample, smp = r - step * nsample;
        const float4 a = *reinterpret_cast<const float4*>(temb + (int64_t)step * D + k);
        const float4 b = *reinterpret_cast<const float4*>(cemb + (int64_t)smp * D + k);
        float v[4] = {a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w};
        bf16x4 hi, lo;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float sv = v[e] / (1.f + expf(-v[e]));          // same expression as the row-linear kernel's input activation
            hi[e] = f2bf(sv);
            lo[e] = f2bf(sv - bf2f(hi[e]));
        }
        *reinterpret_cast<bf16x4*>(out + (int64_t)r * D + k) = hi;
        *reinterpret_cast<bf16x4*>(out + plane + (int64_t)r * D + k) = lo;
    }
}
int launch_silu_sum_planes(const float* temb, const float* cemb, int rows, int D, int nsample, bf16_t* out, int64_t plane, hipStream_t st) {
    if (D % 4) VB_FAIL(VB_E_INVALID, "silu_sum_planes: D %% 4");
    int64_t blocks = ((int64_t)rows * (D / 4) + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(silu_sum_planes_kernel, dim3((int)blocks), dim3(256), 0, st, temb, cemb, rows, D, nsample, out, plane);
    VB_CHECK_LAUNCH();
    return VB_OK;
}

// out[i] = i / div   (row -> step index of the tabulated conditioning vectors)
__global__ void iota_div_kernel(int64_t* out, int n, int div) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = i / div;
}
int launch_iota_div(int64_t* out, int n, int div, hipStream_t st) {
    hipLaunchKernelGGL(iota_div_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, out, n, div);
    VB_CHECK_LAUNCH();
    return VB_OK;
}
