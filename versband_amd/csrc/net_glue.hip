// Glue kernels of the conv-net executor (gfx950), called by convnet.hip only (VAE, HiFi-GAN / BigVGAN, long-form windows): GroupNorm
// statistics and apply, the pre-activated transposed planes of the DMA-fed convs, the anti-aliased periodic activation, the split
// planes and the transposed softmax of the VAE attention, the cross-fade of long-form windows, and the VAE posterior with row lengths.
#include "kernels.h"

// ---------------------------------------------------------------------------
// GroupNorm statistics (autoencoder1d.py:165-166): one block per (b, group); the group's
// channels are contiguous in [B][C][T].  Two-pass mean / biased variance.
//
// One body, two instantiations that differ in indexing alone.  Plain: the group is one flat slab of n = C/groups * T samples, read as
// p[i], as float4 when n % 4 == 0 and the slab is 16-byte aligned.  LENS (row lengths, vb_vae_decode_lens): the group of row b is C/groups
// channel rows of L = len[b] * len_mul valid samples at pitch T, and valid sample i (flat, channel-major) of the compacted clip [C/groups][L]
// goes to the thread the plain form gives it - float4 group i / 4 to thread (i / 4) % 1024 exactly when the compacted slab would take that
// path (n % 4 == 0; its base is then 16-byte aligned in an aligned buffer), one float per thread otherwise.  A group of four inside one
// channel row is one 16-byte load when the row pieces are aligned (L % 4 == 0, T % 4 == 0), four 4-byte loads where it straddles two
// rows.  Nothing behind a row's end is read.  The arithmetic is the body's own, so row b's statistics are the plain form's on the clip
// alone, bit for bit.
// ---------------------------------------------------------------------------
#define GS_T 1024
template <bool LENS>
__global__ void __launch_bounds__(GS_T) gn_stats_kernel(const float* __restrict__ x, int C, int T, int groups, float eps,
                                                       const int* __restrict__ len, int len_mul, float* mean, float* rstd) {
    // Contraction is off and every fused multiply-add is spelled out, so that both instantiations round alike whatever the loads around
    // the arithmetic look like (tests/test_gpu_vae_lens.py holds the two to the same bits, and to those of the kernels before them).
#pragma clang fp contract(off)
    using idx_t = std::conditional_t<LENS, int, int64_t>;          // (LENS: the launcher keeps a group under 2^31 samples)
    __shared__ float red[GS_T / 64];
    __shared__ float s_mean;
    const int bg = blockIdx.x;
    const int cpg = C / groups;
    const int L = LENS ? len[bg / groups] * len_mul : T;
    const idx_t n = (idx_t)cpg * L;
    const float* p = x + (int64_t)bg * cpg * T;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool aligned = (reinterpret_cast<uintptr_t>(p) & 15) == 0;
    const bool vec = (n & 3) == 0 && (LENS || aligned);
    const bool quad = (L & 3) == 0 && (T & 3) == 0 && aligned;     // (LENS only)
    const idx_t n4 = vec ? n / 4 : 0;
    auto at = [&](idx_t i) -> float {
        if constexpr (LENS) { const int r = i / L; return p[(int64_t)r * T + (i - r * L)]; }
        else return p[i];
    };
    auto at4 = [&](idx_t i4) -> float4 {
        if constexpr (LENS) {
            const int i = 4 * i4;
            if (quad) { const int r = i / L; return *reinterpret_cast<const float4*>(p + (int64_t)r * T + (i - r * L)); }
            return make_float4(at(i), at(i + 1), at(i + 2), at(i + 3));
        } else {
            return reinterpret_cast<const float4*>(p)[i4];
        }
    };
    float s = 0.f;
    for (idx_t i = threadIdx.x; i < n4; i += GS_T) {
        const float4 v = at4(i);
        s += (v.x + v.y) + (v.z + v.w);
    }
    for (idx_t i = n4 * 4 + threadIdx.x; i < n; i += GS_T) s += at(i);
    s = wave_sum(s);
    if (lane == 0) red[wave] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = 0.f;
        for (int w = 0; w < GS_T / 64; ++w) t += red[w];
        s_mean = t / (float)n;
    }
    __syncthreads();
    const float m = s_mean;
    float v = 0.f;
    for (idx_t i = threadIdx.x; i < n4; i += GS_T) {
        const float4 q = at4(i);
        const float d0 = q.x - m, d1 = q.y - m, d2 = q.z - m, d3 = q.w - m;
        v += fmaf(d0, d0, d1 * d1) + fmaf(d2, d2, d3 * d3);
    }
    for (idx_t i = n4 * 4 + threadIdx.x; i < n; i += GS_T) { float d = at(i) - m; v = fmaf(d, d, v); }
    v = wave_sum(v);
    __syncthreads();
    if (lane == 0) red[wave] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = 0.f;
        for (int w = 0; w < GS_T / 64; ++w) t += red[w];
        mean[bg] = m;
        rstd[bg] = rsqrtf(t / (float)n + eps);
    }
}
int launch_gn_stats(const float* x, int B, int C, int T, int groups, float eps, float* mean, float* rstd, hipStream_t st, const int* len,
                    int len_mul) {
    if (C % groups) VB_FAIL(VB_E_INVALID, "gn_stats: C%%groups");
    if (len && (len_mul < 1 || (int64_t)(C / groups) * T >= (1ll << 31))) VB_FAIL(VB_E_INVALID, "gn_stats: len_mul < 1 or a group of 2^31 samples");
    hipLaunchKernelGGL(len ? gn_stats_kernel<true> : gn_stats_kernel<false>, dim3(B * groups), dim3(GS_T), 0, st, x, C, T, groups, eps, len, len_mul,
                       mean, rstd);
    VB_CHECK_LAUNCH();
    return VB_OK;
}

// GroupNorm affine (+ swish) applied once, for the wide VAE layers: the conv kernels can fuse it into their staging, but a
// layer with Co/128 output-channel tiles would then redo the exp/div of every input element Co/128 times
__global__ void __launch_bounds__(256) gn_apply_kernel(const float* __restrict__ x, const float* __restrict__ mean,
                                                      const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                      const float* __restrict__ beta, int C, int T, int groups, int swish, float* out,
                                                      const int* __restrict__ len, int len_mul) {
    const int row = blockIdx.y;                 // b * C + c
    const int b = row / C, c = row - b * C;
    const int L = len ? len[b] * len_mul : T;   // row lengths: the ACTIVATED tensor ends at the row's own length, zeros behind it
    const int grp = c / (C / groups);
    const float rs = rstd[b * groups + grp] * gamma[c];
    const float sh = beta[c] - mean[b * groups + grp] * rs;
    const float* xr = x + (int64_t)row * T;
    float* orow = out + (int64_t)row * T;
    for (int t = (blockIdx.x * 256 + threadIdx.x) * 4; t < T; t += gridDim.x * 1024) {
        if (t + 3 < T && (T & 3) == 0) {
            const float4 v = *reinterpret_cast<const float4*>(xr + t);
            float o[4] = {v.x * rs + sh, v.y * rs + sh, v.z * rs + sh, v.w * rs + sh};
            if (swish) {
#pragma unroll
                for (int k = 0; k < 4; ++k) o[k] = o[k] / (1.f + __expf(-o[k]));
            }
            if (t + 3 >= L) {
#pragma unroll
                for (int k = 0; k < 4; ++k) o[k] = t + k < L ? o[k] : 0.f;
            }
            *reinterpret_cast<float4*>(orow + t) = make_float4(o[0], o[1], o[2], o[3]);
        } else {
            for (int k = t; k < min(t + 4, T); ++k) {
                float o = xr[k] * rs + sh;
                if (swish) o = o / (1.f + __expf(-o));
                orow[k] = k < L ? o : 0.f;
            }
        }
    }
}
int launch_gn_apply(const float* x, const float* mean, const float* rstd, const float* gamma, const float* beta, int B, int C, int T,
                    int groups, int swish, float* out, hipStream_t st, const int* len, int len_mul) {
    if (C % groups) VB_FAIL(VB_E_INVALID, "gn_apply: C %% groups");
    hipLaunchKernelGGL(gn_apply_kernel, dim3(cdiv(T, 1024), B * C), dim3(256), 0, st, x, mean, rstd, gamma, beta, C, T, groups, swish, out, len,
                       len_mul);
    VB_CHECK_LAUNCH();
    return VB_OK;
}

// Pre-pass for wide conv layers: x f32 [B][C][T] -> activated, split-bf16, TRANSPOSED planes [2][B][Tp][C] (C contiguous), with
// XT_HEAD zero rows in front and zero rows behind (Tp = T_eff + XT_HEAD + XT_TAIL), so the conv kernel can DMA its input window
// straight into LDS: the pointwise transform (GroupNorm affine, swish, LeakyReLU), the hi/lo split, the transpose and the zero
// padding happen ONCE here instead of once per output-channel tile of the convolution (12 tiles on the 1536-channel layers).
// NPL == 1 (the single-pass bf16 convolutions): only the round-to-nearest plane [B][Tp][C] - plane 0 of the NPL == 2 form bit for bit;
// the rounding residual is neither computed nor stored.
template <int NPL>
__global__ void __launch_bounds__(256) xt_planes_kernel(const float* __restrict__ x, const float* __restrict__ mean, const float* __restrict__ rstd,
                                                       const float* __restrict__ gamma, const float* __restrict__ beta, int groups, int act,
                                                       float slope, int upsample2, int C, int T_in, int Tp, bf16_t* out, int64_t plane,
                                                       const int* __restrict__ len, int len_mul) {
    __shared__ float tile[64][65];
    const int b = blockIdx.z, c0 = blockIdx.y * 64, r0 = blockIdx.x * 64;          // r = row of the padded image
    // (row lengths: the activated image of row b ends at len[b] * len_mul positions - len_mul counts the upsampling - zero rows behind it)
    const int T_eff = len ? len[b] * len_mul : (upsample2 ? 2 * T_in : T_in);
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int cpg = groups > 0 ? C / groups : 1;
    {
        const int t = r0 + tx - XT_HEAD;
        const bool tin = t >= 0 && t < T_eff;
        const int ts = upsample2 ? (t >> 1) : t;
        for (int cc = ty; cc < 64; cc += 4) {
            const int c = c0 + cc;
            float v = 0.f;
            if (tin && c < C) {
                v = x[((int64_t)b * C + c) * T_in + ts];
                if (act == ACT_GN || act == ACT_GN_SWISH) {
                    const int grp = c / cpg;
                    const float rs = rstd[b * groups + grp] * gamma[c];
                    v = v * rs + (beta[c] - mean[b * groups + grp] * rs);
                    if (act == ACT_GN_SWISH) v = v / (1.f + __expf(-v));
                } else if (act == ACT_LRELU) {
                    v = v > 0.f ? v : v * slope;
                }
            }
            tile[tx][cc] = v;
        }
    }
    __syncthreads();
    const int tr = threadIdx.x >> 2, cg = (threadIdx.x & 3) * 16;
    const int r = r0 + tr;
    if (r < Tp && c0 + cg < C) {
        bf16x8 hi[2], lo[2];
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const float v = tile[tr][cg + e];
            const bf16_t h = f2bf(v);
            hi[e >> 3][e & 7] = h;
            if constexpr (NPL == 2) lo[e >> 3][e & 7] = f2bf(v - bf2f(h));
        }
        bf16_t* dst = out + ((int64_t)b * Tp + r) * C + c0 + cg;
        *reinterpret_cast<bf16x8*>(dst) = hi[0];
        *reinterpret_cast<bf16x8*>(dst + 8) = hi[1];
        if constexpr (NPL == 2) {
            *reinterpret_cast<bf16x8*>(dst + plane) = lo[0];
            *reinterpret_cast<bf16x8*>(dst + plane + 8) = lo[1];
        }
    }
}
int launch_xt_planes(const float* x, const float* mean, const float* rstd, const float* gamma, const float* beta, int groups, int act,
                     float slope, int upsample2, int B, int C, int T_in, int nplanes, bf16_t* out, hipStream_t st, const int* len, int len_mul) {
    if (C % 16) VB_FAIL(VB_E_INVALID, "xt_planes: C %% 16");
    if (nplanes != 1 && nplanes != 2) VB_FAIL(VB_E_INVALID, "xt_planes: %d planes (1 or 2)", nplanes);
    if (!aligned16(out)) VB_FAIL(VB_E_INVALID, "xt_planes: the planes are not 16-byte aligned");
    if ((act == ACT_GN || act == ACT_GN_SWISH) && (!mean || !rstd || !gamma || !beta || groups < 1 || C % groups))
        VB_FAIL(VB_E_INVALID, "xt_planes: GroupNorm input without its statistics / affine, or C %% groups");
    const int Tp = xt_rows(upsample2 ? 2 * T_in : T_in);
    const dim3 grid(cdiv(Tp, 64), cdiv(C, 64), B);
    if (nplanes == 1)
        hipLaunchKernelGGL(xt_planes_kernel<1>, grid, dim3(256), 0, st, x, mean, rstd, gamma, beta, groups, act, slope, upsample2, C, T_in, Tp, out,
                           (int64_t)0, len, len_mul);
    else
        hipLaunchKernelGGL(xt_planes_kernel<2>, grid, dim3(256), 0, st, x, mean, rstd, gamma, beta, groups, act, slope, upsample2, C, T_in, Tp, out,
                           (int64_t)B * Tp * C, len, len_mul);
    VB_CHECK_LAUNCH();
    return VB_OK;
}

// BigVGAN anti-aliased periodic activation (alias_free_torch Activation1d, ratio 2, 12-tap Kaiser-sinc filter f):
//   up[v]  = 2 * sum_i xp[i] f[v + 15 - 2 i]          xp = x replicate-padded by 5          (UpSample1d, resample.py:10-32)
//   s[v]   = up[v] + inv_beta * sin^2(alpha * up[v])                                         (Snake / SnakeBeta, activations.py)
//   out[t] = sum_k f[k] s[clamp(2 t + k - 5, 0, 2T-1)]                                       (DownSample1d / LowPassFilter1d)
// One workgroup = 256 outputs of one (batch, channel) row: the 523 intermediate samples are computed once into LDS.
// Row lengths (vb_bigvgan_forward_lens): row b = row / C ends at Tr = len[b] * len_mul samples of its pitch T, and the replicate padding
// of both filters starts there - the three bounds below (the fill of xs, the intermediate index, the store) are Tr instead of T, everything
// else is the one code of the plain form, so a row's valid samples are the bits of the plain kernel on that clip alone at T = Tr (the
// tiles start at multiples of 256 either way).  Nothing at or behind x[row][Tr] is loaded; out[row][Tr .. T) is written as exact zeros, by a
// workgroup whose tile lies wholly behind the row's end before it loads anything.  len == nullptr: Tr = T, the plain form.
#define AA_TT 256
__global__ void __launch_bounds__(256) aa_act_kernel(const float* __restrict__ x, const float* __restrict__ alpha, const float* __restrict__ inv_beta,
                                                    const float* __restrict__ filt, int C, int T, float* out, const int* __restrict__ len,
                                                    int len_mul) {
    __shared__ float xs[AA_TT + 16];
    __shared__ float ss[2 * AA_TT + 16];
    __shared__ float f[12];
    const int row = blockIdx.y, c = row % C;
    const int t0 = blockIdx.x * AA_TT;
    const float* xr = x + (int64_t)row * T;
    const int tid = threadIdx.x;
    const int Tr = len ? min(len[row / C] * len_mul, T) : T;        // (uniform over the workgroup)
    if (t0 >= Tr) {
        if (t0 + tid < T) out[(int64_t)row * T + t0 + tid] = 0.f;
        return;
    }
    if (tid < 12) f[tid] = filt[tid];
    for (int j = tid; j < AA_TT + 16; j += 256) {
        int pos = t0 - 6 + j;
        pos = pos < 0 ? 0 : (pos > Tr - 1 ? Tr - 1 : pos);
        xs[j] = xr[pos];
    }
    __syncthreads();
    const float a = alpha[c], ib = inv_beta[c];
    for (int q = tid; q < 2 * AA_TT + 11; q += 256) {
        int v = 2 * t0 - 5 + q;
        v = v < 0 ? 0 : (v > 2 * Tr - 1 ? 2 * Tr - 1 : v);
        const int i_lo = (v + 5) >> 1;                      // ceil((v + 4) / 2)
        float up = 0.f;
#pragma unroll
        for (int m = 0; m < 6; ++m) {
            const int i = i_lo + m;
            const int tap = v + 15 - 2 * i;                 // 11 - (v+5)%2 ... >= 0 by construction for m < 6
            if (tap >= 0 && tap < 12) up += xs[i - t0 + 1] * f[tap];
        }
        up *= 2.f;
        const float sn = sinf(up * a);
        ss[q] = up + ib * (sn * sn);
    }
    __syncthreads();
    const int t = t0 + tid;
    if (t < T) {
        float acc = 0.f;
        if (t < Tr) {
#pragma unroll
            for (int k = 0; k < 12; ++k) acc += f[k] * ss[2 * tid + k];
        }
        out[(int64_t)row * T + t] = acc;
    }
}
int launch_aa_act(const float* x, const float* alpha, const float* inv_beta, const float* filt, int B, int C, int T, float* out, hipStream_t st,
                  const int* len, int len_mul) {
    if (len && len_mul < 1) VB_FAIL(VB_E_INVALID, "aa_act: row lengths with len_mul = %d (>= 1)", len_mul);
    if (B < 1 || C < 1 || T < 1 || (int64_t)B * C > 65535 || T > (1 << 30))
        VB_FAIL(VB_E_INVALID, "aa_act: B=%d C=%d T=%d (B * C rows <= 65535, T <= 2^30)", B, C, T);
    hipLaunchKernelGGL(aa_act_kernel, dim3(cdiv(T, AA_TT), B * C), dim3(256), 0, st, x, alpha, inv_beta, filt, C, T, out, len, len_mul);
    VB_CHECK_LAUNCH();
    return VB_OK;
}

// f32 [rows][cols] -> split-bf16 planes [2][rows][cpad] (VB_OP_SPLIT_PLANES: per-batch weights of the VAE attention)
__global__ void split_rows_kernel(const float* __restrict__ x, int64_t rows, int cols, int cpad, bf16_t* out, int64_t plane) {
    const int q = cpad >> 2;
    const int64_t total = rows * q;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / q;
        const int c = (int)(i - r * q) * 4;
        float v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = (c + k < cols) ? x[r * cols + c + k] : 0.f;
        bf16x4 hi, lo;
#pragma unroll
        for (int k = 0; k < 4; ++k) { hi[k] = f2bf(v[k]); lo[k] = f2bf(v[k] - bf2f(hi[k])); }
        *reinterpret_cast<bf16x4*>(out + r * cpad + c) = hi;
        *reinterpret_cast<bf16x4*>(out + plane + r * cpad + c) = lo;
    }
}
int launch_split_rows(const float* x, int64_t rows, int cols, int cpad, bf16_t* out, int64_t plane, hipStream_t st) {
    if (cpad % 4 || cpad < cols) VB_FAIL(VB_E_INVALID, "split_rows: cpad=%d cols=%d", cpad, cols);
    int64_t blocks = (rows * (cpad / 4) + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(split_rows_kernel, dim3((int)blocks), dim3(256), 0, st, x, rows, cols, cpad, out, plane);
    VB_CHECK_LAUNCH();
    return VB_OK;
}

// softmax over the last dim of s[B][R][Cc], written transposed: out_t[b][c][r].  One body, two instantiations.  LENS (row lengths,
// vb_vae_decode_lens; Cc = R): s [B][R][R] holds row b's scores in its leading L x L block (L = len[b] * len_mul); query row r < L takes its
// softmax over the keys c < L with the lane stride and the order of the plain form at Cc = L, and everything outside the block of the
// transposed result - keys and queries behind the row's end - is written as exact zeros.  Nothing outside the block is read.
template <bool LENS>
__global__ void __launch_bounds__(256) softmax_rows_t_kernel(const float* __restrict__ s, int R, int Cc, const int* __restrict__ len, int len_mul,
                                                            float* out_t) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int b = blockIdx.y;
    const int lane = threadIdx.x & 63;
    if (row >= R) return;
    const int L = LENS ? len[b] * len_mul : Cc;                  // the keys of this row's softmax
    float* o = out_t + (int64_t)b * Cc * R + row;
    if (LENS && row >= L) {
        for (int c = lane; c < Cc; c += 64) o[(int64_t)c * R] = 0.f;
        return;
    }
    const float* p = s + ((int64_t)b * R + row) * Cc;
    float m = -INFINITY;
    for (int c = lane; c < L; c += 64) m = fmaxf(m, p[c]);
    m = wave_max(m);
    float sum = 0.f;
    for (int c = lane; c < L; c += 64) sum += expf(p[c] - m);
    sum = wave_sum(sum);
    const float inv = 1.f / sum;
    for (int c = lane; c < L; c += 64) o[(int64_t)c * R] = expf(p[c] - m) * inv;
    if (LENS)
        for (int c = L + lane; c < Cc; c += 64) o[(int64_t)c * R] = 0.f;
}
int launch_softmax_rows_t(const float* s, int B, int R, int Ccols, float* out_t, hipStream_t st, const int* len, int len_mul) {
    if (len && (len_mul < 1 || Ccols != R)) VB_FAIL(VB_E_INVALID, "softmax_rows_t: len_mul < 1, or row lengths on scores that are not square");
    hipLaunchKernelGGL(len ? softmax_rows_t_kernel<true> : softmax_rows_t_kernel<false>, dim3(cdiv(R, 4), B), dim3(256), 0, st, s, R, Ccols, len,
                       len_mul, out_t);
    VB_CHECK_LAUNCH();
    return VB_OK;
}


// ---------------------------------------------------------------------------
// long-form generation (BASELINE configs[4], build-defined: versband_amd/longform.py): cross-fade of the window results
//   out[b][c][t] = sum_w wgt_w(t) * parts[w*B + b][c][t - s_w] / sum_w wgt_w(t)
// wgt = 1 inside a window, linear ramps (k+1)/(ov+1) over the overlap with the previous window and 1 - (k+1)/(ov+1) over the overlap
// with the next one (the interior points of linspace(0, 1, ov + 2)), the minimum of the two where both apply - window order and
// arithmetic of longform.crossfade_windows (the torch restatement the oracle fixture was generated with).
// ---------------------------------------------------------------------------
struct XfadeStarts { int s[64]; };
__global__ void __launch_bounds__(256) crossfade_windows_kernel(const float* __restrict__ parts, XfadeStarts st, int nw, int B, int C, int n, int T,
                                                                float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)B * C * T) return;
    const int t = (int)(i % T);
    const int64_t bc = i / T;
    const int b = (int)(bc / C), c = (int)(bc - (int64_t)b * C);
    float acc = 0.f, wsum = 0.f;
    for (int w = 0; w < nw; ++w) {
        const int s = st.s[w], u = t - s;
        if (u < 0 || u >= n) continue;
        float wt = 1.f;
        if (w > 0) {
            const int ov = st.s[w - 1] + n - s;
            if (ov > 0 && u < ov) wt = (float)(u + 1) / (float)(ov + 1);
        }
        if (w + 1 < nw) {
            const int ov = s + n - st.s[w + 1];
            if (ov > 0 && u >= n - ov) wt = fminf(wt, 1.f - (float)(u - (n - ov) + 1) / (float)(ov + 1));
        }
        acc += parts[(((int64_t)w * B + b) * C + c) * n + u] * wt;
        wsum += wt;
    }
    out[i] = acc / wsum;
}
int launch_crossfade_windows(const float* parts, const int* starts, int nw, int B, int C, int n, int T, float* out, hipStream_t st) {
    if (nw < 1 || nw > 64) VB_FAIL(VB_E_INVALID, "crossfade: %d windows (1..64)", nw);
    XfadeStarts xs;
    for (int w = 0; w < 64; ++w) xs.s[w] = w < nw ? starts[w] : 0;
    for (int w = 0; w < nw; ++w)
        if (xs.s[w] < 0 || xs.s[w] + n > T || (w > 0 && (xs.s[w] <= xs.s[w - 1] || xs.s[w] > xs.s[w - 1] + n)))
            VB_FAIL(VB_E_INVALID, "crossfade: window %d at %d (length %d) does not continue the cover of [0, %d)", w, xs.s[w], n, T);
    if (xs.s[0] != 0 || xs.s[nw - 1] + n != T) VB_FAIL(VB_E_INVALID, "crossfade: the windows do not cover [0, %d)", T);
    const int64_t tot = (int64_t)B * C * T;
    hipLaunchKernelGGL(crossfade_windows_kernel, dim3(cdiv(tot, 256)), dim3(256), 0, st, parts, xs, nw, B, C, n, T, out);
    VB_CHECK_LAUNCH();
    return VB_OK;
}

// ---------------------------------------------------------------------------
// The VAE posterior with row lengths (vb_posterior_lens; DiagonalGaussianDistribution.sample / .mode followed by the scale of
// get_first_stage_encoding, cfm1_audio.py): moments [B][2E][T], mean = channels [0, E), logvar = channels [E, 2E), in fp32
//   z[b][c][t] = scale * (mean + expf(0.5f * clamp(logvar, -30, 20)) * noise)   t <  len[b]      (NOISE = false: scale * mean)
//   z[b][c][t] = 0                                                              t >= len[b]
// The zero tail of the moments is logvar = 0, std = 1: the elementwise path would leave the noise in z's padding, so the tail is a select
// here and neither the noise nor the moments are loaded behind a row's end (they may hold NaN).  grid = (pieces of a row, E, B), the
// lengths by value in the argument block (lp.B = 0: full rows).  VEC: one float4 per lane (T % 4 == 0 and 16-byte bases, the host checked);
// the group a row ends in takes 4-byte loads of its own samples.  Contraction is off: product, sum and scale round one by one, as written.
// ---------------------------------------------------------------------------
template <bool NOISE>
__device__ __forceinline__ float posterior_value(float mean, float logvar, float eps, float scale) {
#pragma clang fp contract(off)
    if constexpr (!NOISE) return scale * mean;
    const float sd = expf(0.5f * fminf(fmaxf(logvar, -30.f), 20.f));
    return scale * (mean + sd * eps);
}
template <bool VEC, bool NOISE>
__global__ void __launch_bounds__(256) posterior_lens_kernel(const float* __restrict__ mom, const float* __restrict__ noise, const LensPlan lp, int E,
                                                            int T, float scale, float* __restrict__ z) {
    const int b = blockIdx.z, c = blockIdx.y;
    const int t = (blockIdx.x * 256 + threadIdx.x) * (VEC ? 4 : 1);
    if (t >= T) return;
    const int L = lp.B ? lp.len[b] : T;
    const float* mp = mom + ((int64_t)b * 2 * E + c) * T + t;
    const float* vp = mp + (int64_t)E * T;
    const float* np = NOISE ? noise + ((int64_t)b * E + c) * T + t : nullptr;
    float* zp = z + ((int64_t)b * E + c) * T + t;
    if constexpr (VEC) {
        float o[4] = {0.f, 0.f, 0.f, 0.f};
        if (t + 4 <= L) {
            const float4 m = *reinterpret_cast<const float4*>(mp);
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f), n = v;
            if constexpr (NOISE) { v = *reinterpret_cast<const float4*>(vp); n = *reinterpret_cast<const float4*>(np); }
            o[0] = posterior_value<NOISE>(m.x, v.x, n.x, scale); o[1] = posterior_value<NOISE>(m.y, v.y, n.y, scale);
            o[2] = posterior_value<NOISE>(m.z, v.z, n.z, scale); o[3] = posterior_value<NOISE>(m.w, v.w, n.w, scale);
        } else {
#pragma unroll
            for (int k = 0; k < 3; ++k)
                if (t + k < L) o[k] = posterior_value<NOISE>(mp[k], NOISE ? vp[k] : 0.f, NOISE ? np[k] : 0.f, scale);
        }
        *reinterpret_cast<float4*>(zp) = make_float4(o[0], o[1], o[2], o[3]);
    } else {
        *zp = t < L ? posterior_value<NOISE>(*mp, NOISE ? *vp : 0.f, NOISE ? *np : 0.f, scale) : 0.f;
    }
}
int launch_posterior_lens(const float* moments, const float* noise, int B, int E, int T, const LensPlan& lp, float scale, float* z, hipStream_t st) {
    if (B < 1 || B > 65535 || E < 1 || E > 65535 || T < 1 || (lp.B && lp.B != B))
        VB_FAIL(VB_E_INVALID, "posterior_lens: B=%d E=%d T=%d with %d lengths (B, E in 1..65535, T >= 1, one length per row)", B, E, T, lp.B);
    const bool vec = T % 4 == 0 && aligned16(moments) && aligned16(z) && (!noise || aligned16(noise));
    const dim3 grid(cdiv(T, vec ? 1024 : 256), E, B);
    auto go = [&](auto kernel) { hipLaunchKernelGGL(kernel, grid, dim3(256), 0, st, moments, noise, lp, E, T, scale, z); };
    if (vec) { if (noise) go(posterior_lens_kernel<true, true>); else go(posterior_lens_kernel<true, false>); }
    else { if (noise) go(posterior_lens_kernel<false, true>); else go(posterior_lens_kernel<false, false>); }
    VB_CHECK_LAUNCH();
    return VB_OK;
}

// ---------------------------------------------------------------------------
// chunked vocoder with row lengths (vb_hifigan_forward_chunked_lens): one gather and one scatter per chunk.  Both are copies with a
// select: grid = (pieces of a row, channels, rows), one float4 (VEC) or one float per lane, the rows' indices and lengths by value.
// ---------------------------------------------------------------------------
template <bool VEC>
__global__ void __launch_bounds__(256) chunk_gather_kernel(const float* __restrict__ mel, const ChunkRows cr, int C, int T, int lo, int tc,
                                                           float* __restrict__ out) {
    const int j = blockIdx.z, c = blockIdx.y;
    const int t = (blockIdx.x * 256 + threadIdx.x) * (VEC ? 4 : 1);
    if (t >= tc) return;
    const int n = cr.n[j];
    const float* src = mel + ((int64_t)cr.row[j] * C + c) * T + lo + t;
    float* dst = out + ((int64_t)j * C + c) * tc + t;
    if constexpr (VEC) {
        // (tc % 4 == 0: the four frames lie inside the chunk; the row's own end may fall among them)
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (t + 4 <= n) v = *reinterpret_cast<const float4*>(src);
        else if (t < n) {
            v.x = src[0];
            if (t + 1 < n) v.y = src[1];
            if (t + 2 < n) v.z = src[2];
        }
        *reinterpret_cast<float4*>(dst) = v;
    } else {
        *dst = t < n ? *src : 0.f;
    }
}
int launch_chunk_gather(const float* mel, const ChunkRows& cr, int C, int T, int lo, int tc, float* out, hipStream_t st) {
    if (cr.n_active < 1 || cr.n_active > 64 || C < 1 || C > 65535 || lo < 0 || tc < 1 || lo + tc > T)
        VB_FAIL(VB_E_INVALID, "chunk_gather: %d rows, C=%d, frames [%d, %d) of %d", cr.n_active, C, lo, lo + tc, T);
    for (int j = 0; j < cr.n_active; ++j)
        if (cr.row[j] < 0 || cr.n[j] < 1 || cr.n[j] > tc) VB_FAIL(VB_E_INVALID, "chunk_gather: compact row %d = clip %d with %d of %d frames", j, cr.row[j], cr.n[j], tc);
    const bool vec = aligned16(mel) && aligned16(out) && T % 4 == 0 && lo % 4 == 0 && tc % 4 == 0;
    const dim3 grid(cdiv(tc, vec ? 1024 : 256), C, cr.n_active);
    if (vec) hipLaunchKernelGGL(chunk_gather_kernel<true>, grid, dim3(256), 0, st, mel, cr, C, T, lo, tc, out);
    else hipLaunchKernelGGL(chunk_gather_kernel<false>, grid, dim3(256), 0, st, mel, cr, C, T, lo, tc, out);
    VB_CHECK_LAUNCH();
    return VB_OK;
}
template <bool VEC>
__global__ void __launch_bounds__(256) chunk_scatter_kernel(const float* __restrict__ src, const ChunkScatter cs, int C, int64_t Tw, int64_t off_w,
                                                            int nw, int64_t Ts, int64_t off_s, float* __restrict__ wav) {
    // Tw / Ts: row pitch of wav / src in samples; off_w / off_s: where the chunk's kept samples start in a row of each; nw: how many
    const int b = blockIdx.z, c = blockIdx.y;
    const int i = (blockIdx.x * 256 + threadIdx.x) * (VEC ? 4 : 1);
    if (i >= nw) return;
    const int slot = cs.slot[b];
    const int keep = slot < 0 ? 0 : cs.keep[b];        // samples of this row's own; VEC: a multiple of 4 like i and nw (hop % 4 == 0)
    float* dst = wav + ((int64_t)b * C + c) * Tw + off_w + i;
    if constexpr (VEC) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (i < keep) v = *reinterpret_cast<const float4*>(src + ((int64_t)slot * C + c) * Ts + off_s + i);
        *reinterpret_cast<float4*>(dst) = v;
    } else {
        *dst = i < keep ? src[((int64_t)slot * C + c) * Ts + off_s + i] : 0.f;
    }
}
int launch_chunk_scatter(const float* src, const ChunkScatter& cs, int B, int C, int T, int hop, int s, int e, int lo, int tc, float* wav,
                         hipStream_t st) {
    if (B < 1 || B > 64 || C < 1 || C > 65535 || hop < 1 || lo < 0 || lo > s || s >= e || e > T || tc < 0
        || (int64_t)(e - s) * hop > INT32_MAX)
        VB_FAIL(VB_E_INVALID, "chunk_scatter: B=%d C=%d hop=%d, frames [%d, %d) of %d from a chunk at [%d, %d)", B, C, hop, s, e, T, lo, lo + tc);
    ChunkScatter k = cs;                               // keep: frames -> samples
    for (int b = 0; b < B; ++b) {
        if (k.slot[b] >= k.n_active || k.n_active > 64 || k.keep[b] > e - s || (k.slot[b] >= 0 && k.keep[b] > 0 && s - lo + k.keep[b] > tc)) VB_FAIL(VB_E_INVALID, "chunk_scatter: row %d keeps %d frames of %d from compact row %d", b, k.keep[b], e - s, k.slot[b]);
        k.keep[b] = k.slot[b] < 0 || k.keep[b] < 0 ? 0 : k.keep[b] * hop;
    }
    const int nw = (e - s) * hop;
    const bool vec = aligned16(src) && aligned16(wav) && hop % 4 == 0;
    const dim3 grid(cdiv(nw, vec ? 1024 : 256), C, B);
    const int64_t Tw = (int64_t)T * hop, Ts = (int64_t)tc * hop, off_w = (int64_t)s * hop, off_s = (int64_t)(s - lo) * hop;
    if (vec) hipLaunchKernelGGL(chunk_scatter_kernel<true>, grid, dim3(256), 0, st, src, k, C, Tw, off_w, nw, Ts, off_s, wav);
    else hipLaunchKernelGGL(chunk_scatter_kernel<false>, grid, dim3(256), 0, st, src, k, C, Tw, off_w, nw, Ts, off_s, wav);
    VB_CHECK_LAUNCH();
    return VB_OK;
}
