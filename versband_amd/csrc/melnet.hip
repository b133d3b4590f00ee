// Log-mel front-end (gfx950) - MelNet.forward of the reference (preprocess/NAT_mel.py:42-86), SURVEY 8(f) N4.
//
//   y = clamp(wav, -1, 1); reflect-pad (n_fft - hop)/2 on both sides (+ n_fft/2 when center); STFT (window folded into the basis);
//   mag = sqrt(re^2 + im^2 + 1e-9); mel = basis @ mag; out = log10(max(mel, 1e-5)).
//
// n_fft is a multiple of the hop (1280 = 4 x 320), so frame t is the concatenation of hop-blocks t .. t+taps-1 of the padded
// signal and the windowed DFT of all frames is ONE convolution over hop-blocks: input X[c][j] = padded[j*hop + c] (hop "channels",
// T + taps - 1 blocks), taps = n_fft / hop, weights W[q][c][o] = window[q*hop + c] * {cos, -sin}(2 pi f (q*hop + c) / n_fft).
// It runs on the exact-fp32 MFMA convolution kernel (conv1d_f32.hip; 2*1282*1280 flop per frame = 4.9 GFLOP per 20 s clip - a
// few tens of microseconds of v_mfma_f32_32x32x2f32), output transposed [b][t][Co4] so that the tail reads a frame's spectrum
// contiguously.  Two small kernels sit either side: frames_kernel (clamp + reflect + de-interleave into hop channels through an
// LDS tile so that both the read and the write are coalesced) and mel_tail_kernel (magnitude into LDS, mel filterbank, log10).
#include "engine.h"

// X[b][c][j] = clamp(wav[b][r_L(r_L1(j*hop + c - pad2) - pad)]),  c < hop, j < J: the reference reflect-pads by `pad` (NAT_mel.py:71) and
// torch.stft(center=True) reflect-pads THAT signal (length L1 = L + 2 pad) by pad2 = n_fft/2 again - two reflections, not one of pad + pad2
// len (nullable; device [B] row lengths in samples): row b is a clip of Lb = len[b] samples at pitch L.  Both reflections turn round at the
// row's OWN end (L1 = Lb + 2 pad), the row has Jb = Tb + taps - 1 hop-blocks of its own, Tb = 1 + (Lb + 2 (pad + pad2) - taps * hop) / hop,
// blocks j >= Jb are exact zeros and wav[b][k >= Lb] is never loaded (the caller's padding may be NaN).  A workgroup wholly behind Jb
// stores its zeros before it loads anything.  Null: Lb = L, Jb = J - the same instructions on the same values.
#define FR_JT 16
__global__ void __launch_bounds__(256) frames_kernel(const float* __restrict__ wav, int L, int hop, int pad, int pad2, int J, float* __restrict__ X,
                                                     const int* __restrict__ len, int taps) {
    extern __shared__ __attribute__((aligned(16))) float tile[];     // [FR_JT][hop + 1]
    const int b = blockIdx.y, j0 = blockIdx.x * FR_JT;
    const int pitch = hop + 1;
    const float* w = wav + (int64_t)b * L;
    float* xb = X + (int64_t)b * hop * J;
    const int Lb = len ? len[b] : L;
    const int Jb = len ? (Lb + 2 * (pad + pad2) - taps * hop) / hop + taps : J;
    if (j0 >= Jb) {
        for (int id = threadIdx.x; id < FR_JT * hop; id += 256) {
            const int c = id / FR_JT, j = j0 + (id - c * FR_JT);
            if (j < J) xb[(int64_t)c * J + j] = 0.f;
        }
        return;
    }
    for (int id = threadIdx.x; id < FR_JT * hop; id += 256) {
        const int jj = id / hop, c = id - jj * hop;
        const int j = j0 + jj;
        float v = 0.f;
        if (j < Jb) {
            const int L1 = Lb + 2 * pad;
            int k = j * hop + c - pad2;
            if (k < 0) k = -k;
            if (k >= L1) k = 2 * (L1 - 1) - k;
            k -= pad;
            if (k < 0) k = -k;
            if (k >= Lb) k = 2 * (Lb - 1) - k;
            k = k < 0 ? 0 : (k >= Lb ? Lb - 1 : k);     // only reachable when a padding exceeds its signal, which the launcher rejects
            v = fminf(fmaxf(w[k], -1.f), 1.f);
        }
        tile[jj * pitch + c] = v;
    }
    __syncthreads();
    for (int id = threadIdx.x; id < FR_JT * hop; id += 256) {
        const int c = id / FR_JT, jj = id - c * FR_JT;
        const int j = j0 + jj;
        if (j < J) xb[(int64_t)c * J + j] = tile[jj * pitch + c];
    }
}
int launch_stft_frames(const float* wav, int B, int L, int hop, int pad, int pad2, int J, float* X, hipStream_t st, const int* len, int taps) {
    if (pad >= L || pad2 >= L + 2 * pad) VB_FAIL(VB_E_INVALID, "melnet: reflect padding %d (+ %d) needs more than %d samples", pad, pad2, L);
    if (len && taps < 1) VB_FAIL(VB_E_INVALID, "melnet: row lengths with taps = %d (n_fft / hop >= 1)", taps);
    const size_t lds = (size_t)FR_JT * (hop + 1) * sizeof(float);
    if (lds > 64 * 1024) VB_FAIL(VB_E_INVALID, "melnet: hop %d too large", hop);
    hipLaunchKernelGGL(frames_kernel, dim3(cdiv(J, FR_JT), B), dim3(256), lds, st, wav, L, hop, pad, pad2, J, X, len, taps);
    VB_CHECK_LAUNCH();
    return VB_OK;
}

// spec f32 [B][T][Co4] (re at [0, nb), im at [im_off, im_off + nb)); basisT f32 [nb][n_mels]; mel f32 [B][n_mels][T]
// block = MT_FT frames of one clip; threads = n_mels x 4 frame groups (4 frames each)
// tlen (nullable; device [B] row lengths in frames): row b has Tb = tlen[b] frames of its own; frames t >= Tb are stored as 0.0f (the
// zeros-behind-the-end rule, not log10(1e-5)) and their spectrum is not loaded; a workgroup wholly behind Tb only stores.  Null: Tb = T.
#define MT_FT 16
__global__ void mel_tail_kernel(const float* __restrict__ spec, int T, int Co4, int nb, int im_off, const float* __restrict__ basisT,
                                int n_mels, float* __restrict__ mel, const int* __restrict__ tlen) {
    extern __shared__ __attribute__((aligned(16))) float mag[];      // [nb][MT_FT]
    const int b = blockIdx.y, t0 = blockIdx.x * MT_FT;
    const int Tb = tlen ? tlen[b] : T;
    const int m = threadIdx.x % n_mels, fg = threadIdx.x / n_mels;      // blockDim = 4 * n_mels
    float* mb = mel + ((int64_t)b * n_mels + m) * T;
    if (t0 >= Tb) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int t = t0 + fg * 4 + i;
            if (t < T) mb[t] = 0.f;
        }
        return;
    }
    const float* sb = spec + ((int64_t)b * T + t0) * Co4;
    for (int id = threadIdx.x; id < MT_FT * nb; id += blockDim.x) {
        const int tt = id / nb, f = id - tt * nb;
        float v = 0.f;
        if (t0 + tt < Tb) {
            const float re = sb[(int64_t)tt * Co4 + f], im = sb[(int64_t)tt * Co4 + im_off + f];
            v = sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(re, re), __fmul_rn(im, im)), 1e-9f));     // spec.pow(2).sum(-1) + 1e-9, :76
        }
        mag[f * MT_FT + tt] = v;
    }
    __syncthreads();
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    for (int f = 0; f < nb; ++f) {
        const float w = basisT[(int64_t)f * n_mels + m];
        const float4 g = *reinterpret_cast<const float4*>(&mag[f * MT_FT + fg * 4]);
        a0 = fmaf(w, g.x, a0); a1 = fmaf(w, g.y, a1); a2 = fmaf(w, g.z, a2); a3 = fmaf(w, g.w, a3);
    }
    const float acc[4] = {a0, a1, a2, a3};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int t = t0 + fg * 4 + i;
        if (t < T) mb[t] = t < Tb ? log10f(fmaxf(acc[i], 1e-5f)) : 0.f;      // dynamic_range_compression_torch, :26-27
    }
}
int launch_mel_tail(const float* spec, int B, int T, int Co4, int nb, int im_off, const float* basisT, int n_mels, float* mel, hipStream_t st,
                    const int* tlen) {
    if (n_mels < 1 || n_mels * 4 > 1024) VB_FAIL(VB_E_INVALID, "melnet: n_mels %d (1..256)", n_mels);
    const size_t lds = (size_t)nb * MT_FT * sizeof(float);
    if (lds > 64 * 1024) VB_FAIL(VB_E_INVALID, "melnet: %d frequency bins do not fit the magnitude tile", nb);
    hipLaunchKernelGGL(mel_tail_kernel, dim3(cdiv(T, MT_FT), B), dim3(4 * n_mels), lds, st, spec, T, Co4, nb, im_off, basisT, n_mels, mel, tlen);
    VB_CHECK_LAUNCH();
    return VB_OK;
}

// Masked mean absolute distance of two log-mels (scripts/infer_batched.py --eval_mel; vb_mel_dist_lens): a [B][M][Ta], b [B][M][Tb],
// f (device [B]) frames to compare, 1 <= f[r] <= min(Ta, Tb).  With d = a - b over m < M, t < f[r] (N = M * f[r] elements, i = m * f[r] + t):
//     mu = remove_offset ? sum(d) / N : 0;   out[r] = sum(|d - mu|) / N;   out_offset[r] = mu
// One workgroup of MD_THREADS per row, two passes over the row, nothing behind f[r] is loaded (it may be NaN).  THE REDUCTION SHAPE, fixed:
// thread x adds its elements i = x, x + MD_THREADS, ... in ascending order into one fp32 accumulator that starts at 0 (ceil(N / MD_THREADS)
// additions at most), then an LDS tree of log2(MD_THREADS) = 10 levels, level s adding slot x + s to slot x for s = 512, 256, ... 1.  The
// longest chain of additions behind a sum is k = ceil(N / 1024) + 10.  No atomics and no second launch: the result is a pure function of the
// inputs, identical from run to run.
#define MD_THREADS 1024
__device__ __forceinline__ float md_block_sum(float v, float* red) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = MD_THREADS / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] = __fadd_rn(red[threadIdx.x], red[threadIdx.x + s]);
        __syncthreads();
    }
    const float r = red[0];
    __syncthreads();                                                 // (red is written again by the next pass)
    return r;
}
__global__ void __launch_bounds__(MD_THREADS) mel_dist_kernel(const float* __restrict__ a, int Ta, const float* __restrict__ b, int Tb, int M,
                                                              const int* __restrict__ frames, int remove_offset, float* __restrict__ out,
                                                              float* __restrict__ out_offset) {
    __shared__ float red[MD_THREADS];
    const int r = blockIdx.x, f = frames[r];
    const int N = M * f;
    const float* ar = a + (int64_t)r * M * Ta;
    const float* br = b + (int64_t)r * M * Tb;
    float mu = 0.f;
    if (remove_offset) {
        float acc = 0.f;
        for (int i = threadIdx.x; i < N; i += MD_THREADS) {
            const int m = i / f, t = i - m * f;
            acc = __fadd_rn(acc, __fsub_rn(ar[(int64_t)m * Ta + t], br[(int64_t)m * Tb + t]));
        }
        mu = md_block_sum(acc, red) / (float)N;
    }
    float acc = 0.f;
    for (int i = threadIdx.x; i < N; i += MD_THREADS) {
        const int m = i / f, t = i - m * f;
        acc = __fadd_rn(acc, fabsf(__fsub_rn(__fsub_rn(ar[(int64_t)m * Ta + t], br[(int64_t)m * Tb + t]), mu)));
    }
    const float sum = md_block_sum(acc, red);
    if (threadIdx.x == 0) {
        out[r] = sum / (float)N;
        if (out_offset) out_offset[r] = mu;
    }
}
int launch_mel_dist(const float* a, int Ta, const float* b, int Tb, int B, int M, const int* frames, int remove_offset, float* out, float* out_offset,
                    hipStream_t st) {
    if (B < 1 || M < 1 || Ta < 1 || Tb < 1 || (int64_t)M * std::min(Ta, Tb) > (1 << 30))
        VB_FAIL(VB_E_INVALID, "mel_dist: B=%d M=%d Ta=%d Tb=%d (all >= 1, M * min(Ta, Tb) <= 2^30)", B, M, Ta, Tb);
    hipLaunchKernelGGL(mel_dist_kernel, dim3(B), dim3(MD_THREADS), 0, st, a, Ta, b, Tb, M, frames, remove_offset, out, out_offset);
    VB_CHECK_LAUNCH();
    return VB_OK;
}

// ---- host driver: log-mel front-end ------------------------------------------------------------------------
static inline int mel_im_off(const vb_mel_config& c) { return (c.n_fft / 2 + 1 + 3) / 4 * 4; }
struct MelWs { float* X; float* spec; int T, J, pad, pad2; size_t total; };
static MelWs carve_mel(void* base, const vb_mel_config& c, int B, int L, int center) {
    MelWs o;
    Carver cv(base);
    o.pad = (c.n_fft - c.hop) / 2; o.pad2 = center ? c.n_fft / 2 : 0;
    const int pad = o.pad + o.pad2;
    o.T = L + 2 * pad >= c.n_fft ? 1 + (L + 2 * pad - c.n_fft) / c.hop : 0;
    o.J = o.T + c.n_fft / c.hop - 1;
    o.X = cv.take<float>((size_t)B * c.hop * o.J);
    o.spec = cv.take<float>((size_t)B * o.T * 2 * mel_im_off(c));
    o.total = cv.off;
    return o;
}
extern "C" {

int vb_melnet_load(vb_ctx* ctx, const vb_mel_config* cfg, const float* dft_w, const float* basis_t) {
    if (!ctx || !cfg || !dft_w || !basis_t) VB_FAIL(VB_E_INVALID, "melnet_load: null argument");
    if (cfg->hop < 1 || cfg->n_fft < cfg->hop || cfg->n_fft % cfg->hop || cfg->n_fft % 2 || (cfg->n_fft - cfg->hop) % 2)
        VB_FAIL(VB_E_INVALID, "melnet_load: n_fft %d must be an even multiple of the hop %d (and n_fft - hop even)", cfg->n_fft, cfg->hop);
    if (cfg->n_fft / cfg->hop - 1 > 64) VB_FAIL(VB_E_INVALID, "melnet_load: n_fft / hop = %d too large", cfg->n_fft / cfg->hop);
    if (cfg->n_mels < 1 || cfg->n_mels > 256) VB_FAIL(VB_E_INVALID, "melnet_load: n_mels %d", cfg->n_mels);
    ctx->melcfg = *cfg; ctx->mel_dft = dft_w; ctx->mel_basis_t = basis_t; ctx->mel_loaded = true;
    return VB_OK;
}
int vb_melnet_frames(const vb_mel_config* cfg, int L, int center) { return cfg ? carve_mel(nullptr, *cfg, 1, L, center).T : 0; }
size_t vb_melnet_workspace_bytes(const vb_mel_config* cfg, int B, int L, int center) { return cfg ? carve_mel(nullptr, *cfg, B, L, center).total : 0; }
int vb_melnet_forward(vb_ctx* ctx, const float* wav, int B, int L, int center, float* mel, float* spec, void* ws, void* stream) {
    if (!ctx || !ctx->mel_loaded) VB_FAIL(VB_E_STATE, "melnet_forward: front-end not loaded");
    if (!wav || !ws || (!mel && !spec) || B < 1) VB_FAIL(VB_E_INVALID, "melnet_forward: bad argument");
    VB_HIP(hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    const vb_mel_config& c = ctx->melcfg;
    MelWs s = carve_mel(ws, c, B, L, center);
    if (s.T < 1) VB_FAIL(VB_E_INVALID, "melnet_forward: %d samples (+ 2 x %d) are shorter than one %d-sample frame", L, s.pad + s.pad2, c.n_fft);
    const int nb = c.n_fft / 2 + 1, im_off = mel_im_off(c), Co4 = 2 * im_off;
    float* sp = spec ? spec : s.spec;
    VB_TRY(launch_stft_frames(wav, B, L, c.hop, s.pad, s.pad2, s.J, s.X, st));
    ConvArgs a;
    a.x = s.X; a.x_bstride = (int64_t)c.hop * s.J; a.Ci = c.hop; a.T_in = s.J; a.w = ctx->mel_dft; a.Co = Co4; a.ksize = c.n_fft / c.hop;
    a.dil = 1; a.pad = 0; a.out = sp; a.out_bstride = (int64_t)s.T * Co4; a.T_out = s.T; a.out_transposed = 1; a.B = B;
    VB_TRY(launch_conv1d(a, st));
    if (mel) VB_TRY(launch_mel_tail(sp, B, s.T, Co4, nb, im_off, ctx->mel_basis_t, c.n_mels, mel, st));
    return VB_OK;
}

// Row lengths (include/versband_hip.h): the plain call's workspace + the two length tables (samples for frames_kernel, frames for the tail
// pass over spec and mel_tail_kernel).  The STFT stays the ONE convolution over the padded J: row b's blocks behind J_b are zero, but the
// taps - 1 blocks before J_b are its last frames' and the frames t >= T_b still read them - so spec gets the nets' tail pass (net_run's
// call shape for a transposed output: one row of (T - T_b) * Co4 samples per clip) and is exactly zero behind T_b before mel_tail reads it.
size_t vb_melnet_lens_workspace_bytes(const vb_mel_config* cfg, int B, int L, int center) {
    return cfg ? carve_mel(nullptr, *cfg, B, L, center).total + 2 * align_up(64 * sizeof(int)) : 0;
}
int vb_melnet_forward_lens(vb_ctx* ctx, const float* wav, int B, int L, int center, const vb_lens* lens, float* mel, float* spec, void* ws,
                           void* stream) {
    LensPlan lp;
    if (lens && lens->len) VB_TRY(lens_plan(lens->len, B, L, &lp));
    if (!lp.B) return vb_melnet_forward(ctx, wav, B, L, center, mel, spec, ws, stream);      // no lengths, or every row full: the plain entry point
    if (!ctx || !ctx->mel_loaded) VB_FAIL(VB_E_STATE, "melnet_forward_lens: front-end not loaded");
    if (!wav || !ws || (!mel && !spec)) VB_FAIL(VB_E_INVALID, "melnet_forward_lens: bad argument");
    const vb_mel_config& c = ctx->melcfg;
    MelWs s = carve_mel(ws, c, B, L, center);
    LensPlan lt;                                                                             // row lengths in frames
    lt.B = B;
    for (int b = 0; b < B; ++b) {                                                            // what launch_stft_frames checks for the call, per row
        const int n = lp.len[b];
        if (s.pad >= n || s.pad2 >= n + 2 * s.pad)
            VB_FAIL(VB_E_INVALID, "melnet_forward_lens: row %d: reflect padding %d (+ %d) needs more than %d samples", b, s.pad, s.pad2, n);
        lt.len[b] = carve_mel(nullptr, c, 1, n, center).T;
        if (lt.len[b] < 1)
            VB_FAIL(VB_E_INVALID, "melnet_forward_lens: row %d: %d samples (+ 2 x %d) are shorter than one %d-sample frame", b, n, s.pad + s.pad2, c.n_fft);
    }
    VB_HIP(hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    int* table_n = reinterpret_cast<int*>(static_cast<char*>(ws) + s.total);
    int* table_t = reinterpret_cast<int*>(static_cast<char*>(ws) + s.total + align_up(64 * sizeof(int)));
    VB_TRY(launch_lens_table(lp, table_n, st));
    VB_TRY(launch_lens_table(lt, table_t, st));
    const int nb = c.n_fft / 2 + 1, im_off = mel_im_off(c), Co4 = 2 * im_off;
    float* sp = spec ? spec : s.spec;
    VB_TRY(launch_stft_frames(wav, B, L, c.hop, s.pad, s.pad2, s.J, s.X, st, table_n, c.n_fft / c.hop));
    ConvArgs a;
    a.x = s.X; a.x_bstride = (int64_t)c.hop * s.J; a.Ci = c.hop; a.T_in = s.J; a.w = ctx->mel_dft; a.Co = Co4; a.ksize = c.n_fft / c.hop;
    a.dil = 1; a.pad = 0; a.out = sp; a.out_bstride = (int64_t)s.T * Co4; a.T_out = s.T; a.out_transposed = 1; a.B = B;
    VB_TRY(launch_conv1d(a, st));
    VB_TRY(launch_tail_zero(sp, lt, table_t, B, 1, s.T, Co4, st));
    if (mel) VB_TRY(launch_mel_tail(sp, B, s.T, Co4, nb, im_off, ctx->mel_basis_t, c.n_mels, mel, st, table_t));
    return VB_OK;
}
size_t vb_mel_dist_workspace_bytes(int B) { return B >= 1 && B <= 64 ? align_up(64 * sizeof(int)) : 0; }
int vb_mel_dist_lens(const float* a, int Ta, const float* b, int Tb, int B, int M, const int32_t* frames, int remove_offset, float* out,
                     float* out_offset, void* ws, void* stream) {
    if (!a || !b || !out || !ws || M < 1 || Ta < 1 || Tb < 1) VB_FAIL(VB_E_INVALID, "mel_dist_lens: null pointer or M/Ta/Tb < 1");
    LensPlan lp;
    VB_TRY(lens_plan(frames, B, std::min(Ta, Tb), &lp));      // (B <= 64, 1 <= frames[b] <= min(Ta, Tb): the row is named)
    lp.B = B;                                                 // (full rows are rows like the others here)
    hipStream_t st = (hipStream_t)stream;
    VB_TRY(launch_lens_table(lp, static_cast<int*>(ws), st));
    return launch_mel_dist(a, Ta, b, Tb, B, M, static_cast<const int*>(ws), remove_offset, out, out_offset, st);
}

}  // extern "C"
