// T5 encoder helpers (gfx950): token-embedding gather and the self-attention of the text encoder.
// The encoder sees 80 tokens per caption: its projections are small GEMMs on the shared bf16x3 MFMA kernel; attention is
// 80 x 80 x 64 per (caption, head) - 0.4 MFLOP - so it runs as a plain fp32 kernel, one workgroup per (caption, head), with
// q, k, v of the head in LDS.  HF semantics (transformers T5Attention): scores = q k^T + position_bias, NO 1/sqrt(d) scaling,
// softmax in fp32, no mask (the reference passes none, ldm/modules/encoders/modules.py:221).
#include "engine.h"

__global__ void gather_rows_kernel(const int64_t* __restrict__ idx, const float* __restrict__ table, int rows, int D, int vocab, float* out) {
    const int r = blockIdx.x;
    int64_t id = idx[r];
    if (id < 0) id = 0;
    if (id >= vocab) id = vocab - 1;
    const float* src = table + id * D;
    for (int k = threadIdx.x * 4; k < D; k += blockDim.x * 4) *reinterpret_cast<float4*>(out + (int64_t)r * D + k) = *reinterpret_cast<const float4*>(src + k);
}
int launch_gather_rows(const int64_t* idx, const float* table, int rows, int D, int vocab, float* out, hipStream_t st) {
    if (D % 4) VB_FAIL(VB_E_INVALID, "gather_rows: D %% 4");
    hipLaunchKernelGGL(gather_rows_kernel, dim3(rows), dim3(256), 0, st, idx, table, rows, D, vocab, out);
    VB_CHECK_LAUNCH();
    return VB_OK;
}

#define T5_LMAX 128
#define T5_DKV 64
// qkv planes [B*L][3*heads*dkv] (q | k | v), out planes [B*L][heads*dkv]; block = (head, caption), 256 threads
__global__ void __launch_bounds__(256) t5_attn_kernel(Planes qkv, const float* __restrict__ pos_bias, int pos_len, int L, int heads,
                                                     Planes out) {
    __shared__ float qs[T5_LMAX][T5_DKV + 1], ks[T5_LMAX][T5_DKV + 1], vs[T5_LMAX][T5_DKV + 1];
    __shared__ float ps[4][T5_LMAX];
    const int h = blockIdx.x, b = blockIdx.y;
    const int inner = heads * T5_DKV, ld = 3 * inner;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int id = tid; id < L * T5_DKV; id += 256) {
        const int t = id / T5_DKV, d = id - t * T5_DKV;
        const int64_t base = ((int64_t)b * L + t) * ld + h * T5_DKV + d;
        float q = bf2f(qkv.p[base]), k = bf2f(qkv.p[base + inner]), v = bf2f(qkv.p[base + 2 * inner]);
        if (qkv.np == 2) { q += bf2f(qkv.p[qkv.plane + base]); k += bf2f(qkv.p[qkv.plane + base + inner]); v += bf2f(qkv.p[qkv.plane + base + 2 * inner]); }
        qs[t][d] = q; ks[t][d] = k; vs[t][d] = v;
    }
    __syncthreads();
    // one wave per query row (rows wave, wave+4, ...): lanes over keys (2 per lane up to 128), then over d for P.V
    for (int i = wave; i < L; i += 4) {
        float s[2];
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
            const int j = lane + 64 * jj;
            float acc = -INFINITY;
            if (j < L) {
                acc = 0.f;
                for (int d = 0; d < T5_DKV; ++d) acc += qs[i][d] * ks[j][d];
                acc += pos_bias[((int64_t)h * pos_len + i) * pos_len + j];
            }
            s[jj] = acc;
        }
        float m = fmaxf(s[0], s[1]);
        for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
        float p0 = (lane < L) ? expf(s[0] - m) : 0.f, p1 = (lane + 64 < L) ? expf(s[1] - m) : 0.f;
        float l = p0 + p1;
        for (int o = 32; o > 0; o >>= 1) l += __shfl_xor(l, o, 64);
        const float inv = 1.f / l;
        ps[wave][lane] = p0 * inv;
        ps[wave][lane + 64] = p1 * inv;
        __builtin_amdgcn_s_waitcnt(0xc07f);
        __builtin_amdgcn_wave_barrier();
        float o = 0.f;                               // lane = d
        for (int j = 0; j < L; ++j) o += ps[wave][j] * vs[j][lane];
        const int64_t oi = ((int64_t)b * L + i) * inner + h * T5_DKV + lane;
        const bf16_t hi = f2bf(o);
        out.p[oi] = hi;
        if (out.np == 2) out.p[out.plane + oi] = f2bf(o - bf2f(hi));
        __builtin_amdgcn_wave_barrier();
    }
}
int launch_t5_attention(Planes qkv, const float* pos_bias, int pos_len, int B, int L, int heads, int dkv, Planes out, hipStream_t st) {
    if (dkv != T5_DKV || L > T5_LMAX || L > pos_len || L < 1) VB_FAIL(VB_E_INVALID, "t5_attention: d_kv=%d L=%d (built for d_kv 64, L <= 128)", dkv, L);
    hipLaunchKernelGGL(t5_attn_kernel, dim3(heads, B), dim3(256), 0, st, qkv, pos_bias, pos_len, L, heads, out);
    VB_CHECK_LAUNCH();
    return VB_OK;
}

// ---- host driver: T5 text encoder ----------------------------------------------------------------------
struct T5Ws { float* h; bf16_t* nrm; bf16_t* qkv; bf16_t* att; bf16_t* ff; size_t total; };
static T5Ws carve_t5(void* base, const vb_t5_config& c, int B, int L) {
    T5Ws o;
    Carver cv(base);
    const size_t R = (size_t)B * L, inner = (size_t)c.heads * c.d_kv;
    o.h = cv.take<float>(R * c.d_model);
    o.nrm = cv.take<bf16_t>(2 * R * c.d_model);
    o.qkv = cv.take<bf16_t>(2 * R * 3 * inner);
    o.att = cv.take<bf16_t>(2 * R * inner);
    o.ff = cv.take<bf16_t>(2 * R * c.d_ff);
    o.total = cv.off;
    return o;
}
extern "C" {

int vb_t5_load(vb_ctx* ctx, const vb_t5_config* cfg, const vb_t5_weights* w) {
    if (!ctx || !cfg || !w) VB_FAIL(VB_E_INVALID, "t5_load: null argument");
    if (cfg->layers < 1 || cfg->layers > VB_T5_MAX_LAYERS) VB_FAIL(VB_E_INVALID, "t5_load: layers %d", cfg->layers);
    if (cfg->d_kv != 64) VB_FAIL(VB_E_INVALID, "t5_load: d_kv %d unsupported (attention kernel is built for 64)", cfg->d_kv);
    if (cfg->d_model % 64 || cfg->d_ff % 64 || cfg->d_model > 1024) VB_FAIL(VB_E_INVALID, "t5_load: d_model %d / d_ff %d", cfg->d_model, cfg->d_ff);
    ctx->t5cfg = *cfg;
    ctx->t5w = *w;
    ctx->t5_loaded = true;
    return VB_OK;
}
size_t vb_t5_workspace_bytes(const vb_t5_config* cfg, int B, int L) { return carve_t5(nullptr, *cfg, B, L).total; }
int vb_t5_encode(vb_ctx* ctx, const int64_t* ids, int B, int L, float* out, void* ws, void* stream) {
    if (!ctx || !ctx->t5_loaded) VB_FAIL(VB_E_STATE, "t5_encode: T5 not loaded");
    VB_HIP(hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    const vb_t5_config& c = ctx->t5cfg;
    const vb_t5_weights& w = ctx->t5w;
    if (L > w.pos_len) VB_FAIL(VB_E_INVALID, "t5_encode: L=%d exceeds the position-bias table (%d)", L, w.pos_len);
    T5Ws s = carve_t5(ws, c, B, L);
    const int R = B * L, D = c.d_model, inner = c.heads * c.d_kv;
    VB_TRY(launch_gather_rows(ids, w.embed, R, D, c.vocab, s.h, st));
    Planes nrm = mkp(s.nrm, (int64_t)R * D, 2), qkv = mkp(s.qkv, (int64_t)R * 3 * inner, 2), att = mkp(s.att, (int64_t)R * inner, 2);
    Planes ff = mkp(s.ff, (int64_t)R * c.d_ff, 2);
    for (int i = 0; i < c.layers; ++i) {
        const vb_t5_layer& lw = w.layers[i];
        // x += O(softmax(Q K^T + bias) V),  Q/K/V from T5LayerNorm(x)   (T5LayerSelfAttention)
        VB_TRY(launch_rmsnorm_mod(s.h, lw.ln0, nullptr, nullptr, 0, R, D, L, c.eps, nrm, st));
        GemmArgs g = gemm_operands(nrm.p, nrm.plane, D, lw.wqkv, (int64_t)3 * inner * D, D, R, 3 * inner, D, 3);
        g.epi = EPI_PLANES; g.out = qkv; g.ldc = 3 * inner;
        VB_TRY(launch_gemm(g, st));
        VB_TRY(launch_t5_attention(qkv, w.pos_bias, w.pos_len, B, L, c.heads, c.d_kv, att, st));
        g = gemm_operands(att.p, att.plane, inner, lw.wo, (int64_t)D * inner, inner, R, D, inner, 3);
        g.epi = EPI_RESID_GATE; g.out32 = s.h; g.ldc32 = D; g.gate = w.ones; g.gate_ld = 0; g.T = L;
        VB_TRY(launch_gemm(g, st));
        // x += Wo(gelu_new(Wi0 n) * Wi1 n),  n = T5LayerNorm(x)   (T5LayerFF, gated-gelu)
        VB_TRY(launch_rmsnorm_mod(s.h, lw.ln1, nullptr, nullptr, 0, R, D, L, c.eps, nrm, st));
        g = gemm_operands(nrm.p, nrm.plane, D, lw.wi, (int64_t)2 * c.d_ff * D, D, R, 2 * c.d_ff, D, 3);
        g.epi = EPI_GEGLU; g.out = ff; g.ldc = c.d_ff;
        VB_TRY(launch_gemm(g, st));
        g = gemm_operands(ff.p, ff.plane, c.d_ff, lw.wo_ff, (int64_t)D * c.d_ff, c.d_ff, R, D, c.d_ff, 3);
        g.epi = EPI_RESID_GATE; g.out32 = s.h; g.ldc32 = D; g.gate = w.ones; g.gate_ld = 0; g.T = L;
        VB_TRY(launch_gemm(g, st));
    }
    VB_TRY(launch_rmsnorm_mod(s.h, w.final_ln, nullptr, nullptr, 0, R, D, L, c.eps, nrm, st));
    VB_TRY(launch_planes_to_f32(nrm, (int64_t)R * D, out, st));
    return VB_OK;
}

}  // extern "C"
