// C-ABI wrappers of single kernels (tests, tools and the parity harness call them; the engines do not).
#include "engine.h"

extern "C" {

int vb_rmsnorm_modulate(const float* h, const float* w, const float* shift, const float* scale, int mod_ld, int rows, int D, int T,
                        float eps, void* out_planes, int np, void* stream) {
    return launch_rmsnorm_mod(h, w, shift, scale, mod_ld, rows, D, T, eps, mkp((bf16_t*)out_planes, (int64_t)rows * D, np),
                              (hipStream_t)stream);
}
int vb_router_top1(const float* logits, const float* gumbel, int N, int E, int32_t* idx, void* stream) {
    return launch_router_top1(logits, gumbel, N, E, idx, (hipStream_t)stream);
}
int vb_route_bucket_scratch_ints(int N, int E) { return bucket_scratch_ints(N, E); }
int vb_route_bucket_pairs(const int32_t* ic, const int32_t* ia, int N, int E, int32_t* group_off, int32_t* perm, int32_t* pair_off,
                          int32_t* pair_pa, void* stream) {
    if (!pair_off || !pair_pa) VB_FAIL(VB_E_INVALID, "route_bucket_pairs: null pair outputs");
    return launch_bucket(ic, ia, N, E, group_off, perm, (hipStream_t)stream, pair_off, pair_pa);
}
int vb_route_bucket(const int32_t* ic, const int32_t* ia, int N, int E, int32_t* group_off, int32_t* perm, void* stream) {
    return launch_bucket(ic, ia, N, E, group_off, perm, (hipStream_t)stream);
}
int vb_gemm_bf16(const void* A, const void* Bw, const float* bias, int M, int N, int K, int np, float* C, void* stream) {
    GemmArgs g = gemm_operands(A, (int64_t)M * K, K, Bw, (int64_t)N * K, K, M, N, K, np == 2 ? 3 : 1);
    g.epi = EPI_F32; g.bias = bias; g.out32 = C; g.ldc32 = N;
    return launch_gemm(g, (hipStream_t)stream);
}
int vb_grouped_swiglu(const void* u, const int32_t* perm, const int32_t* group_off, int G, int n_slots, const void* w13,
                      const void* w2, const float* row_scale, int D, int H, int np, void* hidden, float* out, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    const int nseg = np == 2 ? 3 : 1;
    GemmArgs g = gemm_operands(u, (int64_t)n_slots * D, D, w13, (int64_t)G * 2 * H * D, D, n_slots, 2 * H, D, nseg);
    g.a_rows = perm; g.b_group_stride = (int64_t)2 * H * D; g.ngroups = G; g.group_off = group_off;
    g.epi = EPI_SWIGLU; g.out = mkp((bf16_t*)hidden, (int64_t)n_slots * H, np); g.ldc = H;
    VB_TRY(launch_gemm(g, st));
    g = gemm_operands(hidden, (int64_t)n_slots * H, H, w2, (int64_t)G * D * H, H, n_slots, D, H, nseg);
    g.b_group_stride = (int64_t)D * H; g.ngroups = G; g.group_off = group_off;
    g.epi = EPI_SCATTER_F32; g.out32 = out; g.ldc32 = D; g.rows_out = perm; g.row_scale = row_scale;
    return launch_gemm(g, st);
}
int vb_band_ffn(const void* y, int ldy, const void* w13, const void* w2, int M, int H, int E, int band, const float* gate, int gate_ld, int T,
                float* out32, int ldc32, void* stream) {
    if (!y || !w13 || !w2 || !gate || !out32 || M < 1 || H < 1 || E < 1 || band < 1 || T < 1) VB_FAIL(VB_E_INVALID, "band_ffn: null pointer or M/H/E/band/T < 1");
    if (ldy < E * band || ldc32 < E * band || gate_ld < E * band || ldy % 8 || ldc32 % 4 || gate_ld % 4)
        VB_FAIL(VB_E_INVALID, "band_ffn: ldy/ldc32/gate_ld must hold E*band columns (ldy %% 8, ldc32 %% 4, gate_ld %% 4 == 0)");
    BandFfnArgs bf;
    bf.y = (const bf16_t*)y; bf.ldy = ldy; bf.w13 = (const bf16_t*)w13; bf.w2 = (const bf16_t*)w2; bf.M = M; bf.H = H; bf.E = E;
    bf.band = band; bf.out32 = out32; bf.ldc32 = ldc32; bf.gate = gate; bf.gate_ld = gate_ld; bf.T = T;
    return launch_band_ffn(bf, (hipStream_t)stream);
}
int vb_routed_ffn_pair(const void* u, const int32_t* perm, const int32_t* group_off, const int32_t* pair_off, const int32_t* pair_pa, const void* w13,
                       const void* w2, const float* mc, const float* ma, int N, int D, int H, int E, void* hidden, void* out, void* stream) {
    if (!u || !perm || !group_off || !pair_off || !pair_pa || !w13 || !w2 || !mc || !ma || !hidden || !out || N < 1 || D < 1 || H < 1 || E < 1)
        VB_FAIL(VB_E_INVALID, "routed_ffn_pair: null pointer or N/D/H/E < 1");
    hipStream_t st = (hipStream_t)stream;
    GemmArgs g = gemm_operands(u, (int64_t)N * D, D, w13, (int64_t)2 * E * 2 * H * D, D, 2 * N, 2 * H, D, 1);
    g.a_rows = perm; g.b_group_stride = (int64_t)2 * H * D; g.ngroups = 2 * E; g.group_off = group_off;
    g.epi = EPI_SWIGLU; g.out = mkp((bf16_t*)hidden, (int64_t)2 * N * H, 1); g.ldc = H;
    g.row_scale = mc; g.row_scale2 = ma; g.scale_split = N;
    VB_TRY(launch_gemm(g, st));
    MoeW2PairArgs pw;
    pw.Hs = (const bf16_t*)hidden; pw.W2 = (const bf16_t*)w2; pw.pair_off = pair_off; pw.perm = perm; pw.pair_pa = pair_pa;
    pw.out = (bf16_t*)out; pw.N = N; pw.D = D; pw.H = H; pw.E = E;
    return launch_moe_w2_pair(pw, st);
}
int vb_caption_gate(const void* x, const void* keys, const float* score_bias, const float* vw, const float* bg, const float* la, int la_rows,
                    const float* hl, int hl_ld, const float* g1, const float* g2, const float* g3, uint64_t seed, int64_t clip_base, int nfe,
                    int block, int Beff, int B, int T, int K, int NS, int Hh, int E, int form, float* scores, int32_t* clip_off, int32_t* ic,
                    int32_t* ia, float* mc, float* ma, float* lc_out, int32_t* cnt, int cnt_G, int cnt_pairs, void* stream) {
    if (!x || !keys || !score_bias || !vw || !bg || !la || !hl || !ic || !ia || !mc || !ma || Beff < 1 || B < 1 || T < 1 || K < 1 || NS < 1 ||
        Hh < 1 || E < 1 || la_rows < 1 || hl_ld < 2)
        VB_FAIL(VB_E_INVALID, "caption_gate: null pointer or a size < 1");
    if ((g1 || g2 || g3) && !(g1 && g2 && g3)) VB_FAIL(VB_E_INVALID, "caption_gate: injected noise needs g1, g2 and g3");
    if (cnt && cnt_G != (cnt_pairs ? E * E : 2 * E)) VB_FAIL(VB_E_INVALID, "caption_gate: cnt_G=%d does not match E=%d pairs=%d", cnt_G, E, cnt_pairs);
    hipStream_t st = (hipStream_t)stream;
    const int N = Beff * T;
    ScoreRouterArgs sr;
    sr.A = (const bf16_t*)x; sr.lda = K; sr.Bm = (const bf16_t*)keys; sr.ldb = K; sr.bias = score_bias; sr.K = K; sr.Beff = Beff;
    RouterDev& r = sr.r;
    r.Wg = vw; r.bg = bg; r.la = la; r.la_rows = la_rows; r.hl = hl; r.hl_ld = hl_ld; r.g1 = g1; r.g2 = g2; r.g3 = g3; r.T = T; r.E = E; r.B = B;
    r.ic = ic; r.ia = ia; r.mc = mc; r.ma = ma; r.seed = seed; r.clip_base = clip_base; r.nfe_base = nfe; r.block = block; r.NS = NS; r.Hh = Hh;
    r.cnt = cnt; r.cnt_G = cnt_G; r.cnt_pairs = cnt_pairs;
    if (form == 1) {
        if (!gate_route_supported(NS, K, E, Hh)) VB_FAIL(VB_E_INVALID, "caption_gate: form 1 does not support NS=%d K=%d E=%d heads=%d", NS, K, E, Hh);
        if (lc_out) VB_FAIL(VB_E_INVALID, "caption_gate: form 1 writes no logits");
        return launch_gate_route(sr, st);
    }
    if (form != 0) VB_FAIL(VB_E_INVALID, "caption_gate: form %d", form);
    if (!scores || !clip_off) VB_FAIL(VB_E_INVALID, "caption_gate: form 0 needs the [N][NS] score scratch and the [Beff + 1] clip offsets");
    VB_TRY(launch_iota_mul(clip_off, Beff + 1, T, st));
    GemmArgs g = gemm_operands(x, (int64_t)N * K, K, keys, (int64_t)Beff * NS * K, K, N, NS, K, 1);
    g.b_group_stride = (int64_t)NS * K; g.ngroups = Beff; g.group_off = clip_off; g.group_rows = T;
    g.epi = EPI_F32; g.bias = score_bias; g.bias_group_stride = NS; g.out32 = scores; g.ldc32 = NS;
    VB_TRY(launch_gemm(g, st));
    r.N = N; r.D = K; r.sc = scores; r.lc_out = lc_out;
    return launch_router(r, st);
}
int vb_qkv_rope(const void* u, const void* wqkv, const float* rope_cos, const float* rope_sin, int B, int T, int Tpad, int H, int hd, int np,
                void* q, void* k, void* vt, void* stream) {
    if (!u || !wqkv || !rope_cos || !rope_sin || !q || !k || !vt || B < 1 || T < 1 || H < 1 || hd < 2 || Tpad < T || (np != 1 && np != 2))
        VB_FAIL(VB_E_INVALID, "qkv_rope: null pointer, B/T/H < 1, hd < 2, Tpad < T or np not 1 / 2");
    const int D = H * hd, N = B * T;
    const int64_t ND = (int64_t)N * D;
    GemmArgs g = gemm_operands(u, ND, D, wqkv, (int64_t)3 * D * D, D, N, 3 * D, D, np == 2 ? 3 : 1);
    g.epi = EPI_QKV_ROPE; g.q = mkp((bf16_t*)q, ND, np); g.k = mkp((bf16_t*)k, ND, np); g.vt = mkp((bf16_t*)vt, (int64_t)B * D * Tpad, np);
    g.rope_cos = rope_cos; g.rope_sin = rope_sin; g.H = H; g.hd = hd; g.Tpad = Tpad; g.D = D; g.T = T;
    return launch_gemm(g, (hipStream_t)stream);
}
int vb_attention(const void* q, const void* k, const void* vt, const void* ky, const void* vyt, const float* cross_w, int B, int T,
                 int Tpad, int L, int Lpad, int H, int hd, int np, void* out, void* stream) {
    return vb_attention_lens(q, k, vt, ky, vyt, cross_w, B, T, Tpad, L, Lpad, H, hd, np, nullptr, out, stream);
}
int vb_attention_lens(const void* q, const void* k, const void* vt, const void* ky, const void* vyt, const float* cross_w, int B, int T,
                      int Tpad, int L, int Lpad, int H, int hd, int np, const int32_t* key_len, void* out, void* stream) {
    if (key_len && !k) VB_FAIL(VB_E_INVALID, "attention_lens: key_len without self-attention keys");
    AttnArgs a;
    const int64_t ND = (int64_t)B * T * H * hd;
    a.q = wpl(q, ND, np); a.k = wpl(k, ND, np); a.vt = wpl(vt, (int64_t)B * H * hd * Tpad, np);
    a.ky = wpl(ky, (int64_t)B * L * H * hd, np); a.vyt = wpl(vyt, (int64_t)B * H * hd * Lpad, np);
    a.cross_w = cross_w; a.out = wpl(out, ND, np); a.B = B; a.T = T; a.Tpad = Tpad; a.L = L; a.Lpad = Lpad; a.H = H; a.hd = hd;
    a.has_self = k != nullptr; a.has_cross = ky != nullptr; a.kv_batch_mod = 0; a.scale = 1.0f / sqrtf((float)hd);
    a.key_len = key_len; a.key_len_mod = B;
    return launch_attention(a, (hipStream_t)stream);
}
int vb_conv1d_f32(const float* x, const float* w, const float* bias, int B, int Ci, int T_in, int Co, int ksize, int dil, int pad,
                  int tr_stride, int tr_pad, int tr_k, int T_out, int in_act, float in_slope, const float* res, float* out,
                  const void* w_x3, int ci_pad, void* stream) {
    ConvArgs a;
    if (w_x3) {
        const int phases = tr_stride > 1 ? tr_stride : 1;
        const int ntaps = tr_stride > 1 ? (tr_k + tr_stride - 1) / tr_stride : ksize;
        a.wp = (const bf16_t*)w_x3; a.Ci_pad = ci_pad; a.wp_plane = (int64_t)phases * ntaps * Co * ci_pad;
    }
    a.x = x; a.x_bstride = (int64_t)Ci * T_in; a.Ci = Ci; a.T_in = T_in; a.w = w; a.bias = bias; a.Co = Co; a.ksize = ksize;
    a.dil = dil; a.pad = pad; a.in_act = in_act; a.in_slope = in_slope; a.out = out; a.out_bstride = (int64_t)Co * T_out;
    a.T_out = T_out; a.res = res; a.res_bstride = (int64_t)Co * T_out; a.B = B; a.tr_stride = tr_stride; a.tr_pad = tr_pad; a.tr_k = tr_k;
    return launch_conv1d(a, (hipStream_t)stream);
}
int vb_conv1d_f32_mf(const float* x, const float* w, const float* w_mf, const float* bias, int B, int Ci, int T_in, int Co, int ksize, int dil,
                     int pad, int T_out, int in_act, float in_slope, const float* res, float alpha, float beta, float* out, void* stream) {
    if (!x || !w || !w_mf || !out || B < 1 || T_in < 1) VB_FAIL(VB_E_INVALID, "conv1d_f32_mf: null pointer or B/T < 1");
    ConvArgs a;
    a.x = x; a.x_bstride = (int64_t)Ci * T_in; a.Ci = Ci; a.T_in = T_in; a.w = w; a.w_mf = w_mf; a.bias = bias; a.Co = Co; a.ksize = ksize;
    a.dil = dil; a.pad = pad; a.in_act = in_act; a.in_slope = in_slope; a.out = out; a.out_bstride = (int64_t)Co * T_out;
    a.T_out = T_out; a.res = res; a.res_bstride = (int64_t)Co * T_out; a.B = B; a.alpha = alpha; a.beta = beta;
    return launch_conv1d(a, (hipStream_t)stream);
}
int vb_respair_f32(const float* x, const float* w1, const float* b1, const float* w2, const float* b2, int B, int C, int T, int k, int dil,
                   float slope, float alpha, float beta, float* out, void* stream) {
    if (!x || !w1 || !b1 || !w2 || !b2 || !out || B < 1 || T < 1) VB_FAIL(VB_E_INVALID, "respair_f32: null pointer or B/T < 1");
    RespairF32Args a;
    a.x = x; a.out = out; a.B = B; a.C = C; a.T = T; a.k = k; a.dil = dil; a.w1 = w1; a.w2 = w2; a.b1 = b1; a.b2 = b2;
    a.slope = slope; a.alpha = alpha; a.beta = beta;
    return launch_respair_f32(a, (hipStream_t)stream);
}
int vb_respair_f32_mf(const float* x, const float* w1_mf, const float* b1, const float* w2_mf, const float* b2, int B, int C, int T, int k, int dil,
                      float slope, float alpha, float beta, float* out, void* stream) {
    if (!x || !w1_mf || !b1 || !w2_mf || !b2 || !out || B < 1 || T < 1) VB_FAIL(VB_E_INVALID, "respair_f32_mf: null pointer or B/T < 1");
    RespairF32Args a;
    a.x = x; a.out = out; a.B = B; a.C = C; a.T = T; a.k = k; a.dil = dil; a.w1 = w1_mf; a.w2 = w2_mf; a.b1 = b1; a.b2 = b2;
    a.slope = slope; a.alpha = alpha; a.beta = beta;
    return launch_respair_f32w(a, (hipStream_t)stream);
}
int vb_conv1d_bf16(const float* x, const void* w_bf16, int ci_pad, const float* bias, int B, int Ci, int T_in, int Co, int ksize, int dil,
                   int pad, int tr_stride, int tr_pad, int tr_k, int T_out, int upsample2, int in_stride, int in_phase, int in_act,
                   float in_slope, const float* gn_mean, const float* gn_rstd, const float* gn_gamma, const float* gn_beta, int gn_groups,
                   const float* res, float alpha, float beta, float* out, void* stream) {
    if (!x || !w_bf16 || !out || B < 1 || T_in < 1 || T_out < 1 || Ci < 1 || Co < 1) VB_FAIL(VB_E_INVALID, "conv1d_bf16: null pointer or B/T/Ci/Co < 1");
    if ((in_act == ACT_GN || in_act == ACT_GN_SWISH) && (!gn_mean || !gn_rstd || !gn_gamma || !gn_beta || gn_groups < 1))
        VB_FAIL(VB_E_INVALID, "conv1d_bf16: GroupNorm input without its statistics / affine");
    ConvArgs a;
    a.wp = (const bf16_t*)w_bf16; a.Ci_pad = ci_pad; a.wp_bf16 = true;
    a.x = x; a.x_bstride = (int64_t)Ci * T_in; a.Ci = Ci; a.T_in = T_in; a.bias = bias; a.Co = Co; a.ksize = ksize;
    a.dil = dil; a.pad = pad; a.upsample2 = upsample2; a.in_stride = in_stride > 1 ? in_stride : 1; a.in_phase = in_phase;
    a.in_act = in_act; a.in_slope = in_slope; a.gn_mean = gn_mean; a.gn_rstd = gn_rstd; a.gn_gamma = gn_gamma; a.gn_beta = gn_beta;
    a.gn_groups = gn_groups > 0 ? gn_groups : 32;
    a.out = out; a.out_bstride = (int64_t)Co * T_out; a.T_out = T_out; a.res = res; a.res_bstride = (int64_t)Co * T_out; a.B = B;
    a.alpha = alpha; a.beta = beta; a.tr_stride = tr_stride; a.tr_pad = tr_pad; a.tr_k = tr_k;
    return launch_conv1d(a, (hipStream_t)stream);
}
size_t vb_xt_planes_bytes(int B, int C, int T_in, int upsample2, int nplanes) {
    if (B < 1 || C < 1 || T_in < 1 || (nplanes != 1 && nplanes != 2)) return 0;
    return (size_t)nplanes * B * xt_rows(upsample2 ? 2 * T_in : T_in) * C * sizeof(bf16_t);
}
int vb_xt_planes(const float* x, int B, int C, int T_in, int upsample2, int in_act, float in_slope, const float* gn_mean, const float* gn_rstd,
                 const float* gn_gamma, const float* gn_beta, int gn_groups, int nplanes, void* planes, void* stream) {
    if (!x || !planes || B < 1 || C < 1 || T_in < 1) VB_FAIL(VB_E_INVALID, "xt_planes: null pointer or B/C/T < 1");
    return launch_xt_planes(x, gn_mean, gn_rstd, gn_gamma, gn_beta, gn_groups, in_act, in_slope, upsample2, B, C, T_in, nplanes, (bf16_t*)planes,
                            (hipStream_t)stream);
}
int vb_gn_stats_lens(const float* x, int B, int C, int T, int groups, const int32_t* len, float* mean, float* rstd, void* stream) {
    if (!x || !mean || !rstd || B < 1 || C < 1 || T < 1 || groups < 1) VB_FAIL(VB_E_INVALID, "gn_stats_lens: null pointer or B/C/T/groups < 1");
    return launch_gn_stats(x, B, C, T, groups, 1e-6f, mean, rstd, (hipStream_t)stream, len);
}
int vb_softmax_rows_t_lens(const float* s, int B, int T, const int32_t* len, float* out_t, void* stream) {
    if (!s || !out_t || B < 1 || T < 1) VB_FAIL(VB_E_INVALID, "softmax_rows_t_lens: null pointer or B/T < 1");
    return launch_softmax_rows_t(s, B, T, T, out_t, (hipStream_t)stream, len);
}
int vb_aa_act(const float* x, const float* alpha, const float* inv_beta, const float* filt, int B, int C, int T, const int32_t* len, int len_mul,
              float* out, void* stream) {
    if (!x || !alpha || !inv_beta || !filt || !out || B < 1 || C < 1 || T < 1) VB_FAIL(VB_E_INVALID, "aa_act: null pointer or B/C/T < 1");
    return launch_aa_act(x, alpha, inv_beta, filt, B, C, T, out, (hipStream_t)stream, len, len_mul);
}
size_t vb_conv1d_bf16_xt_scratch_bytes(int B, int Ci, int T_in, int upsample2) { return vb_xt_planes_bytes(B, Ci, T_in, upsample2, 1); }
int vb_conv1d_bf16_xt(const float* x, const void* w_bf16, int ci_pad, const float* bias, int B, int Ci, int T_in, int Co, int ksize, int dil,
                      int pad, int tr_stride, int tr_pad, int tr_k, int T_out, int upsample2, int in_stride, int in_phase, int in_act,
                      float in_slope, const float* gn_mean, const float* gn_rstd, const float* gn_gamma, const float* gn_beta, int gn_groups,
                      const float* res, float alpha, float beta, float* out, void* planes_scratch, void* stream) {
    if (!x || !w_bf16 || !out || !planes_scratch || B < 1 || T_in < 1 || T_out < 1 || Ci < 1 || Co < 1)
        VB_FAIL(VB_E_INVALID, "conv1d_bf16_xt: null pointer or B/T/Ci/Co < 1");
    if (tr_stride > 1 || in_stride > 1) VB_FAIL(VB_E_INVALID, "conv1d_bf16_xt: the planes feed stride-1 convolutions only");
    hipStream_t st = (hipStream_t)stream;
    VB_TRY(launch_xt_planes(x, gn_mean, gn_rstd, gn_gamma, gn_beta, gn_groups, in_act, in_slope, upsample2, B, Ci, T_in, 1, (bf16_t*)planes_scratch, st));
    ConvArgs a;
    a.wp = (const bf16_t*)w_bf16; a.Ci_pad = ci_pad; a.wp_bf16 = true;
    a.xt = (const bf16_t*)planes_scratch; a.xt_np = 1;         // (the activation is in the plane: the convolution itself has none)
    a.x = x; a.x_bstride = (int64_t)Ci * T_in; a.Ci = Ci; a.T_in = T_in; a.bias = bias; a.Co = Co; a.ksize = ksize;
    a.dil = dil; a.pad = pad; a.upsample2 = upsample2;
    a.out = out; a.out_bstride = (int64_t)Co * T_out; a.T_out = T_out; a.res = res; a.res_bstride = (int64_t)Co * T_out; a.B = B;
    a.alpha = alpha; a.beta = beta; a.tr_stride = tr_stride; a.tr_pad = tr_pad; a.tr_k = tr_k;
    return launch_conv1d(a, st);
}
int vb_respair_bf16(const float* x, const void* w1_bf16, const float* b1, const void* w2_bf16, const float* b2, int B, int C, int T, int k,
                    int dil, float slope, float alpha, float beta, float* out, void* stream) {
    if (!x || !w1_bf16 || !b1 || !w2_bf16 || !b2 || !out || B < 1 || T < 1) VB_FAIL(VB_E_INVALID, "respair_bf16: null pointer or B/T < 1");
    RespairArgs a;
    a.x = x; a.out = out; a.B = B; a.C = C; a.T = T; a.k = k; a.dil = dil; a.w1 = (const bf16_t*)w1_bf16; a.w2 = (const bf16_t*)w2_bf16;
    a.b1 = b1; a.b2 = b2; a.slope = slope; a.alpha = alpha; a.beta = beta;
    return launch_respair_bf16(a, (hipStream_t)stream);
}
int vb_conv1d_f32_ups(const float* x, const float* w, const float* bias, int B, int Ci, int T_in, int Co, int ksize, int dil, int pad, int T_out,
                      int in_act, float in_slope, const float* res, float* out, void* stream) {
    if (!x || !w || !out || B < 1 || T_in < 1 || T_out < 1 || Ci < 1 || Co < 1) VB_FAIL(VB_E_INVALID, "conv1d_f32_ups: null pointer or B/T/Ci/Co < 1");
    ConvArgs a;
    a.x = x; a.x_bstride = (int64_t)Ci * T_in; a.Ci = Ci; a.T_in = T_in; a.w = w; a.bias = bias; a.Co = Co; a.ksize = ksize;
    a.dil = dil; a.pad = pad; a.upsample2 = 1; a.in_act = in_act; a.in_slope = in_slope; a.out = out; a.out_bstride = (int64_t)Co * T_out;
    a.T_out = T_out; a.res = res; a.res_bstride = (int64_t)Co * T_out; a.B = B;
    return launch_conv1d(a, (hipStream_t)stream);
}
int vb_conv1d_x3_xt(const float* x, const void* w_x3, int ci_pad, const float* bias, int B, int Ci, int T_in, int Co, int ksize, int dil, int pad,
                    int T_out, int upsample2, int in_act, float in_slope, const float* res, float alpha, float beta, float* out,
                    void* planes_scratch, void* stream) {
    if (!x || !w_x3 || !out || !planes_scratch || B < 1 || T_in < 1 || T_out < 1 || Ci < 1 || Co < 1)
        VB_FAIL(VB_E_INVALID, "conv1d_x3_xt: null pointer or B/T/Ci/Co < 1");
    hipStream_t st = (hipStream_t)stream;
    VB_TRY(launch_xt_planes(x, nullptr, nullptr, nullptr, nullptr, 0, in_act, in_slope, upsample2, B, Ci, T_in, 2, (bf16_t*)planes_scratch, st));
    ConvArgs a;
    a.wp = (const bf16_t*)w_x3; a.Ci_pad = ci_pad; a.wp_plane = (int64_t)ksize * Co * ci_pad;
    a.xt = (const bf16_t*)planes_scratch; a.xt_np = 2;         // (the activation is in the planes: the convolution itself has none)
    a.x = x; a.x_bstride = (int64_t)Ci * T_in; a.Ci = Ci; a.T_in = T_in; a.bias = bias; a.Co = Co; a.ksize = ksize;
    a.dil = dil; a.pad = pad; a.upsample2 = upsample2;
    a.out = out; a.out_bstride = (int64_t)Co * T_out; a.T_out = T_out; a.res = res; a.res_bstride = (int64_t)Co * T_out; a.B = B;
    a.alpha = alpha; a.beta = beta;
    return launch_conv1d(a, st);
}
int vb_respair_x3(const float* x, const void* w1_x3, const float* b1, const void* w2_x3, const float* b2, int B, int C, int T, int k, int dil,
                  float slope, float alpha, float beta, float* out, void* stream) {
    if (!x || !w1_x3 || !b1 || !w2_x3 || !b2 || !out || B < 1 || T < 1) VB_FAIL(VB_E_INVALID, "respair_x3: null pointer or B/T < 1");
    RespairArgs a;
    a.x = x; a.out = out; a.B = B; a.C = C; a.T = T; a.k = k; a.dil = dil; a.w1 = (const bf16_t*)w1_x3; a.w2 = (const bf16_t*)w2_x3;
    a.b1 = b1; a.b2 = b2; a.slope = slope; a.alpha = alpha; a.beta = beta;
    return launch_respair(a, (hipStream_t)stream);
}
int vb_fill_gumbel(float* out, int B, int n_branch, int T, int width, uint64_t seed, int64_t clip_base, int nfe, int block, int gate,
                   void* stream) {
    return launch_fill_gumbel(out, B, n_branch, T, width, seed, clip_base, nfe, nullptr, block, gate, (hipStream_t)stream);
}
int vb_cast_planes(const float* x, int64_t n, void* out, int np, void* stream) {
    return launch_cast_planes(x, n, mkp((bf16_t*)out, n, np), (hipStream_t)stream);
}

}  // extern "C"
