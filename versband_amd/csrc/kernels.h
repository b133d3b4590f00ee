// Internal launch API shared by the engines and the C-ABI wrappers.
#pragma once
#include <type_traits>

#include "common.h"

// ---------------------------------------------------------------------------
// bf16 MFMA GEMM   C[m][n] = sum_k A[m][k] * B[n][k]   (both operands K-contiguous)
// ---------------------------------------------------------------------------
enum GemmEpi {
    EPI_PLANES = 0,          // out planes[m][coff+n] = v (+bias)
    EPI_F32 = 1,             // out32[m][coff+n] = v (+bias)
    EPI_QKV_ROPE = 2,        // q,k planes with RoPE; v written transposed per head
    EPI_RESID_GATE = 3,      // out32[m][coff+n] += gate[b(m)][coff+n] * v
    EPI_SWIGLU = 4,          // interleaved (w1,w3) columns -> planes[m][coff + n/2] = silu(v0)*v1
    EPI_SCATTER_F32 = 5,     // out32[rows_out[m]][n] = row_scale[rows_out[m]] * v
    EPI_SCATTER_ADD_PLANES = 6,  // planes[tok][n] = y32_in[tok][n] + row_scale[tok]*v
    EPI_GELU_PLANES = 7,     // planes = gelu_erf(v + bias)
    EPI_HEADS_T = 8,         // planes[((b*H+h)*hd+d)*Tpad + t] = v (+bias),  m = b*T+t, n = h*hd+d
    EPI_GEGLU = 10,          // planes[m][n/2] = gelu_new(v[n]) * v[n+1]  (T5 gated-GELU FFN, rows of wi_0 / wi_1 interleaved)
    EPI_F32_CT = 9,          // out32[(b*N + n)*T + t] = v + bias  (channel-major [B][N][T] output of the FinalLayer), m = b*T+t
    EPI_COUNT = 9
};

struct GemmArgs {
    const bf16_t* A = nullptr; int64_t a_plane = 0; int lda = 0;
    const int* a_rows = nullptr;      // optional row gather (slot -> token)
    int a_koff_group = 0;             // A column offset per group index
    const bf16_t* B = nullptr; int64_t b_plane = 0; int ldb = 0; int64_t b_group_stride = 0;
    int M = 0, N = 0, K = 0;
    int nseg = 1;                     // 1 = plain bf16, 3 = bf16x3 split precision
    int ngroups = 1; const int* group_off = nullptr;   // device [ngroups+1] slot offsets (null: one group [0,M))
    int group_rows = 0;               // > 0 (group_off optional then): every group has exactly this many rows (group g = rows [g R, (g+1) R): per-clip
                                      // operands) - the 128 x 128 kernel then keeps all tiles of a group on ONE XCD (group g -> XCD g % 8), so
                                      // a group's B operand is fetched into one L2 instead of all eight
    int c_noff_group = 0;             // output column offset per group
    int epi = EPI_F32;
    const float* bias = nullptr; int64_t bias_group_stride = 0;
    Planes out = {nullptr, 0, 1}; int ldc = 0;
    float* out32 = nullptr; int ldc32 = 0;
    const float* gate = nullptr; int gate_ld = 0; int T = 1;
    const int* rows_out = nullptr; const float* row_scale = nullptr; const float* y32_in = nullptr;
    // EPI_SWIGLU only: per-row gate weight folded into the hidden value BEFORE its bf16 rounding (rows < scale_split take
    // row_scale[a_rows[m]], the others row_scale2[a_rows[m]]): lets the routed w2 product run as one plain K-concatenated GEMM
    const float* row_scale2 = nullptr; int scale_split = 0;
    // EPI_F32 only: out32[m][n] = v + bias + add32[m][n] (same leading dimension), written to row m AND, when dup_rows > 0, to row
    // m + dup_rows (both CFG branches start from the same embedded latent)
    const float* add32 = nullptr; int dup_rows = 0;
    // Conv1d as a GEMM over pre-activated transposed planes (EPI_F32_CT with group_rows = T_out): K = taps * conv_ci walks tap by tap -
    // the A rows of tap j are the rows of tap 0 shifted by j * conv_dil, its B operand sits conv_btap elements behind tap j-1's; group g
    // (a clip) starts at A row g * conv_agrp + conv_arow0; res32 (same [b][n][t] layout as the output) is added in the epilogue.
    int conv_ci = 0, conv_dil = 1, conv_agrp = 0, conv_arow0 = 0; int64_t conv_btap = 0; const float* res32 = nullptr;
    int prof_class = 0;               // kernel class of the HIP-event profiler this launch is counted under (2 = split-bf16 convolution work)
    Planes q = {nullptr, 0, 1}, k = {nullptr, 0, 1}, vt = {nullptr, 0, 1};
    const float* rope_cos = nullptr; const float* rope_sin = nullptr;
    int H = 1, hd = 1, Tpad = 0, D = 0;
};
// the ten operand fields every launch sets; a call site then adds what distinguishes it (epilogue, outputs, groups)
static inline GemmArgs gemm_operands(const void* A, int64_t a_plane, int lda, const void* B, int64_t b_plane, int ldb, int M, int N, int K, int nseg) {
    GemmArgs g;
    g.A = (const bf16_t*)A; g.a_plane = a_plane; g.lda = lda; g.B = (const bf16_t*)B; g.b_plane = b_plane; g.ldb = ldb;
    g.M = M; g.N = N; g.K = K; g.nseg = nseg;
    return g;
}
int launch_gemm(const GemmArgs& a, hipStream_t st);
void gemm_conv_tile(int B, int T_out, int Co, int* bm, int* bn);      // the tile of a conv-mode launch (GemmArgs::conv_*), host only
// routed experts, second product of BOTH groups in one launch over (caption, acoustic) pair buckets (bf16, E <= 4; moe_w2_pair_kernel):
// out[tok][:] = Hs[caption slot] W2[c]^T + Hs[acoustic slot] W2[E + a]^T  with the gate weights m_c / m_a already folded into the
// hidden rows by the SwiGLU epilogue (GemmArgs::row_scale / row_scale2): one accumulator, K = 2H
struct MoeW2PairArgs {
    const bf16_t* Hs = nullptr; const bf16_t* W2 = nullptr;     // [2N][H] bf16 slot order (gate-scaled); [2E][D][H]
    const int* pair_off = nullptr; const int* perm = nullptr; const int* pair_pa = nullptr;        // launch_bucket pair-mode outputs
    bf16_t* out = nullptr;                                      // out [N][D] bf16
    int N = 0, D = 0, H = 0, E = 0;
};
int launch_moe_w2_pair(const MoeW2PairArgs& a, hipStream_t st);
// fused band-expert FFN (bf16): out32[:, e*band .. ] += gate * ( W2_e . (silu(W1_e y_e) * (W3_e y_e)) ), y_e = y[:, e*band ..]
struct BandFfnArgs {
    const bf16_t* y = nullptr; int ldy = 0;          // [M][ldy] bf16 (one plane)
    const bf16_t* w13 = nullptr; const bf16_t* w2 = nullptr;   // [E][2H][band] interleaved w1/w3 rows, [E][band][H]
    int M = 0, H = 0, E = 0, band = 0;
    float* out32 = nullptr; int ldc32 = 0; const float* gate = nullptr; int gate_ld = 0; int T = 1;
};
int launch_band_ffn(const BandFfnArgs& a, hipStream_t st);
int band_ffn_tile_rows(int band);                    // tokens per workgroup of the fused kernel (band = 192 or 96)

// ---------------------------------------------------------------------------
// flash attention over bf16 planes (head_dim 96): out = softmax(q k^T s) v  [+ w_h * softmax(q ky^T s) vy]
// ---------------------------------------------------------------------------
struct AttnArgs {
    Planes q;            // [B*T][H*hd]
    Planes k;            // [B*T][H*hd]       (self; may be null when !has_self)
    Planes vt;           // [B][H][hd][Tpad]
    Planes ky;           // [B*L][H*hd]       (cross; may be null)
    Planes vyt;          // [B][H][hd][Lpad]
    const float* cross_w;  // [H] per-head weight of the cross term (null -> 1)
    Planes out;          // [B*T][H*hd]
    int B, T, Tpad, L, Lpad, H, hd;
    int has_self, has_cross;
    int kv_batch_mod;    // cross K/V batch index = b % kv_batch_mod (0: = b)
    float scale;
    // row lengths (vb_lens), self pass only: device [key_len_mod] - batch row b attends over its first key_len[b % key_len_mod] keys and its
    // query rows from there on are padding (null: T keys, no padding)
    const int* key_len = nullptr; int key_len_mod = 1;
};
int launch_attention(const AttnArgs& a, hipStream_t st);

// ---------------------------------------------------------------------------
// fp32 MFMA implicit-GEMM Conv1d   out[b][co][t] over x[b][ci][t]
// ---------------------------------------------------------------------------
enum ConvAct { ACT_NONE = 0, ACT_LRELU = 1, ACT_GN_SWISH = 2, ACT_TANH = 3, ACT_GN = 4 };
struct ConvArgs {
    const float* x = nullptr; int64_t x_bstride = 0; int Ci = 0; int T_in = 0; int x_bmod = 0;
    const float* w = nullptr;        // packed [phase][tap][Ci][Co]
    int64_t w_bstride = 0;           // per-batch weights (VAE attention), 0 = shared
    const float* bias = nullptr;
    int Co = 0, ksize = 1, dil = 1, pad = 0;
    int upsample2 = 0;               // nearest x2 on the input (T_in is the un-upsampled length)
    int in_stride = 1, in_phase = 0; // the convolution reads x[i * in_stride + in_phase] (Downsample1D as two polyphase convs)
    int in_act = ACT_NONE; float in_slope = 0.f;
    const float* gn_mean = nullptr; const float* gn_rstd = nullptr;   // [B][groups]
    const float* gn_gamma = nullptr; const float* gn_beta = nullptr; int gn_groups = 32;
    float* out = nullptr; int64_t out_bstride = 0; int T_out = 0;
    const float* res = nullptr; int64_t res_bstride = 0;   // residual [b][co][t] (same layout as out)
    float alpha = 1.f;               // out = beta*out + alpha*(acc*acc_scale + bias + res)
    float beta = 0.f;
    float acc_scale = 1.f;
    int out_act = ACT_NONE; float out_slope = 0.f;
    int out_transposed = 0;          // out[b][t][co] (+ add[b % add_bmod][t][co])
    const float* add = nullptr; int64_t add_bstride = 0; int add_bmod = 0;
    int B = 1;
    // transposed convolution (polyphase): stride u > 1
    int tr_stride = 1; int tr_pad = 0; int tr_k = 0;
    // optional split-bf16 weights [2][phase][tap][Co][Ci_pad] (Ci_pad % 32 == 0): selects the bf16x3 MFMA kernel
    const bf16_t* wp = nullptr; int64_t wp_plane = 0; int Ci_pad = 0;
    int64_t wp_bstride = 0;          // per-batch split weights (bf16 elements inside a plane), VAE attention
    bool wp_bf16 = false;            // wp holds ONE plane (the round-to-nearest bf16 weights): the single-pass bf16 kernel (conv1d_bf16.hip)
    // optional pre-activated transposed split planes of the input (xt_planes_kernel): [2][B][xt_rows(T_in)][Ci]; x / in_act /
    // GroupNorm fields are then ignored and the window is DMA'd straight into LDS.  xt_np = planes the buffer holds: 2 for the split weights,
    // 1 (the round-to-nearest plane alone, [B][xt_rows(T_in)][Ci]) for wp_bf16
    const bf16_t* xt = nullptr; int xt_np = 2;
    // optional minimal-filtering weights [P][Ci][Co] fp32 (pack.py:pack_conv_mf): selects conv1d_f32w_kernel (fp32 products, F(2,3)) where it applies
    const float* w_mf = nullptr;
    // row lengths (device [B], in units of len_mul input positions, upsampling counted): the ACTIVATED input of row b ends at
    // row_len[b] * len_mul, the register-staged kernels zero-pad from there on (GroupNorm maps a zero tail to something else); null = T
    const int* row_len = nullptr; int len_mul = 1;
};
int launch_conv1d(const ConvArgs& a, hipStream_t st);
// fused HiFi-GAN ResBlock1 pair (respair_x3.hip; checks, descriptor and epilogue shared with the bf16 form: respair_dev.h): out = beta*out + alpha*(x + b2 + conv2(lrelu(b1 + conv1_dil(lrelu(x)))))
struct RespairArgs {
    const float* x = nullptr; float* out = nullptr; int B = 1, C = 0, T = 0, k = 3, dil = 1;
    const bf16_t* w1 = nullptr; const bf16_t* w2 = nullptr;     // split planes [2][k][C][C]
    const float* b1 = nullptr; const float* b2 = nullptr;
    float slope = 0.1f, alpha = 1.f, beta = 0.f;
    const int* row_len = nullptr; int len_mul = 1;     // row lengths (device [B], in units of len_mul samples): the intermediate is zero from row_len[b] * len_mul on; null = T
};
int launch_respair(const RespairArgs& a, hipStream_t st);
// the same pair in single-pass bf16 (respair_bf16.hip; same window rules and checks, respair_dev.h): w1 / w2 = ONE plane [k][C][C] each, the intermediate rounded to bf16 once; C = 32 / 64
int launch_respair_bf16(const RespairArgs& a, hipStream_t st);
// the same pair in exact fp32 (respair_f32.hip; v_mfma_f32_32x32x2_f32, weights fp32 packed [k][Ci][Co]): C = 32 / 64 / 128
struct RespairF32Args {
    const float* x = nullptr; float* out = nullptr; int B = 1, C = 0, T = 0, k = 3, dil = 1;
    const float* w1 = nullptr; const float* w2 = nullptr; const float* b1 = nullptr; const float* b2 = nullptr;
    float slope = 0.1f, alpha = 1.f, beta = 0.f;
    const int* row_len = nullptr; int len_mul = 1;     // as RespairArgs
};
bool respair_f32_supported(const RespairF32Args& a);
int launch_respair_f32(const RespairF32Args& a, hipStream_t st);
// the same pair with F(2,3) minimal filtering (respair_f32w.hip): w1 / w2 = pseudo-tap weights [P][C][C] (pack.py:pack_conv_mf); C = 32, k = 3 / 7 / 11
bool respair_f32w_supported(const RespairF32Args& a);
int launch_respair_f32w(const RespairF32Args& a, hipStream_t st);
// intermediate positions per workgroup (the `run` of pair_fill_common) of the two fp32 pairs: what vb_respair_plan reports
int respair_f32_run(void);
int respair_f32w_run(int C, int dil);

// ---------------------------------------------------------------------------
// elementwise.hip: norms, casts and small helpers of the DiT, T5 and the sampler's tabulation; rowlin.hip, t5.hip, melnet.hip
// ---------------------------------------------------------------------------
int launch_rmsnorm_mod(const float* h, const float* w, const float* shift, const float* scale, int mod_ld,
                       int rows, int D, int T, float eps, Planes out, hipStream_t st);
int launch_layernorm(const float* x, const float* w, const float* b, int rows, int D, float eps, float* out32, Planes outp,
                     hipStream_t st);
int launch_cast_planes(const float* x, int64_t n, Planes out, hipStream_t st);
int launch_planes_to_f32(Planes in, int64_t n, float* out, hipStream_t st);
int launch_fill_f32(float* p, int64_t n, float v, hipStream_t st);
int launch_mean_rows(const float* x, int B, int L, int D, float* out, hipStream_t st);
// (indices clamped to [0, vocab); len: device [B] row lengths in units of len_mul positions - out is 0 from len_mul * len[b] on)
int launch_embed_t(const int64_t* idx, const float* table, int B, int T, int D, int vocab, float* out, hipStream_t st, const int* len = nullptr, int len_mul = 1);
int launch_pool_add(const float* a, const float* b, int B, int C, int T_in, float* out, hipStream_t st);
int launch_transpose_bct_btc(const float* in, int B, int C, int T_in, int T_out, float* out, hipStream_t st);
// proj_in as a GEMM: latent windows as K-contiguous split planes, conv weights re-laid as a GEMM operand
// (len: device [B] row lengths - the clip of row b ends at len[b], taps beyond it are zero; null: T)
int launch_im2col_latent(const float* x, int B, int C, int T, int taps, int pad, int KP, bf16_t* out, int64_t plane, hipStream_t st, const int* len = nullptr);
// row lengths of a call (vb_lens): out[b][c][t] = t < len[b] * len_mul ? x[b][c][t] : 0, what a general convolution kernel reads in place of x
// (T: the pitch of x in samples; len_mul: samples per unit of len - the VAE encoder's input runs at in_tmul mel frames per latent token)
int launch_mask_latent(const float* x, int B, int C, int T, const int* len, float* out, hipStream_t st, int len_mul = 1);
// the validated lengths of a call, by value in the kernel's argument block like WindowPlan, and their way into the workspace table.
// lens_plan checks len (HOST array) for B rows of T tokens: B <= 64, 1 <= len[b] <= T; VB_E_INVALID names the row otherwise.  B = 0 in
// the plan: every row is full, the call is the plain one.
struct LensPlan {
    int B = 0; int len[64] = {};
    int first_short(int T) const { for (int b = 0; b < B; ++b) if (len[b] < T) return b; return 0; }      // (for messages)
};
int lens_plan(const int32_t* len, int B, int T, LensPlan* out);
int launch_lens_table(const LensPlan& lp, int* out, hipStream_t st);
// row lengths in a conv net (vb_hifigan_forward_lens): out[b][c][len[b] * tmul .. T * tmul) = 0 for every row shorter than T, in one launch
// whose grid covers only the tails (rows x channels x the longest tail); 16-byte stores when the row pitch, every short row's tail start and
// the base allow, 4-byte stores otherwise.  len: the device table of lp's lengths.  Nothing is launched when no row is short.
int launch_tail_zero(float* out, const LensPlan& lp, const int* len, int B, int C, int T, int tmul, hipStream_t st);
int launch_conv_w_to_gemm(const bf16_t* w3, int64_t w3_plane, int taps, int D, int KP, bf16_t* out, hipStream_t st);
int launch_rows_dot(const float* x, const float* W, const float* bias, int N, int D, int E, float* out, hipStream_t st);
// LayerNorm (no affine, eps) + adaLN modulate -> split-bf16 planes (FinalLayer input, vocal2music_moe.py:287-291)
int launch_layernorm_mod_planes(const float* h, const float* shift, const float* scale, int mod_ld, int rows, int D, int T, float eps,
                                Planes out, hipStream_t st);
int launch_silu_sum_planes(const float* temb, const float* cemb, int rows, int D, int nsample, bf16_t* out, int64_t plane, hipStream_t st);
int launch_iota_div(int64_t* out, int n, int div, hipStream_t st);
// row linears (rowlin.hip)
int launch_gemv_rows(const float* x, int x_ld, const float* x2, int x2_ld, int x2_mod, const float* W, const float* bias,
                     int R, int N, int K, int act_in, float* out, int out_ld, hipStream_t st);
int launch_gemv_rows_idx(const float* x, int x_ld, const int64_t* idx, const float* x2, int x2_ld, int x2_mod, const float* W,
                         const float* bias, int R, int N, int K, int act_in, float* out, int out_ld, hipStream_t st, int sin_rows = 0);
// (sin_rows > 0: x is the timestep-sinusoid table with that many rows; indices outside it are evaluated on the fly)
int launch_final_layer(const float* h, const float* shift, const float* scale, int mod_ld, const float* W, const float* bias,
                       int rows, int D, int T, int C, float eps, float* out, hipStream_t st);
bool final_layer_fused_ok(int D, int C);
int launch_final_layer_fused(const float* h, const float* shift, const float* scale, int mod_ld, const float* W, const float* bias,
                             int rows, int D, int T, int C, float eps, float* out, hipStream_t st);
// T5 (t5.hip)
int launch_gather_rows(const int64_t* idx, const float* table, int rows, int D, int vocab, float* out, hipStream_t st);
int launch_t5_attention(Planes qkv, const float* pos_bias, int pos_len, int B, int L, int heads, int dkv, Planes out, hipStream_t st);
// log-mel front-end (melnet.hip)
// (len: device [B] row lengths in samples - row b reflects at its own end and is zero from its own last hop-block on, taps = n_fft / hop;
//  tlen: device [B] row lengths in frames - mel is 0 from tlen[b] on; null: the whole row)
int launch_stft_frames(const float* wav, int B, int L, int hop, int pad, int pad2, int J, float* X, hipStream_t st, const int* len = nullptr, int taps = 0);
int launch_mel_tail(const float* spec, int B, int T, int Co4, int nb, int im_off, const float* basisT, int n_mels, float* mel, hipStream_t st,
                    const int* tlen = nullptr);
// out[r] = mean over m < M, t < frames[r] of |a - b - mu_r|, mu_r = the mean of a - b over the same range (remove_offset) or 0; out_offset
// (nullable) = mu_r.  frames: device [B].  One workgroup per row, a fixed reduction shape (melnet.hip)
int launch_mel_dist(const float* a, int Ta, const float* b, int Tb, int B, int M, const int* frames, int remove_offset, float* out, float* out_offset,
                    hipStream_t st);

// ---------------------------------------------------------------------------
// sampler_step.hip: the sampler's update and step bookkeeping (+ the fused form of the update, rowlin.hip)
// ---------------------------------------------------------------------------
// known region of a sampler call (vb_keep with its time table on the device): ref / x0 [B][C][T], mask [B][T], tn_table[k] = t after step k
struct EulerKeep { const float* ref; const float* x0; const float* mask; const float* tn_table; float sigma_min; };
// One step's CFG + Euler update, described once for both of its launches: x [B][C][T] += dt_table[step] * (v_u + s (v_c - v_u)) with
// s = cfg_scale, or scale_rows[b] (vb_sample_cfg_rows: device [B], cfg_scale is then unused), then - keep != nullptr - the known tokens
// put back on the probability path (common.h:keep_path / keep_blend).  Every form is the same two fused multiply-adds
// (common.h:euler_cfg_update).  The fields from k on are the step advance the fused launch does for the NEXT step: host step index k,
// device counter `step` (null: no advance) and t_idx_cur[0..Beff) = t_table[min(k + 1, n_steps - 1)].
struct EulerStep {
    float* x = nullptr; float cfg_scale = 0.f; const float* scale_rows = nullptr; const float* dt_table = nullptr;
    const EulerKeep* keep = nullptr;
    // vb_sample_cfg_sched, beside scale_rows only: this step's guidance weight w, the row's scale becomes fmaf(w, scale_rows[b] - 1, 1).
    // 1 = the ROWS form; anything else is the SCHED form (euler_form).  (A scalar scale is combined on the host: cfg_scale.)
    float row_weight = 1.f;
    int k = 0; int* step = nullptr; int64_t* t_idx_cur = nullptr; const int64_t* t_table = nullptr; int n_steps = 0, Beff = 0;
};
// The update's kernel-argument block, the same for both launches and every form: all that any form reads.  The kernels' template flags
// <KEEP, ROWS, SCHED> select the code, so an instance reads the fields of its form only (kp: KEEP; scale_rows: ROWS, cfg_scale otherwise;
// weight: SCHED) and the others cost kernel-argument bytes.  dt_val is the stand-alone launch's step size where dt_table is null
// (vb_euler_cfg_step); the fields from k on are the fused launch's step advance.  Value-initialised: what the FinalLayer without an
// update is given.
struct EulerDev {
    float* x; float cfg_scale; const float* dt_table; int k; int* step; int64_t* t_idx_cur; const int64_t* t_table; int n_steps, Beff;
    EulerKeep kp; const float* scale_rows; float weight, dt_val;
};
inline EulerDev euler_dev(const EulerStep& es, float dt_val = 0.f) {
    return {es.x, es.cfg_scale, es.dt_table, es.k, es.step, es.t_idx_cur, es.t_table, es.n_steps, es.Beff,
            es.keep ? *es.keep : EulerKeep{}, es.scale_rows, es.row_weight, dt_val};
}
// The form of one update, decided once for both launches: KEEP with a known region, ROWS with per-row scales, SCHED when those scales
// stand under a step weight other than 1 - and there is an unconditional half to guide against (the fused launch always has one).
struct EulerForm { bool keep, rows, sched; };
inline EulerForm euler_form(const EulerStep& es, bool has_uncond) {
    const bool rows = es.scale_rows != nullptr;
    return {es.keep != nullptr, rows, rows && has_uncond && es.row_weight != 1.f};
}
// go(KEEP, ROWS, SCHED) with the form as std::bool_constants: the six legal forms (SCHED implies ROWS), each one kernel instance
template <class Go>
void euler_dispatch(EulerForm f, Go&& go) {
    const std::true_type yes; const std::false_type no;
    if (f.keep) { if (f.sched) go(yes, yes, yes); else if (f.rows) go(yes, yes, no); else go(yes, no, no); }
    else { if (f.sched) go(no, yes, yes); else if (f.rows) go(no, yes, no); else go(no, no, no); }
}
// FinalLayer + the update + the step advance as one launch (rows = 2 x (B T) token rows, conditional half first; reads es.k, not *es.step)
int launch_final_layer_euler(const float* h, const float* shift, const float* scale, int mod_ld, const float* W, const float* bias,
                             int rows, int D, int T, int C, float eps, const EulerStep& es, hipStream_t st);
// the update as a launch of its own over v [2B or B][per] (per = C * T; has_uncond = 0: v holds B rows and no scale is read):
// dt = es.dt_table[*es.step], or dt_val when es.dt_table is null; the step-advance fields are not used (launch_step_ctl)
int launch_euler_cfg(const EulerStep& es, const float* v, int B, int64_t per, int T, int has_uncond, float dt_val, hipStream_t st);
// projection on entry: x <- blend(mask, r(t_0), x) with t_0 = tn_table[0] - dt_table[0]
int launch_keep_project(float* x, int B, int64_t per, int T, const float* dt_table, const EulerKeep& keep, hipStream_t st);
// joint windows (vb_sample_cfg_windows): the validated plan, by value in the kernel's argument block (nothing on the device to fill, and
// a captured graph holds its own copy).  window_plan checks starts (HOST array) for B rows of n tokens: 1 <= nw <= 64, B % nw == 0,
// starts[0] >= 0, starts[w] < starts[w+1] <= starts[w] + n, starts[w+2] >= starts[w] + n; VB_E_INVALID names the window otherwise.
struct WindowPlan { int nw = 0; int s[64] = {}; };
int window_plan(const int32_t* starts, int nw, int B, int n, WindowPlan* out);
// x [nw*Bc][C][n] (row = w*Bc + b): both copies of every overlapping token <- fmaf(g, x[ib] - x[ia], x[ia]), g = (u + 1) / (ov + 1)
int launch_window_blend(float* x, const WindowPlan& wp, int Bc, int C, int n, hipStream_t st);
// window rows (vb_sample_cfg_window_rows): joint windows of clips of different lengths - the validated pair table, by value in the kernel's
// argument block like WindowPlan.  Row r is a window of clip group[r] over its tokens [start[r], start[r] + len[r]); consecutive rows
// (ra, rb) of a group with ov = start[ra] + len[ra] - start[rb] > 0 are one pair: token off_a + u of row ra and token u of row rb,
// off_a = len[ra] - ov, are the same token.  window_rows_plan checks group / start (HOST arrays; len: the call's LensPlan, B = 0 in it:
// every row has T) for B <= 64 rows: start[r] >= 0, ascending within a group, no gap, ov <= len[rb], no token under three rows;
// VB_E_INVALID names the row otherwise.  np = 0: no group has two overlapping rows, the call is the one without the block.  B rows in
// at least one group give at most 63 pairs.  The kernel is handed the pairs alone; group / start are kept for the graph key.
struct WindowPairs {
    struct Pair { int ra, rb, off_a, ov; };
    int np = 0; Pair p[63] = {};
};
struct WindowRowsPlan {
    WindowPairs pairs; int ov_max = 0;
    int B = 0; int group[64] = {}; int start[64] = {};
};
int window_rows_plan(const int32_t* group, const int32_t* start, const LensPlan& lp, int B, int T, WindowRowsPlan* out);
// x [B][C][T]: both copies of every overlapping token of every pair <- fmaf(g, x[ib] - x[ia], x[ia]), g = (u + 1) / (ov + 1)
int launch_window_rows_blend(float* x, const WindowRowsPlan& wr, int C, int T, hipStream_t st);
int launch_sampler_params(int* step, uint64_t seed, int64_t clip_base, int nfe_base, hipStream_t st);   // step[4..9]: noise key of the call
int launch_step_ctl(int* step, int64_t* t_idx_cur, const int64_t* t_table, int n_steps, int Beff, int reset, hipStream_t st);

// ---------------------------------------------------------------------------
// routing.hip: Band-MoE router and bucketing (+ the fused score + router kernel, score_router.hip)
// ---------------------------------------------------------------------------
// Band-MoE router: call arguments and the kernel's argument block in one (the device side is router_dev.h).  Both users - launch_router and the
// fused score + router kernel - get it from ONE fill (dit.hip: router_args), so a per-row option is threaded through once.
// SC = true: "folded" caption gate.  The token features are not materialised at all: `sc` holds the token's attention
// SCORES against its clip's caption keys for all heads ([N][NS], NS = L * Hh, column = key * Hh + head; scale, q-projection
// and q-bias already inside - one grouped GEMM against per-clip folded keys), `Wg` holds per clip VW[key*Hh+head][e] =
// value_row(head) . (gate weight row e restricted to the head), so   logit_e = sum_heads sum_keys softmax(scores)_key VW_e.
struct RouterDev {
    Planes cq = {nullptr, 0, 1}; const float* Wg = nullptr; const float* bg = nullptr; const float* la = nullptr; int la_rows = 0; const float* hl = nullptr; int hl_ld = 0;
    const float* g1 = nullptr; const float* g2 = nullptr; const float* g3 = nullptr; int N = 0, T = 0, D = 0, E = 0;
    int* ic = nullptr; int* ia = nullptr; float* mc = nullptr; float* ma = nullptr; float* lc_out = nullptr; int B = 0;
    uint64_t seed = 0; int64_t clip_base = 0; int nfe_base = 0; const int* step = nullptr; int block = 0; const float* sc = nullptr; int NS = 0, Hh = 1;
    // vb_sample_cfg_rows: device [B] global clip ids - row b of every branch draws from the stream of clip clip_rows[b] instead of clip_base + b
    const int64_t* clip_rows = nullptr;
    // bucket counts as a side product (round 5): cnt[(n / RT_CNT_BLOCK) * cnt_G + group] += 1 for the token's expert pair (cnt_pairs) or its two
    // expert groups - what bucket_count_kernel computed in a launch of its own; the table must be zero on entry (launch_bucket's place kernel
    // clears the table of the NEXT launch).  Integer atomics: the sums do not depend on their order.
    int* cnt = nullptr; int cnt_G = 0; int cnt_pairs = 0;
};
// (B <= 0 is taken as 1; NS / Hh count only with sc)
int launch_router(const RouterDev& a, hipStream_t st);
// fused caption-gate scores + router (score_router.hip): bf16 token features x per-clip folded keys -> routing decisions, the
// [N][NS] score matrix stays in LDS.  Bit-identical to launch_gemm(EPI_F32 scores) + launch_router(sc = scores).
// The GEMM side, and the router's own argument block for everything else: the caller fills r as for launch_router with Wg = the per-clip
// VW [Beff][NS][E]; launch_score_router owns r.N (= Beff * T), r.D (= K), r.sc, r.lc_out and r.cnt (all null: nothing is read back or counted).
struct ScoreRouterArgs {
    const bf16_t* A = nullptr; int lda = 0;          // token features [Beff*T][lda] bf16
    const bf16_t* Bm = nullptr; int ldb = 0;         // folded keys [Beff][NS][ldb] bf16
    const float* bias = nullptr;                     // [Beff][NS]
    int K = 0, Beff = 0;
    RouterDev r;
};
bool score_router_supported(int NS, int K, int E, int Hh);
int launch_score_router(const ScoreRouterArgs& a, hipStream_t st);
// the product form of the same fusion (gate_route.hip: softmax and contraction lane-local in the MFMA's accumulator layout; NS = 640, K = 768,
// E = 4, 8 heads).  Same arguments, same bits; unlike launch_score_router it keeps r.cnt / cnt_G / cnt_pairs: it counts as launch_router does.
bool gate_route_supported(int NS, int K, int E, int Hh);
int launch_gate_route(const ScoreRouterArgs& a, hipStream_t st);
// (pair_off / pair_pa non-null, E*E <= 16: rank by (caption, acoustic) expert PAIR; both expert-group orders derive from it - see
//  bucket_place_kernel.  pair_off [E*E + 1], pair_pa [N] = acoustic slot of the token in pair / caption slot p)
// counts_ready (round 5): the per-256-token-block group counts were already accumulated by the router (RouterDev::cnt) - the count launch is
// skipped; counts_clear: a second table the place kernel zeroes for the next router launch (ping-pong, see bucket_counts)
int launch_bucket(const int* ic, const int* ia, int N, int E, int* group_off, int* perm, hipStream_t st, int* pair_off = nullptr,
                  int* pair_pa = nullptr, const int* counts_ready = nullptr, int* counts_clear = nullptr);
int bucket_scratch_ints(int N, int E);   // perm buffers must hold 2N + this many ints
bool bucket_router_counts_ok(int N);     // the launch takes the two-kernel (count + place) form whose count the router can provide
int* bucket_counts(int* perm, int N, int which);    // count table `which` (0 / 1) in the scratch tail of the perm buffer
int bucket_counts_ints(int N);           // ints of both tables together (to clear them once per call)
int launch_gate_fold(Planes kc, Planes vct, const float* bq_s, const float* wcg, int Beff, int L, int Lpad, int Hh, int hd, int E,
                     float* cbias, float* vw, hipStream_t st);
int launch_iota_mul(int* out, int n, int mul, hipStream_t st);
int launch_router_top1(const float* logits, const float* gumbel, int N, int E, int* idx, hipStream_t st);
int launch_fill_gumbel(float* out, int B, int n_branch, int T, int width, uint64_t seed, int64_t clip_base, int nfe_base,
                       const int* step, int block, int gate, hipStream_t st);

// ---------------------------------------------------------------------------
// net_glue.hip: what the conv-net executor runs between its convolutions
// ---------------------------------------------------------------------------
// (len non-null - row lengths, vb_vae_decode_lens; device [B], in units of len_mul samples: the statistics of row b's first len[b] * len_mul
//  samples per channel, the bits of the plain form on that clip alone)
int launch_gn_stats(const float* x, int B, int C, int T, int groups, float eps, float* mean, float* rstd, hipStream_t st, const int* len = nullptr,
                    int len_mul = 1);
// (len non-null: out is zero from len[b] * len_mul on - the activated tensor ends at the row's own length)
int launch_gn_apply(const float* x, const float* mean, const float* rstd, const float* gamma, const float* beta, int B, int C, int T,
                    int groups, int swish, float* out, hipStream_t st, const int* len = nullptr, int len_mul = 1);
// transposed split planes for the DMA-fed conv path (see xt_planes_kernel): rows of the padded image
#define XT_HEAD 64
#define XT_TAIL 384
static inline int xt_rows(int T_eff) { return T_eff + XT_HEAD + XT_TAIL; }
// nplanes: 2 = split planes [2][B][xt_rows][C] (hi, lo), 1 = the round-to-nearest plane alone (the single-pass bf16 convolutions)
int launch_xt_planes(const float* x, const float* mean, const float* rstd, const float* gamma, const float* beta, int groups, int act,
                     float slope, int upsample2, int B, int C, int T_in, int nplanes, bf16_t* out, hipStream_t st, const int* len = nullptr,
                     int len_mul = 1);       // (len non-null: zero rows from position len[b] * len_mul of the - upsampled - image on)
// (len non-null: row b ends at len[b] * len_mul - both filters replicate-pad from there, nothing behind it is read, out is zero behind it)
int launch_aa_act(const float* x, const float* alpha, const float* inv_beta, const float* filt, int B, int C, int T, float* out, hipStream_t st,
                  const int* len = nullptr, int len_mul = 1);
// f32 [rows][cols] -> split-bf16 planes [2][rows][cpad] (cpad % 4 == 0, columns >= cols zero filled)
int launch_split_rows(const float* x, int64_t rows, int cols, int cpad, bf16_t* out, int64_t plane, hipStream_t st);
// (len non-null: s [B][R][R], row b's softmax over its leading len[b] * len_mul keys and queries, exact zeros elsewhere in out_t [B][R][R])
int launch_softmax_rows_t(const float* s, int B, int R, int Ccols, float* out_t, hipStream_t st, const int* len = nullptr, int len_mul = 1);
int launch_crossfade_windows(const float* parts, const int* starts, int nw, int B, int C, int n, int T, float* out, hipStream_t st);   // starts: HOST array
// chunked vocoder with row lengths (vb_hifigan_forward_chunked_lens): the rows of one chunk, by value in the kernels' argument blocks like
// LensPlan.  row[j] / n[j], j < n_active: the clip of compact row j (ascending) and its frames inside the chunk, 1 <= n[j] <= tc.
struct ChunkRows { int n_active = 0; int row[64] = {}; int n[64] = {}; };
// gather: out [n_active][C][tc], out[j][c][t] = t < n[j] ? mel[row[j]][c][lo + t] : 0 (a select: nothing behind a row's own end, nothing
// outside [lo, lo + tc) and nothing of an inactive row is read).  16-byte accesses when both bases, T, lo and tc allow, 4-byte otherwise.
int launch_chunk_gather(const float* mel, const ChunkRows& cr, int C, int T, int lo, int tc, float* out, hipStream_t st);
// scatter: wav [B][C][T*hop], samples [s*hop, e*hop) of EVERY row b: the first keep[b]*hop of them from src [n_active][C][tc*hop] at
// (s - lo)*hop of compact row slot[b], exact zeros behind them; an inactive row (slot[b] < 0 or keep[b] <= 0) is all zeros and reads
// nothing.  16-byte accesses when both bases and hop allow (every offset is a multiple of hop), 4-byte otherwise.
struct ChunkScatter { int n_active = 0; int slot[64] = {}; int keep[64] = {}; };      // (slot[b] < n_active, keep[b] in frames)
int launch_chunk_scatter(const float* src, const ChunkScatter& cs, int B, int C, int T, int hop, int s, int e, int lo, int tc, float* wav,
                         hipStream_t st);
// The VAE posterior with row lengths (vb_posterior_lens): moments [B][2E][T] = (mean, logvar), noise [B][E][T] or null (the mode),
// z[b][c][t] = t < len[b] ? scale * (mean + expf(0.5f * clamp(logvar, -30, 20)) * noise) : 0.  lp: the checked lengths by value (B = 0 in it:
// full rows).  One launch; 16-byte accesses when T % 4 == 0 and the bases allow; neither noise nor moments are read behind a row's end.
int launch_posterior_lens(const float* moments, const float* noise, int B, int E, int T, const LensPlan& lp, float scale, float* z, hipStream_t st);

// ---------------------------------------------------------------------------
// per-kernel-class HIP-event timing (bench.py roofline): 0 = bf16 GEMM (incl. the fused expert kernels), 1 = attention,
// 2 = conv1d (VAE + vocoder), 3 = fused ResBlock pair.  flops / bytes = ALGORITHMIC work of the launch (2 x MACs; operand +
// result bytes touched once), the figures DESIGN.md section 4 states per kernel.
// ---------------------------------------------------------------------------
void prof_start(int cls, double flops, double bytes, hipStream_t st);
void prof_stop(int cls, hipStream_t st);
struct ProfScope {
    int cls; hipStream_t st;
    ProfScope(int c, double flops, double bytes, hipStream_t s) : cls(c), st(s) { prof_start(c, flops, bytes, s); }
    ~ProfScope() { prof_stop(cls, st); }
};
