// DiT engine: the conditioning / workspace layouts, the once-per-clip conditioning precompute, and one network evaluation as a plan
// (dit_plan: which kernel runs, stated once) and named steps.
#include <stdlib.h>

#include "engine.h"

// ------------------------------------------------------------------------------------------
// layouts
// ------------------------------------------------------------------------------------------
#define PIN_KP 192      // K of proj_in as a GEMM: 5 taps x 32 (channels padded) = 160, padded to a multiple of 64
static inline bool gate_fold_ok(const vb_dit_config& c, int L) {
    const int NS = L * c.heads;
    return NS % 64 == 0 && NS <= 1024 && NS <= c.hidden && (c.heads & (c.heads - 1)) == 0 && c.heads <= 64 && !vb_tune().gate_unfolded;
}
CondL carve_cond(void* base, const vb_dit_config& c, int B, int nb, int T, int L) {
    CondL o;
    Carver cv(base);
    const int Beff = B * nb, D = c.hidden, hd = D / c.heads;
    o.Lpad = pad64(L);
    o.n_k = (int64_t)Beff * L * D;
    o.n_vt = (int64_t)Beff * c.heads * hd * o.Lpad;
    o.ac = cv.take<float>((size_t)B * T * D);
    o.cemb = cv.take<float>((size_t)Beff * D);
    for (int i = 0; i < c.depth; ++i) {
        o.ky[i] = cv.take<bf16_t>(o.n_k * c.np);
        o.vyt[i] = cv.take<bf16_t>(o.n_vt * c.np);
        o.kc[i] = cv.take<bf16_t>(o.n_k * c.np);
        o.vct[i] = cv.take<bf16_t>(o.n_vt * c.np);
        o.la[i] = cv.take<float>((size_t)B * T * c.num_experts);
    }
    o.NS = L * c.heads;
    o.fold = gate_fold_ok(c, L);
    o.clip_off = cv.take<int>((size_t)Beff + 1);
    for (int i = 0; i < c.depth; ++i) {
        o.mf[i] = o.fold ? cv.take<bf16_t>((size_t)Beff * o.NS * D * c.np) : nullptr;
        o.cb[i] = o.fold ? cv.take<float>((size_t)Beff * o.NS) : nullptr;
        o.vw[i] = o.fold ? cv.take<float>((size_t)Beff * o.NS * c.num_experts) : nullptr;
    }
    o.pin_w = cv.take<bf16_t>((size_t)2 * D * PIN_KP);
    o.total = cv.off;
    return o;
}

WsL carve_ws(void* base, const vb_dit_config& c, int B, int nb, int T, int L) {
    WsL o;
    Carver cv(base);
    const int Beff = B * nb, D = c.hidden, H = c.ffn_hidden, E = c.num_experts, hd = D / c.heads;
    const int64_t N = (int64_t)Beff * T;
    o.n_tok = N; o.Tpad = pad64(T); o.MODW = c.depth * 6 * D + 2 * D;
    o.n_vt = (int64_t)Beff * c.heads * hd * o.Tpad;
    o.step = cv.take<int>(16);
    o.t_idx_cur = cv.take<int64_t>(Beff);
    o.t_table = cv.take<int64_t>(1024);
    o.dt_table = cv.take<float>(1024);
    o.temb0 = cv.take<float>((size_t)Beff * D);
    o.temb = cv.take<float>((size_t)Beff * D);
    o.mod_all = cv.take<float>((size_t)Beff * o.MODW);
    o.hl = cv.take<float>((size_t)Beff * c.depth * 2);
    o.h = cv.take<float>(N * D);
    o.cq32 = cv.take<float>(N * D);
    o.mc = cv.take<float>(N);
    o.ma = cv.take<float>(N);
    o.y32 = cv.take<float>(N * D);
    o.g1 = cv.take<float>(N * 2);
    o.g2 = cv.take<float>(N * E);
    o.g3 = cv.take<float>(N * E);
    o.v = cv.take<float>((size_t)Beff * c.in_channels * T);
    o.u = cv.take<bf16_t>(N * D * c.np);
    o.q = cv.take<bf16_t>(N * D * c.np);
    o.k = cv.take<bf16_t>(N * D * c.np);
    o.vt = cv.take<bf16_t>(o.n_vt * c.np);
    o.a = cv.take<bf16_t>(N * D * c.np);
    o.qm = cv.take<bf16_t>(N * D * c.np);
    o.cqa = cv.take<bf16_t>(N * D * c.np);
    o.Hs = cv.take<bf16_t>(2 * N * H * c.np);
    o.y = cv.take<bf16_t>(N * D * c.np);
    o.Hf = cv.take<bf16_t>(N * E * H * c.np);
    o.ic = cv.take<int>(N);
    o.ia = cv.take<int>(N);
    o.group_off = cv.take<int>(2 * E + 1);
    o.perm = cv.take<int>(2 * N + bucket_scratch_ints((int)N, E));
    o.pin_a = cv.take<bf16_t>((size_t)2 * B * T * PIN_KP);
    o.pair_off = cv.take<int>(32);
    o.pair_pa = cv.take<int>(N);
    // precompute temporaries
    const int T_mel = 2 * T + 8;
    o.tA = cv.take<float>((size_t)B * D * T_mel);
    o.tB = cv.take<float>((size_t)B * D * T_mel);
    o.tC = cv.take<float>((size_t)B * D * T_mel);
    o.tD = cv.take<float>((size_t)B * D * T_mel);
    o.tE = cv.take<float>((size_t)B * D * T_mel);
    const int64_t NL = (int64_t)Beff * L;
    o.t5p = cv.take<bf16_t>(NL * c.ori_dim * 2);
    o.gel = cv.take<bf16_t>(NL * D * 2);
    o.cap_pre = cv.take<float>(NL * D);
    o.cap32 = cv.take<float>(NL * D);
    o.capp = cv.take<bf16_t>(NL * D * 2);
    o.yp = cv.take<bf16_t>(NL * D * 2);
    o.pooled = cv.take<float>((size_t)Beff * D);
    o.pooled_ln = cv.take<float>((size_t)Beff * D);
    o.temb0_s = cv.take<float>((size_t)PRE_STEPS * D);
    o.temb_s = cv.take<float>((size_t)PRE_STEPS * D);
    o.hl_s = cv.take<float>((size_t)PRE_STEPS * c.depth * 2);
    o.mod_s = cv.take<float>((size_t)PRE_STEPS * Beff * o.MODW);
    o.row_step = cv.take<int64_t>((size_t)PRE_STEPS * Beff);
    o.modA = cv.take<bf16_t>((size_t)2 * PRE_STEPS * Beff * c.hidden);
    o.tn_table = cv.take<float>(1024);
    o.len_table = cv.take<int>(64);
    o.total = cv.off;
    return o;
}

// ------------------------------------------------------------------------------------------
// plan: which kernel every step of an evaluation runs
// ------------------------------------------------------------------------------------------
// bucket counts as a side product of the router (round 5): two count tables in ping-pong - the router of block evaluation e adds into table
// e & 1, the place kernel that reads it clears table (e + 1) & 1 for the next router.  DitEval::evals_before < 0: a stand-alone call clears
// both tables itself; the sampler clears them once per call (inside the captured graph) and passes the number of block evaluations already done.
// (the tables stay right only while EVERY block evaluation of a call runs router(table e & 1) -> place(clears table (e + 1) & 1)
//  under one plan; a choice that varied between blocks or steps would need its own clear.)
static bool router_counts_eligible(int N) { return bucket_router_counts_ok(N) && !vb_tune().bucket_count_launch; }
// routed w2 as ONE launch over (caption, acoustic) pair buckets: bf16 mode, E*E <= 16 groups; otherwise the two grouped w2 launches
// (at EVERY batch size: the pair form and the two-launch form round differently - the gate weight rides in the bf16 hidden rows -
//  and a clip's bits must not depend on the batch it rides in)
static bool w2_pair_eligible(const vb_dit_config& c) {
    return c.np == 1 && c.num_experts * c.num_experts <= 16 && c.ffn_hidden % 64 == 0 && c.hidden % 16 == 0 && vb_tune().w2_pair;
}
// band experts, both products in one launch with the hidden kept in LDS (bf16 production mode; VB_BAND_UNFUSED: tuning / A-B switch, tests
// compare both)
// (a fused workgroup owns 192 tokens x one band for ~50 us whatever the batch: below ~128 workgroups - half a round of the
//  CUs, i.e. fewer than 4 clips x 2 branches - the two grouped GEMMs, bit-identical, are faster: 55.4 -> 50.4 ms per pass at
//  one clip, 69.9 -> 65.3 at two, break-even at four, profiles/r02_band_small_batch.txt)
static bool band_fused_eligible(const vb_dit_config& c, int N) {
    const int E = c.num_experts, band = c.hidden / E;
    return c.np == 1 && (band == 192 || band == 96) && c.ffn_hidden % 64 == 0 && E <= 8 && 8 % E == 0 && !vb_tune().band_unfused &&
           (int64_t)cdiv(N, band_ffn_tile_rows(band)) * E >= 128;
}
// proj_in reads the split-plane weights (as a GEMM operand, or in the conv kernel under VB_PROJ_IN_CONV)
static bool proj_in_split_w_eligible(const vb_dit_config& c, const vb_dit_weights& w) { return w.proj_in_w3 && c.in_channels <= 32; }
// scores + router in one launch (score_router.hip: the [N][NS] score matrix stays in LDS; bit-identical to the two launches).
// MEASURED SLOWER - 91 us against 32 + 22 at 8 clips: its mainloop runs 36 us with one 4-wave workgroup per CU and the
// router's per-token wave-wide shuffles take 63 us without many waves per SIMD to hide them - so it is an opt-in experiment
// (VB_SCORE_FUSED=1), kept with its test as the record.
static bool score_fused_eligible(const vb_dit_config& c, int Beff, int T, int L) {
#ifdef VB_EXPERIMENTS
    return c.np == 1 && vb_tune().score_fused && score_router_supported(L * c.heads, c.hidden, c.num_experts, c.heads) && (int64_t)Beff * cdiv(T, 64) >= 96;
#else
    return false;
#endif
}
// the product form of that fusion (gate_route.hip): softmax and value/gate contraction lane-local in the MFMA's accumulator layout, no score
// matrix in memory, bit-identical to the two launches - so the choice may follow the token count.  bf16 mode, fold layout, 80 keys x 8 heads,
// 4 experts, hidden 768; everything else keeps score GEMM + router.  VB_GATE_ROUTE=0: the two launches (tests, A/B); =1: fused at every count.
// MEASURED (8 clips x 2 branches, one stream, same box, parent / head alternating): 40.3 / 40.1 us per launch against 25.7 + 17.8 and
// 25.9 + 17.9 us of score GEMM + router - 3.4 us (8 %) less, the parent's own spread being 0.3 us; well short of the 20-28 us the kernel was
// sized for, and too little to show in the whole benchmark (profiles/r16_gate_route_ab.txt).  Fetches 34 MB (tokens + folded keys), writes
// 0.4 MB where the two launches wrote 31.5 MB and read them back (docs/history.md).  The launch is one round of one workgroup per CU and
// takes its ~40 us at any batch, while the two launches shrink with the token count: at one clip x 2 branches (24 tiles) the whole
// benchmark ran 45.0 against 41.4 ms per step with it, ~18 us per block evaluation MORE.  Measured to win: 192 tiles (per launch, above) and
// 96 tiles (4 clips x 2 branches per stream, the default command: median 1242.9 against the parent's 1227.7-1240.5 mel-s/s); 48 tiles
// were not measured and stay with the two launches.
constexpr int GATE_ROUTE_MIN_TILES = 96;     // 64-token tiles (= workgroups) from which the one launch is taken
static bool gate_route_eligible(const vb_dit_config& c, int Beff, int T, int L) {
    if (c.np != 1 || !gate_fold_ok(c, L) || !gate_route_supported(L * c.heads, c.hidden, c.num_experts, c.heads)) return false;
    const int knob = vb_tune().gate_route;
    return knob >= 0 ? knob != 0 : (int64_t)Beff * cdiv(T, 64) >= GATE_ROUTE_MIN_TILES;
}
// FinalLayer form.  FINAL_EULER_FUSED is what the sampler's evaluations take (both CFG branches in the batch, VB_EULER_LAUNCH off); VB_FINAL_GEMM=1
// selects the split-planes kernel + MFMA GEMM the fused kernel replaced (tests compare them)
static FinalRoute final_route(const vb_dit_config& c, const vb_dit_weights& w, int nb, int N) {
    if (w.final_w && final_layer_fused_ok(c.hidden, c.in_channels) && !vb_tune().final_gemm)
        return nb == 2 && !vb_tune().euler_launch ? FINAL_EULER_FUSED : FINAL_FUSED;
    if (w.final_wp && c.in_channels % 4 == 0 && (int64_t)2 * N * c.ffn_hidden >= (int64_t)N * c.hidden) return FINAL_GEMM;
    return FINAL_ROWS;
}
DitPlan dit_plan(const vb_ctx* ctx, int B, int nb, int T, int L, int nb_active) {
    const vb_dit_config& c = ctx->cfg;
    const int nba = nb_active > 0 ? nb_active : nb;
    const int Beff = B * nba, N = Beff * T;          // the rows the launches count
    DitPlan p;
    p.w = &ctx->w;
    // the layout (model, knobs and L alone: the same for every nb_active)
    p.w2_pair = w2_pair_eligible(c);
    p.proj_in_split_w = proj_in_split_w_eligible(c, ctx->w);
    p.proj_in_gemm = p.proj_in_split_w && !vb_tune().proj_in_conv;
    p.fold_layout = gate_fold_ok(c, L);
    // kernels picked from the token count: the active rows
    p.router_counts = router_counts_eligible(N);
    p.band_fused = band_fused_eligible(c, N);
    p.score_fused = score_fused_eligible(c, Beff, T, L);
    p.gate_route = !p.score_fused && gate_route_eligible(c, Beff, T, L);
    p.final_route = final_route(c, ctx->w, nba, N);
    return p;
}

// ------------------------------------------------------------------------------------------
// DiT: conditioning precompute
// ------------------------------------------------------------------------------------------
// acoustic stem (vocal2music_moe.py:388-393) -> cd.ac
// lens (device [B], null: none): the embeddings are zero from mel position 2 * len[b] on, so the k5p2 convolutions see the zero padding of
// the clip alone; the pool and the 1x1 projection are position-local
static int precompute_acoustic(const vb_dit_config& c, const vb_dit_weights& w, const int64_t* midi, const int64_t* beats, int B, int T, int T_mel,
                               const int* lens, const CondL& cd, const WsL& s, hipStream_t st) {
    const int D = c.hidden, T_ac = T_mel / 2;
    ConvArgs cv;
    for (int which = 0; which < 2; ++which) {
        VB_TRY(launch_embed_t(which ? beats : midi, which ? w.beats_emb : w.midi_emb, B, T_mel, D, which ? 3 : 130, s.tA, st, lens, 2));   // Embedding(3) / Embedding(130), vocal2music_moe.py:337-350
        cv = ConvArgs();
        cv.x = s.tA; cv.x_bstride = (int64_t)D * T_mel; cv.Ci = D; cv.T_in = T_mel;
        cv.w = which ? w.beats_conv_w : w.midi_conv_w; cv.bias = which ? w.beats_conv_b : w.midi_conv_b;
        cv.Co = D; cv.ksize = 5; cv.pad = 2; cv.out = which ? s.tC : s.tB; cv.out_bstride = (int64_t)D * T_mel; cv.T_out = T_mel;
        cv.out_act = ACT_LRELU; cv.out_slope = 0.01f; cv.B = B;
        if (const void* w3 = which ? w.beats_conv_w3 : w.midi_conv_w3; w3 && D % 32 == 0 && !vb_tune().stem_f32) {
            cv.wp = (const bf16_t*)w3; cv.Ci_pad = D; cv.wp_plane = (int64_t)5 * D * D;
        }
        VB_TRY(launch_conv1d(cv, st));
    }
    VB_TRY(launch_pool_add(s.tB, s.tC, B, D, T_mel, s.tD, st));
    cv = ConvArgs();
    cv.x = s.tD; cv.x_bstride = (int64_t)D * T_ac; cv.Ci = D; cv.T_in = T_ac; cv.w = w.final_proj_w; cv.bias = w.final_proj_b;
    cv.Co = D; cv.ksize = 1; cv.pad = 0; cv.out = s.tE; cv.out_bstride = (int64_t)D * T_ac; cv.T_out = T_ac; cv.B = B;
    if (w.final_proj_w3 && D % 32 == 0 && !vb_tune().stem_f32) { cv.wp = (const bf16_t*)w.final_proj_w3; cv.Ci_pad = D; cv.wp_plane = (int64_t)D * D; }
    VB_TRY(launch_conv1d(cv, st));
    return launch_transpose_bct_btc(s.tE, B, D, T_ac, T, cd.ac, st);
}
// caption embedding (ConditionEmbedder, flag_large_dit_moe.py:149-160) in split precision -> s.cap32 / s.capp, pooled caption -> cd.cemb
static int precompute_caption(const vb_dit_config& c, const vb_dit_weights& w, const float* t5, int Beff, int L, const CondL& cd, const WsL& s,
                              hipStream_t st) {
    const int D = c.hidden;
    const int64_t NL = (int64_t)Beff * L;
    Planes t5p = mkp(s.t5p, NL * c.ori_dim, 2);
    VB_TRY(launch_cast_planes(t5, NL * c.ori_dim, t5p, st));
    GemmArgs g = gemm_operands(t5p.p, t5p.plane, c.ori_dim, w.c_emb0, (int64_t)D * c.ori_dim, c.ori_dim, (int)NL, D, c.ori_dim, 3);
    g.epi = EPI_GELU_PLANES; g.bias = w.c_emb0_b; g.out = mkp(s.gel, NL * D, 2); g.ldc = D;
    VB_TRY(launch_gemm(g, st));
    g = gemm_operands(s.gel, NL * D, D, w.c_emb2, (int64_t)D * D, D, (int)NL, D, D, 3);
    g.epi = EPI_F32; g.bias = w.c_emb2_b; g.out32 = s.cap_pre; g.ldc32 = D;
    VB_TRY(launch_gemm(g, st));
    VB_TRY(launch_layernorm(s.cap_pre, w.c_ln_w, w.c_ln_b, (int)NL, D, 1e-5f, s.cap32, mkp(s.capp, NL * D, 2), st));
    // pooled caption -> cap_embedder (vocal2music_moe.py:367-370,410-413)
    VB_TRY(launch_mean_rows(s.cap32, Beff, L, D, s.pooled, st));
    VB_TRY(launch_layernorm(s.pooled, w.cap_ln_w, w.cap_ln_b, Beff, D, 1e-5f, s.pooled_ln, Planes{nullptr, 0, 1}, st));
    return launch_gemv_rows(s.pooled_ln, D, nullptr, 0, 1, w.cap_lin_w, w.cap_lin_b, Beff, D, D, 0, cd.cemb, D, st);
}
static int dit_precompute(vb_ctx* ctx, const float* t5, const int64_t* midi, const int64_t* beats, int B, int nb, int T, int T_mel,
                          int L, const LensPlan& lp, void* cond, void* ws, hipStream_t st) {
    const vb_dit_config& c = ctx->cfg;
    const vb_dit_weights& w = ctx->w;
    if (T_mel > 2 * T + 8) VB_FAIL(VB_E_INVALID, "precompute: T_mel=%d too long for T=%d", T_mel, T);
    const int T_ac = T_mel / 2;
    if (abs(T - T_ac) > 2) VB_FAIL(VB_E_INVALID, "precompute: latent length %d vs conditioning length %d differ by more than 2 "
                                   "(vocal2music_moe.py:397 would leave the shapes mismatched)", T, T_ac);
    const DitPlan p = dit_plan(ctx, B, nb, T, L);
    CondL cd = carve_cond(cond, c, B, nb, T, L);
    WsL s = carve_ws(ws, c, B, nb, T, L);
    const int Beff = B * nb, D = c.hidden, E = c.num_experts, hd = D / c.heads, np = c.np;
    const int64_t NL = (int64_t)Beff * L;
    if (lp.B) VB_TRY(launch_lens_table(lp, s.len_table, st));
    VB_TRY(precompute_acoustic(c, w, midi, beats, B, T, T_mel, lp.B ? s.len_table : nullptr, cd, s, st));
    VB_TRY(precompute_caption(c, w, t5, Beff, L, cd, s, st));

    // ---- per block: context K/V for Attention and MoE.cross_attention, acoustic gate logits
    for (int i = 0; i < c.depth; ++i) {
        const vb_dit_block_weights& bw = w.blocks[i];
        Planes yp = mkp(s.yp, NL * D, 2);
        VB_TRY(launch_rmsnorm_mod(s.cap32, bw.y_norm_w, nullptr, nullptr, 0, (int)NL, D, L, c.norm_eps, yp, st));
        VB_HIP(hipMemsetAsync(cd.vyt[i], 0, (size_t)cd.n_vt * np * sizeof(bf16_t), st));
        VB_HIP(hipMemsetAsync(cd.vct[i], 0, (size_t)cd.n_vt * np * sizeof(bf16_t), st));
        for (int which = 0; which < 4; ++which) {
            // 0: ky = y Wk_y^T   1: vy^T   2: kc = cap Wk^T + bk   3: vc^T
            const void* W = which == 0 ? bw.wky : which == 1 ? bw.wvy : which == 2 ? bw.wk_m : bw.wv_m;
            GemmArgs g = gemm_operands(which < 2 ? yp.p : s.capp, NL * D, D, W, (int64_t)D * D, D, (int)NL, D, D, 3);
            g.bias = which == 2 ? bw.bk_m : which == 3 ? bw.bv_m : nullptr;
            if (which == 0 || which == 2) {
                g.epi = EPI_PLANES; g.out = mkp(which == 0 ? cd.ky[i] : cd.kc[i], cd.n_k, np); g.ldc = D;
            } else {
                g.epi = EPI_HEADS_T; g.out = mkp(which == 1 ? cd.vyt[i] : cd.vct[i], cd.n_vt, np);
                g.T = L; g.H = c.heads; g.hd = hd; g.Tpad = cd.Lpad;
            }
            VB_TRY(launch_gemm(g, st));
        }
        VB_TRY(launch_rows_dot(cd.ac, bw.wag, bw.bag, B * T, D, E, cd.la[i], st));
        if (p.gate_fold(i)) {
            // Mf[b][key*heads + head][:] = hd^-1/2 * sum_d Kc[b][key][head*hd + d] * Wq[head*hd + d][:]   (one launch, head = grid z)
            GemmArgs g = gemm_operands(cd.kc[i], cd.n_k, D, bw.wqt_s, (int64_t)D * D, D, (int)NL, D, hd, np == 2 ? 3 : 1);
            g.a_koff_group = hd; g.b_group_stride = hd; g.ngroups = c.heads;
            g.epi = EPI_PLANES; g.out = mkp(cd.mf[i], (int64_t)Beff * cd.NS * D, np); g.ldc = c.heads * D; g.c_noff_group = D;
            VB_TRY(launch_gemm(g, st));
            VB_TRY(launch_gate_fold(mkp(cd.kc[i], cd.n_k, np), mkp(cd.vct[i], cd.n_vt, np), bw.bq_s, bw.wcg, Beff, L, cd.Lpad, c.heads, hd, E,
                                    cd.cb[i], cd.vw[i], st));
        }
    }
    VB_TRY(launch_iota_mul(cd.clip_off, Beff + 1, T, st));
    if (p.proj_in_split_w)
        VB_TRY(launch_conv_w_to_gemm((const bf16_t*)w.proj_in_w3, (int64_t)5 * D * 32, 5, D, PIN_KP, cd.pin_w, st));
    return VB_OK;
}

// ------------------------------------------------------------------------------------------
// DiT: one evaluation (both CFG branches batched: rows [0,B) cond, [B,2B) uncond; DitEval::nb_active = 1 beside nb = 2: the
// conditional rows alone, in the two-branch layout)
// ------------------------------------------------------------------------------------------
// what the steps of one evaluation share
struct Eval {
    const vb_dit_config& c; const vb_dit_weights& w; const DitEval& ev; hipStream_t st;
    const DitPlan p; const CondL cd; const WsL s;
    const int Beff, D, H, E, hd, np, nseg, N, MODW, band;     // Beff, N: the ACTIVE rows / tokens - what every launch counts
    const int BeffL, NL;                                      // rows / tokens of the layout (ev.nb): strides, table offsets
    const int64_t ND;                                         // plane stride of the [N][D] bf16 buffers (layout)
    const int eval0;                                          // block evaluations before this one: block i's router counts into table (eval0 + i) & 1
    const float* mod_all; const float* hl; int hl_ld;        // this evaluation's adaLN modulations and high-level gate logits (conditioning_vectors)
    Planes u, q, k, vt, a, qm, cqa, Hs, y, Hf;
    Eval(vb_ctx* ctx, const DitEval& e, hipStream_t stream)
        : c(ctx->cfg), w(ctx->w), ev(e), st(stream), p(dit_plan(ctx, e.B, e.nb, e.T, e.L, e.nb_active)),
          cd(carve_cond(const_cast<void*>(e.cond), ctx->cfg, e.B, e.nb, e.T, e.L)), s(carve_ws(e.ws, ctx->cfg, e.B, e.nb, e.T, e.L)),
          Beff(e.B * (e.nb_active > 0 ? e.nb_active : e.nb)), D(c.hidden), H(c.ffn_hidden), E(c.num_experts), hd(D / c.heads), np(c.np),
          nseg(np == 2 ? 3 : 1), N(Beff * e.T), MODW(s.MODW), band(D / E), BeffL(e.B * e.nb), NL((int)s.n_tok), ND((int64_t)NL * D),
          eval0(e.evals_before < 0 ? 0 : e.evals_before),
          mod_all(s.mod_all), hl(s.hl), hl_ld(c.depth * 2),
          u(mkp(s.u, ND, np)), q(mkp(s.q, ND, np)), k(mkp(s.k, ND, np)), vt(mkp(s.vt, s.n_vt, np)), a(mkp(s.a, ND, np)), qm(mkp(s.qm, ND, np)),
          cqa(mkp(s.cqa, ND, np)), Hs(mkp(s.Hs, (int64_t)2 * NL * H, np)), y(mkp(s.y, ND, np)), Hf(mkp(s.Hf, (int64_t)NL * E * H, np)) {}
    const float* mod(int i) const { return mod_all + (size_t)i * 6 * D; }      // shift_msa, scale_msa, gate_msa, shift_mlp, scale_mlp, gate_mlp
    float scale() const { return 1.0f / sqrtf((float)hd); }
    int* counts(int i) const { return bucket_counts(s.perm, NL, (eval0 + i) & 1); }      // (where the layout puts them, whatever the active rows)
};

// timestep embedding + all adaLN modulations + high-level gate logits (depend on (t, caption) only)
// (the sampler tabulates them for all steps up front and passes this step's rows in pre_mod / pre_hl)
static int conditioning_vectors(Eval& e) {
    const vb_dit_config& c = e.c; const vb_dit_weights& w = e.w; const WsL& s = e.s;
    const int Beff = e.Beff, D = e.D, MODW = e.MODW;
    if (e.ev.pre_mod) {
        e.mod_all = e.ev.pre_mod; e.hl = e.ev.pre_hl; e.hl_ld = 0;
        return VB_OK;
    }
    VB_TRY(launch_gemv_rows_idx(w.t_freq_table, 256, e.ev.t_idx, nullptr, 0, 1, w.t_mlp0_w, w.t_mlp0_b, Beff, D, 256, 0, s.temb0, D, e.st, T_FREQ_ROWS));
    VB_TRY(launch_gemv_rows(s.temb0, D, nullptr, 0, 1, w.t_mlp2_w, w.t_mlp2_b, Beff, D, D, 1, s.temb, D, e.st));
    VB_TRY(launch_gemv_rows(s.temb, D, e.cd.cemb, D, Beff, w.adaln_w, w.adaln_b, Beff, MODW, D, 1, s.mod_all, MODW, e.st));
    return launch_gemv_rows(s.temb, D, nullptr, 0, 1, w.hl_w, w.hl_b, Beff, c.depth * 2, D, 0, s.hl, c.depth * 2, e.st);
}

// h = proj_in(x)^T + acoustic   (vocal2music_moe.py:395,415)
// As a GEMM (round 3): the k = 5 convolution over 20 channels is a K = 100 product per token - as a conv launch it was 1152 workgroups
// each staging 80 KB of weights for 60 MFMAs per wave (79 us per evaluation, 0.7 TB/s of output).  The latent windows are laid out as
// K-contiguous split planes (im2col, 6016 x 192 at 8 clips), multiplied with the re-laid conv weights in split precision (fp32-class,
// as before), + bias + acoustic embedding in the epilogue, and the row is written for BOTH CFG branches (they embed the same x).
static int embed_latent(const Eval& e) {
    const vb_dit_config& c = e.c; const vb_dit_weights& w = e.w; const WsL& s = e.s;
    const int B = e.ev.B, T = e.ev.T, D = e.D;
    if (e.p.proj_in_gemm) {
        const int BT = B * T;
        VB_TRY(launch_im2col_latent(e.ev.x, B, c.in_channels, T, 5, 2, PIN_KP, s.pin_a, (int64_t)BT * PIN_KP, e.st, e.ev.lens));
        GemmArgs g = gemm_operands(s.pin_a, (int64_t)BT * PIN_KP, PIN_KP, e.cd.pin_w, (int64_t)D * PIN_KP, PIN_KP, BT, D, PIN_KP, 3);
        g.epi = EPI_F32; g.bias = w.proj_in_b; g.out32 = s.h; g.ldc32 = D;
        g.add32 = e.cd.ac; g.dup_rows = e.Beff == 2 * B ? BT : 0; g.prof_class = 2;       // split-precision convolution work: counted with the conv class
        return launch_gemm(g, e.st);
    }
    // a general convolution kernel: with row lengths it reads a masked copy of x (in the im2col buffer, which this route leaves free)
    const float* x = e.ev.x;
    if (e.ev.lens) {
        float* xm = reinterpret_cast<float*>(s.pin_a);
        VB_TRY(launch_mask_latent(x, B, c.in_channels, T, e.ev.lens, xm, e.st));
        x = xm;
    }
    ConvArgs cv;
    cv.x = x; cv.x_bstride = (int64_t)c.in_channels * T; cv.Ci = c.in_channels; cv.T_in = T; cv.x_bmod = B;
    cv.w = w.proj_in_w; cv.bias = w.proj_in_b; cv.Co = D; cv.ksize = 5; cv.pad = 2;
    if (e.p.proj_in_split_w) { cv.wp = (const bf16_t*)w.proj_in_w3; cv.Ci_pad = 32; cv.wp_plane = (int64_t)5 * D * 32; }
    cv.out = s.h; cv.out_bstride = (int64_t)T * D; cv.T_out = T; cv.out_transposed = 1;
    cv.add = e.cd.ac; cv.add_bstride = (int64_t)T * D; cv.add_bmod = B; cv.B = e.Beff;
    return launch_conv1d(cv, e.st);
}

// attention (flag_large_dit_moe.py:323-406): h += gate_msa * Wo attn(q, k, v | y),  q/k/v from the modulated RMSNorm of h
static int attention_half(const Eval& e, int i) {
    const vb_dit_config& c = e.c; const vb_dit_block_weights& bw = e.w.blocks[i]; const WsL& s = e.s; const CondL& cd = e.cd;
    const int T = e.ev.T, D = e.D, N = e.N, MODW = e.MODW, np = e.np;
    const float* mod = e.mod(i);
    VB_TRY(launch_rmsnorm_mod(s.h, bw.attn_norm_w, mod, mod + D, MODW, N, D, T, c.norm_eps, e.u, e.st));
    GemmArgs g = gemm_operands(e.u.p, e.ND, D, bw.wqkv, (int64_t)3 * D * D, D, N, 3 * D, D, e.nseg);
    g.epi = EPI_QKV_ROPE; g.q = e.q; g.k = e.k; g.vt = e.vt;
    g.rope_cos = e.w.rope_cos; g.rope_sin = e.w.rope_sin; g.H = c.heads; g.hd = e.hd; g.Tpad = s.Tpad; g.D = D; g.T = T;
    VB_TRY(launch_gemm(g, e.st));
    AttnArgs at;
    at.q = e.q; at.k = e.k; at.vt = e.vt; at.ky = mkp(cd.ky[i], cd.n_k, np); at.vyt = mkp(cd.vyt[i], cd.n_vt, np);
    at.cross_w = bw.cross_w; at.out = e.a; at.B = e.Beff; at.T = T; at.Tpad = s.Tpad; at.L = e.ev.L; at.Lpad = cd.Lpad; at.H = c.heads;
    at.hd = e.hd; at.has_self = 1; at.has_cross = 1; at.kv_batch_mod = 0; at.scale = e.scale();
    at.key_len = e.ev.lens; at.key_len_mod = e.ev.B;
    VB_TRY(launch_attention(at, e.st));
    g = gemm_operands(e.a.p, e.ND, D, bw.wo, (int64_t)D * D, D, N, D, D, e.nseg);
    g.epi = EPI_RESID_GATE; g.out32 = s.h; g.ldc32 = D; g.gate = mod + 2 * D; g.gate_ld = MODW; g.T = T;
    return launch_gemm(g, e.st);
}

// gate noise of block i: injected Gumbel arrays (parity path) or, all null, counter-based draws generated inside the router kernel
struct GateNoise { const float* g1 = nullptr; const float* g2 = nullptr; const float* g3 = nullptr; };
static GateNoise gate_noise(const Eval& e, int i) {
    GateNoise n;
    if (const vb_noise* nz = e.ev.noise; nz && nz->g1) {
        const size_t so = (size_t)e.ev.noise_step * e.c.depth + i;
        n.g1 = nz->g1 + so * e.NL * 2; n.g2 = nz->g2 + so * e.NL * e.E; n.g3 = nz->g3 + so * e.NL * e.E;      // (arrays of the layout; the conditional rows come first)
    }
    return n;
}
// the router's argument block for block i, as far as launch_router and the fused score + router kernel share it
static RouterDev router_args(const Eval& e, int i) {
    const vb_dit_block_weights& bw = e.w.blocks[i]; const WsL& s = e.s; const vb_noise* noise = e.ev.noise;
    const GateNoise gn = gate_noise(e, i);
    RouterDev r;
    r.bg = bw.bcg; r.la = e.cd.la[i]; r.la_rows = e.ev.B * e.ev.T; r.hl = e.hl + i * 2; r.hl_ld = e.hl_ld;
    r.g1 = gn.g1; r.g2 = gn.g2; r.g3 = gn.g3; r.T = e.ev.T; r.E = e.E; r.B = e.ev.B; r.ic = s.ic; r.ia = s.ia; r.mc = s.mc; r.ma = s.ma;
    r.seed = noise ? noise->seed : 0; r.clip_base = noise ? noise->clip_base : 0; r.nfe_base = noise ? noise->nfe : 0;
    r.step = e.ev.step_ptr; r.block = i; r.NS = e.cd.NS; r.Hh = e.c.heads; r.clip_rows = e.ev.clip_rows;
    return r;
}
// the one-launch forms' arguments: the GEMM side + the router's block (with the count table: launch_score_router ignores it)
static ScoreRouterArgs score_router_args(const Eval& e, int i) {
    const CondL& cd = e.cd;
    ScoreRouterArgs sr;
    sr.A = e.u.p; sr.lda = e.D; sr.Bm = cd.mf[i]; sr.ldb = e.D; sr.bias = cd.cb[i]; sr.K = e.D; sr.Beff = e.Beff;
    sr.r = router_args(e, i); sr.r.Wg = cd.vw[i];
    sr.r.cnt = e.p.router_counts ? e.counts(i) : nullptr; sr.r.cnt_G = e.p.w2_pair ? e.E * e.E : 2 * e.E; sr.r.cnt_pairs = e.p.w2_pair ? 1 : 0;
    return sr;
}
// Band-MoE gates (vocal2music_moe.py:117-151): modulated RMSNorm of h -> u, caption-gate logits, routing decisions (s.ic / s.ia / s.mc / s.ma)
// and the expert buckets of launch_bucket
static int caption_gate_and_route(const Eval& e, int i) {
    const vb_dit_config& c = e.c; const vb_dit_block_weights& bw = e.w.blocks[i]; const WsL& s = e.s; const CondL& cd = e.cd;
    const int T = e.ev.T, D = e.D, N = e.N, E = e.E, np = e.np;
    const float* mod = e.mod(i);
    VB_TRY(launch_rmsnorm_mod(s.h, bw.ffn_norm_w, mod + 3 * D, mod + 4 * D, e.MODW, N, D, T, c.norm_eps, e.u, e.st));
    const bool fold = e.p.gate_fold(i), fused_router = fold && e.p.score_fused;
    if (fused_router) {
#ifdef VB_EXPERIMENTS
        VB_TRY(launch_score_router(score_router_args(e, i), e.st));
#endif
    } else if (fold && e.p.gate_route) {
        VB_TRY(launch_gate_route(score_router_args(e, i), e.st));
    } else {
        if (fold) {
            // caption gate, folded: scores of every token against its clip's caption keys for all heads in ONE grouped GEMM
            // (q-projection, q-bias and softmax scale live in the per-clip operand), then softmax + value/gate contraction +
            // routing in the router kernel.  Replaces q-projection GEMM + cross-attention launch + 768-wide gate dot.
            GemmArgs g = gemm_operands(e.u.p, e.ND, D, cd.mf[i], (int64_t)e.BeffL * cd.NS * D, D, N, cd.NS, D, e.nseg);
            g.b_group_stride = (int64_t)cd.NS * D; g.ngroups = e.Beff; g.group_off = cd.clip_off; g.group_rows = T;
            g.epi = EPI_F32; g.bias = cd.cb[i]; g.bias_group_stride = cd.NS; g.out32 = s.y32; g.ldc32 = cd.NS;
            VB_TRY(launch_gemm(g, e.st));
        } else {
            GemmArgs g = gemm_operands(e.u.p, e.ND, D, bw.wq_m, (int64_t)D * D, D, N, D, D, e.nseg);
            g.epi = EPI_PLANES; g.bias = bw.bq_m; g.out = e.qm; g.ldc = D;
            VB_TRY(launch_gemm(g, e.st));
            AttnArgs at = AttnArgs();
            at.q = e.qm; at.k = Planes{nullptr, 0, np}; at.vt = Planes{nullptr, 0, np}; at.ky = mkp(cd.kc[i], cd.n_k, np);
            at.vyt = mkp(cd.vct[i], cd.n_vt, np); at.cross_w = nullptr; at.out = e.cqa; at.B = e.Beff; at.T = T; at.Tpad = s.Tpad; at.L = e.ev.L;
            at.Lpad = cd.Lpad; at.H = c.heads; at.hd = e.hd; at.has_self = 0; at.has_cross = 1; at.kv_batch_mod = 0; at.scale = e.scale();
            VB_TRY(launch_attention(at, e.st));
        }
        // (MoE.cross_attention.out_proj is folded into the caption gate at pack time: lc = cqa . (Wcg Wo)^T + (Wcg bo + bcg),
        //  so the [N,768]x[768,768] out_proj GEMM never runs - its only consumer is the 768->E gate, vocal2music_moe.py:119-141)
        RouterDev r = router_args(e, i);
        r.cq = e.cqa; r.Wg = fold ? cd.vw[i] : bw.wcg; r.N = N; r.D = D; r.sc = fold ? s.y32 : nullptr;
        r.cnt = e.p.router_counts ? e.counts(i) : nullptr; r.cnt_G = e.p.w2_pair ? E * E : 2 * E; r.cnt_pairs = e.p.w2_pair ? 1 : 0;
        VB_TRY(launch_router(r, e.st));
    }
    const bool rc = e.p.router_counts && !fused_router;       // (the fused score + router kernel does not count)
    VB_TRY(launch_bucket(s.ic, s.ia, N, E, s.group_off, s.perm, e.st, e.p.w2_pair ? s.pair_off : nullptr, s.pair_pa,
                         rc ? e.counts(i) : nullptr, rc ? e.counts(i + 1) : nullptr));
    if (int32_t* route_out = e.ev.route_out) {
        VB_HIP(hipMemcpyAsync(route_out + ((size_t)i * 2 + 0) * N, s.ic, (size_t)N * sizeof(int), hipMemcpyDeviceToDevice, e.st));
        VB_HIP(hipMemcpyAsync(route_out + ((size_t)i * 2 + 1) * N, s.ia, (size_t)N * sizeof(int), hipMemcpyDeviceToDevice, e.st));
    }
    return VB_OK;
}

// routed experts (vocal2music_moe.py:152-185): y = m_c * FFN^c(u) + m_a * FFN^a(u), hidden = silu(u W1^T) * (u W3^T) for both groups in
// one grouped launch
static int routed_experts(const Eval& e, int i) {
    const vb_dit_block_weights& bw = e.w.blocks[i]; const WsL& s = e.s;
    const int D = e.D, H = e.H, N = e.N, E = e.E;
    GemmArgs g = gemm_operands(e.u.p, e.ND, D, bw.w13, (int64_t)2 * E * 2 * H * D, D, 2 * N, 2 * H, D, e.nseg);
    g.a_rows = s.perm; g.b_group_stride = (int64_t)2 * H * D; g.ngroups = 2 * E; g.group_off = s.group_off;
    g.epi = EPI_SWIGLU; g.out = e.Hs; g.ldc = H;
    if (e.p.w2_pair) { g.row_scale = s.mc; g.row_scale2 = s.ma; g.scale_split = N; }      // gate weights ride in the hidden rows
    VB_TRY(launch_gemm(g, e.st));
    if (e.p.w2_pair) {
        MoeW2PairArgs pw;
        pw.Hs = e.Hs.p; pw.W2 = (const bf16_t*)bw.w2; pw.pair_off = s.pair_off; pw.perm = s.perm; pw.pair_pa = s.pair_pa;
        pw.out = e.y.p; pw.N = N; pw.D = D; pw.H = H; pw.E = E;
        return launch_moe_w2_pair(pw, e.st);
    }
    // y = m_c * FFN^c(u)  (store), then y += m_a * FFN^a(u) (planes out)
    g = gemm_operands(e.Hs.p, e.Hs.plane, H, bw.w2, (int64_t)2 * E * D * H, H, N, D, H, e.nseg);
    g.b_group_stride = (int64_t)D * H; g.ngroups = E; g.group_off = s.group_off;
    g.epi = EPI_SCATTER_F32; g.out32 = s.y32; g.ldc32 = D; g.rows_out = s.perm; g.row_scale = s.mc;
    VB_TRY(launch_gemm(g, e.st));
    g.B = (const bf16_t*)bw.w2 + (int64_t)E * D * H; g.group_off = s.group_off + E; g.epi = EPI_SCATTER_ADD_PLANES;
    g.y32_in = s.y32; g.row_scale = s.ma; g.out = e.y; g.ldc = D;
    return launch_gemm(g, e.st);
}

// band experts (frequency-MoE): expert e sees only channel band e and produces only band e;  h += gate_mlp * FFN_e(y_e)
static int band_experts(const Eval& e, int i) {
    const vb_dit_block_weights& bw = e.w.blocks[i]; const WsL& s = e.s;
    const int T = e.ev.T, D = e.D, H = e.H, N = e.N, E = e.E, MODW = e.MODW, band = e.band;
    const float* gate = e.mod(i) + 5 * D;
    if (e.p.band_fused) {
        BandFfnArgs bf;
        bf.y = e.y.p; bf.ldy = D; bf.w13 = (const bf16_t*)bw.w13f; bf.w2 = (const bf16_t*)bw.w2f; bf.M = N; bf.H = H; bf.E = E;
        bf.band = band; bf.out32 = s.h; bf.ldc32 = D; bf.gate = gate; bf.gate_ld = MODW; bf.T = T;
        return launch_band_ffn(bf, e.st);
    }
    GemmArgs g = gemm_operands(e.y.p, e.ND, D, bw.w13f, (int64_t)E * 2 * H * band, band, N, 2 * H, band, e.nseg);
    g.a_koff_group = band; g.b_group_stride = (int64_t)2 * H * band; g.ngroups = E;
    g.epi = EPI_SWIGLU; g.out = e.Hf; g.ldc = E * H; g.c_noff_group = H;
    VB_TRY(launch_gemm(g, e.st));
    g = gemm_operands(e.Hf.p, e.Hf.plane, E * H, bw.w2f, (int64_t)E * band * H, H, N, band, H, e.nseg);
    g.a_koff_group = H; g.b_group_stride = (int64_t)band * H; g.ngroups = E;
    g.epi = EPI_RESID_GATE; g.out32 = s.h; g.ldc32 = D; g.c_noff_group = band; g.gate = gate; g.gate_ld = MODW; g.T = T;
    return launch_gemm(g, e.st);
}

// FinalLayer (vocal2music_moe.py:287-291) -> v [Beff][C][T]
static int final_layer(const Eval& e) {
    const vb_dit_config& c = e.c; const vb_dit_weights& w = e.w; const WsL& s = e.s;
    const int T = e.ev.T, D = e.D, N = e.N, MODW = e.MODW;
    float* v_out = e.ev.v_out;
    const float* modf = e.mod_all + (size_t)c.depth * 6 * D;
    const EulerStep* es = e.ev.euler;
    switch (e.p.final_route == FINAL_EULER_FUSED && !es ? FINAL_FUSED : e.p.final_route) {
    case FINAL_EULER_FUSED:
        return launch_final_layer_euler(s.h, modf, modf + D, MODW, w.final_w, w.final_b, N, D, T, c.in_channels, 1e-6f, *es, e.st);
    case FINAL_FUSED:
        // one wave per token row: LayerNorm + modulate in registers, the 768 x 20 projection against LDS-resident weights (exact fp32)
        return launch_final_layer_fused(s.h, modf, modf + D, MODW, w.final_w, w.final_b, N, D, T, c.in_channels, 1e-6f, v_out, e.st);
    case FINAL_GEMM: {
        // LN + modulate -> split planes (plane 0 in u, plane 1 in the free expert-hidden buffer), then the projection on the MFMA
        // GEMM in split precision (fp32-class in both modes) with a channel-major epilogue: 62 us -> ~35 us per evaluation
        Planes ln{s.u, (int64_t)(s.Hs - s.u), 2};
        VB_TRY(launch_layernorm_mod_planes(s.h, modf, modf + D, MODW, N, D, T, 1e-6f, ln, e.st));
        GemmArgs g = gemm_operands(ln.p, ln.plane, D, w.final_wp, (int64_t)c.in_channels * D, D, N, c.in_channels, D, 3);
        g.epi = EPI_F32_CT; g.bias = w.final_b; g.out32 = v_out; g.T = T;
        return launch_gemm(g, e.st);
    }
    case FINAL_ROWS:
        break;
    }
    return launch_final_layer(s.h, modf, modf + D, MODW, w.final_w, w.final_b, N, D, T, c.in_channels, 1e-6f, v_out, e.st);
}

int dit_forward(vb_ctx* ctx, const DitEval& ev, hipStream_t st) {
    Eval e(ctx, ev, st);
    const vb_dit_config& c = e.c;
    if (ev.T > c.max_len) VB_FAIL(VB_E_INVALID, "dit_forward: T=%d exceeds the RoPE table (max_len=%d, vocal2music_moe.py:421)", ev.T, c.max_len);
    if (ev.zero_vt) VB_HIP(hipMemsetAsync(e.s.vt, 0, (size_t)e.s.n_vt * e.np * sizeof(bf16_t), st));
    if (ev.nb_active < 0 || ev.nb_active > ev.nb) VB_FAIL(VB_E_INVALID, "dit_forward: nb_active=%d of nb=%d", ev.nb_active, ev.nb);
    if (e.p.router_counts && ev.evals_before < 0)
        VB_TRY(launch_fill_f32(reinterpret_cast<float*>(bucket_counts(e.s.perm, e.NL, 0)), bucket_counts_ints(e.NL), 0.f, st));
    VB_TRY(conditioning_vectors(e));
    VB_TRY(embed_latent(e));
    for (int i = 0; i < c.depth; ++i) {
        VB_TRY(attention_half(e, i));
        VB_TRY(caption_gate_and_route(e, i));      // Band-MoE (vocal2music_moe.py:117-185)
        VB_TRY(routed_experts(e, i));
        VB_TRY(band_experts(e, i));
    }
    return final_layer(e);
}

extern "C" {

int vb_dit_load(vb_ctx* ctx, const vb_dit_config* cfg, const vb_dit_weights* w) {
    if (!ctx || !cfg || !w) VB_FAIL(VB_E_INVALID, "dit_load: null argument");
    if (cfg->depth < 1 || cfg->depth > VB_MAX_DEPTH) VB_FAIL(VB_E_INVALID, "dit_load: depth %d", cfg->depth);
    if (cfg->np != 1 && cfg->np != 2) VB_FAIL(VB_E_INVALID, "dit_load: np %d", cfg->np);
    if (cfg->hidden % cfg->heads || cfg->hidden / cfg->heads != 96)
        VB_FAIL(VB_E_INVALID, "dit_load: head_dim %d unsupported (kernels are built for 96)", cfg->hidden / (cfg->heads ? cfg->heads : 1));
    if (cfg->hidden % cfg->num_experts || (cfg->hidden / cfg->num_experts) % 8) VB_FAIL(VB_E_INVALID, "dit_load: band width must be a multiple of 8");
    if (cfg->context_dim != cfg->hidden) VB_FAIL(VB_E_INVALID, "dit_load: context_dim must equal hidden_size (vocal2music_moe.py:367-373)");
    if (cfg->num_experts > 16) VB_FAIL(VB_E_INVALID, "dit_load: num_experts %d > 16", cfg->num_experts);
    if (cfg->hidden > 768) VB_FAIL(VB_E_INVALID, "dit_load: hidden %d > 768 (router register tile)", cfg->hidden);
    // captured sampler graphs hold the OLD weight pointers and launch geometry in their kernel nodes: a (re)load drops them all
    for (SampleGraph& g : ctx->graphs) g.destroy();
    ctx->graphs.clear();
    ctx->cfg = *cfg;
    ctx->w = *w;
    ctx->dit_loaded = true;
    return VB_OK;
}
size_t vb_dit_cond_bytes(const vb_dit_config* cfg, int B, int n_branch, int T, int L) {
    return carve_cond(nullptr, *cfg, B, n_branch, T, L).total;
}
size_t vb_dit_workspace_bytes(const vb_dit_config* cfg, int B, int n_branch, int T, int L) {
    return carve_ws(nullptr, *cfg, B, n_branch, T, L).total;
}
int vb_dit_precompute_cond(vb_ctx* ctx, const float* t5, const int64_t* midi, const int64_t* beats, int B, int n_branch, int T,
                           int T_mel, int L, void* cond, void* ws, void* stream) {
    return vb_dit_precompute_cond_lens(ctx, t5, midi, beats, B, n_branch, T, T_mel, L, nullptr, cond, ws, stream);
}
int vb_dit_precompute_cond_lens(vb_ctx* ctx, const float* t5, const int64_t* midi, const int64_t* beats, int B, int n_branch, int T,
                                int T_mel, int L, const vb_lens* lens, void* cond, void* ws, void* stream) {
    if (!ctx || !ctx->dit_loaded) VB_FAIL(VB_E_STATE, "precompute_cond: DiT not loaded");
    if (n_branch < 1 || n_branch > 2 || B < 1) VB_FAIL(VB_E_INVALID, "precompute_cond: B=%d n_branch=%d", B, n_branch);
    LensPlan lp;
    if (lens && lens->len) VB_TRY(lens_plan(lens->len, B, T, &lp));
    if (lp.B && T_mel != 2 * T)
        VB_FAIL(VB_E_INVALID, "precompute_cond_lens: T_mel=%d is not 2 * T = %d, which row lengths need (row %d has length %d)", T_mel, 2 * T,
                lp.first_short(T), lp.len[lp.first_short(T)]);
    VB_HIP(hipSetDevice(ctx->device));
    RoctxRange rr("vb_dit_precompute_cond");
    return dit_precompute(ctx, t5, midi, beats, B, n_branch, T, T_mel, L, lp, cond, ws, (hipStream_t)stream);
}
int vb_dit_forward(vb_ctx* ctx, const float* x, const int64_t* t_idx, const void* cond, const vb_noise* noise, int B, int n_branch,
                   int T, int L, float* v_out, int32_t* route_out, void* ws, void* stream) {
    return vb_dit_forward_lens(ctx, x, t_idx, cond, noise, B, n_branch, T, L, nullptr, v_out, route_out, ws, stream);
}
int vb_dit_forward_lens(vb_ctx* ctx, const float* x, const int64_t* t_idx, const void* cond, const vb_noise* noise, int B, int n_branch,
                        int T, int L, const vb_lens* lens, float* v_out, int32_t* route_out, void* ws, void* stream) {
    if (!ctx || !ctx->dit_loaded) VB_FAIL(VB_E_STATE, "dit_forward: DiT not loaded");
    LensPlan lp;
    if (lens && lens->len) VB_TRY(lens_plan(lens->len, B, T, &lp));
    VB_HIP(hipSetDevice(ctx->device));        // the calling host thread may be new (one thread per stream): bind it to the context's GPU
    DitEval ev;
    ev.x = x; ev.t_idx = t_idx; ev.cond = cond; ev.ws = ws; ev.B = B; ev.nb = n_branch; ev.T = T; ev.L = L;
    ev.noise = noise; ev.v_out = v_out; ev.route_out = route_out; ev.zero_vt = true;
    if (lp.B) {
        int* table = carve_ws(ws, ctx->cfg, B, n_branch, T, L).len_table;
        VB_TRY(launch_lens_table(lp, table, (hipStream_t)stream));
        ev.lens = table;
    }
    return dit_forward(ctx, ev, (hipStream_t)stream);
}

}  // extern "C"
