/* libversband_hip.so - C ABI of the MI355X-native AccompBand inference path.
 *
 * The reference (AaronZ345/VersBand) is pure Python with no native layer; these entry
 * points are what a maintainer binds (ctypes) underneath the reference's
 * own operator API.  Each entry cites the reference interface it replaces
 * (paths relative to the reference tree).
 *
 * Conventions
 *   - every tensor is a caller-owned, contiguous DEVICE pointer (torch `data_ptr()`);
 *     nothing here allocates or frees device memory: scratch is passed in and its size is
 *     queried with the matching *_workspace_bytes();
 *   - every launch goes to the `stream` argument (a hipStream_t passed as void*);
 *   - return value: 0 = ok, <0 = VB_E_*; vb_last_error() returns a thread-local message;
 *   - no exceptions cross the ABI; one host thread per context / GPU
 *     (scripts/test_final.py:475 spawns one process per GPU).
 *
 * "planes" tensors are bf16 with np planes: plane 0 = round-to-nearest bf16 of the value,
 * plane 1 (np == 2 only) = bf16 of the rounding residual, stored numel elements after
 * plane 0.  np == 2 selects the split-precision ("bf16x3") MFMA path used for parity;
 * np == 1 is the plain bf16 production path.
 */
#ifndef VERSBAND_HIP_H
#define VERSBAND_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VB_OK 0
#define VB_E_INVALID (-1)
#define VB_E_HIP (-2)
#define VB_E_STATE (-3)
#define VB_MAX_DEPTH 16

typedef struct vb_ctx vb_ctx;

int vb_ctx_create(int device, vb_ctx** out);
int vb_ctx_destroy(vb_ctx* ctx);
const char* vb_last_error(void);
int vb_abi_version(void);
/* sha256 (hex) over the library's sources, the public header and the compile flags it was built from; versband_amd/_lib.py compares
 * it with the sources on disk so a stale binary is never run (struct layouts may have moved), and loads a prebuilt library as it is
 * when no sources are shipped beside it */
const char* vb_source_digest(void);
/* 1 when built with -DVB_EXPERIMENTS (ablation instances and the measured-slower kernels of DESIGN.md section 5; never shipped) */
int vb_has_experiments(void);

/* HIP-event timing of one kernel class inside a region (bench.py roofline): bit 0 = bf16 GEMM,
 * bit 1 = attention, bit 2 = conv1d, bit 3 = fused ResBlock pair.  Events are recorded on the launch stream around every launch of
 * the enabled classes; vb_prof_read synchronises the device and sums the elapsed times.
 * Bits 8..15 of class_mask = sampling period n of class 0 (time every n-th launch per host thread; 0/1 = every launch), bits 16..19 = the period of
 * classes 1..3 (0 = the same n), bits 20..23 / 24..27 = which launch of a period is timed (class 0 / the others): walking the phases over as many
 * regions times every launch exactly once per cycle without bracketing neighbouring launches.
 * vb_prof_read: ms_sum, flops and bytes (algorithmic work of those launches) cover the `timed` launches only; `launches` counts all launches of the class. */
/* Tuning / A-B knobs (environment variables, read once per process; a tool or test that changes one at run time calls this
 * afterwards).  Not needed by a product caller.  Kernel selection, results bit-identical: VB_GEMM_TILE (22|33|24|42|11|21),
 * VB_GEMM_SMALL / VB_GEMM_SMALL_TILES (64x64 tiles below that many 128x128 tiles), VB_GEMM_VARIANT, VB_GEMM_NCHUNK, VB_GEMM_P8*,
 * VB_ROUTER_TPW (tokens per wave), VB_BAND_UNFUSED, VB_MOE_UNFUSED, VB_SCORE_FUSED, VB_CONV_CFG, VB_CONV_DIRECT_EPI, VB_NO_GRAPH,
 * VB_BUCKET_COUNT_LAUNCH (bucket counts by their own launch instead of the router's side counts), VB_EULER_LAUNCH (FinalLayer / Euler update /
 * step advance as three launches per step instead of one).
 * Changing the arithmetic (same algorithm, low-order bits differ): VB_ATTN_DEFER (log2 threshold of the deferred softmax rescale,
 * default 8, 0 = exact running maximum), VB_STEM_F32, VB_GATE_UNFOLDED.  Timing-only ablations (results WRONG): VB_GEMM_ABLATE,
 * VB_CONV_ABLATE, VB_ATTN_ABLATE. */
void vb_tune_reload(void);
int vb_prof_enable(int class_mask);
int vb_prof_read(int cls, double* ms_sum, double* flops, double* bytes, int64_t* launches, int64_t* timed);

/* ---------------------------------------------------------------- DiT + Band-MoE ----
 * TxtFlagLargeImprovedDiTV2 (ldm/modules/diffusionmodules/vocal2music_moe.py:293-520),
 * constructor params of configs/vocal2music.yaml:36-43. */
typedef struct {
    int in_channels, hidden, heads, depth, num_experts, ffn_hidden, context_dim, ori_dim, max_len;
    int np;            /* 1 = bf16, 2 = split precision (parity mode) */
    float norm_eps;
} vb_dit_config;

typedef struct {
    /* bf16 planes (np planes each, plane stride = numel) */
    const void* wqkv;   /* [3D][D]  rows wq|wk|wv              flag_large_dit_moe.py:173-181 */
    const void* wo;     /* [D][D]                               :193 */
    const void* wq_m;   /* MoE.cross_attention in_proj rows 0:D vocal2music_moe.py:79 */
    const void* wo_m;   /* MoE.cross_attention.out_proj (kept for reference; folded into wcg/bcg, no GEMM runs on it) */
    const void* w13;    /* [2E][2H][D] routed experts, rows interleaved w1_0,w3_0,w1_1,...  (caption group first) */
    const void* w2;     /* [2E][D][H] */
    const void* w13f;   /* [E][2H][band]  band experts restricted to their channel band (:171-178) */
    const void* w2f;    /* [E][band][H] */
    const void* wky;    /* attention.wk_y [D][ctx]   (precompute only) */
    const void* wvy;    /* attention.wv_y */
    const void* wk_m;   /* MoE.cross_attention in_proj rows D:2D (precompute only) */
    const void* wv_m;   /* rows 2D:3D */
    const void* wqt_s;  /* optional (2 planes): (in_proj rows 0:D)^T * hd^-1/2, [D in][D out] - folds the MoE q-projection into the
                           per-clip caption keys so the gate scores come from ONE grouped GEMM (precompute only) */
    /* fp32 */
    const float* bq_m; const float* bo_m; const float* bk_m; const float* bv_m;
    const float* bq_s;               /* bq_m * hd^-1/2 (with wqt_s) */
    const float* attn_norm_w; const float* ffn_norm_w; const float* y_norm_w;
    const float* cross_w;            /* tanh(attention.gate) [heads]   :401 */
    const float* wcg; const float* bcg;   /* caption_gating_network with cross_attention.out_proj folded in: Wg*Wo [E][D], Wg*bo+bg [E] */
    const float* wag; const float* bag;   /* acoustic_gating_network (precompute only) */
} vb_dit_block_weights;

typedef struct {
    vb_dit_block_weights blocks[VB_MAX_DEPTH];
    const float* t_freq_table;       /* [1000][256] sinusoid table (TimestepEmbedder.timestep_embedding) */
    const float* t_mlp0_w; const float* t_mlp0_b; const float* t_mlp2_w; const float* t_mlp2_b;
    const float* adaln_w; const float* adaln_b;   /* stacked [depth*6D + 2D][D]: blocks' adaLN then final_layer's */
    const void* adaln_wp;                         /* optional: the same matrix as split-bf16 planes [2][rows][D]; lets the sampler tabulate
                                                     all steps' modulations with one bf16x3 MFMA GEMM instead of an fp32 row-linear */
    const float* hl_w; const float* hl_b;         /* stacked high_level_gating_network [depth*2][D] */
    const float* proj_in_w; const float* proj_in_b;  /* conv packed [5][C][D] */
    const void* proj_in_w3;                          /* same weights as split-bf16 planes [2][5][D][32] (bf16x3 conv kernel) */
    const float* final_w; const float* final_b;      /* final_layer.linear [C][D] */
    const void* final_wp;                            /* optional: final_layer.linear as split-bf16 planes [2][C][D] (FinalLayer on the MFMA GEMM) */
    const float* rope_cos; const float* rope_sin;    /* [max_len][hd/2]  precompute_freqs_cis */
    /* precompute only */
    const float* midi_emb; const float* beats_emb;
    const float* midi_conv_w; const float* midi_conv_b;    /* packed [5][D][D] */
    const float* beats_conv_w; const float* beats_conv_b;
    const float* final_proj_w; const float* final_proj_b;  /* packed [1][D][D] */
    const void* midi_conv_w3; const void* beats_conv_w3; const void* final_proj_w3;   /* optional: the three stem convolutions' weights as
                                                              split-bf16 planes [2][taps][D][D] (bf16x3 conv kernel instead of exact fp32) */
    const void* c_emb0; const float* c_emb0_b;             /* planes(2) [D][ori] */
    const void* c_emb2; const float* c_emb2_b;             /* planes(2) [D][D] */
    const float* c_ln_w; const float* c_ln_b;
    const float* cap_ln_w; const float* cap_ln_b;
    const float* cap_lin_w; const float* cap_lin_b;
} vb_dit_weights;

/* replaces: model construction + load_state_dict (scripts/test_final.py:140-151).  The
 * structs are copied; the device tensors they point to stay owned by the caller. */
int vb_dit_load(vb_ctx* ctx, const vb_dit_config* cfg, const vb_dit_weights* w);

size_t vb_dit_cond_bytes(const vb_dit_config* cfg, int B, int n_branch, int T, int L);
size_t vb_dit_workspace_bytes(const vb_dit_config* cfg, int B, int n_branch, int T, int L);

/* Everything of TxtFlagLargeDiT.forward that does not depend on (x,t): acoustic stem
 * (vocal2music_moe.py:388-393), caption embedding + pooled embedding (:407-413), per block
 * context K/V of Attention and MoE.cross_attention and the acoustic gate logits.
 *   t5    f32 [n_branch*B][L][ori_dim]   (cond rows, then uncond rows)
 *   midi, beats  int64 [B][T_mel]        (context['c_concat'], :384-385)
 *   cond  caller buffer of vb_dit_cond_bytes() */
int vb_dit_precompute_cond(vb_ctx* ctx, const float* t5, const int64_t* midi, const int64_t* beats, int B, int n_branch,
                           int T, int T_mel, int L, void* cond, void* ws, void* stream);

/* Injected Gumbel noise (parity path): g = -log(Exp(1)) draws, rows = n_branch*B*T tokens,
 * per block: g1 [rows][2], g2 [rows][E], g3 [rows][E] (order of MoE.forward :134,150,151).
 * Layout [depth][rows][w].  NULL => the engine draws its own (counter based, keyed by
 * (seed, global clip, nfe, block, gate)). */
typedef struct {
    const float* g1; const float* g2; const float* g3;
    uint64_t seed; int64_t clip_base; int nfe;
} vb_noise;

/* One network evaluation for the cond and uncond branches together:
 * replaces the two apply_model() calls of Wrapper_cfg.forward (ldm/models/diffusion/cfm1_audio.py:158-159)
 * -> DiffusionWrapper.forward (ddpm.py:1418-1436) -> TxtFlagLargeDiT.forward.
 *   x      f32 [B][C][T]        (shared by both branches)
 *   t_idx  int64 [n_branch*B]   integer diffusion index (cfm1_audio.py:156)
 *   v_out  f32 [n_branch*B][C][T]
 *   route_out  optional int32 [depth][2][rows] routed expert indices (caption, acoustic) */
int vb_dit_forward(vb_ctx* ctx, const float* x, const int64_t* t_idx, const void* cond, const vb_noise* noise, int B,
                   int n_branch, int T, int L, float* v_out, int32_t* route_out, void* ws, void* stream);

/* x += dt * (v_u + s (v_c - v_u))  - Wrapper_cfg.forward :160 + torchdyn fixed-step Euler */
int vb_euler_cfg_step(float* x, const float* v, int B, int64_t per_item, float cfg_scale, float dt, int has_uncond, void* stream);

/* CFMSampler.sample_cfg (ldm/models/diffusion/cfm1_audio_sampler.py:87-116): n_steps Euler steps.
 *   t_idx_table int64[n_steps], dt_table f32[n_steps] : host OR device arrays (copied with hipMemcpyDefault on the stream; host arrays must outlive that copy)
 *   noise: NULL or per-step injected noise laid out [step][depth][rows][w]
 *   traj  optional f32 [n_steps+1][B][C][T] */
int vb_sample_cfg(vb_ctx* ctx, float* x, const void* cond, int B, int n_branch, int T, int L, int n_steps,
                  const int64_t* t_idx_table, const float* dt_table, float cfg_scale, const vb_noise* noise, float* traj,
                  void* ws, void* stream);
/* The same sampler with a KNOWN REGION held on the model's probability path (inpainting, continuation; build-defined, the reference has
 * none).  The flow-matching model is trained on x_t = t x1 + (1 - (1 - sigma_min) t) x0 (ldm/models/diffusion/cfm1_audio.py:38-43).  After
 * the Euler step k that ends at time tn = t_next[k], every element (b, c, t) of the state becomes, in fp32 and in exactly this arithmetic,
 *     xn = fmaf(dt, e, x)                                        (the plain update; e = the CFG-combined velocity)
 *     r  = fmaf(tn, ref, (1 - (1 - sigma_min) * tn) * x0)
 *     x  = fmaf(m, r, (1 - m) * xn)                              m = mask[b][t]
 * so m = 0 leaves xn and m = 1 gives r, both bit for bit; a fractional m is a soft edge (the caller's choice).  The free tokens evolve
 * under the DiT, whose self-attention sees the known tokens at the right noise level at every step.  On entry the state is projected
 * the same way at t_0 = t_next[0] - dt_table[0] (exact on a linspace grid): x = fmaf(m, r(t_0), (1 - m) x) - it matters when the call
 * starts inside the path (t_start); at t_0 = 0 with x = x0 it changes nothing.  traj[0] is the projected state.
 *   ref, x0  f32 [B][C][T]  the known content (sampler latent scale) and the noise the sampler started from (device)
 *   mask     f32 [B][T]     in [0, 1] (device; not range-checked here)
 *   t_next   f32 [n_steps]  time after each step; host OR device, copied like dt_table
 * The final state of a kept token at t = 1 is ref + sigma_min * x0, NOT ref: that is the end point of the path the model was trained on.
 * keep == NULL is exactly vb_sample_cfg.  Graph capture works as below; the key also holds ref, x0, mask and sigma_min, so a call with
 * other buffers captures its own graph and a plain call never replays a keep graph.  The fused (one launch per step) and the separate
 * (n_branch == 1, VB_EULER_LAUNCH) update forms are one device function - the same two fused multiply-adds - and bit-identical. */
typedef struct { const float* ref; const float* x0; const float* mask; const float* t_next; float sigma_min; } vb_keep;
int vb_sample_cfg_keep(vb_ctx* ctx, float* x, const void* cond, int B, int n_branch, int T, int L, int n_steps,
                       const int64_t* t_idx_table, const float* dt_table, float cfg_scale, const vb_keep* keep,
                       const vb_noise* noise, float* traj, void* ws, void* stream);
/* The same sampler with PER-ROW guidance scale and noise key: rows that differ in guidance scale (the scales of one item) or whose global
 * clip indices are not contiguous (items sharded rank::world, same-length items picked out of a manifest) share one call.  All rows of a
 * call still share L, and T unless row lengths are given (vb_lens, below).
 *   cfg_scale  f32 [B]    (device) row b is guided by cfg_scale[b]: e = fmaf(cfg_scale[b], v_c - v_u, v_u), the fused multiply-add
 *                         evaluation of v_u + cfg_scale[b] * (v_c - v_u), in EVERY update form - fused into FinalLayer, with a known region,
 *                         the separate launch (VB_EULER_LAUNCH): all are the same two fused multiply-adds, the arithmetic of the scalar
 *                         call, so row b equals the scalar call with that scale bit for bit.  The scalar argument is ignored.  With
 *                         n_branch == 1 there is nothing to guide and the array is not read.
 *   clip       int64 [B]  (device) row b of BOTH branches draws its router noise from the stream of global clip clip[b] instead of
 *                         noise->clip_base + b; seed and nfe stay per call.  With injected noise arrays (noise->g1) the ids are unused.
 * Either member may be NULL; rows == NULL or both NULL is exactly vb_sample_cfg_keep (which, like vb_sample_cfg, forwards here).  Both
 * arrays are read from device memory when the kernels run, and the graph key holds the two POINTERS (and 0 in place of the scalar scale
 * beside cfg_scale): rewriting the arrays in place and calling again replays the same graph with the new values, a call with other row
 * buffers, or with none, captures its own graph and never replays a rows graph. */
typedef struct { const float* cfg_scale; const int64_t* clip; } vb_rows;
int vb_sample_cfg_rows(vb_ctx* ctx, float* x, const void* cond, int B, int n_branch, int T, int L, int n_steps,
                       const int64_t* t_idx_table, const float* dt_table, float cfg_scale, const vb_rows* rows, const vb_keep* keep,
                       const vb_noise* noise, float* traj, void* ws, void* stream);
/* The same sampler over JOINT WINDOWS of long clips (build-defined; the MultiDiffusion construction on this sampler).  The B rows are nw
 * windows of Bc = B / nw clips, x [nw*Bc][C][n] with row = w*Bc + b and n = T the window length; window w covers the clip's tokens
 * [starts[w], starts[w] + n).  Neighbouring windows overlap in ov = starts[w] + n - starts[w+1] tokens: token n - ov + u of row w*Bc + b
 * and token u of row (w+1)*Bc + b are the same token of clip b.  After every Euler step both copies take one consensus value, in fp32
 * and in exactly this arithmetic, for every u in [0, ov), clip b and channel c:
 *     ia = ((w*Bc + b)*C + c)*n + (n - ov + u)        ib = (((w+1)*Bc + b)*C + c)*n + u
 *     g  = (float)(u + 1) / (float)(ov + 1)           (the later window's ramp weight (u + 1) / (ov + 1), the one vb_crossfade_windows uses)
 *     m  = fmaf(g, x[ib] - x[ia], x[ia]);   x[ia] = x[ib] = m
 * so equal copies come back unchanged bit for bit, and overlapping tokens of neighbouring rows are bit-identical after every step, in
 * every traj[k] and in the result: the windows are stitched by plain slicing, without a fade.  Every window's self-attention sees at
 * every step the state its neighbour sees in the overlap.
 * Order within a step: (1) the Euler + CFG update - fused into FinalLayer or the separate launch - with the known-region blend when
 * keep is given, (2) the overlap consensus, (3) the traj copy.  A known region that is equal in both windows stays on its path bit for
 * bit.  The consensus also runs once on entry, after the keep projection and before traj[0]: rows that disagree in their overlaps
 * start from the consensus, rows cut from one start noise are not changed.  It is one kernel in both update forms, so VB_EULER_LAUNCH
 * stays bit-identical to the fused form.
 *   starts  int32 [nw]  HOST array of window starts, ascending; read during the call only.
 * VB_E_INVALID, with the window named in vb_last_error(), when: nw < 1 or nw > 64; B % nw != 0; starts[0] < 0;
 * starts[w] < starts[w+1] <= starts[w] + n is violated (descending starts, or a gap); starts[w+2] < starts[w] + n (a token under three
 * windows - the pairs above would no longer be disjoint).
 * win == NULL or nw == 1 is exactly vb_sample_cfg_rows (which, like vb_sample_cfg and vb_sample_cfg_keep, forwards here).  The captured
 * graph includes the consensus launches; its key holds nw and the VALUES of starts, so another plan on the same buffers captures its
 * own graph and a plain call never replays a windows graph. */
typedef struct { const int32_t* starts; int nw; } vb_windows;     /* starts: HOST array of nw window starts, ascending */
int vb_sample_cfg_windows(vb_ctx* ctx, float* x, const void* cond, int B, int n_branch, int T, int L, int n_steps,
                          const int64_t* t_idx_table, const float* dt_table, float cfg_scale, const vb_windows* win, const vb_rows* rows,
                          const vb_keep* keep, const vb_noise* noise, float* traj, void* ws, void* stream);
/* The same sampler with PER-STEP GUIDANCE WEIGHTS (build-defined; guidance intervals and guidance ramps): vb_sample_cfg_windows plus a
 * schedule.  weight is a HOST array of n_steps finite floats in [0, 16], read during the call only; anything else is VB_E_INVALID, with
 * the step named in vb_last_error(), before anything is launched.  With s the call's scalar scale, or rows->cfg_scale[b] for row b,
 * step k is one of three kinds:
 *   weight[k] == 1   today's step: the same launches, arguments and bits as vb_sample_cfg_windows.
 *   weight[k] == 0   a single-branch step: only the conditional rows [0, B) are evaluated - about half a network evaluation - and the
 *                    update is x = fmaf(dt, v_c, x), the update of an n_branch == 1 call.  The unconditional rows are neither read nor
 *                    written in that step.
 *   otherwise        both branches under the step's effective scale s_k = fmaf(weight[k], s - 1, 1):
 *                    e = fmaf(s_k, v_c - v_u, v_u), x = fmaf(dt, e, x).  A scalar s is combined on the host; per-row scales are combined
 *                    per token on the device, in exactly this arithmetic.
 * The known-region blend (keep) and the overlap consensus (win) follow the update exactly as in any step, in the order stated above.
 * Router noise is keyed as if every step had two branches: the conditional rows of step k draw from the stream (seed, clip, evaluation
 * k, branch 0, block, gate) whatever the kind of this or any other step, so a schedule changes no other step's noise and one replayed
 * graph serves any seed.  Injected noise arrays (noise->g1) keep their two-branch layout; a single-branch step reads its first B*T rows.
 * guidance == NULL, weight == NULL or all weights == 1 is exactly vb_sample_cfg_windows (which, like the three before it, forwards here):
 * same launches, same graph.  With n_branch == 1 there is nothing to guide and the schedule is not read, as the scales are not.
 * Which steps run one branch is baked into the captured graph, and the weights are launch arguments: the graph key holds the VALUES of
 * weight, so another schedule on the same buffers captures its own graph.  rows->cfg_scale is still read when the kernels run:
 * rewriting it in place replays the same graph.  The fused and the separate (VB_EULER_LAUNCH) update forms stay bit-identical. */
typedef struct { const float* weight; } vb_guidance;              /* weight: HOST array of n_steps step weights in [0, 16] */
int vb_sample_cfg_sched(vb_ctx* ctx, float* x, const void* cond, int B, int n_branch, int T, int L, int n_steps,
                        const int64_t* t_idx_table, const float* dt_table, float cfg_scale, const vb_guidance* guidance,
                        const vb_windows* win, const vb_rows* rows, const vb_keep* keep, const vb_noise* noise, float* traj, void* ws,
                        void* stream);
/* ROW LENGTHS (build-defined; the reference pads and attends over everything in training and runs batch 1 at inference): clips of
 * different lengths as rows of one call.  T is the padded row length of the call and len[b] <= T row b's own length; its tokens are
 * [0, len[b]), the rest of the row is padding.  THE CONTRACT: row b of a call with lengths is the call on that clip alone - on its valid
 * tokens, x, every traj[k], v_out and route_out equal what the same entry point computes for B = 1, T = len[b] (precompute with
 * T_mel = 2 len[b]) on the row's first len[b] tokens, with the same blocks sliced and the row's noise key (rows->clip[b], or
 * noise->clip_base + b).  Only three places of a network evaluation look past a token's own row, and each has one mechanism:
 *   self-attention   row b attends over its first len[b] keys (a device table of the lengths in the workspace; both branches read
 *                    len[b % B]); query rows from len[b] on are padding.  Cross-attention over the L caption keys is unchanged.
 *   proj_in          the k = 5 taps at t >= len[b] read as zero, on every route (x itself is not modified).
 *   acoustic stem    (precompute) the midi / beats embeddings are zero from mel position 2 len[b] on, so the k = 5 convolutions see the zero
 *                    padding of the clip alone; a call with lengths requires T_mel == 2 T (the +-2 crop / repeat tolerance of
 *                    vocal2music_moe.py:397 stays for calls without lengths).
 * Everything else is token-local and runs over the padding tokens too (wasted work of at most the padding share, never wrong).
 * Padding: the padding of midi / beats / x is never read into a valid token - it may hold anything, NaN included.  The padding tokens
 * of x, traj, v_out and route_out are written and UNSPECIFIED, but finite when the caller's padding of x was finite (the update kernels
 * are the ones of a plain call and run over every token); a host that wants a defined tensor clears them (the Python host does).
 *   len  int32 [B]  HOST array of row lengths, 1 <= len[b] <= T; read during the call only.
 * VB_E_INVALID, with the row named in vb_last_error(), before anything is launched and with x unchanged, when: len[b] < 1; len[b] > T;
 * B > 64; T_mel != 2 T (precompute); win with nw > 1 beside lengths (joint windows are equal-length by construction).  Windows of clips of
 * different lengths are rows of their own length under a per-row plan: vb_sample_cfg_window_rows (below).
 * lens == NULL, len == NULL or all len[b] == T is exactly the entry point without lengths (vb_sample_cfg_sched, which like the four before
 * it forwards here; vb_dit_forward; vb_dit_precompute_cond - both forward to their _lens forms): same launches, same graph key, same bits.
 * keep, rows and guidance compose unchanged (all are token-local); single-branch steps read the same table.  The lengths reach the
 * device through a launch argument at the head of the step loop, which a captured graph holds: the graph key holds the VALUES of len,
 * so another set of lengths on the same buffers captures its own graph and a plain call never replays a lengths graph.  Hosts detect
 * the feature by the presence of these symbols (vb_abi_version() stays 3).  Every conv net takes row lengths through an entry point of its own
 * (below): vb_hifigan_forward_lens, vb_vae_decode_lens, vb_vae_encode_lens, vb_bigvgan_forward_lens and the chunked forms. */
typedef struct { const int32_t* len; } vb_lens;                   /* len: HOST array of B row lengths, 1 <= len[b] <= T */
int vb_dit_precompute_cond_lens(vb_ctx* ctx, const float* t5, const int64_t* midi, const int64_t* beats, int B, int n_branch, int T,
                                int T_mel, int L, const vb_lens* lens, void* cond, void* ws, void* stream);
int vb_dit_forward_lens(vb_ctx* ctx, const float* x, const int64_t* t_idx, const void* cond, const vb_noise* noise, int B, int n_branch,
                        int T, int L, const vb_lens* lens, float* v_out, int32_t* route_out, void* ws, void* stream);
int vb_sample_cfg_lens(vb_ctx* ctx, float* x, const void* cond, int B, int n_branch, int T, int L, int n_steps,
                       const int64_t* t_idx_table, const float* dt_table, float cfg_scale, const vb_lens* lens, const vb_guidance* guidance,
                       const vb_windows* win, const vb_rows* rows, const vb_keep* keep, const vb_noise* noise, float* traj, void* ws,
                       void* stream);
/* WINDOW ROWS (build-defined): joint windows of long clips of DIFFERENT lengths as rows of one call - a per-row window plan in place of
 * the one starts[nw] array of vb_windows, beside row lengths.  Row r is a window of long clip group[r] and covers that clip's tokens
 * [start[r], start[r] + len[r]), with len[r] the row's length from the vb_lens block of the same call, or T without one.  Rows of one
 * group appear in ascending start; they need not be adjacent (the interleaved layout of vb_windows is the special case
 * group[r] = r % Bc, start[r] = starts[r / Bc]).  Group ids are labels: any values, equal for the rows of one clip.
 * For each group, consecutive rows (ra, rb) form a consensus pair with ov = start[ra] + len[ra] - start[rb]: token len[ra] - ov + u of
 * row ra and token u of row rb are the same token of the clip.  On entry (after the keep projection, before traj[0]) and after every
 * Euler step both copies take one consensus value, in the arithmetic of vb_sample_cfg_windows, for every u in [0, ov) and channel c:
 *     ia = (ra*C + c)*T + (len[ra] - ov + u)          ib = (rb*C + c)*T + u
 *     g  = (float)(u + 1) / (float)(ov + 1);   m = fmaf(g, x[ib] - x[ia], x[ia]);   x[ia] = x[ib] = m
 * in the documented order within a step: update (with the keep blend), consensus, traj copy.  Only valid tokens are touched: a row's
 * padding is neither read nor written by the consensus.  It is one kernel in both update forms, so VB_EULER_LAUNCH stays bit-identical.
 * Everything else of a network evaluation is token-local or reads the length table, so THE CONTRACT of vb_lens extends by groups: the
 * rows of a group, on their valid tokens, equal the same entry point on that group's rows alone with the same noise keys (rows->clip).
 *   group, start  int32 [B]  HOST arrays, read during the call only.
 * VB_E_INVALID, with the row named in vb_last_error(), before anything is launched and with x unchanged, when: group or start is null;
 * B > 64; start[r] < 0; for consecutive rows (ra, rb) of a group start[rb] <= start[ra] (not ascending), start[rb] > start[ra] + len[ra]
 * (a gap) or ov > len[rb]; for consecutive rows (ra, rb, rc) of a group start[rc] < start[ra] + len[ra] (a token under three rows - the
 * pairs would no longer be disjoint); win with nw > 1 beside the block (one plan describes the rows, not two).
 * A group of one row has no pair.  wrows == NULL, or a block in which no group has two rows, is exactly vb_sample_cfg_lens (which, like
 * the five before it, forwards here with NULL): same launches, same graph key, same bits.  The captured graph includes the consensus
 * launches; its key holds the VALUES of group, start and len, so another plan on the same buffers captures its own graph, and a plain
 * call, a vb_windows call or a lengths-only call never replays a window-rows graph.  vb_windows keeps its own kernel and plan (no 64-row
 * cap, B / nw clips per pair).  Hosts detect the feature by the presence of these symbols (vb_abi_version() stays 3). */
typedef struct { const int32_t* group; const int32_t* start; } vb_window_rows;   /* HOST arrays of B entries each */
int vb_sample_cfg_window_rows(vb_ctx* ctx, float* x, const void* cond, int B, int n_branch, int T, int L, int n_steps,
                              const int64_t* t_idx_table, const float* dt_table, float cfg_scale, const vb_window_rows* wrows,
                              const vb_lens* lens, const vb_guidance* guidance, const vb_windows* win, const vb_rows* rows,
                              const vb_keep* keep, const vb_noise* noise, float* traj, void* ws, void* stream);
/* The overlap consensus alone, on x [nw*Bc][C][n] with B = nw*Bc rows (the unit, like vb_euler_cfg_step): same formula, same checks. */
int vb_window_blend(float* x, const int32_t* starts, int nw, int B, int C, int n, void* stream);
/* The window-rows consensus alone, on x [B][C][T] (the unit): len is a HOST array of B row lengths in [1, T], NULL = every row has T. */
int vb_window_rows_blend(float* x, const int32_t* group, const int32_t* start, const int32_t* len, int B, int C, int T, void* stream);
/* The step loop of vb_sample_cfg is captured into a hipGraph the second time a call arrives with the same buffers / shape on a
 * capturable (non-default) stream and replayed from then on (noise key via device memory: any seed / clip base replays).
 * Number of instantiated graphs this context holds (0 = every call so far ran eagerly): */
int vb_sample_graphs(vb_ctx* ctx);

/* ---------------------------------------------------- conv nets (VAE decoder, HiFi-GAN) ----
 * AutoencoderKL.decode (ldm/models/autoencoder1d.py:55-58, Decoder1D :480-512) and
 * HifiGanGenerator.forward (vocoder/hifigan/modules/hifigan.py:126-143) both run as a flat op
 * list over fp32 [B][C][T] buffers; the list is built from the model config by the host side. */
typedef struct { int channels; int tmul; int square; } vb_buf_desc;   /* square: 1 = [T*tmul]^2 floats, 2 = channels x roundup(T*tmul, 32),
                                                                         3 = channels x (T*tmul + 448) floats (two transposed bf16 planes with halo),
                                                                         4 = half of that (ONE transposed bf16 plane with halo) */
/* VB_OP_SPLIT_PLANES: x (f32 [B][rows][cols], rows = Co, cols = Ci, -1 = the buffer's time length) -> out = split-bf16
 * planes [2][B][rows][roundup(cols, 32)]; a later VB_OP_CONV with w_buf = that buffer and wfmt = VB_WFMT_BUF_X3 uses them as
 * per-batch weights on the bf16x3 kernel (the VAE decoder's single-head attention) */
/* VB_OP_RESPAIR: fused HiFi-GAN ResBlock1 pair (vocoder/hifigan/modules/hifigan.py ResBlock1.forward), Ci = Co:
 * out = beta*out + alpha*(x + bias2 + conv2_k( lrelu( bias + conv1_{k,dil}( lrelu(x) ) ) )); the first convolution's weights sit in
 * the slot of the op's format, the second's in w2 (same format) */
/* VB_OP_GN_APPLY: out = GroupNorm affine of x from `stats` (+ swish when in_act == VB_ACT_GN_SWISH), same layout */
/* VB_OP_AA_ACT: BigVGAN anti-aliased Snake / SnakeBeta (vocoder/bigvgan/alias_free_torch/act.py): out = down2(snake(up2(x))), Ci channels,
 * gn_gamma = alpha (exp'ed when log-scale), gn_beta = 1 / (beta + 1e-9), w = the 12-tap Kaiser-sinc filter */
/* VB_OP_XT_PLANES: x (f32 [B][Ci][T]) -> out = pre-activated (in_act with `stats` / gn_gamma / gn_beta / in_slope), nearest-x2
 * upsampled (upsample2), split-bf16 TRANSPOSED planes [2][B][T + 448][Ci] with zero halo rows (out: a buffer of square = 3); a VB_OP_CONV
 * with x_planes = 1 reads them by DMA.  wfmt = VB_WFMT_BF16: the one-plane form - only the round-to-nearest plane [B][T + 448][Ci], plane 0
 * of the split form bit for bit (out: a buffer of square = 4) - which a BF16 VB_OP_CONV with x_planes = 1 reads */
enum { VB_OP_CONV = 0, VB_OP_GN_STATS = 1, VB_OP_SOFTMAX_T = 2, VB_OP_SPLIT_PLANES = 3, VB_OP_RESPAIR = 4, VB_OP_GN_APPLY = 5, VB_OP_AA_ACT = 6,
       VB_OP_XT_PLANES = 7 };
enum { VB_ACT_NONE = 0, VB_ACT_LRELU = 1, VB_ACT_GN_SWISH = 2, VB_ACT_TANH = 3, VB_ACT_GN = 4 };
/* Weight format of an op (vb_net_op.wfmt):
 *   F32     w: fp32 packed [phase][tap][Ci][Co]                       (pack.py:pack_conv / pack_conv_transpose)
 *   X3      w_x3: split-bf16 planes [2][phase][tap][Co][ci_pad]       (pack.py:pack_conv_x3; ci_pad = Ci rounded up to 32)
 *   MF      w_mf: fp32 F(2,3) minimal-filtering pseudo-taps [P][Ci][Co] of the same filter, 16-byte aligned (pack.py:pack_conv_mf)
 *   BUF_F32 w_buf: per-batch fp32 weights written by earlier ops      (the VAE attention's products)
 *   BUF_X3  w_buf: per-batch split planes from a VB_OP_SPLIT_PLANES
 *   BF16    w_x3: ONE plane [phase][tap][Co][ci_pad] of round-to-nearest bf16 weights - plane 0 of X3 (pack.py:pack_conv_bf16)
 * Allowed (kind, wfmt) pairs and the weight fields each reads; vb_net_load refuses any other pair, a NULL in a field the pair reads,
 * and a non-NULL weight pointer (w, w_x3, w_mf, w2) or a w_buf id in a field it does not read:
 *   CONV     F32      w                              the exact-fp32 kernels
 *   CONV     X3       w_x3, ci_pad, w                the bf16x3 kernels; w feeds the one-output-channel kernel (Co = 1: conv_post)
 *   CONV     MF       w_mf, w                        conv1d_f32w_kernel where launch_conv1d's run-time conditions hold, else the direct kernels on w
 *   CONV     BUF_F32  w_buf                          exact fp32
 *   CONV     BUF_X3   w_buf                          bf16x3
 *   RESPAIR  F32      w, w2, bias, bias2             respair_f32_kernel, C = 32 / 64 / 128
 *   RESPAIR  X3       w_x3, ci_pad, w2, bias, bias2  respair_x3 (split planes [2][k][C][C]), C = 32 / 64
 *   RESPAIR  MF       w_mf, w2, bias, bias2          respair_f32w_kernel (both 16-byte aligned), C = 32 / 64
 *   CONV     BF16     w_x3, ci_pad, w (Co = 1 only)  conv1d_bf16_kernel (one plane [phase][tap][Co][ci_pad]); w feeds the one-output-channel kernel
 *   RESPAIR  BF16     w_x3, ci_pad, w2, bias, bias2  respair_bf16_kernel (one plane [k][C][C] each), C = 32 / 64
 *   AA_ACT   NONE     w (the filter)
 *   XT_PLANES NONE    -                              split planes (two) for an X3 CONV with x_planes = 1
 *   XT_PLANES BF16    -                              ONE plane for a BF16 CONV with x_planes = 1 (the "bf16xt" op list)
 *   other    NONE     -
 * BF16 is the single-pass bf16 mode: every product is RN_bf16(weight) * RN_bf16(activated input), accumulated in fp32 - outside the 1e-3
 * parity contract by design (see vb_conv1d_bf16).  A BF16 CONV carries w exactly when Co == 1; a BF16 RESPAIR with C outside 32 / 64 is refused.
 * It also refuses an X3 / BF16 op whose ci_pad is not Ci rounded up to 32, MF weights that are not 16-byte aligned, and a RESPAIR without
 * Ci == Co or whose x / out differ in time length (buffer tmul; in_tmul / out_tmul for the I/O ids).  The failing op's index is in
 * vb_last_error().  Input planes must match the reader: XT_PLANES NONE writes a buffer of square = 3 and XT_PLANES BF16 one of square = 4;
 * a CONV with x_planes = 1 is X3 over a square = 3 buffer or BF16 over a square = 4 buffer - a split buffer into a BF16 conv, a one-plane
 * buffer into an X3 conv, x_planes with any other format, and a one-plane buffer into a BF16 conv of one output channel (the fp32
 * one-output-channel kernel reads no planes) are refused.  A BF16 CONV over planes runs as a one-pass GEMM on the DMA-fed 128 x 128 kernel
 * where the layer qualifies (Co >= 384, Ci % 64 == 0, plain channel-major output) and on conv1d_bf16_kernel's DMA-fed input mode otherwise
 * (VB_CONV_GEMM_OFF=1: always).  Conditions that depend on T or on buffer addresses are checked when the op runs. */
enum { VB_WFMT_NONE = 0, VB_WFMT_F32 = 1, VB_WFMT_X3 = 2, VB_WFMT_MF = 3, VB_WFMT_BUF_F32 = 4, VB_WFMT_BUF_X3 = 5, VB_WFMT_BF16 = 6 };
#define VB_BUF_INPUT (-2)
#define VB_BUF_OUTPUT (-3)
typedef struct {
    int kind;
    int wfmt;                             /* VB_WFMT_*: which weight fields the op reads (table above) */
    int x, out, res, stats, w_buf;        /* buffer ids, -1 = none */
    const float* w; const float* bias; const float* gn_gamma; const float* gn_beta;
    int Ci, Co, ksize, dil, pad, upsample2, in_act, out_act, out_transposed, tr_stride, tr_pad, tr_k, gn_groups;
    float in_slope, out_slope, alpha, beta, acc_scale;
    const void* w_x3; int ci_pad;            /* X3: split-bf16 weights and their padded input-channel count */
    const float* w_mf;                       /* MF: F(2,3) pseudo-tap weights */
    const void* w2; const float* bias2;      /* VB_OP_RESPAIR: the second convolution's weights (in the op's format) and bias */
    int in_stride, in_phase;                 /* VB_OP_CONV: the convolution reads x[i*in_stride + in_phase] (0/1 = plain) */
    int x_planes;                            /* VB_OP_CONV: x is a VB_OP_XT_PLANES buffer (upsample2 then describes how it was made) */
} vb_net_op;

enum { VB_NET_VAE = 0, VB_NET_VOCODER = 1, VB_NET_VAE_ENCODER = 2 };
/* buffer lengths are T * tmul of the base length T passed at run time; in_tmul / out_tmul give the I/O tensors' lengths
 * (decoder: 1 / 2; vocoder: 1 / hop; encoder: 2 / 1 with T = the latent length) */
int vb_net_load(vb_ctx* ctx, int which, const vb_net_op* ops, int n_ops, const vb_buf_desc* bufs, int n_bufs, int in_channels,
                int out_channels, int in_tmul, int out_tmul);
size_t vb_net_workspace_bytes(vb_ctx* ctx, int which, int B, int T);
/* decode_first_stage (ldm/models/diffusion/ddpm_audio.py:379-392): z [B][C][T] -> mel [B][80][2T] */
int vb_vae_decode(vb_ctx* ctx, const float* z, int B, int T, float* mel, void* ws, void* stream);
/* AutoencoderKL.encode (ldm/models/autoencoder1d.py:49-53, Encoder1D :315-409): mel [B][80][2T] -> moments [B][2*embed][T]
 * (mean = first half of the channels, logvar = second half; DiagonalGaussianDistribution is applied by the caller) */
int vb_vae_encode(vb_ctx* ctx, const float* mel, int B, int T, float* moments, void* ws, void* stream);
/* HifiGAN.spec2wav (vocoder/hifigan/hifigan.py:20-30): mel [B][80][T] -> wav [B][T*hop] */
int vb_hifigan_forward(vb_ctx* ctx, const float* mel, int B, int T, float* wav, void* ws, void* stream);
/* HiFi-GAN with ROW LENGTHS (build-defined): mels of different lengths as rows of one call.  mel [B][in_ch][T], T the padded length;
 * lens->len the HOST array of B mel-frame lengths, 1 <= len[b] <= T, checked like the sampler's (B <= 64; VB_E_INVALID names the row,
 * nothing is launched and wav is unchanged).  wav [B][out_ch][T*hop]: row b holds len[b]*hop samples followed by exact zeros.  The
 * caller's mel padding, samples [len[b], T) of a row, is never read into a valid sample; it may hold NaN.
 * lens == NULL, len == NULL or every row full is vb_hifigan_forward on the same buffers: same launches, same bits.
 * How it works.  Every input activation of the generator is a LeakyReLU or none (f(0) = 0), every convolution zero-pads, and every op
 * computes a clip from that clip alone.  So when row b's tail is zero in every activation buffer a convolution reads, its valid samples get
 * exactly the operands the zero fill of the clip-alone call supplies: the mel is copied into the workspace with its tails zeroed, and after
 * every op that writes an activation buffer (the output included) one small launch zeroes out[b, :, len[b]*tmul : T*tmul] - its grid covers
 * the tails only.  The fused ResBlock1 pairs keep their intermediate in LDS and pad the ACTIVATED intermediate with zeros outside [0, T):
 * with lengths that bound is the row's own length (a device table of the lengths in the workspace), at that one place of each kernel.
 * THE ROUTE RULE.  Kernel routes depend on a stage's length T*tmul only through (T*tmul) % 4 - minimal-filtering eligibility, staged
 * (16-byte) epilogues, quad window rows, the fp32 pairs - and through 16-byte alignment of the row bases, which follows from it.  (T and B
 * also enter the TILE choice of the conv and GEMM kernels; every tile of a kernel accumulates in the same order, so tiles never change a
 * bit.)  This call picks routes from the padded T, the call on the clip alone from len[b].  Hence:
 *   len[b] == T (mod 4)   row b's first len[b]*hop samples equal vb_hifigan_forward on that clip alone BIT FOR BIT;
 *   otherwise             the two agree to fp32 roundoff (an op may run the direct kernel in one call and the F(2,3) kernel in the other).
 * A host that wants bit-exact rows groups its clips by length mod 4 (harness.plan_vocoder_calls).
 * Refused with VB_E_INVALID before anything is launched, naming the op and why: a vocoder program with an op other than VB_OP_CONV /
 * VB_OP_RESPAIR / VB_OP_XT_PLANES (BigVGAN's VB_OP_AA_ACT: its anti-aliasing filters replicate-pad at the row end), an input activation
 * other than none / LeakyReLU, GroupNorm statistics, dynamic channel counts, w_buf weights, a transposed output.  The VAE decoder,
 * the VAE encoder, the chunked vocoder and BigVGAN have their own entry points (vb_vae_decode_lens, vb_vae_encode_lens,
 * vb_hifigan_forward_chunked_lens, vb_bigvgan_forward_lens / vb_bigvgan_forward_chunked_lens).
 * ws: vb_hifigan_lens_workspace_bytes(ctx, B, T) bytes = vb_net_workspace_bytes + the masked mel + the length table.  Hosts detect the
 * feature by the presence of these symbols (vb_abi_version() stays 3). */
size_t vb_hifigan_lens_workspace_bytes(vb_ctx* ctx, int B, int T);
int vb_hifigan_forward_lens(vb_ctx* ctx, const float* mel, int B, int T, const vb_lens* lens, float* wav, void* ws, void* stream);
/* VAE decoder with ROW LENGTHS (build-defined): latents of different lengths as rows of one decode call.  z [B][zc][T], T the padded latent
 * length; lens->len the HOST array of B latent lengths, 1 <= len[b] <= T, B <= 64, checked like the sampler's (VB_E_INVALID names the row,
 * nothing is launched and mel is unchanged).  mel [B][80][2T]: row b holds 2*len[b] frames that are vb_vae_decode on that clip alone,
 * followed by exact zeros.  The caller's latent padding is never read into a valid frame (it may hold NaN), and neither is anything
 * already in the workspace (0xFF bytes give the bits of a zeroed one).  Row b does not depend on the other rows' contents or lengths.
 * lens == NULL, len == NULL or every row full is vb_vae_decode on the same buffers: same launches, same bits.
 * How it works.  The latent is copied into the workspace with its tails zeroed and every op that writes an activation buffer is followed
 * by the tail-zero launch of the HiFi-GAN call (a transposed output [T][C] as one row of T*C samples per clip), so every raw buffer a
 * convolution reads is zero behind row b's end.  Zero tails alone do not settle the decoder; three things read the device table of lengths:
 *   GroupNorm statistics     gn_stats_kernel<LENS> reduces row b's own cpg x len[b]*tmul samples at pitch T*tmul with the thread assignment,
 *                            the float4 grouping (x+y)+(z+w) and the two-pass final order of the plain form on the compacted clip (one body).
 *   GroupNorm (+ swish) in   every consumer pads the ACTIVATED tensor with zeros from len[b]*tmul on instead of T*tmul: conv_tile's one bound for
 *                            the register-staged convolutions (fp32, split, bf16), gn_apply_kernel (zeros behind the row end),
 *                            xt_planes_kernel (zero rows behind it).
 *   attention                softmax_rows_t_kernel<LENS> takes max and sum over the keys c < len[b] (lane stride and order of the plain form
 *                            at len[b] columns) and writes exact zeros for the keys and queries behind the row's end; q, k, v (transposed
 *                            or not) are tail-zeroed and the split planes are made from them, so every added term of the two products -
 *                            Co or Ci = the padded T - is an exact 0 * 0.  The score buffer gets no tail pass: only the row's own block is read.
 * THE ROUTE RULE.  Beside (T*tmul) % 4 and row alignment (the vocoder's rule: staged epilogues, quad window rows, minimal filtering, and
 * here the float4 paths of gn_apply / gn_stats), the attention's two products take a channel count from the length.  None of those
 * predicates changes a bit: Ci % 16 and Co % 4 choose between the DMA-fed and the register-staged exact-fp32 kernel, which are
 * bit-identical (one chunk order); the split planes round Ci to 32 (Ci_pad, cpad) with zero columns, and a longer padded Ci only appends
 * all-zero chunks behind the clip's own; Ci % 64 is a condition of the conv-as-GEMM route, which a product with per-clip weights never
 * takes.  (T and B also enter the tile choice; tiles never change a bit.)  What changes bits is the vocoder's residue, hence:
 *   len[b] == T (mod 4)   row b's 2*len[b] frames equal vb_vae_decode on that clip alone BIT FOR BIT, in every precision;
 *   otherwise             the two agree to the precision's roundoff (an op may run the direct kernel in one call and the F(2,3) kernel in
 *                         the other, or a glue kernel its float4 path).
 * No op had to be excepted.  A host that wants bit-exact rows groups its clips by length mod 4 (harness.plan_decode_calls).
 * Refused with VB_E_INVALID before anything is launched, naming the op and why: VB_OP_AA_ACT, VB_OP_RESPAIR, in_stride > 1, tr_stride > 1
 * (ops the decoder's program does not contain).  The VAE encoder (Downsample1D pads on the right of the row's own end) takes lengths
 * through vb_vae_encode_lens (below), BigVGAN through vb_bigvgan_forward_lens.
 * ws: vb_vae_decode_lens_workspace_bytes(ctx, B, T) bytes = vb_net_workspace_bytes + the masked latent + the length table.  Hosts detect
 * the feature by the presence of these symbols (vb_abi_version() stays 3, vb_net_op is unchanged). */
size_t vb_vae_decode_lens_workspace_bytes(vb_ctx* ctx, int B, int T);
int vb_vae_decode_lens(vb_ctx* ctx, const float* z, int B, int T, const vb_lens* lens, float* mel, void* ws, void* stream);
/* VAE encoder with ROW LENGTHS (build-defined): mels of different lengths as rows of one encode call.  ONE UNIT, LATENT TOKENS, serves
 * encode, sample and decode: T is the padded LATENT length and lens->len the HOST array of B latent lengths, 1 <= len[b] <= T, B <= 64,
 * checked like the sampler's (VB_E_INVALID names the row, nothing is launched and moments is unchanged).  mel [B][in_ch][T*in_tmul]
 * (in_tmul = 2^downsamplings, 2 in the shipped config): row b owns mel frames [0, len[b]*in_tmul); a mel whose length is no multiple of
 * in_tmul has no latent length and is not described by this call.  moments [B][2*embed][T]: row b holds len[b] columns that are
 * vb_vae_encode on that clip alone, followed by exact zeros.  The caller's mel padding is never read into a valid value (it may hold NaN),
 * and neither is anything already in the workspace (0xFF bytes give the bits of a zeroed one).  Row b does not depend on the other rows'
 * contents or lengths.  lens == NULL, len == NULL or every row full is vb_vae_encode on the same buffers: same launches, same bits.
 * How it works.  The decoder's scheme (above) on the encoder's program: the mel is copied into the workspace with its tails zeroed from
 * len[b]*in_tmul on, every op that writes an activation buffer is followed by the tail-zero launch at that buffer's own rate, and GroupNorm
 * statistics, GroupNorm (+ swish) inputs - the k = 5 convolutions, gn_apply, xt_planes - and the mid attention read the device table of
 * lengths exactly as there.  What the decoder does not contain is Downsample1D: one zero on the right of the clip, then a k = 3 stride-2
 * convolution, which the program runs as two polyphase VB_OP_CONVs with in_stride = 2 (phase 0: taps 0 and 2 with the bias; phase 1: tap
 * 1 with beta = 1), both without input activation.  They get NO length table (launch_conv1d goes on refusing row lengths with in_stride):
 * the last output of row b reaches for x[2*len'] (len' = the row's length at the output's rate), the first sample of the tail the previous
 * op's tail pass zeroed - the reference's right pad on the clip alone - and for a full row it is the kernel's own zero padding behind
 * T_eff = T_in / 2, as in the plain call.  The tail pass after the first of the two clears the bias it wrote behind the row's end, the
 * second adds w1 * 0 to that zero.
 * THE ROUTE RULE.  The stages run at tmul = in_tmul .. 1, so the predicates see (T*tmul) % 4.  Everything that looks at a length on the
 * encoder's routes: T_eff of the strided convolutions (T_in / in_stride of the PADDED row for both phases, a function of T alone - the row's
 * own end is the zero tail, not a bound); staged (16-byte) epilogues (T_out % 4, row alignment); quad window rows and F(2,3) eligibility of
 * the stride-1 k = 3 / 5 convolutions without GroupNorm input (T % 4; the strided pair never qualifies for either: in_stride == 1 is a
 * condition of the DMA-fed and the minimal-filtering kernels); the float4 paths of gn_stats (cpg * len * tmul % 4) and gn_apply (T % 4), which
 * regroup loads, and in gn_stats the partial sums; the attention's channel counts (Ci % 16 / Co % 4 between two bit-identical fp32 kernels,
 * Ci_pad rounding with zero columns, Ci % 64 of a route per-clip weights never take).  Tiles never change a bit.  (T*tmul) % 4 for every
 * tmul in {in_tmul .. 1} is a function of T % 4, so the decoder's rule holds with the same modulus:
 *   len[b] == T (mod 4)   row b's len[b] columns equal vb_vae_encode on that clip alone BIT FOR BIT, in every precision;
 *   otherwise             the two agree to the precision's roundoff.
 * A host that wants bit-exact rows groups its clips by latent length mod 4 (harness.plan_encode_calls).
 * Refused with VB_E_INVALID before anything is launched, naming the op and why: upsample2, tr_stride > 1, VB_OP_AA_ACT and VB_OP_RESPAIR
 * (not ops of the encoder's program), and in_stride > 1 on anything but a VB_OP_CONV with in_act none and stats = -1 (an activated
 * down-convolution would pad the activated row).  vb_vae_decode_lens goes on refusing in_stride > 1.
 * ws: vb_vae_encode_lens_workspace_bytes(ctx, B, T) bytes = vb_net_workspace_bytes + the masked mel + the length table.  Hosts detect
 * the feature by the presence of these symbols (vb_abi_version() stays 3, vb_net_op is unchanged). */
size_t vb_vae_encode_lens_workspace_bytes(vb_ctx* ctx, int B, int T);
int vb_vae_encode_lens(vb_ctx* ctx, const float* mel, int B, int T, const vb_lens* lens, float* moments, void* ws, void* stream);
/* The posterior of those moments with row lengths (build-defined; DiagonalGaussianDistribution.sample / .mode and the scale of
 * get_first_stage_encoding in one launch).  moments [B][2E][T] (mean = channels [0, E), logvar = [E, 2E)), noise [B][E][T] or NULL, in fp32:
 *   z[b][c][t] = scale * (mean + expf(0.5f * clamp(logvar, -30, 20)) * noise)   for t <  len[b]       (noise == NULL: scale * mean)
 *   z[b][c][t] = 0                                                              for t >= len[b]
 * len: HOST array of B lengths (1 <= len[b] <= T, B <= 64, checked as above; they travel by value in the launch, nothing is allocated);
 * NULL = full rows.  Neither the noise nor the moments are read behind a row's end (both may hold NaN there): the zero tail of the moments is
 * logvar = 0, std = 1, so the elementwise form would leave the noise in z's padding, which the sampler's contract forbids.  16-byte
 * accesses when T % 4 == 0 and the three bases are 16-byte aligned, 4-byte otherwise; same values either way. */
int vb_posterior_lens(const float* moments, const float* noise /* NULL = mode */, int B, int E, int T,
                      const int32_t* len /* HOST, NULL = full rows */, float scale, float* z, void* stream);

/* Long-form generation (BASELINE configs[4]; build-defined, the reference stops at max_len = 1500 latent tokens: vocal2music_moe.py:421).
 * vb_crossfade_windows: window results parts [nw*B][C][n] (row = w*B + b; windows of equal length n starting at starts[w], a HOST array,
 * covering [0, T) with overlaps) -> out [B][C][T], linear cross-fade over every overlap, weights normalised to one (ramp weights
 * (u + 1) / (ov + 1) in fp32: equal to torch.linspace(0, 1, ov + 2)[1:-1] up to fp32 rounding of the ramp, ~1 ulp, not bit for bit).
 * vb_hifigan_forward_chunked: HifiGAN.spec2wav over a long mel in chunks of `chunk` frames with `halo` frames of context on both sides -
 * identical to whole-clip vocoding when halo >= the generator's receptive field; scratch_in >= B*in_ch*(chunk + 2*halo) floats,
 * scratch_out >= B*out_ch*(chunk + 2*halo)*hop floats, ws = vb_net_workspace_bytes(ctx, VB_NET_VOCODER, B, chunk + 2*halo). */
int vb_crossfade_windows(const float* parts, const int32_t* starts, int nw, int B, int C, int n, int T, float* out, void* stream);
int vb_hifigan_forward_chunked(vb_ctx* ctx, const float* mel, int B, int T, int chunk, int halo, float* wav, void* ws, float* scratch_in,
                               float* scratch_out, void* stream);
/* The chunked vocoder with ROW LENGTHS (build-defined): long mels of different lengths as rows of one chunked call.  mel [B][in_ch][T], T
 * the padded length; lens->len the HOST array of B mel-frame lengths, 1 <= len[b] <= T, B <= 64.  wav [B][out_ch][T*hop] is written
 * completely: row b holds len[b]*hop samples followed by exact zeros.  The mel padding is never read (it may hold NaN).
 * THE PLAN (vb_hifigan_chunked_lens_plan; host only, launches nothing; the entry point runs the same function).  The chunk grid is the one
 * of vb_hifigan_forward_chunked: s = 0, chunk, 2*chunk, ... < T, e = min(s + chunk, T), lo = max(0, s - halo); T <= chunk + 2*halo is ONE
 * step over the whole rows (s = lo = 0, e = T), as there.  In chunk k the ACTIVE rows are those with len[b] > s, in ascending b - a row
 * that ended before the chunk is not run at all; active row j has n_j = min(len[b], s + chunk + halo) - lo >= 1 frames inside the chunk
 * (n_j = len[b] in the one-step case); the chunk's width is tc_k = max_j n_j (every row full: the hi - lo of the plain loop).  The export
 * writes s, lo, tc, n_active [n_chunks] and rows, n [n_chunks][64] (entries j >= n_active: -1 and 0); chunk k keeps the frames
 * [s_k, min(e_k, len[b])) of an active row, e_k = s_(k+1) or T.  VB_E_INVALID when the grid has more than max_chunks steps (*n_chunks then
 * holds the count) or an argument is refused.
 * PER CHUNK: one gather launch copies the active rows into scratch_in, compact [n_active][in_ch][tc_k], exact zeros at t >= n_j by a
 * select (the masked input: nothing outside [lo, lo + tc_k) of an active row and nothing of an inactive row is read); the length table of
 * {n_j} is written; the generator runs on n_active rows of tc_k frames with those lengths (vb_hifigan_forward_lens's machinery; the plain
 * run when every active row is full); one scatter launch writes samples [s*hop, e*hop) of ALL B rows: row b's up to min(e, len[b])*hop
 * from its compact row at (s - lo)*hop, exact zeros behind, and all of an inactive row.  Both kernels use 16-byte accesses when the base
 * pointers, the row pitches and lo, tc_k, T (gather) / hop (scatter) allow, 4-byte ones otherwise - same bits either way.
 * CONTRACT.  Row b's first len[b]*hop samples are the chunk loop over that clip alone ON THE SAME GRID: for each s the plain
 * vb_hifigan_forward of mel[b, :, lo : min(len[b], s + chunk + halo)], of which the samples of [s, min(e, len[b])) are kept.  They match
 * BIT FOR BIT in every chunk where n_j == tc_k (mod 4) - kernel routes depend on a length only through that residue (THE ROUTE RULE of
 * vb_hifigan_forward_lens) - and to fp32 roundoff elsewhere.  The residue condition holds in every chunk when chunk, halo, T and every
 * len[b] are multiples of 4; the plan export shows, per chunk and row, whether it holds.  (The clip alone on ITS OWN grid -
 * vb_hifigan_forward_chunked at T = len[b] - differs where a chunk's trailing halo is cut by len[b] < T only in the one-step rule: a clip
 * with len[b] <= chunk + 2*halo < T is chunked here and run whole there; the two agree like chunked and whole vocoding do.)
 * lens == NULL, lens->len == NULL or every row full: vb_hifigan_forward_chunked on the same buffers, same launches, same bits.
 * T <= chunk + 2*halo: vb_hifigan_forward_lens (the workspace below covers it).
 * Refused with VB_E_INVALID before anything is launched, wav untouched: B > 64 or a length outside [1, T] (the row is named), chunk < 1 or
 * halo < 0, no vocoder loaded, a program that takes no row lengths (the message of vb_hifigan_forward_lens, naming the op: BigVGAN's
 * VB_OP_AA_ACT, which vb_bigvgan_forward_chunked_lens takes).  scratch_in / scratch_out as for vb_hifigan_forward_chunked at (B, chunk + 2*halo); ws:
 * vb_hifigan_chunked_lens_workspace_bytes = the net's workspace at (B, chunk + 2*halo) + the length table, or the lens call's at (B, T).
 * Hosts detect the feature by the presence of these symbols (vb_abi_version() stays 3). */
size_t vb_hifigan_chunked_lens_workspace_bytes(vb_ctx* ctx, int B, int T, int chunk, int halo);
int vb_hifigan_forward_chunked_lens(vb_ctx* ctx, const float* mel, int B, int T, int chunk, int halo, const vb_lens* lens, float* wav, void* ws,
                                    float* scratch_in, float* scratch_out, void* stream);
int vb_hifigan_chunked_lens_plan(int B, int T, int chunk, int halo, const int32_t* len, int max_chunks, int32_t* s, int32_t* lo, int32_t* tc,
                                 int32_t* n_active, int32_t* rows, int32_t* n, int* n_chunks);
/* BigVGAN with ROW LENGTHS (build-defined), for a program loaded as VB_NET_VOCODER: mels of different lengths as rows of one vocoder call,
 * whole rows or chunked.  Arguments, checks and workspaces as for vb_hifigan_forward_lens / vb_hifigan_forward_chunked_lens: mel
 * [B][in_ch][T], T the padded length; lens->len the HOST array of B mel-frame lengths, 1 <= len[b] <= T, B <= 64.
 * CONTRACT.  Row b's first len[b]*hop samples are vb_hifigan_forward on that clip alone - BIT FOR BIT when len[b] == T (mod 4), to the
 * precision's roundoff otherwise: THE ROUTE RULE of vb_hifigan_forward_lens, unchanged (VB_OP_AA_ACT adds no predicate on a length: one
 * kernel, one tile grid from sample 0, whatever T).  The rest of the row is exact zeros.  The caller's mel padding is never read into a
 * valid sample (it may hold NaN).  lens == NULL, len == NULL or every row full is vb_hifigan_forward (chunked: vb_hifigan_forward_chunked)
 * on the same buffers: same launches, same bits.  The chunked call is the chunk loop over the clip alone on the same grid, in the words
 * of vb_hifigan_forward_chunked_lens (plan: vb_hifigan_chunked_lens_plan; bit for bit in every chunk where n_j == tc_k (mod 4)).
 * How it works.  The generator's convolutions have no input activation and zero-pad, its transposed convolutions are the HiFi-GAN's,
 * residual adds and tanh write buffers that get the tail-zero launch: the zero-tail machinery of vb_hifigan_forward_lens carries them.
 * VB_OP_AA_ACT, out = down2(snake(up2(x))), REPLICATE-pads at the row end in both filters, which no tail value can stand in for: its kernel
 * reads the device table of lengths and takes row b's end, len[b]*tmul, for the three bounds that are T in the plain call - the clamp of
 * the input window, the clamp of the up-sampled index, the store bound.  Nothing at or behind x[b][c][len[b]*tmul] is loaded (whatever an
 * earlier op left there, NaN included), the outputs behind the row's end are written as exact zeros by the same kernel (no tail-zero
 * launch follows it), and a workgroup whose 256 outputs all lie behind the end stores zeros and returns before it loads anything.  A
 * valid output is computed by the instructions of the plain call in their order.
 * Refused with VB_E_INVALID before anything is launched, wav untouched: B > 64 or a length outside [1, T] (the row is named), chunk < 1
 * or halo < 0, no vocoder loaded, and a program with an op other than VB_OP_CONV / VB_OP_RESPAIR / VB_OP_XT_PLANES / VB_OP_AA_ACT or with
 * anything else vb_hifigan_forward_lens refuses (the op is named).  The HiFi-GAN entry points keep refusing VB_OP_AA_ACT.
 * ws: vb_bigvgan_lens_workspace_bytes = vb_net_workspace_bytes + the masked mel + the length table; chunked:
 * vb_bigvgan_chunked_lens_workspace_bytes = vb_hifigan_chunked_lens_workspace_bytes, scratch_in / scratch_out as there.  Hosts detect
 * the feature by the presence of these symbols (vb_abi_version() stays 3, vb_net_op is unchanged). */
size_t vb_bigvgan_lens_workspace_bytes(vb_ctx* ctx, int B, int T);
int vb_bigvgan_forward_lens(vb_ctx* ctx, const float* mel, int B, int T, const vb_lens* lens, float* wav, void* ws, void* stream);
size_t vb_bigvgan_chunked_lens_workspace_bytes(vb_ctx* ctx, int B, int T, int chunk, int halo);
int vb_bigvgan_forward_chunked_lens(vb_ctx* ctx, const float* mel, int B, int T, int chunk, int halo, const vb_lens* lens, float* wav, void* ws,
                                    float* scratch_in, float* scratch_out, void* stream);

/* ------------------------------------------------------------ T5 text encoder ----
 * FrozenTextVocalEmbedder.forward (ldm/modules/encoders/modules.py:216-233): T5EncoderModel(input_ids).last_hidden_state, no
 * attention mask.  HF T5 encoder stack (transformers T5Stack / T5Block / T5Attention / T5DenseGatedActDense / T5LayerNorm):
 * per block  x += O(softmax(Q K^T + rel_pos_bias) V)  on RMS-normed x (no 1/sqrt(d) scaling), x += Wo(gelu_new(Wi0 n) * Wi1 n);
 * final RMS norm.  Runs in split precision (fp32-class) on the same GEMM kernel as the DiT.  The tokenizer stays upstream. */
#define VB_T5_MAX_LAYERS 48
typedef struct { int vocab, d_model, d_kv, heads, d_ff, layers; float eps; } vb_t5_config;
typedef struct {
    const float* ln0;     /* layer.0.layer_norm.weight [d_model] */
    const void* wqkv;     /* planes(2) [3*heads*d_kv][d_model]: q | k | v rows */
    const void* wo;       /* planes(2) [d_model][heads*d_kv] */
    const float* ln1;     /* layer.1.layer_norm.weight */
    const void* wi;       /* planes(2) [2*d_ff][d_model]: rows interleaved wi_0[j], wi_1[j] */
    const void* wo_ff;    /* planes(2) [d_model][d_ff] */
} vb_t5_layer;
typedef struct {
    const float* embed;       /* shared.weight [vocab][d_model] */
    const float* pos_bias;    /* [heads][Lmax][Lmax] relative-position bias of block 0 (shared by all blocks), built by the host */
    int pos_len;              /* Lmax */
    const float* final_ln;    /* encoder.final_layer_norm.weight */
    const float* ones;        /* [d_model] ones (residual "gate") */
    vb_t5_layer layers[VB_T5_MAX_LAYERS];
} vb_t5_weights;
int vb_t5_load(vb_ctx* ctx, const vb_t5_config* cfg, const vb_t5_weights* w);
size_t vb_t5_workspace_bytes(const vb_t5_config* cfg, int B, int L);
/* ids int64 [B][L] -> out f32 [B][L][d_model] */
int vb_t5_encode(vb_ctx* ctx, const int64_t* ids, int B, int L, float* out, void* ws, void* stream);

/* ------------------------------------------------------------ log-mel front-end ----
 * MelNet.forward (preprocess/NAT_mel.py:64-86): clamp to [-1, 1]; reflect-pad (n_fft - hop)/2 samples on both sides (:71; when
 * `center` is set torch.stft reflect-pads the padded signal by n_fft/2 once more); STFT (n_fft, hop; the Hann window - zero-padded to n_fft when win < n_fft - is
 * folded into the basis); sqrt(re^2 + im^2 + 1e-9); mel_basis @ .; log10(max(., 1e-5)).  n_fft must be a multiple of the hop:
 * the windowed DFT of all frames then is one convolution over hop-blocks on the exact-fp32 MFMA convolution kernel.
 *   dft_w   f32 [n_fft/hop][hop][Co4], Co4 = 2*im_off, im_off = roundup(n_fft/2 + 1, 4): column f (< n_fft/2 + 1) = w[n] cos(2 pi f n / n_fft),
 *           column im_off + f = -w[n] sin(2 pi f n / n_fft), n = tap*hop + c; other columns zero
 *   basis_t f32 [n_fft/2 + 1][n_mels]  (the mel filterbank, transposed)
 *   wav f32 [B][L] -> mel f32 [B][n_mels][T] and / or spec f32 [B][T][Co4] (either may be NULL), T = vb_melnet_frames() */
typedef struct { int n_fft, hop, n_mels; } vb_mel_config;
int vb_melnet_load(vb_ctx* ctx, const vb_mel_config* cfg, const float* dft_w, const float* basis_t);
int vb_melnet_frames(const vb_mel_config* cfg, int L, int center);
size_t vb_melnet_workspace_bytes(const vb_mel_config* cfg, int B, int L, int center);
int vb_melnet_forward(vb_ctx* ctx, const float* wav, int B, int L, int center, float* mel, float* spec, void* ws, void* stream);
/* The front-end with ROW LENGTHS (build-defined): waveforms of different lengths as rows of one call.  wav [B][L], L the padded length;
 * lens->len the HOST array of B lengths in samples, checked like the sampler's (B <= 64, 1 <= len[b] <= L) and then row by row for what the
 * plain call needs of its one L: pad < len[b], n_fft/2 < len[b] + 2 pad when `center`, T_b = vb_melnet_frames(cfg, len[b], center) >= 1.
 * VB_E_INVALID names the row; nothing is launched and mel / spec are unchanged.
 * THE CONTRACT.  Row b's first T_b frames of mel (and of spec) are vb_melnet_forward on that clip alone; the rest of the row, frames
 * [T_b, T), is exact zero - 0.0f in mel, not log10(1e-5) - and the padding of wav, samples [len[b], L) of a row, is not read (it may
 * hold NaN).  Row b does not depend on the other rows' contents or lengths.
 * lens == NULL, len == NULL or every row full is vb_melnet_forward on the same buffers: same launches, same bits.
 * How it works.  Zero padding cannot imitate the clip alone: both reflections (by pad, and by n_fft/2 when centred) turn round at the
 * row's own end, so the framing kernel reads the end from a device table of the lengths, writes exact zeros from hop-block
 * J_b = T_b + n_fft/hop - 1 on and loads nothing behind len[b].  The STFT stays the one convolution over the padded block count.  Its
 * frames t >= T_b still see row b's last n_fft/hop - 1 blocks, so spec (the caller's, or the workspace's) gets the conv nets' tail pass - one
 * row of (T - T_b) * Co4 samples per clip - and the mel tail kernel stores 0.0f for t >= T_b from a table of the T_b.
 * BIT FOR BIT, ALWAYS.  The convolution has fp32 weights, no minimal-filtering form and a transposed output (no staged epilogue), so it
 * runs one of the two exact-fp32 kernels: the DMA-fed one when T + n_fft/hop - 1 is a multiple of 4, the register-staged one otherwise
 * (vb_conv1d_plan: VB_ROUTE_F32G / VB_ROUTE_F32).  The two are bit-identical - one chunk, tap and channel-pair order - and so is every
 * tile of either (T and B enter the tile choice only), so an output element's accumulation order depends on neither T nor B nor the
 * route: no congruence between len[b] and L is needed, and a host has nothing to group.  The framing and the mel tail are per-element.
 * ws: vb_melnet_lens_workspace_bytes(cfg, B, L, center) = vb_melnet_workspace_bytes + the two length tables.  Hosts detect the feature by
 * the presence of these symbols (vb_abi_version() stays 3). */
size_t vb_melnet_lens_workspace_bytes(const vb_mel_config* cfg, int B, int L, int center);
int vb_melnet_forward_lens(vb_ctx* ctx, const float* wav, int B, int L, int center, const vb_lens* lens, float* mel, float* spec, void* ws,
                           void* stream);
/* Masked mean absolute distance of two log-mels (the two numbers of scripts/infer_batched.py --eval_mel), no vb_ctx: a f32 [B][M][Ta],
 * b f32 [B][M][Tb], frames the HOST array of B frame counts to compare, checked like row lengths (B <= 64, 1 <= frames[r] <= min(Ta, Tb);
 * VB_E_INVALID names the row, nothing is launched).  With d = a - b over m < M, t < frames[r] and N = M * frames[r]:
 *     mu_r = remove_offset ? sum(d) / N : 0;     out[r] = sum |d - mu_r| / N;     out_offset[r] = mu_r   (out_offset may be NULL)
 * Nothing behind frames[r] is loaded (it may hold NaN).  One launch, one workgroup of 1024 threads per row, two passes over the row.  The
 * reduction shape is fixed: thread x adds elements i = x, x + 1024, ... (i = m * frames[r] + t) in ascending order into one fp32
 * accumulator, then an LDS tree of 10 levels; no atomics.  The result is a pure function of the inputs and identical from run to run,
 * and the longest chain of additions behind a sum is k = ceil(N / 1024) + 10, so |out - exact| <= 2 k 2^-24 (mean |d| + |mu|).
 * ws: vb_mel_dist_workspace_bytes(B) bytes (the device copy of frames; 0 for a B outside 1..64). */
size_t vb_mel_dist_workspace_bytes(int B);
int vb_mel_dist_lens(const float* a, int Ta, const float* b, int Tb, int B, int M, const int32_t* frames /* HOST */, int remove_offset,
                     float* out, float* out_offset /* nullable */, void* ws, void* stream);

/* ------------------------------------------------------------------- unit kernels ---- */
/* RMSNorm (flag_large_dit_moe.py:52-77) * w then modulate (:80-81); shift/scale [B][mod_ld] or NULL */
int vb_rmsnorm_modulate(const float* h, const float* w, const float* shift, const float* scale, int mod_ld, int rows, int D,
                        int T, float eps, void* out_planes, int np, void* stream);
/* first argmax of logits + gumbel (hard Gumbel-softmax, vocal2music_moe.py:81-93) */
int vb_router_top1(const float* logits, const float* gumbel, int N, int E, int32_t* idx, void* stream);
/* stable bucketing of tokens by (caption, acoustic) expert: group_off int32[2E+1]; perm int32[2N + scratch] where the
 * first 2N entries are the slot -> token permutation and scratch = vb_route_bucket_scratch_ints(N, E) */
int vb_route_bucket_scratch_ints(int N, int E);
int vb_route_bucket(const int32_t* ic, const int32_t* ia, int N, int E, int32_t* group_off, int32_t* perm, void* stream);
/* the same bucketing ranked by (caption expert, acoustic expert) PAIR (E*E <= 16), what the single-launch routed w2 product reads
 * (vocal2music_moe.py:154-167): pair_off int32[E*E+1] in caption-major order; the caption slots [0,N) ARE the pair slots, the acoustic
 * slots [N,2N) hold the same buckets acoustic-major; pair_pa int32[N] = acoustic slot of the token in pair slot p.  Inside an expert
 * group the rows are ordered by (other expert, token) instead of by token */
int vb_route_bucket_pairs(const int32_t* ic, const int32_t* ia, int N, int E, int32_t* group_off, int32_t* perm, int32_t* pair_off,
                          int32_t* pair_pa, void* stream);
/* generic GEMM  C[M][N] f32 = A[M][K] planes x B[N][K]^T planes (+bias) */
int vb_gemm_bf16(const void* A, const void* Bw, const float* bias, int M, int N, int K, int np, float* C, void* stream);
/* grouped SwiGLU expert FFN (FeedForward, flag_large_dit_moe.py:480-485) over routed buckets:
 *   u planes [Ntok][D]; perm/group_off from vb_route_bucket (G groups); w13 [G][2H][D] interleaved, w2 [G][D][H];
 *   out f32 [Ntok][D] = row_scale[tok] * FFN_g(u[tok]) written at perm order; hidden scratch planes [Nslots][H] */
int vb_grouped_swiglu(const void* u, const int32_t* perm, const int32_t* group_off, int G, int n_slots, const void* w13,
                      const void* w2, const float* row_scale, int D, int H, int np, void* hidden, float* out, void* stream);
/* The MoE block's fused kernels, each alone (bf16 mode only; no eligibility rule and no token-count threshold of the engine applies):
 * band-expert FFN in one launch (vocal2music_moe.py:171-178): expert e reads band e of y and updates band e of out32 in place,
 *   out32[m][e*band + n] += gate[m / T][e*band + n] * ( W2_e . (silu(W1_e y_e[m]) * (W3_e y_e[m])) )[n]
 *   y bf16 [M][ldy]; w13 bf16 [E][2H][band], w1 / w3 rows interleaved; w2 bf16 [E][band][H]; gate f32 [ceil(M / T)][gate_ld];
 *   out32 f32 [M][ldc32].  band = 192 or 96, H % 64 == 0, E divides 8. */
int vb_band_ffn(const void* y, int ldy, const void* w13, const void* w2, int M, int H, int E, int band, const float* gate, int gate_ld, int T,
                float* out32, int ldc32, void* stream);
/* routed experts in the pair form (vocal2music_moe.py:152-167), the two launches of the engine: the grouped SwiGLU over the 2E expert groups
 * of group_off with the gate weights folded into the hidden rows (slot < N: mc[token], otherwise ma[token]; token = perm[slot]) ->
 * hidden bf16 [2N][H]; then the pair-bucketed second product -> out bf16 [N][D] = Hs[p] W2[c]^T + Hs[pair_pa[p]] W2[E + a]^T at row perm[p].
 *   u bf16 [N][D]; perm / group_off / pair_off / pair_pa from vb_route_bucket_pairs; w13 bf16 [2E][2H][D] interleaved; w2 bf16 [2E][D][H];
 *   mc, ma f32 [N].  H % 64 == 0, D % 16 == 0, E*E <= 16. */
int vb_routed_ffn_pair(const void* u, const int32_t* perm, const int32_t* group_off, const int32_t* pair_off, const int32_t* pair_pa, const void* w13,
                       const void* w2, const float* mc, const float* ma, int N, int D, int H, int E, void* hidden, void* out, void* stream);
/* folded caption gate + router (vocal2music_moe.py:117-151) on the caller's operands, N = Beff * T token rows, row = (branch * B + b) * T + t:
 *   x bf16 [N][K] token features; keys bf16 [Beff][NS][K] folded keys; score_bias f32 [Beff][NS]; vw f32 [Beff][NS][E]; bg f32 [E];
 *   score column = key * Hh + head; logit_e = sum over heads and keys of softmax_keys(x . keys^T + score_bias) * vw[..][e]  (+ bg[e])
 *   la f32 [la_rows][E] acoustic logits, row n % la_rows; hl f32 [Beff][hl_ld], columns 0 / 1 = the high-level gate's logits of row n / T;
 *   g1 [N][2], g2 [N][E], g3 [N][E] injected Gumbel noise, or all null: drawn on the device from (seed, clip_base + b, nfe, branch, block)
 *   ic = argmax(logit + bg + g2), ia = argmax(la + g3) (first maximum), (mc, ma) = softmax(hl + g1); lc_out (form 0, optional) f32 [N][E] =
 *   logit + bg; cnt (optional, zero on entry) int32 [ceil(N / 256)][cnt_G]: tokens per 256-token block and expert pair ic * E + ia
 *   (cnt_pairs = 1, cnt_G = E*E) or per expert group ic / E + ia (cnt_pairs = 0, cnt_G = 2E).
 * form 0: grouped score GEMM into scores (scratch f32 [N][NS]; clip_off scratch int32 [Beff + 1]) + the router launch;
 * form 1: the one-launch kernel (NS = 640, K = 768, E = 4, Hh = 8; VB_E_INVALID otherwise; lc_out must be null). */
int vb_caption_gate(const void* x, const void* keys, const float* score_bias, const float* vw, const float* bg, const float* la, int la_rows,
                    const float* hl, int hl_ld, const float* g1, const float* g2, const float* g3, uint64_t seed, int64_t clip_base, int nfe,
                    int block, int Beff, int B, int T, int K, int NS, int Hh, int E, int form, float* scores, int32_t* clip_off, int32_t* ic,
                    int32_t* ia, float* mc, float* ma, float* lc_out, int32_t* cnt, int cnt_G, int cnt_pairs, void* stream);
/* the launch that produces attention's inputs, alone: the QKV projection with the RoPE / V-transpose epilogue, as one DiT block runs it
 * (Attention.forward, flag_large_dit_moe.py:381-402).  D = H * hd, row m = b * T + t:
 *   u planes [B*T][D]; wqkv planes [3D][D] (rows: q, k, v thirds); rope_cos / rope_sin f32 [>= T][hd / 2];
 *   q, k planes [B*T][D]: the pair (2j, 2j+1) of every head rotated by (cos, sin)[t][j]; vt planes [B][H][hd][Tpad] = V transposed per head.
 * Only the columns < T of vt are written: the caller owns the pad columns [T, Tpad) (vb_attention needs them finite).  No tile route or
 * store form is chosen here - launch_gemm's own rules and the VB_GEMM_TILE / VB_QKV_* / VB_GEMM_P8_OFF switches apply as in the engine. */
int vb_qkv_rope(const void* u, const void* wqkv, const float* rope_cos, const float* rope_sin, int B, int T, int Tpad, int H, int hd, int np,
                void* q, void* k, void* vt, void* stream);
/* fused self (+cross) attention, head_dim 96 (Attention.forward, flag_large_dit_moe.py:381-402) */
int vb_attention(const void* q, const void* k, const void* vt, const void* ky, const void* vyt, const float* cross_w, int B, int T,
                 int Tpad, int L, int Lpad, int H, int hd, int np, void* out, void* stream);
/* the same with row lengths (the unit of vb_lens): key_len = DEVICE int32 [B], row b's self pass attends over its first key_len[b] keys (K
 * and V^T keep their strides T / Tpad; V^T must be finite up to the end of the last 64-key tile it touches) and its first key_len[b]
 * output rows equal vb_attention on those tokens alone, bit for bit; the output rows from key_len[b] on are finite.  NULL: vb_attention. */
int vb_attention_lens(const void* q, const void* k, const void* vt, const void* ky, const void* vyt, const float* cross_w, int B, int T,
                      int Tpad, int L, int Lpad, int H, int hd, int np, const int32_t* key_len, void* out, void* stream);
/* fp32 Conv1d / ConvTranspose1d on [B][C][T] (weights packed [phase][tap][Ci][Co]); w_x3 != NULL runs the
 * split-bf16 (bf16x3) MFMA kernel on weights packed [2][phase][tap][Co][ci_pad] instead of the exact-f32 MFMA kernel */
int vb_conv1d_f32(const float* x, const float* w, const float* bias, int B, int Ci, int T_in, int Co, int ksize, int dil, int pad,
                  int tr_stride, int tr_pad, int tr_k, int T_out, int in_act, float in_slope, const float* res, float* out,
                  const void* w_x3, int ci_pad, void* stream);
/* Conv1d in fp32 with 1-D minimal filtering (conv1d_f32w.hip; the HiFi-GAN ResBlock convolutions, vocoder/hifigan/modules/hifigan.py:27-64):
 * out = beta*out + alpha*(conv_{k,dil,pad}(act(x)) + bias + res); w = packed [k][Ci][Co] (the fallback when the layer is not eligible),
 * w_mf = the same filter as F(2,3) pseudo-taps [P][Ci][Co] (pack.py:pack_conv_mf).  k = 3 / 5 / 7 / 11, stride 1, Ci % 16 == 0, Co % 4 == 0,
 * Co >= 32, T % 4 == 0 (anything else runs the direct kernels on w).  Agrees with vb_conv1d_f32 to fp32 roundoff, not bit for bit. */
int vb_conv1d_f32_mf(const float* x, const float* w, const float* w_mf, const float* bias, int B, int Ci, int T_in, int Co, int ksize, int dil,
                     int pad, int T_out, int in_act, float in_slope, const float* res, float alpha, float beta, float* out, void* stream);
/* HiFi-GAN ResBlock1 pair in exact fp32, one launch (vocoder/hifigan/modules/hifigan.py:27-64; respair_f32.hip):
 * out = beta*out + alpha*(x + b2 + conv2_{k,1}(lrelu(b1 + conv1_{k,dil}(lrelu(x))))), x / out [B][C][T] (distinct buffers), weights fp32
 * packed [k][C ci][C co]; C = 32 / 64 / 128, odd k <= 17, (k-1)*dil <= 60, T % 4 == 0.  Equals two vb_conv1d_f32 launches bit for bit. */
int vb_respair_f32(const float* x, const float* w1, const float* b1, const float* w2, const float* b2, int B, int C, int T, int k, int dil,
                   float slope, float alpha, float beta, float* out, void* stream);
/* The same pair with F(2,3) minimal filtering in both convolutions (respair_f32w.hip): w1_mf / w2_mf = pseudo-tap weights [P][C][C]
 * (pack.py:pack_conv_mf); C = 32 / 64, k = 3 / 7 / 11, (k-1)*dil <= 60, T % 4 == 0.  Agrees with two vb_conv1d_f32_mf launches to fp32
 * roundoff (about a third of the elements differ by one ulp, < 4e-6 of the output's max-abs), not bit for bit. */
int vb_respair_f32_mf(const float* x, const float* w1_mf, const float* b1, const float* w2_mf, const float* b2, int B, int C, int T, int k, int dil,
                      float slope, float alpha, float beta, float* out, void* stream);
/* Conv1d / ConvTranspose1d in single-pass bf16 (conv1d_bf16.hip), the arithmetic of the conv nets' "bf16" precision, stated exactly:
 *   out = beta*out + alpha*( sum_{ci,j} RN_bf16(W)[j][co][ci] * RN_bf16( act_in(x)[ci][t + j*dil - pad] ) + bias + res )
 * act_in = none / LeakyReLU / GroupNorm affine (+ swish) from gn_mean / gn_rstd [B][gn_groups] and gn_gamma / gn_beta [Ci], applied to the
 * nearest-x2 upsampled (upsample2) or strided (x[i*in_stride + in_phase]) input and padded with zeros AFTER the activation; the
 * activations are rounded to bf16 (round to nearest even) after it; products are exact in fp32 and accumulated in fp32, so only the
 * accumulation order is free.  w_bf16 = ONE plane [phase][tap][Co][ci_pad] (pack.py:pack_conv_bf16, ci_pad = Ci rounded up to 32,
 * 16-byte aligned); the remaining arguments as vb_conv1d_f32.  Not within the 1e-3 parity contract (operand error 2^-9). */
int vb_conv1d_bf16(const float* x, const void* w_bf16, int ci_pad, const float* bias, int B, int Ci, int T_in, int Co, int ksize, int dil,
                   int pad, int tr_stride, int tr_pad, int tr_k, int T_out, int upsample2, int in_stride, int in_phase, int in_act,
                   float in_slope, const float* gn_mean, const float* gn_rstd, const float* gn_gamma, const float* gn_beta, int gn_groups,
                   const float* res, float alpha, float beta, float* out, void* stream);
/* The same convolution over a pre-activated plane, the wide-layer route of the "bf16xt" precision (stride 1 only: tr_stride <= 1,
 * in_stride <= 1): first the planes pre-pass (VB_OP_XT_PLANES, one-plane form) writes RN_bf16(act_in(x)), nearest-x2 upsampled when
 * upsample2, transposed with zero halo rows into planes_scratch (vb_conv1d_bf16_xt_scratch_bytes bytes, 16-byte aligned); then the
 * convolution reads that plane by DMA - as a one-pass GEMM (Co >= 384, Ci % 64 == 0, alpha == 1, beta == 0) or on conv1d_bf16_kernel's
 * DMA-fed input mode (anything else with Co > 64 and Ci % 32 == 0; VB_CONV_GEMM_OFF=1: always).  Same arithmetic definition as
 * vb_conv1d_bf16: the routes differ by where the activation is applied and by accumulation order only.  Hosts detect the "bf16xt"
 * precision by the presence of this symbol (vb_abi_version() stays 3). */
size_t vb_conv1d_bf16_xt_scratch_bytes(int B, int Ci, int T_in, int upsample2);
int vb_conv1d_bf16_xt(const float* x, const void* w_bf16, int ci_pad, const float* bias, int B, int Ci, int T_in, int Co, int ksize, int dil,
                      int pad, int tr_stride, int tr_pad, int tr_k, int T_out, int upsample2, int in_stride, int in_phase, int in_act,
                      float in_slope, const float* gn_mean, const float* gn_rstd, const float* gn_gamma, const float* gn_beta, int gn_groups,
                      const float* res, float alpha, float beta, float* out, void* planes_scratch, void* stream);
/* The planes pre-pass alone: x f32 [B][C][T_in] -> planes [nplanes][B][T_eff + 448][C] bf16 (T_eff = 2 T_in when upsample2), 64 zero rows
 * in front of every clip and 384 behind; nplanes = 2: round-to-nearest value and its rounding residual, 1: the value alone (bit-equal to
 * plane 0 of the two-plane form).  C % 16 == 0; planes 16-byte aligned, vb_xt_planes_bytes bytes. */
size_t vb_xt_planes_bytes(int B, int C, int T_in, int upsample2, int nplanes);
int vb_xt_planes(const float* x, int B, int C, int T_in, int upsample2, int in_act, float in_slope, const float* gn_mean, const float* gn_rstd,
                 const float* gn_gamma, const float* gn_beta, int gn_groups, int nplanes, void* planes, void* stream);
/* The two reductions of vb_vae_decode_lens alone (build-defined units).  len: DEVICE array of B row lengths, 1 <= len[b] <= T; NULL runs
 * the plain kernel.  vb_gn_stats_lens: x [B][C][T] -> mean / rstd [B][groups] (eps 1e-6) over row b's first len[b] samples per channel,
 * the bits of the plain kernel on the compacted clip [C][len[b]].  vb_softmax_rows_t_lens: s [B][T][T] -> the transposed softmax
 * out_t [B][T][T] of row b's leading len[b] x len[b] block, exact zeros elsewhere. */
int vb_gn_stats_lens(const float* x, int B, int C, int T, int groups, const int32_t* len, float* mean, float* rstd, void* stream);
int vb_softmax_rows_t_lens(const float* s, int B, int T, const int32_t* len, float* out_t, void* stream);
/* VB_OP_AA_ACT alone (build-defined unit): x [B][C][T] -> out [B][C][T] = down2(snake(up2(x))) with alpha / inv_beta [C] as the op holds
 * them (alpha exp'ed when log-scale, inv_beta = 1 / (beta + 1e-9)) and filt the 12-tap Kaiser-sinc filter.  len: DEVICE array of B row
 * lengths or NULL (the plain kernel); row b ends at len[b] * len_mul <= T samples (len_mul >= 1: the stage's samples per frame): its valid
 * outputs are the plain kernel's on that clip alone bit for bit, nothing at or behind its end is read, out is exact zeros behind it. */
int vb_aa_act(const float* x, const float* alpha, const float* inv_beta, const float* filt, int B, int C, int T, const int32_t* len, int len_mul,
              float* out, void* stream);
/* HiFi-GAN ResBlock1 pair in single-pass bf16, one launch (respair_bf16.hip):
 *   out = beta*out + alpha*(x + b2 + conv2_{k,1}( RN_bf16( lrelu(b1 + conv1_{k,dil}( RN_bf16(lrelu(x)) )) ) ))
 * both convolutions with RN-bf16 weights (w1_bf16 / w2_bf16: one plane [k][C co][C ci] each, pack.py:pack_conv_bf16), exact products, fp32
 * accumulation; the intermediate is rounded to bf16 once and zero outside [0, T).  x / out [B][C][T] (distinct buffers); C = 32 / 64, odd k,
 * (k-1)*dil <= 64.  Equals two vb_conv1d_bf16 launches up to the accumulation order. */
int vb_respair_bf16(const float* x, const void* w1_bf16, const float* b1, const void* w2_bf16, const float* b2, int B, int C, int T, int k,
                    int dil, float slope, float alpha, float beta, float* out, void* stream);
/* Unit entries of three kernels the net executor alone reached (vb_abi_version() stays 3; as vb_qkv_rope, they exist for the unit tests):
 * vb_conv1d_f32_ups: vb_conv1d_f32 over the nearest-x2 upsampled input (T_in = the un-upsampled length; stride 1, no transposed form, fp32
 *   weights only) - conv1d_f32g's upsampled window where it applies, the register-staged kernel otherwise.
 * vb_conv1d_x3_xt: the split-bf16 convolution over pre-activated planes - the two-plane pre-pass (vb_xt_planes, nplanes = 2, into
 *   planes_scratch of vb_xt_planes_bytes(B, Ci, T_in, upsample2, 2) bytes, 16-byte aligned), then the three-pass GEMM (Co >= 384,
 *   Ci % 64 == 0, alpha == 1, beta == 0, T_out == the input length) or conv1d_x3_kernel's DMA-fed input mode; w_x3 = [2][tap][Co][ci_pad].
 * vb_respair_x3: the split-bf16 ResBlock1 pair (respair_x3.hip), w1_x3 / w2_x3 = split planes [2][k][C][C]; otherwise as vb_respair_bf16. */
int vb_conv1d_f32_ups(const float* x, const float* w, const float* bias, int B, int Ci, int T_in, int Co, int ksize, int dil, int pad, int T_out,
                      int in_act, float in_slope, const float* res, float* out, void* stream);
int vb_conv1d_x3_xt(const float* x, const void* w_x3, int ci_pad, const float* bias, int B, int Ci, int T_in, int Co, int ksize, int dil, int pad,
                    int T_out, int upsample2, int in_act, float in_slope, const float* res, float alpha, float beta, float* out,
                    void* planes_scratch, void* stream);
int vb_respair_x3(const float* x, const void* w1_x3, const float* b1, const void* w2_x3, const float* b2, int B, int C, int T, int k, int dil,
                  float slope, float alpha, float beta, float* out, void* stream);
/* The plan of a convolution call, host only: which kernel vb_conv1d_f32 / _f32_mf / _bf16 / _bf16_xt would run on these arguments, on which
 * tile, with which epilogue - from the same descriptor fill, route and tile pickers the launch goes through, under the tuning knobs as they
 * stand (vb_tune_reload).  Nothing is launched and no device memory is touched; unit tests assert it so that a case that stops reaching
 * the kernel and tile it was written for fails.  Shape arguments as vb_conv1d_bf16 (in_act: 0 none, 1 LeakyReLU, 2 GroupNorm + swish,
 * 4 GroupNorm).  wforms = the weight forms the call carries (VB_PLAN_W_*; ci_pad with X3 / BF16), xt = the input comes as pre-activated
 * planes (vb_conv1d_bf16_xt), has_res = a residual is passed, misalign = operands that are only 4-byte aligned (VB_PLAN_*_4B; all others
 * 16-byte).  *route = VB_ROUTE_*, *tile_co x *tile_t = output channels x positions of a workgroup (VB_ROUTE_AS_GEMM: the conv-mode GEMM's
 * tile, 64 x 64 or 128 x 128), *stage_epi = the 16-byte staged epilogue.  Returns what the launch would return for arguments it refuses. */
enum { VB_PLAN_W_F32 = 1, VB_PLAN_W_MF = 2, VB_PLAN_W_X3 = 4, VB_PLAN_W_BF16 = 8 };
enum { VB_PLAN_X_4B = 1, VB_PLAN_OUT_4B = 2, VB_PLAN_RES_4B = 4, VB_PLAN_W_4B = 8 };
enum { VB_ROUTE_AS_GEMM = 0, VB_ROUTE_F32W = 1, VB_ROUTE_CO1 = 2, VB_ROUTE_BF16_XT = 3, VB_ROUTE_BF16 = 4, VB_ROUTE_X3_XT = 5, VB_ROUTE_X3 = 6,
       VB_ROUTE_F32G = 7, VB_ROUTE_F32 = 8 };
int vb_conv1d_plan(int B, int Ci, int T_in, int Co, int ksize, int dil, int pad, int tr_stride, int tr_pad, int tr_k, int T_out,
                   int upsample2, int in_stride, int in_phase, int in_act, int gn_groups, float alpha, float beta, int wforms, int ci_pad,
                   int xt, int has_res, int misalign, int* route, int* tile_co, int* tile_t, int* stage_epi);
/* The same for the fused pairs (form = VB_PAIR_*; misalign: VB_PLAN_X_4B / VB_PLAN_OUT_4B).  No pair launcher picks a tile by grid size: *run =
 * intermediate positions per workgroup, *outputs = the outputs it writes (run - (k - 1), rounded down to 4), *grid_t = workgroups along
 * time, *staged = the 16-byte epilogue.  VB_E_INVALID where the launch refuses the arguments. */
enum { VB_PAIR_F32 = 0, VB_PAIR_MF = 1, VB_PAIR_X3 = 2, VB_PAIR_BF16 = 3 };
int vb_respair_plan(int form, int B, int C, int T, int k, int dil, int misalign, int* run, int* outputs, int* grid_t, int* staged);
/* counter-based Gumbel draws: out[rows][w], rows = n_branch*B*T */
int vb_fill_gumbel(float* out, int B, int n_branch, int T, int width, uint64_t seed, int64_t clip_base, int nfe, int block, int gate,
                   void* stream);
int vb_cast_planes(const float* x, int64_t n, void* out, int np, void* stream);

#ifdef __cplusplus
}
#endif
#endif
