// CFG / Euler sampler (cfm1_audio_sampler.py:107-116): the step loop around dit_forward and its hipGraph cache.
#include "engine.h"

// the launches of one sampler call after its tables are in place: tabulation of the per-step conditioning vectors, then n_steps x
// [step bookkeeping, one network evaluation of both CFG branches, Euler + guidance update]   (cfm1_audio_sampler.py:107-116)
// engine.h:SampleCall says what each member of the call adds to a step.  With step weights (sc.gw) step k is one of three kinds by gw[k] -
//   1: the plain step, launch for launch;
//   0: a single-branch step - the network runs over the conditional rows alone (DitEval::nb_active = 1), FinalLayer writes their velocity
//      and the update is the separate launch without an unconditional half, as in an nb == 1 call;
//   else: both branches under the step's effective scale fmaf(gw[k], s - 1, 1): a scalar s is combined here and handed to the existing
//      instances, per-row scales take the SCHED instances of the update (kernels.h: euler_form) with gw[k] in their arguments.
// The kinds are baked into a captured graph (its key holds the weights).  Keep blend, window consensus and trajectory copy do not
// depend on the kind.
static EulerKeep euler_keep(const vb_keep& k, const WsL& s) { return EulerKeep{k.ref, k.x0, k.mask, s.tn_table, k.sigma_min}; }
static int sample_steps(vb_ctx* ctx, const SampleCall& sc, float* traj, hipStream_t st) {
    const vb_dit_config& c = ctx->cfg;
    const int B = sc.B, n_branch = sc.nb, T = sc.T, L = sc.L, n_steps = sc.n_steps;
    const DitPlan plan = dit_plan(ctx, B, n_branch, T, L);
    WsL s = carve_ws(sc.ws, c, B, n_branch, T, L);
    const int Beff = B * n_branch;
    const int64_t per = (int64_t)c.in_channels * T;
    // row lengths: the values travel in the launch's argument block (a captured graph holds them; its key does too)
    if (sc.lens.B) VB_TRY(launch_lens_table(sc.lens, s.len_table, st));
    // (a kernel, not hipMemsetAsync: the captured step loop then consists of kernel nodes only)
    VB_TRY(launch_fill_f32(reinterpret_cast<float*>(s.vt), (int64_t)s.n_vt * c.np / 2, 0.f, st));
    // The timestep embedding, every block's adaLN modulation and the high-level gate logits depend on (t_k, caption)
    // only: tabulate them for ALL steps in four launches instead of four GEMVs inside every network evaluation.
    const bool tab = n_steps <= PRE_STEPS;
    const int D = c.hidden, MODW = s.MODW;
    if (tab) {
        const vb_dit_weights& w = ctx->w;
        CondL cd = carve_cond(const_cast<void*>(sc.cond), c, B, n_branch, T, L);
        VB_TRY(launch_gemv_rows_idx(w.t_freq_table, 256, s.t_table, nullptr, 0, 1, w.t_mlp0_w, w.t_mlp0_b, n_steps, D, 256, 0, s.temb0_s, D, st, T_FREQ_ROWS));
        VB_TRY(launch_gemv_rows(s.temb0_s, D, nullptr, 0, 1, w.t_mlp2_w, w.t_mlp2_b, n_steps, D, D, 1, s.temb_s, D, st));
        VB_TRY(launch_iota_div(s.row_step, n_steps * Beff, Beff, st));
        if (w.adaln_wp) {
            // [steps x samples][768] x [19968][768]^T in split-bf16 (fp32-class) on the MFMA GEMM: 0.2 ms instead of 2.2 ms per call
            const int rows = n_steps * Beff;
            const int64_t apl = (int64_t)rows * D;
            VB_TRY(launch_silu_sum_planes(s.temb_s, cd.cemb, rows, D, Beff, s.modA, apl, st));
            GemmArgs g = gemm_operands(s.modA, apl, D, w.adaln_wp, (int64_t)MODW * D, D, rows, MODW, D, 3);
            g.epi = EPI_F32; g.bias = w.adaln_b; g.out32 = s.mod_s; g.ldc32 = MODW;
            VB_TRY(launch_gemm(g, st));
        } else {
            VB_TRY(launch_gemv_rows_idx(s.temb_s, D, s.row_step, cd.cemb, D, Beff, w.adaln_w, w.adaln_b, n_steps * Beff, MODW, D, 1, s.mod_s, MODW, st));
        }
        VB_TRY(launch_gemv_rows(s.temb_s, D, nullptr, 0, 1, w.hl_w, w.hl_b, n_steps, c.depth * 2, D, 0, s.hl_s, c.depth * 2, st));
    }
    // the router's count tables, cleared once per call inside the captured graph (DitPlan::router_counts)
    if (plan.router_counts) {
        const int N = (int)s.n_tok;
        VB_TRY(launch_fill_f32(reinterpret_cast<float*>(bucket_counts(s.perm, N, 0)), bucket_counts_ints(N), 0.f, st));
    }
    // FinalLayer, CFG combination, Euler update and the step counter's advance as ONE launch per step (round 5; VB_EULER_LAUNCH=1 keeps the three
    // launches: same arithmetic, bit-identical)
    // (the device step counter s.step ends a call at n_steps with the fused Euler launch and at n_steps - 1 with the separate launches; nothing
    //  reads it after the call, launch_step_ctl resets it at k == 0)
    const bool fuse = plan.final_route == FINAL_EULER_FUSED;
    const EulerKeep kp = sc.keep ? euler_keep(*sc.keep, s) : EulerKeep{};
    EulerStep es;
    es.x = sc.x; es.cfg_scale = sc.cfg_scale; es.dt_table = s.dt_table; es.keep = sc.keep ? &kp : nullptr;
    es.scale_rows = n_branch == 2 ? sc.rows.cfg_scale : nullptr;      // (one branch: there is nothing to guide, the scales are unused)
    es.step = s.step; es.t_idx_cur = s.t_idx_cur; es.t_table = s.t_table; es.n_steps = n_steps; es.Beff = Beff;
    bool advanced = false;        // the previous step's update launch advanced the device step counter (the fused form does)
    bool single_prev = false;
    for (int k = 0; k < n_steps; ++k) {
        RoctxRange rs("euler_step");
        const float wk = sc.gw ? sc.gw[k] : 1.f;
        const bool single = sc.gw && wk == 0.f;
        const bool fuse_k = fuse && !single;
        // the router's count tables are in step only while every evaluation counts the same rows (DitPlan::router_counts): a change between
        // one and two branches starts them afresh
        if (k > 0 && single != single_prev && plan.router_counts)
            VB_TRY(launch_fill_f32(reinterpret_cast<float*>(bucket_counts(s.perm, (int)s.n_tok, 0)), bucket_counts_ints((int)s.n_tok), 0.f, st));
        single_prev = single;
        if (k == 0 || !advanced) VB_TRY(launch_step_ctl(s.step, s.t_idx_cur, s.t_table, n_steps, Beff, k == 0, st));
        EulerStep ek = es;
        ek.k = k;
        if (single) ek.scale_rows = nullptr;                          // (one branch: nothing to guide, as in an n_branch == 1 call)
        else if (sc.gw && wk != 1.f) {
            if (ek.scale_rows) ek.row_weight = wk; else ek.cfg_scale = fmaf(wk, sc.cfg_scale - 1.f, 1.f);
        }
        DitEval ev;
        ev.x = sc.x; ev.t_idx = s.t_idx_cur; ev.cond = sc.cond; ev.ws = sc.ws; ev.B = B; ev.nb = n_branch; ev.T = T; ev.L = L;
        if (single) ev.nb_active = 1;
        ev.noise = sc.noise; ev.noise_step = k; ev.step_ptr = s.step; ev.v_out = s.v; ev.clip_rows = sc.rows.clip;
        if (sc.lens.B) ev.lens = s.len_table;
        if (tab) { ev.pre_mod = s.mod_s + (size_t)k * Beff * MODW; ev.pre_hl = s.hl_s + (size_t)k * c.depth * 2; }
        ev.evals_before = k * c.depth;
        if (fuse_k) ev.euler = &ek;
        VB_TRY(dit_forward(ctx, ev, st));
        if (!fuse_k) VB_TRY(launch_euler_cfg(ek, s.v, B, per, T, n_branch == 2 && !single, 0.f, st));
        advanced = fuse_k;
        if (sc.windows) VB_TRY(launch_window_blend(sc.x, sc.wp, B / sc.wp.nw, c.in_channels, T, st));
        if (sc.wrows) VB_TRY(launch_window_rows_blend(sc.x, sc.wr, c.in_channels, T, st));
        if (traj) VB_HIP(hipMemcpyAsync(traj + (size_t)(k + 1) * B * per, sc.x, (size_t)B * per * sizeof(float), hipMemcpyDeviceToDevice, st));
    }
    return VB_OK;
}

// the cache entry of this call's key: found, or inserted over the least recently used of 8
static SampleGraph* graph_entry(vb_ctx* ctx, const SampleGraph::Key& key) {
    SampleGraph* e = nullptr;
    for (SampleGraph& gph : ctx->graphs)
        if (gph.key == key) { e = &gph; break; }
    if (!e) {
        if (ctx->graphs.size() >= 8) {
            size_t lru = 0;
            for (size_t i = 1; i < ctx->graphs.size(); ++i) if (ctx->graphs[i].last_use < ctx->graphs[lru].last_use) lru = i;
            ctx->graphs[lru].destroy();
            ctx->graphs.erase(ctx->graphs.begin() + lru);
        }
        ctx->graphs.emplace_back();
        e = &ctx->graphs.back();
        e->key = key;
    }
    e->last_use = ++ctx->graph_clock;
    e->seen += 1;
    return e;
}

// ---- vb_sample_cfg_window_rows as its steps: sample_call, sample_prologue, sample_graph | sample_steps -------------------------------
// check the ABI arguments before anything is launched and state the call once.  Every normalisation happens here: per-row scales zero
// the scalar one, a schedule of all ones or beside one branch (nothing to guide) is the plain call, and so are one window and row
// lengths that all equal T (lens_plan), and window rows none of whose groups has two overlapping rows (window_rows_plan).
static int sample_call(vb_ctx* ctx, float* x, const void* cond, int B, int n_branch, int T, int L, int n_steps, float cfg_scale,
                       const vb_window_rows* wrows, const vb_lens* lens, const vb_guidance* guidance, const vb_windows* win, const vb_rows* rows, const vb_keep* keep, const vb_noise* noise,
                       void* ws, SampleCall& sc) {
    sc.x = x; sc.cond = cond; sc.ws = ws; sc.B = B; sc.nb = n_branch; sc.T = T; sc.L = L; sc.n_steps = n_steps; sc.keep = keep; sc.noise = noise;
    if (rows) sc.rows = *rows;
    sc.cfg_scale = sc.rows.cfg_scale ? 0.f : cfg_scale;          // unused beside the array; one value in the graph key
    if (!ctx || !ctx->dit_loaded) VB_FAIL(VB_E_STATE, "sample_cfg: DiT not loaded");
    if (n_steps < 1 || n_steps > 1024) VB_FAIL(VB_E_INVALID, "sample_cfg: n_steps=%d", n_steps);
    if (keep && (!keep->ref || !keep->x0 || !keep->mask || !keep->t_next)) VB_FAIL(VB_E_INVALID, "sample_cfg_keep: ref, x0, mask and t_next must all be given");
    if (guidance && guidance->weight && n_branch == 2) {          // (host array)
        for (int k = 0; k < n_steps; ++k) {
            const float w = guidance->weight[k];
            if (!(w >= 0.f && w <= 16.f)) VB_FAIL(VB_E_INVALID, "sample_cfg_sched: weight[%d] = %g is not a finite value in [0, 16]", k, (double)w);
            if (w != 1.f) sc.gw = guidance->weight;
        }
    }
    if (win) VB_TRY(window_plan(win->starts, win->nw, B, T, &sc.wp));
    sc.windows = win && sc.wp.nw > 1;
    if (lens && lens->len) {
        VB_TRY(lens_plan(lens->len, B, T, &sc.lens));
        if (sc.lens.B && sc.windows)
            VB_FAIL(VB_E_INVALID, "sample_cfg_lens: row %d has length %d of %d beside %d joint windows, which are equal-length by construction",
                    sc.lens.first_short(T), sc.lens.len[sc.lens.first_short(T)], T, sc.wp.nw);
    }
    if (wrows) {
        if (sc.windows)
            VB_FAIL(VB_E_INVALID, "sample_cfg_window_rows: %d joint windows beside window rows (row 0 would stand under two plans)", sc.wp.nw);
        VB_TRY(window_rows_plan(wrows->group, wrows->start, sc.lens, B, T, &sc.wr));
        sc.wrows = sc.wr.pairs.np > 0;
    }
    return VB_OK;
}

// what runs in front of the step loop, outside a captured graph: the step tables' way into the workspace, the state the first
// evaluation sees (and traj[0] holds), the noise key
static int sample_prologue(vb_ctx* ctx, const SampleCall& sc, const int64_t* t_idx_table, const float* dt_table, float* traj, hipStream_t st) {
    const vb_dit_config& c = ctx->cfg;
    WsL s = carve_ws(sc.ws, c, sc.B, sc.nb, sc.T, sc.L);
    const int64_t per = (int64_t)c.in_channels * sc.T;
    // (tables may live on the host or on the device; a host caller must keep them alive until the stream has consumed them)
    VB_HIP(hipMemcpyAsync(s.t_table, t_idx_table, (size_t)sc.n_steps * sizeof(int64_t), hipMemcpyDefault, st));
    VB_HIP(hipMemcpyAsync(s.dt_table, dt_table, (size_t)sc.n_steps * sizeof(float), hipMemcpyDefault, st));
    if (sc.keep) {
        // the times travel like the step sizes do (a device table read behind the step counter); the entry projection runs here, outside
        // the captured loop, so that traj[0] is the state the first evaluation sees
        VB_HIP(hipMemcpyAsync(s.tn_table, sc.keep->t_next, (size_t)sc.n_steps * sizeof(float), hipMemcpyDefault, st));
        VB_TRY(launch_keep_project(sc.x, sc.B, per, sc.T, s.dt_table, euler_keep(*sc.keep, s), st));
    }
    // rows that disagree in their overlaps start from the consensus; rows cut from one start noise are not changed by it
    if (sc.windows) VB_TRY(launch_window_blend(sc.x, sc.wp, sc.B / sc.wp.nw, c.in_channels, sc.T, st));
    if (sc.wrows) VB_TRY(launch_window_rows_blend(sc.x, sc.wr, c.in_channels, sc.T, st));
    if (traj) VB_HIP(hipMemcpyAsync(traj, sc.x, (size_t)sc.B * per * sizeof(float), hipMemcpyDeviceToDevice, st));
    // the noise key travels through device memory (the router reads it behind the step counter): nothing a replayed graph bakes in
    const vb_noise* noise = sc.noise;
    return launch_sampler_params(s.step, noise ? noise->seed : 0, noise ? noise->clip_base : 0, noise ? noise->nfe : 0, st);
}

// ---- the step loop as ONE hipGraph (cfm1_audio_sampler.py:107-116 is ~3000 dependent launches at 50 steps): a call whose
// buffers and shape were seen before replays the captured, instantiated graph - one host call instead of thousands, which is
// what bounds small batches and several concurrent streams (the HIP runtime serialises launches of different host threads).
// Returns the call's graph, captured now if its key arrives for the second time; nullptr (run eagerly) when the key is new (its first
// call also warms every kernel's one-time attributes outside a capture) or capture was refused once.
static hipGraphExec_t sample_graph(vb_ctx* ctx, const SampleCall& sc, hipStream_t st) {
    SampleGraph* e = graph_entry(ctx, sample_key(sc));
    if (!e->exec && !e->failed && e->seen >= 2) {
        if (hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal) == hipSuccess) {
            const int rc = sample_steps(ctx, sc, nullptr, st);
            hipGraph_t gr = nullptr;
            const hipError_t ee = hipStreamEndCapture(st, &gr);
            if (rc == VB_OK && ee == hipSuccess && gr && hipGraphInstantiate(&e->exec, gr, nullptr, nullptr, 0) == hipSuccess) {
                e->graph = gr;
            } else {
                if (gr) (void)hipGraphDestroy(gr);
                e->exec = nullptr; e->failed = true;
                (void)hipGetLastError();
            }
        } else {
            e->failed = true;
            (void)hipGetLastError();
        }
    }
    return e->exec;
}

extern "C" {

int vb_euler_cfg_step(float* x, const float* v, int B, int64_t per_item, float cfg_scale, float dt, int has_uncond, void* stream) {
    EulerStep es;
    es.x = x; es.cfg_scale = cfg_scale;
    return launch_euler_cfg(es, v, B, per_item, 1, has_uncond, dt, (hipStream_t)stream);
}
int vb_sample_cfg(vb_ctx* ctx, float* x, const void* cond, int B, int n_branch, int T, int L, int n_steps,
                  const int64_t* t_idx_table, const float* dt_table, float cfg_scale, const vb_noise* noise, float* traj, void* ws,
                  void* stream) {
    return vb_sample_cfg_sched(ctx, x, cond, B, n_branch, T, L, n_steps, t_idx_table, dt_table, cfg_scale, nullptr, nullptr, nullptr, nullptr, noise, traj, ws, stream);
}
int vb_sample_cfg_keep(vb_ctx* ctx, float* x, const void* cond, int B, int n_branch, int T, int L, int n_steps,
                       const int64_t* t_idx_table, const float* dt_table, float cfg_scale, const vb_keep* keep, const vb_noise* noise,
                       float* traj, void* ws, void* stream) {
    return vb_sample_cfg_sched(ctx, x, cond, B, n_branch, T, L, n_steps, t_idx_table, dt_table, cfg_scale, nullptr, nullptr, nullptr, keep, noise, traj, ws, stream);
}
int vb_sample_cfg_rows(vb_ctx* ctx, float* x, const void* cond, int B, int n_branch, int T, int L, int n_steps,
                       const int64_t* t_idx_table, const float* dt_table, float cfg_scale, const vb_rows* rows, const vb_keep* keep,
                       const vb_noise* noise, float* traj, void* ws, void* stream) {
    return vb_sample_cfg_sched(ctx, x, cond, B, n_branch, T, L, n_steps, t_idx_table, dt_table, cfg_scale, nullptr, nullptr, rows, keep, noise, traj, ws, stream);
}
int vb_window_blend(float* x, const int32_t* starts, int nw, int B, int C, int n, void* stream) {
    if (!x || C < 1) VB_FAIL(VB_E_INVALID, "window_blend: null x or C < 1");
    WindowPlan wp;
    VB_TRY(window_plan(starts, nw, B, n, &wp));
    return launch_window_blend(x, wp, B / nw, C, n, (hipStream_t)stream);
}
int vb_sample_cfg_windows(vb_ctx* ctx, float* x, const void* cond, int B, int n_branch, int T, int L, int n_steps,
                          const int64_t* t_idx_table, const float* dt_table, float cfg_scale, const vb_windows* win, const vb_rows* rows,
                          const vb_keep* keep, const vb_noise* noise, float* traj, void* ws, void* stream) {
    return vb_sample_cfg_sched(ctx, x, cond, B, n_branch, T, L, n_steps, t_idx_table, dt_table, cfg_scale, nullptr, win, rows, keep, noise, traj, ws, stream);
}
int vb_sample_cfg_sched(vb_ctx* ctx, float* x, const void* cond, int B, int n_branch, int T, int L, int n_steps,
                        const int64_t* t_idx_table, const float* dt_table, float cfg_scale, const vb_guidance* guidance,
                        const vb_windows* win, const vb_rows* rows, const vb_keep* keep, const vb_noise* noise, float* traj, void* ws,
                        void* stream) {
    return vb_sample_cfg_lens(ctx, x, cond, B, n_branch, T, L, n_steps, t_idx_table, dt_table, cfg_scale, nullptr, guidance, win, rows, keep, noise, traj, ws, stream);
}
int vb_sample_cfg_lens(vb_ctx* ctx, float* x, const void* cond, int B, int n_branch, int T, int L, int n_steps,
                       const int64_t* t_idx_table, const float* dt_table, float cfg_scale, const vb_lens* lens, const vb_guidance* guidance,
                       const vb_windows* win, const vb_rows* rows, const vb_keep* keep, const vb_noise* noise, float* traj, void* ws,
                       void* stream) {
    return vb_sample_cfg_window_rows(ctx, x, cond, B, n_branch, T, L, n_steps, t_idx_table, dt_table, cfg_scale, nullptr, lens, guidance, win, rows, keep, noise, traj, ws, stream);
}
int vb_window_rows_blend(float* x, const int32_t* group, const int32_t* start, const int32_t* len, int B, int C, int T, void* stream) {
    if (!x || C < 1) VB_FAIL(VB_E_INVALID, "window_rows_blend: null x or C < 1");
    LensPlan lp;
    if (len) VB_TRY(lens_plan(len, B, T, &lp));
    WindowRowsPlan wr;
    VB_TRY(window_rows_plan(group, start, lp, B, T, &wr));
    return launch_window_rows_blend(x, wr, C, T, (hipStream_t)stream);
}
int vb_sample_cfg_window_rows(vb_ctx* ctx, float* x, const void* cond, int B, int n_branch, int T, int L, int n_steps,
                              const int64_t* t_idx_table, const float* dt_table, float cfg_scale, const vb_window_rows* wrows,
                              const vb_lens* lens, const vb_guidance* guidance, const vb_windows* win, const vb_rows* rows,
                              const vb_keep* keep, const vb_noise* noise, float* traj, void* ws, void* stream) {
    SampleCall sc;
    VB_TRY(sample_call(ctx, x, cond, B, n_branch, T, L, n_steps, cfg_scale, wrows, lens, guidance, win, rows, keep, noise, ws, sc));
    VB_HIP(hipSetDevice(ctx->device));
    RoctxRange rr("vb_sample_cfg");
    hipStream_t st = (hipStream_t)stream;
    VB_TRY(sample_prologue(ctx, sc, t_idx_table, dt_table, traj, st));
    // Eager when: a trajectory or injected noise arrays are requested (parity path), the per-launch HIP-event profiler is on, the
    // stream cannot capture (legacy default stream), VB_NO_GRAPH is set, or sample_graph has no graph for the call.
    const bool graphable = !vb_tune().no_graph && !prof_enabled() && !traj && !(noise && noise->g1) && n_steps <= PRE_STEPS && st != nullptr;
    if (hipGraphExec_t exec = graphable ? sample_graph(ctx, sc, st) : nullptr) {
        VB_HIP(hipGraphLaunch(exec, st));
        return VB_OK;
    }
    return sample_steps(ctx, sc, traj, st);
}
int vb_sample_graphs(vb_ctx* ctx) {
    int n = 0;
    if (ctx) for (const SampleGraph& g : ctx->graphs) n += g.exec != nullptr;
    return n;
}

}  // extern "C"
