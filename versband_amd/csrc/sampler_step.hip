// The sampler's own kernels (gfx950), called by sampler.hip: the CFG + Euler update where it is a launch of its own (n_branch == 1,
// VB_EULER_LAUNCH, vb_euler_cfg_step; the sampler's default path fuses it into FinalLayer, rowlin.hip: final_layer_kernel<NQ, true>),
// the entry projection of a known region, the overlap consensus of joint windows (one starts array, or a per-row pair table), and the
// step bookkeeping behind the device-side step counter.
#include <algorithm>
#include <type_traits>

#include "kernels.h"

// ---------------------------------------------------------------------------
// CFG + Euler:  x[b] += dt * (v_u + s*(v_c - v_u))     (cfm1_audio.py:160 + fixed-step Euler)
// v holds the cond rows [0,B) then the uncond rows [B,2B); the arithmetic is common.h:euler_cfg_update, as in the fused launch.
// One kernel over one argument block (kernels.h: EulerDev; this launch reads the device's *step, not the host's k), its forms as flags:
// dt = dt_table[*step], or dt_val when there is no table (vb_euler_cfg_step).
// KEEP (vb_sample_cfg_keep): the blend with the known region at t = tn_table[*step]; mask, ref and x0 are read in these instances only.
// ROWS (vb_sample_cfg_rows): clip b = i / per takes scale_rows[b] instead of cfg_scale.
// SCHED (vb_sample_cfg_sched, per-row scales under a step weight that is neither 0 nor 1): s = fmaf(weight, scale_rows[b] - 1, 1).
// ---------------------------------------------------------------------------
template <bool KEEP, bool ROWS, bool SCHED>
__global__ void euler_cfg_kernel(const float* __restrict__ v, int64_t n, int64_t per, int T, int has_uncond, const EulerDev ed) {
    static_assert(ROWS || !SCHED, "the step weight belongs to the per-row scales (a scalar scale is combined on the host)");
    const int k = ed.step ? *ed.step : 0;
    const float dt = ed.dt_table ? ed.dt_table[k] : ed.dt_val;
    KeepAt ka{};
    if constexpr (KEEP) ka.tn = ed.kp.tn_table[k];
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t b = (KEEP || ROWS) ? i / per : 0;
    const float vc = v[i];
    float vu = 0.f, s = ed.cfg_scale;
    if (has_uncond) {
        vu = v[n + i];
        if constexpr (ROWS) s = ed.scale_rows[b];
        if constexpr (SCHED) s = fmaf(ed.weight, s - 1.f, 1.f);
    }
    if constexpr (KEEP) {
        ka.m = ed.kp.mask[b * T + (i - b * per) % T];
        ka.sigma_min = ed.kp.sigma_min; ka.ref = ed.kp.ref[i]; ka.x0 = ed.kp.x0[i];
    }
    ed.x[i] = euler_cfg_update<KEEP>(ed.x[i], vc, vu, has_uncond != 0, s, dt, ka);
}
int launch_euler_cfg(const EulerStep& es, const float* v, int B, int64_t per, int T, int has_uncond, float dt_val, hipStream_t st) {
    if (es.keep && (!es.dt_table || !es.step || T < 1)) VB_FAIL(VB_E_INVALID, "euler_cfg: a known region needs the step tables and T");
    const int64_t n = (int64_t)B * per;
    euler_dispatch(euler_form(es, has_uncond != 0), [&](auto keep, auto rows, auto sched) {
        hipLaunchKernelGGL((euler_cfg_kernel<decltype(keep)::value, decltype(rows)::value, decltype(sched)::value>), dim3((unsigned)((n + 255) / 256)),
                           dim3(256), 0, st, v, n, per, T, has_uncond, euler_dev(es, dt_val));
    });
    VB_CHECK_LAUNCH();
    return VB_OK;
}
// known region on entry: the state a call starts from is put on the path at t_0 = tn_table[0] - dt_table[0] (exact for a linspace
// grid: the difference of neighbouring grid points is); a no-op at t_0 = 0 with x = x0
__global__ void keep_project_kernel(float* x, int64_t n, int64_t per, int T, const float* dt_table, const EulerKeep kp) {
    const float t0 = kp.tn_table[0] - dt_table[0];
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t b = i / per;
    const float m = kp.mask[b * T + (i - b * per) % T];
    x[i] = keep_blend(m, keep_path(t0, kp.sigma_min, kp.ref[i], kp.x0[i]), x[i]);
}
int launch_keep_project(float* x, int B, int64_t per, int T, const float* dt_table, const EulerKeep& keep, hipStream_t st) {
    int64_t n = (int64_t)B * per;
    hipLaunchKernelGGL(keep_project_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, x, n, per, T, dt_table, keep);
    VB_CHECK_LAUNCH();
    return VB_OK;
}
// ---------------------------------------------------------------------------
// Joint windows (vb_sample_cfg_windows, vb_window_blend): x [nw*Bc][C][n], row = w*Bc + b, holds the windows of Bc long clips.  The
// last ov = starts[w] + n - starts[w+1] tokens of window w and the first ov of window w + 1 are the same tokens of the clip; after
// every step both copies take one consensus value, the cross-fade of the two at that token (the later window's ramp weight, the one
// crossfade_windows_kernel uses):
//     g = (float)(u + 1) / (float)(ov + 1);   m = fmaf(g, x[ib] - x[ia], x[ia]);   x[ia] = x[ib] = m
// Equal copies come back unchanged bit for bit (fmaf(g, 0, a) = a).  One thread owns one (ia, ib) pair and no token lies under three
// windows (window_plan refuses such a plan), so the pairs are disjoint: no race, no dependence on the launch shape.
// grid: y = the pair of windows (w, w + 1), x over Bc * C * ov of that pair (the widest overlap sizes it)
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) window_blend_kernel(float* x, const WindowPlan wp, int Bc, int C, int n) {
    const int w = blockIdx.y;
    const int ov = wp.s[w] + n - wp.s[w + 1];
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (ov <= 0 || i >= (int64_t)Bc * C * ov) return;
    const int u = (int)(i % ov);
    const int64_t bc = i / ov;                                   // b * C + c: rows of one window are contiguous
    const int64_t ia = ((int64_t)w * Bc * C + bc) * n + (n - ov + u);
    const int64_t ib = ((int64_t)(w + 1) * Bc * C + bc) * n + u;
    const float g = (float)(u + 1) / (float)(ov + 1);
    const float a = x[ia];
    const float m = fmaf(g, x[ib] - a, a);
    x[ia] = m;
    x[ib] = m;
}
int window_plan(const int32_t* starts, int nw, int B, int n, WindowPlan* out) {
    if (nw < 1 || nw > 64) VB_FAIL(VB_E_INVALID, "windows: %d windows (1..64)", nw);
    if (!starts) VB_FAIL(VB_E_INVALID, "windows: starts is null");
    if (B < 1 || n < 1 || B % nw != 0) VB_FAIL(VB_E_INVALID, "windows: %d rows of %d tokens are not %d windows of whole clips", B, n, nw);
    if (starts[0] < 0) VB_FAIL(VB_E_INVALID, "windows: window 0 starts at %d", starts[0]);
    for (int w = 0; w + 1 < nw; ++w) {
        if (starts[w + 1] <= starts[w] || starts[w + 1] > starts[w] + n)
            VB_FAIL(VB_E_INVALID, "windows: window %d at %d does not continue window %d at %d (length %d): descending or a gap", w + 1,
                    starts[w + 1], w, starts[w], n);
        if (w + 2 < nw && starts[w + 2] < starts[w] + n)
            VB_FAIL(VB_E_INVALID, "windows: window %d at %d reaches into window %d at %d (length %d): a token under three windows", w + 2,
                    starts[w + 2], w, starts[w], n);
    }
    WindowPlan p;
    p.nw = nw;
    for (int w = 0; w < nw; ++w) p.s[w] = starts[w];
    *out = p;
    return VB_OK;
}
// row lengths of a call (vb_lens; HOST array): checked before anything is launched.  Lengths that all equal T are the plain call (B = 0).
int lens_plan(const int32_t* len, int B, int T, LensPlan* out) {
    if (!len) VB_FAIL(VB_E_INVALID, "lens: len is null");
    if (B < 1 || B > 64) VB_FAIL(VB_E_INVALID, "lens: %d rows (1..64); row %d has no slot in the table", B, B < 1 ? 0 : 64);
    LensPlan p;
    bool full = true;
    for (int b = 0; b < B; ++b) {
        if (len[b] < 1 || len[b] > T) VB_FAIL(VB_E_INVALID, "lens: row %d has length %d (1..T = %d)", b, len[b], T);
        p.len[b] = len[b];
        full = full && len[b] == T;
    }
    p.B = full ? 0 : B;
    *out = p;
    return VB_OK;
}
int launch_window_blend(float* x, const WindowPlan& wp, int Bc, int C, int n, hipStream_t st) {
    int ov_max = 0;
    for (int w = 0; w + 1 < wp.nw; ++w) ov_max = std::max(ov_max, wp.s[w] + n - wp.s[w + 1]);
    if (ov_max <= 0) return VB_OK;                               // one window, or windows that only touch
    const int64_t tot = (int64_t)Bc * C * ov_max;
    hipLaunchKernelGGL(window_blend_kernel, dim3((unsigned)((tot + 255) / 256), (unsigned)(wp.nw - 1)), dim3(256), 0, st, x, wp, Bc, C, n);
    VB_CHECK_LAUNCH();
    return VB_OK;
}
// ---------------------------------------------------------------------------
// Window rows (vb_sample_cfg_window_rows, vb_window_rows_blend): x [B][C][T], row r a window of clip group[r] with its own length.  The
// consensus of window_blend_kernel over a pair TABLE instead of one starts array: pair j says that token off_a + u of row ra and token
// u of row rb are the same token, u in [0, ov).  Same arithmetic, one thread per (ia, ib), pairs disjoint by window_rows_plan (no token
// under three rows, ov <= len[rb]); off_a + ov = len[ra] <= T and ov <= len[rb] <= T, so only valid tokens are read or written.
// grid: y = the pair, x over C * ov of that pair (the widest overlap sizes it)
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) window_rows_blend_kernel(float* x, const WindowPairs wp, int C, int T) {
    const WindowPairs::Pair p = wp.p[blockIdx.y];
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)C * p.ov) return;
    const int u = (int)(i % p.ov);
    const int64_t c = i / p.ov;
    const int64_t ia = ((int64_t)p.ra * C + c) * T + (p.off_a + u);
    const int64_t ib = ((int64_t)p.rb * C + c) * T + u;
    const float g = (float)(u + 1) / (float)(p.ov + 1);
    const float a = x[ia];
    const float m = fmaf(g, x[ib] - a, a);
    x[ia] = m;
    x[ib] = m;
}
int window_rows_plan(const int32_t* group, const int32_t* start, const LensPlan& lp, int B, int T, WindowRowsPlan* out) {
    if (!group || !start) VB_FAIL(VB_E_INVALID, "window_rows: %s is null (row 0 has no plan)", !group ? "group" : "start");
    if (B < 1 || B > 64) VB_FAIL(VB_E_INVALID, "window_rows: %d rows (1..64); row %d has no slot in the table", B, B < 1 ? 0 : 64);
    if (T < 1) VB_FAIL(VB_E_INVALID, "window_rows: rows of %d tokens", T);
    WindowRowsPlan p;
    p.B = B;
    int len[64];
    for (int r = 0; r < B; ++r) { len[r] = lp.B ? lp.len[r] : T; p.group[r] = group[r]; p.start[r] = start[r]; }
    for (int r = 0; r < B; ++r) {
        if (start[r] < 0) VB_FAIL(VB_E_INVALID, "window_rows: row %d starts at %d", r, start[r]);
        int ra = -1, rz = -1;                                      // the rows of r's group before it: the last, and the one before that
        for (int q = r - 1; q >= 0 && rz < 0; --q)
            if (group[q] == group[r]) { if (ra < 0) ra = q; else rz = q; }
        if (ra < 0) continue;
        const int64_t end_a = (int64_t)start[ra] + len[ra];
        if (start[r] <= start[ra])
            VB_FAIL(VB_E_INVALID, "window_rows: row %d at %d does not come after row %d at %d of group %d (rows of a group ascend)", r, start[r],
                    ra, start[ra], group[r]);
        if (start[r] > end_a)
            VB_FAIL(VB_E_INVALID, "window_rows: a gap between row %d at %d (length %d) and row %d at %d of group %d", ra, start[ra], len[ra], r,
                    start[r], group[r]);
        const int ov = (int)(end_a - start[r]);
        if (ov > len[r])
            VB_FAIL(VB_E_INVALID, "window_rows: row %d of length %d lies inside its overlap of %d tokens with row %d (group %d)", r, len[r], ov, ra,
                    group[r]);
        if (rz >= 0 && start[r] < (int64_t)start[rz] + len[rz])
            VB_FAIL(VB_E_INVALID, "window_rows: row %d at %d reaches into row %d at %d (length %d) of group %d: a token under three rows", r,
                    start[r], rz, start[rz], len[rz], group[r]);
        if (ov > 0) {                                              // (rows that only touch have nothing to reconcile)
            p.pairs.p[p.pairs.np++] = WindowPairs::Pair{ra, r, len[ra] - ov, ov};
            p.ov_max = std::max(p.ov_max, ov);
        }
    }
    *out = p;
    return VB_OK;
}
int launch_window_rows_blend(float* x, const WindowRowsPlan& wr, int C, int T, hipStream_t st) {
    if (wr.pairs.np <= 0) return VB_OK;
    const int64_t tot = (int64_t)C * wr.ov_max;
    hipLaunchKernelGGL(window_rows_blend_kernel, dim3((unsigned)((tot + 255) / 256), (unsigned)wr.pairs.np), dim3(256), 0, st, x, wr.pairs, C, T);
    VB_CHECK_LAUNCH();
    return VB_OK;
}
// step bookkeeping for graph replay: (reset) step=0 or step+=1; t_idx_cur[:] = t_table[step]
__global__ void step_advance_kernel(int* step, int64_t* t_idx_cur, const int64_t* t_table, int n_steps, int Beff, int reset) {
    __shared__ int s;
    if (threadIdx.x == 0) {
        s = reset ? 0 : (*step + 1);
        *step = s;
    }
    __syncthreads();
    int k = s < n_steps ? s : n_steps - 1;
    for (int i = threadIdx.x; i < Beff; i += blockDim.x) t_idx_cur[i] = t_table[k];
}
// noise key of a sampler call -> the parameter block behind the step counter: step[4..9] = {seed, clip_base, nfe_base} as 3 x int64
__global__ void sampler_params_kernel(int* step, unsigned long long seed, long long clip_base, int nfe_base) {
    long long* prm = reinterpret_cast<long long*>(step + 4);
    prm[0] = (long long)seed; prm[1] = clip_base; prm[2] = nfe_base;
}
int launch_sampler_params(int* step, uint64_t seed, int64_t clip_base, int nfe_base, hipStream_t st) {
    hipLaunchKernelGGL(sampler_params_kernel, dim3(1), dim3(1), 0, st, step, (unsigned long long)seed, (long long)clip_base, nfe_base);
    VB_CHECK_LAUNCH();
    return VB_OK;
}
int launch_step_ctl(int* step, int64_t* t_idx_cur, const int64_t* t_table, int n_steps, int Beff, int reset, hipStream_t st) {
    hipLaunchKernelGGL(step_advance_kernel, dim3(1), dim3(64), 0, st, step, t_idx_cur, t_table, n_steps, Beff, reset);
    VB_CHECK_LAUNCH();
    return VB_OK;
}
