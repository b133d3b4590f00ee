// The sampler's own kernels (gfx950), called by sampler.hip: the CFG + Euler update where it is a launch of its own (n_branch == 1,
// VB_EULER_LAUNCH, vb_euler_cfg_step; the sampler's default path fuses it into FinalLayer, rowlin.hip: final_layer_kernel<NQ, true>),
// the entry projection of a known region, and the step bookkeeping behind the device-side step counter.
#include <type_traits>

#include "kernels.h"

// ---------------------------------------------------------------------------
// CFG + Euler:  x[b] += dt * (v_u + s*(v_c - v_u))     (cfm1_audio.py:160 + fixed-step Euler)
// v holds the cond rows [0,B) then the uncond rows [B,2B); the arithmetic is common.h:euler_cfg_update, as in the fused launch.
// dt = dt_table[*step], or dt_val when there is no table (vb_euler_cfg_step).
// KEEP (vb_sample_cfg_keep): the blend with the known region at t = tn_table[*step]; mask, ref and x0 are read in these instances only.
// ROWS (vb_sample_cfg_rows): clip b = i / per takes scale_rows[b] instead of cfg_scale.
// ---------------------------------------------------------------------------
template <bool KEEP, bool ROWS>
__global__ void euler_cfg_kernel(float* x, const float* __restrict__ v, int64_t n, int64_t per, int T, float cfg_scale,
                                 const float* __restrict__ scale_rows, const float* dt_table, const int* step, float dt_val,
                                 int has_uncond, const EulerKeep kp) {
    const int k = step ? *step : 0;
    const float dt = dt_table ? dt_table[k] : dt_val;
    KeepAt ka{};
    if constexpr (KEEP) ka.tn = kp.tn_table[k];
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t b = (KEEP || ROWS) ? i / per : 0;
    const float vc = v[i];
    float vu = 0.f, s = cfg_scale;
    if (has_uncond) {
        vu = v[n + i];
        if constexpr (ROWS) s = scale_rows[b];
    }
    if constexpr (KEEP) {
        ka.m = kp.mask[b * T + (i - b * per) % T];
        ka.sigma_min = kp.sigma_min; ka.ref = kp.ref[i]; ka.x0 = kp.x0[i];
    }
    x[i] = euler_cfg_update<KEEP>(x[i], vc, vu, has_uncond != 0, s, dt, ka);
}
int launch_euler_cfg(const EulerStep& es, const float* v, int B, int64_t per, int T, int has_uncond, float dt_val, hipStream_t st) {
    if (es.keep && (!es.dt_table || !es.step || T < 1)) VB_FAIL(VB_E_INVALID, "euler_cfg: a known region needs the step tables and T");
    const int64_t n = (int64_t)B * per;
    auto go = [&](auto keep, auto rows) {
        hipLaunchKernelGGL((euler_cfg_kernel<decltype(keep)::value, decltype(rows)::value>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st,
                           es.x, v, n, per, T, es.cfg_scale, es.scale_rows, es.dt_table, (const int*)es.step, dt_val, has_uncond,
                           es.keep ? *es.keep : EulerKeep{});
    };
    const std::true_type yes; const std::false_type no;
    if (es.keep && es.scale_rows) go(yes, yes); else if (es.keep) go(yes, no); else if (es.scale_rows) go(no, yes); else go(no, no);
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
