// Conv1d / polyphase ConvTranspose1d, host side: the launch descriptor with the checks that fail a call, the route among the conv kernels
// (conv1d_f32.hip, conv1d_x3.hip, conv1d_bf16.hip, conv1d_f32g.hip, conv1d_f32w.hip, the GEMM for wide pre-transposed layers) and launch_conv1d.
#include <stdlib.h>

#include "kernels.h"
#include "respair_dev.h"
#include "../../include/versband_hip.h"

// ---- launch_conv1d: descriptor (+ the checks that fail the call; n_count = output positions per phase) -> route -> launch
static int conv1d_fill(const ConvArgs& a, ConvDev& d, int& n_count) {
    d.x = a.x; d.x_bstride = a.x_bstride; d.Ci = a.Ci; d.T_in = a.T_in; d.x_bmod = a.x_bmod;
    d.w = a.w; d.w_bstride = a.w_bstride; d.bias = a.bias; d.Co = a.Co; d.dil = a.dil; d.pad = a.pad;
    d.upsample2 = a.upsample2; d.in_act = a.in_act; d.in_slope = a.in_slope;
    d.in_stride = a.in_stride > 0 ? a.in_stride : 1; d.in_phase = a.in_phase;
    if (d.in_stride > 1 && (a.upsample2 || a.tr_stride > 1)) VB_FAIL(VB_E_INVALID, "conv1d: in_stride with upsample/transpose");
    d.gn_mean = a.gn_mean; d.gn_rstd = a.gn_rstd; d.gn_gamma = a.gn_gamma; d.gn_beta = a.gn_beta; d.gn_groups = a.gn_groups;
    d.out = a.out; d.out_bstride = a.out_bstride; d.T_out = a.T_out; d.res = a.res; d.res_bstride = a.res_bstride;
    d.alpha = a.alpha; d.beta = a.beta; d.acc_scale = a.acc_scale; d.out_act = a.out_act; d.out_slope = a.out_slope;
    d.out_transposed = a.out_transposed; d.add = a.add; d.add_bstride = a.add_bstride; d.add_bmod = a.add_bmod;
    d.wp = a.wp; d.wp_plane = a.wp_plane; d.Ci_pad = a.Ci_pad; d.wp_bstride = a.wp_bstride;
    d.xt = a.xt; d.xt_Tp = xt_rows(a.upsample2 ? 2 * a.T_in : a.T_in); d.xt_plane = (int64_t)a.B * d.xt_Tp * a.Ci;
    if (a.wp_bf16 && (!a.wp || a.wp_bstride || a.w_mf)) VB_FAIL(VB_E_INVALID, "conv1d: bf16 weights are one shared plane (no per-clip or minimal-filtering weights)");
    if (a.xt && (a.Ci % 32 || a.tr_stride > 1 || a.in_stride > 1 || !a.wp || a.x_bmod || a.pad > XT_HEAD))
        VB_FAIL(VB_E_INVALID, "conv1d: XT input needs Ci %% 32 == 0, stride 1, split weights, pad <= %d", XT_HEAD);
    if (a.xt && a.xt_np != (a.wp_bf16 ? 1 : 2))
        VB_FAIL(VB_E_INVALID, "conv1d: XT input of %d plane(s): bf16 weights read a one-plane buffer, split weights a two-plane one", a.xt_np);
    // (the DMA'd windows of the last time tile reach at most 64 + 256 rows past row T_out of the padded image: inside its XT_TAIL zero rows)
    if (a.xt && a.T_out > (a.upsample2 ? 2 * a.T_in : a.T_in) + XT_HEAD)
        VB_FAIL(VB_E_INVALID, "conv1d: XT input of %d positions cannot feed %d outputs", a.upsample2 ? 2 * a.T_in : a.T_in, a.T_out);
    d.stage_epi = 0;
    d.row_len = a.row_len; d.len_mul = a.len_mul;
    if (a.row_len && (d.in_stride > 1 || a.x_bmod || a.len_mul < 1)) VB_FAIL(VB_E_INVALID, "conv1d: row lengths with in_stride, folded clips or len_mul < 1");
    if (a.tr_stride > 1) {
        d.phases = a.tr_stride; d.tr_pad = a.tr_pad; d.ntaps = (a.tr_k + a.tr_stride - 1) / a.tr_stride; d.dil = 1;
        n_count = cdiv(a.T_out, a.tr_stride);
        if (a.out_transposed) VB_FAIL(VB_E_INVALID, "conv1d: transposed output not supported with tr_stride");
    } else {
        d.phases = 1; d.tr_pad = 0; d.ntaps = a.ksize; n_count = a.T_out;
    }
    if ((d.ntaps - 1) * d.dil > CONV_HALO) VB_FAIL(VB_E_INVALID, "conv1d: halo %d exceeds %d", (d.ntaps - 1) * d.dil, CONV_HALO);
    if (a.out_transposed && (a.Co % 4)) VB_FAIL(VB_E_INVALID, "conv1d: transposed output needs Co%%4==0");
    if ((a.in_act == ACT_GN_SWISH || a.in_act == ACT_GN) && (a.Ci % a.gn_groups)) VB_FAIL(VB_E_INVALID, "conv1d: Ci %% groups");
    return VB_OK;
}

// Wide layers over pre-activated transposed planes ARE GEMMs (rows = clip x time, K = taps x Ci, both operands K-contiguous
// already): the DMA-fed 128 x 128 GEMM kernel walks K tap by tap (GemmArgs::conv_*), three bf16 passes for the split precision, one
// (nseg = 1: the one activation plane against the one weight plane [tap][Co][Ci_pad], plane 0 of the split packing, so the tap stride is
// the same) for bf16 weights; bias + residual in a channel-major epilogue.  The tap walk at one segment: gemm_k_offsets takes step t as
// (seg, kt) = (t / KT, t % KT) with KT = taps * Ci / 64 - seg stays 0, no plane offset is ever added, and the ring's stage index t % NST and
// its counted waits depend on the step count alone (the prologues of both DMA kernels guard total < ring depth: K = 64 is one step).
// launch_gemm's conv-mode tile choice does not look at K (gemm_route's last rule): 128 x 128, or 64 x 64 under 200 workgroups, as for split.  Measured on these shapes (tools/conv_as_gemm_calib.py): 750-840 TFLOP/s of bf16
// MFMA work against ~385 of conv1d_x3_kernel, which stages weights through registers and synchronises per (tap, 32 channels).
// (B * T_out / Co beyond launch_gemm's reciprocal-divide range fall through to the conv kernels - ADVICE r3)
static bool conv1d_as_gemm_eligible(const ConvArgs& a, const ConvDev& d) {
    return a.xt && a.wp && a.Co >= 384 && a.Ci % 64 == 0 && a.Ci_pad == a.Ci && a.Co % 4 == 0 && d.phases == 1 && !a.wp_bstride && !a.w_bstride &&
           a.alpha == 1.f && a.beta == 0.f && a.acc_scale == 1.f && a.out_act == ACT_NONE && !a.out_transposed && !a.add &&
           a.out_bstride == (int64_t)a.Co * a.T_out && (!a.res || a.res_bstride == a.out_bstride) &&
           a.T_out == (a.upsample2 ? 2 * a.T_in : a.T_in) && (int64_t)a.B * a.T_out < (1 << 21) && a.Co < (1 << 21);
}
static int launch_conv1d_as_gemm(const ConvArgs& a, const ConvDev& d, hipStream_t st) {
    GemmArgs g;
    g.A = a.xt; g.a_plane = d.xt_plane; g.lda = a.Ci; g.B = a.wp; g.b_plane = a.wp_plane; g.ldb = a.Ci_pad;
    g.M = a.B * a.T_out; g.N = a.Co; g.K = d.ntaps * a.Ci; g.nseg = a.wp_bf16 ? 1 : 3; g.ngroups = a.B;
    g.group_rows = a.T_out; g.T = a.T_out; g.epi = EPI_F32_CT; g.bias = a.bias; g.out32 = a.out; g.res32 = a.res;
    g.conv_ci = a.Ci; g.conv_dil = d.dil; g.conv_agrp = d.xt_Tp; g.conv_arow0 = XT_HEAD - a.pad; g.conv_btap = (int64_t)a.Co * a.Ci_pad;
    g.prof_class = 2;
    return launch_gemm(g, st);
}
// staged epilogue (conv_epilogue_staged; the minimal-filtering kernel has no other): plain [b][co][t] output whose rows start 16-B aligned
static bool conv1d_stage_epi_eligible(const ConvArgs& a) {
    return a.tr_stride <= 1 && !a.out_transposed && a.T_out % 4 == 0 && a.out_bstride % 4 == 0 && (!a.res || a.res_bstride % 4 == 0) &&
           aligned16(a.out) && (!a.res || aligned16(a.res));
}
// conv1d_co1_kernel: one output channel of an ordinary stride-1 convolution, shared fp32 weights, input transform none / LeakyReLU
static bool conv1d_co1_eligible(const ConvArgs& a, const ConvDev& d) {
    return a.Co == 1 && a.w && !a.xt && !a.w_bstride && !a.x_bmod && d.phases == 1 && d.in_stride == 1 && !a.upsample2 && !a.out_transposed &&
           (a.in_act == ACT_NONE || a.in_act == ACT_LRELU);
}
// conv1d_x3_kernel: split-bf16 weights are there - and per clip where the fp32 ones are
static bool conv1d_x3_eligible(const ConvArgs& a) { return a.wp && (!a.w_bstride || a.wp_bstride); }

enum ConvRoute { CONV_AS_GEMM, CONV_F32W, CONV_CO1, CONV_BF16_XT, CONV_BF16, CONV_X3_XT, CONV_X3, CONV_F32G, CONV_F32 };
static_assert(CONV_AS_GEMM == VB_ROUTE_AS_GEMM && CONV_F32W == VB_ROUTE_F32W && CONV_CO1 == VB_ROUTE_CO1 && CONV_BF16_XT == VB_ROUTE_BF16_XT &&
              CONV_BF16 == VB_ROUTE_BF16 && CONV_X3_XT == VB_ROUTE_X3_XT && CONV_X3 == VB_ROUTE_X3 && CONV_F32G == VB_ROUTE_F32G &&
              CONV_F32 == VB_ROUTE_F32, "vb_conv1d_plan reports ConvRoute under the public names");
// Which kernel runs: the first candidate, in this order, whose conditions hold and whose A/B knob has not switched it off; the register-staged
// fp32 kernel takes everything.  Settles d.stage_epi on the way (VB_CONV_DIRECT_EPI=1: the direct epilogue - no minimal filtering then).
static ConvRoute conv1d_route(const ConvArgs& a, ConvDev& d) {
    const VbTune& tune = vb_tune();
    if (conv1d_as_gemm_eligible(a, d) && !tune.conv_gemm_off) return CONV_AS_GEMM;
    d.stage_epi = (conv1d_stage_epi_eligible(a) && !tune.conv_direct_epi) ? 1 : 0;
    if (conv1d_f32w_eligible(a, d) && !tune.conv_mf_off) return CONV_F32W;
    if (conv1d_co1_eligible(a, d) && !tune.conv_f32_old) return CONV_CO1;             // (VB_CONV_F32_OLD=1: the MFMA kernels)
    if (a.wp_bf16) return a.xt ? CONV_BF16_XT : CONV_BF16;                            // one weight plane: no other kernel reads it
    if (conv1d_x3_eligible(a)) return a.xt ? CONV_X3_XT : CONV_X3;
    // exact fp32, DMA-fed; VB_CONV_F32_OLD=1 keeps the register-staged kernel (bit-identical, tests compare the two)
    if (conv1d_f32g_eligible(a, d) && !tune.conv_f32_old) return CONV_F32G;
    return CONV_F32;
}

int launch_conv1d(const ConvArgs& a, hipStream_t st) {
    ConvDev d;
    int n_count;
    VB_TRY(conv1d_fill(a, d, n_count));
    const ConvRoute route = conv1d_route(a, d);
    if (route == CONV_AS_GEMM) return launch_conv1d_as_gemm(a, d, st);      // (launch_gemm profiles itself: GemmArgs::prof_class)
    // (flops of the profiler's class table: EXECUTED MFMA work - the minimal-filtering kernel runs pseudo-taps / 2 products per output)
    const double taps_eff = route == CONV_F32W ? 0.5 * conv1d_f32w_pseudo_taps(a.ksize) : (a.tr_stride > 1 ? (double)a.tr_k / a.tr_stride : (double)a.ksize);
    ProfScope prof(2, 2.0 * a.B * a.Co * a.Ci * (double)a.T_out * taps_eff,
                   4.0 * a.B * ((double)a.Ci * a.T_in + (double)a.Co * a.T_out * (1.0 + (a.res ? 1.0 : 0.0) + (a.beta != 0.f ? 1.0 : 0.0)))
                       + 4.0 * (double)a.Co * a.Ci * (a.tr_stride > 1 ? a.tr_k : a.ksize), st);
    switch (route) {
        case CONV_AS_GEMM: break;      // (left above)
        case CONV_F32W: d.ww = a.w_mf; launch_conv1d_f32w(d, a.B, st); break;
        case CONV_CO1: launch_conv1d_co1(d, a.B, st); break;
        case CONV_BF16_XT:
        case CONV_BF16: VB_TRY(launch_conv1d_bf16(d, conv_staged_tile(a.Co, n_count, a.B, d.phases), n_count, a.B, route == CONV_BF16_XT, st)); break;
        case CONV_X3_XT:
        case CONV_X3: VB_TRY(launch_conv1d_x3(d, conv_staged_tile(a.Co, n_count, a.B, d.phases), n_count, a.B, route == CONV_X3_XT, st)); break;
        case CONV_F32G: launch_conv1d_f32g(d, n_count, a.B, a.upsample2, st); break;
        case CONV_F32: launch_conv1d_f32(d, n_count, a.B, st); break;
    }
    VB_CHECK_LAUNCH();
    return VB_OK;
}

// ---- the plan of a call, host only (vb_conv1d_plan): descriptor -> route -> the tile that route's launcher picks.  Nothing is launched and no
// pointer is read: the operands are stand-in addresses that carry only what the route looks at - presence and 16-byte alignment.
static void conv_tile_dims(ConvTileId id, int* co, int* t) {
    static const int dims[4][2] = {{128, 128}, {128, 64}, {64, 128}, {32, 256}};
    *co = dims[id][0]; *t = dims[id][1];
}
extern "C" int vb_conv1d_plan(int B, int Ci, int T_in, int Co, int ksize, int dil, int pad, int tr_stride, int tr_pad, int tr_k, int T_out,
                              int upsample2, int in_stride, int in_phase, int in_act, int gn_groups, float alpha, float beta, int wforms,
                              int ci_pad, int xt, int has_res, int misalign, int* route, int* tile_co, int* tile_t, int* stage_epi) {
    if (B < 1 || Ci < 1 || T_in < 1 || Co < 1 || T_out < 1 || !route || !tile_co || !tile_t || !stage_epi)
        VB_FAIL(VB_E_INVALID, "conv1d_plan: B/Ci/T/Co < 1 or null result pointer");
    if (!(wforms & (VB_PLAN_W_F32 | VB_PLAN_W_X3 | VB_PLAN_W_BF16))) VB_FAIL(VB_E_INVALID, "conv1d_plan: no weight form the kernels can run on");
    auto at = [&](int bit, uintptr_t slot) { return (const void*)(slot * 4096 + ((misalign & bit) ? 4 : 0)); };
    ConvArgs a;
    a.B = B; a.x = (const float*)at(VB_PLAN_X_4B, 1); a.x_bstride = (int64_t)Ci * T_in; a.Ci = Ci; a.T_in = T_in; a.Co = Co; a.ksize = ksize;
    a.dil = dil; a.pad = pad; a.tr_stride = tr_stride; a.tr_pad = tr_pad; a.tr_k = tr_k; a.T_out = T_out; a.upsample2 = upsample2;
    a.in_stride = in_stride > 1 ? in_stride : 1; a.in_phase = in_phase; a.in_act = in_act; a.gn_groups = gn_groups > 0 ? gn_groups : 32;
    a.alpha = alpha; a.beta = beta;
    a.out = (float*)at(VB_PLAN_OUT_4B, 2); a.out_bstride = (int64_t)Co * T_out;
    if (has_res) { a.res = (const float*)at(VB_PLAN_RES_4B, 3); a.res_bstride = a.out_bstride; }
    if (wforms & VB_PLAN_W_F32) a.w = (const float*)at(VB_PLAN_W_4B, 4);
    if (wforms & VB_PLAN_W_MF) a.w_mf = (const float*)at(VB_PLAN_W_4B, 5);
    if (wforms & (VB_PLAN_W_X3 | VB_PLAN_W_BF16)) {
        const int phases = tr_stride > 1 ? tr_stride : 1, ntaps = tr_stride > 1 ? (tr_k + tr_stride - 1) / tr_stride : ksize;
        a.wp = (const bf16_t*)at(0, 6); a.Ci_pad = ci_pad; a.wp_plane = (int64_t)phases * ntaps * Co * ci_pad; a.wp_bf16 = (wforms & VB_PLAN_W_BF16) != 0;
    }
    if (xt) { a.xt = (const bf16_t*)at(0, 7); a.xt_np = a.wp_bf16 ? 1 : 2; a.in_act = ACT_NONE; }      // (the activation is in the plane)
    ConvDev d;
    int n_count;
    VB_TRY(conv1d_fill(a, d, n_count));
    const ConvRoute r = conv1d_route(a, d);
    *route = (int)r; *stage_epi = d.stage_epi; *tile_co = 0; *tile_t = 0;
    switch (r) {
        case CONV_AS_GEMM: gemm_conv_tile(a.B, a.T_out, a.Co, tile_t, tile_co); break;      // (conv mode: 64 x 64 under VB_GEMM_SMALL_TILES workgroups, else 128 x 128)
        case CONV_F32W: conv1d_f32w_tile(d, tile_co, tile_t); break;
        case CONV_CO1: conv1d_co1_tile(tile_co, tile_t); break;
        case CONV_BF16_XT: case CONV_BF16: case CONV_X3_XT: case CONV_X3: conv_tile_dims(conv_staged_tile(a.Co, n_count, a.B, d.phases), tile_co, tile_t); break;
        case CONV_F32G: conv1d_f32g_tile(d, n_count, a.B, a.upsample2, tile_co, tile_t); break;
        case CONV_F32: conv1d_f32_tile(d, tile_co, tile_t); break;
    }
    return VB_OK;
}
// The same for the fused pairs: form = VB_PAIR_F32 / _MF / _X3 / _BF16.  The launchers choose no tile by grid size - a form has one run length
// per (C, dil) - so the plan is the support check, the run (intermediate positions per workgroup), the outputs a workgroup writes, the
// workgroups along time and the epilogue form.
extern "C" int vb_respair_plan(int form, int B, int C, int T, int k, int dil, int misalign, int* run, int* outputs, int* grid_t, int* staged) {
    if (B < 1 || T < 1 || !run || !outputs || !grid_t || !staged) VB_FAIL(VB_E_INVALID, "respair_plan: B/T < 1 or null result pointer");
    const float* x = (const float*)(uintptr_t)(4096 + ((misalign & VB_PLAN_X_4B) ? 4 : 0));
    float* out = (float*)(uintptr_t)(2 * 4096 + ((misalign & VB_PLAN_OUT_4B) ? 4 : 0));
    const void* w = (const void*)(uintptr_t)(3 * 4096);
    int r;
    if (form == VB_PAIR_F32 || form == VB_PAIR_MF) {
        RespairF32Args a;
        a.x = x; a.out = out; a.B = B; a.C = C; a.T = T; a.k = k; a.dil = dil; a.w1 = (const float*)w; a.w2 = (const float*)w;
        if (!(form == VB_PAIR_F32 ? respair_f32_supported(a) : respair_f32w_supported(a))) VB_FAIL(VB_E_INVALID, "respair_plan: C=%d k=%d dil=%d T=%d not supported by form %d", C, k, dil, T, form);
        r = form == VB_PAIR_F32 ? respair_f32_run() : respair_f32w_run(C, dil);
        PairLaunchT<PairF32Dev> L{};
        VB_TRY(pair_fill_common(a, "respair_plan", r, (double)k, L));
        *staged = L.d.staged;
    } else if (form == VB_PAIR_X3 || form == VB_PAIR_BF16) {
        RespairArgs a;
        a.x = x; a.out = out; a.B = B; a.C = C; a.T = T; a.k = k; a.dil = dil; a.w1 = (const bf16_t*)w; a.w2 = (const bf16_t*)w;
        PairLaunch L{};
        VB_TRY(pair_fill(a, "respair_plan", L));
        r = PAIR_T; *staged = L.d.staged;
    } else VB_FAIL(VB_E_INVALID, "respair_plan: form %d", form);
    *run = r; *outputs = pair_run_outputs(r, k); *grid_t = cdiv(T, *outputs);
    return VB_OK;
}
