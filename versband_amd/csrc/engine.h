// What the host translation units of libversband_hip.so share (runtime.hip, dit.hip, sampler.hip, convnet.hip, abi_units.hip and the
// host drivers at the end of t5.hip / melnet.hip): the context, the workspace carver, the DiT layouts and the calls that cross files.
// No device allocation happens on the host side: all scratch is carved out of caller buffers (sizes from *_bytes()).
#pragma once
#include <algorithm>
#include <array>
#include <tuple>
#include <vector>

#include "../../include/versband_hip.h"
#include "kernels.h"

struct NetProgram {
    std::vector<vb_net_op> ops;
    std::vector<vb_buf_desc> bufs;
    int in_ch = 0, out_ch = 0, in_tmul = 1, out_tmul = 1;
    bool loaded = false;
};
// one captured + instantiated step loop of vb_sample_cfg (hipGraph), keyed by everything the launches bake in (the key of a call is
// made in one place: sample_key, beside SampleCall)
struct SampleGraph {
    struct Key {
        const void* x = nullptr; const void* cond = nullptr; const void* ws = nullptr;
        int B = 0, nb = 0, T = 0, L = 0, n_steps = 0; float cfg_scale = 0.f;
        unsigned tune_gen = 0;            // a captured graph bakes the knob-dependent kernel selection in
        const void* keep_ref = nullptr; const void* keep_x0 = nullptr; const void* keep_mask = nullptr; float sigma_min = 0.f;   // vb_sample_cfg_keep (all null: a plain call)
        const void* rows_scale = nullptr; const void* rows_clip = nullptr;   // vb_sample_cfg_rows: the two POINTERS (cfg_scale is 0 beside rows_scale); their contents are read when the kernels run
        int nw = 0; std::array<int, 64> starts{};    // vb_sample_cfg_windows: the plan's VALUES (the kernel argument holds them); nw = 0: no windows
        int nlens = 0; std::array<int, 64> lens{};   // vb_sample_cfg_lens: the row lengths' VALUES (the table fill at the head of the step loop holds them); nlens = 0: no lengths
        int nwr = 0; std::array<int, 64> wr_group{}, wr_start{}, wr_len{};   // vb_sample_cfg_window_rows: the VALUES of group, start and the rows' lengths (the pair table in the kernel argument comes from them); nwr = 0: no window rows
        bool sched = false; std::array<float, 64> weights{};   // vb_sample_cfg_sched: the step weights' VALUES (launch arguments, and which steps run one branch); sched = false: no schedule
        auto tie() const { return std::tie(x, cond, ws, B, nb, T, L, n_steps, cfg_scale, tune_gen, keep_ref, keep_x0, keep_mask, sigma_min, rows_scale, rows_clip, nw, starts, nlens, lens, nwr, wr_group, wr_start, wr_len, sched, weights); }
        bool operator==(const Key& o) const { return tie() == o.tie(); }
    } key;
    int seen = 0;                         // calls with this key so far (the first runs eagerly, the second captures)
    bool failed = false;                  // capture was refused once (e.g. legacy default stream): stay eager
    hipGraph_t graph = nullptr; hipGraphExec_t exec = nullptr;
    uint64_t last_use = 0;
    void destroy() {
        if (exec) (void)hipGraphExecDestroy(exec);
        if (graph) (void)hipGraphDestroy(graph);
        exec = nullptr; graph = nullptr;
    }
};
struct vb_ctx {
    int device = 0;
    std::vector<SampleGraph> graphs; uint64_t graph_clock = 0;
    bool dit_loaded = false;
    vb_dit_config cfg;
    vb_dit_weights w;
    NetProgram nets[3];
    bool t5_loaded = false;
    vb_t5_config t5cfg;
    vb_t5_weights t5w;
    bool mel_loaded = false;
    vb_mel_config melcfg;
    const float* mel_dft = nullptr; const float* mel_basis_t = nullptr;
};

static inline size_t align_up(size_t x, size_t a = 256) { return (x + a - 1) / a * a; }
struct Carver {
    char* base; size_t off = 0;
    explicit Carver(void* b) : base(static_cast<char*>(b)) {}
    template <typename T> T* take(size_t n) {
        T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
        off = align_up(off + n * sizeof(T));
        return p;
    }
};
static inline int pad64(int x) { return (x + 63) / 64 * 64; }
static inline Planes mkp(bf16_t* p, int64_t numel, int np) { return Planes{p, numel, np}; }
static inline Planes wpl(const void* p, int64_t numel, int np) { return Planes{(bf16_t*)p, numel, np}; }

// ---- runtime.hip ----------------------------------------------------------------------------
// roctx range (rocprofv3 --marker-trace); the profiler's marker library is looked up at run time
struct RoctxRange {
    bool on;
    explicit RoctxRange(const char* name);
    ~RoctxRange();
};
bool prof_enabled();      // the per-launch HIP-event profiler (vb_prof_enable) is on: the sampler then stays eager

// ---- dit.hip: layouts, one network evaluation -------------------------------------------------
struct CondL {
    float* ac; float* cemb;
    bf16_t* ky[VB_MAX_DEPTH]; bf16_t* vyt[VB_MAX_DEPTH]; bf16_t* kc[VB_MAX_DEPTH]; bf16_t* vct[VB_MAX_DEPTH];
    float* la[VB_MAX_DEPTH];
    // folded caption gate (see router_kernel<.., true>): per clip and block the caption keys with the MoE q-projection folded in
    // (planes [Beff][NS = L*heads][D], row = key*heads + head), the q-bias part of the scores and the gate-contracted values
    bf16_t* mf[VB_MAX_DEPTH]; float* cb[VB_MAX_DEPTH]; float* vw[VB_MAX_DEPTH]; int* clip_off; int NS; bool fold;
    bf16_t* pin_w;       // proj_in weights as a GEMM operand: split planes [2][D][PIN_KP], k = tap * 32 + ci (conv_w_to_gemm_kernel)
    int64_t n_k, n_vt; int Lpad;
    size_t total;
};
#define T_FREQ_ROWS 1000  // rows of vb_dit_weights.t_freq_table (pack.timestep_table); other indices are computed in the kernel
#define PRE_STEPS 64      // sampler steps whose adaLN / gate vectors are tabulated up front
struct WsL {
    int* step; int64_t* t_idx_cur; int64_t* t_table; float* dt_table;
    float* tn_table;                                                // vb_sample_cfg_keep: t after every step (carved last: no other offset moves)
    int* len_table;                                                 // vb_lens: the row lengths [B <= 64] (carved after it, by the same rule)
    float *temb0, *temb, *mod_all, *hl, *h, *cq32, *mc, *ma, *y32, *g1, *g2, *g3, *v;
    bf16_t* modA;                                                   // A operand (planes) of the adaLN tabulation GEMM
    float *temb0_s, *temb_s, *hl_s, *mod_s; int64_t* row_step;     // per-sample tables of the conditioning vectors of every step
    bf16_t *u, *q, *k, *vt, *a, *qm, *cqa, *Hs, *y, *Hf, *pin_a;
    int *ic, *ia, *group_off, *perm, *pair_off, *pair_pa;
    // precompute temporaries
    float *tA, *tB, *tC, *tD, *tE, *cap_pre, *cap32, *pooled, *pooled_ln;
    bf16_t *t5p, *gel, *capp, *yp;
    int64_t n_tok, n_vt; int Tpad, MODW;
    size_t total;
};
CondL carve_cond(void* base, const vb_dit_config& c, int B, int nb, int T, int L);
WsL carve_ws(void* base, const vb_dit_config& c, int B, int nb, int T, int L);

// Every choice one network evaluation makes, stated once (dit_plan): each member is a function of the loaded model, the knobs and
// (B, nb, T, L) alone, so precompute, evaluation and sampler cannot disagree, and none depends on anything that varies between the
// blocks of an evaluation.
// An evaluation over nb_active < nb branches of the nb layout (a single-branch step of vb_sample_cfg_sched): the members that describe
// the LAYOUT (proj_in_split_w, proj_in_gemm, fold_layout, w2_pair - model and L alone) are those of nb; the members that pick a kernel
// from the token count (router_counts, band_fused, score_fused, gate_route, final_route) follow the active rows, i.e. are those of an nb_active call.
enum FinalRoute {
    FINAL_EULER_FUSED,   // FinalLayer + CFG + Euler update + step advance as one launch: only with DitEval::euler (the sampler);
                         // an evaluation without it takes FINAL_FUSED, whose conditions this route includes
    FINAL_FUSED,         // one wave per token row, projection against LDS-resident weights
    FINAL_GEMM,          // LayerNorm + modulate to split planes, projection on the MFMA GEMM
    FINAL_ROWS           // the generic kernel
};
struct DitPlan {
    const vb_dit_weights* w = nullptr;
    bool router_counts = false, w2_pair = false, band_fused = false, proj_in_split_w = false, proj_in_gemm = false;
    bool fold_layout = false, score_fused = false, gate_route = false;
    FinalRoute final_route = FINAL_ROWS;
    // block i takes the folded caption gate: the layout holds its operands and the pack carries the folded weights
    bool gate_fold(int i) const { return fold_layout && w->blocks[i].wqt_s && w->blocks[i].bq_s; }
};
DitPlan dit_plan(const vb_ctx* ctx, int B, int nb, int T, int L, int nb_active = 0);      // nb_active = 0: nb

// one network evaluation (both CFG branches batched: rows [0,B) cond, [B,2B) uncond); a caller fills what it uses
struct DitEval {
    const float* x = nullptr; const int64_t* t_idx = nullptr; const void* cond = nullptr; void* ws = nullptr;
    int B = 0, nb = 0, T = 0, L = 0;
    // branches evaluated (0: all nb).  1 beside nb = 2: the conditional rows [0, B) alone, in the layout of nb - cond, workspace, plane
    // strides, injected-noise arrays and the tabulated pre_mod rows keep their two-branch offsets; every row and group count follows B
    int nb_active = 0;
    const vb_noise* noise = nullptr; int noise_step = 0; const int* step_ptr = nullptr;
    const int64_t* clip_rows = nullptr;                         // vb_sample_cfg_rows: device [B] global clip ids of the router noise (null: noise->clip_base + b)
    float* v_out = nullptr; int32_t* route_out = nullptr;
    bool zero_vt = false;                                       // clear the padded V^T planes first (a stand-alone call)
    // vb_lens: device [B] row lengths (null: every row has T tokens).  The three places that look across a clip's end read it: proj_in's
    // taps, the self-attention's keys, and - in precompute - the acoustic stem.  Both branches read len[b % B].
    const int* lens = nullptr;
    const float* pre_mod = nullptr; const float* pre_hl = nullptr;   // this step's rows of the sampler's tabulated conditioning vectors
    int evals_before = -1;                                      // block evaluations already done in this call (< 0: stand-alone, see DitPlan::router_counts)
    const EulerStep* euler = nullptr;                           // sampler only: FinalLayer does this step's update in the same launch (x in place, v_out not written)
};
int dit_forward(vb_ctx* ctx, const DitEval& ev, hipStream_t st);

// ---- sampler.hip: one sampler call ------------------------------------------------------------
// One call of vb_sample_cfg_window_rows (the older entry points forward to it), validated and normalised where it is made
// (sampler.hip:sample_call): the step loop launches from it and the graph cache keys on it, so an option is one member here.
// THE RULE: anything a launch of the step loop bakes in is in the key (sample_key, below), by ADDRESS where the kernels read through the
// pointer when they run, by VALUE where the launch argument - or the choice of launch - holds the value itself (SampleGraph::Key says which).
struct SampleCall {
    float* x = nullptr; const void* cond = nullptr; void* ws = nullptr;
    int B = 0, nb = 0, T = 0, L = 0, n_steps = 0;
    float cfg_scale = 0.f;                  // 0 beside rows.cfg_scale, which replaces it
    vb_rows rows{nullptr, nullptr};         // either may be null: clip b is guided by rows.cfg_scale[b] (unused with nb == 1) and draws its router noise as clip rows.clip[b]
    const vb_keep* keep = nullptr;          // every update also puts the known tokens back on the probability path at the time after the step (t_next: a workspace table, like dt)
    // windows: more than one (one is the plain call) - the rows are wp.nw windows of B / nw clips; after every update, in either form, the
    // overlapping tokens of neighbouring windows take their consensus value, before the trajectory copy
    WindowPlan wp; bool windows = false;
    LensPlan lens;                          // row lengths: lens.B == B when some row is shorter than T, else 0 (the plain call); the step loop starts by writing them to the workspace table
    // window rows: the rows are windows of clips of different lengths, described row by row (kernels.h: WindowRowsPlan); the consensus runs
    // where the windows' does, over the plan's pair table.  wrows = some group has two overlapping rows (none: the call without the block)
    WindowRowsPlan wr; bool wrows = false;
    const float* gw = nullptr;              // host [n_steps] step weights (sample_steps has the kinds of step); null unless nb == 2 and some weight differs from 1
    const vb_noise* noise = nullptr;        // NOT keyed: the noise key travels through device memory, injected arrays keep a call eager
};
static_assert(PRE_STEPS <= 64, "the graph key holds the step weights of a graphable call (SampleGraph::Key::weights)");
inline SampleGraph::Key sample_key(const SampleCall& sc) {
    SampleGraph::Key key;
    key.x = sc.x; key.cond = sc.cond; key.ws = sc.ws; key.B = sc.B; key.nb = sc.nb; key.T = sc.T; key.L = sc.L; key.n_steps = sc.n_steps; key.cfg_scale = sc.cfg_scale;
    key.tune_gen = vb_tune_generation();
    if (sc.keep) { key.keep_ref = sc.keep->ref; key.keep_x0 = sc.keep->x0; key.keep_mask = sc.keep->mask; key.sigma_min = sc.keep->sigma_min; }
    key.rows_scale = sc.rows.cfg_scale; key.rows_clip = sc.rows.clip;
    if (sc.windows) { key.nw = sc.wp.nw; std::copy(sc.wp.s, sc.wp.s + 64, key.starts.begin()); }
    if (sc.lens.B) { key.nlens = sc.lens.B; std::copy(sc.lens.len, sc.lens.len + 64, key.lens.begin()); }
    if (sc.wrows) {
        key.nwr = sc.wr.B; std::copy(sc.wr.group, sc.wr.group + 64, key.wr_group.begin()); std::copy(sc.wr.start, sc.wr.start + 64, key.wr_start.begin());
        for (int r = 0; r < sc.wr.B; ++r) key.wr_len[r] = sc.lens.B ? sc.lens.len[r] : sc.T;
    }
    if (sc.gw) { key.sched = true; std::copy(sc.gw, sc.gw + sc.n_steps, key.weights.begin()); }      // (a keyed call is graphable: n_steps <= PRE_STEPS = 64)
    return key;
}

// ---- convnet.hip ----------------------------------------------------------------------------
// row lengths of a conv-net run (vb_hifigan_forward_lens): the validated plan and its device table in the workspace
struct NetLens { LensPlan lp; const int* table = nullptr; };
int net_run(vb_ctx* ctx, int which, const float* in, int B, int T, float* out, void* ws, hipStream_t st, const NetLens* nl = nullptr);
