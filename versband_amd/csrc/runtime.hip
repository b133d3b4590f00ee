// Process-wide runtime of libversband_hip.so: the last-error string, the VB_* knob loader, the roctx shim, the per-launch HIP-event
// profiler, and the context's lifetime.
#include <stdlib.h>
#include <string.h>

#include <dlfcn.h>

#include <atomic>
#include <mutex>

#include "engine.h"

thread_local char g_vb_err[512] = "";

// ---- tuning knobs ---------------------------------------------------------------------------
static VbTune g_tune;
static std::atomic<bool> g_tune_loaded{false};
static std::atomic<unsigned> g_tune_gen{0};
static std::mutex g_tune_mu;
static int env_int(const char* k, int dflt) { const char* v = getenv(k); return (v && *v) ? atoi(v) : dflt; }
static void tune_load() {
    VbTune t;
    // product knobs: result-preserving selections the tests flip to compare both forms, plus VB_ATTN_DEFER / VB_NO_GRAPH
    t.router_tpw = env_int("VB_ROUTER_TPW", 0);
    if (const char* v = getenv("VB_ATTN_DEFER")) t.attn_defer_thr = (float)atof(v);     // log2 units; 0 = exact running maximum
    t.gemm_small = env_int("VB_GEMM_SMALL", 11); t.gemm_small_tiles = env_int("VB_GEMM_SMALL_TILES", 200);
    t.gemm_tile = env_int("VB_GEMM_TILE", -1);
    t.conv_direct_epi = getenv("VB_CONV_DIRECT_EPI") != nullptr;
    t.band_unfused = getenv("VB_BAND_UNFUSED") != nullptr;
    t.w2_pair = env_int("VB_W2_PAIR", 1);
    t.qkv_p16_off = getenv("VB_QKV_P16_OFF") != nullptr;
    t.no_xcd_groups = getenv("VB_NO_XCD_GROUPS") != nullptr;
    t.qkv_vt16_off = getenv("VB_QKV_VT16_OFF") != nullptr;
    t.rmsnorm_generic = getenv("VB_RMSNORM_GENERIC") != nullptr;
    t.wide_resid = env_int("VB_WIDE_RESID", 1);
    t.big_tile_min_k = env_int("VB_BIG_TILE_MIN_K", 384);
    t.proj_in_conv = getenv("VB_PROJ_IN_CONV") != nullptr;
    t.conv_gemm_off = getenv("VB_CONV_GEMM_OFF") != nullptr;
    t.final_gemm = getenv("VB_FINAL_GEMM") != nullptr;
    t.router_generic = getenv("VB_ROUTER_GENERIC") != nullptr;
    t.gate_route = env_int("VB_GATE_ROUTE", -1);      // 0: score GEMM + router launches, 1: the one-launch caption gate at every token count
    t.band_epi_old = getenv("VB_BAND_EPI_OLD") != nullptr;
    t.conv_f32_old = getenv("VB_CONV_F32_OLD") != nullptr;
    t.gemm_p8_off = getenv("VB_GEMM_P8_OFF") != nullptr;
    t.bucket_count_launch = getenv("VB_BUCKET_COUNT_LAUNCH") != nullptr;
    t.euler_launch = getenv("VB_EULER_LAUNCH") != nullptr;
    t.conv_f32_rt_taps = getenv("VB_CONV_F32_RT_TAPS") != nullptr;
    t.conv_mf_off = getenv("VB_CONV_MF_OFF") != nullptr; t.conv_mf_occ = env_int("VB_MF_OCC", 2);        // minimal-filtering weights ignored: the direct fp32 kernels (A/B)
    t.no_graph = getenv("VB_NO_GRAPH") != nullptr;
#ifdef VB_EXPERIMENTS
    // experiments build only (VB_BUILD_EXPERIMENTS=1 python -m versband_amd.build): ablations and the measured-slower kernels
    t.gemm_variant = env_int("VB_GEMM_VARIANT", 1); t.gemm_ablate = env_int("VB_GEMM_ABLATE", 0);
    t.gemm_nchunk = env_int("VB_GEMM_NCHUNK", 0); t.gemm_p8 = env_int("VB_GEMM_P8", -1);
    t.gemm_p8_mask = env_int("VB_GEMM_P8_MASK", 0); t.gemm_p8_direct = env_int("VB_GEMM_P8_DIRECT", 0); t.gemm_p8_p16 = env_int("VB_GEMM_P8_P16", 0);
    t.conv_ablate = env_int("VB_CONV_ABLATE", 0);
    t.attn_ablate = env_int("VB_ATTN_ABLATE", 0); t.attn_variant = env_int("VB_ATTN_VARIANT", -1);
    t.score_fused = getenv("VB_SCORE_FUSED") != nullptr;
    t.gemm_pk_f32 = env_int("VB_GEMM_PK_F32", 0); t.gemm_pk = env_int("VB_GEMM_PK", 0); t.gemm_p8_ring = env_int("VB_GEMM_P8_RING", 0);
    // round-2 A/B switches no test flips any more: the caption gate without the fold, the once-per-clip stem convolutions in exact fp32
    t.gate_unfolded = getenv("VB_GATE_UNFOLDED") != nullptr; t.stem_f32 = getenv("VB_STEM_F32") != nullptr;
#endif
    g_tune = t;
    g_tune_gen.fetch_add(1, std::memory_order_relaxed);
    g_tune_loaded.store(true, std::memory_order_release);
}
const VbTune& vb_tune() {
    if (!g_tune_loaded.load(std::memory_order_acquire)) {
        std::lock_guard<std::mutex> lk(g_tune_mu);
        if (!g_tune_loaded.load(std::memory_order_relaxed)) tune_load();
    }
    return g_tune;
}
unsigned vb_tune_generation() { (void)vb_tune(); return g_tune_gen.load(std::memory_order_relaxed); }
// (tools / tests only, single-threaded by contract: no launch may be in flight on another host thread while the knobs change)
extern "C" void vb_tune_reload(void) {
    std::lock_guard<std::mutex> lk(g_tune_mu);
    tune_load();
}

// ---- roctx ranges (rocprofv3 --marker-trace): the profiler's marker library is looked up at run time, nothing links against it ----
typedef int (*roctx_push_fn)(const char*);
typedef int (*roctx_pop_fn)(void);
static roctx_push_fn g_roctx_push = nullptr;
static roctx_pop_fn g_roctx_pop = nullptr;
static std::once_flag g_roctx_once;
static void roctx_init() {
    for (const char* name : {"librocprofiler-sdk-roctx.so", "librocprofiler-sdk-roctx.so.1", "libroctx64.so", "libroctx64.so.4"}) {
        void* h = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
        if (!h) continue;
        g_roctx_push = (roctx_push_fn)dlsym(h, "roctxRangePushA");
        g_roctx_pop = (roctx_pop_fn)dlsym(h, "roctxRangePop");
        if (g_roctx_push && g_roctx_pop) return;
        g_roctx_push = nullptr; g_roctx_pop = nullptr;
    }
}
RoctxRange::RoctxRange(const char* name) {
    std::call_once(g_roctx_once, roctx_init);
    on = g_roctx_push != nullptr;
    if (on) (void)g_roctx_push(name);
}
RoctxRange::~RoctxRange() { if (on) (void)g_roctx_pop(); }

// ---- kernel-class profiling -----------------------------------------------------------------
#define PROF_CLASSES 4
#define PROF_POOL 32768
static int g_prof_mask = 0;
static std::vector<hipEvent_t> g_prof_ev;          // pool of events (pairs)
static size_t g_prof_next = 0;
struct ProfRec { int cls; size_t ev; };
static std::vector<ProfRec> g_prof_recs;
static double g_prof_flops[PROF_CLASSES] = {0, 0, 0, 0};
static double g_prof_bytes[PROF_CLASSES] = {0, 0, 0, 0};
static long long g_prof_launches[PROF_CLASSES] = {0, 0, 0, 0};
static thread_local size_t g_prof_open = (size_t)-1;
static thread_local unsigned g_prof_tick[PROF_CLASSES] = {0, 0, 0, 0};
static thread_local unsigned g_prof_tick_gen = 0;
static std::atomic<unsigned> g_prof_gen{1};         // bumped by vb_prof_enable: every host thread restarts its launch counters
static int g_prof_every[PROF_CLASSES] = {1, 1, 1, 1};   // time every n-th launch of a class (per host thread) ...
static int g_prof_phase[PROF_CLASSES] = {0, 0, 0, 0};   // ... the one with launch index % n == phase
static std::mutex g_prof_mu;                        // several host threads (one per stream) may launch concurrently
void prof_start(int cls, double flops, double bytes, hipStream_t st) {
    g_prof_open = (size_t)-1;
    if (!(g_prof_mask & (1 << cls))) return;
    const unsigned gen = g_prof_gen.load(std::memory_order_relaxed);
    if (g_prof_tick_gen != gen) { g_prof_tick_gen = gen; for (unsigned& t : g_prof_tick) t = 0; }
    const bool sampled = (int)(g_prof_tick[cls]++ % (unsigned)g_prof_every[cls]) == g_prof_phase[cls];
    std::lock_guard<std::mutex> lk(g_prof_mu);
    g_prof_launches[cls] += 1;
    if (!sampled || g_prof_next + 2 > g_prof_ev.size()) return;      // counted, not timed
    g_prof_flops[cls] += flops;
    g_prof_bytes[cls] += bytes;
    g_prof_open = g_prof_next;
    g_prof_next += 2;
    (void)hipEventRecord(g_prof_ev[g_prof_open], st);
}
void prof_stop(int cls, hipStream_t st) {
    if (g_prof_open == (size_t)-1) return;
    (void)hipEventRecord(g_prof_ev[g_prof_open + 1], st);
    {
        std::lock_guard<std::mutex> lk(g_prof_mu);
        g_prof_recs.push_back(ProfRec{cls, g_prof_open});
    }
    g_prof_open = (size_t)-1;
}
bool prof_enabled() { return g_prof_mask != 0; }

extern "C" {

const char* vb_last_error(void) { return g_vb_err; }
int vb_abi_version(void) { return 3; }
// (vb_source_digest() lives in a two-line translation unit versband_amd/build.py generates: csrc/build/vb_digest.cpp)
int vb_has_experiments(void) {
#ifdef VB_EXPERIMENTS
    return 1;
#else
    return 0;
#endif
}

int vb_prof_enable(int class_mask) {
    if (class_mask && g_prof_ev.empty()) {
        g_prof_ev.resize(2 * PROF_POOL);
        for (auto& e : g_prof_ev) VB_HIP(hipEventCreate(&e));
    }
    g_prof_mask = class_mask & 0xff;
    // bits 8..15: sampling period n of class 0 (the GEMM class: ~1250 launches per pass); bits 16..19: period of the other classes (0 = the same n);
    // bits 20..23 / 24..27: the phase of class 0 / of the others - a caller that walks all phases over as many passes times EVERY launch exactly
    // once per cycle without ever bracketing two neighbouring launches (back-to-back event pairs read long kernels twice as long)
    const int e0 = ((class_mask >> 8) & 0xff) > 0 ? ((class_mask >> 8) & 0xff) : 1;
    const int e1 = ((class_mask >> 16) & 0xf) > 0 ? ((class_mask >> 16) & 0xf) : e0;
    for (int i = 0; i < PROF_CLASSES; ++i) {
        g_prof_every[i] = i == 0 ? e0 : e1;
        g_prof_phase[i] = ((class_mask >> (i == 0 ? 20 : 24)) & 0xf) % g_prof_every[i];
    }
    g_prof_gen.fetch_add(1, std::memory_order_relaxed);
    g_prof_next = 0;
    g_prof_recs.clear();
    for (int i = 0; i < PROF_CLASSES; ++i) { g_prof_flops[i] = 0; g_prof_bytes[i] = 0; g_prof_launches[i] = 0; }
    return VB_OK;
}
int vb_prof_read(int cls, double* ms_sum, double* flops, double* bytes, int64_t* launches, int64_t* timed) {
    if (cls < 0 || cls >= PROF_CLASSES) VB_FAIL(VB_E_INVALID, "prof_read: class %d", cls);
    VB_HIP(hipDeviceSynchronize());
    double ms = 0; int64_t n = 0;
    for (const ProfRec& r : g_prof_recs) {
        if (r.cls != cls) continue;
        float t = 0.f;
        VB_HIP(hipEventElapsedTime(&t, g_prof_ev[r.ev], g_prof_ev[r.ev + 1]));
        ms += t; ++n;
    }
    *ms_sum = ms; *flops = g_prof_flops[cls]; *bytes = g_prof_bytes[cls]; *launches = g_prof_launches[cls]; *timed = n;
    return VB_OK;
}

int vb_ctx_create(int device, vb_ctx** out) {
    if (!out) VB_FAIL(VB_E_INVALID, "ctx_create: null out");
    int n = 0;
    VB_HIP(hipGetDeviceCount(&n));
    if (device < 0 || device >= n) VB_FAIL(VB_E_INVALID, "ctx_create: device %d of %d", device, n);
    VB_HIP(hipSetDevice(device));
    vb_ctx* c = new vb_ctx();
    c->device = device;
    memset(&c->cfg, 0, sizeof(c->cfg));
    memset(&c->w, 0, sizeof(c->w));
    *out = c;
    return VB_OK;
}
int vb_ctx_destroy(vb_ctx* ctx) {
    if (ctx) for (SampleGraph& g : ctx->graphs) g.destroy();
    delete ctx;
    return VB_OK;
}

}  // extern "C"
