// Caption-gate scores + Band-MoE router in ONE launch (gfx950, bf16 production mode).
//
// The folded caption gate (dit.hip, vocal2music_moe.py:119-151) was two launches: a grouped GEMM writing every token's attention
// scores against its clip's caption keys for all heads ([N][NS] fp32, NS = L * heads = 640: 30.8 MB per block evaluation at 8 clips)
// and the router kernel reading them back (softmax per head, contraction with the per-clip VW, Gumbel arg-max).  Here a workgroup
// owns 64 tokens of one clip and ALL NS score columns, so the scores never leave the CU:
//   * mainloop: [64 x K] x [NS x K]^T on the bf16 MFMA pipe, 4 waves, wave w owns all 64 rows x columns [w NS/4, (w+1) NS/4)
//     (2 x NJ accumulator tiles of 32 x 32); BK = 32, 3-stage LDS ring filled by global_load_lds (one stage = 64 + NS rows of 64 B =
//     45 KB at NS = 640), counted vmcnt, same lane-linear image + source-side XOR swizzle and the same ascending order of 16-deep
//     k-steps as gemm_bf16_glds_kernel - the scores are bit-identical to the two-launch path;
//   * epilogue: scores + per-clip bias go to LDS 32 rows at a time (the ring is free after the loop), and every wave runs
//     router_tokens() - the router kernel's own code - on 8 of those rows, reading the score rows from LDS instead of HBM.
// Grid: clips x ceil(T / 64) workgroups, the tiles of a clip on one XCD (its 983 KB of folded keys stay in that L2).
// The tile image, the DMA feed, the fragment reads and the MFMA step are gemm_tile.h's (BKT = 32, A = 64 token rows, B = NS key rows); the
// schedule - ring depth, counted waits, barrier - and the epilogue are this kernel's own.
#include "gemm_tile.h"
#include "router_dev.h"

#define SR_BM 64
#define SR_NST 3

struct ScoreRouterDev {
    const bf16_t* A; int lda;                               // token features [N][lda] (bf16)
    const bf16_t* Bm; int64_t b_clip_stride; int ldb;       // folded keys per clip: [Beff][NS][ldb]
    const float* bias; int bias_clip_stride;                // [Beff][NS]
    int K, Beff, tiles_per_clip;
    unsigned long long* trace;                              // tuning only (vbdbg_sr_trace): per block {start, loop end, end}
    RouterDev r;
};
static unsigned long long* g_sr_trace = nullptr;
extern "C" void vbdbg_sr_trace(void* buf) { g_sr_trace = static_cast<unsigned long long*>(buf); }   // tuning tool hook, not ABI

template <int NJ, int PP>
__global__ void __launch_bounds__(256) score_router_kernel(const ScoreRouterDev p) {
    constexpr int NS = NJ * 128;
    using Feed = TileFeed<SR_BM, NS, 32, 4>;          // a stage: 64 token rows, then NS key rows of 64 B; 1 + 2 NJ 1-KB DMA pieces per wave
    constexpr int STAGE = Feed::STAGE;
    constexpr int PITCH = NS + 4;                     // floats per staged score row
    static_assert(32 * PITCH * 4 <= SR_NST * STAGE, "score staging must fit in the ring");
    extern __shared__ __attribute__((aligned(16))) unsigned char sr_lds[];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int Lb = blockIdx.x, jx = Lb >> 3;
    const int clip = (jx / p.tiles_per_clip) * 8 + (Lb & 7);
    if (clip >= p.Beff) return;
    const int tile = jx % p.tiles_per_clip;
    const int T = p.r.T;
    const int row0 = clip * T + tile * SR_BM;
    const int rows_end = (clip + 1) * T;

    unsigned long long tq0 = 0, tq1 = 0;
    if (p.trace) tq0 = __builtin_amdgcn_s_memtime();
    const bf16_t* asrc[Feed::PA];
    const bf16_t* bsrc[Feed::PB];
    Feed::rows(asrc, p.A, p.lda, row0, rows_end, row0, false, wave, lane, [](int row) { return row; });
    Feed::rows(bsrc, p.Bm + (int64_t)clip * p.b_clip_stride, p.ldb, 0, NS, 0, false, wave, lane, [](int row) { return row; });
    auto issue = [&](int t) { Feed::issue(asrc, bsrc, wave, sr_lds + (t % SR_NST) * STAGE, t * 32, t * 32); };

    f32x16 acc[2][NJ];
    acc_zero(acc);

    const int KT = p.K / 32;
#pragma unroll
    for (int t = 0; t < SR_NST - 1; ++t)
        if (t < KT) issue(t);
    const int frow = lane & 31, fk = lane >> 5;
    for (int t = 0; t < KT; ++t) {
        if (t + 1 < KT) wait_vmcnt<Feed::LPT>();   // tile t landed, tile t + 1 may stay in flight
        else wait_vmcnt<0>();
        __builtin_amdgcn_s_barrier();                 // ... everywhere; everyone is done reading stage (t - 1) % NST
        if (t + SR_NST - 1 < KT) issue(t + SR_NST - 1);
        const unsigned char* As = sr_lds + (t % SR_NST) * STAGE;
        const unsigned char* Bs = As + Feed::ABYTES;
        bf16x8 af[2][2], bf[2][NJ];
        frag_load<2, NJ, 32>(As, Bs, 0, wave * 32 * NJ, 0, fk, frow, af[0], bf[0]);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            if (ks + 1 < 2) frag_load<2, NJ, 32>(As, Bs, 0, wave * 32 * NJ, ks + 1, fk, frow, af[(ks + 1) & 1], bf[(ks + 1) & 1]);
            __builtin_amdgcn_sched_barrier(0);
            mfma_step(af[ks & 1], bf[ks & 1], acc);
            __builtin_amdgcn_sched_barrier(0);
        }
    }

    if (p.trace) tq1 = __builtin_amdgcn_s_memtime();
    // ---- scores (+ bias) -> LDS, 32 token rows at a time; then the router on those rows
    float* stg = reinterpret_cast<float*>(sr_lds);
    const float* bias = p.bias + (int64_t)clip * p.bias_clip_stride;
    // (two explicit instances: a loop over `half` is not unrolled around the inlined router and would index acc[] dynamically -> scratch)
    auto do_half = [&](auto half_c) __attribute__((always_inline)) {
        constexpr int half = decltype(half_c)::value;
        __syncthreads();                              // ring reads (half 0) / the previous half's router reads are done
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int col = wave * 32 * NJ + j * 32 + q * 8 + fk * 4;
                const float4 b4 = *reinterpret_cast<const float4*>(bias + col);
                float4 v;
                v.x = acc[half][j][q * 4 + 0] + b4.x; v.y = acc[half][j][q * 4 + 1] + b4.y;
                v.z = acc[half][j][q * 4 + 2] + b4.z; v.w = acc[half][j][q * 4 + 3] + b4.w;
                *reinterpret_cast<float4*>(stg + frow * PITCH + col) = v;
            }
        __syncthreads();
#pragma unroll 1
        for (int gi = 0; gi < 2; ++gi) {
            const int lr = wave * 8 + gi * 4;         // first of this wave's 4 rows in the staged half
            const int n0 = row0 + half * 32 + lr;
            if (n0 < rows_end) router_tokens<PP, true, 4>(p.r, n0, rows_end, stg + lr * PITCH, PITCH, nullptr);
        }
    };
    do_half(std::integral_constant<int, 0>());
    do_half(std::integral_constant<int, 1>());
    if (p.trace && tid == 0) {
        __builtin_amdgcn_s_waitcnt(0);
        unsigned long long* tr = p.trace + (size_t)blockIdx.x * 4;
        tr[0] = tq0; tr[1] = tq1; tr[2] = __builtin_amdgcn_s_memtime(); tr[3] = 1;
    }
}

bool score_router_supported(int NS, int K, int E, int Hh) {
    const int nj = NS / 128;
    return NS % 128 == 0 && nj >= 4 && nj <= 6 && K % 32 == 0 && K >= 64 && E >= 2 && 2 * E + 2 <= 32 && Hh >= 1 && Hh <= 64 && (Hh & (Hh - 1)) == 0;
}

template <int NJ, int PP>
static void launch_sr(const ScoreRouterDev& d, dim3 grid, hipStream_t st) {
    constexpr size_t lds = (size_t)SR_NST * (SR_BM + NJ * 128) * 64;
    static OnceFlags attr;
    vb_set_max_lds_once(attr, reinterpret_cast<const void*>(score_router_kernel<NJ, PP>), (int)lds);
    hipLaunchKernelGGL((score_router_kernel<NJ, PP>), grid, dim3(256), lds, st, d);
}

int launch_score_router(const ScoreRouterArgs& a, hipStream_t st) {
    const int NS = a.r.NS, T = a.r.T;
    if (!score_router_supported(NS, a.K, a.r.E, a.r.Hh)) VB_FAIL(VB_E_INVALID, "score_router: NS=%d K=%d E=%d heads=%d unsupported", NS, a.K, a.r.E, a.r.Hh);
    if (a.lda % 8 || a.ldb % 8 || T < 1 || a.Beff < 1) VB_FAIL(VB_E_INVALID, "score_router: lda/ldb must be multiples of 8, T and clips positive");
    ScoreRouterDev d;
    d.A = a.A; d.lda = a.lda; d.Bm = a.Bm; d.b_clip_stride = (int64_t)NS * a.ldb; d.ldb = a.ldb; d.bias = a.bias; d.bias_clip_stride = NS;
    d.K = a.K; d.Beff = a.Beff; d.tiles_per_clip = cdiv(T, SR_BM); d.trace = g_sr_trace;
    d.r = a.r;
    d.r.N = a.Beff * T; d.r.D = a.K; d.r.sc = nullptr; d.r.lc_out = nullptr; d.r.cnt = nullptr; if (d.r.B <= 0) d.r.B = 1;
    const double n_tok = (double)a.Beff * T;
    ProfScope prof(0, 2.0 * n_tok * NS * a.K, 2.0 * (n_tok * a.K + (double)a.Beff * NS * a.K) + 16.0 * n_tok, st);
    const dim3 grid(d.tiles_per_clip * ((a.Beff + 7) / 8 * 8));
    const int nj = NS / 128;
    const bool pp4 = 2 * a.r.E + 2 <= 16;
#define VB_SR_CASE(NJ) case NJ: if (pp4) launch_sr<NJ, 4>(d, grid, st); else launch_sr<NJ, 2>(d, grid, st); break;
    switch (nj) {
        VB_SR_CASE(4)
        VB_SR_CASE(5)
        VB_SR_CASE(6)
        default: VB_FAIL(VB_E_INVALID, "score_router: NS=%d", NS);
    }
#undef VB_SR_CASE
    VB_CHECK_LAUNCH();
    return VB_OK;
}
