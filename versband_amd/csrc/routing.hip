// Band-MoE routing (gfx950): the router kernel (device side: router_dev.h) with its launch table - router_form picks (tokens side by side,
// tokens per wave, fixed shape), launch_router_form maps that to one of the 13 instances -, the per-clip constants of the folded caption gate,
// the stand-alone top-1 / noise kernels of the C-ABI unit wrappers, and the stable bucketing of tokens by routed expert or expert pair: keys,
// ballot pass, starts, offsets and scatter as one helper each, the three bucket kernels as their schedules.
// Called by dit.hip (caption_gate_and_route, precompute) and abi_units.hip.
#include "kernels.h"
#include "router_dev.h"

template <int PP, bool SC, int RT_TPW = RT_TPW_MAX, int KPL = 16, int EE = 0>
__global__ void __launch_bounds__(256) router_kernel(const RouterDev a) {
    // gate weights staged once per block (every wave re-reading E*D floats per token through L1/L2 was the kernel's
    // whole cost); a wave then walks RT_TPW tokens
    extern __shared__ float rt_ws[];
    if constexpr (!SC) {
        for (int i = threadIdx.x * 4; i < a.E * a.D; i += 256 * 4) *reinterpret_cast<float4*>(rt_ws + i) = *reinterpret_cast<const float4*>(a.Wg + i);
        __syncthreads();
    }
    const int n0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * RT_TPW;
    if (n0 >= a.N) return;
    router_tokens<PP, SC, RT_TPW, KPL, EE>(a, n0, a.N, SC ? a.sc + (int64_t)n0 * a.NS : nullptr, a.NS, rt_ws);
}
template <int PP, bool SC, int TPW, int KPL = 16, int EE = 0>
static void launch_router_v(dim3 grid, size_t lds, hipStream_t st, const RouterDev& a) {
    hipLaunchKernelGGL((router_kernel<PP, SC, TPW, KPL, EE>), grid, dim3(256), lds, st, a);
}
// tokens per wave: TWO (round 3; rounds 1-2: four).  Two tokens side by side amortise the noise generator and the arg-max, keep the
// wave's registers at half of the four-token form and put twice the waves on a SIMD: same box, 12032 tokens 23.1 -> 20.0 us, whole
// runs +1.2 % (8 clips, two streams), +2.9 % (E = 8, 32 clips), +1.8 % (4 x 120 s).  A launch that would not even put one workgroup on
// every CU that way (one or two clips) takes one token per wave instead - the kernel is pure latency there (29 us at 1504 tokens).
// The shape of configs/vocal2music.yaml (80 caption keys x 8 heads = 10 score columns per lane, E = 4) runs with both as compile-time
// constants: 10 exponentials per token instead of 16 and - what matters - loads the compiler can hoist: under the run-time bound
// `i < NS / 64` every one of the token's ten 16-byte gate-weight loads sat behind its own branch, ten L2 latencies in a row
// (19.7 -> 15.2 us at 12032 tokens; VB_ROUTER_GENERIC: the run-time-bound form, same bits).  E = 8 keeps the run-time form: with
// 20 weight registers per score column the hoisted form needs 220 VGPRs = two waves per SIMD and measured 0.7 % behind it (32 clips).
struct RouterForm { int pp, tpw; bool fixed; };      // tokens side by side, tokens per wave, KPL = 10 / EE = 4 as constants
static RouterForm router_form(int N, int E, int NS, bool sc, const VbTune& tune) {
    const int forced = tune.router_tpw;                       // VB_ROUTER_TPW=1|2|4 (tuning)
    const bool small = forced ? forced == 1 : cdiv(N, 4 * RT_TPW_MAX) < 256;
    const bool two = forced ? forced == 2 && 2 * E + 2 <= 32 : 2 * E + 2 <= 32;
    const bool fixed = sc && NS == 640 && E == 4 && !tune.router_generic;
    if (small) return {1, 1, fixed};
    if (two) return {2, 2, fixed};
    return {2 * E + 2 <= 16 ? 4 : (2 * E + 2 <= 32 ? 2 : 1), RT_TPW_MAX, fixed};
}
// form -> instance: (PP, TPW) in {(1,1), (2,2), (4,4), (2,4), (1,4)} for both SC, + the first three with KPL = 10, EE = 4 for SC (13 in all)
static_assert(RT_TPW_MAX == 4, "the table below takes every tpw other than 1 and 2 as the four-token form");
template <bool SC>
static void launch_router_form(const RouterForm& f, dim3 grid, size_t lds, hipStream_t st, const RouterDev& a) {
    if constexpr (SC) {
        if (f.fixed) {       // (E = 4: pp is 4 wherever tpw is)
            if (f.tpw == 1) launch_router_v<1, true, 1, 10, 4>(grid, lds, st, a);
            else if (f.tpw == 2) launch_router_v<2, true, 2, 10, 4>(grid, lds, st, a);
            else launch_router_v<4, true, 4, 10, 4>(grid, lds, st, a);
            return;
        }
    }
    if (f.tpw == 1) launch_router_v<1, SC, 1>(grid, lds, st, a);
    else if (f.tpw == 2) launch_router_v<2, SC, 2>(grid, lds, st, a);
    else if (f.pp == 4) launch_router_v<4, SC, 4>(grid, lds, st, a);
    else if (f.pp == 2) launch_router_v<2, SC, 4>(grid, lds, st, a);
    else launch_router_v<1, SC, 4>(grid, lds, st, a);
}
int launch_router(const RouterDev& in, hipStream_t st) {
    RouterDev a = in;
    a.B = in.B > 0 ? in.B : 1; a.NS = in.sc ? in.NS : 0; a.Hh = in.sc ? in.Hh : 1;
    const int N = a.N, D = a.D, E = a.E, NS = in.NS, Hh = in.Hh;
    const RouterForm f = router_form(N, E, NS, a.sc != nullptr, vb_tune());
    const dim3 grid(cdiv(N, 4 * f.tpw));
    if (a.sc) {
        // folded caption gate: logits from attention scores + per-clip VW (see router_tokens)
        if (NS % 64 || NS > 1024 || Hh < 1 || Hh > 64 || (Hh & (Hh - 1))) VB_FAIL(VB_E_INVALID, "router: NS=%d heads=%d unsupported", NS, Hh);
        launch_router_form<true>(f, grid, 0, st, a);
    } else {
        if ((E * D) % 4 != 0 || (size_t)E * D * sizeof(float) > 64 * 1024) VB_FAIL(VB_E_INVALID, "router: E*D=%d unsupported", E * D);
        launch_router_form<false>(f, grid, (size_t)E * D * sizeof(float), st, a);
    }
    VB_CHECK_LAUNCH();
    return VB_OK;
}

// Per-clip constants of the folded caption gate (once per clip and block):
//   cbias[b][j*Hh + h] = sum_d bq_s[h*hd + d] * Kc[b][j][h*hd + d]                      (q-bias part of the scores)
//   VW[b][j*Hh + h][e] = sum_d Vc^T[b][h][d][j] * Wcg[e][h*hd + d]                      (values pre-contracted with the gate rows)
__global__ void __launch_bounds__(256) gate_fold_kernel(Planes kc, Planes vct, const float* __restrict__ bq_s, const float* __restrict__ wcg,
                                                       int Beff, int L, int Lpad, int Hh, int hd, int E, float* cbias, float* vw) {
    const int D = Hh * hd;
    const int total = Beff * L * Hh;
    for (int id = blockIdx.x * 256 + threadIdx.x; id < total; id += gridDim.x * 256) {
        const int h = id % Hh, bj = id / Hh;
        const int j = bj % L, b = bj / L;
        const bf16_t* kr = kc.p + ((int64_t)(b * L + j)) * D + h * hd;
        float cb = 0.f;
        for (int d = 0; d < hd; ++d) {
            float kv = bf2f(kr[d]);
            if (kc.np == 2) kv += bf2f(kr[kc.plane + d]);
            cb += bq_s[h * hd + d] * kv;
        }
        cbias[id] = cb;
        const bf16_t* vr = vct.p + ((int64_t)(b * Hh + h) * hd) * Lpad + j;
        for (int e = 0; e < E; ++e) {
            float acc = 0.f;
            for (int d = 0; d < hd; ++d) {
                float vv = bf2f(vr[(int64_t)d * Lpad]);
                if (vct.np == 2) vv += bf2f(vr[vct.plane + (int64_t)d * Lpad]);
                acc += vv * wcg[(int64_t)e * D + h * hd + d];
            }
            vw[(int64_t)id * E + e] = acc;
        }
    }
}
int launch_gate_fold(Planes kc, Planes vct, const float* bq_s, const float* wcg, int Beff, int L, int Lpad, int Hh, int hd, int E,
                     float* cbias, float* vw, hipStream_t st) {
    hipLaunchKernelGGL(gate_fold_kernel, dim3(cdiv(Beff * L * Hh, 256)), dim3(256), 0, st, kc, vct, bq_s, wcg, Beff, L, Lpad, Hh, hd, E, cbias, vw);
    VB_CHECK_LAUNCH();
    return VB_OK;
}
__global__ void iota_mul_kernel(int* out, int n, int mul) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = i * mul;
}
int launch_iota_mul(int* out, int n, int mul, hipStream_t st) {
    hipLaunchKernelGGL(iota_mul_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, out, n, mul);
    VB_CHECK_LAUNCH();
    return VB_OK;
}

// idx[n] = first argmax_e (logits[n][e] + gumbel[n][e])   (hard Gumbel-softmax, :81-93)
__global__ void router_top1_kernel(const float* __restrict__ logits, const float* __restrict__ gum, int N, int E, int* idx) {
    int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    float best = -INFINITY; int bi = 0;
    for (int e = 0; e < E; ++e) {
        float z = logits[(int64_t)n * E + e] + gum[(int64_t)n * E + e];
        if (z > best) { best = z; bi = e; }
    }
    idx[n] = bi;
}
int launch_router_top1(const float* logits, const float* gumbel, int N, int E, int* idx, hipStream_t st) {
    hipLaunchKernelGGL(router_top1_kernel, dim3(cdiv(N, 256)), dim3(256), 0, st, logits, gumbel, N, E, idx);
    VB_CHECK_LAUNCH();
    return VB_OK;
}

// element (row n = (branch*B + b)*T + t, e) of stream (seed, clip_base + b, nfe, branch, block, gate)
// (vb_fill_gumbel only: not on the sampler's path, whose router draws inside router_phase_b - so it takes no per-row clip ids)
__global__ void fill_gumbel_kernel(float* out, int B, int n_branch, int T, int width, uint64_t seed, int64_t clip_base,
                                   int nfe_base, const int* step, int block, int gate) {
    const int64_t n_el = (int64_t)n_branch * B * T * width;
    const int nfe = nfe_base + (step ? *step : 0);
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < n_el; i += stride) {
        int64_t row = i / width; int e = (int)(i - row * width);
        int bb = (int)(row / T), t = (int)(row - (int64_t)bb * T);
        int branch = bb / B, b = bb - branch * B;
        out[i] = gumbel_draw(seed, clip_base + b, nfe, branch, block, gate, t, width, e);
    }
}
int launch_fill_gumbel(float* out, int B, int n_branch, int T, int width, uint64_t seed, int64_t clip_base, int nfe_base,
                       const int* step, int block, int gate, hipStream_t st) {
    int64_t n = (int64_t)n_branch * B * T * width;
    int blocks = (int)((n + 255) / 256);
    if (blocks > 2048) blocks = 2048;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(fill_gumbel_kernel, dim3(blocks), dim3(256), 0, st, out, B, n_branch, T, width, seed, clip_base, nfe_base, step,
                       block, gate);
    VB_CHECK_LAUNCH();
    return VB_OK;
}

// ---------------------------------------------------------------------------
// Stable bucketing of tokens by routed expert: slots [0,N) caption groups, [N,2N) acoustic groups;
// perm[slot] = token, group_off[2E+1].  Two multi-block kernels (deterministic, ascending token order inside a group):
//   bucket_count : per 256-token block, per group counts (wave ballots)       -> counts[nblk][2E]
//   bucket_place : every block re-derives its bases from the small counts table, ranks its tokens with ballots and
//                  writes perm; block 0 also writes group_off.
// and, for small token counts, both in one workgroup (bucket_small).  `counts` lives right behind perm's 2N entries (perm buffers
// are sized 2N + nblk*2E + 64 by the engine).
// ---------------------------------------------------------------------------
#define BK_T 256
#define BK_G 32          // groups a launch can rank: 2E expert groups, or E*E (caption, acoustic) PAIR groups when E*E <= 16
// Pair mode (pair_off != null, E*E <= 16): the tokens are ranked ONCE, by their (caption expert c, acoustic expert a) pair.  Both
// expert-group orders fall out of the same E*E counts: the caption slots are the pair slots in c-major order (a caption group = E
// consecutive pair buckets), the acoustic slots the same buckets laid out a-major behind them - the order of the rows INSIDE an
// expert group is free (every row of a grouped GEMM is independent), so one rank per token serves perm (both halves), group_off and
// the single-launch w2 product (moe_w2_pair_kernel), whose caption-half rows are then simply its own row range:
//   perm[p] = token of pair slot p = caption slot p;  perm[pair_pa[p]] = the same token's acoustic slot;  pair_off[E*E + 1].
//
// The pieces of the algorithm, each once; the kernels below are their schedules (what is counted where, and every barrier).
// Keys of token n: in pair mode ONE key, c * E + a (ka stays -1); otherwise the caption group c and the acoustic group E + a.  A token at
// or past N gets -1, which matches no group - so every lane runs the ballot pass, whatever its token.
template <bool PAIRS>
__device__ __forceinline__ void bucket_keys(const int* __restrict__ ic, const int* __restrict__ ia, int n, int N, int E, int& kc, int& ka) {
    kc = -1; ka = -1;
    if (n < N) {
        if constexpr (PAIRS) kc = ic[n] * E + ia[n];
        else { kc = ic[n]; ka = E + ia[n]; }
    }
}
// Ballot pass over the G groups: lane 0 stores the wave's count of every group into wc[0..G); -> rc / ra = how many lower lanes of the wave
// hold the same key (the stable rank inside the wave).  Wave-wide ballots: EVERY lane of EVERY wave calls this, never under `n < N`.
template <bool PAIRS>
__device__ __forceinline__ void bucket_ballots(int kc, int ka, int E, int G, int lane, int* wc, int& rc, int& ra) {
    const unsigned long long lower = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    rc = 0; ra = 0;
    for (int g = 0; g < G; ++g) {
        const unsigned long long m = __ballot(PAIRS ? (kc == g) : (g < E ? (kc == g) : (ka == g)));
        if (lane == 0) wc[g] = __popcll(m);
        if (g == kc) rc = __popcll(m & lower);
        if (!PAIRS && g == ka) ra = __popcll(m & lower);
    }
}
// Starts of group g from the per-group totals (no serial section: every group works out its own): s = everything in a group before it
// (pair mode: the caption-major order of the pair buckets); pair mode also s2, the start of the same bucket in acoustic-major order behind
// the N caption slots - everything with a smaller acoustic expert, then the same a with a smaller caption expert.
template <bool PAIRS>
__device__ __forceinline__ void bucket_starts(const int* tot, int g, int E, int G, int N, int& s, int& s2) {
    s = 0; s2 = 0;
    for (int i = 0; i < g; ++i) s += tot[i];
    if constexpr (PAIRS) {
        const int c = g / E, a = g - c * E;
        int before = 0;
        for (int i = 0; i < G; ++i) {
            const int c2 = i / E, a2 = i - c2 * E;
            if (a2 < a || (a2 == a && c2 < c)) before += tot[i];
        }
        s2 = N + before;
    }
}
// group_off (and pair_off) from those starts, by the thread of group g < G; end = s + the group's total
template <bool PAIRS>
__device__ __forceinline__ void bucket_offsets(int g, int s, int s2, int end, int E, int G, int N, int* group_off, int* pair_off) {
    if constexpr (PAIRS) {
        const int c = g / E, a = g - c * E;
        pair_off[g] = s;
        if (g == G - 1) pair_off[G] = end;
        if (a == 0) group_off[c] = s;                     // caption group c starts at its first pair bucket
        if (c == 0) group_off[E + a] = s2;                // acoustic group a starts at pair (0, a) in a-major order
        if (g == 0) { group_off[E] = N; group_off[2 * E] = 2 * N; }
    } else {
        group_off[g] = s;
        if (g == G - 1) group_off[G] = end;
    }
}
// token n into its slots: rc / ra = its rank among the tokens of its key(s) that the bases do not already count
template <bool PAIRS>
__device__ __forceinline__ void bucket_scatter(int n, int kc, int ka, int rc, int ra, const int* base, const int* base2, int* perm, int* pair_pa) {
    if constexpr (PAIRS) {
        const int pc = base[kc] + rc, pa = base2[kc] + rc;
        perm[pc] = n;
        perm[pa] = n;
        pair_pa[pc] = pa;
    } else {
        perm[base[kc] + rc] = n;
        perm[base[ka] + ra] = n;
    }
}

template <bool PAIRS>
__global__ void __launch_bounds__(BK_T) bucket_count_kernel(const int* __restrict__ ic, const int* __restrict__ ia, int N, int E, int G,
                                                           int* counts) {
    __shared__ int wc[4][BK_G];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int kc, ka, rc, ra;       // (the ranks are not used here)
    bucket_keys<PAIRS>(ic, ia, blockIdx.x * BK_T + tid, N, E, kc, ka);
    bucket_ballots<PAIRS>(kc, ka, E, G, lane, wc[wave], rc, ra);
    __syncthreads();
    if (tid < G) counts[blockIdx.x * G + tid] = wc[0][tid] + wc[1][tid] + wc[2][tid] + wc[3][tid];
}
template <bool PAIRS>
__global__ void __launch_bounds__(BK_T) bucket_place_kernel(const int* __restrict__ ic, const int* __restrict__ ia, int N, int E, int G,
                                                           const int* __restrict__ counts, int nblk, int* group_off, int* perm,
                                                           int* pair_off, int* pair_pa, int* counts_clear) {
    // (round 5) this block's row of the OTHER count table: the next router launch adds into it
    if (counts_clear && threadIdx.x < G) counts_clear[blockIdx.x * G + threadIdx.x] = 0;
    __shared__ int base[BK_G];        // slot of this block's first token of every group (pair mode: caption slot)
    __shared__ int base2[BK_G];       // pair mode: acoustic slot of this block's first token of every pair
    __shared__ int wc[4][BK_G];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // group start = sum of all earlier groups' totals; + this group's tokens in earlier blocks.  The counts table is
    // summed by the whole block (thread = (row-of-counts, group)), not by G serial threads.
    __shared__ int tot[BK_G], bef[BK_G];
    if (tid < BK_G) { tot[tid] = 0; bef[tid] = 0; }
    __syncthreads();
    {
        const int g = tid % G;
        int t = 0, bf = 0;
        for (int b = tid / G; b < nblk; b += BK_T / G) {
            const int cnt = counts[b * G + g];
            t += cnt;
            if (b < (int)blockIdx.x) bf += cnt;
        }
        if (tid < (BK_T / G) * G) { atomicAdd(&tot[g], t); atomicAdd(&bef[g], bf); }
    }
    __syncthreads();
    if (tid < G) {
        int s, s2;
        bucket_starts<PAIRS>(tot, tid, E, G, N, s, s2);
        base[tid] = s + bef[tid];
        if constexpr (PAIRS) base2[tid] = s2 + bef[tid];
        if (blockIdx.x == 0) bucket_offsets<PAIRS>(tid, s, s2, s + tot[tid], E, G, N, group_off, pair_off);
    }
    const int n = blockIdx.x * BK_T + tid;
    int kc, ka, rc, ra;
    bucket_keys<PAIRS>(ic, ia, n, N, E, kc, ka);
    bucket_ballots<PAIRS>(kc, ka, E, G, lane, wc[wave], rc, ra);
    __syncthreads();
    if (n < N) {
        for (int w = 0; w < wave; ++w) {      // + the lower waves of the block
            rc += wc[w][kc];
            if constexpr (!PAIRS) ra += wc[w][ka];
        }
        bucket_scatter<PAIRS>(n, kc, ka, rc, ra, base, base2, perm, pair_pa);
    }
}
// (Round 3, measured and removed: count + place as ONE launch at up to 64 blocks, every block re-deriving all chunks' counts itself
//  instead of reading the table of a first launch: correct, bit-identical - and 62.7 us against 4.7 + 6.3, because the walk over the 47
//  chunks is 47 dependent L2 round trips per block.)
// Small token counts (one or two clips: the reference's serving shape, scripts/test_final.py:357): count + place in ONE launch of one
// 1024-thread workgroup - at 1504 tokens the two multi-block kernels above are two ~4.6-us launch floors for 6 blocks of work.
// Same result, bit for bit (stable: ascending token order inside a group).
#define BKS_T 1024
#define BKS_CH 4            // chunks of 1024 tokens: N <= 4096
template <bool PAIRS>
__global__ void __launch_bounds__(BKS_T) bucket_small_kernel(const int* __restrict__ ic, const int* __restrict__ ia, int N, int E,
                                                            int* group_off, int* perm, int* pair_off, int* pair_pa) {
    __shared__ int cnt[BKS_CH * 16][BK_G];      // [chunk * 16 + wave][group]: count, then exclusive prefix inside the group
    __shared__ int gbase[BK_G];                 // group start (pair mode: caption-major start of the pair bucket)
    __shared__ int gbase2[BK_G];                // pair mode: acoustic-major start of the pair bucket (slots [N, 2N))
    __shared__ int tot[BK_G];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int G = PAIRS ? E * E : 2 * E;
    const int nch = (N + BKS_T - 1) / BKS_T;
    int kc[BKS_CH], ka[BKS_CH], rc[BKS_CH], ra[BKS_CH];
#pragma unroll
    for (int ch = 0; ch < BKS_CH; ++ch) {
        kc[ch] = -1; ka[ch] = -1; rc[ch] = 0; ra[ch] = 0;      // (for the chunks past the end, which the block skips as one: nch is uniform)
        if (ch < nch) {
            bucket_keys<PAIRS>(ic, ia, ch * BKS_T + tid, N, E, kc[ch], ka[ch]);
            bucket_ballots<PAIRS>(kc[ch], ka[ch], E, G, lane, cnt[ch * 16 + wave], rc[ch], ra[ch]);
        }
    }
    __syncthreads();
    if (tid < G) {
        int run = 0;
        for (int i = 0; i < nch * 16; ++i) { const int c = cnt[i][tid]; cnt[i][tid] = run; run += c; }
        tot[tid] = run;
    }
    __syncthreads();
    if (tid < G) {
        int s, s2;
        bucket_starts<PAIRS>(tot, tid, E, G, N, s, s2);
        gbase[tid] = s;
        if constexpr (PAIRS) gbase2[tid] = s2;
        bucket_offsets<PAIRS>(tid, s, s2, s + tot[tid], E, G, N, group_off, pair_off);
    }
    __syncthreads();
#pragma unroll
    for (int ch = 0; ch < BKS_CH; ++ch) {
        const int n = ch * BKS_T + tid;
        if (ch < nch && n < N) {      // + the chunks and waves before this one
            const int* before = cnt[ch * 16 + wave];
            rc[ch] += before[kc[ch]];
            if constexpr (!PAIRS) ra[ch] += before[ka[ch]];
            bucket_scatter<PAIRS>(n, kc[ch], ka[ch], rc[ch], ra[ch], gbase, gbase2, perm, pair_pa);
        }
    }
}
static_assert(RT_CNT_BLOCK == BK_T, "the router counts per bucket block");
bool bucket_router_counts_ok(int N) { return N > BKS_T * BKS_CH; }
int bucket_counts_ints(int N) { return 2 * (cdiv(N, BK_T) * BK_G + 32); }
int* bucket_counts(int* perm, int N, int which) { return perm + 2 * (size_t)N + (size_t)which * (cdiv(N, BK_T) * BK_G + 32); }
template <bool PAIRS>
static void launch_bucket_t(const int* ic, const int* ia, int N, int E, int* group_off, int* perm, hipStream_t st, int* pair_off, int* pair_pa,
                            const int* counts_ready, int* counts_clear) {
    if (N <= BKS_T * BKS_CH) {
        hipLaunchKernelGGL(bucket_small_kernel<PAIRS>, dim3(1), dim3(BKS_T), 0, st, ic, ia, N, E, group_off, perm, pair_off, pair_pa);
        return;
    }
    const int G = PAIRS ? E * E : 2 * E;
    const int nblk = cdiv(N, BK_T);
    int* counts = bucket_counts(perm, N, 0);     // scratch tail of the perm buffer (see bucket_scratch_ints)
    if (!counts_ready) hipLaunchKernelGGL(bucket_count_kernel<PAIRS>, dim3(nblk), dim3(BK_T), 0, st, ic, ia, N, E, G, counts);
    hipLaunchKernelGGL(bucket_place_kernel<PAIRS>, dim3(nblk), dim3(BK_T), 0, st, ic, ia, N, E, G, counts_ready ? counts_ready : counts, nblk, group_off,
                       perm, pair_off, pair_pa, counts_clear);
}
int launch_bucket(const int* ic, const int* ia, int N, int E, int* group_off, int* perm, hipStream_t st, int* pair_off, int* pair_pa,
                  const int* counts_ready, int* counts_clear) {
    if (E > 16) VB_FAIL(VB_E_INVALID, "bucket: E=%d > 16", E);
    const bool pairs = pair_off != nullptr;
    if (pairs && E * E > 16) VB_FAIL(VB_E_INVALID, "bucket: pair mode needs E*E <= 16 (E=%d)", E);
    if (N <= BKS_T * BKS_CH && counts_ready) VB_FAIL(VB_E_INVALID, "bucket: router-side counts belong to the two-kernel form (N > %d)", BKS_T * BKS_CH);
    if (pairs) launch_bucket_t<true>(ic, ia, N, E, group_off, perm, st, pair_off, pair_pa, counts_ready, counts_clear);
    else launch_bucket_t<false>(ic, ia, N, E, group_off, perm, st, nullptr, nullptr, counts_ready, counts_clear);
    VB_CHECK_LAUNCH();
    return VB_OK;
}
int bucket_scratch_ints(int N, int E) { (void)E; return bucket_counts_ints(N) + 64; }
