// Band-MoE routing (gfx950): the router kernel and its launch table (device side: router_dev.h), the per-clip constants of the folded
// caption gate, the stand-alone top-1 / noise kernels of the C-ABI unit wrappers, and the stable bucketing of tokens by routed expert
// or expert pair.  Called by dit.hip (router_bucket, precompute) and abi_units.hip.
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
int launch_router(const RouterDev& in, hipStream_t st) {
    RouterDev a = in;
    a.B = in.B > 0 ? in.B : 1; a.NS = in.sc ? in.NS : 0; a.Hh = in.sc ? in.Hh : 1;
    const int N = a.N, D = a.D, E = a.E, NS = in.NS, Hh = in.Hh;
    // tokens per wave: TWO (round 3; rounds 1-2: four).  Two tokens side by side amortise the noise generator and the arg-max, keep the
    // wave's registers at half of the four-token form and put twice the waves on a SIMD: same box, 12032 tokens 23.1 -> 20.0 us, whole
    // runs +1.2 % (8 clips, two streams), +2.9 % (E = 8, 32 clips), +1.8 % (4 x 120 s).  A launch that would not even put one workgroup on
    // every CU that way (one or two clips) takes one token per wave instead - the kernel is pure latency there (29 us at 1504 tokens).
    // The shape of configs/vocal2music.yaml (80 caption keys x 8 heads = 10 score columns per lane, E = 4) runs with both as compile-time
    // constants: 10 exponentials per token instead of 16 and - what matters - loads the compiler can hoist: under the run-time bound
    // `i < NS / 64` every one of the token's ten 16-byte gate-weight loads sat behind its own branch, ten L2 latencies in a row
    // (19.7 -> 15.2 us at 12032 tokens; VB_ROUTER_GENERIC: the run-time-bound form, same bits).  E = 8 keeps the run-time form: with
    // 20 weight registers per score column the hoisted form needs 220 VGPRs = two waves per SIMD and measured 0.7 % behind it (32 clips).
    const int forced = vb_tune().router_tpw;                  // VB_ROUTER_TPW=1|2|4 (tuning)
    const bool small = forced ? forced == 1 : cdiv(N, 4 * RT_TPW_MAX) < 256;
    const bool two = forced ? forced == 2 && 2 * E + 2 <= 32 : 2 * E + 2 <= 32;
    const dim3 grid(cdiv(N, 4 * (small ? 1 : (two ? 2 : RT_TPW_MAX))));
    const int pp = 2 * E + 2 <= 16 ? 4 : (2 * E + 2 <= 32 ? 2 : 1);
    if (a.sc) {
        // folded caption gate: logits from attention scores + per-clip VW (see router_tokens)
        if (NS % 64 || NS > 1024 || Hh < 1 || Hh > 64 || (Hh & (Hh - 1))) VB_FAIL(VB_E_INVALID, "router: NS=%d heads=%d unsupported", NS, Hh);
        const bool fixed = NS == 640 && !vb_tune().router_generic;
        if (fixed && E == 4) {
            if (small) launch_router_v<1, true, 1, 10, 4>(grid, 0, st, a);
            else if (two) launch_router_v<2, true, 2, 10, 4>(grid, 0, st, a);
            else launch_router_v<4, true, 4, 10, 4>(grid, 0, st, a);
        } else if (small) launch_router_v<1, true, 1>(grid, 0, st, a);
        else if (two) launch_router_v<2, true, 2>(grid, 0, st, a);
        else if (pp == 4) launch_router_v<4, true, 4>(grid, 0, st, a);
        else if (pp == 2) launch_router_v<2, true, 4>(grid, 0, st, a);
        else launch_router_v<1, true, 4>(grid, 0, st, a);
        VB_CHECK_LAUNCH();
        return VB_OK;
    }
    if ((E * D) % 4 != 0 || (size_t)E * D * sizeof(float) > 64 * 1024) VB_FAIL(VB_E_INVALID, "router: E*D=%d unsupported", E * D);
    const size_t lds = (size_t)E * D * sizeof(float);
    if (small) launch_router_v<1, false, 1>(grid, lds, st, a);
    else if (two) launch_router_v<2, false, 2>(grid, lds, st, a);
    else if (pp == 4) launch_router_v<4, false, 4>(grid, lds, st, a);
    else if (pp == 2) launch_router_v<2, false, 4>(grid, lds, st, a);
    else launch_router_v<1, false, 4>(grid, lds, st, a);
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
// `counts` lives right behind perm's 2N entries (perm buffers are sized 2N + nblk*2E + 64 by the engine).
// ---------------------------------------------------------------------------
#define BK_T 256
#define BK_G 32          // groups a launch can rank: 2E expert groups, or E*E (caption, acoustic) PAIR groups when E*E <= 16
// Pair mode (pair_off != null, E*E <= 16): the tokens are ranked ONCE, by their (caption expert c, acoustic expert a) pair.  Both
// expert-group orders fall out of the same E*E counts: the caption slots are the pair slots in c-major order (a caption group = E
// consecutive pair buckets), the acoustic slots the same buckets laid out a-major behind them - the order of the rows INSIDE an
// expert group is free (every row of a grouped GEMM is independent), so one rank per token serves perm (both halves), group_off and
// the single-launch w2 product (moe_w2_pair_kernel), whose caption-half rows are then simply its own row range:
//   perm[p] = token of pair slot p = caption slot p;  perm[pair_pa[p]] = the same token's acoustic slot;  pair_off[E*E + 1].
template <bool PAIRS>
__global__ void __launch_bounds__(BK_T) bucket_count_kernel(const int* __restrict__ ic, const int* __restrict__ ia, int N, int E, int G,
                                                           int* counts) {
    __shared__ int wc[4][BK_G];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = blockIdx.x * BK_T + tid;
    const int gc = n < N ? ic[n] : -1, ga = n < N ? E + ia[n] : -1;
    const int gp = n < N ? gc * E + (ga - E) : -1;
    for (int g = 0; g < G; ++g) {
        const unsigned long long m = __ballot(PAIRS ? (gp == g) : (g < E ? (gc == g) : (ga == g)));
        if (lane == 0) wc[wave][g] = __popcll(m);
    }
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
        int before_groups = 0;
        for (int g = 0; g < tid; ++g) before_groups += tot[g];
        base[tid] = before_groups + bef[tid];
        if constexpr (PAIRS) {
            // a-major order of the same buckets: everything with a smaller acoustic expert, then the same a with a smaller caption expert
            const int c = tid / E, a = tid - c * E;
            int beforeT = 0;
            for (int g = 0; g < G; ++g) {
                const int c2 = g / E, a2 = g - c2 * E;
                if (a2 < a || (a2 == a && c2 < c)) beforeT += tot[g];
            }
            base2[tid] = N + beforeT + bef[tid];
            if (blockIdx.x == 0) {
                pair_off[tid] = before_groups;
                if (tid == G - 1) pair_off[G] = before_groups + tot[tid];
                if (a == 0) group_off[c] = before_groups;                 // caption group c starts at its first pair bucket
                if (c == 0) group_off[E + a] = N + beforeT;               // acoustic group a starts at pair (0, a) in a-major order
                if (tid == 0) { group_off[E] = N; group_off[2 * E] = 2 * N; }
            }
        } else if (blockIdx.x == 0) {
            group_off[tid] = before_groups;
            if (tid == G - 1) group_off[G] = before_groups + tot[tid];
        }
    }
    const int n = blockIdx.x * BK_T + tid;
    const int gc = n < N ? ic[n] : -1, ga = n < N ? E + ia[n] : -1;
    const int gp = n < N ? gc * E + (ga - E) : -1;
    int rank_c = 0, rank_a = 0;
    const unsigned long long lower = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    for (int g = 0; g < G; ++g) {
        const unsigned long long m = __ballot(PAIRS ? (gp == g) : (g < E ? (gc == g) : (ga == g)));
        if (lane == 0) wc[wave][g] = __popcll(m);
        if constexpr (PAIRS) {
            if (g == gp) rank_c = __popcll(m & lower);
        } else {
            if (g == gc) rank_c = __popcll(m & lower);
            if (g == ga) rank_a = __popcll(m & lower);
        }
    }
    __syncthreads();
    if (n < N) {
        if constexpr (PAIRS) {
            int r = rank_c;
            for (int w = 0; w < wave; ++w) r += wc[w][gp];
            const int pc = base[gp] + r, pa = base2[gp] + r;
            perm[pc] = n;
            perm[pa] = n;
            pair_pa[pc] = pa;
        } else {
            int pc = base[gc] + rank_c, pa = base[ga] + rank_a;
            for (int w = 0; w < wave; ++w) { pc += wc[w][gc]; pa += wc[w][ga]; }
            perm[pc] = n;
            perm[pa] = n;
        }
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
    __shared__ int gbase[BK_G + 1];             // group start (pair mode: caption-major start of the pair bucket)
    __shared__ int gbase2[BK_G];                // pair mode: acoustic-major start of the pair bucket (slots [N, 2N))
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int G = PAIRS ? E * E : 2 * E;
    const int nch = (N + BKS_T - 1) / BKS_T;
    int gc[BKS_CH], ga[BKS_CH], rc[BKS_CH], ra[BKS_CH];
    const unsigned long long lower = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
#pragma unroll
    for (int ch = 0; ch < BKS_CH; ++ch) {
        gc[ch] = -1; ga[ch] = -1; rc[ch] = 0; ra[ch] = 0;
        if (ch < nch) {
            const int n = ch * BKS_T + tid;
            if (n < N) {
                if (PAIRS) { gc[ch] = ic[n] * E + ia[n]; } else { gc[ch] = ic[n]; ga[ch] = E + ia[n]; }
            }
            for (int g = 0; g < G; ++g) {
                const unsigned long long m = __ballot(PAIRS ? (gc[ch] == g) : (g < E ? (gc[ch] == g) : (ga[ch] == g)));
                if (lane == 0) cnt[ch * 16 + wave][g] = __popcll(m);
                if (g == gc[ch]) rc[ch] = __popcll(m & lower);
                if (!PAIRS && g == ga[ch]) ra[ch] = __popcll(m & lower);
            }
        }
    }
    __syncthreads();
    __shared__ int tot[BK_G];
    if (tid < G) {
        int run = 0;
        for (int i = 0; i < nch * 16; ++i) { const int c = cnt[i][tid]; cnt[i][tid] = run; run += c; }
        tot[tid] = run;
    }
    __syncthreads();
    if (tid < G) {
        // every group works out its own start from the totals (no serial section): caption-major prefix, and in pair mode the
        // acoustic-major start of the same bucket (everything with a smaller acoustic expert, then the same a with a smaller c)
        int before = 0;
        for (int g = 0; g < tid; ++g) before += tot[g];
        gbase[tid] = before;
        if (tid == G - 1) gbase[G] = before + tot[tid];
        if (PAIRS) {
            const int c = tid / E, a = tid - c * E;
            int b2 = 0;
            for (int g2 = 0; g2 < G; ++g2) {
                const int c2 = g2 / E, a2 = g2 - c2 * E;
                if (a2 < a || (a2 == a && c2 < c)) b2 += tot[g2];
            }
            gbase2[tid] = N + b2;
        }
    }
    __syncthreads();
    if (PAIRS) {
        if (tid <= G) pair_off[tid] = gbase[tid];
        if (tid < E) { group_off[tid] = gbase[tid * E]; group_off[E + tid] = gbase2[tid]; }      // caption group c = pair (c, 0); acoustic a = pair (0, a)
        if (tid == 0) { group_off[E] = N; group_off[2 * E] = 2 * N; }
    } else {
        if (tid <= G) group_off[tid] = gbase[tid];
    }
#pragma unroll
    for (int ch = 0; ch < BKS_CH; ++ch) {
        const int n = ch * BKS_T + tid;
        if (ch < nch && n < N) {
            if (PAIRS) {
                const int r = cnt[ch * 16 + wave][gc[ch]] + rc[ch];
                const int pc = gbase[gc[ch]] + r, pa = gbase2[gc[ch]] + r;
                perm[pc] = n;
                perm[pa] = n;
                pair_pa[pc] = pa;
            } else {
                perm[gbase[gc[ch]] + cnt[ch * 16 + wave][gc[ch]] + rc[ch]] = n;
                perm[gbase[ga[ch]] + cnt[ch * 16 + wave][ga[ch]] + ra[ch]] = n;
            }
        }
    }
}
static_assert(RT_CNT_BLOCK == BK_T, "the router counts per bucket block");
bool bucket_router_counts_ok(int N) { return N > BKS_T * BKS_CH; }
int bucket_counts_ints(int N) { return 2 * (cdiv(N, BK_T) * BK_G + 32); }
int* bucket_counts(int* perm, int N, int which) { return perm + 2 * (size_t)N + (size_t)which * (cdiv(N, BK_T) * BK_G + 32); }
int launch_bucket(const int* ic, const int* ia, int N, int E, int* group_off, int* perm, hipStream_t st, int* pair_off, int* pair_pa,
                  const int* counts_ready, int* counts_clear) {
    if (E > 16) VB_FAIL(VB_E_INVALID, "bucket: E=%d > 16", E);
    const bool pairs = pair_off != nullptr;
    if (pairs && E * E > 16) VB_FAIL(VB_E_INVALID, "bucket: pair mode needs E*E <= 16 (E=%d)", E);
    if (N <= BKS_T * BKS_CH) {
        if (counts_ready) VB_FAIL(VB_E_INVALID, "bucket: router-side counts belong to the two-kernel form (N > %d)", BKS_T * BKS_CH);
        if (pairs) hipLaunchKernelGGL(bucket_small_kernel<true>, dim3(1), dim3(BKS_T), 0, st, ic, ia, N, E, group_off, perm, pair_off, pair_pa);
        else hipLaunchKernelGGL(bucket_small_kernel<false>, dim3(1), dim3(BKS_T), 0, st, ic, ia, N, E, group_off, perm, nullptr, nullptr);
        VB_CHECK_LAUNCH();
        return VB_OK;
    }
    const int G = pairs ? E * E : 2 * E;
    const int nblk = cdiv(N, BK_T);
    int* counts = bucket_counts(perm, N, 0);     // scratch tail of the perm buffer (see bucket_scratch_ints)
    if (pairs) {
        if (!counts_ready) hipLaunchKernelGGL(bucket_count_kernel<true>, dim3(nblk), dim3(BK_T), 0, st, ic, ia, N, E, G, counts);
        hipLaunchKernelGGL(bucket_place_kernel<true>, dim3(nblk), dim3(BK_T), 0, st, ic, ia, N, E, G, counts_ready ? counts_ready : counts, nblk, group_off,
                           perm, pair_off, pair_pa, counts_clear);
    } else {
        if (!counts_ready) hipLaunchKernelGGL(bucket_count_kernel<false>, dim3(nblk), dim3(BK_T), 0, st, ic, ia, N, E, G, counts);
        hipLaunchKernelGGL(bucket_place_kernel<false>, dim3(nblk), dim3(BK_T), 0, st, ic, ia, N, E, G, counts_ready ? counts_ready : counts, nblk, group_off,
                           perm, nullptr, nullptr, counts_clear);
    }
    VB_CHECK_LAUNCH();
    return VB_OK;
}
int bucket_scratch_ints(int N, int E) { (void)E; return bucket_counts_ints(N) + 64; }
