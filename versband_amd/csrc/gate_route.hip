// Caption gate in ONE launch, lane-local (gfx950, bf16 production mode, 80 caption keys x 8 heads, 4 experts, hidden 768):
// scores, per-head softmax, value/gate contraction and the Band-MoE routing decisions of 64 tokens per workgroup.  Replaces the grouped
// score GEMM (12032 x 640 x 768 -> 31 MB of fp32 scores written) + router_kernel (the same 31 MB read back, one wave per two tokens,
// every max / sum / logit a wave-wide butterfly) of dit.hip: caption_gate_and_route; bit-identical to them (see "Bits").
//
// Layout.  A workgroup owns 64 tokens of one clip x all NS = 640 score columns ns = key * 8 + head.  Its 4 waves split as
// (th = wave & 1: tokens 32 th ..) x (c = wave >> 1: the keys of parity c).  The MFMA is issued "swapped" (folded keys Mf as its A
// operand, gemm_tile.h), so a lane of a 32 x 32 accumulator owns ONE token (lane & 31) and the rows 8 q + 4 fk + r (fk = lane >> 5).
// The Mf rows are PERMUTED on their way into LDS (the DMA's source rows, free) so that row 8 q + 4 fk + r of wave (., c)'s tile u is
//     key = 8 u + 2 q + c,   head = 4 fk + r            (u = 0..9, q = 0..3, r = 0..3)
// i.e. in the router's terms (key = kr + 8 i: kr = key residue, i = 0..9) tile u IS step i and q picks kr = 2 q + c.  A lane then holds,
// for its token and four whole heads, 4 of the 8 key residues with all ten steps each: every sequential chain of router_tokens is
// lane-local, the other four residues sit in the same lane of wave ^ 2.
//
// Main loop.  The token operand stays in registers (48 k-steps x 16 B per lane = 192 VGPRs, as band_ffn_kernel keeps y); only Mf goes
// through LDS: loads of [128 rows x 64 k] = 16 KB (4 DMA pieces per wave, full 128-B lines), load q = (k-tile q / 5, row chunk q % 5:
// the tiles u = 2 (q % 5), + 1 of both parities), an 8-slot ring with seven loads (112 KB) in flight behind the one being multiplied,
// counted vmcnt, one barrier per load; the fragments of load q + 1 are read in front of the MFMAs of load q.  k ascends in 16-deep steps
// of v_mfma_f32_32x32x16_bf16 for every accumulator - the order of every other route, so the score bits are the GEMM's.
// LDS reads: a wave reads its parity's half of every load (8 KB of 16), all four waves together 2 x the 0.98 MB of Mf = 1.97 MB per
// workgroup - 6.4 us at 128 B/clk/CU, the same as the 6.4 us of MFMA work at peak; the DMA stream (0.98 MB at ~110 GB/s per CU = 8.9 us)
// is the floor of the loop.
//
// Bits.  router_tokens<., true, ., 10, 4> (router_dev.h) computes, per token and head h, with key = kr + 8 i on lane kr * 8 + h:
//     m      = max over all 80 keys                                   (exact whatever the order)
//     p[key] = __expf(score[key] - m)
//     l[kr]  = (((0 + p[kr]) + p[kr + 8]) + ...) + p[kr + 72]         sequential over i
//     L      = ((l0 + l1) + (l2 + l3)) + ((l4 + l5) + (l6 + l7))      butterfly lane ^ 8, ^ 16, ^ 32
//     x[kr][h][e] = (fma chain over i of p[kr + 8 i] * VW[key][h][e], from 0) * (1 / L)
//     logit[e] = reduce_logits: pairs lane ^ 32 (kr ^ 4), ^ 16 (kr ^ 2), ^ 8 (kr ^ 1), then ^ 4 (h ^ 4), ^ 2 (h ^ 2), ^ 1 (h ^ 1):
//         a1[kr & 3][h] = x[kr] + x[kr ^ 4];  a2[kr & 1][h] = a1[kr & 3] + a1[(kr & 3) ^ 2];  a3[h] = a2[0] + a2[1];
//         b[h & 3] = a3[h] + a3[h ^ 4];  (b0 + b2) + (b1 + b3)
// (IEEE addition is commutative, so which lane of a pair adds does not matter; only the tree does.)  Here the chains over i run over the
// tiles u in a lane; l's first pair level (kr ^ 1) and the logits' third (kr ^ 1) cross the two parity waves - through LDS -, the logits'
// first two levels (q ^ 2, q ^ 1) are lane-local, the head levels are summed by one thread per (token, expert) from LDS in the order above.
// The rest - bias, Gumbel draws, first-maximum arg-max, high-level gate, ic / ia / mc / ma, the count table - is router_phase_b itself,
// fed the four logits per token from LDS.
#include "gemm_tile.h"
#include "router_dev.h"

constexpr int GR_TOK = 64, GR_NS = 640, GR_K = 768, GR_E = 4;
constexpr int GR_NSLOT = 8, GR_SLOT = 128 * 128;                 // ring slots; a load = 128 Mf rows x 64 k bf16
constexpr int GR_NRC = GR_NS / 128, GR_KT = GR_K / 64, GR_NLOAD = GR_KT * GR_NRC, GR_NT = GR_NS / 64;      // 5 row chunks x 12 k-tiles = 60 loads; 10 tiles per wave
constexpr int GR_RING = GR_NSLOT * GR_SLOT;                      // 128 KB; after the loop: the exchange buffers below
constexpr int GR_VW = GR_NS * GR_E * 4, GR_CB = GR_NS * 4;       // the clip's VW and score bias, staged once
constexpr int GR_LDS = GR_RING + GR_VW + GR_CB;
// exchange buffers inside the (then free) ring: partial maxima [4 waves][64 lanes][4], partial sums [4][64][16], a2 [64 tokens][68], logits [64][4]
constexpr int GR_MX = 0, GR_LX = 4096, GR_AX = 32768, GR_LG = 65536, GR_AXP = 68;
static_assert(GR_LX + 4 * 64 * 16 * 4 <= GR_AX && GR_AX + GR_TOK * GR_AXP * 4 <= GR_LG && GR_LG + GR_TOK * GR_E * 4 <= GR_RING, "exchange buffers");
static_assert(GR_LDS <= 160 * 1024, "LDS of a CU");

struct GateRouteDev {
    const bf16_t* A; int lda;                               // token features [N][lda] (bf16)
    const bf16_t* Mf; int64_t mf_clip_stride; int ldb;      // folded keys per clip: [Beff][NS][ldb]
    const float* bias;                                      // [Beff][NS]
    int Beff, tiles_per_clip;
    RouterDev r;                                            // Wg = VW [Beff][NS][E]
};

__global__ void __launch_bounds__(256) gate_route_kernel(const GateRouteDev p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char gl[];
    unsigned char* ring = gl;
    float* vws = reinterpret_cast<float*>(gl + GR_RING);
    float* cbs = reinterpret_cast<float*>(gl + GR_RING + GR_VW);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int th = wave & 1, c = wave >> 1;
    const int frow = lane & 31, fk = lane >> 5;
    // XCD x = block & 7 serves the clips x, x + 8, ...: all tiles of a clip on one XCD, its 983 KB of folded keys in that L2
    const int Lb = blockIdx.x, jx = Lb >> 3;
    const int clip = (jx / p.tiles_per_clip) * 8 + (Lb & 7);
    if (clip >= p.Beff) return;
    const int T = p.r.T;
    const int row0 = clip * T + (jx % p.tiles_per_clip) * GR_TOK;
    const int rows_end = (clip + 1) * T;

    // the clip's VW (10 KB: ten DMA pieces, in front of the ring's loads - whatever is issued first has landed when load 0 has) and score
    // bias (160 float4 through registers, written to LDS behind the ring's first loads)
    const float4* vwg = reinterpret_cast<const float4*>(p.r.Wg + (int64_t)clip * GR_NS * GR_E);
    const float4* cbg = reinterpret_cast<const float4*>(p.bias + (int64_t)clip * GR_NS);
    for (int j = wave; j < GR_VW / 1024; j += 4)
        __builtin_amdgcn_global_load_lds((glb_ptr_t)(vwg + j * 64 + lane), (lds_ptr_t)(gl + GR_RING + j * 1024), 16, 0, 0);
    float4 cr = make_float4(0.f, 0.f, 0.f, 0.f);
    if (tid < GR_NS / 4) cr = cbg[tid];
    // the register-resident token fragments: rows past the clip's end read the tile's first row and are never stored
    bf16x8 ay[GR_K / 16];
    {
        int row = row0 + th * 32 + frow;
        if (row >= rows_end) row = row0;
        const bf16_t* src = p.A + (int64_t)row * p.lda + fk * 8;
#pragma unroll
        for (int kk = 0; kk < GR_K / 16; ++kk) ay[kk] = *reinterpret_cast<const bf16x8*>(src + kk * 16);
    }
    // this lane's 4 DMA pieces of a load: LDS row r = 64 c' + 32 (u & 1) + 8 q + 4 fk' + r' (TileFeed's piece order and source-side swizzle)
    // <- Mf row ns = 128 (q % 5) + 64 (u & 1) + 16 q + 8 c' + 4 fk' + r'
    int moff[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r = 8 * (wave * 4 + i) + (lane >> 3);
        const int ns = (r >> 6) * 8 + ((r >> 5) & 1) * 64 + ((r >> 3) & 3) * 16 + ((r >> 2) & 1) * 4 + (r & 3);
        moff[i] = ns * p.ldb + (((lane & 7) ^ tile_swz<64>(r)) << 3);
    }
    const bf16_t* mf = p.Mf + (int64_t)clip * p.mf_clip_stride;
    auto issue = [&](int q) {
        const int kt = q / GR_NRC, rc = q - kt * GR_NRC;
        const bf16_t* src = mf + (int64_t)rc * 128 * p.ldb + kt * 64;
        unsigned char* dst = ring + (q & (GR_NSLOT - 1)) * GR_SLOT;
#pragma unroll
        for (int i = 0; i < 4; ++i)
            __builtin_amdgcn_global_load_lds((glb_ptr_t)(src + moff[i]), (lds_ptr_t)(dst + (wave * 4 + i) * 1024), 16, 0, 0);
    };
    static_for<0, GR_NSLOT>([&](auto q) { issue(decltype(q)::value); });
    if (tid < GR_NS / 4) reinterpret_cast<float4*>(cbs)[tid] = cr;

    f32x16 acc[GR_NT];
#pragma unroll
    for (int u = 0; u < GR_NT; ++u)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[u][r] = 0.f;
    // load q's fragments for this wave: its parity's two 32-row tiles, all four k-steps
    bf16x8 bf[2][4][2];
    auto frags = [&](int q, bf16x8 (&f)[4][2]) {
        const unsigned char* Bs = ring + (q & (GR_NSLOT - 1)) * GR_SLOT;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) frag_load<2, 64>(Bs, c * 64, ks, fk, frow, f[ks]);
    };
    wait_vmcnt<(GR_NSLOT - 1) * 4>();             // load 0 landed (and everything issued before it)
    __builtin_amdgcn_s_waitcnt(0xc07f);           // own LDS writes (VW, bias) done before the barrier publishes them
    __builtin_amdgcn_s_barrier();
    frags(0, bf[0]);
    // step q: load q + 1 landed everywhere -> refill the slot step q - 1 multiplied with load q + 8 -> read load q + 1's fragments -> load q's MFMAs
    static_for<0, GR_NLOAD>([&](auto qc) {
        constexpr int q = decltype(qc)::value, kt = q / GR_NRC, rc = q % GR_NRC;
        if constexpr (q + 1 < GR_NLOAD) {
            constexpr int left = GR_NLOAD - 2 - q;       // loads behind q + 1 that exist
            wait_vmcnt<(left < GR_NSLOT - 2 ? left : GR_NSLOT - 2) * 4>();
            __builtin_amdgcn_s_waitcnt(0xc07f);          // this wave's fragment reads of load q are in its registers
            __builtin_amdgcn_s_barrier();
            if constexpr (q + GR_NSLOT < GR_NLOAD) issue(q + GR_NSLOT);
            frags(q + 1, bf[(q + 1) & 1]);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            acc[2 * rc] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bf[q & 1][ks][0], ay[kt * 4 + ks], acc[2 * rc], 0, 0, 0);
            acc[2 * rc + 1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bf[q & 1][ks][1], ay[kt * 4 + ks], acc[2 * rc + 1], 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
    });
    __syncthreads();                              // the ring is free: exchange buffers from here on

    // ---- scores: + bias; acc[u][4 q + r] = score(key 8 u + 2 q + c, head 4 fk + r) of this lane's token
    const int nsl = 8 * c + 4 * fk;               // + 64 u + 16 q (+ r): the lane's score columns
#pragma unroll
    for (int u = 0; u < GR_NT; ++u)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float4 b4 = *reinterpret_cast<const float4*>(cbs + 64 * u + 16 * q + nsl);
            acc[u][4 * q + 0] += b4.x; acc[u][4 * q + 1] += b4.y; acc[u][4 * q + 2] += b4.z; acc[u][4 * q + 3] += b4.w;
        }
    // ---- m: the lane's 40 keys per head, then the other parity's (same lane of wave ^ 2)
    float m[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        m[r] = -INFINITY;
#pragma unroll
        for (int u = 0; u < GR_NT; ++u)
#pragma unroll
            for (int q = 0; q < 4; ++q) m[r] = fmaxf(m[r], acc[u][4 * q + r]);
    }
    float4* mx = reinterpret_cast<float4*>(ring + GR_MX);
    mx[wave * 64 + lane] = make_float4(m[0], m[1], m[2], m[3]);
    __syncthreads();
    {
        const float4 o = mx[(wave ^ 2) * 64 + lane];
        m[0] = fmaxf(m[0], o.x); m[1] = fmaxf(m[1], o.y); m[2] = fmaxf(m[2], o.z); m[3] = fmaxf(m[3], o.w);
    }
    // ---- p = exp(s - m) in place; l[q][r]: the chain of key residue 2 q + c over its ten steps
    float l[4][4];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int r = 0; r < 4; ++r) l[q][r] = 0.f;
#pragma unroll
    for (int u = 0; u < GR_NT; ++u)
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                acc[u][4 * q + r] = __expf(acc[u][4 * q + r] - m[r]);
                l[q][r] += acc[u][4 * q + r];
            }
    float4* lx = reinterpret_cast<float4*>(ring + GR_LX);
#pragma unroll
    for (int q = 0; q < 4; ++q) lx[(wave * 64 + lane) * 4 + q] = make_float4(l[q][0], l[q][1], l[q][2], l[q][3]);
    __syncthreads();
    float inv[4];
    {
        float s[4][4];      // s[q][r] = l[2 q] + l[2 q + 1]
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float4 o = lx[((wave ^ 2) * 64 + lane) * 4 + q];
            s[q][0] = l[q][0] + o.x; s[q][1] = l[q][1] + o.y; s[q][2] = l[q][2] + o.z; s[q][3] = l[q][3] + o.w;
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) inv[r] = 1.f / ((s[0][r] + s[1][r]) + (s[2][r] + s[3][r]));
    }
    // ---- value/gate contraction: chains over the steps, VW rows from LDS (two distinct addresses per wave: broadcast reads)
    float4 ct[4][4];        // [q][r] -> experts
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int r = 0; r < 4; ++r) ct[q][r] = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int u = 0; u < GR_NT; ++u)
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float4 w = *reinterpret_cast<const float4*>(vws + (64 * u + 16 * q + nsl + r) * 4);
                const float pv = acc[u][4 * q + r];
                ct[q][r].x += pv * w.x; ct[q][r].y += pv * w.y; ct[q][r].z += pv * w.z; ct[q][r].w += pv * w.w;
            }
    // ---- x = chain * inv; the two lane-local tree levels (kr ^ 4 = q ^ 2, kr ^ 2 = q ^ 1); a2 -> LDS [token][parity][head][expert]
    float* ax = reinterpret_cast<float*>(ring + GR_AX);
    // (router_tokens rounds chain * inv before reduce_logits adds - its selects keep the compiler from fusing the two; pinned here)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma clang fp contract(off)
        float4 x[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) { x[q].x = ct[q][r].x * inv[r]; x[q].y = ct[q][r].y * inv[r]; x[q].z = ct[q][r].z * inv[r]; x[q].w = ct[q][r].w * inv[r]; }
        float4 a2;
        a2.x = (x[0].x + x[2].x) + (x[1].x + x[3].x); a2.y = (x[0].y + x[2].y) + (x[1].y + x[3].y);
        a2.z = (x[0].z + x[2].z) + (x[1].z + x[3].z); a2.w = (x[0].w + x[2].w) + (x[1].w + x[3].w);
        *reinterpret_cast<float4*>(ax + (th * 32 + frow) * GR_AXP + c * 32 + (4 * fk + r) * 4) = a2;
    }
    __syncthreads();
    // ---- one thread per (token, expert): the parity level, then the head levels
    float* lg = reinterpret_cast<float*>(ring + GR_LG);
    {
        const float* at = ax + (tid >> 2) * GR_AXP + (tid & 3);
        float a3[8];
#pragma unroll
        for (int h = 0; h < 8; ++h) a3[h] = at[h * 4] + at[32 + h * 4];
        const float b0 = a3[0] + a3[4], b1 = a3[1] + a3[5], b2 = a3[2] + a3[6], b3 = a3[3] + a3[7];
        lg[tid] = (b0 + b2) + (b1 + b3);
    }
    __syncthreads();
    // ---- the router's phase B on this wave's 16 tokens, four side by side, its four rounds unrolled in one call (a loop of four calls
    // measured the same: 39.0 against 40.2 us per launch)
    {
        const int lt = wave * 16;
        const int n0 = row0 + lt;
        if (n0 < rows_end)
            router_phase_b<4, 16>(p.r, n0, rows_end, [&](int t0, int tokq, int sl) { return sl < GR_E ? lg[(lt + t0 + tokq) * GR_E + sl] : 0.f; });
    }
}

bool gate_route_supported(int NS, int K, int E, int Hh) { return NS == GR_NS && K == GR_K && E == GR_E && Hh == 8; }

int launch_gate_route(const ScoreRouterArgs& a, hipStream_t st) {
    const int T = a.r.T;
    if (!gate_route_supported(a.r.NS, a.K, a.r.E, a.r.Hh)) VB_FAIL(VB_E_INVALID, "gate_route: NS=%d K=%d E=%d heads=%d unsupported", a.r.NS, a.K, a.r.E, a.r.Hh);
    if (a.lda % 8 || a.ldb % 8 || T < 1 || a.Beff < 1) VB_FAIL(VB_E_INVALID, "gate_route: lda/ldb must be multiples of 8, T and clips positive");
    GateRouteDev d;
    d.A = a.A; d.lda = a.lda; d.Mf = a.Bm; d.mf_clip_stride = (int64_t)GR_NS * a.ldb; d.ldb = a.ldb; d.bias = a.bias;
    d.Beff = a.Beff; d.tiles_per_clip = cdiv(T, GR_TOK);
    d.r = a.r;
    d.r.N = a.Beff * T; d.r.D = a.K; d.r.sc = nullptr; d.r.lc_out = nullptr; if (d.r.B <= 0) d.r.B = 1;
    const double n_tok = (double)a.Beff * T;
    ProfScope prof(0, 2.0 * n_tok * GR_NS * a.K, 2.0 * (n_tok * a.K + (double)a.Beff * GR_NS * a.K) + 16.0 * n_tok, st);
    static OnceFlags attr;
    vb_set_max_lds_once(attr, reinterpret_cast<const void*>(gate_route_kernel), GR_LDS);
    hipLaunchKernelGGL(gate_route_kernel, dim3(d.tiles_per_clip * ((a.Beff + 7) / 8 * 8)), dim3(256), GR_LDS, st, d);
    VB_CHECK_LAUNCH();
    return VB_OK;
}
