// Fused kernels of the Band-MoE feed-forwards (gfx950): the routed experts' second product as one pair-bucketed launch
// (moe_w2_pair_kernel) and the band experts' whole FFN in one kernel (band_ffn_kernel, band_ffn96_kernel).  Tile walk, swizzle, DMA feed and
// the MFMA step are the GEMM kernels' (gemm_tile.h), P16 layout and the gated-residual epilogue too (gemm_dev.h).
#include "gemm_tile.h"

// ---- routed experts, second product, ONE launch (vocal2music_moe.py:154-167: y = m_c FFN^c(u) + m_a FFN^a(u)) ------------------
// The two w2 GEMMs (caption group: scatter m_c * H_c W2c^T as fp32; acoustic group: read it back, add m_a * H_a W2a^T, write bf16
// planes) round-tripped a [N][768] fp32 partial sum through HBM: 37 MB written + 37 MB re-read per block evaluation at 8 clips, for
// two launches at 10-13 % of the MFMA peak.  Here the tokens are bucketed by their (caption expert, acoustic expert) PAIR (E*E groups,
// bucket_place_kernel: the caption slots ARE the pair slots) and ONE grouped launch walks K = 2H as a plain GEMM: first half A = the
// tile's own rows of the routed hidden tensor (caption slots, contiguous) against W2c[c], second half A = the tokens' acoustic-slot
// rows (gathered) against W2a[a].  The per-token gate weights m_c / m_a ride in the hidden rows (folded in by the SwiGLU epilogue
// before the bf16 rounding - the same relative rounding error as scaling the fp32 product afterwards), so one accumulator serves.
// Tile 128 x (64 TN): 128 x 192 when that brings the launch from two rounds of the CUs down to one (8 clips: 110 row tiles x 4
// = 440 workgroups at two per CU), 128 x 128 otherwise.  Ring / swizzle / P16 column layout as in gemm_bf16_glds_kernel<*, 64, 2>.
struct PairDev {
    const bf16_t* Hs; int ldh;                               // routed hidden [2N][H] bf16, slot order (caption slots, then acoustic slots)
    const bf16_t* W2; int64_t w_stride; int ldw;             // [2E][D][H]
    const int* pair_off; const int* perm; const int* pair_pa;   // pair slot p: caption row = p, acoustic row = pair_pa[p], token = perm[p]
    bf16_t* out; int ldc;                                    // y planes [N][D] (one plane: bf16 production mode)
    int N, D, H, E, n_tiles;
};
template <int TN>
__global__ void __launch_bounds__(NTHREADS) __attribute__((amdgpu_waves_per_eu(2, 2))) moe_w2_pair_kernel(const PairDev p) {
    constexpr int BKT = 64, NST = 2;
    constexpr int BNP = 64 * TN;                             // columns per tile
    using Feed = TileFeed<BM, BNP, BKT, 4>;
    __shared__ __attribute__((aligned(16))) unsigned char lds[NST * Feed::STAGE];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 1, wc = wave & 1;

    int g = 0, row0 = 0, rows_end = 0, tile_n, rt;
    const int tmg = tile_xcd_order(p.n_tiles, tile_n, rt);
    if (!tile_group_search<BM>(p.pair_off, p.E * p.E, tmg, g, row0, rows_end)) return;
    const int ec = g / p.E, ea = g - ec * p.E;
    const int n0 = tile_n * BNP;
    const int KT = p.H / BKT;
    const int total = 2 * KT;

    const bf16_t* asrc[2][Feed::PA]; const bf16_t* bsrc[Feed::PB];     // B: one pointer per piece, the expert half is a uniform offset
    const int64_t boff1 = (int64_t)(p.E + ea - ec) * p.w_stride;
    Feed::rows(asrc[0], p.Hs, p.ldh, row0, rows_end, row0, false, wave, lane, [](int slot) { return slot; });          // caption half: the pair slots ARE the caption slots
    Feed::rows(asrc[1], p.Hs, p.ldh, row0, rows_end, row0, false, wave, lane, [&](int slot) { return p.pair_pa[slot]; });   // acoustic half: gathered
    // P16 column layout: a lane ends up with 16 consecutive output columns
    Feed::rows(bsrc, p.W2 + (int64_t)ec * p.w_stride, p.ldw, n0, p.D, 0, true, wave, lane, [](int nrow) { return nrow; });
    auto issue = [&](int t) {
        const int half = t >= KT ? 1 : 0;
        const int k0 = (t - half * KT) * BKT;
        const bf16_t* ap[Feed::PA];
#pragma unroll
        for (int i = 0; i < Feed::PA; ++i) ap[i] = half ? asrc[1][i] : asrc[0][i];
        Feed::issue(ap, bsrc, wave, lds + (t % NST) * Feed::STAGE, k0, (half ? boff1 : 0) + k0);
    };

    f32x16 acc[2][TN];
    acc_zero(acc);

    issue(0);
    const int frow = lane & 31, fk = lane >> 5;
    for (int t = 0; t < total; ++t) {
        const int st = t % NST;
        wait_vmcnt<0>();
        __builtin_amdgcn_s_barrier();           // tile t landed everywhere; everyone finished reading stage (t-1)%NST
        if (t + 1 < total) issue(t + 1);
        const unsigned char* As = lds + st * Feed::STAGE;
        const unsigned char* Bs = As + Feed::ABYTES;
        bf16x8 af[2][2], bf[2][TN];
        frag_load<2, TN, BKT>(As, Bs, wr * 64, wc * 32 * TN, 0, fk, frow, af[0], bf[0]);
#pragma unroll
        for (int ks = 0; ks < BKT / 16; ++ks) {
            const int cur = ks & 1;
            if (ks + 1 < BKT / 16) frag_load<2, TN, BKT>(As, Bs, wr * 64, wc * 32 * TN, ks + 1, fk, frow, af[cur ^ 1], bf[cur ^ 1]);
            __builtin_amdgcn_sched_barrier(0);
            mfma_step(af[cur], bf[cur], acc);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    // epilogue: a lane owns one token row and 16 consecutive columns per 32 x 32 tile (P16 layout): 16-byte stores
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int slot = row0 + wr * 64 + i * 32 + frow;
        if (slot >= rows_end) continue;
        const int tok = p.perm[slot];
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int n = n0 + wc * 32 * TN + j * 32 + fk * 16;
            if (n >= p.D) continue;                                       // D % 16 == 0
            float o[16];
#pragma unroll
            for (int e = 0; e < 16; ++e) o[e] = acc[i][j][e];
            store8p(p.out, 0, 1, (int64_t)tok * p.ldc + n, o);
            store8p(p.out, 0, 1, (int64_t)tok * p.ldc + n + 8, o + 8);
        }
    }
}
int launch_moe_w2_pair(const MoeW2PairArgs& a, hipStream_t st) {
    if (a.H % 64 || a.D % 16 || a.E < 1 || a.E * a.E > 16) VB_FAIL(VB_E_INVALID, "moe_w2_pair: H=%d D=%d E=%d unsupported", a.H, a.D, a.E);
    PairDev d;
    d.Hs = a.Hs; d.ldh = a.H; d.W2 = a.W2; d.w_stride = (int64_t)a.D * a.H; d.ldw = a.H;
    d.pair_off = a.pair_off; d.perm = a.perm; d.pair_pa = a.pair_pa;
    d.out = a.out; d.ldc = a.D; d.N = a.N; d.D = a.D; d.H = a.H; d.E = a.E;
    const int mt = cdiv(a.N, BM) + a.E * a.E;                    // upper bound of the row tiles over all pair groups
    ProfScope prof(0, 2.0 * a.N * a.D * 2.0 * a.H, 2.0 * a.N * a.H * 2.0 + 2.0 * a.E * a.D * a.H * 2.0 + (double)a.N * a.D * 2.0, st);
    // 128 x 192 tiles when 128 x 128 would need a second round of the 512 workgroup slots (two per CU) and 192-wide tiles do not
    const int wide = vb_tune().w2_pair == 3 || (vb_tune().w2_pair == 1 && a.D % 192 == 0 && mt * cdiv(a.D, 128) > 512 && mt * (a.D / 192) <= 512);
    if (wide) {
        d.n_tiles = a.D / 192;
        hipLaunchKernelGGL(moe_w2_pair_kernel<3>, dim3(d.n_tiles * ((mt + 7) / 8 * 8)), dim3(NTHREADS), 0, st, d);
    } else {
        d.n_tiles = cdiv(a.D, BN);
        hipLaunchKernelGGL(moe_w2_pair_kernel<2>, dim3(d.n_tiles * ((mt + 7) / 8 * 8)), dim3(NTHREADS), 0, st, d);
    }
    VB_CHECK_LAUNCH();
    return VB_OK;
}

// ---- band-expert FFN, fused ------------------------------------------------------------------------------------------
// Band-MoE "frequency" experts (vocal2music_moe.py:171-178; FeedForward flag_large_dit_moe.py:480-485): expert e sees only
// the 192-channel band e of y and produces only band e:   z[:, band e] = W2_e . ( silu(W1_e y_e) * (W3_e y_e) ).
// As two grouped GEMMs this wrote and re-read the [N][E*512] hidden tensor (98 MB per block evaluation) and streamed every
// weight byte through L2->LDS at 64 flop/B (the feed that bounds these K = 192 / 512 GEMMs).  Here one
// workgroup owns 192 tokens x one band (12032 tokens x 4 bands = 252 workgroups = one round of the 256 CUs):
//   * the token tile's band y_e [192 x 192] is DMA'd into LDS once and stays;
//   * the hidden dimension is walked in chunks of 64: w1/w3 rows of the chunk (interleaved, [128 x 192]) stream through a
//     2-stage ring as three K-slabs -> acc1 [192 x 128] -> SwiGLU lane-locally -> bf16 chunk [192 x 64] into LDS as the A
//     operand of the second product -> one slab of w2 [192 x 64] -> acc2 [192 x 192] += ...   (171 flop per byte DMA'd);
//   * the gated residual epilogue of the unfused w2 GEMM is reused as is (staged_epilogue<EPI_RESID_GATE>).
// bf16 (np = 1) only: the split-precision parity mode keeps the two-GEMM path.
struct BandDev {
    GemmDev ep;                    // epilogue view: out32/ldc32, gate/gate_ld, T/rT, c_noff_group = band, N = band
    const bf16_t* Y; int ldy;      // [M][ldy], band e at column e * 192
    const bf16_t* W13; const bf16_t* W2;   // [E][2H][192] (w1/w3 rows interleaved), [E][192][H]
    int M, H, E;
};
#define BF_BM 192
#define BF_BAND 192
template <bool HOIST>      // HOIST: see staged_epilogue (VB_BAND_EPI_OLD=1 selects the two-pass form)
__global__ void __launch_bounds__(NTHREADS) band_ffn_kernel(const BandDev p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char bl[];
    constexpr int HCH = BF_BM * 128;              // bytes of the [192 x 64] bf16 hidden chunk
    constexpr int NSLOT = 8;                      // ring slots of 16 KB
    unsigned char* Hs = bl;
    unsigned char* ring = bl + HCH;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 1, wc = wave & 1;
    const int frow = lane & 31, fk = lane >> 5;
    // XCD x handles band x % E (the band's 590 KB of weights stay in that XCD's L2), two XCDs per band at E = 4
    const int L = blockIdx.x;
    const int e = (L & 7) % p.E;
    const int rt = (L >> 3) * (8 / p.E) + (L & 7) / p.E;
    const int row0 = rt * BF_BM;
    if (row0 >= p.M) return;
    const int rows_end = p.M;
    const int r8 = lane >> 3, cs = lane & 7;
    unsigned long long tq0 = 0, tq1 = 0, tq2 = 0;
    if (p.ep.trace) tq0 = __builtin_amdgcn_s_memtime();

    // The token tile's band y_e [192 x 192] is this workgroup's A operand for the whole first product: every wave keeps the
    // fragments of its 96 rows in registers (3 row tiles x 12 k-steps x 16 B per lane = 144 VGPRs, loaded once), which leaves
    // the LDS to the weight stream.
    bf16x8 ay[3][12];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        int row = row0 + wr * 96 + i * 32 + frow;
        if (row >= rows_end) row = row0;
        const bf16_t* src = p.Y + (int64_t)row * p.ldy + e * BF_BAND + fk * 8;
#pragma unroll
        for (int kk = 0; kk < 12; ++kk) ay[i][kk] = *reinterpret_cast<const bf16x8*>(src + kk * 16);
    }
    const bf16_t* w13 = p.W13 + (int64_t)e * 2 * p.H * BF_BAND;
    const bf16_t* w2 = p.W2 + (int64_t)e * BF_BAND * p.H;
    // weight stream: per hidden chunk 5 loads - three K-slabs of w13 [128 x 64] (16 KB, 4 DMA pieces per wave) and two K-halves
    // of the w2 slab [192 x 32] (12 KB, 3 pieces per wave) - through a ring of eight 16-KB slots, SEVEN loads ahead of the one
    // being multiplied.  A load is 18-24 MFMAs of work per wave (0.4 us) against a ~2.3 us L2 round trip: the stream rate is
    // (bytes in flight) / latency, so one-ahead double buffering ran at 69 us per launch and three-ahead at 59; the waits are
    // counted vmcnt, never a drain.
    int a_off[4], b_off[3];          // element offsets of this lane's DMA pieces inside a w13 slab / a w2 half-slab
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r = 8 * (wave * 4 + i) + r8;
        a_off[i] = r * BF_BAND + ((cs ^ tile_swz<64>(r)) << 3);
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int r = 16 * (wave * 3 + i) + (lane >> 2);
        b_off[i] = r * p.H + (((lane & 3) ^ tile_swz<32>(r)) << 3);
    }
    const int nchunk = p.H / 64;
    const int nload = nchunk * 5;
    auto issue = [&](int q) {
        unsigned char* dst = ring + (q & (NSLOT - 1)) * 16384;
        while (q >= nload) q -= 5;                // past the end: reload the same-typed piece of the last chunk into a dead slot, so
                                                  // every step sees the piece counts its counted vmcnt assumes
        const int hc = q / 5, t = q - hc * 5;
        if (t < 3) {
            const bf16_t* src = w13 + (int64_t)hc * 128 * BF_BAND + t * 64;
#pragma unroll
            for (int i = 0; i < 4; ++i)
                __builtin_amdgcn_global_load_lds((glb_ptr_t)(src + a_off[i]), (lds_ptr_t)(dst + (wave * 4 + i) * 1024), 16, 0, 0);
        } else {
            const bf16_t* src = w2 + hc * 64 + (t - 3) * 32;
#pragma unroll
            for (int i = 0; i < 3; ++i)
                __builtin_amdgcn_global_load_lds((glb_ptr_t)(src + b_off[i]), (lds_ptr_t)(dst + (wave * 3 + i) * 1024), 16, 0, 0);
        }
    };
#pragma unroll
    for (int q = 0; q < NSLOT - 1; ++q) issue(q);

    f32x16 acc1[3][2], acc2[3][3];
    acc_zero(acc1);
    acc_zero(acc2);
    // step q multiplies load q; loads q+1 .. q+6 (already issued) may stay in flight: AHEAD = their DMA pieces per wave
    auto step_begin = [&](int q, auto ahead) -> const unsigned char* {
        wait_vmcnt<decltype(ahead)::value>();
        __builtin_amdgcn_s_waitcnt(0xc07f);       // own LDS writes (SwiGLU chunk) done before the barrier publishes them
        __builtin_amdgcn_s_barrier();             // load q landed everywhere; everyone is done with load q-1's slot
        issue(q + NSLOT - 1);                     // -> slot (q-1) % NSLOT
        return ring + (q & (NSLOT - 1)) * 16384;
    };
    // fragment reads run one k-step ahead of the MFMAs that use them (one wave per SIMD: an LDS round trip in front of every batch of
    // six MFMAs was as long as the batch)
    auto phase_a = [&](int kc, const unsigned char* Bs) {
        bf16x8 bf[2][2];
        frag_load<2, 64>(Bs, wc * 64, 0, fk, frow, bf[0]);
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            if (ks + 1 < 4) frag_load<2, 64>(Bs, wc * 64, ks + 1, fk, frow, bf[(ks + 1) & 1]);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < 3; ++i) mfma_row(ay[i][kc * 4 + ks], bf[ks & 1], acc1[i]);      // (A: the register-resident token fragments)
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    auto phase_b = [&](const unsigned char* Bs, int khalf) {
        bf16x8 af[2][3], bf[2][3];
        auto rd = [&](int ks, int slot) {       // hidden chunk: 64-deep rows, k half khalf; w2 half-slab: 32-deep rows
            frag_load<3, 64>(Hs, wr * 96, khalf * 2 + ks, fk, frow, af[slot]);
            frag_load<3, 32>(Bs, wc * 96, ks, fk, frow, bf[slot]);
        };
        rd(0, 0);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            if (ks + 1 < 2) rd(ks + 1, (ks + 1) & 1);
            __builtin_amdgcn_sched_barrier(0);
            mfma_step(af[ks & 1], bf[ks & 1], acc2);
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    using std::integral_constant;
#pragma unroll 1
    for (int hc = 0; hc < nchunk; ++hc) {
        const int q0 = hc * 5;
        // piece counts per wave of the six loads behind the consumed one (pattern A4 A4 A4 B3 B3, cyclic)
        const unsigned char* b0 = step_begin(q0 + 0, integral_constant<int, 22>());
        if (hc == 0 && p.ep.trace) tq1 = __builtin_amdgcn_s_memtime();
        phase_a(0, b0);
        phase_a(1, step_begin(q0 + 1, integral_constant<int, 22>()));
        phase_a(2, step_begin(q0 + 2, integral_constant<int, 21>()));
        {
            // SwiGLU on the interleaved (w1, w3) column pairs -> this chunk's hidden values, bf16, as the next A operand
            typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int row = wr * 96 + i * 32 + frow;
                        const int h0 = wc * 32 + j * 16 + q * 4 + fk * 2;
                        bf16x2 hv;
                        hv[0] = f2bf(silu_f(acc1[i][j][q * 4 + 0]) * acc1[i][j][q * 4 + 1]);
                        hv[1] = f2bf(silu_f(acc1[i][j][q * 4 + 2]) * acc1[i][j][q * 4 + 3]);
                        *reinterpret_cast<bf16x2*>(Hs + lds_off_t<64>(row, h0 >> 3) + (h0 & 7) * 2) = hv;
#pragma unroll
                        for (int r = 0; r < 4; ++r) acc1[i][j][q * 4 + r] = 0.f;
                    }
        }
        phase_b(step_begin(q0 + 3, integral_constant<int, 21>()), 0);
        phase_b(step_begin(q0 + 4, integral_constant<int, 22>()), 1);
    }
    wait_vmcnt<0>();                              // the dummy tail loads
    if (p.ep.trace) tq2 = __builtin_amdgcn_s_memtime();
    // gated residual: h[:, band e] += gate * z   (same epilogue as the unfused w2 GEMM; LDS is free now)
    // (round 3: the same epilogue straight from the accumulators in the P16 column layout - no LDS slab, no epilogue barriers - measured
    //  62.9 against 63.5 us: the 74 MB read-modify-write of all 252 workgroups at once is an HBM burst, not an instruction-issue problem)
    staged_epilogue<EPI_RESID_GATE, 3, 3, 2, NTHREADS, HOIST>(p.ep, e, acc2, reinterpret_cast<float*>(bl), row0, rows_end, 0, tid, wr, wc, frow, fk);
    if (p.ep.trace && tid == 0) {
        __builtin_amdgcn_s_waitcnt(0);
        unsigned long long* tr = p.ep.trace + (size_t)blockIdx.x * 4;
        tr[0] = tq0; tr[1] = tq1; tr[2] = tq2; tr[3] = __builtin_amdgcn_s_memtime();
    }
}

// ---- band-expert FFN, fused, 96-channel bands (8 experts per group, BASELINE configs[2]) ------------------------------------
// Same idea as band_ffn_kernel for band = 96: at E = 8 the hidden tensor of the band experts is [N][8 x 512] bf16 - 394 MB written by
// the w1/w3 GEMM and read back by the w2 GEMM per block evaluation at 32 clips (306 + 166 us, profiles/r02_final_c3_kernel_stats.csv).
// One workgroup owns 256 tokens x one band; 4 waves, wave w owns rows [64 w, 64 w + 64) in BOTH products (2 row tiles; 4 column tiles
// of the 128-column w1/w3 chunk, 3 column tiles of the 96 outputs), so a wave reads back only the hidden values it wrote itself:
//   * y_e [64 x 96] per wave lives in registers (2 x 6 fragments);
//   * per 64-wide hidden chunk 4 loads through a ring of eight 12-KB slots, seven ahead: three K-slabs of w13 [128 rows x 32] (8 KB,
//     2 DMA pieces per wave) and the w2 slab [96 rows x 64] (12 KB, 3 pieces per wave); counted vmcnt (pattern 2 2 2 3);
//   * acc1 [64 x 128] -> SwiGLU lane-locally -> bf16 hidden chunk [64 x 64] in LDS -> acc2 [64 x 96] += hidden . w2 slab;
//   * gated residual epilogue straight from the MFMA layout (wave_epilogue<EPI_RESID_GATE>): a lane owns one row and 4 consecutive
//     columns, 16-byte loads / stores.
// k runs ascending in both products, as in the grouped GEMMs: bit-identical to the unfused path.
#define B96_BM 256
#define B96_BAND 96
#define B96_SLOT 12288
__global__ void __launch_bounds__(NTHREADS) band_ffn96_kernel(const BandDev p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char bl96[];
    constexpr int HCH = B96_BM * 128;             // bytes of the [256 x 64] bf16 hidden chunk
    constexpr int NSLOT = 8;
    unsigned char* Hs = bl96;
    unsigned char* ring = bl96 + HCH;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int frow = lane & 31, fk = lane >> 5;
    const int L = blockIdx.x;
    const int e = (L & 7) % p.E;
    const int rt = (L >> 3) * (8 / p.E) + (L & 7) / p.E;
    const int row0 = rt * B96_BM;
    if (row0 >= p.M) return;
    const int rows_end = p.M;

    bf16x8 ay[2][6];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        int row = row0 + wave * 64 + i * 32 + frow;
        if (row >= rows_end) row = row0;
        const bf16_t* src = p.Y + (int64_t)row * p.ldy + e * B96_BAND + fk * 8;
#pragma unroll
        for (int kk = 0; kk < 6; ++kk) ay[i][kk] = *reinterpret_cast<const bf16x8*>(src + kk * 16);
    }
    const bf16_t* w13 = p.W13 + (int64_t)e * 2 * p.H * B96_BAND;
    const bf16_t* w2 = p.W2 + (int64_t)e * B96_BAND * p.H;
    int a_off[2], b_off[3];          // element offsets of this lane's DMA pieces inside a w13 K-slab / the w2 slab
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int r = 16 * (wave * 2 + i) + (lane >> 2);                  // 16 rows x 64 B per piece
        a_off[i] = r * B96_BAND + (((lane & 3) ^ tile_swz<32>(r)) << 3);
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int r = 8 * (wave * 3 + i) + (lane >> 3);                   // 8 rows x 128 B per piece
        b_off[i] = r * p.H + (((lane & 7) ^ tile_swz<64>(r)) << 3);
    }
    const int nchunk = p.H / 64;
    const int nload = nchunk * 4;
    auto issue = [&](int q) {
        unsigned char* dst = ring + (q & (NSLOT - 1)) * B96_SLOT;
        while (q >= nload) q -= 4;                // past the end: same-typed dummy reload into a dead slot (keeps the counted vmcnt pattern)
        const int hc = q >> 2, t = q & 3;
        if (t < 3) {
            const bf16_t* src = w13 + (int64_t)hc * 128 * B96_BAND + t * 32;
#pragma unroll
            for (int i = 0; i < 2; ++i)
                __builtin_amdgcn_global_load_lds((glb_ptr_t)(src + a_off[i]), (lds_ptr_t)(dst + (wave * 2 + i) * 1024), 16, 0, 0);
        } else {
            const bf16_t* src = w2 + hc * 64;
#pragma unroll
            for (int i = 0; i < 3; ++i)
                __builtin_amdgcn_global_load_lds((glb_ptr_t)(src + b_off[i]), (lds_ptr_t)(dst + (wave * 3 + i) * 1024), 16, 0, 0);
        }
    };
#pragma unroll
    for (int q = 0; q < NSLOT - 1; ++q) issue(q);

    f32x16 acc1[2][4], acc2[2][3];
    acc_zero(acc1);
    acc_zero(acc2);
    // step q multiplies load q; loads q+1 .. q+6 (already issued) may stay in flight: AHEAD = their DMA pieces per wave
    auto step_begin = [&](int q, auto ahead) -> const unsigned char* {
        wait_vmcnt<decltype(ahead)::value>();
        __builtin_amdgcn_s_waitcnt(0xc07f);       // own LDS traffic done before the barrier
        __builtin_amdgcn_s_barrier();             // load q landed everywhere; everyone is done with load q-1's slot
        issue(q + NSLOT - 1);                     // -> slot (q-1) % NSLOT
        return ring + (q & (NSLOT - 1)) * B96_SLOT;
    };
    auto phase_a = [&](int t, const unsigned char* Bs) {
        bf16x8 bf[2][4];
        frag_load<4, 32>(Bs, 0, 0, fk, frow, bf[0]);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            if (ks + 1 < 2) frag_load<4, 32>(Bs, 0, ks + 1, fk, frow, bf[1]);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < 2; ++i) mfma_row(ay[i][t * 2 + ks], bf[ks], acc1[i]);            // (A: the register-resident token fragments)
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    auto phase_b = [&](const unsigned char* Bs) {
        bf16x8 af[2][2], bf[2][3];
        frag_load<2, 3, 64>(Hs, Bs, wave * 64, 0, 0, fk, frow, af[0], bf[0]);
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            if (ks + 1 < 4) frag_load<2, 3, 64>(Hs, Bs, wave * 64, 0, ks + 1, fk, frow, af[(ks + 1) & 1], bf[(ks + 1) & 1]);
            __builtin_amdgcn_sched_barrier(0);
            mfma_step(af[ks & 1], bf[ks & 1], acc2);
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    using std::integral_constant;
#pragma unroll 1
    for (int hc = 0; hc < nchunk; ++hc) {
        const int q0 = hc * 4;
        // pieces per wave of the six loads behind the consumed one (pattern A2 A2 A2 B3, cyclic)
        phase_a(0, step_begin(q0 + 0, integral_constant<int, 13>()));
        phase_a(1, step_begin(q0 + 1, integral_constant<int, 14>()));
        phase_a(2, step_begin(q0 + 2, integral_constant<int, 14>()));
        {
            // SwiGLU on the interleaved (w1, w3) column pairs -> this chunk's hidden values (rows of this wave only), bf16
            typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int row = wave * 64 + i * 32 + frow;
                        const int h0 = j * 16 + q * 4 + fk * 2;
                        bf16x2 hv;
                        hv[0] = f2bf(silu_f(acc1[i][j][q * 4 + 0]) * acc1[i][j][q * 4 + 1]);
                        hv[1] = f2bf(silu_f(acc1[i][j][q * 4 + 2]) * acc1[i][j][q * 4 + 3]);
                        *reinterpret_cast<bf16x2*>(Hs + lds_off_t<64>(row, h0 >> 3) + (h0 & 7) * 2) = hv;
#pragma unroll
                        for (int r = 0; r < 4; ++r) acc1[i][j][q * 4 + r] = 0.f;
                    }
        }
        phase_b(step_begin(q0 + 3, integral_constant<int, 13>()));
    }
    wait_vmcnt<0>();                              // the dummy tail loads
    // gated residual: h[:, band e] += gate * z   (same arithmetic as the unfused w2 GEMM's epilogue)
    wave_epilogue<EPI_RESID_GATE, 2, 3>(p.ep, e, acc2, row0 + wave * 64, rows_end, 0, frow, fk);
}

int launch_band_ffn(const BandFfnArgs& a, hipStream_t st) {
    if ((a.band != BF_BAND && a.band != B96_BAND) || a.H % 64 || (8 % a.E) || a.E > 8) VB_FAIL(VB_E_INVALID, "band_ffn: band=%d H=%d E=%d unsupported", a.band, a.H, a.E);
    BandDev d;
    memset(&d, 0, sizeof(d));
    d.Y = a.y; d.ldy = a.ldy; d.W13 = a.w13; d.W2 = a.w2; d.M = a.M; d.H = a.H; d.E = a.E;
    d.ep.out32 = a.out32; d.ep.ldc32 = a.ldc32; d.ep.gate = a.gate; d.ep.gate_ld = a.gate_ld; d.ep.T = a.T > 0 ? a.T : 1;
    d.ep.rT = 1.0f / (float)d.ep.T; d.ep.rhd = 1.f; d.ep.rD = 1.f; d.ep.hd = 1; d.ep.D = 1;
    d.ep.c_noff_group = a.band; d.ep.N = a.band; d.ep.M = a.M; d.ep.trace = g_gemm_trace;
    if (a.M >= (1 << 21)) VB_FAIL(VB_E_INVALID, "band_ffn: M exceeds fdiv()");
    ProfScope prof(0, 2.0 * a.M * a.E * ((double)2 * a.H * a.band + (double)a.band * a.H),
                   (double)a.M * a.E * a.band * (2.0 + 8.0) + (double)a.E * 3.0 * a.H * a.band * 2.0, st);
    if (a.band == B96_BAND) {
        const int tiles96 = cdiv(a.M, B96_BM);
        const int nblk96 = cdiv(tiles96, 8 / a.E) * 8;
        constexpr size_t lds96 = (size_t)B96_BM * 128 + 8 * B96_SLOT;      // hidden chunk (32 KB) + 8 ring slots of 12 KB = 128 KB
        static OnceFlags attr96;
        vb_set_max_lds_once(attr96, reinterpret_cast<const void*>(band_ffn96_kernel), (int)lds96);
        hipLaunchKernelGGL(band_ffn96_kernel, dim3(nblk96), dim3(NTHREADS), lds96, st, d);
        VB_CHECK_LAUNCH();
        return VB_OK;
    }
    const int row_tiles = cdiv(a.M, BF_BM);
    const int per8 = 8 / a.E;                         // row tiles per group of 8 consecutive blocks
    const int nblk = cdiv(row_tiles, per8) * 8;
    constexpr size_t lds = (size_t)BF_BM * 128 + 8 * 16384;   // hidden chunk (24 KB) + 8 ring slots of 16 KB = 152 KB
    static OnceFlags attr;
    static OnceFlags attr_old;
    const bool hoist = !vb_tune().band_epi_old;
    if (hoist) vb_set_max_lds_once(attr, reinterpret_cast<const void*>(band_ffn_kernel<true>), (int)lds);
    else vb_set_max_lds_once(attr_old, reinterpret_cast<const void*>(band_ffn_kernel<false>), (int)lds);
    if (hoist) hipLaunchKernelGGL(band_ffn_kernel<true>, dim3(nblk), dim3(NTHREADS), lds, st, d);
    else hipLaunchKernelGGL(band_ffn_kernel<false>, dim3(nblk), dim3(NTHREADS), lds, st, d);
    VB_CHECK_LAUNCH();
    return VB_OK;
}
