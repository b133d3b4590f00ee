// Fused kernels of the Band-MoE feed-forwards (gfx950): the routed experts' second product as one pair-bucketed launch
// (moe_w2_pair_kernel) and the band experts' whole FFN in one kernel (band_ffn_kernel: one body over BandGeom<192> / BandGeom<96>).
// Tile walk, swizzle, DMA feed, the two-stage K walk and the MFMA step are the GEMM kernels' (gemm_tile.h), P16 layout and the
// gated-residual epilogue too (gemm_dev.h).
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
    const int frow = lane & 31, fk = lane >> 5;
    gemm_walk_2stage<Feed>(lds, total, issue, wr * 64, wc * 32 * TN, fk, frow, acc);
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
    // (192-wide tiles only where they cover D: n_tiles = D / 192 leaves the columns past the last whole tile uncomputed, so VB_W2_PAIR=3
    //  at D % 192 != 0 falls back to the 128-wide tiles, whose last tile is ragged)
    const int wide = a.D % 192 == 0 && (vb_tune().w2_pair == 3 || (vb_tune().w2_pair == 1 && mt * cdiv(a.D, 128) > 512 && mt * (a.D / 192) <= 512));
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
// the band e of y (BAND = 192 channels at 4 experts, 96 at 8) and produces only band e:
//   z[:, band e] = W2_e . ( silu(W1_e y_e) * (W3_e y_e) ).
// As two grouped GEMMs this wrote and re-read the [N][E*512] hidden tensor (98 MB per block evaluation at E = 4) and streamed every
// weight byte through L2->LDS at 64 flop/B (the feed that bounds these K = 192 / 512 GEMMs).  Here one
// workgroup owns ROWS tokens x one band:
//   * the token tile's band y_e [ROWS x BAND] is this workgroup's A operand for the whole first product: every wave keeps the fragments
//     of its rows in registers, loaded once, which leaves the LDS to the weight stream;
//   * the hidden dimension is walked in chunks of 64: the w1/w3 rows of the chunk (interleaved, [128 x BAND]) stream through the ring
//     as BAND / K1 K-slabs -> acc1 [ROWS x 128] -> SwiGLU lane-locally -> bf16 chunk [ROWS x 64] into LDS as the A operand of the
//     second product -> the chunk's w2 slab [BAND x 64], in 64 / K2 loads -> acc2 [ROWS x BAND] += ...;
//   * the weight stream runs through a ring of NSLOT = 8 slots, SEVEN loads ahead of the one being multiplied.  A load is 18-24 MFMAs
//     of work per wave (0.4 us) against a ~2.3 us L2 round trip: the stream rate is (bytes in flight) / latency, so one-ahead double
//     buffering ran at 69 us per launch and three-ahead at 59; the waits are counted vmcnt (band_pieces_ahead), never a drain;
//   * the gated residual epilogue of the unfused w2 GEMM is reused as is.
// k runs ascending in both products, as in the grouped GEMMs: bit-identical to the unfused path.
// bf16 (np = 1) only: the split-precision parity mode keeps the two-GEMM path.
struct BandDev {
    GemmDev ep;                    // epilogue view: out32/ldc32, gate/gate_ld, T/rT, c_noff_group = band, N = band
    const bf16_t* Y; int ldy;      // [M][ldy], band e at column e * BAND
    const bf16_t* W13; const bf16_t* W2;   // [E][2H][BAND] (w1/w3 rows interleaved), [E][BAND][H]
    int M, H, E;
};
constexpr int BAND_NSLOT = 8;      // ring slots (a power of two); a load is issued NSLOT - 1 loads ahead of the step that multiplies it

// What the two band widths choose; BandGeom derives the rest.  ROWS tokens per workgroup, 4 waves as (4 / WC) x WC, a wave owns TM 32-row
// tiles and TN1 / TN2 32-column tiles of the first / second product; K1 / K2 = depth of a w13 K-slab / of a w2 load; STAGED: which epilogue.
template <int BAND> struct BandChoice;
// 192-channel bands (4 experts): 12032 tokens x 4 bands = 252 workgroups = one round of the 256 CUs.  192 x 192 per workgroup, 2 x 2
// waves: a wave keeps the fragments of its 96 rows of y_e in registers (3 row tiles x 12 k-steps x 16 B per lane = 144 VGPRs).  Per
// hidden chunk 5 loads - three K-slabs of w13 [128 x 64] (16 KB, 4 DMA pieces per wave) and two K-halves of the w2 slab [192 x 32]
// (12 KB, 3 pieces per wave) - through 16-KB slots: 171 flop per byte DMA'd.  Epilogue: staged_epilogue<EPI_RESID_GATE> through the
// then free LDS (HOIST: see there; VB_BAND_EPI_OLD=1 selects the two-pass form).
// (round 3: the same epilogue straight from the accumulators in the P16 column layout - no LDS slab, no epilogue barriers - measured
//  62.9 against 63.5 us: the 74 MB read-modify-write of all 252 workgroups at once is an HBM burst, not an instruction-issue problem)
template <> struct BandChoice<192> {
    static constexpr int ROWS = 192, WC = 2, TM = 3, TN1 = 2, TN2 = 3, K1 = 64, K2 = 32;
    static constexpr bool STAGED = true, TRACE = true;      // TRACE: the per-block time stamps of vbdbg_gemm_trace
};
// 96-channel bands (8 experts per group, BASELINE configs[2]): at E = 8 the hidden tensor of the band experts is [N][8 x 512] bf16 -
// 394 MB written by the w1/w3 GEMM and read back by the w2 GEMM per block evaluation at 32 clips (306 + 166 us,
// profiles/r02_final_c3_kernel_stats.csv).  256 tokens per workgroup, 4 x 1 waves: wave w owns rows [64 w, 64 w + 64) in BOTH products
// (4 column tiles of the 128-column w1/w3 chunk, 3 of the 96 outputs), so a wave reads back only the hidden values it wrote itself;
// y_e [64 x 96] per wave is 2 x 6 fragments.  Per hidden chunk 4 loads - three K-slabs of w13 [128 x 32] (8 KB, 2 DMA pieces per wave)
// and the w2 slab [96 x 64] (12 KB, 3 pieces per wave) - through 12-KB slots.  Epilogue straight from the MFMA layout
// (wave_epilogue<EPI_RESID_GATE>): a lane owns one row and 4 consecutive columns, 16-byte loads / stores.
template <> struct BandChoice<96> {
    static constexpr int ROWS = 256, WC = 1, TM = 2, TN1 = 4, TN2 = 3, K1 = 32, K2 = 64;
    static constexpr bool STAGED = false, TRACE = false;
};
template <int BAND_> struct BandGeom : BandChoice<BAND_> {
    using C = BandChoice<BAND_>;
    static constexpr int BAND = BAND_;
    static constexpr int KY = BAND / 16;                    // k-steps of the first product = y_e fragments per row tile
    static constexpr int NA = BAND / C::K1, NB = 64 / C::K2, NL = NA + NB;      // loads per hidden chunk: w13 K-slabs, then w2 loads
    static constexpr int PA = C::K1 / 16, PB = BAND * C::K2 / 2048;             // DMA pieces (1 KB) per wave of a w13 slab [128 x K1] / a w2 load [BAND x K2]
    static constexpr int SLOT = (128 * C::K1 > BAND * C::K2 ? 128 * C::K1 : BAND * C::K2) * 2;
    static constexpr int HCH = C::ROWS * 128;               // bytes of the [ROWS x 64] bf16 hidden chunk
    static constexpr int LDS = HCH + BAND_NSLOT * SLOT;
    static_assert((4 / C::WC) * C::TM * 32 == C::ROWS && C::WC * C::TN1 * 32 == 128 && C::WC * C::TN2 * 32 == BAND, "the waves tile both products");
    static_assert(PA * 4 * 1024 == 128 * C::K1 * 2 && PB * 4 * 1024 == BAND * C::K2 * 2, "the waves share the pieces evenly");
};
static_assert(BandGeom<192>::LDS == 152 * 1024 && BandGeom<192>::SLOT == 16384 && BandGeom<192>::NL == 5, "hidden chunk 24 KB + 8 slots of 16 KB");
static_assert(BandGeom<96>::LDS == 128 * 1024 && BandGeom<96>::SLOT == 12288 && BandGeom<96>::NL == 4, "hidden chunk 32 KB + 8 slots of 12 KB");

// The counted wait of step s of a chunk (s = 0 .. NL - 1): step s multiplies load s; the NSLOT - 2 loads behind it (already issued) may stay
// in flight - their DMA pieces per wave, summed over the cyclic pattern of a chunk's loads (PA x NA, then PB x NB).
template <class G> constexpr int band_pieces_ahead(int s) {
    int n = 0;
    for (int i = 1; i <= BAND_NSLOT - 2; ++i) n += (s + i) % G::NL < G::NA ? G::PA : G::PB;
    return n;
}
constexpr int band_wait192(int s) { return band_pieces_ahead<BandGeom<192>>(s); }
constexpr int band_wait96(int s) { return band_pieces_ahead<BandGeom<96>>(s); }
static_assert(band_wait192(0) == 22 && band_wait192(1) == 22 && band_wait192(2) == 21 && band_wait192(3) == 21 && band_wait192(4) == 22, "pattern A4 A4 A4 B3 B3");
static_assert(band_wait96(0) == 13 && band_wait96(1) == 14 && band_wait96(2) == 14 && band_wait96(3) == 13, "pattern A2 A2 A2 B3");

// element offset of a lane's DMA piece i (of P per wave) inside a [4 P x 512 / K rows][K] slab of a matrix of row pitch ld: TileFeed's piece
// order and source-side swizzle (gemm_tile.h), as a 32-bit offset from one uniform base.
// (One piece per call: filling the caller's array through a reference cost the 96-channel instance 4 VGPRs - the compiler no longer
//  saw its second w13 piece as the first plus a constant and kept two 64-bit offsets.)
template <int K, int P> __device__ __forceinline__ int band_piece_offset(int i, int ld, int wave, int lane) {
    constexpr int CH = K / 8, RPP = 64 / CH;
    const int r = RPP * (wave * P + i) + lane / CH;
    return r * ld + (((lane % CH) ^ tile_swz<K>(r)) << 3);
}

template <int BAND, bool HOIST>      // HOIST: see staged_epilogue; only where the geometry takes that epilogue
__global__ void __launch_bounds__(NTHREADS) band_ffn_kernel(const BandDev p) {
    using G = BandGeom<BAND>;
    using std::integral_constant;
    static_assert(G::STAGED || !HOIST, "HOIST is a form of the staged epilogue");
    constexpr int NSLOT = BAND_NSLOT;
    extern __shared__ __attribute__((aligned(16))) unsigned char bl[];
    unsigned char* Hs = bl;
    unsigned char* ring = bl + G::HCH;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> (G::WC >> 1), wc = wave & (G::WC - 1);        // WC = 1 or 2
    const int frow = lane & 31, fk = lane >> 5;
    // XCD x handles band x % E (the band's 590 KB of weights stay in that XCD's L2), two XCDs per band at E = 4
    const int L = blockIdx.x;
    const int e = (L & 7) % p.E;
    const int rt = (L >> 3) * (8 / p.E) + (L & 7) / p.E;
    const int row0 = rt * G::ROWS;
    if (row0 >= p.M) return;
    const int rows_end = p.M;
    unsigned long long tq0 = 0, tq1 = 0, tq2 = 0;
    if constexpr (G::TRACE) { if (p.ep.trace) tq0 = __builtin_amdgcn_s_memtime(); }

    bf16x8 ay[G::TM][G::KY];         // the register-resident token fragments
#pragma unroll
    for (int i = 0; i < G::TM; ++i) {
        int row = row0 + wr * G::TM * 32 + i * 32 + frow;
        if (row >= rows_end) row = row0;
        const bf16_t* src = p.Y + (int64_t)row * p.ldy + e * BAND + fk * 8;
#pragma unroll
        for (int kk = 0; kk < G::KY; ++kk) ay[i][kk] = *reinterpret_cast<const bf16x8*>(src + kk * 16);
    }
    const bf16_t* w13 = p.W13 + (int64_t)e * 2 * p.H * BAND;
    const bf16_t* w2 = p.W2 + (int64_t)e * BAND * p.H;
    int a_off[G::PA], b_off[G::PB];  // this lane's DMA pieces inside a w13 K-slab / a w2 load
#pragma unroll
    for (int i = 0; i < G::PA; ++i) a_off[i] = band_piece_offset<G::K1, G::PA>(i, BAND, wave, lane);
#pragma unroll
    for (int i = 0; i < G::PB; ++i) b_off[i] = band_piece_offset<G::K2, G::PB>(i, p.H, wave, lane);
    const int nchunk = p.H / 64;
    const int nload = nchunk * G::NL;
    auto issue = [&](int q) {        // load q = load q % NL of chunk q / NL -> slot q % NSLOT
        unsigned char* dst = ring + (q & (NSLOT - 1)) * G::SLOT;
        while (q >= nload) q -= G::NL;            // past the end: reload the same-typed piece of the last chunk into a dead slot, so
                                                  // every step sees the piece counts its counted vmcnt assumes
        // (NL = 4 as a shift: q >= 0, but the compiler does not know it, and a signed q / 4 leaves t a run-time value - a branch on the
        //  load type in every step where the shift lets it fold t)
        const int hc = G::NL == 4 ? q >> 2 : q / G::NL, t = q - hc * G::NL;
        if (t < G::NA) {
            const bf16_t* src = w13 + (int64_t)hc * 128 * BAND + t * G::K1;
#pragma unroll
            for (int i = 0; i < G::PA; ++i)
                __builtin_amdgcn_global_load_lds((glb_ptr_t)(src + a_off[i]), (lds_ptr_t)(dst + (wave * G::PA + i) * 1024), 16, 0, 0);
        } else {
            const bf16_t* src = w2 + hc * 64 + (t - G::NA) * G::K2;
#pragma unroll
            for (int i = 0; i < G::PB; ++i)
                __builtin_amdgcn_global_load_lds((glb_ptr_t)(src + b_off[i]), (lds_ptr_t)(dst + (wave * G::PB + i) * 1024), 16, 0, 0);
        }
    };
#pragma unroll
    for (int q = 0; q < NSLOT - 1; ++q) issue(q);

    f32x16 acc1[G::TM][G::TN1], acc2[G::TM][G::TN2];
    acc_zero(acc1);
    acc_zero(acc2);
    // step s of chunk hc multiplies load q = hc NL + s; loads q+1 .. q+6 stay in flight
    auto step_begin = [&](int q, auto s) -> const unsigned char* {
        wait_vmcnt<band_pieces_ahead<G>(decltype(s)::value)>();
        __builtin_amdgcn_s_waitcnt(0xc07f);       // own LDS writes (SwiGLU chunk) done before the barrier publishes them
        __builtin_amdgcn_s_barrier();             // load q landed everywhere; everyone is done with load q-1's slot
        issue(q + NSLOT - 1);                     // -> slot (q-1) % NSLOT
        return ring + (q & (NSLOT - 1)) * G::SLOT;
    };
    // fragment reads run one k-step ahead of the MFMAs that use them (one wave per SIMD: an LDS round trip in front of every batch of
    // six MFMAs was as long as the batch)
    auto phase_a = [&](int kc, const unsigned char* Bs) {        // K-slab kc of w13 against ay
        bf16x8 bf[2][G::TN1];
        frag_load<G::TN1, G::K1>(Bs, wc * G::TN1 * 32, 0, fk, frow, bf[0]);
#pragma unroll
        for (int ks = 0; ks < G::K1 / 16; ++ks) {
            if (ks + 1 < G::K1 / 16) frag_load<G::TN1, G::K1>(Bs, wc * G::TN1 * 32, ks + 1, fk, frow, bf[(ks + 1) & 1]);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < G::TM; ++i) mfma_row(ay[i][kc * (G::K1 / 16) + ks], bf[ks & 1], acc1[i]);
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    auto phase_b = [&](int kb, const unsigned char* Bs) {        // hidden chunk (64-deep rows), its k part kb, against w2 load kb (K2-deep rows)
        bf16x8 af[2][G::TM], bf[2][G::TN2];
        auto rd = [&](int ks, int slot) {
            frag_load<G::TM, 64>(Hs, wr * G::TM * 32, kb * (G::K2 / 16) + ks, fk, frow, af[slot]);
            frag_load<G::TN2, G::K2>(Bs, wc * G::TN2 * 32, ks, fk, frow, bf[slot]);
        };
        rd(0, 0);
#pragma unroll
        for (int ks = 0; ks < G::K2 / 16; ++ks) {
            if (ks + 1 < G::K2 / 16) rd(ks + 1, (ks + 1) & 1);
            __builtin_amdgcn_sched_barrier(0);
            mfma_step(af[ks & 1], bf[ks & 1], acc2);
            __builtin_amdgcn_sched_barrier(0);
        }
    };
#pragma unroll 1
    for (int hc = 0; hc < nchunk; ++hc) {
        const int q0 = hc * G::NL;
        static_for<0, G::NA>([&](auto s) {
            const unsigned char* Bs = step_begin(q0 + s, s);
            if constexpr (G::TRACE && s == 0) { if (hc == 0 && p.ep.trace) tq1 = __builtin_amdgcn_s_memtime(); }
            phase_a(s, Bs);
        });
        {
            // SwiGLU on the interleaved (w1, w3) column pairs -> this chunk's hidden values, bf16, as the next A operand
            typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
#pragma unroll
            for (int i = 0; i < G::TM; ++i)
#pragma unroll
                for (int j = 0; j < G::TN1; ++j)
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int row = wr * G::TM * 32 + i * 32 + frow;
                        const int h0 = wc * G::TN1 * 16 + j * 16 + q * 4 + fk * 2;
                        bf16x2 hv;
                        hv[0] = f2bf(silu_f(acc1[i][j][q * 4 + 0]) * acc1[i][j][q * 4 + 1]);
                        hv[1] = f2bf(silu_f(acc1[i][j][q * 4 + 2]) * acc1[i][j][q * 4 + 3]);
                        *reinterpret_cast<bf16x2*>(Hs + lds_off_t<64>(row, h0 >> 3) + (h0 & 7) * 2) = hv;
#pragma unroll
                        for (int r = 0; r < 4; ++r) acc1[i][j][q * 4 + r] = 0.f;
                    }
        }
        static_for<0, G::NB>([&](auto kb) { phase_b(kb, step_begin(q0 + G::NA + kb, integral_constant<int, G::NA + kb>())); });
    }
    wait_vmcnt<0>();                              // the dummy tail loads
    if constexpr (G::TRACE) { if (p.ep.trace) tq2 = __builtin_amdgcn_s_memtime(); }
    // gated residual: h[:, band e] += gate * z   (same epilogue as the unfused w2 GEMM; LDS is free now)
    if constexpr (G::STAGED) staged_epilogue<EPI_RESID_GATE, G::TM, G::TN2, G::WC, NTHREADS, HOIST>(p.ep, e, acc2, reinterpret_cast<float*>(bl), row0, rows_end, 0, tid, wr, wc, frow, fk);
    else wave_epilogue<EPI_RESID_GATE, G::TM, G::TN2>(p.ep, e, acc2, row0 + wr * G::TM * 32, rows_end, 0, frow, fk);
    if constexpr (G::TRACE) {
        if (p.ep.trace && tid == 0) {
            __builtin_amdgcn_s_waitcnt(0);
            unsigned long long* tr = p.ep.trace + (size_t)blockIdx.x * 4;
            tr[0] = tq0; tr[1] = tq1; tr[2] = tq2; tr[3] = __builtin_amdgcn_s_memtime();
        }
    }
}

int band_ffn_tile_rows(int band) { return band == 192 ? BandGeom<192>::ROWS : BandGeom<96>::ROWS; }

template <int BAND, bool HOIST> static int band_ffn_launch(const BandDev& d, hipStream_t st) {
    using G = BandGeom<BAND>;
    const int nblk = cdiv(cdiv(d.M, G::ROWS), 8 / d.E) * 8;       // 8 / E row tiles per group of 8 consecutive blocks (one per XCD)
    static OnceFlags attr;
    vb_set_max_lds_once(attr, reinterpret_cast<const void*>(band_ffn_kernel<BAND, HOIST>), G::LDS);
    hipLaunchKernelGGL((band_ffn_kernel<BAND, HOIST>), dim3(nblk), dim3(NTHREADS), G::LDS, st, d);
    VB_CHECK_LAUNCH();
    return VB_OK;
}
int launch_band_ffn(const BandFfnArgs& a, hipStream_t st) {
    if ((a.band != 192 && a.band != 96) || a.H % 64 || (8 % a.E) || a.E > 8) VB_FAIL(VB_E_INVALID, "band_ffn: band=%d H=%d E=%d unsupported", a.band, a.H, a.E);
    BandDev d;
    memset(&d, 0, sizeof(d));
    d.Y = a.y; d.ldy = a.ldy; d.W13 = a.w13; d.W2 = a.w2; d.M = a.M; d.H = a.H; d.E = a.E;
    d.ep.out32 = a.out32; d.ep.ldc32 = a.ldc32; d.ep.gate = a.gate; d.ep.gate_ld = a.gate_ld; d.ep.T = a.T > 0 ? a.T : 1;
    d.ep.rT = 1.0f / (float)d.ep.T; d.ep.rhd = 1.f; d.ep.rD = 1.f; d.ep.hd = 1; d.ep.D = 1;
    d.ep.c_noff_group = a.band; d.ep.N = a.band; d.ep.M = a.M; d.ep.trace = g_gemm_trace;
    if (a.M >= (1 << 21)) VB_FAIL(VB_E_INVALID, "band_ffn: M exceeds fdiv()");
    ProfScope prof(0, 2.0 * a.M * a.E * ((double)2 * a.H * a.band + (double)a.band * a.H),
                   (double)a.M * a.E * a.band * (2.0 + 8.0) + (double)a.E * 3.0 * a.H * a.band * 2.0, st);
    if (a.band == 96) return band_ffn_launch<96, false>(d, st);
    return vb_tune().band_epi_old ? band_ffn_launch<192, false>(d, st) : band_ffn_launch<192, true>(d, st);
}
