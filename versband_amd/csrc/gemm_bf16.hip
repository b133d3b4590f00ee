// bf16 MFMA GEMM for the DiT (gfx950):  C[m][n] = sum_k A[m][k] * B[n][k], fp32 accumulation, epilogues EPI_* (kernels.h).
// Every kernel walks K in the same 16-deep MFMA steps and shares the epilogue arithmetic (gemm_dev.h), so the routes are bit-identical.
// launch_gemm (end of the file) = gemm_fill -> gemm_route -> gemm_grid -> launch; which kernel serves which GemmRoute:
//   GEMM_T128          128 x 128, two workgroups per CU: gemm_bf16_glds_kernel (tile DMA, K % 32 == 0; P16 layout for QKV + RoPE / SwiGLU),
//                      gemm_bf16_kernel (register-staged) for any other K                                        -> launch_t
//   GEMM_WIDE_RESID    128 x 192, two per CU, plain gated residual: gemm_bf16_wide_resid_kernel
//   GEMM_BIG_192       192 x 192, one per CU: gemm_bf16_big_kernel<3, 3>                                          -> launch_big
//   GEMM_SMALL_64      64 x 64 (one or two clips, conv-as-GEMM at small batches): gemm_bf16_big_kernel<1, 1>      -> launch_big
//   GEMM_SMALL_128x64  128 x 64 (VB_GEMM_SMALL=21): gemm_bf16_big_kernel<2, 1>                                    -> launch_big
//   GEMM_P8            256 x 256, 8 waves, P16 epilogues (QKV + RoPE, routed SwiGLU): gemm_bf16_p8_kernel         -> launch_p8_product
//   experiments build: GEMM_P8_VARIANT (other schedules / epilogues of the 8-wave kernel, launch_p8), GEMM_PK / GEMM_PK_F32 (persistent
//                      kernel, gemm_bf16_pk.hip)
// What the main loops share - tile walk, LDS tile image and swizzle, DMA feed, k-tile offsets, the MFMA step - is gemm_tile.h; a kernel
// body here is its schedule.  The fused Band-MoE kernels built from the same pieces are in band_ffn.hip.
#include "gemm_tile.h"

#define P8_MIN_TILES 96     // selection threshold of the 8-wave 256 x 256 kernel (tiles of the launch)

// ---- register-staged 128 x 128 kernel (any K % 8 == 0) ----------------------------------------------------------------
//
//  * 128x128x64 block tile, 256 threads = 4 waves (2x2), each wave 64x64 as 2x2
//    v_mfma_f32_32x32x16_bf16 tiles, fp32 accumulation.
//  * Both operands are K-contiguous; tiles are register-staged into the XOR-swizzled
//    LDS image of gemm_tile.h (lds_off_t), zero-filled past K and past the last row.
//  * LDS is double buffered: global loads of tile t+1 are in flight while the MFMAs
//    of tile t run; one barrier per K tile.
//  * The MFMA is issued "swapped" (weights as the A operand) so a lane owns one
//    output ROW m and 4 consecutive output COLUMNS per accumulator quad: pairwise
//    epilogues (RoPE, SwiGLU) are lane-local and stores are 8-16 B per lane.
//  * nseg == 3 is the split-precision mode: the K loop walks (A_hi,B_hi), (A_lo,B_hi),
//    (A_hi,B_lo) - three bf16 passes give fp32-class products.
//  * Grouped problems (Band-MoE experts): the grid's y index walks the m-tiles of all
//    groups; group row ranges come from a device array written by the bucket kernel.
template <int EPI>
__global__ void __launch_bounds__(NTHREADS) gemm_bf16_kernel(const GemmDev p) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[2][2][BM * BK * 2];   // [buf][A/B][16 KB]

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1;

    int g, row0, rows_end, n0;
    if (!gemm_tile_pos<BM, BN, TILE_GROUPS>(p, g, row0, rows_end, n0)) return;
    const int K = p.K;
    const int KT = (K + BK - 1) / BK;
    const int total = KT * p.nseg;

    // ---- per-thread global load slots: 4 chunks of A, 4 chunks of B ----------------
    const bf16_t* aptr[4]; const bf16_t* bptr[4]; bool aval[4], bval[4]; int lds_w[4];
    const int cch = tid & 7;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        int r = (tid >> 3) + i * 32;
        int slot = row0 + r;
        aval[i] = slot < rows_end;
        int arow = aval[i] ? (p.a_rows ? p.a_rows[slot] : slot) : 0;
        aptr[i] = p.A + (int64_t)arow * p.lda + g * p.a_koff_group + cch * 8;
        int nrow = n0 + r;
        bval[i] = nrow < p.N;
        bptr[i] = p.B + g * p.b_group_stride + (int64_t)(bval[i] ? nrow : 0) * p.ldb + cch * 8;
        lds_w[i] = lds_off_t<BK>(r, cch);
    }

    f32x16 acc[2][2];
    acc_zero(acc);

    uint4 ra[4], rb[4];
    auto gload = [&](int t) {
        int seg = t / KT;
        int k0 = (t - seg * KT) * BK;
        int64_t ao = (seg == 1) ? p.a_plane : 0;
        int64_t bo = (seg == 2) ? p.b_plane : 0;
        bool kin = (k0 + cch * 8) < K;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            ra[i] = (aval[i] && kin) ? *reinterpret_cast<const uint4*>(aptr[i] + ao + k0) : make_uint4(0, 0, 0, 0);
            rb[i] = (bval[i] && kin) ? *reinterpret_cast<const uint4*>(bptr[i] + bo + k0) : make_uint4(0, 0, 0, 0);
        }
    };
    auto lstore = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            *reinterpret_cast<uint4*>(&lds[buf][0][lds_w[i]]) = ra[i];
            *reinterpret_cast<uint4*>(&lds[buf][1][lds_w[i]]) = rb[i];
        }
    };

    gload(0);
    lstore(0);
    __syncthreads();

    const int frow = lane & 31, fk = lane >> 5;
    for (int t = 0; t < total; ++t) {
        const int buf = t & 1;
        if (t + 1 < total) gload(t + 1);
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            // (this kernel's own fragment read, A and B alternating: through frag_load - A's fragments, then B's - every instance gained
            //  four s_waitcnt between its MFMAs and 4 VGPRs)
            bf16x8 af[2], bf[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                af[i] = *reinterpret_cast<const bf16x8*>(&lds[buf][0][lds_off_t<BK>(wr * 64 + i * 32 + frow, ks * 2 + fk)]);
                bf[i] = *reinterpret_cast<const bf16x8*>(&lds[buf][1][lds_off_t<BK>(wc * 64 + i * 32 + frow, ks * 2 + fk)]);
            }
            mfma_step(af, bf, acc);
        }
        if (t + 1 < total) lstore(buf ^ 1);
        __syncthreads();
    }

    wave_epilogue<EPI>(p, g, acc, row0 + wr * 64, rows_end, n0 + wc * 64, frow, fk);
}

// ---- 128 x 128 tiles DMA'd straight into an LDS ring (gemm_tile.h: TileFeed, source-side swizzle) -----------------------------------
// NST stages: tiles t+1 .. t+NST-1 are in flight while tile t is multiplied; the wait is a COUNTED
// s_waitcnt vmcnt((NST-2)*loads_per_tile) + a raw s_barrier, so the DMA queue is never drained inside the loop.
// Needs K % BKT == 0 (no zero fill on this path); out-of-range rows read a clamped valid row and are never stored.
// ABL (tuning only): 1 = no tile DMA in the loop, 2 = no MFMA, 3 = no LDS fragment reads
template <int EPI, int BKT, int NST, int ABL = 0, bool P16 = false>
__global__ void __launch_bounds__(NTHREADS) __attribute__((amdgpu_waves_per_eu(BKT * NST == 96 ? 3 : 1, BKT * NST == 96 ? 3 : 8)))
gemm_bf16_glds_kernel(const GemmDev p) {
    static_assert(!P16 || EPI == EPI_QKV_ROPE || EPI == EPI_SWIGLU, "the P16 column layout is wired for the QKV + RoPE and SwiGLU epilogues");
    using Feed = TileFeed<BM, BN, BKT, 4>;
    constexpr int LPT = Feed::LPT, OPB = Feed::ABYTES;
    __shared__ __attribute__((aligned(16))) unsigned char lds[NST * Feed::STAGE];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 1, wc = wave & 1;
    unsigned long long t_start = 0;
    if constexpr (EPI == EPI_F32) { if (p.trace) t_start = __builtin_amdgcn_s_memtime(); }

    int g, row0, rows_end, n0;
    if (!gemm_tile_pos<BM, BN, TILE_UNIFORM_XCD>(p, g, row0, rows_end, n0)) return;
    const int KT = (ABL == 5) ? 0 : p.K / BKT;
    const int total = KT * p.nseg;
    // QKV, P16: a tile of the V third exchanges the operands' roles (see wave_epilogue_vt_p16) - the permutation then belongs to the TOKEN rows
    bool vsec = false;
    if constexpr (P16 && EPI == EPI_QKV_ROPE) vsec = n0 >= 2 * p.D && (p.T & 15) == 0 && (p.Tpad & 7) == 0 && !p.no_vt16;       // (16-byte V^T stores: T and the padded pitch)

    const bf16_t* asrc[Feed::PA]; const bf16_t* bsrc[Feed::PB];
    gemm_feed_setup<EPI, Feed>(p, g, row0, rows_end, n0, vsec, P16 && !vsec, wave, lane, asrc, bsrc);
    auto issue = [&](int t) {
        int64_t ao, bo;
        gemm_k_offsets<EPI, BKT>(p, t, KT, ao, bo);
        Feed::issue(asrc, bsrc, wave, lds + (t % NST) * Feed::STAGE, ao, bo, 0, Feed::PA);
    };

    f32x16 acc[2][2];
    acc_zero(acc);

#pragma unroll
    for (int t = 0; t < NST - 1; ++t)
        if (t < total) issue(t);
    const int frow = lane & 31, fk = lane >> 5;
    for (int t = 0; t < total; ++t) {
        const int st = t % NST;
        // tiles t+1 .. min(total-1, t+NST-2) may stay in flight
        const int ahead = min(total - 1, t + NST - 2) - t;
        if (NST >= 4 && ahead >= 2) wait_vmcnt<2 * LPT>();
        else if (NST >= 3 && ahead >= 1) wait_vmcnt<LPT>();
        else wait_vmcnt<0>();
        __builtin_amdgcn_s_barrier();           // tile t landed everywhere; everyone finished reading stage (t-1)%NST
        if (ABL != 1 && t + NST - 1 < total) issue(t + NST - 1);
        // (V third of QKV: the weight tile plays the token tile's part and vice versa - a uniform pointer exchange, same code)
        const unsigned char* As = &lds[(st * 2 + (vsec ? 1 : 0)) * OPB];
        const unsigned char* Bs = &lds[(st * 2 + (vsec ? 0 : 1)) * OPB];
        // fragment reads are software-pipelined in registers: the ds_reads of k-step ks+1 are issued before the MFMAs of
        // k-step ks (the compiler otherwise reuses one register set and serialises read -> wait -> 4 MFMA per k-step)
        bf16x8 af[2][2], bf[2][2];
        auto fload = [&](int ks, int slot) {
            if constexpr (ABL == 3) {
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int e = 0; e < 8; ++e) { af[slot][i][e] = (bf16_t)(float)(t + e); bf[slot][i][e] = (bf16_t)(float)(ks + e); }
            } else {
                frag_load<2, 2, BKT>(As, Bs, wr * 64, wc * 64, ks, fk, frow, af[slot], bf[slot]);
            }
        };
        fload(0, 0);
#pragma unroll
        for (int ks = 0; ks < BKT / 16; ++ks) {
            const int cur = ks & 1;
            if (ks + 1 < BKT / 16) fload(ks + 1, cur ^ 1);
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (ABL == 2) {
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j)
#pragma unroll
                        for (int e = 0; e < 8; ++e) acc[i][j][e] += (float)af[cur][i][e] * (float)bf[cur][j][e];
            } else {
                mfma_step(af[cur], bf[cur], acc);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    }

    unsigned long long t_loop = 0;
    if constexpr (EPI == EPI_F32) { if (p.trace) t_loop = __builtin_amdgcn_s_memtime(); }
    if constexpr (ABL == 4) {
        float sink = 0.f;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) sink += acc[i][j][0] + acc[i][j][9];
        if (sink == 12345.678f) p.out32[0] = sink;
    } else {
        // (conv-as-GEMM, EPI_F32_CT: a channel-major epilogue staged through LDS - 16-byte residual loads and stores - measured the same
        //  as the direct 4-byte one, 234 vs 230 us per VAE layer: these launches are mainloop-bound at K = 1920 .. 7680; not kept)
        if constexpr (P16 && EPI == EPI_QKV_ROPE) {
            if (vsec) wave_epilogue_vt_p16<2, 2>(p, acc, n0 + wr * 64, row0 + wc * 64, rows_end, frow, fk);
            else wave_epilogue_qkv_p16<2, 2>(p, acc, row0 + wr * 64, rows_end, n0 + wc * 64, frow, fk);
        }
        else if constexpr (P16 && EPI == EPI_SWIGLU) wave_epilogue_swiglu_p16<2, 2>(p, g, acc, row0 + wr * 64, rows_end, n0 + wc * 64, frow, fk);
        else if constexpr (STAGED_EPI(EPI)) staged_epilogue<EPI, 2, 2>(p, g, acc, reinterpret_cast<float*>(lds), row0, rows_end, n0, tid, wr, wc, frow, fk);
        else wave_epilogue<EPI>(p, g, acc, row0 + wr * 64, rows_end, n0 + wc * 64, frow, fk);
    }
    if constexpr (EPI == EPI_F32) gemm_trace_write(p, t_start, t_start, t_loop);       // (no prologue timestamp in this kernel)
}

// ---- 128 x 192 tiles, two workgroups per CU, gated-residual epilogue in the P16 layout (attention out-proj at >= 8 clips) ----------
// 12032 x 768 makes 564 tiles of 128 x 128 (1.1 rounds of the 512 two-per-CU slots, priced as 2) and 252 of 192 x 192 on the one-per-CU
// kernel, whose tiles all reach their read-modify-write epilogue together (39.8 us, 12.4 % MFMA-busy).  128 x 192 tiles make 376
// workgroups = ONE round at two per CU (80 KB of LDS each): the co-resident workgroup overlaps the other's epilogue, and the P16 layout
// gives a lane 16 consecutive fp32 columns (four 16-byte loads of h, four of the gate row, four stores).  Same k order and epilogue
// arithmetic as every other tile configuration (test_gemm_tile_configurations_round_alike).
// (Round 3, built, measured and removed - verdict item 1c: the Band-MoE input RMSNorm fused into this launch by "last arriver": every
//  workgroup publishes its stores with an agent-scope release, bumps its row panel's counter, and the workgroup that lands the panel's
//  last column tile normalises the 128 rows.  Bit-identical to the separate launch, no spinning, no placement assumed - and the
//  agent-scope release is a buffer_wbl2 per workgroup: 36 -> 202 us per launch (1272 -> 1155 mel-s/s).  Dropping the release would
//  lean on all column tiles of a panel sharing one XCD's L2, which the programming model does not promise.  The tail's registers also
//  slowed the un-fused path of the same kernel, 36 -> 55 us.)
template <int TN>
__global__ void __launch_bounds__(NTHREADS) __attribute__((amdgpu_waves_per_eu(2, 2))) gemm_bf16_wide_resid_kernel(const GemmDev p) {
    constexpr int BKT = 64, NST = 2;
    constexpr int BNP = 64 * TN;
    using Feed = TileFeed<BM, BNP, BKT, 4>;
    __shared__ __attribute__((aligned(16))) unsigned char lds[NST * Feed::STAGE];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 1, wc = wave & 1;
    int g, row0, rows_end, n0;
    if (!gemm_tile_pos<BM, BNP, TILE_UNGROUPED>(p, g, row0, rows_end, n0)) return;
    const int KT = p.K / BKT;
    const int total = KT * p.nseg;

    // (plain rows of both operands: this kernel is launched without groups or gathered rows, gemm_wide_resid_shape)
    const bf16_t* asrc[Feed::PA]; const bf16_t* bsrc[Feed::PB];
    Feed::rows(asrc, p.A, p.lda, row0, rows_end, row0, false, wave, lane, [](int r) { return r; });
    Feed::rows(bsrc, p.B, p.ldb, n0, p.N, 0, true, wave, lane, [](int r) { return r; });
    auto issue = [&](int t) {
        int64_t ao, bo;
        gemm_k_offsets<EPI_RESID_GATE, BKT>(p, t, KT, ao, bo);
        Feed::issue(asrc, bsrc, wave, lds + (t % NST) * Feed::STAGE, ao, bo);
    };
    f32x16 acc[2][TN];
    acc_zero(acc);
    const int frow = lane & 31, fk = lane >> 5;
    gemm_walk_2stage<Feed>(lds, total, issue, wr * 64, wc * 32 * TN, fk, frow, acc);
    // epilogue (EPI_RESID_GATE): out32[m][n..n+15] = fmaf(gate[clip(m)][n..], v, out32[m][n..]); loads of a row slab first, then the stores
    // (round 3, measured and dropped: both row slabs' residual values requested together - 248 VGPRs, 38.4 against 36.6 us)
    {
#pragma clang fp contract(off)
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int m = row0 + wr * 64 + i * 32 + frow;
            if (m >= rows_end) continue;
            float* hrow = p.out32 + (int64_t)m * p.ldc32;
            const float* grow = p.gate + (int64_t)fdiv(m, p.rT) * p.gate_ld;
            float4 hv[TN][4], gv[TN][4];
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const int n = n0 + wc * 32 * TN + j * 32 + fk * 16;
                if (n < p.N) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        hv[j][q] = *reinterpret_cast<const float4*>(hrow + n + 4 * q);
                        gv[j][q] = *reinterpret_cast<const float4*>(grow + n + 4 * q);
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const int n = n0 + wc * 32 * TN + j * 32 + fk * 16;
                if (n >= p.N) continue;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    float4 o;
                    o.x = fmaf(gv[j][q].x, acc[i][j][4 * q + 0], hv[j][q].x); o.y = fmaf(gv[j][q].y, acc[i][j][4 * q + 1], hv[j][q].y);
                    o.z = fmaf(gv[j][q].z, acc[i][j][4 * q + 2], hv[j][q].z); o.w = fmaf(gv[j][q].w, acc[i][j][4 * q + 3], hv[j][q].w);
                    *reinterpret_cast<float4*>(hrow + n + 4 * q) = o;
                }
            }
        }
    }
}

// ---- gemm_bf16_big_kernel: (64 TM) x (64 TN) block tiles, 192 x 192 at one workgroup per CU ---------------------------------------
// Per-block traces of the 128x128 kernel (tools/gemm_trace.py) show a k-iteration costs ~1500 cycles against 640 cycles
// of MFMA: every iteration moves 32 KB through the CU's 64 B/clk vector-memory path (512 cycles at best) and waits for
// the tile issued one iteration earlier, and a launch of M=12032 x N=768 leaves 2.2 tiles per CU (priced as 3).  This
// kernel raises the flops per byte DMA'd and fits the tile grid to the 256 CUs instead:
//   * block tile (64 TM) x (64 TN), 4 waves as 2x2, a wave owns (32 TM) x (32 TN) = TM x TN MFMA 32x32 tiles;
//     192x192 (TM = TN = 3) moves 48 KB per 1440 MFMA cycles and makes 63 x 4 = 252 tiles of 12032 x 768;
//   * BK = 64, NSTB-stage LDS ring filled by global_load_lds (same lane-linear image + source-side XOR swizzle as
//     above), counted vmcnt waits: NSTB-1 tiles in flight;
//   * fragment reads double-buffered in registers across the 4 k-steps of a tile;
//   * epilogue staged through LDS (free after the loop): a slab of 64 rows x BN goes to LDS as fp32, is read back
//     row-major so a lane owns 4 consecutive columns AND a wave covers whole 128-B lines - residual/bias loads and all
//     stores become full-line transactions (the MFMA layout stores 32-B pieces of 32 different rows per instruction).
// ABL (tuning only): 1 = no tile DMA inside the loop, 2 = no MFMA, 3 = no fragment reads
template <int EPI, int TM, int TN, int NSTB, int ABL = 0>
__global__ void __launch_bounds__(NTHREADS) gemm_bf16_big_kernel(const GemmDev p) {
    constexpr int BMB = 64 * TM, BNB = 64 * TN;
    using Feed = TileFeed<BMB, BNB, 64, 4>;
    constexpr int LPT = Feed::LPT, ABYTES = Feed::ABYTES, STAGE = Feed::STAGE;
    extern __shared__ __attribute__((aligned(16))) unsigned char ldsb[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 1, wc = wave & 1;
    unsigned long long t_start = 0, t_pro = 0, t_loop = 0;
    if constexpr (EPI == EPI_F32) { if (p.trace) t_start = __builtin_amdgcn_s_memtime(); }

    int g, row0, rows_end, n0;
    if (!gemm_tile_pos<BMB, BNB, TILE_UNIFORM>(p, g, row0, rows_end, n0)) return;
    const int KT = p.K / 64;
    const int total = KT * p.nseg;

    const bf16_t* asrc[Feed::PA]; const bf16_t* bsrc[Feed::PB];
    gemm_feed_setup<EPI, Feed>(p, g, row0, rows_end, n0, false, false, wave, lane, asrc, bsrc);
    auto issue = [&](int t) {
        int64_t ao, bo;
        gemm_k_offsets<EPI, 64>(p, t, KT, ao, bo);
        Feed::issue(asrc, bsrc, wave, ldsb + (t % NSTB) * STAGE, ao, bo);
    };

    f32x16 acc[TM][TN];
    acc_zero(acc);

    // Software pipeline across tiles (NSTB = 3 stages, 2 tiles of DMA in flight):
    //   a tile's LAST fragment set (k-step 3) is read into registers during k-step 2, so its stage is dead at the
    //   "boundary" inside iteration t: [lgkmcnt(0)] [tile t+1 landed] [barrier] -> read k-step 0 of tile t+1, queue the
    //   k-step-3 MFMAs of tile t, and refill stage t%3 with tile t+3 while they run.  LDS latency, the barrier and the DMA
    //   issue of a tile boundary all sit in the shadow of 9 MFMAs instead of in front of them.
    static_assert(NSTB == 3, "pipeline written for a 3-stage ring");
#pragma unroll
    for (int t = 0; t < NSTB; ++t)
        if (t < total) issue(t);
    const int frow = lane & 31, fk = lane >> 5;
    bf16x8 af[2][TM], bf[2][TN];
    auto fload = [&](int st, int ks, int slot) {
        const unsigned char* As = ldsb + st * STAGE;
        const unsigned char* Bs = As + ABYTES;
        if constexpr (ABL == 3) {
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int e = 0; e < 8; ++e) af[slot][i][e] = (bf16_t)(float)(st + e + i);
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int e = 0; e < 8; ++e) bf[slot][j][e] = (bf16_t)(float)(ks + e + j);
            return;
        }
        frag_load<TM, TN, 64>(As, Bs, wr * 32 * TM, wc * 32 * TN, ks, fk, frow, af[slot], bf[slot]);
    };
    auto mfmas = [&](int slot) {
        if constexpr (ABL == 2) {
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
#pragma unroll
                    for (int e = 0; e < 2; ++e) acc[i][j][e] += (float)af[slot][i][e] * (float)bf[slot][j][e];
        } else {
            mfma_step(af[slot], bf[slot], acc);
        }
    };
    if (total > 2) wait_vmcnt<2 * LPT>();
    else if (total > 1) wait_vmcnt<LPT>();
    else wait_vmcnt<0>();
    __builtin_amdgcn_s_barrier();
    if (total > 0) fload(0, 0, 0);
    if constexpr (EPI == EPI_F32) { if (p.trace) t_pro = __builtin_amdgcn_s_memtime(); }
    int st = 0;
    for (int t = 0; t < total; ++t) {
        // k-steps 0..2 (fragments of k-step ks+1 are requested before the MFMAs of ks are queued)
        fload(st, 1, 1);
        __builtin_amdgcn_sched_barrier(0);
        mfmas(0);
        __builtin_amdgcn_sched_barrier(0);
        fload(st, 2, 0);
        __builtin_amdgcn_sched_barrier(0);
        mfmas(1);
        __builtin_amdgcn_sched_barrier(0);
        fload(st, 3, 1);
        __builtin_amdgcn_sched_barrier(0);
        mfmas(0);
        __builtin_amdgcn_sched_barrier(0);
        // boundary
        const int nst = st == NSTB - 1 ? 0 : st + 1;
        __builtin_amdgcn_s_waitcnt(0xc07f);                 // lgkmcnt(0): k-step 3 fragments are in registers -> stage st is dead
        if (t + 1 < total) {
            if (t + 2 < total) wait_vmcnt<LPT>(); else wait_vmcnt<0>();     // tile t+1 landed (tile t+2 may stay in flight)
        }
        __builtin_amdgcn_s_barrier();
        if (t + 1 < total) fload(nst, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        mfmas(1);
        __builtin_amdgcn_sched_barrier(0);
        if (ABL != 1 && t + NSTB < total) issue(t + NSTB);               // refills stage st
        st = nst;
    }

    if constexpr (EPI == EPI_F32) { if (p.trace) t_loop = __builtin_amdgcn_s_memtime(); }
    // gated residual on the 192 x 192 and 64 x 64 tiles (out-proj / unfused band w2 at 32 clips, long form, one or two clips): residual loads
    // requested before the staging, like the fused band-expert kernel (see staged_epilogue HOIST)
    if constexpr (EPI == EPI_RESID_GATE && ((TM == 3 && TN == 3) || (TM == 1 && TN == 1))) {
        if (!p.epi_old) staged_epilogue<EPI, TM, TN, 2, NTHREADS, true>(p, g, acc, reinterpret_cast<float*>(ldsb), row0, rows_end, n0, tid, wr, wc, frow, fk);
        else staged_epilogue<EPI, TM, TN>(p, g, acc, reinterpret_cast<float*>(ldsb), row0, rows_end, n0, tid, wr, wc, frow, fk);
    } else
    staged_epilogue<EPI, TM, TN>(p, g, acc, reinterpret_cast<float*>(ldsb), row0, rows_end, n0, tid, wr, wc, frow, fk);
    if constexpr (EPI == EPI_F32) gemm_trace_write(p, t_start, t_pro, t_loop);
}

// ---- 256 x 256 tiles, 8 waves (gemm_bf16_p8_kernel).  Round 2 measured it slower inside the DiT (quad-layout epilogues, docs/history.md, round 2) and
// kept it in the experiments build; with the P16 epilogues of round 3 it wins on the two wide projections (round 4, same box:
// QKV + RoPE 65.3 -> 60.7 us, whole two-stream run +3.2 %, two clips 56.8 -> 51.8 ms) and the product library instantiates exactly those
// two forms (software-pipelined schedule, P16 layout; ring shape: launch_p8_product).  The other schedules / ring shapes /
// ablations below compile only with -DVB_EXPERIMENTS (`VB_BUILD_EXPERIMENTS=1 python -m versband_amd.build`) ----
// 256 x 256 tiles, 8 waves in two staggered groups ("ping-pong") ------------------------------------
// What bounds the 4-wave kernels above is the L2 -> LDS feed (52-60 GB/s per CU whatever the ring, section 5 of DESIGN.md): at
// 64 flop per byte DMA'd (128^2) or 96 (192^2) the MFMA pipe idles half the time, and with one wave per SIMD every barrier, DMA
// issue and LDS read of a wave is dead time of its SIMD's matrix pipe.  This kernel
//   * moves 128 flop per byte DMA'd: block tile 256 x 256 (accumulators = half of the CU's register file), 8 waves as 2 (M) x 4
//     (N), a wave owns 128 x 64 = 4 x 2 MFMA 32x32 tiles;
//   * keeps (NST-1) ring stages of [256 + 256 rows] x BKT in flight (BKT = 32: five 32-KB stages = all 160 KB of LDS, 128 KB in
//     flight) with counted vmcnt - never a drain inside the loop;
//   * runs the two waves of every SIMD in OPPOSITE phases: the wave rows (wr = 0 / 1) are staggered by one s_barrier, so while
//     one wave issues its 16 MFMAs of a 32-deep sub-stage (512 matrix-pipe cycles, s_setprio 1) its partner reads the 12
//     fragments of its next sub-stage from LDS, issues its DMA pieces and waits for them - load latency, DMA issue and the
//     barriers sit beside the partner's MFMAs instead of in front of one's own (MI355X_MICROARCH.md, "Two waves per SIMD").
// Barrier algebra (k-th s_barrier of group 0 pairs with the k-th of group 1; group 1 executes one extra barrier first):
//   group 0:  L(0) X M(0) Y L(1) X M(1) Y ...          group 1:  E L(0) X M(0) Y L(1) ...
//   -> g0's X(u) = g1's Y(u-1), g0's Y(u) = g1's X(u).  Stage t is read by g0 in L_g0(t) and by g1 one half-period later; its
//   slot is refilled in the L phase of stage t+1 (both groups are past their reads by then), and "stage t+1 has landed
//   everywhere" is each wave's counted vmcnt in its last L phase of stage t followed by the barrier both groups pass before
//   either reads it.  Past the end the ring keeps issuing dummy reloads into dead slots so the counts stay uniform.
// Accumulation order per output element is the same as in every other variant (k ascending in 16-deep MFMA steps): bit-identical.
// PP = 1: the ping-pong schedule above.  PP = 0: every wave is software-pipelined on its own instead - the fragments of k-step
// ks+1 are requested before the 8 MFMAs of k-step ks are queued, the DMA pieces of the stage NST-1 ahead are issued between those
// MFMAs, ONE barrier per ring stage whose latency (and the next stage's first fragment reads) hides behind the last 8 MFMAs of
// the stage; the two waves of a SIMD are not synchronised against each other and simply fill each other's issue gaps.
// ABL (tuning only, PP = 0): 1 = no DMA inside the loop, 2 = no fragment reads, 3 = no MFMA, 4 = no barrier, 5 = no epilogue
template <int EPI, int BKT, int NST, int PP, int ABL = 0, int STG = 1>
__global__ void __launch_bounds__(512) gemm_bf16_p8_kernel(const GemmDev p) {
    constexpr int BMP = 256, BNP = 256;
    constexpr int NSUB = BKT / 32;                 // 32-deep sub-stages per ring stage
    using Feed = TileFeed<BMP, BNP, BKT, 8>;
    constexpr int OPB = Feed::ABYTES;              // bytes of one operand of a stage
    constexpr int STAGE = Feed::STAGE;
    constexpr int PPW = Feed::PA;                  // 1-KB DMA pieces per wave per operand per stage
    constexpr int LPT = Feed::LPT;                 // DMA instructions per wave per stage
    static_assert(NST >= 2 && (NST - 2) * LPT < 64, "ring depth vs vmcnt range");
    extern __shared__ __attribute__((aligned(16))) unsigned char ldsp[];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 2, wc = wave & 3;

    int g, row0, rows_end, n0;
    if (!gemm_tile_pos<BMP, BNP, TILE_GROUPS>(p, g, row0, rows_end, n0)) return;
    const int KT = p.K / BKT;
    const int total = KT * p.nseg;

    const bf16_t* asrc[PPW]; const bf16_t* bsrc[PPW];
    gemm_feed_setup<EPI, Feed>(p, g, row0, rows_end, n0, false, STG == 2, wave, lane, asrc, bsrc);      // STG = 2: P16 column layout
    // issue state: stage counter, its ring slot and its (segment, k) position - advanced incrementally (scalar adds / selects, no
    // division in the loop); past the last stage the position stays on the last one: dummy reloads into dead slots
    int iss_t = 0, iss_slot = 0, iss_kt = 0, iss_seg = 0;
    auto issue_pieces = [&](int q0, int q1) {           // DMA pieces [q0, q1) of the current issue stage
        int64_t ao, bo;
        gemm_seg_offsets<BKT>(p, iss_seg, iss_kt, ao, bo);
        Feed::issue(asrc, bsrc, wave, ldsp + iss_slot * STAGE, ao, bo, q0, q1);
    };
    auto issue_advance = [&]() {
        iss_t += 1;
        iss_slot = iss_slot == NST - 1 ? 0 : iss_slot + 1;
        if (iss_t < total) {
            iss_kt += 1;
            if (iss_kt == KT) { iss_kt = 0; iss_seg += 1; }
        }
    };
    auto issue = [&]() { issue_pieces(0, PPW); issue_advance(); };

    f32x16 acc[4][2];
    acc_zero(acc);

    // (both schedules read a k-step's two B fragments before its four A fragments: the first MFMA pair waits for three reads, not five)
    const int frow = lane & 31, fk = lane >> 5;
    bf16x8 af[2][4], bf[2][2];
    auto fload = [&](int st, int sub) {
        const unsigned char* As = ldsp + st * STAGE;
        const unsigned char* Bs = As + OPB;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            frag_load<2, BKT>(Bs, wc * 64, sub * 2 + ks, fk, frow, bf[ks]);
            frag_load<4, BKT>(As, wr * 128, sub * 2 + ks, fk, frow, af[ks]);
        }
    };

#pragma unroll
    for (int t = 0; t < NST - 1; ++t) issue();
    wait_vmcnt<(NST - 2) * LPT>();                 // this wave's pieces of stage 0 have landed
    __builtin_amdgcn_s_barrier();
    if constexpr (PP == 0) {
        constexpr int KS = BKT / 16;               // 16-deep k-steps per ring stage
        bf16x8 fa[2][4], fb[2][2];
        auto fload1 = [&](int st_, int ks, int slot) {
            if constexpr (ABL == 2) { if (st_ >= 0) return; }
            const unsigned char* As = ldsp + st_ * STAGE;
            const unsigned char* Bs = As + OPB;
            frag_load<2, BKT>(Bs, wc * 64, ks, fk, frow, fb[slot]);
            frag_load<4, BKT>(As, wr * 128, ks, fk, frow, fa[slot]);
        };
        auto mfma2 = [&](int slot, int i) {
            if constexpr (ABL == 3) {
                acc[i][0][0] += (float)fb[slot][0][0] * (float)fa[slot][i][1];
                acc[i][1][0] += (float)fb[slot][1][2] * (float)fa[slot][i][3];
                return;
            }
            mfma_row(fa[slot][i], fb[slot], acc[i]);
        };
        if constexpr (ABL == 2) {
#pragma unroll
            for (int sl = 0; sl < 2; ++sl) {
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int e = 0; e < 8; ++e) fb[sl][j][e] = (bf16_t)(float)(lane + e + j);
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int e = 0; e < 8; ++e) fa[sl][i][e] = (bf16_t)(float)(lane - e + i);
            }
        }
        if (total > 0) fload1(0, 0, 0);
        int st = 0;
        for (int t = 0; t < total; ++t) {
            const int nst = st == NST - 1 ? 0 : st + 1;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                const int cur = ks & 1;
                if (ks == KS - 1) {
                    // stage boundary: my reads of stage t are in registers; after the barrier stage t+1 is here for everyone and
                    // the slot of stage t may be refilled
                    __builtin_amdgcn_s_waitcnt(0xc07f);
                    if constexpr (ABL != 1) wait_vmcnt<(NST - 2) * LPT>();
                    if constexpr (ABL != 4) __builtin_amdgcn_s_barrier();
                    __builtin_amdgcn_sched_barrier(0);
                }
                // 8 MFMAs of k-step ks.  The NEXT k-step's fragment reads are issued two MFMAs INTO the batch (not in front of
                // it): the compiler waits lgkmcnt(0) before a batch's first MFMA, and this way nothing younger than the batch's
                // own fragments is outstanding at that point - the reads fly under the remaining six MFMAs.  The DMA pieces of
                // the stage NST-1 ahead go between the MFMA pairs of the stage's first k-step.
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    mfma2(cur, i);
                    __builtin_amdgcn_sched_barrier(0);
                    if (i == 0) {
                        if (ks < KS - 1) fload1(st, ks + 1, cur ^ 1);
                        else fload1(nst, 0, cur ^ 1);        // (past the last stage: a landed dummy reload)
                        __builtin_amdgcn_sched_barrier(0);
                    }
                    if (ABL != 1 && ks == 0 && i < PPW) {
                        issue_pieces(i, i + 1);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
                if (ks == 0) issue_advance();
            }
            st = nst;
        }
        wait_vmcnt<0>();
        if constexpr (ABL == 5) {
            float sink = 0.f;
#pragma unroll
            for (int i = 0; i < 4; ++i) sink += acc[i][0][0] + acc[i][1][9];
            if (sink == 12345.678f) p.out32[0] = sink;
            return;
        }
        if constexpr (STG == 2) {
            // round 3 (prepared, NOT yet measured): the P16 epilogues of the 4-wave kernels on the 256 x 256 tile - the quad-layout epilogue
            // was what this kernel lost on in round 2 (docs/history.md, round 3 open items); the V third keeps the row-per-lane stores
            static_assert(EPI == EPI_QKV_ROPE || EPI == EPI_SWIGLU, "P16 epilogues exist for QKV + RoPE and SwiGLU");
            if constexpr (EPI == EPI_QKV_ROPE) wave_epilogue_qkv_p16<4, 2>(p, acc, row0 + wr * 128, rows_end, n0 + wc * 64, frow, fk);
            else wave_epilogue_swiglu_p16<4, 2>(p, g, acc, row0 + wr * 128, rows_end, n0 + wc * 64, frow, fk);
        }
        else if constexpr (STG) staged_epilogue<EPI, 4, 2, 4, 512>(p, g, acc, reinterpret_cast<float*>(ldsp), row0, rows_end, n0, tid, wr, wc, frow, fk);
        else wave_epilogue<EPI, 4, 2>(p, g, acc, row0 + wr * 128, rows_end, n0 + wc * 64, frow, fk);
        return;
    }
    if (wr == 1) __builtin_amdgcn_s_barrier();     // stagger: group 1 runs one half-period behind group 0
    int st = 0;
    for (int t = 0; t < total; ++t) {
#pragma unroll
        for (int sub = 0; sub < NSUB; ++sub) {
            // ---- L: refill the slot both groups have left, fetch this sub-stage's fragments, make sure stage t+1 is here
            if (sub == 0) issue();
            fload(st, sub);
            if (sub == NSUB - 1) wait_vmcnt<(NST - 2) * LPT>();
            __builtin_amdgcn_s_waitcnt(0xc07f);    // lgkmcnt(0): fragments in registers
            __builtin_amdgcn_sched_barrier(0);
            __builtin_amdgcn_s_barrier();          // X
            __builtin_amdgcn_sched_barrier(0);
            // ---- M: 16 MFMAs, the partner wave of this SIMD is in its L phase
            __builtin_amdgcn_s_setprio(1);
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) mfma_step(af[ks], bf[ks], acc);
            __builtin_amdgcn_s_setprio(0);
            __builtin_amdgcn_sched_barrier(0);
            __builtin_amdgcn_s_barrier();          // Y
            __builtin_amdgcn_sched_barrier(0);
        }
        st = st == NST - 1 ? 0 : st + 1;
    }
    if (wr == 0) __builtin_amdgcn_s_barrier();     // re-align the two groups
    wait_vmcnt<0>();                               // the dummy tail reloads must have landed before LDS becomes the staging slab
    staged_epilogue<EPI, 4, 2, 4, 512>(p, g, acc, reinterpret_cast<float*>(ldsp), row0, rows_end, n0, tid, wr, wc, frow, fk);
}

// ---- launchers ---------------------------------------------------------------------------------------------------------------------
// P16 column layout (gemm_dev.h), the one statement of where it applies: N % 16 == 0 and
//   QKV + RoPE: 16 consecutive columns per lane whenever heads and sections are 16-aligned and no grouping is involved;
//   SwiGLU (routed w1/w3, gathered rows, grouped): 16-byte hidden stores straight from the accumulators instead of the LDS-staged slab (no
//   epilogue barriers); ldc and the group's column offset must keep the stores 16-byte aligned.
// The kernels that take it also need K % 64 == 0 (their callers check that).  VB_QKV_P16_OFF=1 switches the layout off everywhere.
static bool gemm_p16_eligible(int epi, const GemmDev& d) {
    if (vb_tune().qkv_p16_off || d.N % 16) return false;
    if (epi == EPI_QKV_ROPE) return d.hd % 16 == 0 && d.D % 16 == 0 && !d.group_off && d.ngroups <= 1;
    if (epi == EPI_SWIGLU) return d.ldc % 8 == 0 && d.c_noff_group % 8 == 0;
    return false;
}

// p8 variants (VB_GEMM_P8): ping-pong 1 = BK 32 x 5 stages, 2 = BK 32 x 4, 3 = BK 64 x 2; software-pipelined 4 / 5 / 6 = the same rings
template <int EPI, int BKT, int NST, int PP, int ABL = 0, int STG = 1>
static void launch_p8_v(const GemmDev& d, dim3 grid, hipStream_t st) {
    constexpr size_t lds = (size_t)NST * 2 * 256 * BKT * 2;
    static_assert(lds >= (size_t)256 * 68 * 4 && lds <= 160 * 1024, "LDS budget");
    static OnceFlags attr;
    vb_set_max_lds_once(attr, reinterpret_cast<const void*>(gemm_bf16_p8_kernel<EPI, BKT, NST, PP, ABL, STG>), (int)lds);
    hipLaunchKernelGGL((gemm_bf16_p8_kernel<EPI, BKT, NST, PP, ABL, STG>), grid, dim3(512), lds, st, d);
}
// product form (tile configuration 89): software-pipelined schedule, BK 32 x 5 stages, P16 column layout - QKV + RoPE and SwiGLU only
template <int EPI>
static void launch_p8_product(const GemmDev& d, dim3 grid, hipStream_t st) {
    // Ring shape (round 5): 64-deep stages x 2 (128 KB) instead of 32-deep x 5 (160 KB).  A DMA instruction of a 32-deep stage covers 16
    // rows x HALF a 128-B line, and both halves of every line cross the CU's 64 B/clk fill path: tools/probe/tile_feed_probe measures 66 GB/s
    // per CU for that pattern against 110 for full lines - less than a 256 x 256 tile's MFMAs consume at full rate (77).  Two 64-deep stages
    // have one stage of lead instead of four, and still win: same box, whole network evaluation 1821 -> 1786 us at 8 clips, 1237 -> 1218 at 4
    // (QKV + RoPE 64.3 -> 62.0 us, routed SwiGLU unchanged; profiles/r05_p8_ring_ab.txt).  Bit-identical (same k order).
    if constexpr (EPI == EPI_QKV_ROPE || EPI == EPI_SWIGLU) {
#ifdef VB_EXPERIMENTS
        if (vb_tune().gemm_p8_ring == 325 && d.K % 32 == 0) { launch_p8_v<EPI, 32, 5, 0, 0, 2>(d, grid, st); return; }       // the round-4 ring (A/B)
        if (vb_tune().gemm_p8_ring == 324 && d.K % 32 == 0) { launch_p8_v<EPI, 32, 4, 0, 0, 2>(d, grid, st); return; }
#endif
        if (d.K % 64 == 0) launch_p8_v<EPI, 64, 2, 0, 0, 2>(d, grid, st);
        else launch_p8_v<EPI, 32, 5, 0, 0, 2>(d, grid, st);
    }
}
#ifdef VB_EXPERIMENTS
#ifndef P8_DEFAULT_BKT
#define P8_DEFAULT_BKT 32
#define P8_DEFAULT_NST 5
#define P8_DEFAULT_PP 0
#endif
template <int EPI>
static void launch_p8(const GemmDev& d, dim3 grid, hipStream_t st, int variant) {
    if constexpr (EPI == EPI_F32) {      // the alternative schedules / ring shapes exist for the micro-benchmark only (tools/gemm_p8_bench.py)
        if (variant == 1) { launch_p8_v<EPI, 32, 5, 1>(d, grid, st); return; }
        if (variant == 2) { launch_p8_v<EPI, 32, 4, 1>(d, grid, st); return; }
        if (variant == 3 && d.K % 64 == 0) { launch_p8_v<EPI, 64, 2, 1>(d, grid, st); return; }
        if (variant == 4) { launch_p8_v<EPI, 32, 5, 0>(d, grid, st); return; }
        if (variant == 5) { launch_p8_v<EPI, 32, 4, 0>(d, grid, st); return; }
        if (variant == 6 && d.K % 64 == 0) { launch_p8_v<EPI, 64, 2, 0>(d, grid, st); return; }
        if (variant == 11) { launch_p8_v<EPI, 32, 5, 0, 1>(d, grid, st); return; }       // ablations of the pipelined 32 x 5 ring
        if (variant == 12) { launch_p8_v<EPI, 32, 5, 0, 2>(d, grid, st); return; }
        if (variant == 13) { launch_p8_v<EPI, 32, 5, 0, 3>(d, grid, st); return; }
        if (variant == 14) { launch_p8_v<EPI, 32, 5, 0, 4>(d, grid, st); return; }
        if (variant == 15) { launch_p8_v<EPI, 32, 5, 0, 5>(d, grid, st); return; }
    }
    if constexpr (EPI == EPI_QKV_ROPE || EPI == EPI_SWIGLU) {
        // VB_GEMM_P8_P16: P16 column layout (needs the software-pipelined schedule, K % 64 == 0 and 16-byte aligned output rows, like the 4-wave form)
        if ((vb_tune().gemm_p8_p16 & (1 << EPI)) && P8_DEFAULT_PP == 0 && d.K % 64 == 0 && gemm_p16_eligible(EPI, d)) {
            launch_p8_v<EPI, P8_DEFAULT_BKT, P8_DEFAULT_NST, 0, 0, 2>(d, grid, st);
            return;
        }
        if (vb_tune().gemm_p8_direct & (1 << EPI)) { launch_p8_v<EPI, P8_DEFAULT_BKT, P8_DEFAULT_NST, P8_DEFAULT_PP, 0, 0>(d, grid, st); return; }
    }
    launch_p8_v<EPI, P8_DEFAULT_BKT, P8_DEFAULT_NST, P8_DEFAULT_PP>(d, grid, st);
}
template <int EPI> struct P8Epi { static constexpr bool ok = EPI == EPI_PLANES || EPI == EPI_F32 || EPI == EPI_QKV_ROPE || EPI == EPI_RESID_GATE ||
                                                            EPI == EPI_SWIGLU || EPI == EPI_SCATTER_F32 || EPI == EPI_SCATTER_ADD_PLANES; };

#endif  // VB_EXPERIMENTS

template <int EPI, int TM, int TN, int NSTB>
static void launch_big(const GemmDev& d, dim3 grid, hipStream_t st) {
    constexpr size_t lds = (size_t)NSTB * (64 * TM + 64 * TN) * 128;
#ifdef VB_EXPERIMENTS
    if constexpr (EPI == EPI_F32 && TM == 3 && TN == 3) {
        const int abl = vb_tune().gemm_ablate;
        if (abl >= 1 && abl <= 3) {
            auto k = abl == 1 ? gemm_bf16_big_kernel<EPI, TM, TN, NSTB, 1> : (abl == 2 ? gemm_bf16_big_kernel<EPI, TM, TN, NSTB, 2> : gemm_bf16_big_kernel<EPI, TM, TN, NSTB, 3>);
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            hipLaunchKernelGGL(k, grid, dim3(NTHREADS), lds, st, d);
            return;
        }
    }
#endif
    static_assert(lds >= (size_t)64 * (64 * TN + 4) * 4, "epilogue staging slab must fit in the ring");
    static OnceFlags attr;
    vb_set_max_lds_once(attr, reinterpret_cast<const void*>(gemm_bf16_big_kernel<EPI, TM, TN, NSTB>), (int)lds);
    hipLaunchKernelGGL((gemm_bf16_big_kernel<EPI, TM, TN, NSTB>), grid, dim3(NTHREADS), lds, st, d);
}

#ifdef VB_EXPERIMENTS
// the ring shapes / ablations tools/gemm_bench.py compares (VB_GEMM_VARIANT / VB_GEMM_ABLATE); true = launched
template <int EPI>
static bool launch_t_experiments(const GemmDev& d, dim3 grid, hipStream_t st) {
    const int variant = vb_tune().gemm_variant;
    const int abl = vb_tune().gemm_ablate;
    if constexpr (EPI == EPI_F32) {
        if (abl == 1 && d.K % 64 == 0) { hipLaunchKernelGGL((gemm_bf16_glds_kernel<EPI, 64, 2, 1>), grid, dim3(NTHREADS), 0, st, d); return true; }
        if (abl == 2 && d.K % 64 == 0) { hipLaunchKernelGGL((gemm_bf16_glds_kernel<EPI, 64, 2, 2>), grid, dim3(NTHREADS), 0, st, d); return true; }
        if (abl == 3 && d.K % 64 == 0) { hipLaunchKernelGGL((gemm_bf16_glds_kernel<EPI, 64, 2, 3>), grid, dim3(NTHREADS), 0, st, d); return true; }
        if (abl == 4 && d.K % 64 == 0) { hipLaunchKernelGGL((gemm_bf16_glds_kernel<EPI, 64, 2, 4>), grid, dim3(NTHREADS), 0, st, d); return true; }
        if (abl == 5 && d.K % 64 == 0) { hipLaunchKernelGGL((gemm_bf16_glds_kernel<EPI, 64, 2, 5>), grid, dim3(NTHREADS), 0, st, d); return true; }
    }
    if (variant == 0) { hipLaunchKernelGGL(gemm_bf16_kernel<EPI>, grid, dim3(NTHREADS), 0, st, d); return true; }
    if (variant == 2 && d.K % 32 == 0) { hipLaunchKernelGGL((gemm_bf16_glds_kernel<EPI, 32, 4>), grid, dim3(NTHREADS), 0, st, d); return true; }
    if (variant == 3 && d.K % 32 == 0) { hipLaunchKernelGGL((gemm_bf16_glds_kernel<EPI, 32, 3>), grid, dim3(NTHREADS), 0, st, d); return true; }
    if ((variant == 4 || variant == 5) && d.K % 64 == 0) {
        // deeper rings of the 128 x 128 tile (3 stages = 96 KB, 4 = 128 KB: one workgroup per CU) - the one-clip A/B of round 5: SLOWER, 41.6 ms per
        // clip with either against 40.8 with the two-stage ring at two workgroups per CU (same box, two runs each, parity ok): DESIGN 5.0
        if constexpr (EPI == EPI_QKV_ROPE || EPI == EPI_SWIGLU) {
            if (gemm_p16_eligible(EPI, d)) {
                if (variant == 4) { hipLaunchKernelGGL((gemm_bf16_glds_kernel<EPI, 64, 3, 0, true>), grid, dim3(NTHREADS), 0, st, d); }
                else { hipLaunchKernelGGL((gemm_bf16_glds_kernel<EPI, 64, 4, 0, true>), grid, dim3(NTHREADS), 0, st, d); }
                return true;
            }
        }
        if (variant == 4) { hipLaunchKernelGGL((gemm_bf16_glds_kernel<EPI, 64, 3>), grid, dim3(NTHREADS), 0, st, d); }
        else { hipLaunchKernelGGL((gemm_bf16_glds_kernel<EPI, 64, 4>), grid, dim3(NTHREADS), 0, st, d); }
        return true;
    }
    return false;
}
#endif

template <int EPI>
static void launch_t(const GemmDev& d, dim3 grid, hipStream_t st) {
    // 128 x 128 tiles, two workgroups per CU: tile DMA (global_load_lds) with BK = 64 x 2 stages - in the P16 layout where that applies;
    // K % 64 = 32 (96-channel bands at 8 experts) takes BK = 32 x 4 stages; anything else the register-staged kernel.
#ifdef VB_EXPERIMENTS
    if (launch_t_experiments<EPI>(d, grid, st)) return;
#endif
    if constexpr (EPI == EPI_QKV_ROPE || EPI == EPI_SWIGLU) {
        if (d.K % 64 == 0 && gemm_p16_eligible(EPI, d)) { hipLaunchKernelGGL((gemm_bf16_glds_kernel<EPI, 64, 2, 0, true>), grid, dim3(NTHREADS), 0, st, d); return; }
    }
    if (d.K % 64 == 0) hipLaunchKernelGGL((gemm_bf16_glds_kernel<EPI, 64, 2>), grid, dim3(NTHREADS), 0, st, d);
    else if (d.K % 32 == 0) hipLaunchKernelGGL((gemm_bf16_glds_kernel<EPI, 32, 4>), grid, dim3(NTHREADS), 0, st, d);   // K = 96 bands (8 experts)
    else hipLaunchKernelGGL(gemm_bf16_kernel<EPI>, grid, dim3(NTHREADS), 0, st, d);
}

// ---- launch_gemm: descriptor (+ the checks that fail the call) -> route -> grid -> launch ----------------------------------------------
unsigned long long* g_gemm_trace = nullptr;
extern "C" void vbdbg_gemm_trace(void* buf) { g_gemm_trace = static_cast<unsigned long long*>(buf); }   // tuning tool hook, not ABI

// "row-range groups": the groups partition the rows (device array of offsets, or uniform groups of group_rows rows each); otherwise
// ngroups > 1 means the same rows against several operands (grid z)
static bool gemm_row_groups(const GemmArgs& a) { return a.group_off != nullptr || a.group_rows > 0; }
static int gemm_grid_z(const GemmArgs& a) { return gemm_row_groups(a) ? 1 : (a.ngroups > 0 ? a.ngroups : 1); }

static int gemm_fill(const GemmArgs& a, GemmDev& d) {
    if (a.N % 4 || a.K % 8 || a.lda % 8 || a.ldb % 8) VB_FAIL(VB_E_INVALID, "gemm: N%%4, K%%8, lda%%8, ldb%%8 must be 0 (N=%d K=%d)", a.N, a.K);
    if (a.nseg != 1 && a.nseg != 3) VB_FAIL(VB_E_INVALID, "gemm: nseg must be 1 or 3");
    d.A = a.A; d.a_plane = a.a_plane; d.lda = a.lda; d.a_rows = a.a_rows; d.a_koff_group = a.a_koff_group;
    d.B = a.B; d.b_plane = a.b_plane; d.ldb = a.ldb; d.b_group_stride = a.b_group_stride;
    d.M = a.M; d.N = a.N; d.K = a.K; d.nseg = a.nseg; d.ngroups = a.ngroups; d.group_off = a.group_off;
    d.c_noff_group = a.c_noff_group; d.bias = a.bias; d.bias_group_stride = a.bias_group_stride;
    d.out = a.out.p; d.out_plane = a.out.plane; d.out_np = a.out.np; d.ldc = a.ldc;
    d.out32 = a.out32; d.ldc32 = a.ldc32; d.gate = a.gate; d.gate_ld = a.gate_ld; d.T = a.T > 0 ? a.T : 1;
    d.rows_out = a.rows_out; d.row_scale = a.row_scale; d.y32_in = a.y32_in; d.row_scale2 = a.row_scale2; d.scale_split = a.scale_split;
    d.add32 = a.add32; d.dup_rows = a.dup_rows;
    d.conv_ci = a.conv_ci; d.conv_ktap = 0; d.conv_dil = a.conv_dil; d.conv_agrp = a.conv_agrp; d.conv_arow0 = a.conv_arow0; d.conv_btap = a.conv_btap;
    d.res32 = a.res32;
    if (a.conv_ci > 0) {
        if (a.epi != EPI_F32_CT || a.group_rows <= 0 || a.conv_ci % 64 || a.K % a.conv_ci || a.a_rows || a.group_rows != (a.T > 0 ? a.T : 1))
            VB_FAIL(VB_E_INVALID, "gemm: conv mode needs EPI_F32_CT, uniform groups of T rows, Ci %% 64 == 0");
        d.conv_ktap = a.conv_ci / 64;
    }
    d.q = a.q.p; d.q_plane = a.q.plane; d.k = a.k.p; d.k_plane = a.k.plane; d.vt = a.vt.p; d.vt_plane = a.vt.plane;
    d.qkv_np = a.q.np; d.rope_cos = a.rope_cos; d.rope_sin = a.rope_sin; d.H = a.H; d.hd = a.hd > 0 ? a.hd : 1;
    d.Tpad = a.Tpad; d.D = a.D > 0 ? a.D : 1;
    d.rT = 1.0f / (float)d.T; d.rhd = 1.0f / (float)d.hd; d.rD = 1.0f / (float)d.D;
    if (a.M >= (1 << 21) || (int64_t)a.N * (a.ngroups > 0 ? a.ngroups : 1) >= (1 << 21)) VB_FAIL(VB_E_INVALID, "gemm: index ranges exceed fdiv()");
    d.trace = g_gemm_trace; d.abl = vb_tune().gemm_ablate; d.no_vt16 = vb_tune().qkv_vt16_off ? 1 : 0; d.epi_old = vb_tune().band_epi_old ? 1 : 0;
    return VB_OK;
}

// bytes the launch moves, for the profiler's class table: both operands (per bf16 plane pass) + the epilogue's result (+ read-modify) bytes
static double gemm_prof_bytes(const GemmArgs& a) {
    const double gz = gemm_grid_z(a);                                                   // groups that share the row range multiply the work
    const double npl = a.nseg == 3 ? 2.0 : 1.0, MN = (double)a.M * a.N * gz;
    double ob;
    switch (a.epi) {
        case EPI_F32: case EPI_F32_CT: case EPI_SCATTER_F32: ob = 4.0 * MN; break;
        case EPI_RESID_GATE: ob = 8.0 * MN; break;
        case EPI_SWIGLU: case EPI_GEGLU: ob = MN * a.out.np; break;
        case EPI_SCATTER_ADD_PLANES: ob = MN * (4.0 + 2.0 * a.out.np); break;
        case EPI_QKV_ROPE: ob = 2.0 * MN * a.q.np; break;
        default: ob = 2.0 * MN * a.out.np; break;
    }
    return 2.0 * npl * ((double)a.M * a.K * (a.a_koff_group ? gz : 1.0) + (double)a.N * a.K * (a.ngroups > 1 ? a.ngroups : 1)) + ob;
}

// Tile configurations.  (The 128 x 256 / 256 x 128 forms spilled - 576-640 B of scratch at 254-256 VGPRs - and were removed in round 4.)
enum GemmRoute {
    GEMM_T128, GEMM_WIDE_RESID, GEMM_BIG_192, GEMM_SMALL_64, GEMM_SMALL_128x64, GEMM_P8,
#ifdef VB_EXPERIMENTS
    GEMM_P8_VARIANT, GEMM_PK, GEMM_PK_F32,      // (the persistent kernel sizes its own grid)
#endif
    GEMM_ROUTE_COUNT
};
// (bm, bn) of each route, in the enum's order (the experiments forms walk the 8-wave kernel's tile)
struct GemmTile { int bm, bn; };
static constexpr GemmTile GEMM_TILE[] = {
    {BM, BN}, {BM, 192}, {192, 192}, {64, 64}, {128, 64}, {256, 256},
#ifdef VB_EXPERIMENTS
    {256, 256}, {256, 256}, {256, 256},
#endif
};
static_assert(sizeof(GEMM_TILE) / sizeof(GEMM_TILE[0]) == GEMM_ROUTE_COUNT, "one tile per GemmRoute, in the enum's order");
// tiles a launch makes with bm x bn tiles: row-range groups may each end in a partial row tile, groups sharing the rows multiply the grid
static int64_t gemm_tiles(const GemmArgs& a, int bm, int bn) {
    return (int64_t)(gemm_row_groups(a) ? cdiv(a.M, bm) + a.ngroups : cdiv(a.M, bm)) * cdiv(a.N, bn) * gemm_grid_z(a);
}

// One eligibility predicate per route other than GEMM_T128 (gemm_route adds K % 64 == 0, the DMA ring of these kernels, and the A/B knobs).
// 128 x 192 serves the plain gated-residual GEMM (VB_GEMM_TILE=23 forces it on that shape) ...
static bool gemm_wide_resid_shape(const GemmArgs& a) { return a.epi == EPI_RESID_GATE && !gemm_row_groups(a) && a.ngroups <= 1 && a.N % 192 == 0; }
// ... and is taken where 128 x 128 tiles need a second round of the 512 two-per-CU slots and 128 x 192 tiles do not
static bool gemm_wide_resid_eligible(const GemmArgs& a) {
    const int64_t t23 = (int64_t)cdiv(a.M, BM) * (a.N / 192);
    return gemm_wide_resid_shape(a) && gemm_tiles(a, BM, BN) > 512 && t23 <= 512;
}
// measured (tools/gemm_tilecfg.py): the 192x192 kernel wins when its tiles fit one round of the 256 CUs
// (12032 x 768: 252 tiles); with several rounds per CU the 128x128 kernel (two co-resident workgroups
// overlapping each other's epilogue) is as fast or faster.
// (K >= 384 since round 3: at one clip the band experts' K = 192 first product took the 192 x 192 one-per-CU kernel - three
//  k-iterations under a 24-KB-per-stage ring, 18 us - where 128 x 128 tiles run ~8: one 20 s clip 40.2 -> 38.2 ms)
static bool gemm_big192_eligible(const GemmArgs& a, const VbTune& tune) {
    return gemm_tiles(a, 192, 192) <= 256 + 16 && gemm_tiles(a, BM, BN) > 320 && !a.rows_out && a.K >= tune.big_tile_min_k;      // (row-scatter epilogues measured slower on it)
}
// small problems (one or two clips): 128x128 tiles leave most CUs idle and a tile's 12 k-iterations are pure DMA latency;
// 64x64 tiles (three workgroups per CU) make 4x the tiles.  VB_GEMM_SMALL=0 keeps the 128x128 kernel, 21 takes 128x64.
// (threshold 200 tiles since round 3: at 4 clips x 2 branches - one sub-batch of the two-stream configuration, 282 tiles - the
//  128 x 128 kernel is ahead when another stream shares the GPU: 1287 vs 1280 mel-s/s over three interleaved runs; per-clip
//  grouped launches with >= 8 clips keep the 128 x 128 kernel for its XCD-affine tile order)
static bool gemm_small_eligible(const GemmArgs& a, const VbTune& tune) {
    return gemm_tiles(a, BM, BN) < tune.gemm_small_tiles && !(a.group_rows > 0 && a.ngroups >= 8 && a.ngroups % 8 == 0 && !tune.no_xcd_groups);
}
// 8-wave 256 x 256 kernel with the P16 epilogues (round 4) on the two wide projections - QKV + RoPE and the routed SwiGLU - whenever the
// launch makes at least P8_MIN_TILES of its tiles (two clips and up; one clip keeps the small tiles) and the P16 layout applies (the
// conditions of the 4-wave P16 forms).  Same k order, same epilogue arithmetic: bit-identical to the 4-wave kernels
// (VB_GEMM_P8_OFF=1 keeps those; test_p8_p16_projections_are_bit_identical), so a clip's bits still do not depend on its batch.
static bool gemm_p8_eligible(const GemmArgs& a, const GemmDev& d) {
    return (a.epi == EPI_QKV_ROPE || a.epi == EPI_SWIGLU) && a.K % 64 == 0 && a.conv_ci == 0 && a.group_rows == 0 && gemm_p16_eligible(a.epi, d) &&
           gemm_tiles(a, 256, 256) >= P8_MIN_TILES;
}
// conv-as-GEMM: 128 x 128 tiles, or 64 x 64 (three workgroups per CU) when 128 x 128 would make fewer than 200 workgroups - one or two
// clips; same k order in both, so a clip's bits do not depend on the batch
static bool gemm_conv_small_eligible(const GemmArgs& a, const VbTune& tune) {
    return (int64_t)a.ngroups * cdiv(a.group_rows, BM) * cdiv(a.N, BN) < tune.gemm_small_tiles;
}
static GemmRoute gemm_conv_route(const GemmArgs& a, const VbTune& tune) {
    return (tune.gemm_small == 11 && gemm_conv_small_eligible(a, tune)) ? GEMM_SMALL_64 : GEMM_T128;
}
// the tile (rows = positions x columns = output channels) a conv-mode launch of B clips x T_out rows x Co columns takes: vb_conv1d_plan
void gemm_conv_tile(int B, int T_out, int Co, int* bm, int* bn) {
    GemmArgs a; a.ngroups = B; a.group_rows = T_out; a.N = Co;
    const GemmTile t = GEMM_TILE[gemm_conv_route(a, vb_tune())];
    *bm = t.bm; *bn = t.bn;
}

#ifdef VB_EXPERIMENTS
// The experiments build's opt-ins, over the product's choice.  None of them is on by default.
static GemmRoute gemm_route_experiments(const GemmArgs& a, const GemmDev& d, const VbTune& tune, GemmRoute route) {
    if (a.epi == EPI_F32 && tune.gemm_pk_f32 > 0 && a.K % 64 == 0 && !gemm_row_groups(a) && a.ngroups <= 1 && a.conv_ci == 0 && !a.add32) return GEMM_PK_F32;
    // round 5: the persistent form of the 8-wave tile (gemm_bf16_pk_kernel, bit-identical again) - MEASURED NOT FASTER (profiles/r05_gemm_pk_ab.txt,
    // DESIGN 5.0): an experiments-build opt-in (VB_GEMM_PK=1), the product keeps the per-tile launch
    const bool pk_ok = a.epi == EPI_SWIGLU ? (!a.group_off || a.ngroups <= PK_MAX_GROUPS)
                                           : ((d.T & 15) == 0 && (d.Tpad & 7) == 0 && !d.no_vt16 && ((2 * d.D) & 255) == 0 && a.q.np == a.vt.np);
    if (route == GEMM_P8 && tune.gemm_pk > 0 && gemm_grid_z(a) == 1 && pk_ok && (int64_t)a.M * a.lda < (1ll << 31) &&
        (int64_t)(a.ngroups > 0 ? a.ngroups : 1) * a.b_group_stride + (int64_t)a.N * a.ldb < (1ll << 31)) route = GEMM_PK;
    // 8-wave 256 x 256 kernel (gemm_bf16_p8_kernel): taken when the problem makes enough of its tiles to occupy a good part of the chip - it
    // moves half the bytes per flop through the L2 -> LDS feed, so it wins even at ~55 % of the CUs busy (12032 x 768: 141 tiles);
    // small problems (one 20 s clip: 18 tiles) stay on the 128 x 128 kernel.  VB_GEMM_P8 = 0 off / 1..3 force a ring shape.
    const int p8 = tune.gemm_p8;
    const bool epi_ok = a.epi == EPI_PLANES || a.epi == EPI_F32 || a.epi == EPI_QKV_ROPE || a.epi == EPI_RESID_GATE ||
                        a.epi == EPI_SWIGLU || a.epi == EPI_SCATTER_F32 || a.epi == EPI_SCATTER_ADD_PLANES;
    if (epi_ok && a.K % 32 == 0 && p8 != 0 && tune.gemm_tile < 0) {
        // measured (tools/gemm_p8_bench.py, profiles/r02_gemm_p8_microbench.txt): with one workgroup per CU nothing overlaps a
        // tile's epilogue, so the 8-wave kernel only wins where the mainloop outweighs the output traffic - the wide
        // projections (N >= 1024: QKV, routed w1/w3); the N = 768 / 640 launches stay on the two-per-CU 128 x 128 kernel
        // and inside the DiT even those lose (A/B in the pipeline, profiles/r02_p8_pipeline_ab.txt: GEMM class 74 -> 86 ms per pass):
        // QKV's RoPE / V-transpose epilogue and the gathered grouped SwiGLU cost more on a 256-row tile than the mainloop gains.
        // The kernel therefore stays an opt-in (VB_GEMM_P8 >= 1) - kept for the micro-benchmark and as the record of the experiment.
        if (p8 > 0) route = GEMM_P8_VARIANT;
        else if ((tune.gemm_p8_mask & (1 << a.epi)) && gemm_tiles(a, 256, 256) >= P8_MIN_TILES) route = GEMM_P8_VARIANT;     // per-epilogue opt-in (A/B tool)
    }
    return route;
}
#endif

// Which kernel runs.  Later rules override earlier ones: a forced tile (VB_GEMM_TILE=22|33|11|21|23, the bit-identity tests) or else the
// first eligible of wide-resid / big / small; the 8-wave kernel over those; QKV never on 192 x 192; the experiments opt-ins; conv mode last.
static int gemm_route(const GemmArgs& a, const GemmDev& d, const VbTune& tune, GemmRoute& route) {
    route = GEMM_T128;
    if (a.K % 64 == 0) {
        const int forced = tune.gemm_tile;
        if (forced >= 0) {
            switch (forced) {
                case 22: break;
                case 33: route = GEMM_BIG_192; break;
                case 11: route = GEMM_SMALL_64; break;
                case 21: route = GEMM_SMALL_128x64; break;
                case 23: if (gemm_wide_resid_shape(a)) route = GEMM_WIDE_RESID; break;
                default: VB_FAIL(VB_E_INVALID, "gemm: VB_GEMM_TILE=%d is not a tile configuration (22, 33, 11, 21, 23)", forced);
            }
        } else if (gemm_wide_resid_eligible(a) && tune.wide_resid) route = GEMM_WIDE_RESID;
        else if (gemm_big192_eligible(a, tune)) route = GEMM_BIG_192;
        else if (tune.gemm_small && gemm_small_eligible(a, tune)) route = tune.gemm_small == 21 ? GEMM_SMALL_128x64 : GEMM_SMALL_64;
    }
    if (gemm_p8_eligible(a, d) && tune.gemm_tile < 0 && !tune.gemm_p8_off) route = GEMM_P8;
    // the 192 x 192 tile with the RoPE / V-transpose epilogue needs more registers than a wave has (640 B of scratch at 256 VGPRs): QKV takes the
    // 128 x 128 tiles wherever the rules above (or VB_GEMM_TILE) say 192 x 192 - M in (2176, 2560] rows - bit-identical like every tile choice
    if (route == GEMM_BIG_192 && a.epi == EPI_QKV_ROPE) route = GEMM_T128;
#ifdef VB_EXPERIMENTS
    route = gemm_route_experiments(a, d, tune, route);
#endif
    if (a.conv_ci > 0) route = gemm_conv_route(a, tune);
    return VB_OK;
}

// Grid and group setup of the route's tile: d.n_tiles, d.grp_*, d.ncc / d.rpx and the launch grid (x = column tiles x row tiles rounded to the
// 8 XCDs, z = groups that share the rows)
static int gemm_grid(const GemmArgs& a, GemmDev& d, GemmRoute route, const VbTune& tune, dim3& grid) {
    const GemmTile t = GEMM_TILE[route];
    const bool uniform_ok = route == GEMM_T128 || (route == GEMM_SMALL_64 && a.conv_ci > 0);      // uniform groups: 128 x 128 kernel; 64 x 64 in conv mode
    int mt = gemm_row_groups(a) ? (cdiv(a.M, t.bm) + a.ngroups) : cdiv(a.M, t.bm);
    d.n_tiles = cdiv(a.N, t.bn);
    d.grp_rows = 0; d.grp_tiles = 0; d.grp_xcd = 0;
    if (a.group_rows > 0 && !a.group_off && !uniform_ok)
        VB_FAIL(VB_E_INVALID, "gemm: uniform groups without an offset array run on the 128 x 128 kernel (or 64 x 64 in conv mode) only");
    if (a.conv_ci > 0 && (!uniform_ok || a.K % 64)) VB_FAIL(VB_E_INVALID, "gemm: conv mode runs on the 128 x 128 / 64 x 64 DMA kernels (K %% 64 == 0)");
    if (uniform_ok && a.group_rows > 0 && a.K % 32 == 0) {
        d.grp_rows = a.group_rows; d.grp_tiles = cdiv(a.group_rows, t.bm);
        d.grp_xcd = (a.conv_ci == 0 && a.ngroups % 8 == 0 && !tune.no_xcd_groups) ? 1 : 0;
        mt = d.grp_xcd ? a.ngroups * d.grp_tiles : (a.ngroups * d.grp_tiles + 7) / 8 * 8;
    }
    //  uniform groups described only by group_rows must have been taken up above: on any other route (K % 32 != 0 -> the
    // register-staged kernel) every row would silently run against group 0's operand
    if (a.group_rows > 0 && !a.group_off && d.grp_rows == 0) VB_FAIL(VB_E_INVALID, "gemm: uniform row groups need K %% 32 == 0 (K=%d)", a.K);
    grid = dim3(d.n_tiles * ((mt + 7) / 8 * 8), 1, gemm_grid_z(a));
    d.ncc = 0; d.rpx = (mt + 7) / 8;
    if (route == GEMM_T128 && !gemm_row_groups(a)) {       // VB_GEMM_NCHUNK=c (tuning, default off until measured in the pipeline): column chunking for wide N
        const int c = tune.gemm_nchunk;
        if (c > 0 && d.n_tiles > c && d.n_tiles % c == 0) d.ncc = c;
    }
    return VB_OK;
}

template <int EPI>
static void gemm_launch(GemmRoute route, const GemmDev& d, dim3 grid, hipStream_t st) {
    switch (route) {
        case GEMM_WIDE_RESID: hipLaunchKernelGGL(gemm_bf16_wide_resid_kernel<3>, grid, dim3(NTHREADS), 0, st, d); break;    // (EPI_RESID_GATE: gemm_wide_resid_shape)
#ifdef VB_EXPERIMENTS
        case GEMM_P8_VARIANT: if constexpr (P8Epi<EPI>::ok) launch_p8<EPI>(d, grid, st, vb_tune().gemm_p8); break;
        case GEMM_PK: launch_gemm_pk(EPI, d, st); break;
        case GEMM_PK_F32: break;               // (launched before the grid setup)
#endif
        case GEMM_P8: launch_p8_product<EPI>(d, grid, st); break;
        case GEMM_BIG_192: if constexpr (EPI != EPI_QKV_ROPE) launch_big<EPI, 3, 3, 3>(d, grid, st); break;
        case GEMM_SMALL_64: launch_big<EPI, 1, 1, 3>(d, grid, st); break;
        case GEMM_SMALL_128x64: launch_big<EPI, 2, 1, 3>(d, grid, st); break;
        case GEMM_T128: launch_t<EPI>(d, grid, st); break;
        case GEMM_ROUTE_COUNT: break;
    }
}

int launch_gemm(const GemmArgs& a, hipStream_t st) {
    if (a.M <= 0 || a.N <= 0) return VB_OK;
    const VbTune& tune = vb_tune();
    GemmDev d;
    VB_TRY(gemm_fill(a, d));
    ProfScope prof(a.prof_class, 2.0 * a.M * a.N * gemm_grid_z(a) * a.K, gemm_prof_bytes(a), st);
    GemmRoute route;
    VB_TRY(gemm_route(a, d, tune, route));
#ifdef VB_EXPERIMENTS
    if (route == GEMM_PK_F32) { launch_gemm_pk_f32(d, st, tune.gemm_pk_f32); VB_CHECK_LAUNCH(); return VB_OK; }      // (sizes its own grid)
#endif
    dim3 grid;
    VB_TRY(gemm_grid(a, d, route, tune, grid));
    switch (a.epi) {
#define VB_GEMM_CASE(E) case E: gemm_launch<E>(route, d, grid, st); break;
        VB_GEMM_CASE(EPI_PLANES)
        VB_GEMM_CASE(EPI_F32)
        VB_GEMM_CASE(EPI_QKV_ROPE)
        VB_GEMM_CASE(EPI_RESID_GATE)
        VB_GEMM_CASE(EPI_SWIGLU)
        VB_GEMM_CASE(EPI_SCATTER_F32)
        VB_GEMM_CASE(EPI_SCATTER_ADD_PLANES)
        VB_GEMM_CASE(EPI_GELU_PLANES)
        VB_GEMM_CASE(EPI_HEADS_T)
        VB_GEMM_CASE(EPI_F32_CT)
        VB_GEMM_CASE(EPI_GEGLU)
#undef VB_GEMM_CASE
        default: VB_FAIL(VB_E_INVALID, "gemm: bad epilogue %d", a.epi);
    }
    VB_CHECK_LAUNCH();
    return VB_OK;
}
