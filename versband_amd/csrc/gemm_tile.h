// What the bf16 GEMM kernels' main loops share (gemm_bf16.hip, band_ffn.hip), each piece defined once: which tile a workgroup owns, the LDS
// tile image and its swizzle, the tile DMA feed, the operand offsets of a k-tile, and the 16-deep MFMA step.  What differs between the
// kernels - where the counted waits, the barriers, the fragment prefetch and the refill sit - stays in the kernels; the one schedule with two
// users, the two-stage K walk of the 128 x 64 TN kernels, is here too (gemm_walk_2stage).
// Everything here is forced inline over caller-owned arrays of compile-time extent (a runtime-indexed register array would become scratch),
// and `wave` is the caller's readfirstlane value, so stage bases and piece offsets stay scalar.
#pragma once
#include "gemm_dev.h"

// ---- LDS tile image ----------------------------------------------------------------------------------------------------------------
// A tile row holds BKT bf16 = BKT / 8 chunks of 16 bytes.  Chunk c of row r lives at chunk slot c ^ tile_swz(r), so that the ds_read_b128
// fragment reads of 16 consecutive rows hit 16 distinct 16-byte slots.  The XOR is ONE INVOLUTION used from both sides: lds_off_t applies it
// to the chunk a fragment read wants, TileFeed::rows applies it to the chunk a DMA lane fetches (the DMA image must be lane-linear, so the
// swizzle is applied to the SOURCE: LDS slot (r, c') receives global chunk c' ^ tile_swz(r)).  Change one and the other changes with it.
template <int BKT> __device__ __forceinline__ int tile_swz(int row) {
    static_assert(BKT == 64 || BKT == 32, "tile rows of 128 or 64 bytes");
    if constexpr (BKT == 64) return (row >> 1) & 7;
    else return (row >> 2) & 3;
}
template <int BKT> __device__ __forceinline__ int lds_off_t(int row, int c) {      // byte offset of chunk c of row `row` inside a [rows][BKT] bf16 tile
    return row * (BKT * 2) + ((c ^ tile_swz<BKT>(row)) << 4);
}

// ---- which tile is this block --------------------------------------------------------------------------------------------------------
// XCD-aware tile order: block L runs on XCD L % 8 (8 private L2s).  All column tiles of one row tile are consecutive blocks of the SAME XCD,
// so an A tile is fetched into one L2 once instead of once per column tile.  -> column tile, row tile rt of this XCD; returns the row-tile
// index of the launch (over all groups)
__device__ __forceinline__ int tile_xcd_order(int n_tiles, int& tile_n, int& rt) {
    const int L = blockIdx.x, jx = L >> 3;
    tile_n = jx % n_tiles;
    rt = jx / n_tiles;
    return rt * 8 + (L & 7);
}
// row-range groups given by an offset array (written by the bucket kernels): row tile tmg of the launch -> (group, rows); false = padding block
template <int BMT>
__device__ __forceinline__ bool tile_group_search(const int* group_off, int ngroups, int tmg, int& g, int& row0, int& rows_end) {
    for (int gi = 0; gi < ngroups; ++gi) {
        const int lo = group_off[gi], hi = group_off[gi + 1];
        const int nt = (hi - lo + BMT - 1) / BMT;
        if (tmg < nt) { g = gi; row0 = lo + tmg * BMT; rows_end = hi; return true; }
        tmg -= nt;
    }
    return false;
}
// What a kernel's tile walk supports is a template choice (no kernel carries a branch for a grouping it is never launched with):
enum TileGroups {
    TILE_UNGROUPED,        // one row range, one operand pair (128 x 192 gated-residual kernel)
    TILE_GROUPS,           // + offset-array groups, groups that share the rows (blockIdx.z)
    TILE_UNIFORM,          // + uniform groups of grp_rows rows (conv-as-GEMM: one clip per group)
    TILE_UNIFORM_XCD,      // + XCD-affine uniform groups (grp_xcd) and column chunking for wide N (ncc): the 128 x 128 DMA kernel
};
// false for a padding block (the grid is rounded up to the 8 XCDs and, with groups, to an upper bound of their row tiles)
template <int BMT, int BNT, TileGroups TG>
__device__ __forceinline__ bool gemm_tile_pos(const GemmDev& p, int& g, int& row0, int& rows_end, int& n0) {
    int tile_n, rt, tmg;
    if (TG == TILE_UNIFORM_XCD && p.ncc > 0) {
        // wide N (QKV: 18 column tiles = 3.5 MB of weights against a 4 MB L2 per XCD): an XCD walks ALL its row tiles for one
        // chunk of ncc column tiles before moving to the next chunk, so the live weight set is ncc/nN of the matrix
        const int L = blockIdx.x, jx = L >> 3;
        const int per = p.rpx * p.ncc;
        const int ch = jx / per, rem = jx - ch * per;
        rt = rem / p.ncc;
        tile_n = ch * p.ncc + (rem - rt * p.ncc);
        tmg = rt * 8 + (L & 7);
    } else {
        tmg = tile_xcd_order(p.n_tiles, tile_n, rt);
    }
    n0 = tile_n * BNT;
    g = 0;
    if (TG >= TILE_UNIFORM && p.grp_rows > 0) {
        int lt;       // row tile inside the group
        if (TG == TILE_UNIFORM_XCD && p.grp_xcd) {
            // per-group B operands (caption-gate scores: one folded key matrix per clip) and a multiple of 8 groups: XCD x = L & 7 serves
            // the groups x, x + 8, ... - all row tiles of a group on one XCD, its B operand in one L2 (it was fetched by all eight)
            g = (blockIdx.x & 7) + 8 * (rt / p.grp_tiles);
            lt = rt % p.grp_tiles;
        } else {
            // shared B operand (conv-as-GEMM) or a group count the XCDs do not divide: plain enumeration of (group, row tile)
            g = tmg / p.grp_tiles;
            lt = tmg - g * p.grp_tiles;
        }
        if (g >= p.ngroups) return false;
        row0 = g * p.grp_rows + lt * BMT; rows_end = (g + 1) * p.grp_rows;
        return row0 < rows_end;
    }
    if (TG >= TILE_GROUPS && p.group_off) return tile_group_search<BMT>(p.group_off, p.ngroups, tmg, g, row0, rows_end);
    if constexpr (TG >= TILE_GROUPS) g = blockIdx.z;      // groups that share the row range (band experts)
    row0 = tmg * BMT; rows_end = p.M;
    return row0 < rows_end;
}

// ---- tile feed: DMA (global_load_lds, 16 B / lane, no VGPR staging, no ds_write) of a [ROWS_A + ROWS_B][BKT] ring stage --------------------
// A stage is the A tile followed by the B tile.  A wave-wide DMA instruction fills 1 KB = RPP tile rows; the NWAVES waves share an operand's
// pieces, PA / PB per wave: piece i of a wave covers the tile rows RPP * (wave * P + i) ..., lane -> row + lane / CH, chunk slot lane % CH.
// The pointers live in the caller's arrays (one per piece, k offset 0); a k-tile is selected by the uniform offsets ao / bo of issue().
template <int ROWS_A, int ROWS_B, int BKT, int NWAVES>
struct TileFeed {
    static constexpr int CH = BKT / 8;                      // 16-byte chunks per tile row
    static constexpr int RPP = 64 / CH;                     // tile rows per piece
    static constexpr int PA = ROWS_A / RPP / NWAVES, PB = ROWS_B / RPP / NWAVES;
    static constexpr int LPT = PA + PB;                     // DMA instructions per wave per stage (the unit of the counted vmcnt waits)
    static constexpr int ABYTES = ROWS_A * BKT * 2, BBYTES = ROWS_B * BKT * 2, STAGE = ABYTES + BBYTES;
    static_assert(PA * RPP * NWAVES == ROWS_A && PB * RPP * NWAVES == ROWS_B, "the waves share the pieces evenly");

    // source pointers of one operand's NP pieces: tile row r reads row_of(first + r) of the [.][ld] matrix at `base` - first + r clamped to
    // `clamp` at `end` (out-of-range rows read a valid row and are never stored), r permuted for the P16 column layout when p16
    template <int NP, class RowOf>
    static __device__ __forceinline__ void rows(const bf16_t* (&src)[NP], const bf16_t* base, int ld, int first, int end, int clamp, bool p16,
                                                int wave, int lane, RowOf row_of) {
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const int r = RPP * (wave * NP + i) + lane / CH;
            const int c = (lane % CH) ^ tile_swz<BKT>(r);           // source-side swizzle, see lds_off_t
            int row = first + (p16 ? p16_src_row(r) : r);
            if (row >= end) row = clamp;
            src[i] = base + (int64_t)row_of(row) * ld + c * 8;
        }
    }
    // all pieces of a stage: A's, then B's
    static __device__ __forceinline__ void issue(const bf16_t* const (&a)[PA], const bf16_t* const (&b)[PB], int wave, unsigned char* stage,
                                                 int64_t ao, int64_t bo) {
#pragma unroll
        for (int i = 0; i < PA; ++i)
            __builtin_amdgcn_global_load_lds((glb_ptr_t)(a[i] + ao), (lds_ptr_t)(stage + (wave * PA + i) * 1024), 16, 0, 0);
#pragma unroll
        for (int i = 0; i < PB; ++i)
            __builtin_amdgcn_global_load_lds((glb_ptr_t)(b[i] + bo), (lds_ptr_t)(stage + ABYTES + (wave * PB + i) * 1024), 16, 0, 0);
    }
    // pieces [q0, q1) of both operands, pairwise (A's piece q, B's piece q): what a kernel interleaves with its MFMAs
    static __device__ __forceinline__ void issue(const bf16_t* const (&a)[PA], const bf16_t* const (&b)[PB], int wave, unsigned char* stage,
                                                 int64_t ao, int64_t bo, int q0, int q1) {
        static_assert(PA == PB, "pairwise issue");
#pragma unroll
        for (int i = 0; i < PA; ++i) {
            if (i < q0 || i >= q1) continue;
            __builtin_amdgcn_global_load_lds((glb_ptr_t)(a[i] + ao), (lds_ptr_t)(stage + (wave * PA + i) * 1024), 16, 0, 0);
            __builtin_amdgcn_global_load_lds((glb_ptr_t)(b[i] + bo), (lds_ptr_t)(stage + ABYTES + (wave * PB + i) * 1024), 16, 0, 0);
        }
    }
};
// the feed of a GemmDev launch: A rows gathered (a_rows) or, in conv mode, rows of the clip's padded plane image; per-group operand offsets.
// The P16 row permutation goes to B (weight rows -> 16 consecutive output columns per lane) or, with the operands' roles exchanged, to A.
template <int EPI, class Feed>
__device__ __forceinline__ void gemm_feed_setup(const GemmDev& p, int g, int row0, int rows_end, int n0, bool p16_a, bool p16_b, int wave, int lane,
                                                const bf16_t* (&asrc)[Feed::PA], const bf16_t* (&bsrc)[Feed::PB]) {
    Feed::rows(asrc, p.A + g * p.a_koff_group, p.lda, row0, rows_end, row0, p16_a, wave, lane, [&](int slot) {
        int arow = p.a_rows ? p.a_rows[slot] : slot;
        if constexpr (EPI == EPI_F32_CT) {
            if (p.conv_ktap > 0) arow = g * p.conv_agrp + p.conv_arow0 + (slot - g * p.grp_rows);      // clip g's padded plane image, row of tap 0
        }
        return arow;
    });
    Feed::rows(bsrc, p.B + g * p.b_group_stride, p.ldb, n0, p.N, 0, p16_b, wave, lane, [](int nrow) { return nrow; });
}

// ---- operand offsets of a k-tile -----------------------------------------------------------------------------------------------------
// nseg == 3 (split precision) walks (A_hi, B_hi), (A_lo, B_hi), (A_hi, B_lo): segment 1 reads A's second plane, segment 2 B's
template <int BKT>
__device__ __forceinline__ void gemm_seg_offsets(const GemmDev& p, int seg, int kt, int64_t& ao, int64_t& bo) {
    const int k0 = kt * BKT;
    ao = (seg == 1 ? p.a_plane : 0) + k0;
    bo = (seg == 2 ? p.b_plane : 0) + k0;
}
// step t of the K walk (KT k-tiles per segment) -> offsets; conv mode (EPI_F32_CT, 64-deep tiles): k-tile -> (tap, channel chunk), tap j
// reads the rows j * dil below tap 0's
template <int EPI, int BKT>
__device__ __forceinline__ void gemm_k_offsets(const GemmDev& p, int t, int KT, int64_t& ao, int64_t& bo) {
    const int seg = t / KT, kt = t - seg * KT;
    gemm_seg_offsets<BKT>(p, seg, kt, ao, bo);
    if constexpr (EPI == EPI_F32_CT && BKT == 64) {
        if (p.conv_ktap > 0) {
            const int tap = kt / p.conv_ktap, c0 = (kt - tap * p.conv_ktap) * BKT;
            ao = (seg == 1 ? p.a_plane : 0) + (int64_t)tap * p.conv_dil * p.lda + c0;
            bo = (seg == 2 ? p.b_plane : 0) + (int64_t)tap * p.conv_btap + c0;
        }
    }
}

// ---- the 16-deep MFMA step -----------------------------------------------------------------------------------------------------------
template <int TM, int TN> __device__ __forceinline__ void acc_zero(f32x16 (&acc)[TM][TN]) {
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
}
// fragments of k-step ks (16 deep: chunks ks * 2 + fk) of T 32-row tiles of one operand, from tile row `row` on; lane -> row frow, k half fk
template <int T, int BKT>
__device__ __forceinline__ void frag_load(const unsigned char* S, int row, int ks, int fk, int frow, bf16x8 (&f)[T]) {
#pragma unroll
    for (int i = 0; i < T; ++i) f[i] = *reinterpret_cast<const bf16x8*>(S + lds_off_t<BKT>(row + i * 32 + frow, ks * 2 + fk));
}
// both operands, A's fragments first.  The wave's row / column bases are arguments: 2 x 2, 2 x 4 and 1 x 4 wave layouts all occur.
template <int TM, int TN, int BKT>
__device__ __forceinline__ void frag_load(const unsigned char* As, const unsigned char* Bs, int row_a, int row_b, int ks, int fk, int frow,
                                          bf16x8 (&af)[TM], bf16x8 (&bf)[TN]) {
    frag_load<TM, BKT>(As, row_a, ks, fk, frow, af);
    frag_load<TN, BKT>(Bs, row_b, ks, fk, frow, bf);
}
// The MFMA is issued "swapped" (weights as its A operand), so that a lane owns one output ROW and 4 consecutive output COLUMNS per
// accumulator quad: pairwise epilogues (RoPE, SwiGLU) are lane-local and stores are 8-16 B per lane.
template <int TN> __device__ __forceinline__ void mfma_row(const bf16x8& a, const bf16x8 (&bf)[TN], f32x16 (&acc)[TN]) {
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bf[j], a, acc[j], 0, 0, 0);
}
template <int TM, int TN> __device__ __forceinline__ void mfma_step(const bf16x8 (&af)[TM], const bf16x8 (&bf)[TN], f32x16 (&acc)[TM][TN]) {
#pragma unroll
    for (int i = 0; i < TM; ++i) mfma_row<TN>(af[i], bf, acc[i]);
}

// ---- the K walk of the two-stage 128 x 64 TN kernels (moe_w2_pair_kernel, gemm_bf16_wide_resid_kernel) ---------------------------------------
// issue(t) DMAs k-tile t into stage t % 2 of `lds`.  With one tile ahead the wait is a full drain: tile t landed, barrier (everyone finished
// reading stage (t - 1) % 2), refill that stage with tile t + 1, then the k-steps - the fragments of k-step ks + 1 are read in front of the
// MFMAs of k-step ks, between sched_barriers.  row_a / row_b: the wave's first row of the A / B tile.
template <class Feed, int TN, class Issue>
__device__ __forceinline__ void gemm_walk_2stage(const unsigned char* lds, int total, Issue issue, int row_a, int row_b, int fk, int frow,
                                                 f32x16 (&acc)[2][TN]) {
    constexpr int BKT = Feed::CH * 8;
    issue(0);
    for (int t = 0; t < total; ++t) {
        wait_vmcnt<0>();
        __builtin_amdgcn_s_barrier();
        if (t + 1 < total) issue(t + 1);
        const unsigned char* As = lds + (t % 2) * Feed::STAGE;
        const unsigned char* Bs = As + Feed::ABYTES;
        bf16x8 af[2][2], bf[2][TN];
        frag_load<2, TN, BKT>(As, Bs, row_a, row_b, 0, fk, frow, af[0], bf[0]);
#pragma unroll
        for (int ks = 0; ks < BKT / 16; ++ks) {
            const int cur = ks & 1;
            if (ks + 1 < BKT / 16) frag_load<2, TN, BKT>(As, Bs, row_a, row_b, ks + 1, fk, frow, af[cur ^ 1], bf[cur ^ 1]);
            __builtin_amdgcn_sched_barrier(0);
            mfma_step(af[cur], bf[cur], acc);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
}

// ---- per-block trace record (tuning only, vbdbg_gemm_trace): {t_start, t_loop_end, t_end, prologue cycles << 36 | XCC id << 32 | HW id} --------
__device__ __forceinline__ void gemm_trace_write(const GemmDev& p, unsigned long long t_start, unsigned long long t_pro, unsigned long long t_loop) {
    if (p.trace && threadIdx.x == 0) {
        __builtin_amdgcn_s_waitcnt(0);
        unsigned hwid, xcc;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hwid));
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        unsigned long long* tr = p.trace + (size_t)blockIdx.x * 4;
        tr[0] = t_start; tr[1] = t_loop; tr[2] = __builtin_amdgcn_s_memtime();
        tr[3] = ((unsigned long long)(t_pro - t_start) << 36) | ((unsigned long long)xcc << 32) | hwid;
    }
}
