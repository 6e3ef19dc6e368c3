// The 8-wave K/V tile stream of the window, split and packed prefill kernels (prefill_window_kernel.hip,
// prefill_split_kernel.hip, prefill_varlen_kernel.hip, prefill_varlen_window_kernel.hip): one copy of the staging
// scaffold those kernels walk their key range with, and of the pieces around it that they share.
//
// The pipeline is prefill_kernel.hip's (design notes there; that file keeps its own instance, with q-tile pairs and the
// PF / ORD / DIAG builds): a q-tile of 256 query rows, 8 waves of 32 rows, 64-key K/V tiles staged through registers into
// triple-buffered padded LDS images with one barrier per tile, and prefill_core.h's slot-ordered half-step h_block at
// exact scale (ORD 2, PF 2).
//   * A thread owns NLD 16-byte chunks of every K and every V tile.  The staging registers are four named uint4: arrays
//     of them ended up in scratch (prefill_kernel.hip).
//   * Stream position t is tile ts0 + t of the workgroup's range [ts0, wg_end).  Before step t, positions t and t + 1 (K)
//     and t (V) are in LDS and t + 2 (K), t + 1 (V) are in flight in the staging registers.  A position past the end
//     re-reads the range's last tile, so nothing outside the range is read.
//   * A wave computes on the positions [tw0, ntw) and only stages during the workgroup's others: leading idle steps
//     (lower bound only), FULL steps with the ds_writes in the PV slots of the first half-step and the global loads in
//     the QK slots of the second, one TAIL step, trailing idle steps.
//   * Never read: the ragged last tile (Sk % 64 != 0) clamps its rows to the last valid one; with a lower bound the tile
//     that holds it clamps its rows up to the first valid one (a masked key has weight 0, but 0 * NaN is NaN in P.V).
// Whether a lower bound exists is the type of the LowMask hook: with prefill_core.h's NoLowMask none of the first-row
// clamp, the leading idle loop or the lower mask is compiled.
#pragma once
#include "prefill_core.h"

namespace sfa {
namespace prefill {

template <int D>
struct StreamDims {
    static constexpr int NKS = D / 16;                  // k-steps of Q.K^T
    static constexpr int NDB = D / 32;                  // 32-wide d blocks of O^T
    static constexpr int NPV_ = 2 * NDB;
    static constexpr int CPR = D / 8;                   // 16-B chunks per row
    static constexpr int NLD = kBN * CPR / kThreads;    // chunks staged per thread per tile (2 or 1)
    static constexpr int ROWSTEP = kThreads / CPR;      // row distance between a thread's chunks
    static constexpr int NOPS = 2 * NLD;                // op n: even = K chunk n/2, odd = V chunk n/2
    static_assert(NLD >= 1 && NLD <= 2, "staging registers are named kr0, kr1");
};

// What a kernel tells tile_stream about its walk (all of it workgroup-uniform but tw0 / ntw, which are wave-uniform).
struct TileStream {
    const uint16_t *k, *v;              // key 0 of this (batch or sequence, kv head)
    long long k_stride, v_stride;       // elements between two keys
    int Sk;                             // keys of the batch or sequence: where the ragged last tile ends
    int ts0, wg_end, nt;                // the workgroup stages the tiles [ts0, wg_end); nt = max(0, wg_end - ts0)
    int ntw;                            // the wave computes on the stream positions [tw0, ntw)
    int tw0, tlo, first0;               // lower bound only: the tile that holds it and its first valid row there
};

// The window's lower mask of a half-tile of fresh scores (mask_half's register layout): keys below lo get -inf
__device__ __forceinline__ void mask_below(f32x16 &s, int kbase, int h2, int lo) {
#pragma unroll
    for (int r = 0; r < 16; ++r)
        if (kbase + (r & 3) + 8 * (r >> 2) + 4 * h2 < lo) s[r] = ninf();
}

__device__ __forceinline__ constexpr int next3(int x, int tile) { return x == 2 * tile ? 0 : x + tile; }

// The walk: every tile of [ts0, wg_end) through LDS, this wave's share of them into acc (initialised here; left empty --
// zeros, max -inf, sum 0 -- when the wave sees no key).  qp = &Q[row][8 * h2] of this lane's query row; mask_bits(kbase):
// bit 0 set when the 32 keys from kbase need masking for this wave's rows; lim: the last visible key of this lane's row
// (< 0: none).
template <class Tr, int D, class MaskBits, class LowMask>
__device__ __forceinline__ void tile_stream(char *smem, const TileStream &a, const uint16_t *qp, Acc<D, 1> &acc, float c2,
                                            int h2, const int (&lim)[1], const MaskBits &mask_bits,
                                            const LowMask &low_mask) {
    using Vec = typename Tr::mfma_vec;
    using SD = StreamDims<D>;
    using L = Lds<D>;
    constexpr int NQB = 1, PF = 2, ORD = 2;     // one 32-row query block per wave, exact scale, staged softmax
    constexpr int NKS = SD::NKS, NDB = SD::NDB, NPV_ = SD::NPV_, CPR = SD::CPR, NLD = SD::NLD, ROWSTEP = SD::ROWSTEP,
                  NOPS = SD::NOPS;
    constexpr bool LOW = !std::is_same<LowMask, NoLowMask>::value;
    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31;
    const int ts0 = a.ts0, wg_end = a.wg_end, nt = a.nt, ntw = a.ntw;

    // ---- staging: thread owns chunks (row st_row + i*ROWSTEP, chunk st_ch), i < NLD, of every tile ----
    const int st_row = tid / CPR, st_ch = tid % CPR;
    const char *const kg = reinterpret_cast<const char *>(a.k);    // uniform
    const char *const vg = reinterpret_cast<const char *>(a.v);
    const long long k_tile_bytes = 2ll * kBN * a.k_stride, v_tile_bytes = 2ll * kBN * a.v_stride;
    const unsigned k_rowb = (unsigned)(2 * a.k_stride), v_rowb = (unsigned)(2 * a.v_stride);
    char *const k_w = smem + L::KS * st_row + 16 * st_ch;
    char *const v_w = smem + L::V_BASE + L::VS * st_row + 16 * st_ch;
    uint4 kr0, kr1, vr0, vr1;       // plain scalars: arrays of these ended up in scratch (prefill_kernel.hip)
    kr0 = kr1 = vr0 = vr1 = make_uint4(0, 0, 0, 0);

    // Rows of a tile: row r is at r * row bytes from the tile's base.  The ragged last tile clamps its rows to the last
    // valid one, the tile that holds the lower bound to the first valid one (one tile may be both).
    const int n_kv_tiles = (a.Sk + kBN - 1) / kBN;
    const int ragged_tile = (a.Sk % kBN) ? n_kv_tiles - 1 : -1;
    const int last0 = a.Sk - 1 - (n_kv_tiles - 1) * kBN;    // last valid row of the last tile
    const int row0_ = st_row, row1_ = st_row + ROWSTEP;
    const unsigned ch_off = 16u * st_ch;
    // where the K and V tiles of two stream positions live and which of their rows exist: once per step, scalar
    struct TileSrc { const char *k, *v; int fk, lk, fv, lv; };
    auto tile_of = [&](int pos) -> int { return min(ts0 + pos, wg_end - 1); };     // past the end: re-read the last tile
    auto tile_src = [&](int pos_k, int pos_v) -> TileSrc {
        const int tk = tile_of(pos_k), tv = tile_of(pos_v);
        return TileSrc{kg + tk * k_tile_bytes, vg + tv * v_tile_bytes,
                       LOW && tk == a.tlo ? a.first0 : 0, tk == ragged_tile ? last0 : kBN - 1,
                       LOW && tv == a.tlo ? a.first0 : 0, tv == ragged_tile ? last0 : kBN - 1};
    };
    auto row_off = [&](int row, int first, int last, unsigned rowb) -> unsigned {
        if constexpr (LOW) row = max(row, first);
        return (unsigned)min(row, last) * rowb + ch_off;
    };
    auto ld_k = [&](const TileSrc &ts, int i) -> uint4 {
        return *reinterpret_cast<const uint4 *>(ts.k + row_off(i == 0 ? row0_ : row1_, ts.fk, ts.lk, k_rowb));
    };
    auto ld_v = [&](const TileSrc &ts, int i) -> uint4 {
        return *reinterpret_cast<const uint4 *>(ts.v + row_off(i == 0 ? row0_ : row1_, ts.fv, ts.lv, v_rowb));
    };
    auto load_op = [&](int n, const TileSrc &ts) {
        if (n == 0) kr0 = ld_k(ts, 0);
        if (n == 1) vr0 = ld_v(ts, 0);
        if (NLD > 1 && n == 2) kr1 = ld_k(ts, 1);
        if (NLD > 1 && n == 3) vr1 = ld_v(ts, 1);
    };
    auto store_op = [&](int n, int kbuf, int vbuf) {
        if (n == 0) *reinterpret_cast<uint4 *>(k_w + kbuf) = kr0;
        if (n == 1) *reinterpret_cast<uint4 *>(v_w + vbuf) = vr0;
        if (NLD > 1 && n == 2) *reinterpret_cast<uint4 *>(k_w + kbuf + ROWSTEP * L::KS) = kr1;
        if (NLD > 1 && n == 3) *reinterpret_cast<uint4 *>(v_w + vbuf + ROWSTEP * L::VS) = vr1;
    };

    // the two LDS read bases of this lane (everything else is an immediate)
    const char *const k_rd = smem + L::KS * l31 + 16 * h2;                 // K row l31, chunk h2
    const char *const v_rd = smem + L::V_BASE + L::VS * (4 * h2 + ((lane & 15) >> 2)) +
                             32 * ((lane >> 4) & 1) + 16 * ((lane & 3) >> 1) + 8 * (lane & 1);

    // ---- Q^T fragments (B operand): lane holds Q[row][16ks + 8*h2 .. +8] ----
    Vec qf[NQB][NKS];
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) qf[0][ks] = bitcast<Vec>(*reinterpret_cast<const uint4 *>(qp + 16 * ks));

#pragma unroll
    for (int d = 0; d < NDB; ++d)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc.o[0][d][r] = 0.f;
    acc.msc[0] = ninf();
    acc.lsum[0] = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc.cinit[0][r] = 0.f;
    if (nt <= 0) return;

    // ---- staging prologue (prefill_kernel.hip): stream positions 0 and 1 into LDS, 2 (K) and 1 (V) in flight ----
    uint4 kx0, kx1;                         // K(1), prologue only
    {
        const TileSrc ts0_ = tile_src(0, 0);
#pragma unroll
        for (int n = 0; n < NOPS; ++n) load_op(n, ts0_);
        const TileSrc ts1_ = tile_src(1, 1);
        kx0 = ld_k(ts1_, 0);
        kx1 = NLD > 1 ? ld_k(ts1_, 1) : make_uint4(0, 0, 0, 0);
    }
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) asm volatile("" : "+v"(qf[0][ks]));   // launder: prefill_kernel.hip
#pragma unroll
    for (int n = 0; n < NOPS; ++n) store_op(n, 0, 0);
    *reinterpret_cast<uint4 *>(k_w + L::KTILE) = kx0;
    if (NLD > 1) *reinterpret_cast<uint4 *>(k_w + L::KTILE + ROWSTEP * L::KS) = kx1;
    __syncthreads();
    {
        const TileSrc ts1 = tile_src(2, 1);
#pragma unroll
        for (int n = 0; n < NOPS; ++n) load_op(n, ts1);
    }

    int kcur = 0, vcur = 0;     // byte offsets of the K and V buffers of stream position t
    int t = 0;                  // stream position (tile ts0 + t)
    auto advance = [&]() {
        kcur = next3(kcur, L::KTILE);
        vcur = next3(vcur, L::VTILE);
    };
    // non-overlapped form of the staging (TAIL and idle steps): store, sync, load
    auto stage_and_sync = [&](int pos) {
        const int k1_ = next3(kcur, L::KTILE);
#pragma unroll
        for (int n = 0; n < NOPS; ++n) store_op(n, next3(k1_, L::KTILE), next3(vcur, L::VTILE));
        __syncthreads();
        const TileSrc ts_ = tile_src(pos + 3, pos + 2);
#pragma unroll
        for (int n = 0; n < NOPS; ++n) load_op(n, ts_);
        SFA_FENCE();
    };

    f32x16 sA[NQB], sB[NQB];
    float mxA[NQB] = {ninf()}, mxB[NQB] = {ninf()};     // lane-local maxima of the pending half-tiles
#pragma unroll
    for (int r = 0; r < 16; ++r) { sA[0][r] = 0.f; sB[0][r] = 0.f; }
    Vec kpre[PF];                                       // first PF K fragments of the next half-step
#pragma unroll
    for (int i = 0; i < PF; ++i) kpre[i] = bitcast<Vec>(make_uint4(0, 0, 0, 0));
    // ---- leading idle steps: tiles below every row of this wave ----
    if constexpr (LOW) {
        for (; t < a.tw0; ++t) {
            stage_and_sync(t);
            advance();
        }
    }
    // ---- scores of the first half-tile, first fragments of the second ----
    if (t < ntw) {
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) {
            const Vec f = bitcast<Vec>(*reinterpret_cast<const uint4 *>(k_rd + kcur + 32 * ks));
            sA[0] = Tr::mfma32(f, qf[0][ks], sA[0]);
        }
#pragma unroll
        for (int i = 0; i < PF; ++i)
            kpre[i] = bitcast<Vec>(*reinterpret_cast<const uint4 *>(k_rd + kcur + L::KS * 32 + 32 * i));
        mxA[0] = lane_rowmax(sA[0]);
    }

    // ---- FULL steps: this wave needs the next tile as well.  Staging is spread under the MFMAs:
    // the ds_writes ride in the PV slots of H1, the global loads in the QK slots of H2.
    for (; t + 1 < ntw; ++t) {
        const int k1 = next3(kcur, L::KTILE), k2 = next3(k1, L::KTILE);
        const int v1 = next3(vcur, L::VTILE);
        const char *kb = k_rd + kcur, *vb = v_rd + vcur, *kb1 = k_rd + k1;
        const int kbase = (ts0 + t) * kBN;
        auto st_hook = [&](int j) {         // NOPS stores spread evenly over the NPV slots
#pragma unroll
            for (int n = j * NOPS / NPV_; n < (j + 1) * NOPS / NPV_; ++n) store_op(n, k2, v1);
        };
        h_block<Tr, D, NQB, PF, ORD, 1, 0, true, true>(kb, vb, kb1, qf, sB, sA, acc, c2, mxA, mxB,
                                                       mask_bits(kbase), kbase, h2, lim, kpre, NoHook(), st_hook, low_mask);
        __syncthreads();
        const TileSrc ts = tile_src(t + 3, t + 2);
        auto ld_hook = [&](int i) {         // NOPS loads spread evenly over QK slots 1..NKS-1
#pragma unroll
            for (int n = (i - 1) * NOPS / (NKS - 1); n < i * NOPS / (NKS - 1); ++n) load_op(n, ts);
        };
        h_block<Tr, D, NQB, PF, ORD, 0, 1, true, true>(kb1, vb, kb1, qf, sA, sB, acc, c2, mxB, mxA,
                                                       mask_bits(kbase + 32), kbase + 32, h2, lim, kpre, ld_hook, NoHook(), low_mask);
        advance();
    }
    // ---- TAIL step: this wave's last tile (its second half computes no new scores) ----
    if (t < ntw) {
        const char *kb = k_rd + kcur, *vb = v_rd + vcur;
        const int kbase = (ts0 + t) * kBN;
        h_block<Tr, D, NQB, PF, ORD, 1, 0, true, false>(kb, vb, kb, qf, sB, sA, acc, c2, mxA, mxB,
                                                        mask_bits(kbase), kbase, h2, lim, kpre, NoHook(), NoHook(), low_mask);
        stage_and_sync(t);
        h_block<Tr, D, NQB, PF, ORD, 0, 1, false, false>(kb, vb, kb, qf, sA, sB, acc, c2, mxB, mxA,
                                                         mask_bits(kbase + 32), kbase + 32, h2, lim, kpre, NoHook(), NoHook(), low_mask);
        advance();
        ++t;
    }
    // ---- trailing idle steps (tiles beyond this wave's causal limit): keep staging for the others ----
    for (; t < nt; ++t) {
        stage_and_sync(t);
        advance();
    }
}

// The attention sink: one more stream element of the row -- max sink log2(e), sum 1, accumulator 0 -- folded into the
// row's state once, after the walk.  A row with no visible key (ltot == 0) stays empty: the sink joins only a softmax that
// has a key.  sink is the head's logit in natural-log units.
template <int D>
__device__ __forceinline__ void fold_sink(Acc<D, 1> &acc, float &ltot, float sink) {
    // (laundered: contracted into `sk - ms` below as one fma, the product's rounding error would stand where 0 belongs when
    // the sink is the max)
    float sk = sink * 1.4426950408889634f;
    asm volatile("" : "+v"(sk));
    const bool has = ltot > 0.f;
    const float mn = fmaxf(acc.msc[0], sk);
    const float ms = (mn == ninf()) ? 0.f : mn;
    const float a1 = fast_exp2(acc.msc[0] - ms);
#pragma unroll
    for (int d = 0; d < D / 32; ++d)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc.o[0][d][r] *= a1;
    ltot = has ? __builtin_fmaf(ltot, a1, fast_exp2(sk - ms)) : 0.f;
    acc.msc[0] = has ? mn : acc.msc[0];
}

// Normalise, convert and store this lane's share of O[row][:] at orow, and the row's lse at lse[lse_idx] (lse may be null).
// A row with no visible key (ltot == 0) gets zeros and -inf.  For the lanes of rows that exist only.
template <class Tr, int D>
__device__ __forceinline__ void store_row(const Acc<D, 1> &acc, float ltot, uint16_t *orow, float *lse, long long lse_idx,
                                          int h2) {
    const float inv = ltot > 0.f ? 1.0f / ltot : 0.f;
    store_o_row<Tr, D>(orow, acc.o[0], inv, h2);
    if (lse && h2 == 0) lse[lse_idx] = ltot > 0.f ? (acc.msc[0] + __log2f(ltot)) * kLn2 : ninf();
}

}  // namespace prefill
}  // namespace sfa
