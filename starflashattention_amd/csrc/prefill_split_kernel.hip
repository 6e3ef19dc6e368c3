// Prefill forward with a split key range for gfx950 (MI355X): sfa_prefill_split_fwd with two or more splits.
// bf16 / fp16, head_dim 64 / 128, causal (bottom-right aligned) or full, MHA or GQA, [B, H, S, D] tensors with any strides.
//
// Two kernels on one stream:
//   prefill_split_kernel          one workgroup per (batch, head, q-tile, split): the tiles [s C, min((s + 1) C, nkt(qt))) of
//                                 the q-tile's key range, C = tiles_per_split, into fp32 partials (O un-normalised, the
//                                 reference max m in log2 units, the row sum l) in the workspace
//   prefill_split_combine_kernel  per query row: m = max m_s, l = sum 2^(m_s - m) l_s, o = sum 2^(m_s - m) O_s / l,
//                                 lse = (m + log2 l) ln 2, over the splits that are not empty for the row's q-tile
// The tile pipeline is prefill_window_kernel.hip's walk of [ts0, wg_end) (design notes: prefill_kernel.hip): a q-tile of
// 256 query rows, 8 waves of 32 rows, 64-key K/V tiles staged through registers into triple-buffered padded LDS images
// with one barrier per tile, and prefill_core.h's slot-ordered half-step h_block at exact scale (ORD 2, PF 2).  The
// staging scaffold is a copy of that file's (a candidate for sharing once a third user appears).  What differs:
//   * The key range comes from the split index, not from a window: no lower mask, no first-tile clamp, no sink.
//   * A wave computes on the split's tiles up to its last row's causal limit and only stages during the others; a wave
//     whose rows see nothing in this split ends with (m, l) = (-inf, 0) for them.
//   * Full attention (CAUSAL false): every row's limit is Sk - 1, so the same mask hook masks the ragged last tile.
//   * Never read: the ragged last tile clamps its rows to Sk - 1; a stream position past the split's end re-reads the
//     split's own last tile; an empty split's workgroup exits before it reads anything.
//   * The epilogue writes the row's partial: each lane owns 4 consecutive floats of every 8-column group of O^T's
//     accumulator layout, so the partial goes out as 16-byte stores with no lane exchange.
// blockIdx -> (head, q-tile, split) is block_coord's XCD-aware order (prefill_common.h) with the split index as the
// fastest digit: the splits of one (head, q-tile) are neighbours on one XCD and share its L2 for their Q rows.
#include "prefill_core.h"

namespace sfa {

namespace {

using namespace prefill;

// tiles the last row of q-tile qt sees (the partition of include/star_flash_attn.h)
template <bool CAUSAL>
__device__ __forceinline__ int tiles_of_qtile(const PrefillKernelParams &p, int qt) {
    const int nkt_max = (p.Sk + kBN - 1) / kBN;
    if (!CAUSAL) return nkt_max;
    const int lim = min(kBM * (qt + 1), p.Sq) - 1 + p.Sk - p.Sq;
    return lim < 0 ? 0 : lim / kBN + 1;
}

template <class Tr, int D, bool CAUSAL>
__global__ void __launch_bounds__(kThreads, 2)
prefill_split_kernel(const PrefillSplitKernelParams sp) {
    using Vec = typename Tr::mfma_vec;
    constexpr int NQB = 1, PF = 2, ORD = 2;     // one 32-row query block per wave, exact scale, staged softmax
    constexpr int NKS = D / 16;                 // k-steps of Q.K^T
    constexpr int NDB = D / 32;                 // 32-wide d blocks of O^T
    constexpr int NPV_ = 2 * NDB;
    constexpr int CPR = D / 8;                  // 16-B chunks per row
    constexpr int NLD = kBN * CPR / kThreads;   // chunks staged per thread per tile (2 or 1)
    constexpr int ROWSTEP = kThreads / CPR;     // row distance between a thread's chunks
    using L = Lds<D>;
    static_assert(NLD >= 1 && NLD <= 2, "staging registers are named kr0, kr1");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const PrefillKernelParams &p = sp.base;

    // block_coord's map with (q-tile, split) in the place of the q-tile: XCD x owns heads [x*bh_per_xcd, (x+1)*bh_per_xcd)
    // and walks each head's q-tiles heaviest-first, the splits of a q-tile side by side
    const int S = sp.num_splits;
    const int slot = blockIdx.x >> 3;
    const int per_head = p.nq_tiles * S;
    const int bh = (blockIdx.x & 7) * p.bh_per_xcd + slot / per_head;
    if (bh >= p.B * p.Hq) return;
    const int in_head = slot % per_head;
    const int qt = p.nq_tiles - 1 - in_head / S, split = in_head % S;
    const int b = bh / p.Hq, h = bh % p.Hq;
    const int hk = h / (p.Hq / p.Hkv);

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);     // provably wave-uniform
    const int l31 = lane & 31, h2 = lane >> 5;
    const int coff = p.Sk - p.Sq;               // causal: key j visible to row i iff j <= i + coff
    const int q0 = qt * kBM, wq0 = q0 + 32 * wave, qrow = wq0 + l31;

    // ---- the key range of this workgroup: tiles [ts0, wg_end) ----
    const int ts0 = split * sp.tiles_per_split;
    const int wg_end = min(ts0 + sp.tiles_per_split, tiles_of_qtile<CAUSAL>(p, qt));
    const int nt = wg_end - ts0;                // tiles the workgroup stages (workgroup-uniform)
    if (nt <= 0) return;                        // an empty split: nothing read, nothing written (the combine skips it)
    const int wlast = min(wq0 + 31, p.Sq - 1);  // last query row of the wave
    int ntw = 0;                                // end of the tiles this wave computes on, from ts0 (wave-uniform)
    if (wq0 < p.Sq) {
        if (!CAUSAL) ntw = nt;
        else if (wlast + coff >= 0) ntw = max(0, min(wg_end, (wlast + coff) / kBN + 1) - ts0);
    }
    int lim[NQB];                               // last visible key of this lane's row (< 0: none)
    lim[0] = CAUSAL ? min(qrow, p.Sq - 1) + coff : p.Sk - 1;
    const int wlim = CAUSAL ? wq0 + coff : p.Sk - 1;    // the smallest limit of the wave's rows
    // bit 0 set: the 32 keys starting at KBASE need masking for this wave's rows
    auto mask_bits = [&](int kbase) -> int { return kbase + 31 > wlim ? 1 : 0; };

    // ---- staging: thread owns chunks (row st_row + i*ROWSTEP, chunk st_ch), i < NLD, of every tile ----
    const int st_row = tid / CPR, st_ch = tid % CPR;
    const char *const kg = reinterpret_cast<const char *>(p.k + b * p.ks[0] + hk * p.ks[1]);   // uniform
    const char *const vg = reinterpret_cast<const char *>(p.v + b * p.vs[0] + hk * p.vs[1]);
    const long long k_tile_bytes = 2ll * kBN * p.ks[2], v_tile_bytes = 2ll * kBN * p.vs[2];
    const unsigned k_rowb = (unsigned)(2 * p.ks[2]), v_rowb = (unsigned)(2 * p.vs[2]);
    char *const k_w = smem + L::KS * st_row + 16 * st_ch;
    char *const v_w = smem + L::V_BASE + L::VS * st_row + 16 * st_ch;
    uint4 kr0, kr1, vr0, vr1;       // plain scalars: arrays of these ended up in scratch (prefill_kernel.hip)
    kr0 = kr1 = vr0 = vr1 = make_uint4(0, 0, 0, 0);

    // Rows of a tile: row r is at r * row bytes from the tile's base.  The ragged last tile (Sk % 64 != 0) clamps its
    // rows to the last valid one: nothing past Sk is read.
    const int n_kv_tiles = (p.Sk + kBN - 1) / kBN;
    const int ragged_tile = (p.Sk % kBN) ? n_kv_tiles - 1 : -1;
    const int last0 = p.Sk - 1 - (n_kv_tiles - 1) * kBN;    // last valid row of the last tile
    const int row0_ = st_row, row1_ = st_row + ROWSTEP;
    const unsigned ch_off = 16u * st_ch;
    constexpr int NOPS = 2 * NLD;   // op n: even = K chunk n/2, odd = V chunk n/2
    // where the K and V tiles of two stream positions live and which of their rows exist: once per step, scalar
    struct TileSrc { const char *k, *v; int lk, lv; };
    auto tile_of = [&](int pos) -> int { return min(ts0 + pos, wg_end - 1); };     // past the end: re-read the last tile
    auto tile_src = [&](int pos_k, int pos_v) -> TileSrc {
        const int tk = tile_of(pos_k), tv = tile_of(pos_v);
        return TileSrc{kg + tk * k_tile_bytes, vg + tv * v_tile_bytes,
                       tk == ragged_tile ? last0 : kBN - 1, tv == ragged_tile ? last0 : kBN - 1};
    };
    auto row_off = [&](int row, int last, unsigned rowb) -> unsigned { return (unsigned)min(row, last) * rowb + ch_off; };
    auto ld_k = [&](const TileSrc &ts, int i) -> uint4 {
        return *reinterpret_cast<const uint4 *>(ts.k + row_off(i == 0 ? row0_ : row1_, ts.lk, k_rowb));
    };
    auto ld_v = [&](const TileSrc &ts, int i) -> uint4 {
        return *reinterpret_cast<const uint4 *>(ts.v + row_off(i == 0 ? row0_ : row1_, ts.lv, v_rowb));
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

    const float c2 = p.scale_log2;
    // the two LDS read bases of this lane (everything else is an immediate)
    const char *const k_rd = smem + L::KS * l31 + 16 * h2;                 // K row l31, chunk h2
    const char *const v_rd = smem + L::V_BASE + L::VS * (4 * h2 + ((lane & 15) >> 2)) +
                             32 * ((lane >> 4) & 1) + 16 * ((lane & 3) >> 1) + 8 * (lane & 1);

    // ---- Q^T fragments (B operand): lane holds Q[row][16ks + 8*h2 .. +8] ----
    Vec qf[NQB][NKS];
    {
        const uint16_t *qp = p.q + b * p.qs[0] + h * p.qs[1] + (long long)min(qrow, p.Sq - 1) * p.qs[2] + 8 * h2;
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) qf[0][ks] = bitcast<Vec>(*reinterpret_cast<const uint4 *>(qp + 16 * ks));
    }

    Acc<D, NQB> acc;
#pragma unroll
    for (int d = 0; d < NDB; ++d)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc.o[0][d][r] = 0.f;
    acc.msc[0] = ninf();
    acc.lsum[0] = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc.cinit[0][r] = 0.f;

    {
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
#define SFA_NEXT3(X, TILE) (((X) == 2 * (TILE)) ? 0 : (X) + (TILE))
#define SFA_ADVANCE()                                                                               \
    do {                                                                                            \
        kcur = SFA_NEXT3(kcur, L::KTILE);                                                           \
        vcur = SFA_NEXT3(vcur, L::VTILE);                                                           \
    } while (0)
    // non-overlapped form of the staging (TAIL and idle steps): store, sync, load
#define SFA_STAGE_AND_SYNC(T)                                                                       \
    do {                                                                                            \
        const int k1_ = SFA_NEXT3(kcur, L::KTILE);                                                  \
        _Pragma("unroll") for (int n_ = 0; n_ < NOPS; ++n_)                                         \
            store_op(n_, SFA_NEXT3(k1_, L::KTILE), SFA_NEXT3(vcur, L::VTILE));                      \
        __syncthreads();                                                                            \
        const TileSrc ts_ = tile_src((T) + 3, (T) + 2);                                             \
        _Pragma("unroll") for (int n_ = 0; n_ < NOPS; ++n_) load_op(n_, ts_);                       \
        SFA_FENCE();                                                                                \
    } while (0)

        f32x16 sA[NQB], sB[NQB];
        float mxA[NQB] = {ninf()}, mxB[NQB] = {ninf()};     // lane-local maxima of the pending half-tiles
#pragma unroll
        for (int r = 0; r < 16; ++r) { sA[0][r] = 0.f; sB[0][r] = 0.f; }
        Vec kpre[PF];                                       // first PF K fragments of the next half-step
#pragma unroll
        for (int i = 0; i < PF; ++i) kpre[i] = bitcast<Vec>(make_uint4(0, 0, 0, 0));
        // ---- scores of the first half-tile, first fragments of the second ----
        if (t < ntw) {
#pragma unroll
            for (int ks = 0; ks < NKS; ++ks) {
                const Vec a = bitcast<Vec>(*reinterpret_cast<const uint4 *>(k_rd + kcur + 32 * ks));
                sA[0] = Tr::mfma32(a, qf[0][ks], sA[0]);
            }
#pragma unroll
            for (int i = 0; i < PF; ++i)
                kpre[i] = bitcast<Vec>(*reinterpret_cast<const uint4 *>(k_rd + kcur + L::KS * 32 + 32 * i));
            mxA[0] = lane_rowmax(sA[0]);
        }

        // ---- FULL steps: this wave needs the next tile as well.  Staging is spread under the MFMAs:
        // the ds_writes ride in the PV slots of H1, the global loads in the QK slots of H2.
        for (; t + 1 < ntw; ++t) {
            const int k1 = SFA_NEXT3(kcur, L::KTILE), k2 = SFA_NEXT3(k1, L::KTILE);
            const int v1 = SFA_NEXT3(vcur, L::VTILE);
            const char *kb = k_rd + kcur, *vb = v_rd + vcur, *kb1 = k_rd + k1;
            const int kbase = (ts0 + t) * kBN;
            auto st_hook = [&](int j) {         // NOPS stores spread evenly over the NPV slots
#pragma unroll
                for (int n = j * NOPS / NPV_; n < (j + 1) * NOPS / NPV_; ++n) store_op(n, k2, v1);
            };
            h_block<Tr, D, NQB, PF, ORD, 1, 0, true, true>(kb, vb, kb1, qf, sB, sA, acc, c2, mxA, mxB,
                                                           mask_bits(kbase), kbase, h2, lim, kpre, NoHook(), st_hook);
            __syncthreads();
            const TileSrc ts = tile_src(t + 3, t + 2);
            auto ld_hook = [&](int i) {         // NOPS loads spread evenly over QK slots 1..NKS-1
#pragma unroll
                for (int n = (i - 1) * NOPS / (NKS - 1); n < i * NOPS / (NKS - 1); ++n) load_op(n, ts);
            };
            h_block<Tr, D, NQB, PF, ORD, 0, 1, true, true>(kb1, vb, kb1, qf, sA, sB, acc, c2, mxB, mxA,
                                                           mask_bits(kbase + 32), kbase + 32, h2, lim, kpre, ld_hook, NoHook());
            SFA_ADVANCE();
        }
        // ---- TAIL step: this wave's last tile (its second half computes no new scores) ----
        if (t < ntw) {
            const char *kb = k_rd + kcur, *vb = v_rd + vcur;
            const int kbase = (ts0 + t) * kBN;
            h_block<Tr, D, NQB, PF, ORD, 1, 0, true, false>(kb, vb, kb, qf, sB, sA, acc, c2, mxA, mxB,
                                                            mask_bits(kbase), kbase, h2, lim, kpre, NoHook(), NoHook());
            SFA_STAGE_AND_SYNC(t);
            h_block<Tr, D, NQB, PF, ORD, 0, 1, false, false>(kb, vb, kb, qf, sA, sB, acc, c2, mxB, mxA,
                                                             mask_bits(kbase + 32), kbase + 32, h2, lim, kpre, NoHook(), NoHook());
            SFA_ADVANCE();
            ++t;
        }
        // ---- trailing idle steps (tiles beyond this wave's causal limit): keep staging for the others ----
        for (; t < nt; ++t) {
            SFA_STAGE_AND_SYNC(t);
            SFA_ADVANCE();
        }
#undef SFA_NEXT3
#undef SFA_ADVANCE
#undef SFA_STAGE_AND_SYNC
    }

    // ---- epilogue: the row's partial -- O un-normalised, (m, l) -- to the workspace ----
    const float ltot = half_sum(acc.lsum[0]);
    if (qrow < p.Sq) {
        const size_t pidx = (((size_t)bh * p.nq_tiles + qt) * S + split) * kBM + (qrow - q0);
        float *prow = sp.part_o + pidx * D + 4 * h2;
#pragma unroll
        for (int d = 0; d < NDB; ++d)
#pragma unroll
            for (int g = 0; g < 4; ++g)         // this lane's columns 32 d + 8 g + 4 h2 .. + 3
                *reinterpret_cast<float4 *>(prow + 32 * d + 8 * g) =
                    make_float4(acc.o[0][d][4 * g], acc.o[0][d][4 * g + 1], acc.o[0][d][4 * g + 2], acc.o[0][d][4 * g + 3]);
        if (h2 == 0) sp.part_ml[pidx] = make_float2(acc.msc[0], ltot);
    }
}

// One thread per 4 columns of one query row; the D / 4 lanes of a row sit side by side in a wave (2 rows per wave at
// head_dim 128, 4 at 64) and read each partial row as one run of 16-byte loads.
template <class Tr, int D, bool CAUSAL>
__global__ void __launch_bounds__(256)
prefill_split_combine_kernel(const PrefillSplitKernelParams sp) {
    constexpr int LPR = D / 4;                  // lanes per row
    constexpr int RPB = 256 / LPR;              // rows per block
    const PrefillKernelParams &p = sp.base;
    const int nrb = (p.Sq + RPB - 1) / RPB;     // blocks per (batch, head)
    const int bh = blockIdx.x / nrb;
    const int row = (blockIdx.x % nrb) * RPB + threadIdx.x / LPR, col = 4 * (threadIdx.x % LPR);
    if (row >= p.Sq) return;
    const int qt = row / kBM;
    const int C = sp.tiles_per_split;
    // the splits that are not empty for this q-tile: the others were never written and are not read
    const int ns = min(sp.num_splits, (tiles_of_qtile<CAUSAL>(p, qt) + C - 1) / C);
    const size_t pidx0 = (((size_t)bh * p.nq_tiles + qt) * sp.num_splits) * kBM + (row - qt * kBM);
    const float2 *ml = sp.part_ml + pidx0;
    float m = ninf();
    for (int s = 0; s < ns; ++s) {
        const float2 e = ml[(size_t)s * kBM];
        if (e.y > 0.f) m = fmaxf(m, e.x);       // a partial with no key (l = 0) is skipped, never multiplied
    }
    float l = 0.f;
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
    const float *po = sp.part_o + pidx0 * D + col;
    for (int s = 0; s < ns; ++s) {
        const float2 e = ml[(size_t)s * kBM];
        if (!(e.y > 0.f)) continue;
        const float w = fast_exp2(e.x - m);
        const float4 x = *reinterpret_cast<const float4 *>(po + (size_t)s * kBM * D);
        l = __builtin_fmaf(w, e.y, l);
        o.x = __builtin_fmaf(w, x.x, o.x);
        o.y = __builtin_fmaf(w, x.y, o.y);
        o.z = __builtin_fmaf(w, x.z, o.z);
        o.w = __builtin_fmaf(w, x.w, o.w);
    }
    const float inv = l > 0.f ? 1.0f / l : 0.f;         // no partial with a key: zeros and -inf
    const int b = bh / p.Hq, h = bh % p.Hq;
    uint16_t *orow = p.o + b * p.os[0] + h * p.os[1] + (long long)row * p.os[2] + col;
    *reinterpret_cast<uint2 *>(orow) = make_uint2(Tr::pack2(o.x * inv, o.y * inv), Tr::pack2(o.z * inv, o.w * inv));
    if (p.lse && col == 0) p.lse[(long long)bh * p.Sq + row] = l > 0.f ? (m + __log2f(l)) * kLn2 : ninf();
}

template <class Tr, int D, bool CAUSAL>
int launch_t(const PrefillSplitKernelParams &p, hipStream_t stream) {
    const size_t lds = Lds<D>::TOTAL;          // K[3] + V[3], padded rows
    dim3 grid(8u * p.base.bh_per_xcd * p.base.nq_tiles * p.num_splits), block(kThreads);
    static DynLdsAttr attr;
    if (const int rc = attr.ensure(reinterpret_cast<const void *>(&prefill_split_kernel<Tr, D, CAUSAL>), (int)lds,
                                   "prefill_split_kernel"))
        return rc;
    hipLaunchKernelGGL((prefill_split_kernel<Tr, D, CAUSAL>), grid, block, lds, stream, p);
    return check_launch("prefill_split_kernel");
}

template <class Tr, int D, bool CAUSAL>
int combine_t(const PrefillSplitKernelParams &p, hipStream_t stream) {
    constexpr int RPB = 256 / (D / 4);
    dim3 grid((unsigned)((p.base.Sq + RPB - 1) / RPB) * (unsigned)(p.base.B * p.base.Hq)), block(256);   // (checked by the caller)
    hipLaunchKernelGGL((prefill_split_combine_kernel<Tr, D, CAUSAL>), grid, block, 0, stream, p);
    return check_launch("prefill_split_combine_kernel");
}

template <class Tr, int D>
int dispatch_c(const PrefillSplitKernelParams &p, bool causal, bool combine, hipStream_t stream) {
    if (combine) return causal ? combine_t<Tr, D, true>(p, stream) : combine_t<Tr, D, false>(p, stream);
    return causal ? launch_t<Tr, D, true>(p, stream) : launch_t<Tr, D, false>(p, stream);
}

int dispatch(const PrefillSplitKernelParams &p, int dtype, int head_dim, bool causal, bool combine, hipStream_t stream) {
    const bool h = dtype == SFA_DTYPE_FP16;
    if (head_dim == 64) return h ? dispatch_c<Fp16, 64>(p, causal, combine, stream) : dispatch_c<Bf16, 64>(p, causal, combine, stream);
    return h ? dispatch_c<Fp16, 128>(p, causal, combine, stream) : dispatch_c<Bf16, 128>(p, causal, combine, stream);
}

}  // namespace

int launch_prefill_split(const PrefillSplitKernelParams &p, int dtype, int head_dim, bool causal, hipStream_t stream) {
    return dispatch(p, dtype, head_dim, causal, false, stream);
}

int launch_prefill_split_combine(const PrefillSplitKernelParams &p, int dtype, int head_dim, bool causal,
                                 hipStream_t stream) {
    return dispatch(p, dtype, head_dim, causal, true, stream);
}

}  // namespace sfa
