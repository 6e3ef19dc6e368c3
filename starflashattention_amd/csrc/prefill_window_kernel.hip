// Prefill forward with a sliding window and an optional attention sink for gfx950 (MI355X): sfa_prefill_window_fwd.
// bf16 / fp16, head_dim 64 / 128, causal (bottom-right aligned), MHA or GQA, [B, H, S, D] tensors with any strides.
//
// The tile pipeline is prefill_kernel.hip's (design notes there): a q-tile of 256 query rows of one (batch, head), 8
// waves of 32 rows, 64-key K/V tiles staged through registers into triple-buffered padded LDS images with one barrier
// per tile, and prefill_core.h's slot-ordered half-step h_block at exact scale (ORD 2).  What differs:
//   * The key range.  Row i with causal limit lim_i = i + (Sk - Sq) sees the keys [lo_i, lim_i], lo_i = max(0, lim_i + 1 -
//     window).  A workgroup walks only the tiles [lo(first row) / 64, lim(last row) / 64] of its q-tile, and a wave
//     computes only on the tiles between its first row's lo and its last row's lim: during the workgroup's other tiles
//     it only stages (leading and trailing idle steps, as in chunk_attn_kernel of decode_chunk_body.h).
//   * The masks.  The causal mask and the window's lower mask run only on the 32-key halves that need them: mask_bits
//     flags a half that reaches past the wave's smallest limit or below its largest lower bound, and h_block's LowMask
//     hook applies the lower bound next to mask_half.
//   * Never read: no row sees a key below lo_0, the lower bound of query row 0.  The staged rows of the tile that holds
//     lo_0 are clamped to max(row, lo_0) -- a masked key has weight 0, but 0 * NaN is NaN in P.V -- and no workgroup
//     starts below that tile.
//   * One q-tile per workgroup, no balanced pairs: once the window is shorter than the causal limit every q-tile walks
//     the same number of tiles (window / 64 + 4 or 5), so there is no imbalance for a pair to even out.
//   * The sink (template SINK): one more softmax element per row -- logit sinks[h], value row 0 -- folded into the row's
//     state once, in the epilogue, with chunk_attn_kernel's fold.  A row with no visible key stays empty (zeros, lse =
//     -inf).  Without the flag none of it is compiled.
// blockIdx -> (head, q-tile) is block_coord's XCD-aware order (prefill_common.h).
#include "prefill_core.h"

namespace sfa {

namespace {

using namespace prefill;

// The window's lower mask of a half-tile of fresh scores (mask_half's register layout): keys below lo get -inf
__device__ __forceinline__ void mask_below(f32x16 &s, int kbase, int h2, int lo) {
#pragma unroll
    for (int r = 0; r < 16; ++r)
        if (kbase + (r & 3) + 8 * (r >> 2) + 4 * h2 < lo) s[r] = ninf();
}

template <class Tr, int D, bool SINK>
__global__ void __launch_bounds__(kThreads, 2)
prefill_window_kernel(const PrefillWindowKernelParams wp) {
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
    const PrefillKernelParams &p = wp.base;

    const BlockCoord bc = block_coord(p);       // p.nq_tiles = q-tiles per head
    if (bc.bh >= p.B * p.Hq) return;
    const int qt = bc.qt;
    const int b = bc.bh / p.Hq, h = bc.bh % p.Hq;
    const int hk = h / (p.Hq / p.Hkv);

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);     // provably wave-uniform
    const int l31 = lane & 31, h2 = lane >> 5;
    const int coff = p.Sk - p.Sq;               // key j visible to row i iff lo_i <= j <= i + coff
    const int q0 = qt * kBM, wq0 = q0 + 32 * wave, qrow = wq0 + l31;

    // ---- the key range of this workgroup: tiles [ts0, wg_end) ----
    const int win = wp.window;                  // 1 <= win <= Sk (the host clamps: a longer window is the causal mask)
    auto low_of = [&](int limit) -> int { return max(0, limit + 1 - win); };
    const int lo0 = low_of(coff);               // no row sees a key below the first row's lower bound
    const int tlo = lo0 / kBN;
    const int rlast = min(q0 + kBM, p.Sq) - 1;  // last query row of the q-tile
    const int ts0 = low_of(q0 + coff) / kBN;
    const int wg_end = rlast + coff >= 0 ? (rlast + coff) / kBN + 1 : 0;    // (lim <= Sk - 1 for every row)
    const int nt = max(0, wg_end - ts0);        // tiles the workgroup stages (workgroup-uniform)
    const int wlast = min(wq0 + 31, p.Sq - 1);  // last query row of the wave
    int ntw = 0;                                // end of the tiles this wave computes on, from ts0 (wave-uniform)
    if (wq0 < p.Sq && wlast + coff >= 0) ntw = max(0, min(wg_end, (wlast + coff) / kBN + 1) - ts0);
    int lim[NQB];                               // last visible key of this lane's row (< 0: none)
    lim[0] = min(qrow, p.Sq - 1) + coff;
    const int wlim = wq0 + coff;                // the smallest limit of the wave's rows
    // this lane's lower bound, the largest one of the wave's rows, and the leading tiles of the workgroup that lie wholly
    // below the smallest one
    const int lo_r = low_of(lim[0]);
    const int wlo = low_of(wlast + coff);
    const int tw0 = min(max(0, low_of(wlim) / kBN - ts0), ntw);
    // bit 0 set: the 32 keys starting at KBASE need masking for this wave's rows
    auto mask_bits = [&](int kbase) -> int { return (kbase + 31 > wlim || kbase < wlo) ? 1 : 0; };
    auto low_mask = [&](f32x16 &s, int kbase, int) {
        if (kbase < wlo) mask_below(s, kbase, h2, lo_r);
    };

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
    // rows to the last valid one, the tile that holds lo0 to the first valid one: nothing below lo0 or past Sk is read.
    const int n_kv_tiles = (p.Sk + kBN - 1) / kBN;
    const int ragged_tile = (p.Sk % kBN) ? n_kv_tiles - 1 : -1;
    const int last0 = p.Sk - 1 - (n_kv_tiles - 1) * kBN;    // last valid row of the last tile
    const int first0 = lo0 - tlo * kBN;                     // first valid row of the first tile
    const int row0_ = st_row, row1_ = st_row + ROWSTEP;
    const unsigned ch_off = 16u * st_ch;
    constexpr int NOPS = 2 * NLD;   // op n: even = K chunk n/2, odd = V chunk n/2
    // where the K and V tiles of two stream positions live and which of their rows exist: once per step, scalar
    struct TileSrc { const char *k, *v; int fk, lk, fv, lv; };
    auto tile_of = [&](int pos) -> int { return min(ts0 + pos, wg_end - 1); };     // past the end: re-read the last tile
    auto tile_src = [&](int pos_k, int pos_v) -> TileSrc {
        const int tk = tile_of(pos_k), tv = tile_of(pos_v);
        return TileSrc{kg + tk * k_tile_bytes, vg + tv * v_tile_bytes,
                       tk == tlo ? first0 : 0, tk == ragged_tile ? last0 : kBN - 1,
                       tv == tlo ? first0 : 0, tv == ragged_tile ? last0 : kBN - 1};
    };
    auto row_off = [&](int row, int first, int last, unsigned rowb) -> unsigned {
        return (unsigned)min(max(row, first), last) * rowb + ch_off;
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

    if (nt > 0) {
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
        // ---- leading idle steps: tiles below every row of this wave ----
        for (; t < tw0; ++t) {
            SFA_STAGE_AND_SYNC(t);
            SFA_ADVANCE();
        }
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
                                                           mask_bits(kbase), kbase, h2, lim, kpre, NoHook(), st_hook, low_mask);
            __syncthreads();
            const TileSrc ts = tile_src(t + 3, t + 2);
            auto ld_hook = [&](int i) {         // NOPS loads spread evenly over QK slots 1..NKS-1
#pragma unroll
                for (int n = (i - 1) * NOPS / (NKS - 1); n < i * NOPS / (NKS - 1); ++n) load_op(n, ts);
            };
            h_block<Tr, D, NQB, PF, ORD, 0, 1, true, true>(kb1, vb, kb1, qf, sA, sB, acc, c2, mxB, mxA,
                                                           mask_bits(kbase + 32), kbase + 32, h2, lim, kpre, ld_hook, NoHook(), low_mask);
            SFA_ADVANCE();
        }
        // ---- TAIL step: this wave's last tile (its second half computes no new scores) ----
        if (t < ntw) {
            const char *kb = k_rd + kcur, *vb = v_rd + vcur;
            const int kbase = (ts0 + t) * kBN;
            h_block<Tr, D, NQB, PF, ORD, 1, 0, true, false>(kb, vb, kb, qf, sB, sA, acc, c2, mxA, mxB,
                                                            mask_bits(kbase), kbase, h2, lim, kpre, NoHook(), NoHook(), low_mask);
            SFA_STAGE_AND_SYNC(t);
            h_block<Tr, D, NQB, PF, ORD, 0, 1, false, false>(kb, vb, kb, qf, sA, sB, acc, c2, mxB, mxA,
                                                             mask_bits(kbase + 32), kbase + 32, h2, lim, kpre, NoHook(), NoHook(),
                                                             low_mask);
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

    // ---- epilogue: fold the sink, normalise, convert, store O[row][:] and lse ----
    float ltot = half_sum(acc.lsum[0]);
    // SINK: one more stream element of the row -- max sinks[h] log2(e), sum 1, accumulator 0 -- folded in once.  A row
    // with no visible key (ltot == 0) stays empty: the sink joins only a softmax that has a key.
    if constexpr (SINK) {
        // (laundered: contracted into `sk - ms` below as one fma, the product's rounding error would stand where 0
        // belongs when the sink is the max)
        float sk = wp.sinks[h] * 1.4426950408889634f;
        asm volatile("" : "+v"(sk));
        const bool has = ltot > 0.f;
        const float mn = fmaxf(acc.msc[0], sk);
        const float ms = (mn == ninf()) ? 0.f : mn;
        const float a1 = fast_exp2(acc.msc[0] - ms);
#pragma unroll
        for (int d = 0; d < NDB; ++d)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc.o[0][d][r] *= a1;
        ltot = has ? __builtin_fmaf(ltot, a1, fast_exp2(sk - ms)) : 0.f;
        acc.msc[0] = has ? mn : acc.msc[0];
    }
    const float inv = ltot > 0.f ? 1.0f / ltot : 0.f;
    if (qrow < p.Sq) {
        uint16_t *orow = p.o + b * p.os[0] + h * p.os[1] + (long long)qrow * p.os[2];
        store_o_row<Tr, D>(orow, acc.o[0], inv, h2);
        if (p.lse && h2 == 0) {
            const float lse = ltot > 0.f ? (acc.msc[0] + __log2f(ltot)) * kLn2 : ninf();
            p.lse[((long long)b * p.Hq + h) * p.Sq + qrow] = lse;
        }
    }
}

template <class Tr, int D, bool SINK>
int launch_t(const PrefillWindowKernelParams &p, hipStream_t stream) {
    const size_t lds = Lds<D>::TOTAL;          // K[3] + V[3], padded rows
    dim3 grid(8u * p.base.bh_per_xcd * p.base.nq_tiles), block(kThreads);
    static DynLdsAttr attr;
    if (const int rc = attr.ensure(reinterpret_cast<const void *>(&prefill_window_kernel<Tr, D, SINK>), (int)lds,
                                   "prefill_window_kernel"))
        return rc;
    hipLaunchKernelGGL((prefill_window_kernel<Tr, D, SINK>), grid, block, lds, stream, p);
    return check_launch("prefill_window_kernel");
}

template <class Tr, int D>
int launch_d(const PrefillWindowKernelParams &p, hipStream_t stream) {
    return p.sinks ? launch_t<Tr, D, true>(p, stream) : launch_t<Tr, D, false>(p, stream);
}

}  // namespace

int launch_prefill_window(const PrefillWindowKernelParams &p, int dtype, int head_dim, hipStream_t stream) {
    const bool h = dtype == SFA_DTYPE_FP16;
    if (head_dim == 64) return h ? launch_d<Fp16, 64>(p, stream) : launch_d<Bf16, 64>(p, stream);
    return h ? launch_d<Fp16, 128>(p, stream) : launch_d<Bf16, 128>(p, stream);
}

}  // namespace sfa
