// Prefill forward over packed sequences of different lengths with a sliding window and an optional attention sink for
// gfx950 (MI355X): sfa_prefill_varlen_window_fwd.
// bf16 / fp16, head_dim 64 / 128, causal (bottom-right aligned per sequence), MHA or GQA, q / o [total_q, Hq, D] and
// k / v [total_k, Hkv, D] with any token and head strides; sequence b owns the rows [cu_q[b], cu_q[b+1]) and
// [cu_k[b], cu_k[b+1]).
//
// Two kernels on one stream: prefill_varlen_kernel.hip's plan kernel (launch_prefill_varlen_plan), then
// prefill_varlen_window_kernel, one workgroup per (plan slot, query head).  The attention kernel is
// prefill_varlen_kernel's work-item front end joined to prefill_window_kernel's walk and epilogue (design notes in those
// two files and in prefill_kernel.hip); the staging scaffold is a copy of theirs.
//   * From prefill_varlen_kernel: the plan slot and head from blockIdx, the four wave-uniform cu loads, leaving on the
//     marker or on an invalid sequence before any barrier (safe for any cu contents: an invalid sequence is neither read
//     nor written), 64-bit base pointers cu * token stride, the lse row h * total_q + cu_q[b] + row.
//   * From prefill_window_kernel: the tiles [ts0, wg_end) of the q-tile, the wave's own [tw0, ntw) with leading and
//     trailing idle steps, mask_bits with the wave's largest lower bound, the LowMask hook, the first-tile and last-tile
//     clamps through one min(max(row, first), last), and the sink folded once in the epilogue into rows that have a key.
//   * Every quantity is the sequence's own: Sq = n_q, Sk = n_k, coff = n_k - n_q (negative when n_q > n_k: the rows with
//     lim < 0 have no key, and a q-tile of such rows stages nothing and writes zeros and -inf from the empty accumulator,
//     sink or not), lo_0 = max(0, n_k - n_q + 1 - window) relative to the sequence's first key.  The walk is the
//     rectangular kernel's step for step, so a sequence's rows carry that kernel's bits.
//   * Never read: K and V rows of the sequence below lo_0 (the tile that holds lo_0 clamps its rows up to it; it may be
//     the ragged last tile too, n_k = 65 with lo_0 = 64: both clamps apply), rows past the sequence's last key or last
//     query row, and everything of another sequence.
// blockIdx -> (plan slot, head) is prefill_varlen_kernel.hip's map.
#include "prefill_core.h"
#include "prefill_varlen_seq.h"

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
prefill_varlen_window_kernel(const PrefillVarlenWindowKernelParams wp) {
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
    const PrefillVarlenKernelParams &p = wp.base;

    // ---- the work item: plan slot on the slow digit, the head slice on the fast one (all of it workgroup-uniform) ----
    const int hps = p.Hq / p.slices;            // query heads per slice
    const int rest = blockIdx.x / p.slices;
    const int h = (blockIdx.x % p.slices) * hps + rest % hps;
    const int2 item = p.plan[rest / hps];
    const int b = item.x, qt = item.y;
    if (b < 0 || b >= p.B) return;              // the empty marker: before any barrier
    int cq0, cq1, ck0, ck1;
    if (!varlen_seq(p, b, cq0, cq1, ck0, ck1)) return;      // not a range of the tensors: nothing read, nothing written
    const int Sq = cq1 - cq0, Sk = ck1 - ck0;
    if (qt < 0 || qt * kBM >= Sq) return;       // (the plan kernel never writes such an item)
    const int hk = h / (p.Hq / p.Hkv);

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);     // provably wave-uniform
    const int l31 = lane & 31, h2 = lane >> 5;
    const int coff = Sk - Sq;                   // key j visible to row i iff lo_i <= j <= i + coff (may be negative)
    const int q0 = qt * kBM, wq0 = q0 + 32 * wave, qrow = wq0 + l31;

    // ---- the key range of this workgroup: tiles [ts0, wg_end) of the sequence ----
    // 1 <= win <= max(Sk, 1): a window longer than the sequence is the causal mask (lo = 0 for every row).  Every limit is
    // a row of the sequence plus coff, in (-total_q, total_k): limit >= win >= 1 keeps limit + 1 - win in [1, limit].
    const int win = min(wp.window, max(Sk, 1));
    auto low_of = [&](int limit) -> int { return limit < win ? 0 : limit + 1 - win; };
    const int lo0 = low_of(coff);               // no row sees a key below the first row's lower bound
    const int tlo = lo0 / kBN;
    const int rlast = min(q0 + kBM, Sq) - 1;    // last query row of the q-tile
    const int ts0 = low_of(q0 + coff) / kBN;
    const int wg_end = rlast + coff >= 0 ? (rlast + coff) / kBN + 1 : 0;    // (lim <= Sk - 1 for every row)
    const int nt = max(0, wg_end - ts0);        // tiles the workgroup stages (workgroup-uniform); 0: no visible key
    const int wlast = min(wq0 + 31, Sq - 1);    // last query row of the wave
    int ntw = 0;                                // end of the tiles this wave computes on, from ts0 (wave-uniform)
    if (wq0 < Sq && wlast + coff >= 0) ntw = max(0, min(wg_end, (wlast + coff) / kBN + 1) - ts0);
    int lim[NQB];                               // last visible key of this lane's row (< 0: none)
    lim[0] = min(qrow, Sq - 1) + coff;
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
    const char *const kg = reinterpret_cast<const char *>(p.k + (long long)ck0 * p.ks[0] + hk * p.ks[1]);  // uniform
    const char *const vg = reinterpret_cast<const char *>(p.v + (long long)ck0 * p.vs[0] + hk * p.vs[1]);
    const long long k_tile_bytes = 2ll * kBN * p.ks[0], v_tile_bytes = 2ll * kBN * p.vs[0];
    const unsigned k_rowb = (unsigned)(2 * p.ks[0]), v_rowb = (unsigned)(2 * p.vs[0]);
    char *const k_w = smem + L::KS * st_row + 16 * st_ch;
    char *const v_w = smem + L::V_BASE + L::VS * st_row + 16 * st_ch;
    uint4 kr0, kr1, vr0, vr1;       // plain scalars: arrays of these ended up in scratch (prefill_kernel.hip)
    kr0 = kr1 = vr0 = vr1 = make_uint4(0, 0, 0, 0);

    // Rows of a tile: row r is at r * row bytes from the tile's base.  The ragged last tile (Sk % 64 != 0) clamps its
    // rows to the sequence's last key, the tile that holds lo0 to the first valid one: nothing below lo0 and nothing past
    // the sequence's last key -- the next sequence's first rows -- is read.  (One tile may be both.)
    const int n_kv_tiles = (Sk + kBN - 1) / kBN;
    const int ragged_tile = (Sk % kBN) ? n_kv_tiles - 1 : -1;
    const int last0 = Sk - 1 - (n_kv_tiles - 1) * kBN;      // last valid row of the last tile
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

    // ---- Q^T fragments (B operand): lane holds Q[row][16ks + 8*h2 .. +8]; the ragged last q-tile clamps to the
    // sequence's own last row ----
    Vec qf[NQB][NKS];
    {
        const uint16_t *qp = p.q + ((long long)cq0 + min(qrow, Sq - 1)) * p.qs[0] + h * p.qs[1] + 8 * h2;
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

    // ---- epilogue: fold the sink, normalise, convert, store O[row][:] and lse; a row with no visible key gets zeros
    // and -inf ----
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
    if (qrow < Sq) {
        uint16_t *orow = p.o + ((long long)cq0 + qrow) * p.os[0] + h * p.os[1];
        store_o_row<Tr, D>(orow, acc.o[0], inv, h2);
        if (p.lse && h2 == 0) {
            const float lse = ltot > 0.f ? (acc.msc[0] + __log2f(ltot)) * kLn2 : ninf();
            p.lse[(long long)h * p.total_q + cq0 + qrow] = lse;
        }
    }
}

template <class Tr, int D, bool SINK>
int launch_t(const PrefillVarlenWindowKernelParams &p, hipStream_t stream) {
    const size_t lds = Lds<D>::TOTAL;          // K[3] + V[3], padded rows
    dim3 grid((unsigned)p.base.bound * (unsigned)p.base.Hq), block(kThreads);     // (checked by the caller)
    static DynLdsAttr attr;
    if (const int rc = attr.ensure(reinterpret_cast<const void *>(&prefill_varlen_window_kernel<Tr, D, SINK>), (int)lds,
                                   "prefill_varlen_window_kernel"))
        return rc;
    hipLaunchKernelGGL((prefill_varlen_window_kernel<Tr, D, SINK>), grid, block, lds, stream, p);
    return check_launch("prefill_varlen_window_kernel");
}

template <class Tr, int D>
int launch_d(const PrefillVarlenWindowKernelParams &p, hipStream_t stream) {
    return p.sinks ? launch_t<Tr, D, true>(p, stream) : launch_t<Tr, D, false>(p, stream);
}

}  // namespace

int launch_prefill_varlen_window(const PrefillVarlenWindowKernelParams &p, int dtype, int head_dim, hipStream_t stream) {
    if (const int rc = launch_prefill_varlen_plan(p.base, stream)) return rc;
    const bool h = dtype == SFA_DTYPE_FP16;
    if (head_dim == 64) return h ? launch_d<Fp16, 64>(p, stream) : launch_d<Bf16, 64>(p, stream);
    return h ? launch_d<Fp16, 128>(p, stream) : launch_d<Bf16, 128>(p, stream);
}

}  // namespace sfa
