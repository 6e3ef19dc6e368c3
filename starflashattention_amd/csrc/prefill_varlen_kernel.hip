// Prefill forward over packed sequences of different lengths for gfx950 (MI355X): sfa_prefill_varlen_fwd.
// bf16 / fp16, head_dim 64 / 128, causal (bottom-right aligned per sequence) or full, MHA or GQA, q / o [total_q, Hq, D] and
// k / v [total_k, Hkv, D] with any token and head strides; sequence b owns the rows [cu_q[b], cu_q[b+1]) and
// [cu_k[b], cu_k[b+1]).
//
// Two kernels on one stream:
//   prefill_varlen_plan_kernel  one workgroup: from cu_seqlens_q / cu_seqlens_k the compact list of (sequence, q-tile)
//                               work items -- ceil(n_q / 256) per valid sequence with rows, a sequence's last q-tile
//                               first (the heaviest under the causal mask) -- padded with the empty marker (-1, 0) up to
//                               bound = total_q / 256 + B slots (every sequence with rows has ceil(n_q / 256) <=
//                               n_q / 256 + 1 q-tiles); items past the bound are dropped.  decode_varlen_geo.h's pattern:
//                               no host synchronisation, every slot written on every call.
//   prefill_varlen_kernel       one workgroup per (plan slot, query head): the whole key range [0, nkt(qt)) of the
//                               sequence for one q-tile, o and lse written in place.
// The tile pipeline is prefill_split_kernel.hip's walk of [ts0, wg_end) with ts0 = 0 (design notes: prefill_kernel.hip): a
// q-tile of 256 query rows, 8 waves of 32 rows, 64-key K/V tiles staged through registers into triple-buffered padded
// LDS images with one barrier per tile, and prefill_core.h's slot-ordered half-step h_block at exact scale (ORD 2, PF 2).
// The staging scaffold is a copy of that file's; the epilogue is prefill_window_kernel.hip's without the sink.  What
// differs:
//   * The workgroup reads its plan item and its sequence's four cu entries with wave-uniform loads, leaves on the marker
//     before any barrier, and re-derives the sequence's validity (0 <= cu[b] <= cu[b+1] <= total in both arrays): the
//     kernel is safe for any cu contents, and an invalid sequence is neither read nor written.
//   * Sq, Sk and the causal offset are the sequence's own; the base pointers are cu * token stride in 64 bits; the lse
//     row is h * total_q + cu_q[b] + row.
//   * Never read: the ragged last key tile clamps its rows to the sequence's own last key, the ragged last q-tile to its
//     own last row -- never into the next sequence's rows.  A stream position past the end re-reads the last tile.
//   * A sequence with no keys (or a q-tile whose rows all lie above the causal limit) stages nothing: the epilogue
//     writes zeros and lse = -inf from the empty accumulator.
// blockIdx -> (plan slot, head): the plan slot is the slow digit, so every real workgroup is launched before the first
// empty one (decode_varlen_kernel.hip measured why).  With Hq % 8 == 0, blockIdx & 7 selects a slice of Hq / 8 query
// heads (XCD x under round-robin dispatch; a speed hint only) and blockIdx >> 3 = slot * (Hq / 8) + head in slice: the
// q-tiles of one (sequence, kv head) meet on one XCD's L2.  Otherwise blockIdx = slot * Hq + head.
#include "prefill_core.h"

namespace sfa {

namespace {

using namespace prefill;

// The row ranges [q0, q1) and [k0, k1) of sequence b; false unless both are ranges inside [0, total).
__device__ __forceinline__ bool varlen_seq(const PrefillVarlenKernelParams &p, int b, int &q0, int &q1, int &k0, int &k1) {
    q0 = p.cu_q[b], q1 = p.cu_q[b + 1], k0 = p.cu_k[b], k1 = p.cu_k[b + 1];
    return q0 >= 0 && q0 <= q1 && q1 <= p.total_q && k0 >= 0 && k0 <= k1 && k1 <= p.total_k;
}

// plan[i] = (b, q_tile) for the i-th work item, (-1, 0) from the last item up to p.bound.  One workgroup walks the
// sequences 256 at a time: tile counts, an inclusive scan in LDS, then every thread writes its sequence's items.  (The
// scan is 64 bit: 256 sequences of garbage cu contents may each claim total_q / 256 + 1 tiles.)
__global__ void __launch_bounds__(256)
prefill_varlen_plan_kernel(const PrefillVarlenKernelParams p) {
    __shared__ long long scan[256];
    __shared__ int base_s;
    const int tid = threadIdx.x;
    if (tid == 0) base_s = 0;
    __syncthreads();
    for (int b0 = 0; b0 < p.B; b0 += 256) {
        const int b = b0 + tid;
        int tiles = 0;
        if (b < p.B) {
            int q0, q1, k0, k1;
            if (varlen_seq(p, b, q0, q1, k0, k1)) tiles = (q1 - q0 + kBM - 1) / kBM;
        }
        scan[tid] = tiles;
        __syncthreads();
        for (int d = 1; d < 256; d <<= 1) {     // inclusive Hillis-Steele scan
            const long long add = tid >= d ? scan[tid - d] : 0;
            __syncthreads();
            scan[tid] += add;
            __syncthreads();
        }
        const int base = base_s;
        const long long first = base + scan[tid] - tiles;
        for (int i = 0; i < tiles && first + i < p.bound; ++i) p.plan[first + i] = make_int2(b, tiles - 1 - i);
        __syncthreads();
        if (tid == 255) base_s = (int)min(base + scan[255], (long long)p.bound);
        __syncthreads();
    }
    for (int i = base_s + tid; i < p.bound; i += 256) p.plan[i] = make_int2(-1, 0);
}

template <class Tr, int D, bool CAUSAL>
__global__ void __launch_bounds__(kThreads, 2)
prefill_varlen_kernel(const PrefillVarlenKernelParams p) {
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
    const int coff = Sk - Sq;                   // causal: key j visible to row i iff j <= i + coff
    const int q0 = qt * kBM, wq0 = q0 + 32 * wave, qrow = wq0 + l31;

    // ---- the key range of this workgroup: tiles [0, wg_end), the whole range the q-tile's last row sees ----
    constexpr int ts0 = 0;
    const int n_kv_tiles = (Sk + kBN - 1) / kBN;
    int wg_end = n_kv_tiles;
    if (CAUSAL) {
        const int rlim = min(q0 + kBM, Sq) - 1 + coff;      // (<= Sk - 1)
        wg_end = rlim < 0 ? 0 : rlim / kBN + 1;
    }
    const int nt = wg_end;                      // tiles the workgroup stages (workgroup-uniform); 0: no visible key
    const int wlast = min(wq0 + 31, Sq - 1);    // last query row of the wave
    int ntw = 0;                                // end of the tiles this wave computes on (wave-uniform)
    if (wq0 < Sq) {
        if (!CAUSAL) ntw = nt;
        else if (wlast + coff >= 0) ntw = min(wg_end, (wlast + coff) / kBN + 1);
    }
    int lim[NQB];                               // last visible key of this lane's row (< 0: none)
    lim[0] = CAUSAL ? min(qrow, Sq - 1) + coff : Sk - 1;
    const int wlim = CAUSAL ? wq0 + coff : Sk - 1;      // the smallest limit of the wave's rows
    // bit 0 set: the 32 keys starting at KBASE need masking for this wave's rows
    auto mask_bits = [&](int kbase) -> int { return kbase + 31 > wlim ? 1 : 0; };

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
    // rows to the sequence's last key: nothing past it -- the next sequence's first rows -- is read.
    const int ragged_tile = (Sk % kBN) ? n_kv_tiles - 1 : -1;
    const int last0 = Sk - 1 - (n_kv_tiles - 1) * kBN;      // last valid row of the last tile
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

    // ---- epilogue: normalise, convert, store O[row][:] and lse; a row with no visible key gets zeros and -inf ----
    const float ltot = half_sum(acc.lsum[0]);
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

template <class Tr, int D, bool CAUSAL>
int launch_t(const PrefillVarlenKernelParams &p, hipStream_t stream) {
    const size_t lds = Lds<D>::TOTAL;          // K[3] + V[3], padded rows
    dim3 grid((unsigned)p.bound * (unsigned)p.Hq), block(kThreads);     // (checked by the caller)
    static DynLdsAttr attr;
    if (const int rc = attr.ensure(reinterpret_cast<const void *>(&prefill_varlen_kernel<Tr, D, CAUSAL>), (int)lds,
                                   "prefill_varlen_kernel"))
        return rc;
    hipLaunchKernelGGL((prefill_varlen_kernel<Tr, D, CAUSAL>), grid, block, lds, stream, p);
    return check_launch("prefill_varlen_kernel");
}

template <class Tr, int D>
int launch_c(const PrefillVarlenKernelParams &p, bool causal, hipStream_t stream) {
    return causal ? launch_t<Tr, D, true>(p, stream) : launch_t<Tr, D, false>(p, stream);
}

}  // namespace

int launch_prefill_varlen(const PrefillVarlenKernelParams &p, int dtype, int head_dim, bool causal, hipStream_t stream) {
    hipLaunchKernelGGL(prefill_varlen_plan_kernel, dim3(1), dim3(256), 0, stream, p);
    if (const int rc = check_launch("prefill_varlen_plan_kernel")) return rc;
    const bool h = dtype == SFA_DTYPE_FP16;
    if (head_dim == 64) return h ? launch_c<Fp16, 64>(p, causal, stream) : launch_c<Bf16, 64>(p, causal, stream);
    return h ? launch_c<Fp16, 128>(p, causal, stream) : launch_c<Bf16, 128>(p, causal, stream);
}

}  // namespace sfa
