// Prefill forward over packed sequences with a split key range for gfx950 (MI355X): sfa_prefill_varlen_split_fwd with two
// or more splits.  bf16 / fp16, head_dim 64 / 128, causal (bottom-right aligned per sequence) or full, MHA or GQA, the
// packed layout of prefill_varlen_kernel.hip.
//
// After prefill_varlen_kernel.hip's plan kernel (launch_prefill_varlen_plan), three kernels on the same stream:
//   prefill_varlen_split_items_kernel    one workgroup: from the q-tile plan the compact list of (plan slot, split) work
//                                        items -- min(S, ceil(nkt / C)) per slot of a valid sequence, nkt the tiles the
//                                        q-tile's last row sees, in plan order with a slot's splits side by side --
//                                        padded with the empty marker (-1, 0) up to bound * S entries.  Every entry is
//                                        written on every call; an empty split never gets an item.
//   prefill_varlen_split_kernel          one workgroup per (item, query head): the tiles [s C, min((s + 1) C, nkt)) of
//                                        the q-tile's key range -- [s C, nkt) for the last split, so a sequence longer
//                                        than the host's max_seqlen_k is still computed in full -- into fp32 partials in
//                                        the workspace (prefill_split_kernel.hip's format).
//   prefill_varlen_split_combine_kernel  per (plan slot, query head, row): prefill_split_combine_kernel's merge over the
//                                        splits that are not empty for the q-tile, o and lse written in place.
// The front end is prefill_varlen_kernel.hip's (wave-uniform loads of the item and the sequence's four cu entries, leaving
// on the marker or an invalid sequence before any barrier, 64-bit base pointers), the walk prefill_stream.h's tile_stream
// without a lower bound over [ts0, wg_end), the epilogue prefill_split_kernel.hip's partial.  What is this unit's own:
//   * Both kernels re-derive the sequence's validity, Sq, Sk and nkt from the cu arrays: safe for any cu contents, and
//     for any plan or item contents (an index out of range is the marker).
//   * A sequence without keys, and a q-tile above the causal limit, have no items: the combine finds ns = 0 and writes
//     zeros and -inf from no partial at all.  Partials that no workgroup wrote are never read.
//   * A sequence's bits depend on its own rows and (C, S) only: the same walk per split and the same ordered merge as
//     prefill_split_kernel.hip on the sequence's own view wherever that call cuts at the same tiles.
// blockIdx -> (item, head) is prefill_varlen_kernel.hip's map with the item in the place of the plan slot: every working
// workgroup is launched before the first empty one, the splits of one (sequence, q-tile) are neighbours, and with
// Hq % 8 == 0 the heads of one kv head meet on one XCD's L2.
#include "prefill_stream.h"
#include "prefill_varlen_seq.h"

namespace sfa {

namespace {

using namespace prefill;

// ---- the front end: prefill_varlen_seq.h's varlen_item, with the plan slot given instead of read off blockIdx ----
// blockIdx -> (slow digit, query head h): the head slice on the fast digit (all of it workgroup-uniform).
__device__ __forceinline__ int varlen_block(const PrefillVarlenKernelParams &p, int &h) {
    const int hps = p.Hq / p.slices;            // query heads per slice
    const int rest = blockIdx.x / p.slices;
    h = (blockIdx.x % p.slices) * hps + rest % hps;
    return rest / hps;
}

// The work item of plan slot `slot` (< p.bound), all but its head.  False on the plan's empty marker and on a sequence that
// is not a range of the tensors.
__device__ __forceinline__ bool varlen_plan_item(const PrefillVarlenKernelParams &p, int slot, VarlenItem &it) {
    const int2 item = p.plan[slot];
    const int b = item.x;
    it.qt = item.y;
    if (b < 0 || b >= p.B) return false;        // the empty marker
    int cq1, ck1;
    if (!varlen_seq(p, b, it.cq0, cq1, it.ck0, ck1)) return false;
    it.Sq = cq1 - it.cq0, it.Sk = ck1 - it.ck0;
    return it.qt >= 0 && it.qt * kBM < it.Sq;   // (the plan kernel never writes an item that fails this)
}

// ---- prefill_split_kernel.hip's partition, partial and merge, on a sequence's own Sq and Sk.  This unit's own copies:
// moved to a shared header they changed that unit's device code (profiles/prefill_varlen_split_device_code.txt), and a
// sequence must get the same bits from both calls, so the arithmetic below is that unit's, statement for statement. ----
// tiles the last row of q-tile qt sees, for Sq query rows against Sk keys (the partition of include/star_flash_attn.h)
template <bool CAUSAL>
__device__ __forceinline__ int split_tiles_of_qtile(int Sq, int Sk, int qt) {
    const int nkt_max = (Sk + kBN - 1) / kBN;
    if (!CAUSAL) return nkt_max;
    const int lim = min(kBM * (qt + 1), Sq) - 1 + Sk - Sq;
    return lim < 0 ? 0 : lim / kBN + 1;
}

// The row's partial -- O un-normalised at prow (= partial row + 4 h2), (m, l) at *ml -- for the lanes of rows that exist.
// Each lane owns 4 consecutive floats of every 8-column group of O^T's accumulator layout, so the partial goes out as
// 16-byte stores with no lane exchange.
template <int D>
__device__ __forceinline__ void store_partial(const Acc<D, 1> &acc, float ltot, float *prow, float2 *ml, int h2) {
#pragma unroll
    for (int d = 0; d < StreamDims<D>::NDB; ++d)
#pragma unroll
        for (int g = 0; g < 4; ++g)         // this lane's columns 32 d + 8 g + 4 h2 .. + 3
            *reinterpret_cast<float4 *>(prow + 32 * d + 8 * g) =
                make_float4(acc.o[0][d][4 * g], acc.o[0][d][4 * g + 1], acc.o[0][d][4 * g + 2], acc.o[0][d][4 * g + 3]);
    if (h2 == 0) *ml = make_float2(acc.msc[0], ltot);
}

// The merge of one row's ns partials, 4 columns of it: m = max m_s, l = sum 2^(m_s - m) l_s, o = sum 2^(m_s - m) O_s / l in
// ascending s, lse = (m + log2 l) ln 2.  ml / po: the row's (m, l) and this thread's 4 columns in split 0; the next split
// is kBM rows on.  A partial with no key (l = 0) is skipped, never multiplied; none with a key: zeros and -inf.  lse_row
// may be null (and is for every thread but the row's first).
template <class Tr, int D>
__device__ __forceinline__ void merge_partials(const float2 *ml, const float *po, int ns, uint16_t *orow, float *lse_row) {
    float m = ninf();
    for (int s = 0; s < ns; ++s) {
        const float2 e = ml[(size_t)s * kBM];
        if (e.y > 0.f) m = fmaxf(m, e.x);
    }
    float l = 0.f;
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
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
    const float inv = l > 0.f ? 1.0f / l : 0.f;
    *reinterpret_cast<uint2 *>(orow) = make_uint2(Tr::pack2(o.x * inv, o.y * inv), Tr::pack2(o.z * inv, o.w * inv));
    if (lse_row) *lse_row = l > 0.f ? (m + __log2f(l)) * kLn2 : ninf();
}

// items[i] = (plan slot, split) for the i-th work item, (-1, 0) from the last item up to bound * S.  One workgroup walks
// the plan 256 slots at a time: split counts, an inclusive scan in LDS, then every thread writes its slot's items.  (The
// scan is 64 bit, as the plan kernel's; an item past the list's end is dropped, which valid contents never reach.)
template <bool CAUSAL>
__global__ void __launch_bounds__(256)
prefill_varlen_split_items_kernel(const PrefillVarlenSplitKernelParams sp) {
    __shared__ long long scan[256];
    __shared__ long long base_s;
    const PrefillVarlenKernelParams &p = sp.base;
    const int tid = threadIdx.x;
    const int S = sp.num_splits, C = sp.tiles_per_split;
    const long long cap = (long long)p.bound * S;
    if (tid == 0) base_s = 0;
    __syncthreads();
    for (int i0 = 0; i0 < p.bound; i0 += 256) {
        const int slot = i0 + tid;
        int cnt = 0;
        VarlenItem it;
        if (slot < p.bound && varlen_plan_item(p, slot, it))
            cnt = min(S, (split_tiles_of_qtile<CAUSAL>(it.Sq, it.Sk, it.qt) + C - 1) / C);
        scan[tid] = cnt;
        __syncthreads();
        for (int d = 1; d < 256; d <<= 1) {     // inclusive Hillis-Steele scan
            const long long add = tid >= d ? scan[tid - d] : 0;
            __syncthreads();
            scan[tid] += add;
            __syncthreads();
        }
        const long long first = base_s + scan[tid] - cnt;
        for (int s = 0; s < cnt && first + s < cap; ++s) sp.items[first + s] = make_int2(slot, s);
        __syncthreads();
        if (tid == 255) base_s = min(base_s + scan[255], cap);
        __syncthreads();
    }
    for (long long i = base_s + tid; i < cap; i += 256) sp.items[i] = make_int2(-1, 0);
}

template <class Tr, int D, bool CAUSAL>
__global__ void __launch_bounds__(kThreads, 2)
prefill_varlen_split_kernel(const PrefillVarlenSplitKernelParams sp) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const PrefillVarlenKernelParams &p = sp.base;

    VarlenItem it;
    const int2 item = sp.items[varlen_block(p, it.h)];
    const int slot = item.x, split = item.y, S = sp.num_splits;
    if (slot < 0 || slot >= p.bound || split < 0 || split >= S) return;    // the empty marker; before any barrier
    if (!varlen_plan_item(p, slot, it)) return;
    const int h = it.h, qt = it.qt, Sq = it.Sq, Sk = it.Sk;
    const int hk = h / (p.Hq / p.Hkv);

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);     // provably wave-uniform
    const int l31 = lane & 31, h2 = lane >> 5;
    const int coff = Sk - Sq;                   // causal: key j visible to row i iff j <= i + coff
    const int q0 = qt * kBM, wq0 = q0 + 32 * wave, qrow = wq0 + l31;

    // ---- the key range of this workgroup: tiles [ts0, wg_end), open-ended for the last split ----
    const int nkt = split_tiles_of_qtile<CAUSAL>(Sq, Sk, qt);
    TileStream ts{};
    ts.ts0 = split * sp.tiles_per_split;
    ts.wg_end = split == S - 1 ? nkt : min(ts.ts0 + sp.tiles_per_split, nkt);
    ts.nt = ts.wg_end - ts.ts0;                 // tiles the workgroup stages (workgroup-uniform)
    if (ts.nt <= 0) return;                     // an empty split (the items kernel lists none): nothing read or written
    const int wlast = min(wq0 + 31, Sq - 1);    // last query row of the wave
    ts.ntw = 0;                                 // end of the tiles this wave computes on, from ts0 (wave-uniform)
    if (wq0 < Sq) {
        if (!CAUSAL) ts.ntw = ts.nt;
        else if (wlast + coff >= 0) ts.ntw = max(0, min(ts.wg_end, (wlast + coff) / kBN + 1) - ts.ts0);
    }
    int lim[1];                                 // last visible key of this lane's row (< 0: none)
    lim[0] = CAUSAL ? min(qrow, Sq - 1) + coff : Sk - 1;
    const int wlim = CAUSAL ? wq0 + coff : Sk - 1;      // the smallest limit of the wave's rows
    // bit 0 set: the 32 keys starting at KBASE need masking for this wave's rows
    auto mask_bits = [&](int kbase) -> int { return kbase + 31 > wlim ? 1 : 0; };
    ts.k = p.k + (long long)it.ck0 * p.ks[0] + hk * p.ks[1];
    ts.v = p.v + (long long)it.ck0 * p.vs[0] + hk * p.vs[1];
    ts.k_stride = p.ks[0], ts.v_stride = p.vs[0];
    ts.Sk = Sk;

    // (the ragged last q-tile clamps to the sequence's own last row)
    const uint16_t *qp = p.q + ((long long)it.cq0 + min(qrow, Sq - 1)) * p.qs[0] + h * p.qs[1] + 8 * h2;
    Acc<D, 1> acc;
    tile_stream<Tr, D>(smem, ts, qp, acc, p.scale_log2, h2, lim, mask_bits, NoLowMask());

    // ---- epilogue: the row's partial -- O un-normalised, (m, l) -- to the workspace ----
    const float ltot = half_sum(acc.lsum[0]);
    if (qrow < Sq) {
        const size_t pidx = (((size_t)slot * p.Hq + h) * S + split) * kBM + (qrow - q0);
        store_partial<D>(acc, ltot, sp.part_o + pidx * D + 4 * h2, sp.part_ml + pidx, h2);
    }
}

// One thread per 4 columns of one query row, as prefill_split_combine_kernel; 256 / RPB blocks per (plan slot, head).
template <class Tr, int D, bool CAUSAL>
__global__ void __launch_bounds__(256)
prefill_varlen_split_combine_kernel(const PrefillVarlenSplitKernelParams sp) {
    constexpr int LPR = D / 4;                  // lanes per row
    constexpr int RPB = 256 / LPR;              // rows per block
    constexpr int BPT = kBM / RPB;              // blocks per q-tile
    const PrefillVarlenKernelParams &p = sp.base;
    const int rb = blockIdx.x % BPT, sh = blockIdx.x / BPT;
    const int h = sh % p.Hq, slot = sh / p.Hq;
    VarlenItem it;
    if (!varlen_plan_item(p, slot, it)) return;         // the empty marker, an invalid sequence
    const int r = rb * RPB + threadIdx.x / LPR, col = 4 * (threadIdx.x % LPR);
    const int row = it.qt * kBM + r;
    if (row >= it.Sq) return;
    const int C = sp.tiles_per_split, S = sp.num_splits;
    // the splits that are not empty for this q-tile: the others were never written and are not read
    const int ns = min(S, (split_tiles_of_qtile<CAUSAL>(it.Sq, it.Sk, it.qt) + C - 1) / C);
    const size_t pidx0 = (((size_t)slot * p.Hq + h) * S) * kBM + r;
    uint16_t *orow = p.o + ((long long)it.cq0 + row) * p.os[0] + h * p.os[1] + col;
    float *lse_row = p.lse && col == 0 ? p.lse + ((long long)h * p.total_q + it.cq0 + row) : nullptr;
    merge_partials<Tr, D>(sp.part_ml + pidx0, sp.part_o + pidx0 * D + col, ns, orow, lse_row);
}

template <class Tr, int D, bool CAUSAL>
int launch_t(const PrefillVarlenSplitKernelParams &p, hipStream_t stream) {
    const size_t lds = Lds<D>::TOTAL;          // K[3] + V[3], padded rows
    dim3 grid((unsigned)p.base.bound * (unsigned)p.num_splits * (unsigned)p.base.Hq), block(kThreads);  // (checked by the caller)
    static DynLdsAttr attr;
    if (const int rc = attr.ensure(reinterpret_cast<const void *>(&prefill_varlen_split_kernel<Tr, D, CAUSAL>), (int)lds,
                                   "prefill_varlen_split_kernel"))
        return rc;
    hipLaunchKernelGGL((prefill_varlen_split_kernel<Tr, D, CAUSAL>), grid, block, lds, stream, p);
    return check_launch("prefill_varlen_split_kernel");
}

template <class Tr, int D, bool CAUSAL>
int combine_t(const PrefillVarlenSplitKernelParams &p, hipStream_t stream) {
    constexpr int BPT = kBM / (256 / (D / 4));
    dim3 grid((unsigned)p.base.bound * (unsigned)p.base.Hq * (unsigned)BPT), block(256);    // (checked by the caller)
    hipLaunchKernelGGL((prefill_varlen_split_combine_kernel<Tr, D, CAUSAL>), grid, block, 0, stream, p);
    return check_launch("prefill_varlen_split_combine_kernel");
}

template <class Tr, int D>
int dispatch_c(const PrefillVarlenSplitKernelParams &p, bool causal, bool combine, hipStream_t stream) {
    if (combine) return causal ? combine_t<Tr, D, true>(p, stream) : combine_t<Tr, D, false>(p, stream);
    return causal ? launch_t<Tr, D, true>(p, stream) : launch_t<Tr, D, false>(p, stream);
}

int dispatch(const PrefillVarlenSplitKernelParams &p, int dtype, int head_dim, bool causal, bool combine, hipStream_t stream) {
    const bool h = dtype == SFA_DTYPE_FP16;
    if (head_dim == 64) return h ? dispatch_c<Fp16, 64>(p, causal, combine, stream) : dispatch_c<Bf16, 64>(p, causal, combine, stream);
    return h ? dispatch_c<Fp16, 128>(p, causal, combine, stream) : dispatch_c<Bf16, 128>(p, causal, combine, stream);
}

}  // namespace

int launch_prefill_varlen_split_items(const PrefillVarlenSplitKernelParams &p, bool causal, hipStream_t stream) {
    if (causal) hipLaunchKernelGGL(prefill_varlen_split_items_kernel<true>, dim3(1), dim3(256), 0, stream, p);
    else hipLaunchKernelGGL(prefill_varlen_split_items_kernel<false>, dim3(1), dim3(256), 0, stream, p);
    return check_launch("prefill_varlen_split_items_kernel");
}

int launch_prefill_varlen_split(const PrefillVarlenSplitKernelParams &p, int dtype, int head_dim, bool causal,
                                hipStream_t stream) {
    return dispatch(p, dtype, head_dim, causal, false, stream);
}

int launch_prefill_varlen_split_combine(const PrefillVarlenSplitKernelParams &p, int dtype, int head_dim, bool causal,
                                        hipStream_t stream) {
    return dispatch(p, dtype, head_dim, causal, true, stream);
}

}  // namespace sfa
