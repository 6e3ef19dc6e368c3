// Prefill forward over packed sequences of different lengths with a sliding window and an optional attention sink for
// gfx950 (MI355X): sfa_prefill_varlen_window_fwd.
// bf16 / fp16, head_dim 64 / 128, causal (bottom-right aligned per sequence), MHA or GQA, q / o [total_q, Hq, D] and
// k / v [total_k, Hkv, D] with any token and head strides; sequence b owns the rows [cu_q[b], cu_q[b+1]) and
// [cu_k[b], cu_k[b+1]).
//
// Two kernels on one stream: prefill_varlen_kernel.hip's plan kernel (launch_prefill_varlen_plan), then
// prefill_varlen_window_kernel, one workgroup per (plan slot, query head).  The attention kernel is
// prefill_varlen_kernel's work-item front end (varlen_item of prefill_varlen_seq.h) joined to prefill_window_kernel's key
// range; the tile pipeline is prefill_stream.h's tile_stream with a lower bound, the epilogue that header's fold_sink and
// store_row (design notes there, in those two files and in prefill_kernel.hip).
//   * As prefill_varlen_kernel: the plan slot and head from blockIdx, the four wave-uniform cu loads, leaving on the
//     marker or on an invalid sequence before any barrier (safe for any cu contents: an invalid sequence is neither read
//     nor written), 64-bit base pointers cu * token stride, the lse row h * total_q + cu_q[b] + row.
//   * As prefill_window_kernel: the tiles [ts0, wg_end) of the q-tile, the wave's own [tw0, ntw) with leading and
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
#include "prefill_stream.h"
#include "prefill_varlen_seq.h"

namespace sfa {

namespace {

using namespace prefill;

template <class Tr, int D, bool SINK>
__global__ void __launch_bounds__(kThreads, 2)
prefill_varlen_window_kernel(const PrefillVarlenWindowKernelParams wp) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const PrefillVarlenKernelParams &p = wp.base;

    VarlenItem it;
    if (!varlen_item(p, it)) return;            // before any barrier
    const int h = it.h, qt = it.qt, Sq = it.Sq, Sk = it.Sk;
    const int hk = h / (p.Hq / p.Hkv);

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);     // provably wave-uniform
    const int l31 = lane & 31, h2 = lane >> 5;
    const int coff = Sk - Sq;                   // key j visible to row i iff lo_i <= j <= i + coff (may be negative)
    const int q0 = qt * kBM, wq0 = q0 + 32 * wave, qrow = wq0 + l31;

    // ---- the key range of this workgroup: tiles [ts0, wg_end) of the sequence ----
    // 1 <= win <= max(Sk, 1): a window longer than the sequence is the causal mask (lo = 0 for every row).  Every limit is
    // a row of the sequence plus coff, in (-total_q, total_k): limit >= win >= 1 keeps limit + 1 - win in [1, limit].
    TileStream ts{};
    const int win = min(wp.window, max(Sk, 1));
    auto low_of = [&](int limit) -> int { return limit < win ? 0 : limit + 1 - win; };
    const int lo0 = low_of(coff);               // no row sees a key below the first row's lower bound
    ts.tlo = lo0 / kBN;
    ts.first0 = lo0 - ts.tlo * kBN;             // first valid row of the first tile
    const int rlast = min(q0 + kBM, Sq) - 1;    // last query row of the q-tile
    ts.ts0 = low_of(q0 + coff) / kBN;
    ts.wg_end = rlast + coff >= 0 ? (rlast + coff) / kBN + 1 : 0;       // (lim <= Sk - 1 for every row)
    ts.nt = max(0, ts.wg_end - ts.ts0);         // tiles the workgroup stages (workgroup-uniform); 0: no visible key
    const int wlast = min(wq0 + 31, Sq - 1);    // last query row of the wave
    ts.ntw = 0;                                 // end of the tiles this wave computes on, from ts0 (wave-uniform)
    if (wq0 < Sq && wlast + coff >= 0) ts.ntw = max(0, min(ts.wg_end, (wlast + coff) / kBN + 1) - ts.ts0);
    int lim[1];                                 // last visible key of this lane's row (< 0: none)
    lim[0] = min(qrow, Sq - 1) + coff;
    const int wlim = wq0 + coff;                // the smallest limit of the wave's rows
    // this lane's lower bound, the largest one of the wave's rows, and the leading tiles of the workgroup that lie wholly
    // below the smallest one
    const int lo_r = low_of(lim[0]);
    const int wlo = low_of(wlast + coff);
    ts.tw0 = min(max(0, low_of(wlim) / kBN - ts.ts0), ts.ntw);
    // bit 0 set: the 32 keys starting at KBASE need masking for this wave's rows
    auto mask_bits = [&](int kbase) -> int { return (kbase + 31 > wlim || kbase < wlo) ? 1 : 0; };
    auto low_mask = [&](f32x16 &s, int kbase, int) {
        if (kbase < wlo) mask_below(s, kbase, h2, lo_r);
    };
    ts.k = p.k + (long long)it.ck0 * p.ks[0] + hk * p.ks[1];
    ts.v = p.v + (long long)it.ck0 * p.vs[0] + hk * p.vs[1];
    ts.k_stride = p.ks[0], ts.v_stride = p.vs[0];
    ts.Sk = Sk;

    // (the ragged last q-tile clamps to the sequence's own last row)
    const uint16_t *qp = p.q + ((long long)it.cq0 + min(qrow, Sq - 1)) * p.qs[0] + h * p.qs[1] + 8 * h2;
    Acc<D, 1> acc;
    tile_stream<Tr, D>(smem, ts, qp, acc, p.scale_log2, h2, lim, mask_bits, low_mask);

    // ---- epilogue: fold the sink, normalise, convert, store O[row][:] and lse; a row with no visible key gets zeros
    // and -inf ----
    float ltot = half_sum(acc.lsum[0]);
    if constexpr (SINK) fold_sink(acc, ltot, wp.sinks[h]);
    if (qrow < Sq)
        store_row<Tr, D>(acc, ltot, p.o + ((long long)it.cq0 + qrow) * p.os[0] + h * p.os[1], p.lse,
                         (long long)h * p.total_q + it.cq0 + qrow, h2);
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
