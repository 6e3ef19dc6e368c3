// Prefill forward with a sliding window and an optional attention sink for gfx950 (MI355X): sfa_prefill_window_fwd.
// bf16 / fp16, head_dim 64 / 128, causal (bottom-right aligned), MHA or GQA, [B, H, S, D] tensors with any strides.
//
// The tile pipeline is prefill_stream.h's tile_stream with a lower bound (design notes there and in prefill_kernel.hip).
// What is this kernel's own:
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
//     state once, in the epilogue, with chunk_attn_kernel's fold (fold_sink).  A row with no visible key stays empty
//     (zeros, lse = -inf).  Without the flag none of it is compiled.
// blockIdx -> (head, q-tile) is block_coord's XCD-aware order (prefill_common.h).
#include "prefill_stream.h"

namespace sfa {

namespace {

using namespace prefill;

template <class Tr, int D, bool SINK>
__global__ void __launch_bounds__(kThreads, 2)
prefill_window_kernel(const PrefillWindowKernelParams wp) {
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
    TileStream ts{};
    const int win = wp.window;                  // 1 <= win <= Sk (the host clamps: a longer window is the causal mask)
    auto low_of = [&](int limit) -> int { return max(0, limit + 1 - win); };
    const int lo0 = low_of(coff);               // no row sees a key below the first row's lower bound
    ts.tlo = lo0 / kBN;
    ts.first0 = lo0 - ts.tlo * kBN;             // first valid row of the first tile
    const int rlast = min(q0 + kBM, p.Sq) - 1;  // last query row of the q-tile
    ts.ts0 = low_of(q0 + coff) / kBN;
    ts.wg_end = rlast + coff >= 0 ? (rlast + coff) / kBN + 1 : 0;       // (lim <= Sk - 1 for every row)
    ts.nt = max(0, ts.wg_end - ts.ts0);         // tiles the workgroup stages (workgroup-uniform)
    const int wlast = min(wq0 + 31, p.Sq - 1);  // last query row of the wave
    ts.ntw = 0;                                 // end of the tiles this wave computes on, from ts0 (wave-uniform)
    if (wq0 < p.Sq && wlast + coff >= 0) ts.ntw = max(0, min(ts.wg_end, (wlast + coff) / kBN + 1) - ts.ts0);
    int lim[1];                                 // last visible key of this lane's row (< 0: none)
    lim[0] = min(qrow, p.Sq - 1) + coff;
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
    ts.k = p.k + b * p.ks[0] + hk * p.ks[1];
    ts.v = p.v + b * p.vs[0] + hk * p.vs[1];
    ts.k_stride = p.ks[2], ts.v_stride = p.vs[2];
    ts.Sk = p.Sk;

    const uint16_t *qp = p.q + b * p.qs[0] + h * p.qs[1] + (long long)min(qrow, p.Sq - 1) * p.qs[2] + 8 * h2;
    Acc<D, 1> acc;
    tile_stream<Tr, D>(smem, ts, qp, acc, p.scale_log2, h2, lim, mask_bits, low_mask);

    // ---- epilogue: fold the sink, normalise, convert, store O[row][:] and lse ----
    float ltot = half_sum(acc.lsum[0]);
    if constexpr (SINK) fold_sink(acc, ltot, wp.sinks[h]);
    if (qrow < p.Sq)
        store_row<Tr, D>(acc, ltot, p.o + b * p.os[0] + h * p.os[1] + (long long)qrow * p.os[2], p.lse,
                         ((long long)b * p.Hq + h) * p.Sq + qrow, h2);
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
