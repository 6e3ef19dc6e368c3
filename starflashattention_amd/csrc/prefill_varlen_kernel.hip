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
// The tile pipeline is prefill_stream.h's tile_stream without a lower bound, from tile 0 (design notes there and in
// prefill_kernel.hip); the epilogue is that header's store_row.  What is this kernel's own:
//   * The workgroup reads its plan item and its sequence's four cu entries with wave-uniform loads, leaves on the marker
//     before any barrier, and re-derives the sequence's validity (0 <= cu[b] <= cu[b+1] <= total in both arrays): the
//     kernel is safe for any cu contents, and an invalid sequence is neither read nor written (varlen_item of
//     prefill_varlen_seq.h, shared with prefill_varlen_window_kernel.hip).
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
#include "prefill_stream.h"
#include "prefill_varlen_seq.h"

namespace sfa {

namespace {

using namespace prefill;

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
    extern __shared__ __attribute__((aligned(16))) char smem[];

    VarlenItem it;
    if (!varlen_item(p, it)) return;            // before any barrier
    const int h = it.h, qt = it.qt, Sq = it.Sq, Sk = it.Sk;
    const int hk = h / (p.Hq / p.Hkv);

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);     // provably wave-uniform
    const int l31 = lane & 31, h2 = lane >> 5;
    const int coff = Sk - Sq;                   // causal: key j visible to row i iff j <= i + coff
    const int q0 = qt * kBM, wq0 = q0 + 32 * wave, qrow = wq0 + l31;

    // ---- the key range of this workgroup: tiles [0, wg_end), the whole range the q-tile's last row sees ----
    TileStream ts{};
    ts.ts0 = 0;
    ts.wg_end = (Sk + kBN - 1) / kBN;
    if (CAUSAL) {
        const int rlim = min(q0 + kBM, Sq) - 1 + coff;      // (<= Sk - 1)
        ts.wg_end = rlim < 0 ? 0 : rlim / kBN + 1;
    }
    ts.nt = ts.wg_end;                          // tiles the workgroup stages (workgroup-uniform); 0: no visible key
    const int wlast = min(wq0 + 31, Sq - 1);    // last query row of the wave
    ts.ntw = 0;                                 // end of the tiles this wave computes on (wave-uniform)
    if (wq0 < Sq) {
        if (!CAUSAL) ts.ntw = ts.nt;
        else if (wlast + coff >= 0) ts.ntw = min(ts.wg_end, (wlast + coff) / kBN + 1);
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

    // ---- epilogue: normalise, convert, store O[row][:] and lse; a row with no visible key gets zeros and -inf ----
    const float ltot = half_sum(acc.lsum[0]);
    if (qrow < Sq)
        store_row<Tr, D>(acc, ltot, p.o + ((long long)it.cq0 + qrow) * p.os[0] + h * p.os[1], p.lse,
                         (long long)h * p.total_q + it.cq0 + qrow, h2);
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

int launch_prefill_varlen_plan(const PrefillVarlenKernelParams &p, hipStream_t stream) {
    hipLaunchKernelGGL(prefill_varlen_plan_kernel, dim3(1), dim3(256), 0, stream, p);
    return check_launch("prefill_varlen_plan_kernel");
}

int launch_prefill_varlen(const PrefillVarlenKernelParams &p, int dtype, int head_dim, bool causal, hipStream_t stream) {
    if (const int rc = launch_prefill_varlen_plan(p, stream)) return rc;
    const bool h = dtype == SFA_DTYPE_FP16;
    if (head_dim == 64) return h ? launch_c<Fp16, 64>(p, causal, stream) : launch_c<Bf16, 64>(p, causal, stream);
    return h ? launch_c<Fp16, 128>(p, causal, stream) : launch_c<Bf16, 128>(p, causal, stream);
}

}  // namespace sfa
