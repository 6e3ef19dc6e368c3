// Prefill forward with a split key range for gfx950 (MI355X): sfa_prefill_split_fwd with two or more splits.
// bf16 / fp16, head_dim 64 / 128, causal (bottom-right aligned) or full, MHA or GQA, [B, H, S, D] tensors with any strides.
//
// Two kernels on one stream:
//   prefill_split_kernel          one workgroup per (batch, head, q-tile, split): the tiles [s C, min((s + 1) C, nkt(qt))) of
//                                 the q-tile's key range, C = tiles_per_split, into fp32 partials (O un-normalised, the
//                                 reference max m in log2 units, the row sum l) in the workspace
//   prefill_split_combine_kernel  per query row: m = max m_s, l = sum 2^(m_s - m) l_s, o = sum 2^(m_s - m) O_s / l,
//                                 lse = (m + log2 l) ln 2, over the splits that are not empty for the row's q-tile
// The tile pipeline is prefill_stream.h's tile_stream without a lower bound (design notes there and in
// prefill_kernel.hip).  What is this kernel's own:
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
#include "prefill_stream.h"

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
    constexpr int NDB = StreamDims<D>::NDB;
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
    TileStream ts{};
    ts.ts0 = split * sp.tiles_per_split;
    ts.wg_end = min(ts.ts0 + sp.tiles_per_split, tiles_of_qtile<CAUSAL>(p, qt));
    ts.nt = ts.wg_end - ts.ts0;                 // tiles the workgroup stages (workgroup-uniform)
    if (ts.nt <= 0) return;                     // an empty split: nothing read, nothing written (the combine skips it)
    const int wlast = min(wq0 + 31, p.Sq - 1);  // last query row of the wave
    ts.ntw = 0;                                 // end of the tiles this wave computes on, from ts0 (wave-uniform)
    if (wq0 < p.Sq) {
        if (!CAUSAL) ts.ntw = ts.nt;
        else if (wlast + coff >= 0) ts.ntw = max(0, min(ts.wg_end, (wlast + coff) / kBN + 1) - ts.ts0);
    }
    int lim[1];                                 // last visible key of this lane's row (< 0: none)
    lim[0] = CAUSAL ? min(qrow, p.Sq - 1) + coff : p.Sk - 1;
    const int wlim = CAUSAL ? wq0 + coff : p.Sk - 1;    // the smallest limit of the wave's rows
    // bit 0 set: the 32 keys starting at KBASE need masking for this wave's rows
    auto mask_bits = [&](int kbase) -> int { return kbase + 31 > wlim ? 1 : 0; };
    ts.k = p.k + b * p.ks[0] + hk * p.ks[1];
    ts.v = p.v + b * p.vs[0] + hk * p.vs[1];
    ts.k_stride = p.ks[2], ts.v_stride = p.vs[2];
    ts.Sk = p.Sk;

    const uint16_t *qp = p.q + b * p.qs[0] + h * p.qs[1] + (long long)min(qrow, p.Sq - 1) * p.qs[2] + 8 * h2;
    Acc<D, 1> acc;
    tile_stream<Tr, D>(smem, ts, qp, acc, p.scale_log2, h2, lim, mask_bits, NoLowMask());

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
