// Grouped-query decode on the matrix cores, for groups too large for the VALU kernel
// (decode_gqa_kernel.hip is VALU-bound from 8 query heads per kv head on: 4.1 of 6.5 TB/s).
// One workgroup per (batch, kv head, split), four waves, each wave walks its share of the cached rows
// in 32-key tiles on v_mfma_f32_16x16x32 (16 query columns of which G are real):
//   S^T[key][q] = K . Q^T     A = K rows: head-major caches are read from HBM DIRECTLY in operand layout
//                                 (lane (c = l & 15, g = l >> 4) loads K[t + 16kt + c][32ks + 8g .. +8]);
//                                 the reference layout is read row-major and re-laid out through a
//                                 wave-private LDS tile (64-B pieces of strided rows cost 8 %);
//                             B = Q^T held in registers for the whole kernel (re-laid out once through LDS);
//   O^T[d][q] += V^T . P^T    P^T = the exponentiated S^T accumulators, packed (no data movement);
//                             V^T through a wave-private LDS tile: row-major ds_write_b128 in, ds_read_b64_tr_b16
//                             out (no barrier: a wave's LDS operations execute in order).
// The query sits on the lane in both accumulators: one online-softmax state per lane, row max across the
// four 16-lane groups by v_permlane32_swap + v_permlane16_swap.  Scores are scaled in fp32 (exact).
// The new token is one more tile of one valid key whose K/V come from the prologue's registers.
// Per 32 keys a wave issues 16 MFMAs and ~60 VALU instructions for 16 KB of cache: HBM-bound for any G <= 16.
// The kernel's body is decode_mfma16.h (the cache loads, operand-layout or row-major through the K tile, the two-tile
// software pipeline and the append; shared with decode_window_kernel.hip) over decode_mfma_common.h (what does not depend
// on the cache's element type: rejection, prologue, wave slice, paging, the tile math, the merge of the waves; shared with
// decode_kv8_kernel.hip as well).  This file keeps the kernel with G a template constant, and its launchers.
#include <cstdlib>

#include "decode_mfma16.h"

namespace sfa {

namespace {

using namespace decode;

template <class Tr, int D, int G, bool NT, bool KLDS, bool PAGED = false>
__global__ void __launch_bounds__(kDecodeWaves * 64)
decode_gqa_mfma_kernel(const DecodeKernelParams p) {
    mfma16_decode<Tr, D, NT, KLDS, PAGED, /*WINDOW=*/false>(p, G, 0);
}

template <class Tr, int D, int G, bool NT, bool KLDS, bool PAGED = false>
int launch_k(const DecodeKernelParams &p, hipStream_t stream) {
    dim3 grid(p.Hkv, p.num_splits, p.B), block(kDecodeWaves * 64);
    constexpr int lds = MfmaLds<D>::BYTES;
    static DynLdsAttr attr;
    if (const int rc = attr.ensure(reinterpret_cast<const void *>(&decode_gqa_mfma_kernel<Tr, D, G, NT, KLDS, PAGED>), lds,
                                   "decode_gqa_mfma_kernel"))
        return rc;
    hipLaunchKernelGGL((decode_gqa_mfma_kernel<Tr, D, G, NT, KLDS, PAGED>), grid, block, lds, stream, p);
    return check_launch("decode_gqa_mfma_kernel");
}

template <class Tr, int D, int G>
int launch_g(const DecodeKernelParams &p, bool nt, hipStream_t stream) {
    // Reference layout: a K row of this head is a 256-B segment H*D*2 bytes from the next, and fetching it
    // as 64-B operand pieces costs 8 % (5.96 vs 6.44 TB/s): load row-major, re-lay out through LDS.
    // Head-major caches are contiguous, the operand-layout loads go straight to registers (6.7 TB/s).
    if (p.block_table)
        return nt ? launch_k<Tr, D, G, true, true, true>(p, stream) : launch_k<Tr, D, G, false, true, true>(p, stream);
    const bool klds = p.kv_row_stride != D;
    if (klds) return nt ? launch_k<Tr, D, G, true, true>(p, stream) : launch_k<Tr, D, G, false, true>(p, stream);
    return nt ? launch_k<Tr, D, G, true, false>(p, stream) : launch_k<Tr, D, G, false, false>(p, stream);
}

template <class Tr, int D>
int launch_d(const DecodeKernelParams &p, bool nt, hipStream_t stream) {
    if (p.H == 16 * p.Hkv) return launch_g<Tr, D, 16>(p, nt, stream);
    if (p.H == 4 * p.Hkv) return launch_g<Tr, D, 4>(p, nt, stream);
    return launch_g<Tr, D, 8>(p, nt, stream);
}

}  // namespace

// head_dim 64 / 128 / 256, any cache layout, 4, 8 or 16 query heads per kv head
int launch_decode_gqa_mfma(const DecodeKernelParams &p, int dtype, int head_dim, bool nt, hipStream_t stream) {
    const bool h = dtype == SFA_DTYPE_FP16;
    if (head_dim == 64) return h ? launch_d<Fp16, 64>(p, nt, stream) : launch_d<Bf16, 64>(p, nt, stream);
    if (head_dim == 256) return h ? launch_d<Fp16, 256>(p, nt, stream) : launch_d<Bf16, 256>(p, nt, stream);
    return h ? launch_d<Fp16, 128>(p, nt, stream) : launch_d<Bf16, 128>(p, nt, stream);
}

}  // namespace sfa
