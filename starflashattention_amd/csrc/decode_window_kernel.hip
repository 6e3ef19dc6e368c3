// sfa_decode_window: sfa_decode with a sliding window.  The new token at position pos attends to the cache rows
// [lo, pos) and to itself, lo = max(0, pos + 1 - window), computed here from seq_len: rows below lo, and the block_table
// entries of pages that lie wholly below lo, are never read.
//
// One matrix-core kernel for every group size: the body of decode_gqa_mfma_kernel.hip's kernel, decode_mfma16.h, with
// its WINDOW flag set (there: what the window changes in the wave slice, the row and page clamps and the tile's mask) and
// G = 1 .. 16 a run-time value as in decode_kv8_kernel.hip.  With lo = 0 the tile partition, and with it every bit of the
// result, is sfa_decode's.  This file keeps the kernel, its launchers and the split combine.
#include "decode_mfma16.h"

namespace sfa {

namespace {

using namespace decode;

template <class Tr, int D, bool NT, bool KLDS, bool PAGED>
__global__ void __launch_bounds__(kDecodeWaves * 64)
decode_window_kernel(const WindowKernelParams wp) {
    mfma16_decode<Tr, D, NT, KLDS, PAGED, /*WINDOW=*/true>(wp.d, wp.d.H / wp.d.Hkv, wp.window);
}

template <class Tr, int D, bool NT, bool KLDS, bool PAGED>
int launch_k(const WindowKernelParams &wp, hipStream_t stream) {
    const DecodeKernelParams &p = wp.d;
    dim3 grid(p.Hkv, p.num_splits, p.B), block(kDecodeWaves * 64);
    constexpr int lds = MfmaLds<D>::BYTES;
    static DynLdsAttr attr;
    if (const int rc = attr.ensure(reinterpret_cast<const void *>(&decode_window_kernel<Tr, D, NT, KLDS, PAGED>), lds,
                                   "decode_window_kernel"))
        return rc;
    hipLaunchKernelGGL((decode_window_kernel<Tr, D, NT, KLDS, PAGED>), grid, block, lds, stream, wp);
    return check_launch("decode_window_kernel");
}

template <class Tr, int D>
int launch_d(const WindowKernelParams &wp, bool nt, hipStream_t stream) {
    // the cache loads of decode_gqa_mfma_kernel.hip (launch_g): paged and the reference layout row-major through the
    // K tile, head-major caches straight into operand layout
    if (wp.d.block_table)
        return nt ? launch_k<Tr, D, true, true, true>(wp, stream) : launch_k<Tr, D, false, true, true>(wp, stream);
    if (wp.d.kv_row_stride != D)
        return nt ? launch_k<Tr, D, true, true, false>(wp, stream) : launch_k<Tr, D, false, true, false>(wp, stream);
    return nt ? launch_k<Tr, D, true, false, false>(wp, stream) : launch_k<Tr, D, false, false, false>(wp, stream);
}

}  // namespace

// head_dim 64 / 128 / 256, any cache layout, 1, 2, 4, 8 or 16 query heads per kv head; adds the split combine
int launch_decode_window(const WindowKernelParams &wp, int dtype, int head_dim, hipStream_t stream) {
    const DecodeKernelParams &p = wp.d;
    const bool nt = decode_nt(p, head_dim, 2);
    const bool h = dtype == SFA_DTYPE_FP16;
    const int rc = head_dim == 64    ? (h ? launch_d<Fp16, 64>(wp, nt, stream) : launch_d<Bf16, 64>(wp, nt, stream))
                   : head_dim == 256 ? (h ? launch_d<Fp16, 256>(wp, nt, stream) : launch_d<Bf16, 256>(wp, nt, stream))
                                     : (h ? launch_d<Fp16, 128>(wp, nt, stream) : launch_d<Bf16, 128>(wp, nt, stream));
    if (rc != SFA_OK || p.num_splits <= 1) return rc;
    return launch_decode_combine(p, dtype, head_dim, stream);
}

}  // namespace sfa
