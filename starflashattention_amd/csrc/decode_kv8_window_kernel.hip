// sfa_decode_kv8_window: sfa_decode_kv8 with a sliding window.  The new token at position pos attends to the cache rows
// [lo, pos) and to itself, lo = max(0, pos + 1 - window), computed here from seq_len: rows below lo, and the block_table
// entries of pages that lie wholly below lo, are never read.
//
// One matrix-core kernel for every group size: the body of decode_kv8_kernel.hip's kernel, decode_kv8_body.h, with its
// WINDOW flag set (there: what the window changes in the wave slice, the row and page clamps and the tile's mask).  The
// quantised new token, its append, the scales and the two tiles in flight are that body's, unchanged.  With lo = 0 the
// tile partition, and with it every bit of the result, is sfa_decode_kv8's.  This file keeps the kernel, its launchers and
// the split combine.
#include "decode_kv8_body.h"

namespace sfa {

namespace {

using namespace decode;

template <class Tr, int D, bool NT, bool PAGED>
__global__ void __launch_bounds__(kDecodeWaves * 64)
decode_kv8_window_kernel(const Kv8WindowKernelParams wp) {
    kv8_decode<Tr, D, NT, PAGED, /*WINDOW=*/true>(wp.base, wp.window);
}

template <class Tr, int D, bool NT, bool PAGED>
int launch_k(const Kv8WindowKernelParams &wp, hipStream_t stream) {
    const DecodeKernelParams &p = wp.base.d;
    dim3 grid(p.Hkv, p.num_splits, p.B), block(kDecodeWaves * 64);
    constexpr int lds = MfmaLds<D>::BYTES;
    static DynLdsAttr attr;
    if (const int rc = attr.ensure(reinterpret_cast<const void *>(&decode_kv8_window_kernel<Tr, D, NT, PAGED>), lds,
                                   "decode_kv8_window_kernel"))
        return rc;
    hipLaunchKernelGGL((decode_kv8_window_kernel<Tr, D, NT, PAGED>), grid, block, lds, stream, wp);
    return check_launch("decode_kv8_window_kernel");
}

template <class Tr, int D>
int launch_d(const Kv8WindowKernelParams &wp, bool nt, hipStream_t stream) {
    if (wp.base.d.block_table)
        return nt ? launch_k<Tr, D, true, true>(wp, stream) : launch_k<Tr, D, false, true>(wp, stream);
    return nt ? launch_k<Tr, D, true, false>(wp, stream) : launch_k<Tr, D, false, false>(wp, stream);
}

}  // namespace

// head_dim 64 / 128, any cache layout, 1, 2, 4, 8 or 16 query heads per kv head; adds the split combine
int launch_decode_kv8_window(const Kv8WindowKernelParams &wp, int dtype, int head_dim, hipStream_t stream) {
    const DecodeKernelParams &p = wp.base.d;
    const bool nt = decode_nt(p, head_dim, 1);
    const bool h = dtype == SFA_DTYPE_FP16;
    const int rc = head_dim == 64 ? (h ? launch_d<Fp16, 64>(wp, nt, stream) : launch_d<Bf16, 64>(wp, nt, stream))
                                  : (h ? launch_d<Fp16, 128>(wp, nt, stream) : launch_d<Bf16, 128>(wp, nt, stream));
    if (rc != SFA_OK || p.num_splits <= 1) return rc;
    return launch_decode_combine(p, dtype, head_dim, stream);
}

}  // namespace sfa
