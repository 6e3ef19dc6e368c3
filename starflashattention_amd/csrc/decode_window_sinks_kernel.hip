// sfa_decode_window_sinks: sfa_decode_window (decode_window_kernel.hip) with an attention sink -- a learned logit per
// query head that joins every softmax as one more key with a zero value row:
//   o[h] = sum_j exp(s_j) V_j / (exp(sinks[h]) + sum_j exp(s_j)),   j over [lo, pos], s_j = q . K_j * head_dim_inv
// The sink is not scaled by head_dim_inv.  A window >= memory_max_len makes this the sink over the whole history.
//
// The kernel is decode_window_kernel.hip's -- the body of decode_mfma16.h with its WINDOW flag -- with the SINK flag set as
// well: nothing changes in the tiles, the wave slices, the clamps or the append; Tiles::merge_store folds the sink into
// the merged state of split 0 (decode_mfma_common.h), so it is counted once per query row whatever the split count, and
// the split combine is the one every decode call shares.  The sink pointer rides behind the unchanged parameters.  This
// file keeps the kernel and its launchers.
#include "decode_mfma16.h"

namespace sfa {

namespace {

using namespace decode;

template <class Tr, int D, bool NT, bool KLDS, bool PAGED>
__global__ void __launch_bounds__(kDecodeWaves * 64)
decode_window_sinks_kernel(const WindowSinksKernelParams sp) {
    mfma16_decode<Tr, D, NT, KLDS, PAGED, /*WINDOW=*/true, /*SINK=*/true>(sp.base.d, sp.base.d.H / sp.base.d.Hkv,
                                                                          sp.base.window, sp.sinks);
}

template <class Tr, int D, bool NT, bool KLDS, bool PAGED>
int launch_k(const WindowSinksKernelParams &sp, hipStream_t stream) {
    const DecodeKernelParams &p = sp.base.d;
    dim3 grid(p.Hkv, p.num_splits, p.B), block(kDecodeWaves * 64);
    constexpr int lds = MfmaLds<D>::BYTES;
    static DynLdsAttr attr;
    if (const int rc = attr.ensure(reinterpret_cast<const void *>(&decode_window_sinks_kernel<Tr, D, NT, KLDS, PAGED>), lds,
                                   "decode_window_sinks_kernel"))
        return rc;
    hipLaunchKernelGGL((decode_window_sinks_kernel<Tr, D, NT, KLDS, PAGED>), grid, block, lds, stream, sp);
    return check_launch("decode_window_sinks_kernel");
}

template <class Tr, int D>
int launch_d(const WindowSinksKernelParams &sp, bool nt, hipStream_t stream) {
    // the cache loads of decode_window_kernel.hip (launch_d)
    const DecodeKernelParams &p = sp.base.d;
    if (p.block_table)
        return nt ? launch_k<Tr, D, true, true, true>(sp, stream) : launch_k<Tr, D, false, true, true>(sp, stream);
    if (p.kv_row_stride != D)
        return nt ? launch_k<Tr, D, true, true, false>(sp, stream) : launch_k<Tr, D, false, true, false>(sp, stream);
    return nt ? launch_k<Tr, D, true, false, false>(sp, stream) : launch_k<Tr, D, false, false, false>(sp, stream);
}

}  // namespace

// head_dim 64 / 128 / 256, any cache layout, 1, 2, 4, 8 or 16 query heads per kv head; adds the split combine
int launch_decode_window_sinks(const WindowSinksKernelParams &sp, int dtype, int head_dim, hipStream_t stream) {
    const DecodeKernelParams &p = sp.base.d;
    const bool nt = decode_nt(p, head_dim, 2);
    const bool h = dtype == SFA_DTYPE_FP16;
    const int rc = head_dim == 64    ? (h ? launch_d<Fp16, 64>(sp, nt, stream) : launch_d<Bf16, 64>(sp, nt, stream))
                   : head_dim == 256 ? (h ? launch_d<Fp16, 256>(sp, nt, stream) : launch_d<Bf16, 256>(sp, nt, stream))
                                     : (h ? launch_d<Fp16, 128>(sp, nt, stream) : launch_d<Bf16, 128>(sp, nt, stream));
    if (rc != SFA_OK || p.num_splits <= 1) return rc;
    return launch_decode_combine(p, dtype, head_dim, stream);
}

}  // namespace sfa
