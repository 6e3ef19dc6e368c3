// sfa_decode_kv8_window_sinks: sfa_decode_kv8_window (decode_kv8_window_kernel.hip) with an attention sink -- a learned
// logit per query head that joins every softmax as one more key with a zero value row:
//   o[h] = v_scale[hk] sum_j exp(s_j) V8_j / (exp(sinks[h]) + sum_j exp(s_j)),   j over [lo, pos],
//   s_j = q . (k_scale[hk] K8_j) * head_dim_inv
// The sink is scaled neither by head_dim_inv nor by k_scale.  A window >= memory_max_len makes this the sink over the
// whole history of an fp8 cache.
//
// The kernel is decode_kv8_window_kernel.hip's -- the body of decode_kv8_body.h with its WINDOW flag -- with the SINK flag
// set as well: nothing changes in the byte loads, the staging, the wave slices, the clamps, the quantised new token or
// its append; Tiles::merge_store folds the sink into the merged state of split 0 (decode_mfma_common.h), so it is counted
// once per query row whatever the split count, and the split combine is the one every decode call shares.  k_scale is
// part of the score scale, so that state's maximum is in true log2 units; v_scale multiplies the accumulator after the
// fold, and the sink's accumulator is 0.  The sink pointer rides behind the unchanged Kv8WindowKernelParams.  This file
// keeps the kernel and its launchers.
#include "decode_kv8_body.h"

namespace sfa {

namespace {

using namespace decode;

template <class Tr, int D, bool NT, bool PAGED>
__global__ void __launch_bounds__(kDecodeWaves * 64)
decode_kv8_window_sinks_kernel(const Kv8WindowSinksKernelParams sp) {
    kv8_decode<Tr, D, NT, PAGED, /*WINDOW=*/true, /*SINK=*/true>(sp.base.base, sp.base.window, sp.sinks);
}

template <class Tr, int D, bool NT, bool PAGED>
int launch_k(const Kv8WindowSinksKernelParams &sp, hipStream_t stream) {
    const DecodeKernelParams &p = sp.base.base.d;
    dim3 grid(p.Hkv, p.num_splits, p.B), block(kDecodeWaves * 64);
    constexpr int lds = MfmaLds<D>::BYTES;
    static DynLdsAttr attr;
    if (const int rc = attr.ensure(reinterpret_cast<const void *>(&decode_kv8_window_sinks_kernel<Tr, D, NT, PAGED>), lds,
                                   "decode_kv8_window_sinks_kernel"))
        return rc;
    hipLaunchKernelGGL((decode_kv8_window_sinks_kernel<Tr, D, NT, PAGED>), grid, block, lds, stream, sp);
    return check_launch("decode_kv8_window_sinks_kernel");
}

template <class Tr, int D>
int launch_d(const Kv8WindowSinksKernelParams &sp, bool nt, hipStream_t stream) {
    if (sp.base.base.d.block_table)
        return nt ? launch_k<Tr, D, true, true>(sp, stream) : launch_k<Tr, D, false, true>(sp, stream);
    return nt ? launch_k<Tr, D, true, false>(sp, stream) : launch_k<Tr, D, false, false>(sp, stream);
}

}  // namespace

// head_dim 64 / 128, any cache layout, 1, 2, 4, 8 or 16 query heads per kv head; adds the split combine
int launch_decode_kv8_window_sinks(const Kv8WindowSinksKernelParams &sp, int dtype, int head_dim, hipStream_t stream) {
    const DecodeKernelParams &p = sp.base.base.d;
    const bool nt = decode_nt(p, head_dim, 1);
    const bool h = dtype == SFA_DTYPE_FP16;
    const int rc = head_dim == 64 ? (h ? launch_d<Fp16, 64>(sp, nt, stream) : launch_d<Bf16, 64>(sp, nt, stream))
                                  : (h ? launch_d<Fp16, 128>(sp, nt, stream) : launch_d<Bf16, 128>(sp, nt, stream));
    if (rc != SFA_OK || p.num_splits <= 1) return rc;
    return launch_decode_combine(p, dtype, head_dim, stream);
}

}  // namespace sfa
