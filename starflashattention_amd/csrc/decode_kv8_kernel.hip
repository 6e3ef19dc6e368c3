// sfa_decode_kv8: sfa_decode over caches of one byte per element (OCP e4m3, torch's float8_e4m3fn), and
// sfa_kv8_quantize, which moves rows of a 16-bit cache into such a cache.
//
// One matrix-core kernel for every group size: the design of decode_gqa_mfma_kernel.hip, whose body this kernel shares
// through decode_mfma_common.h (rejection, prologue, wave slice, paging, the tile math and the merge of the waves), with
// G = 1 .. 16 a run-time value.  What the fp8 kernels add: the caches are read on the row-major path in all three layouts,
//   a lane loads 16 bytes = 16 elements, so D/16 lanes cover a cache row and one load instruction of a wave 64/(D/16)
//   rows; the bytes are converted to the 16-bit dtype in registers (v_cvt_scalef32_pk_{bf16,f16}_fp8 with scale 1.0:
//   every e4m3 value is exact in fp16 and in bf16) and written to the wave-private K and V tiles in LDS;
// the software pipeline (kInFlight), the quantisation of the new token and its append, and kv8_quantize_kernel.
// The scales never touch the tiles: k_scale[hk] is folded into the fp32 score scale, v_scale[hk] multiplies the fp32
// accumulator once in the epilogue (before the partials are written when the key range is split, so
// decode_combine_kernel merges them unchanged).
// The new token is quantised first, q8(x16 / scale), and takes part in the attention through its dequantised value: the
// output is a function of the cache contents after the step.
// Two tiles per wave are in flight in registers (2 x 8 KB at head_dim 128, the bytes decode_gqa_mfma_kernel keeps in
// flight with one 16-bit tile).
// The body, from the rejection to the merge of the waves, is decode_kv8_body.h (one copy with decode_kv8_window_kernel.hip,
// whose kernels set its WINDOW flag); this file keeps the kernel, its launchers, the split combine and kv8_quantize_kernel.
#include "decode_kv8_body.h"

namespace sfa {

namespace {

using namespace decode;

template <class Tr, int D, bool NT, bool PAGED>
__global__ void __launch_bounds__(kDecodeWaves * 64)
decode_kv8_kernel(const Kv8KernelParams kp) {
    kv8_decode<Tr, D, NT, PAGED, /*WINDOW=*/false>(kp, 0);
}

template <class Tr, int D, bool NT, bool PAGED>
int launch_k(const Kv8KernelParams &kp, hipStream_t stream) {
    const DecodeKernelParams &p = kp.d;
    dim3 grid(p.Hkv, p.num_splits, p.B), block(kDecodeWaves * 64);
    constexpr int lds = MfmaLds<D>::BYTES;
    static DynLdsAttr attr;
    if (const int rc = attr.ensure(reinterpret_cast<const void *>(&decode_kv8_kernel<Tr, D, NT, PAGED>), lds,
                                   "decode_kv8_kernel"))
        return rc;
    hipLaunchKernelGGL((decode_kv8_kernel<Tr, D, NT, PAGED>), grid, block, lds, stream, kp);
    return check_launch("decode_kv8_kernel");
}

template <class Tr, int D>
int launch_d(const Kv8KernelParams &kp, bool nt, hipStream_t stream) {
    if (kp.d.block_table) return nt ? launch_k<Tr, D, true, true>(kp, stream) : launch_k<Tr, D, false, true>(kp, stream);
    return nt ? launch_k<Tr, D, true, false>(kp, stream) : launch_k<Tr, D, false, false>(kp, stream);
}

// ---- sfa_kv8_quantize: dst[r, h, d] = q8(src[r, h, d] / scale[h]).  A thread owns 16 elements: two 16-byte loads, one
// 16-byte store.
template <class Tr>
__global__ void __launch_bounds__(256)
kv8_quantize_kernel(uint8_t *dst, const uint16_t *src, const float *scale, long long rows, int Hkv, int chunks,
                    long long src_row, long long src_head, long long dst_row, long long dst_head) {
    const long long total = rows * Hkv * chunks;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int ch = (int)(i % chunks);
        const long long rh = i / chunks;
        const int h = (int)(rh % Hkv);
        const long long r = rh / Hkv;
        const uint16_t *s = src + r * src_row + h * src_head + 16 * ch;
        const float sc = scale ? scale[h] : 1.0f;
        float x[8], y[8];
        unpack8<Tr>(*reinterpret_cast<const uint4 *>(s), x);
        unpack8<Tr>(*reinterpret_cast<const uint4 *>(s + 8), y);
        const uint2 a = q8x8(x, sc), bq = q8x8(y, sc);
        *reinterpret_cast<uint4 *>(dst + r * dst_row + h * dst_head + 16 * ch) = make_uint4(a.x, a.y, bq.x, bq.y);
    }
}

}  // namespace

// head_dim 64 / 128, any cache layout, 1, 2, 4, 8 or 16 query heads per kv head; adds the split combine
int launch_decode_kv8(const Kv8KernelParams &kp, int dtype, int head_dim, hipStream_t stream) {
    const DecodeKernelParams &p = kp.d;
    const bool nt = decode_nt(p, head_dim, 1);
    const bool h = dtype == SFA_DTYPE_FP16;
    const int rc = head_dim == 64 ? (h ? launch_d<Fp16, 64>(kp, nt, stream) : launch_d<Bf16, 64>(kp, nt, stream))
                                  : (h ? launch_d<Fp16, 128>(kp, nt, stream) : launch_d<Bf16, 128>(kp, nt, stream));
    if (rc != SFA_OK || p.num_splits <= 1) return rc;
    return launch_decode_combine(p, dtype, head_dim, stream);
}

int launch_kv8_quantize(void *dst, const void *src, const float *scale, long long rows, int Hkv, int head_dim,
                        long long src_row, long long src_head, long long dst_row, long long dst_head, int dtype,
                        hipStream_t stream) {
    const int chunks = head_dim / 16;
    const long long threads = rows * Hkv * chunks;
    if (threads == 0) return SFA_OK;
    const long long blocks = (threads + 255) / 256;
    dim3 grid((unsigned)(blocks < 65536 ? blocks : 65536)), block(256);
    if (dtype == SFA_DTYPE_FP16)
        hipLaunchKernelGGL((kv8_quantize_kernel<Fp16>), grid, block, 0, stream, (uint8_t *)dst, (const uint16_t *)src, scale,
                           rows, Hkv, chunks, src_row, src_head, dst_row, dst_head);
    else
        hipLaunchKernelGGL((kv8_quantize_kernel<Bf16>), grid, block, 0, stream, (uint8_t *)dst, (const uint16_t *)src, scale,
                           rows, Hkv, chunks, src_row, src_head, dst_row, dst_head);
    return check_launch("kv8_quantize_kernel");
}

}  // namespace sfa
