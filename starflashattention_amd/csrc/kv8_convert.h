// e4m3 <-> 16 bit: the one copy of the conversions of the fp8 KV cache, for the single-token kernels (decode_kv8_body.h)
// and the multi-token step over such a cache (decode_chunk_body.h under Kv8Geo).
#pragma once
#include "sfa_device.h"

namespace sfa {
namespace decode {

// two e4m3 bytes (the low or the high half of w) -> two 16-bit values, exact
template <class Tr, bool HI> __device__ __forceinline__ uint32_t dq2(uint32_t w);
template <> __device__ __forceinline__ uint32_t dq2<Bf16, false>(uint32_t w) {
    return bitcast<uint32_t>(__builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, 1.0f, false));
}
template <> __device__ __forceinline__ uint32_t dq2<Bf16, true>(uint32_t w) {
    return bitcast<uint32_t>(__builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, 1.0f, true));
}
template <> __device__ __forceinline__ uint32_t dq2<Fp16, false>(uint32_t w) {
    return bitcast<uint32_t>(__builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w, 1.0f, false));
}
template <> __device__ __forceinline__ uint32_t dq2<Fp16, true>(uint32_t w) {
    return bitcast<uint32_t>(__builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w, 1.0f, true));
}
// 8 bytes -> 8 16-bit values
template <class Tr> __device__ __forceinline__ uint4 dq8(uint32_t a, uint32_t b) {
    return make_uint4(dq2<Tr, false>(a), dq2<Tr, true>(a), dq2<Tr, false>(b), dq2<Tr, true>(b));
}

// q8 of four values: clamp to +-448 in fp32 (so the conversion's own overflow mode never matters), round to the nearest
// e4m3 with ties to even, NaN -> 0x7F
__device__ __forceinline__ uint32_t q8x4(float a, float b, float c, float d) {
    auto cl = [](float x) { return fminf(fmaxf(x, -448.f), 448.f); };
    int w = __builtin_amdgcn_cvt_pk_fp8_f32(cl(a), cl(b), 0, false);
    w = __builtin_amdgcn_cvt_pk_fp8_f32(cl(c), cl(d), w, true);
    uint32_t u = (uint32_t)w;
    if (a != a) u = (u & 0xffffff00u) | 0x0000007fu;
    if (b != b) u = (u & 0xffff00ffu) | 0x00007f00u;
    if (c != c) u = (u & 0xff00ffffu) | 0x007f0000u;
    if (d != d) u = (u & 0x00ffffffu) | 0x7f000000u;
    return u;
}
// q8(x[j] / scale) for 8 values (the division is the correctly rounded fp32 one)
__device__ __forceinline__ uint2 q8x8(const float (&x)[8], float scale) {
    return make_uint2(q8x4(x[0] / scale, x[1] / scale, x[2] / scale, x[3] / scale),
                      q8x4(x[4] / scale, x[5] / scale, x[6] / scale, x[7] / scale));
}

}  // namespace decode
}  // namespace sfa
