// Device helpers of the multi-token decode step (decode_chunk_body.h): the per-element bias / RoPE
// arithmetic of the single-token decode kernels, restated once so that a chunk of n tokens writes the cache
// bytes n successive sfa_decode calls would, and the chunk's rejection rule.
#pragma once
#include "decode_common.h"

namespace sfa {
namespace chunk {

// x[0..8) += bias[0..8) (fp32), as decode_kernel.hip adds q / k / v bias
template <class Tr>
__device__ __forceinline__ void add_bias8(float (&x)[8], const uint16_t *bias) {
    float t[8];
    decode::unpack8<Tr>(*reinterpret_cast<const uint4 *>(bias), t);
#pragma unroll
    for (int j = 0; j < 8; ++j) x[j] += t[j];
}

// cos / sin of RoPE pair pj at position pos: decode_kernel.hip's recipe -- the LUT row pos, or fp32 powf / sincosf.
template <class Tr>
__device__ __forceinline__ void rope_cs(int pj, int pos, const DecodeKernelParams &p, float &c, float &s) {
    const int rot = p.rot_dim;
    if (p.cos_tab) {
        const long long ti = (long long)pos * (rot >> 1) + pj;
        c = Tr::to_f32(p.cos_tab[ti]);
        s = Tr::to_f32(p.sin_tab[ti]);
    } else {
        const float inv_freq = 1.0f / powf(10000.0f, (float)(2 * pj) / (float)rot);
        const float ang = (float)pos * inv_freq;
        sincosf(ang, &s, &c);
    }
}

// Interleaved RoPE of this lane's 8 dims (pairs sub*4 .. sub*4+3), cos / sin of pair pj in cs[pj] / sn[pj]:
// decode_kernel.hip's rotation, applied to one vector.
__device__ __forceinline__ void rope8(float (&x)[8], int sub, int rot, const float *cs, const float *sn) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int pj = sub * 4 + i;                 // pair index: dims (2pj, 2pj+1)
        if (2 * pj < rot) {
            const float c = cs[pj], s = sn[pj];
            const float x0 = x[2 * i], x1 = x[2 * i + 1];
            x[2 * i] = x0 * c - x1 * s;
            x[2 * i + 1] = x1 * c + x0 * s;
        }
    }
}

// Which sticky status bit sequence b, with n >= 1 new tokens, raises before anything is touched (every kernel of the
// chunk computes the same value): 1 = pos < 0 or pos + n > memory_max_len; 2 = (paged) a block_table entry of a page covering the new
// rows [pos, pos+n) lies outside the pool.  0 = fine.  Workgroup-collective (all threads must call it).
template <bool PAGED>
__device__ __forceinline__ int reject_code(const DecodeKernelParams &p, int n, int b, int pos) {
    if (pos < 0 || pos > p.M - n) return 1;
    if (PAGED) {
        const int32_t *tbl = p.block_table + (long long)b * p.table_stride;
        const int first = pos >> p.page_shift, last = (pos + n - 1) >> p.page_shift;
        int bad = 0;
        for (int i = first + (int)threadIdx.x; i <= last; i += (int)blockDim.x)
            bad |= (unsigned)tbl[i] >= (unsigned)p.num_pages;
        if (__syncthreads_or(bad)) return 2;
    }
    return 0;
}

// Element offset of row 0 of kv head hk in the (b, layer) cache (contiguous layouts: row r is r * kv_row_stride
// further), or of the (layer, hk) slice of page 0 of the pool (paged: row r is page * page_stride +
// (r & page_mask) * kv_row_stride further).  As in decode_kernel.hip.
template <int D, bool PAGED>
__device__ __forceinline__ long long head_base(const DecodeKernelParams &p, int b, int hk) {
    if (PAGED) return (long long)p.layer * (p.kv_row_stride << p.page_shift) + (long long)hk * p.kv_head_stride;
    return ((long long)b * p.L + p.layer) * p.M * p.Hkv * D + (long long)hk * p.kv_head_stride;
}

}  // namespace chunk
}  // namespace sfa
