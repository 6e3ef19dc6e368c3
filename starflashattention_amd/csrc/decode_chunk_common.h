// Device helpers of the multi-token decode step (decode_chunk_body.h): the rotation of the single-token decode kernels
// applied to one vector, so that a chunk of n tokens writes the cache bytes n successive sfa_decode calls would, and the
// chunk's rejection rule.  The bias, cos / sin and head offset helpers it shares with those kernels are decode_common.h's.
#pragma once
#include "decode_common.h"

namespace sfa {
namespace chunk {

using decode::add_bias8;
using decode::rope_cs;
using decode::head_base;

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

}  // namespace chunk
}  // namespace sfa
