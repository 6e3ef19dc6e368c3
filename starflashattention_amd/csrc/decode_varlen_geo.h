// The ragged geometry of the multi-token decode step (decode_chunk_body.h) and its plan kernel: a token count of its
// own per sequence, packed.  Shared by decode_varlen_kernel.hip and its sliding-window twin,
// decode_varlen_window_kernel.hip; in an unnamed namespace for the reason given in decode_chunk_geo.h.
#pragma once
#include "decode_chunk_body.h"

namespace sfa {

namespace {

// The token range [c0, c1) of sequence b; false when it is empty or not a range inside [0, total).
__device__ __forceinline__ bool seq_range(const VarlenKernelParams &vp, int b, int &c0, int &c1) {
    c0 = vp.cu_tokens[b], c1 = vp.cu_tokens[b + 1];
    return c0 >= 0 && c0 < c1 && c1 <= vp.total;
}

// The sequence that owns packed row `row` (cu[b] <= row < cu[b+1], a valid range), or -1.  Binary search for the last
// b with cu[b] <= row; the range check afterwards makes the answer safe for any cu_tokens contents.
__device__ __forceinline__ int seq_of_row(const VarlenKernelParams &vp, int row, int &c0, int &c1) {
    int lo = 0, hi = vp.c.d.B;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (vp.cu_tokens[mid] <= row) lo = mid; else hi = mid;
    }
    return seq_range(vp, lo, c0, c1) && c0 <= row && row < c1 ? lo : -1;
}

struct RaggedGeo {
    using Params = VarlenKernelParams;
    static __device__ __forceinline__ const ChunkKernelParams &chunk(const Params &vp) { return vp.c; }
    static __device__ __forceinline__ bool prologue(const Params &vp, int &b, int &t, int &n) {
        int c0, c1;
        b = seq_of_row(vp, blockIdx.x, c0, c1);
        if (b < 0) return false;
        t = (int)blockIdx.x - c0, n = c1 - c0;
        return true;
    }
    static __device__ __forceinline__ long long qkv_off(const Params &vp, int b, int t) {
        return (long long)(vp.cu_tokens[b] + t) * vp.c.tok_stride;
    }
    // 1-D grid, plan index on the slow digit: every workgroup of every real item is launched before the first empty slot
    static __device__ __forceinline__ bool attn(const Params &vp, int &b, int &qt, int &hs, int &n, int &R) {
        const int per_item = vp.c.d.Hkv * vp.c.d.num_splits;
        hs = (int)(blockIdx.x % per_item);
        const int2 item = vp.plan[blockIdx.x / per_item];
        b = item.x, qt = item.y;
        if (b < 0) return false;                // the empty marker
        int c0, c1;
        if (!seq_range(vp, b, c0, c1)) return false;
        n = c1 - c0, R = n * vp.c.G;            // (n * G <= total * G, an int: checked by sfa_decode_varlen)
        return qt * prefill::kBM < R;
    }
    // rotated Q [Hkv, total * G, D] and partials [Hkv, S, total * G, ..]: row cu[b] * G + r of kv head hk
    static __device__ __forceinline__ long long q_row(const Params &vp, int b, int hk, long long r) {
        return (long long)hk * vp.rows + (long long)vp.cu_tokens[b] * vp.c.G + r;
    }
    static __device__ __forceinline__ long long part_row(const Params &vp, int b, int hk, int split, long long r) {
        return ((long long)hk * vp.c.d.num_splits + split) * vp.rows + (long long)vp.cu_tokens[b] * vp.c.G + r;
    }
    static __device__ __forceinline__ long long o_tok(const Params &vp, int b, int t) { return vp.cu_tokens[b] + t; }
    static __device__ __forceinline__ bool combine(const Params &vp, long long row, long long &grp, long long &rows,
                                                   long long &r, long long &tok, int &head) {
        if (row >= (long long)vp.c.d.Hkv * vp.rows) return false;
        grp = row / vp.rows, rows = vp.rows, r = row % vp.rows;
        tok = r / vp.c.G;
        head = (int)grp * vp.c.G + (int)(r % vp.c.G);
        int c0, c1;
        return seq_of_row(vp, (int)tok, c0, c1) >= 0;
    }
};

// plan[i] = (b, q_tile) for the i-th work item, (-1, 0) from the last item up to vp.bound.  One workgroup walks the
// sequences 256 at a time: tile counts, an exclusive scan in LDS, then every thread writes its sequence's items.
__global__ void __launch_bounds__(256)
varlen_plan_kernel(const VarlenKernelParams vp) {
    __shared__ int scan[256];
    __shared__ int base_s;
    const int tid = threadIdx.x, B = vp.c.d.B;
    if (tid == 0) base_s = 0;
    __syncthreads();
    for (int b0 = 0; b0 < B; b0 += 256) {
        const int b = b0 + tid;
        int tiles = 0;
        if (b < B) {
            int c0, c1;
            if (seq_range(vp, b, c0, c1)) tiles = ((c1 - c0) * vp.c.G + prefill::kBM - 1) / prefill::kBM;
            else if (c0 != c1) atomicOr(vp.c.d.status, 1);      // not a range of [0, total): skipped
        }
        scan[tid] = tiles;
        __syncthreads();
        for (int d = 1; d < 256; d <<= 1) {     // inclusive Hillis-Steele scan
            const int add = tid >= d ? scan[tid - d] : 0;
            __syncthreads();
            scan[tid] += add;
            __syncthreads();
        }
        const int base = base_s;
        const int first = base + scan[tid] - tiles;
        for (int i = 0; i < tiles; ++i)
            if (first + i < vp.bound) vp.plan[first + i] = make_int2(b, tiles - 1 - i);
        __syncthreads();
        if (tid == 255) base_s = min(base + scan[255], vp.bound);
        __syncthreads();
    }
    for (int i = base_s + tid; i < vp.bound; i += 256) vp.plan[i] = make_int2(-1, 0);
}

}  // namespace

}  // namespace sfa
