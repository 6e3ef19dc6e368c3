// The uniform geometry of the multi-token decode step (decode_chunk_body.h): the same n for every sequence.  Shared by
// decode_chunk_kernel.hip and its sliding-window twin, decode_chunk_window_kernel.hip.  It stays in an unnamed namespace:
// each translation unit instantiates the chunk kernels over a type of its own, so the two sets of kernels never meet
// at link time and the kernels of decode_chunk_kernel.hip keep the names they had when the struct lived there.
#pragma once
#include "decode_chunk_body.h"

namespace sfa {

namespace {

// The same n for every sequence: dense [B, n, ...] qkv / o, the rotated Q [B, Hkv, R, D], partials [B, Hkv, S, R, ..],
// one attention workgroup per (q-tile, kv head * S + split, batch).
struct UniformGeo {
    using Params = ChunkKernelParams;
    static __device__ __forceinline__ const ChunkKernelParams &chunk(const Params &cp) { return cp; }
    static __device__ __forceinline__ bool prologue(const Params &cp, int &b, int &t, int &n) {
        t = blockIdx.x, b = blockIdx.y, n = cp.n;
        return true;
    }
    static __device__ __forceinline__ long long qkv_off(const Params &cp, int b, int t) {
        return (long long)b * cp.d.qkv_stride + (long long)t * cp.tok_stride;
    }
    static __device__ __forceinline__ bool attn(const Params &cp, int &b, int &qt, int &hs, int &n, int &R) {
        qt = (int)gridDim.x - 1 - (int)blockIdx.x;
        hs = blockIdx.y;
        b = blockIdx.z, n = cp.n, R = cp.R;
        return true;
    }
    static __device__ __forceinline__ long long q_row(const Params &cp, int b, int hk, long long r) {
        return ((long long)b * cp.d.Hkv + hk) * cp.R + r;
    }
    static __device__ __forceinline__ long long part_row(const Params &cp, int b, int hk, int split, long long r) {
        return (((long long)b * cp.d.Hkv + hk) * cp.d.num_splits + split) * cp.R + r;
    }
    static __device__ __forceinline__ long long o_tok(const Params &cp, int b, int t) { return (long long)b * cp.n + t; }
    static __device__ __forceinline__ bool combine(const Params &cp, long long row, long long &grp, long long &rows,
                                                   long long &r, long long &tok, int &head) {
        if (row >= (long long)cp.d.B * cp.d.Hkv * cp.R) return false;
        const int ri = (int)(row % cp.R);
        grp = row / cp.R;                       // b * Hkv + hk
        const int hk = (int)(grp % cp.d.Hkv), b = (int)(grp / cp.d.Hkv);
        rows = cp.R, r = ri;
        tok = (long long)b * cp.n + ri / cp.G;
        head = hk * cp.G + ri % cp.G;
        return true;
    }
};

}  // namespace

}  // namespace sfa
