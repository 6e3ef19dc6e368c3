// Multi-token decode step (sfa_decode_chunk) for gfx950 (MI355X): n new tokens per sequence in one call, with
// the semantics of n successive sfa_decode calls -- prompt ingestion into the cache, chunked prefill against the
// cache already built, speculative-decoding verification.
//
// Three launches, ordered by the stream alone:
//   1. chunk_prologue_kernel (memory-bound): bias, interleaved RoPE at position seq_len[b] + t, rounding to the
//      16-bit dtype (decode_chunk_common.h, the arithmetic of decode_kernel.hip), K/V rows appended to the cache
//      (any kv_layout), the rotated Q written to the workspace as [B, Hkv, R = n*G, D] with row r = t*G + g, so a
//      row's causal limit pos + r/G is monotone in r.
//   2. chunk_attn_kernel (the hot path): prefill_kernel.hip's 8-wave, 256-row q-tile -- K/V tiles of 64 keys
//      register-staged into LDS once per workgroup and shared by all waves, h_block (prefill_core.h) at exact scale
//      (ORD 2) -- with three differences: K/V rows are read from the cache (the new rows included: they were
//      written by launch 1), the key count Kb = pos + n and the causal limit of row r, key j visible iff
//      j <= pos + r/G, come from seq_len[b] on the device, and the rows of a workgroup are (token, query head)
//      pairs of ONE kv head, so K/V are read once per group.  When B * Hkv * row tiles cannot fill the chip the
//      key range [0, Kb) is split (on the device, in whole 64-key tiles) and each split writes fp32 partials.
//   3. chunk_combine_kernel (num_splits > 1 only): merges the partials, as decode_combine_kernel does.  A split
//      that lies past a row's causal limit left (m = -inf, l = 0) for it, which the merge ignores.
// The kernels themselves are in decode_chunk_body.h, shared with the ragged sfa_decode_varlen; decode_chunk_geo.h holds
// the uniform geometry (UniformGeo), this file its grids.
// Rejection (decode_chunk_common.h, reject_code): every kernel re-derives it from seq_len / block_table; the
// prologue raises the sticky status bit and touches no cache row, the attention kernel writes NaN outputs.
// A block_table entry outside the pool on a page that is only READ is replaced by page 0, raises bit 2 and turns
// the workgroup's outputs into NaN.
#include "decode_chunk_geo.h"

namespace sfa {

namespace {

using namespace prefill;

}  // namespace

int launch_decode_chunk(const ChunkKernelParams &p, int dtype, int head_dim, hipStream_t stream) {
    const int row_tiles = (p.R + kBM - 1) / kBM;
    return chunk::launch_chunk<UniformGeo>(p, p.d, dtype, head_dim, dim3(p.n, p.d.B),
                                           dim3(row_tiles, p.d.Hkv * p.d.num_splits, p.d.B),
                                           (long long)p.d.B * p.d.Hkv * p.R, stream);
}

}  // namespace sfa
