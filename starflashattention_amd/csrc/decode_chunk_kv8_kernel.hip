// sfa_decode_chunk_kv8 for gfx950 (MI355X): sfa_decode_chunk (decode_chunk_kernel.hip) over an fp8 (e4m3) KV cache with a
// scale per kv head -- row pos + t receives q8(k16 / k_scale[hk]) and q8(v16 / v_scale[hk]), k16 / v16 being what the
// 16-bit call stores, and token t attends to the rows [0, pos + t] of the cache after the append, its own row and the
// other new rows through their quantised values: what n successive sfa_decode_kv8 calls give.  The three launches, the
// grids, the workspace and the rejection rules are the chunk call's; the kernels are decode_chunk_body.h's under the
// uniform geometry with the fp8 flag (byte stores in the prologue, byte staging and conversion into the 16-bit LDS tiles
// and the two scales in the attention kernel: DESIGN.md 5.14).  The combine kernel of this file is the chunk's,
// instantiated over this file's geometry type.
#include "decode_chunk_geo.h"

namespace sfa {

namespace {

using UniformKv8Geo = chunk::Kv8Geo<UniformGeo, ChunkKv8KernelParams>;

}  // namespace

int launch_decode_chunk_kv8(const ChunkKv8KernelParams &kp, int dtype, int head_dim, hipStream_t stream) {
    const ChunkKernelParams &p = kp.base;
    const int row_tiles = (p.R + prefill::kBM - 1) / prefill::kBM;
    return chunk::launch_chunk<UniformKv8Geo>(kp, p.d, dtype, head_dim, dim3(p.n, p.d.B),
                                              dim3(row_tiles, p.d.Hkv * p.d.num_splits, p.d.B),
                                              (long long)p.d.B * p.d.Hkv * p.R, stream);
}

}  // namespace sfa
