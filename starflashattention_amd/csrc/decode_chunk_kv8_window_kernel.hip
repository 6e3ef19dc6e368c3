// sfa_decode_chunk_kv8_window for gfx950 (MI355X): sfa_decode_chunk_kv8 (decode_chunk_kv8_kernel.hip) with a sliding
// window -- row pos + t receives the bytes sfa_decode_chunk_kv8 stores, and token t attends to the rows
// [max(0, pos + t + 1 - window), pos + t] of the cache after the append: what n successive sfa_decode_kv8_window calls
// give.  The three launches, the grids, the workspace and the rejection rules are the chunk call's; the kernels are
// decode_chunk_body.h's under the uniform geometry with both flags.  The fp8 flag acts in the prologue and on the
// staging and the scales of chunk_attn_kernel, the window flag on its key range, lower mask and row clamps; nothing
// below lo_0 = max(0, pos + 1 - window) is read in the cache or the block table, which over bytes that may be 0x7F
// (NaN) is what keeps the output finite.  The combine kernel of this file is the chunk's, instantiated
// over this file's geometry type.
#include "decode_chunk_geo.h"

namespace sfa {

namespace {

using UniformKv8WindowGeo = chunk::Kv8WindowGeo<UniformGeo, ChunkKv8WindowKernelParams>;

}  // namespace

int launch_decode_chunk_kv8_window(const ChunkKv8WindowKernelParams &kp, int dtype, int head_dim, hipStream_t stream) {
    const ChunkKernelParams &p = kp.base;
    const int row_tiles = (p.R + prefill::kBM - 1) / prefill::kBM;
    return chunk::launch_chunk<UniformKv8WindowGeo>(kp, p.d, dtype, head_dim, dim3(p.n, p.d.B),
                                                    dim3(row_tiles, p.d.Hkv * p.d.num_splits, p.d.B),
                                                    (long long)p.d.B * p.d.Hkv * p.R, stream);
}

}  // namespace sfa
