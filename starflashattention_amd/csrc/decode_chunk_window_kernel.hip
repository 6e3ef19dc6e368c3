// sfa_decode_chunk_window for gfx950 (MI355X): sfa_decode_chunk (decode_chunk_kernel.hip) with a sliding window -- token
// t of a sequence at pos = seq_len[b] attends to the rows [max(0, pos + t + 1 - window), pos + t], which is what n
// successive sfa_decode_window calls give.  The three launches, the grids, the workspace and the rejection rules are the
// chunk call's; the kernels are decode_chunk_body.h's under the uniform geometry with the window flag.  Only
// chunk_attn_kernel reads the flag (key range from the window's first tile, lower mask per row, nothing below
// lo_0 = max(0, pos + 1 - window) read in the cache or the block table: DESIGN.md 5.12); the prologue and combine
// kernels of this file are the chunk's, instantiated over this file's geometry type.
#include "decode_chunk_geo.h"

namespace sfa {

namespace {

using UniformWindowGeo = chunk::WindowGeo<UniformGeo, ChunkWindowKernelParams>;

}  // namespace

int launch_decode_chunk_window(const ChunkWindowKernelParams &wp, int dtype, int head_dim, hipStream_t stream) {
    const ChunkKernelParams &p = wp.base;
    const int row_tiles = (p.R + prefill::kBM - 1) / prefill::kBM;
    return chunk::launch_chunk<UniformWindowGeo>(wp, p.d, dtype, head_dim, dim3(p.n, p.d.B),
                                                 dim3(row_tiles, p.d.Hkv * p.d.num_splits, p.d.B),
                                                 (long long)p.d.B * p.d.Hkv * p.R, stream);
}

}  // namespace sfa
