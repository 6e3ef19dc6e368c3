// sfa_decode_chunk_window_sinks for gfx950 (MI355X): sfa_decode_chunk_window (decode_chunk_window_kernel.hip) with an
// attention sink -- sinks[h] joins the softmax of every row of query head h as one more key with a zero value row, which
// is what n successive sfa_decode_window_sinks calls give.  The three launches, the grids, the workspace and the rejection
// rules are the chunk call's; the kernels are decode_chunk_body.h's under the uniform geometry with the window and the
// sink flags.  Only chunk_attn_kernel's epilogue reads the sink flag (split 0 folds the sink into the row's state before
// either store path: DESIGN.md 5.16); the prologue and combine kernels of this file are the chunk's, instantiated over
// this file's geometry type.
#include "decode_chunk_geo.h"

namespace sfa {

namespace {

using UniformWindowSinkGeo = chunk::WindowSinkGeo<UniformGeo, ChunkWindowSinksKernelParams>;

}  // namespace

int launch_decode_chunk_window_sinks(const ChunkWindowSinksKernelParams &sp, int dtype, int head_dim, hipStream_t stream) {
    const ChunkKernelParams &p = sp.base;
    const int row_tiles = (p.R + prefill::kBM - 1) / prefill::kBM;
    return chunk::launch_chunk<UniformWindowSinkGeo>(sp, p.d, dtype, head_dim, dim3(p.n, p.d.B),
                                                     dim3(row_tiles, p.d.Hkv * p.d.num_splits, p.d.B),
                                                     (long long)p.d.B * p.d.Hkv * p.R, stream);
}

}  // namespace sfa
