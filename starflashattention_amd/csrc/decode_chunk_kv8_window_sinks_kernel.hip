// sfa_decode_chunk_kv8_window_sinks for gfx950 (MI355X): sfa_decode_chunk_kv8_window (decode_chunk_kv8_window_kernel.hip)
// with an attention sink -- sinks[h] joins the softmax of every row of query head h as one more key with a zero value
// row, scaled neither by head_dim_inv nor by k_scale, which is what n successive sfa_decode_kv8_window_sinks calls give.
// The three launches, the grids, the workspace and the rejection rules are the chunk call's; the kernels are
// decode_chunk_body.h's under the uniform geometry with the fp8, window and sink flags.  The fp8 flag acts in the
// prologue and on the staging and the scales of chunk_attn_kernel, the window flag on its key range, lower mask and row
// clamps, the sink flag in its epilogue alone: split 0 folds the sink into the row's state -- whose maximum carries
// k_scale already -- before the bad-page NaN and before v_scale on either store path.  The prologue and
// combine kernels of this file are the fp8 chunk's, instantiated over this file's geometry type.
#include "decode_chunk_geo.h"

namespace sfa {

namespace {

using UniformKv8WindowSinkGeo = chunk::Kv8WindowSinkGeo<UniformGeo, ChunkKv8WindowSinksKernelParams>;

}  // namespace

int launch_decode_chunk_kv8_window_sinks(const ChunkKv8WindowSinksKernelParams &sp, int dtype, int head_dim,
                                         hipStream_t stream) {
    const ChunkKernelParams &p = sp.base;
    const int row_tiles = (p.R + prefill::kBM - 1) / prefill::kBM;
    return chunk::launch_chunk<UniformKv8WindowSinkGeo>(sp, p.d, dtype, head_dim, dim3(p.n, p.d.B),
                                                        dim3(row_tiles, p.d.Hkv * p.d.num_splits, p.d.B),
                                                        (long long)p.d.B * p.d.Hkv * p.R, stream);
}

}  // namespace sfa
