// sfa_decode_varlen_kv8_window_sinks for gfx950 (MI355X): sfa_decode_varlen_kv8_window
// (decode_varlen_kv8_window_kernel.hip) with an attention sink -- each token gets exactly what
// sfa_decode_chunk_kv8_window_sinks gives it at pos = seq_len[b].  The plan kernel, the four launches, the grids and the
// workspace are the ragged call's; the kernels are decode_chunk_body.h's under the ragged geometry with the fp8, window
// and sink flags, the last read by chunk_attn_kernel's epilogue alone (decode_chunk_kv8_window_sinks_kernel.hip,
// DESIGN.md 5.17).
#include "decode_varlen_geo.h"

namespace sfa {

namespace {

using RaggedKv8WindowSinkGeo = chunk::Kv8WindowSinkGeo<RaggedGeo, VarlenKv8WindowSinksKernelParams>;

}  // namespace

int launch_decode_varlen_kv8_window_sinks(const VarlenKv8WindowSinksKernelParams &sp, int dtype, int head_dim,
                                          hipStream_t stream) {
    const VarlenKernelParams &vp = sp.base;
    const DecodeKernelParams &p = vp.c.d;
    hipLaunchKernelGGL(varlen_plan_kernel, dim3(1), dim3(256), 0, stream, vp);
    if (const int rc = check_launch("varlen_plan_kernel")) return rc;
    return chunk::launch_chunk<RaggedKv8WindowSinkGeo>(sp, p, dtype, head_dim, dim3(vp.total),
                                                       dim3((unsigned)vp.bound * (unsigned)(p.Hkv * p.num_splits)),
                                                       (long long)p.Hkv * vp.rows, stream);
}

}  // namespace sfa
