// Ragged multi-token decode step (sfa_decode_varlen) for gfx950 (MI355X): sequence b brings n_b = cu_tokens[b+1] -
// cu_tokens[b] new tokens, packed one after another in qkv / o ([total_tokens, ...]); n_b = 0 takes no part.  One call
// serves a mix of prompt chunks, speculative verification and plain decode.  Each token gets exactly what
// sfa_decode_chunk gives it at pos = seq_len[b]; the kernels are the chunk's (decode_chunk_body.h) under the ragged
// geometry RaggedGeo.
//
// Four launches, ordered by the stream alone:
//   0. varlen_plan_kernel (one workgroup): from cu_tokens, the compact list of (sequence, q-tile) work items of the
//      attention kernel -- ceil(n_b * G / 256) per sequence, the heaviest (last) q-tile of a sequence first -- padded
//      with an empty marker (b = -1) up to the host bound total_tokens * G / 256 + batch_size.  It also raises
//      SFA_ERR_SEQ_LEN_RANGE for a sequence whose cu_tokens range is not inside [0, total_tokens] or runs backwards.
//   1. chunk_prologue_kernel<RaggedGeo>: one workgroup per packed row; the row finds its sequence in cu_tokens by
//      binary search.  The rotated Q goes to the workspace packed over tokens: [Hkv, total_tokens * G, D].
//   2. chunk_attn_kernel<RaggedGeo>: a 1-D grid of bound * Hkv * S workgroups, workgroup i serving plan item
//      i / (Hkv * S) and (kv head, split) i % (Hkv * S); it exits on the marker.  The grid follows the token total, not
//      batch_size * max n_b, and because the plan index is the slow digit every real workgroup is launched before the
//      first empty one (with the plan index on the fast grid axis the empty slots sat between the real ones and a launch
//      of about one workgroup per CU ran 1.4x longer: DESIGN.md 5.7).
//   3. chunk_combine_kernel<RaggedGeo> (num_splits > 1): one thread group per packed query row.
// Nothing here trusts cu_tokens: every kernel re-derives 0 <= cu[b] <= cu[b+1] <= total_tokens for the sequence it
// found, a packed row that belongs to no such sequence touches nothing, and plan items past the bound are dropped.
#include "decode_varlen_geo.h"

namespace sfa {

namespace {

using namespace prefill;

}  // namespace

int launch_decode_varlen(const VarlenKernelParams &vp, int dtype, int head_dim, hipStream_t stream) {
    const DecodeKernelParams &p = vp.c.d;
    hipLaunchKernelGGL(varlen_plan_kernel, dim3(1), dim3(256), 0, stream, vp);
    if (const int rc = check_launch("varlen_plan_kernel")) return rc;
    return chunk::launch_chunk<RaggedGeo>(vp, p, dtype, head_dim, dim3(vp.total),
                                          dim3((unsigned)vp.bound * (unsigned)(p.Hkv * p.num_splits)),
                                          (long long)p.Hkv * vp.rows, stream);
}

}  // namespace sfa
