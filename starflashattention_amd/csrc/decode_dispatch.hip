// Picks the attention kernel of sfa_decode, decides its cache-load policy and adds the split combine.  c_api.hip has
// validated the call: dtype is fp16 / bf16, head_dim is 64 / 128 / 256, num_heads / num_heads_kv is 1, 2, 4, 8 or 16.
//   one query head per kv head: decode_kernel.hip, one workgroup per (batch, head, split).
//   grouped queries: one workgroup per (batch, kv head, split) serves the whole group, so the cache is read once.
//     decode_gqa_kernel.hip (VALU, groups of 2 / 4 / 8) is about as busy as HBM at 4 query heads per kv head and
//     VALU-bound at 8 (4.1 TB/s at head_dim 128), so decode_gqa_mfma_kernel.hip (matrix cores, groups of 4 / 8 / 16)
//     takes over -- for groups of 16 always, for 8 at any head_dim, for 4 at head_dim 128 (measured there: DESIGN.md 5.1,
//     BASELINE.md "grouped-query decode"; bench.py's decode_gqa figures).  sfa_debug_set("decode_gqa_mfma", 0) keeps
//     the VALU kernel for A/B, 1 forces the matrix-core kernel for groups of 4.
//   Cache loads: the cache rows are read exactly once per call.  When the two caches together do not fit the 256 MB
//     Infinity Cache nothing of them survives until the next token's call either, so they are loaded non-temporally
//     (BASELINE config 4: 6.30 -> 6.51 TB/s); a small cache keeps the default policy and is re-read from the Infinity
//     Cache / L2.  sfa_debug_set("decode_nt", 0 / 1) overrides (tests, A/B).
//   num_splits > 1: every attention kernel leaves fp32 partials and decode_combine_kernel (decode_kernel.hip) merges them.
#include "sfa_host.h"

namespace sfa {

bool decode_nt(const DecodeKernelParams &p, int head_dim, int elem_bytes) {
    if (const int k = g_knobs.decode_nt.load(std::memory_order_relaxed); k >= 0) return k != 0;
    return 2ll * elem_bytes * p.B * p.L * p.M * p.Hkv * head_dim > (256ll << 20);
}

int launch_decode(const DecodeKernelParams &p, int dtype, int head_dim, hipStream_t stream) {
    const bool nt = decode_nt(p, head_dim, 2);

    const int group = p.H / p.Hkv;
    const int knob = g_knobs.decode_gqa_mfma.load(std::memory_order_relaxed);
    const bool mfma = group == 16 || (group >= 4 && (knob < 0 ? head_dim == 128 || group == 8 : knob != 0));
    const int rc = group == 1 ? launch_decode_mha(p, dtype, head_dim, nt, stream)
                   : mfma     ? launch_decode_gqa_mfma(p, dtype, head_dim, nt, stream)
                              : launch_decode_gqa(p, dtype, head_dim, nt, stream);
    if (rc != SFA_OK || p.num_splits <= 1) return rc;
    return launch_decode_combine(p, dtype, head_dim, stream);
}

}  // namespace sfa
