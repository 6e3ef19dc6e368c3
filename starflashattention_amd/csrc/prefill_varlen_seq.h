// The packed prefill kernels' view of one sequence (prefill_varlen_kernel.hip, prefill_varlen_window_kernel.hip).
#pragma once
#include "sfa_host.h"

namespace sfa {

// The row ranges [q0, q1) and [k0, k1) of sequence b; false unless both are ranges inside [0, total).
__device__ __forceinline__ bool varlen_seq(const PrefillVarlenKernelParams &p, int b, int &q0, int &q1, int &k0, int &k1) {
    q0 = p.cu_q[b], q1 = p.cu_q[b + 1], k0 = p.cu_k[b], k1 = p.cu_k[b + 1];
    return q0 >= 0 && q0 <= q1 && q1 <= p.total_q && k0 >= 0 && k0 <= k1 && k1 <= p.total_k;
}

}  // namespace sfa
