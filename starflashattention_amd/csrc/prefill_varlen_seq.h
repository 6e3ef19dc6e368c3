// The packed prefill kernels' view of one sequence and of one work item (prefill_varlen_kernel.hip,
// prefill_varlen_window_kernel.hip).
#pragma once
#include "prefill_common.h"
#include "sfa_host.h"

namespace sfa {

// The row ranges [q0, q1) and [k0, k1) of sequence b; false unless both are ranges inside [0, total).
__device__ __forceinline__ bool varlen_seq(const PrefillVarlenKernelParams &p, int b, int &q0, int &q1, int &k0, int &k1) {
    q0 = p.cu_q[b], q1 = p.cu_q[b + 1], k0 = p.cu_k[b], k1 = p.cu_k[b + 1];
    return q0 >= 0 && q0 <= q1 && q1 <= p.total_q && k0 >= 0 && k0 <= k1 && k1 <= p.total_k;
}

// One workgroup's work: q-tile qt of a sequence of Sq query rows from cq0 and Sk keys from ck0, for query head h.
struct VarlenItem { int h, qt, Sq, Sk, cq0, ck0; };

// blockIdx -> work item: the plan slot on the slow digit, the head slice on the fast one (all of it workgroup-uniform).
// False -- leave, before any barrier, with nothing read and nothing written -- on the plan's empty marker and on a
// sequence that is not a range of the tensors: the kernels are safe for any cu contents.
__device__ __forceinline__ bool varlen_item(const PrefillVarlenKernelParams &p, VarlenItem &it) {
    const int hps = p.Hq / p.slices;            // query heads per slice
    const int rest = blockIdx.x / p.slices;
    it.h = (blockIdx.x % p.slices) * hps + rest % hps;
    const int2 item = p.plan[rest / hps];
    const int b = item.x;
    it.qt = item.y;
    if (b < 0 || b >= p.B) return false;        // the empty marker
    int cq1, ck1;
    if (!varlen_seq(p, b, it.cq0, cq1, it.ck0, ck1)) return false;
    it.Sq = cq1 - it.cq0, it.Sk = ck1 - it.ck0;
    return it.qt >= 0 && it.qt * prefill::kBM < it.Sq;      // (the plan kernel never writes an item that fails this)
}

}  // namespace sfa
