"""The reference of sfa_prefill_varlen_fwd (packed sequences of different lengths) and the arithmetic of its plan, for
tests/test_prefill_varlen_{cpu,gpu}.py.

prefill_varlen_ref loops over the valid sequences and calls oracle.sdpa_ref on each one's own rows -- the call's contract
verbatim: sequence b gets what sfa_prefill_fwd gives for batch = 1, seqlen_q = n_q, seqlen_k = n_k on its rows.  A
sequence is valid iff 0 <= cu[b] <= cu[b+1] <= total holds in both cu arrays.
"""
import numpy as np

from oracle import sdpa_ref

QTILE = 256         # query rows of a work item (csrc/prefill_varlen_kernel.hip)
ENTRY_BYTES = 8     # one int2 (sequence, q-tile) per plan slot


def valid_sequences(cu_q, cu_k, total_q, total_k):
    """[(b, q0, q1, k0, k1)] of the sequences whose entries are ranges of the tensors (n_q == 0 included)"""
    out = []
    for b in range(len(cu_q) - 1):
        q0, q1, k0, k1 = int(cu_q[b]), int(cu_q[b + 1]), int(cu_k[b]), int(cu_k[b + 1])
        if 0 <= q0 <= q1 <= total_q and 0 <= k0 <= k1 <= total_k:
            out.append((b, q0, q1, k0, k1))
    return out


def prefill_varlen_ref(q, k, v, cu_q, cu_k, causal, scale=None):
    """q [Tq, Hq, D], k / v [Tk, Hkv, D] numpy, cu_q / cu_k integer sequences [B + 1].  Returns (o [Tq, Hq, D] float32,
    lse [Hq, Tq] float32, rows [Tq] bool: the packed query rows that belong to a valid sequence).  Rows of no valid
    sequence hold 0 in o and lse; a row with no visible key holds 0 and -inf."""
    Tq, Hq, D = q.shape
    Tk = k.shape[0]
    o = np.zeros((Tq, Hq, D), np.float32)
    lse = np.zeros((Hq, Tq), np.float32)
    rows = np.zeros(Tq, bool)
    for b, q0, q1, k0, k1 in valid_sequences(cu_q, cu_k, Tq, Tk):
        if q1 == q0:
            continue
        rows[q0:q1] = True
        if k1 == k0:
            lse[:, q0:q1] = -np.inf
            continue
        ob, lb = sdpa_ref(q[q0:q1].transpose(1, 0, 2)[None], k[k0:k1].transpose(1, 0, 2)[None],
                          v[k0:k1].transpose(1, 0, 2)[None], causal=causal, scale=scale, return_lse=True)
        o[q0:q1] = ob[0].transpose(1, 0, 2)
        lse[:, q0:q1] = lb[0]
    return o, lse, rows


def plan_bound(batch, total_q):
    """plan slots of the call: every sequence with rows has ceil(n / 256) <= n // 256 + 1 q-tiles"""
    return total_q // QTILE + batch


def items(cu_q, cu_k=None, total_q=None, total_k=None):
    """work items the plan kernel emits: ceil(n_q / 256) per valid sequence.  Without cu_k only cu_q is judged."""
    cu_q = [int(x) for x in cu_q]
    total_q = cu_q[-1] if total_q is None else total_q
    if cu_k is None:
        cu_k, total_k = [0] * len(cu_q), 0
    return sum(-(-(q1 - q0) // QTILE) for _, q0, q1, _, _ in valid_sequences(cu_q, cu_k, total_q, total_k))


def cu_of(lengths):
    """[0, n_0, n_0 + n_1, ...] as a list"""
    return [0] + [int(x) for x in np.cumsum(lengths)]
