"""fp64 reference of sfa_prefill_varlen_split_fwd and the arithmetic of its partition, plan and workspace, for
tests/test_prefill_varlen_split_{cpu,gpu}.py.  Built on tests/prefill_split_ref.py (tiles, chunks, resolved counts) and
tests/prefill_varlen_ref.py (valid sequences, the q-tile plan's bound).

Partition (include/star_flash_attn.h): nkt_max = ceil(max_seqlen_k / 64); a request for S splits resolves as in
sfa_prefill_split_fwd to C = ceil(nkt_max / min(S, nkt_max)) tiles per split and S' = ceil(nkt_max / C) splits.  For q-tile qt
of a sequence with n_q rows and n_k keys, nkt = prefill_split_ref.qtile_tiles(qt, n_q, n_k, causal); split s < S' - 1 owns
the tiles [s C, min((s + 1) C, nkt)), the last split [(S' - 1) C, nkt); a split with s C >= nkt is empty."""
import numpy as np

from prefill_split_ref import QTILE, TILE, qtile_tiles, resolved_splits, tiles_per_split
from prefill_varlen_ref import ENTRY_BYTES, plan_bound, valid_sequences


def partition(max_seqlen_k, num_splits):
    """(C, S') of a request for num_splits >= 1 under the hint max_seqlen_k >= 1"""
    return tiles_per_split(max_seqlen_k, num_splits), resolved_splits(max_seqlen_k, num_splits)


def split_ranges(qt, n_q, n_k, causal, C, S):
    """[(s, first tile, end tile)] of the non-empty splits of q-tile qt: the last split is open-ended"""
    nkt = qtile_tiles(qt, n_q, n_k, causal)
    out = []
    for s in range(S):
        t0, t1 = s * C, (nkt if s == S - 1 else min((s + 1) * C, nkt))
        if t0 < t1:
            out.append((s, t0, t1))
    return out


def plan_slots(cu_q, cu_k, total_q, total_k):
    """[(b, qt)] in the q-tile plan's order: per valid sequence its last q-tile first"""
    out = []
    for b, q0, q1, _, _ in valid_sequences(cu_q, cu_k, total_q, total_k):
        n = -(-(q1 - q0) // QTILE)
        out += [(b, n - 1 - i) for i in range(n)]
    return out


def work_items(cu_q, cu_k, total_q, total_k, causal, C, S):
    """[(slot, split)] the items kernel lists: min(S, ceil(nkt / C)) per slot, in plan order, a slot's splits ascending"""
    out = []
    for slot, (b, qt) in enumerate(plan_slots(cu_q, cu_k, total_q, total_k)):
        n_q, n_k = int(cu_q[b + 1]) - int(cu_q[b]), int(cu_k[b + 1]) - int(cu_k[b])
        cnt = min(S, -(-qtile_tiles(qt, n_q, n_k, causal) // C))
        assert cnt == len(split_ranges(qt, n_q, n_k, causal, C, S))
        out += [(slot, s) for s in range(cnt)]
    return out


def up256(x):
    return -(-x // 256) * 256


def workspace_bytes(batch, heads_q, total_q, head_dim, S):
    """the documented formula for S resolved splits: plan + items + partials, each rounded up to 256 (S == 1: the plan)"""
    bound = plan_bound(batch, total_q)
    plan = up256(ENTRY_BYTES * bound)
    if S <= 1:
        return plan
    return plan + up256(ENTRY_BYTES * bound * S) + up256(4 * (head_dim + 2) * QTILE * bound * heads_q * S)


def prefill_varlen_split_ref(q, k, v, cu_q, cu_k, causal, max_seqlen_k, num_splits, scale=None):
    """q [Tq, Hq, D], k / v [Tk, Hkv, D], cu_q / cu_k integer sequences [B + 1] -> (o [Tq, Hq, D], lse [Hq, Tq], both
    float64, rows [Tq] bool: the packed query rows of valid sequences).  Per valid sequence and q-tile: the row state of
    every non-empty split over exactly its tiles -- m_s the max score in log2 units, l_s = sum 2^(s_j - m_s),
    O_s = sum 2^(s_j - m_s) V_j -- then the merge in ascending s: m = max m_s, l = sum 2^(m_s - m) l_s,
    o = sum 2^(m_s - m) O_s / l, lse = (m + log2 l) ln 2, over the partials with a key.  A row with none gets zeros and
    -inf; rows of no valid sequence hold 0 in both."""
    q, k, v = (np.asarray(x, np.float64) for x in (q, k, v))
    Tq, Hq, D = q.shape
    Tk, Hkv = k.shape[0], k.shape[1]
    g = Hq // Hkv
    c2 = (D ** -0.5 if scale is None else scale) * np.log2(np.e)
    C, S = partition(max_seqlen_k, num_splits)
    o = np.zeros((Tq, Hq, D))
    lse = np.zeros((Hq, Tq))
    rows = np.zeros(Tq, bool)
    for b, q0, q1, k0, k1 in valid_sequences(cu_q, cu_k, Tq, Tk):
        n_q, n_k = q1 - q0, k1 - k0
        if n_q == 0:
            continue
        rows[q0:q1] = True
        lse[:, q0:q1] = -np.inf
        for h in range(Hq):
            sc = (q[q0:q1, h] @ k[k0:k1, h // g].T) * c2
            if causal:
                sc = np.where(np.arange(n_k)[None, :] <= np.arange(n_q)[:, None] + (n_k - n_q), sc, -np.inf)
            for qt in range(-(-n_q // QTILE)):
                r0, r1 = qt * QTILE, min((qt + 1) * QTILE, n_q)
                parts = []
                for _, t0, t1 in split_ranges(qt, n_q, n_k, causal, C, S):
                    blk = sc[r0:r1, t0 * TILE:min(t1 * TILE, n_k)]
                    m = blk.max(axis=1)
                    p = np.where(np.isfinite(m)[:, None], np.exp2(blk - np.where(np.isfinite(m), m, 0.0)[:, None]), 0.0)
                    parts.append((m, p.sum(axis=1), p @ v[k0 + t0 * TILE:k0 + min(t1 * TILE, n_k), h // g]))
                m = np.full(r1 - r0, -np.inf)
                for ms, ls, _ in parts:
                    m = np.where(ls > 0, np.maximum(m, ms), m)
                lt, ot = np.zeros(r1 - r0), np.zeros((r1 - r0, D))
                for ms, ls, Os in parts:
                    w = np.where(ls > 0, np.exp2(np.where(ls > 0, ms, 0.0) - np.where(np.isfinite(m), m, 0.0)), 0.0)
                    lt += w * ls
                    ot += w[:, None] * Os
                has = lt > 0
                o[q0 + r0:q0 + r1, h][has] = ot[has] / lt[has, None]
                lse[h, q0 + r0:q0 + r1][has] = (m[has] + np.log2(lt[has])) * np.log(2.0)
    return o, lse, rows


# ---- the batches of the two test files: name -> (the (n_q, n_k) of each sequence, max_seqlen_k, the requests) ----
LENS = [(1, 65), (300, 300), (0, 5), (5, 0), (257, 520), (300, 100), (64, 1100)]
BATCHES = {
    "T": (LENS, 520, (2, 3, 4, 7, 9, 100)),     # 9 tiles in the hint; the first six sequences within it, the last beyond
    "U128": (LENS, 128, (2, 100)),              # C = 1: the last split carries up to 17 tiles
    "U64": (LENS, 64, (2,)),                    # one tile: resolves to 1, the call forwards
}
HEADS = [(4, 2), (8, 8)]                        # (Hq, Hkv); the second takes the Hq % 8 == 0 slice path
