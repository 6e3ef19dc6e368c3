"""fp64 reference of sfa_prefill_split_fwd: the documented partition of each q-tile's key tiles into splits, per-split
partial softmax states (m, l, O) over exactly those tile ranges, and the combine's merge of them.

Partition (include/star_flash_attn.h): nkt_max = ceil(Sk / 64).  A request for S splits resolves to C = ceil(nkt_max / S)
tiles per split and S' = ceil(nkt_max / C) splits.  Split s of q-tile qt (256 rows) owns the tiles
[s C, min((s + 1) C, nkt(qt))), nkt(qt) = the tiles the q-tile's last row sees."""
import numpy as np

TILE, QTILE = 64, 256


def key_tiles(Sk):
    return -(-Sk // TILE)


def tiles_per_split(Sk, num_splits):
    """C: the uniform chunk length in tiles (Sk >= 1, num_splits >= 1)"""
    nkt = key_tiles(Sk)
    return -(-nkt // min(num_splits, nkt))


def resolved_splits(Sk, num_splits):
    """S': the count a request for num_splits resolves to (1 when there are no keys)"""
    if Sk <= 0:
        return 1
    return -(-key_tiles(Sk) // tiles_per_split(Sk, num_splits))


def qtile_tiles(qt, Sq, Sk, causal):
    """nkt(qt): tiles the last row of q-tile qt sees"""
    if not causal:
        return key_tiles(Sk)
    lim = min(QTILE * (qt + 1), Sq) - 1 + Sk - Sq
    return 0 if lim < 0 else lim // TILE + 1


def split_range(qt, s, Sq, Sk, causal, num_splits):
    """(first tile, end tile) of split s of q-tile qt; first >= end: the split is empty"""
    C = tiles_per_split(Sk, num_splits)
    return s * C, min((s + 1) * C, qtile_tiles(qt, Sq, Sk, causal))


def prefill_split_ref(q, k, v, causal, num_splits, scale=None):
    """q [B, Hq, Sq, D], k / v [B, Hkv, Sk, D] -> (o [B, Hq, Sq, D], lse [B, Hq, Sq]), both float64: per split the row
    state over the split's tiles -- m_s the max score in log2 units, l_s = sum 2^(s_j - m_s), O_s = sum 2^(s_j - m_s) V_j
    -- and then the combine: m = max m_s, l = sum 2^(m_s - m) l_s, o = sum 2^(m_s - m) O_s / l, lse = (m + log2 l) ln 2,
    over the non-empty partials only.  A row with every partial empty gets zeros and -inf."""
    q, k, v = (np.asarray(x, np.float64) for x in (q, k, v))
    B, Hq, Sq, D = q.shape
    Hkv, Sk = k.shape[1], k.shape[2]
    g = Hq // Hkv
    c2 = (D ** -0.5 if scale is None else scale) * np.log2(np.e)
    S = resolved_splits(Sk, num_splits)
    o = np.zeros((B, Hq, Sq, D))
    lse = np.full((B, Hq, Sq), -np.inf)
    rows = np.arange(Sq)
    for b in range(B):
        for h in range(Hq):
            sc = (q[b, h] @ k[b, h // g].T) * c2
            if causal:
                sc = np.where(np.arange(Sk)[None, :] <= rows[:, None] + (Sk - Sq), sc, -np.inf)
            for qt in range(-(-Sq // QTILE)):
                r0, r1 = qt * QTILE, min((qt + 1) * QTILE, Sq)
                parts = []
                for s in range(S):
                    t0, t1 = split_range(qt, s, Sq, Sk, causal, num_splits)
                    if t0 >= t1:
                        continue
                    blk = sc[r0:r1, t0 * TILE:min(t1 * TILE, Sk)]
                    m = blk.max(axis=1)
                    p = np.where(np.isfinite(m)[:, None], np.exp2(blk - np.where(np.isfinite(m), m, 0.0)[:, None]), 0.0)
                    parts.append((m, p.sum(axis=1), p @ v[b, h // g, t0 * TILE:min(t1 * TILE, Sk)]))
                m = np.full(r1 - r0, -np.inf)
                for ms, ls, _ in parts:
                    m = np.where(ls > 0, np.maximum(m, ms), m)
                lt, ot = np.zeros(r1 - r0), np.zeros((r1 - r0, D))
                for ms, ls, Os in parts:
                    w = np.where(ls > 0, np.exp2(np.where(ls > 0, ms, 0.0) - np.where(np.isfinite(m), m, 0.0)), 0.0)
                    lt += w * ls
                    ot += w[:, None] * Os
                has = lt > 0
                o[b, h, r0:r1][has] = ot[has] / lt[has, None]
                lse[b, h, r0:r1][has] = (m[has] + np.log2(lt[has])) * np.log(2.0)
    return o, lse
