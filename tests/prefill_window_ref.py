"""fp64 reference of sfa_prefill_window_fwd for tests/test_prefill_window_{cpu,gpu}.py.

Row i of a [B, Hq, Sq, D] query with causal limit lim_i = i + (Sk - Sq) sees the keys [lo_i, lim_i],
lo_i = max(0, lim_i + 1 - window), and its softmax counts one more element with logit sinks[h] (natural-log units, NOT
multiplied by the scale) and a zero value row:

    o   = sum_j exp(s_j) V_j / (exp(sinks[h]) + sum_j exp(s_j))
    lse = log(exp(sinks[h]) + sum_j exp(s_j))

A row with no visible key gets zeros and lse = -inf, sink or not: the sink joins only a softmax that has a key.

With sinks=None and window >= Sk the function performs the floating-point operations of
oracle.sdpa_ref(causal=True, return_lse=True), in its order, and returns the same numbers exactly: the lower mask hides
nothing and the sink term is never formed.
"""
import numpy as np


def window_mask(Sq, Sk, window):
    """[Sq, Sk] bool: key j visible to row i"""
    i = np.arange(Sq)[:, None]
    j = np.arange(Sk)[None, :]
    lim = i + (Sk - Sq)
    return (j <= lim) & (j >= lim + 1 - int(window))


def prefill_window_ref(q, k, v, window, sinks=None, scale=None):
    """q [B,Hq,Sq,D], k/v [B,Hkv,Sk,D] float, window int >= 1, sinks None or [Hq] -> (o [B,Hq,Sq,D] float32,
    lse [B,Hq,Sq] float32), fp64 math.  GQA: query head h reads kv head h // (Hq//Hkv)."""
    q = np.asarray(q, dtype=np.float64)
    k = np.asarray(k, dtype=np.float64)
    v = np.asarray(v, dtype=np.float64)
    B, Hq, Sq, D = q.shape
    Hkv, Sk = k.shape[1], k.shape[2]
    assert Hq % Hkv == 0 and int(window) >= 1
    g = Hq // Hkv
    if scale is None:
        scale = 1.0 / np.sqrt(float(D))
    if sinks is not None:
        sinks = np.asarray(sinks, dtype=np.float64)
        assert sinks.shape == (Hq,)
    o = np.zeros((B, Hq, Sq, D), dtype=np.float64)
    lse = np.full((B, Hq, Sq), -np.inf, dtype=np.float64)
    mask = window_mask(Sq, Sk, window)
    for b in range(B):
        for h in range(Hq):
            s = (q[b, h] @ k[b, h // g].T) * scale
            s = np.where(mask, s, -np.inf)
            m = s.max(axis=1, keepdims=True)
            has = np.isfinite(m)                    # the row has a visible key
            if sinks is not None:
                m = np.where(has, np.maximum(m, sinks[h]), m)
            m = np.where(np.isfinite(m), m, 0.0)
            p = np.exp(s - m)
            l = p.sum(axis=1, keepdims=True)
            pv = p @ v[b, h // g]
            if sinks is not None:
                l = l + np.where(has, np.exp(sinks[h] - m), 0.0)
            safe = np.where(l > 0, l, 1.0)
            o[b, h] = pv / safe
            with np.errstate(divide="ignore"):
                lse[b, h] = (m + np.log(l))[:, 0]
    return o.astype(np.float32), lse.astype(np.float32)


def visible_counts(Sq, Sk, window):
    """[Sq] keys each row sees"""
    return window_mask(Sq, Sk, window).sum(axis=1)
