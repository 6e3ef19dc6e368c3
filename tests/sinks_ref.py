"""fp64 references of sfa_decode_window_sinks / sfa_decode_chunk_window_sinks / sfa_decode_varlen_window_sinks for
tests/test_decode_sinks_{cpu,gpu}.py.

An attention sink is one more key of every softmax of query head h, with logit sinks[h] (natural-log units, NOT
multiplied by the softmax scale) and a zero value row:

    o[h] = sum_j exp(s_j) V_j / (exp(sinks[h]) + sum_j exp(s_j)),   j over the row's window [lo, pos]

The prologue (rotated q, the k / v rows the call stores) is taken exactly as window_ref.decode_window_ref and
chunk_window_ref.chunk_window_ref take it, and the attention is theirs with the sink column added: with every sink -inf
the functions here perform the same floating-point operations as those and return the same numbers, exactly.  Each
reference also returns the row's log-sum-exp WITHOUT the sink, from which the tests build sinks of a known weight:

    sinks[h] = lse[anchor, h] + delta_h   =>   the sink's share of the anchor row's softmax is sigmoid(delta_h)

The problem builders, layout converters and TOL of window_ref.py / chunk_window_ref.py are reused by import.
"""
import numpy as np

from oracle import decode_ref, rope_interleaved, round_to
from window_ref import TOL, window_lo  # noqa: F401
from chunk_window_ref import HKV as _HKV, LAYER, rotary_tables

DELTA_LO, DELTA_HI = -3.0, 3.0                  # sigmoid: 0.047 .. 0.953


def deltas(H):
    """a different, material sink weight for every head"""
    return np.linspace(DELTA_LO, DELTA_HI, H)


def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-np.asarray(x, np.float64)))


def make_sinks(lse_anchor, delta=None):
    """lse_anchor [H] (float64, one row's log-sum-exp per head) -> sinks [H] float64; the device gets them as float32"""
    lse_anchor = np.asarray(lse_anchor, np.float64)
    return lse_anchor + (deltas(lse_anchor.shape[0]) if delta is None else delta)


def _sink_f64(sinks, H):
    s = np.full(H, -np.inf) if sinks is None else np.asarray(sinks, np.float64)
    assert s.shape == (H,)
    return s


def decode_window_sinks_ref(q, k, v, k_cache, v_cache, seq_len, idx_layer, rot_dim, window, sinks, dtype="fp16",
                            q_bias=None, k_bias=None, v_bias=None, cos_table=None, sin_table=None, scale=None):
    """window_ref.decode_window_ref with sinks [H] (None = all -inf).  Returns dict(o [B, H, D] float32 unrounded,
    k_row, v_row [B, Hkv, D] float32, lse [B, H] float64 = log sum_j exp(s_j) over [lo, pos], without the sink, o64 = o
    before it is rounded to float32)."""
    q, k, v = (np.asarray(x, np.float32) for x in (q, k, v))
    B, H, D = q.shape
    Hkv = k.shape[1]
    G = H // Hkv
    assert G * Hkv == H
    if scale is None:
        scale = 1.0 / np.sqrt(float(D))
    sk = _sink_f64(sinks, H).reshape(Hkv, G, 1)
    rep = lambda x: None if x is None else np.repeat(np.asarray(x, np.float32), G, axis=0)
    o = np.zeros((B, H, D), np.float64)
    lse = np.zeros((B, H), np.float64)
    k_rows = np.zeros((B, Hkv, D), np.float32)
    v_rows = np.zeros((B, Hkv, D), np.float32)
    for b in range(B):
        pos = int(seq_len[b])
        qkv_x = np.stack([q[b], np.repeat(k[b], G, axis=0), np.repeat(v[b], G, axis=0)])[None]
        dummy_k = np.zeros((1, 1, pos + 1, H, D), np.float32)
        pro = decode_ref(qkv_x, dummy_k, np.zeros_like(dummy_k), [pos], 0, rot_dim, dtype=dtype, q_bias=q_bias,
                         k_bias=rep(k_bias), v_bias=rep(v_bias), cos_table=cos_table, sin_table=sin_table)
        k_rows[b], v_rows[b] = pro["k_row"][0, ::G], pro["v_row"][0, ::G]
        lo = window_lo(pos, window)
        K = np.concatenate([np.asarray(k_cache[b, idx_layer, lo:pos], np.float64), k_rows[b][None].astype(np.float64)])
        V = np.concatenate([np.asarray(v_cache[b, idx_layer, lo:pos], np.float64), v_rows[b][None].astype(np.float64)])
        qr = pro["q_rot"][0].astype(np.float64).reshape(Hkv, G, D)
        sc = np.einsum("kgd,tkd->kgt", qr, K) * scale
        m0 = sc.max(axis=2, keepdims=True)
        lse[b] = (m0 + np.log(np.exp(sc - m0).sum(axis=2, keepdims=True))).reshape(H)
        mx = np.maximum(m0, sk)
        sc -= mx
        p = np.exp(sc)
        p /= p.sum(axis=2, keepdims=True) + np.exp(sk - mx)
        o[b] = np.einsum("kgt,tkd->kgd", p, V).reshape(H, D)
    return dict(o=o.astype(np.float32), k_row=k_rows, v_row=v_rows, lse=lse, o64=o)


def chunk_sinks_ref(prob, window, sinks, scale=None):
    """chunk_window_ref.chunk_window_ref with sinks [H] (None = all -inf); prob.ns may be ragged, which makes this the
    reference of the varlen call as well.  Returns per sequence b (o [n_b, H, D] float32 unrounded, k_rows, v_rows
    [n_b, Hkv, D] float32, lse [n_b, H] float64 without the sink, o in float64)."""
    HKV = getattr(prob, "Hkv", _HKV)            # (a problem built by hand may have another kv-head count)
    D, G, H = prob.D, prob.G, prob.G * HKV
    if scale is None:
        scale = 1.0 / np.sqrt(float(D))
    sk = _sink_f64(sinks, H).reshape(HKV, G, 1, 1)
    f64 = lambda x: None if x is None else x.float().numpy().astype(np.float64)
    qb, kb, vb = f64(prob.qb), f64(prob.kb), f64(prob.vb)
    out = []
    for b, (pos, n) in enumerate(zip(prob.lens, prob.ns)):
        x = prob.qkv[b][:n].float().numpy().astype(np.float64)              # [n, H + 2 Hkv, D]
        q, k, v = x[:, :H], x[:, H:H + HKV], x[:, H + HKV:]
        if qb is not None:
            q, k, v = q + qb, k + kb, v + vb
        qr = np.empty_like(q)
        kr = np.empty_like(k)
        for t in range(n):
            c = s = None
            if prob.tables and prob.rot > 0:
                cos, sin = rotary_tables(prob.dtype, prob.rot)
                c, s = cos[pos + t], sin[pos + t]
            qr[t] = rope_interleaved(q[t], pos + t, prob.rot, cos=c, sin=s)
            kr[t] = rope_interleaved(k[t], pos + t, prob.rot, cos=c, sin=s)
        qr = round_to(qr, prob.dtype).astype(np.float64)
        k_rows, v_rows = round_to(kr, prob.dtype).astype(np.float32), round_to(v, prob.dtype).astype(np.float32)
        if n == 0:
            out.append((np.zeros((0, H, D), np.float32), k_rows, v_rows, np.zeros((0, H), np.float64),
                        np.zeros((0, H, D), np.float64)))
            continue
        lo0 = window_lo(pos, window)
        K = np.concatenate([prob.kf[b, LAYER, lo0:pos].astype(np.float64), k_rows.astype(np.float64)])    # rows lo0 ..
        V = np.concatenate([prob.vf[b, LAYER, lo0:pos].astype(np.float64), v_rows.astype(np.float64)])
        j = lo0 + np.arange(K.shape[0])
        t = np.arange(n)
        lo_t = np.array([window_lo(pos + int(tt), window) for tt in t])
        vis = (j[None, :] >= lo_t[:, None]) & (j[None, :] <= pos + t[:, None])                            # [n, keys]
        q2 = qr.reshape(n, HKV, G, D).transpose(1, 2, 0, 3).reshape(HKV, G * n, D)
        sc = np.matmul(q2, K.transpose(1, 2, 0)).reshape(HKV, G, n, -1) * scale                             # [k, g, t, j]
        sc = np.where(vis[None, None], sc, -np.inf)
        m0 = sc.max(axis=3, keepdims=True)
        lse = (m0 + np.log(np.exp(sc - m0).sum(axis=3, keepdims=True))).reshape(H, n).T                    # [t, h]
        mx = np.maximum(m0, sk)
        sc -= mx
        p = np.exp(sc)
        p /= p.sum(axis=3, keepdims=True) + np.exp(sk - mx)
        o = np.matmul(p.reshape(HKV, G * n, -1), V.transpose(1, 0, 2)).reshape(HKV, G, n, D).transpose(2, 0, 1, 3).reshape(n, H, D)
        out.append((o.astype(np.float32), k_rows, v_rows, lse, o))
    return out


varlen_sinks_ref = chunk_sinks_ref              # the packed call gives each token what the chunk call gives it


class WithSinks:
    """The package `sfa` with the three windowed operators replaced by their _sinks twins at fixed `sinks` (a float32
    device tensor [H], or None = NULL): the run() harnesses of the window tests then drive the sinks calls as they are."""

    def __init__(self, sfa, sinks, **extra):
        self._sfa, self._sinks, self._extra = sfa, sinks, extra     # extra: keyword arguments added to every call

    def __getattr__(self, name):
        return getattr(self._sfa, name)

    def flash_decode_window(self, *args, **kw):
        return self._sfa.flash_decode_window_sinks(*args, self._sinks, **{**kw, **self._extra})

    def flash_decode_chunk_window(self, *args, **kw):
        return self._sfa.flash_decode_chunk_window_sinks(*args, self._sinks, **{**kw, **self._extra})

    def flash_decode_varlen_window(self, *args, **kw):
        return self._sfa.flash_decode_varlen_window_sinks(*args, self._sinks, **{**kw, **self._extra})
