"""References of sfa_decode_window_sinks / sfa_decode_chunk_window_sinks / sfa_decode_varlen_window_sinks for
tests/test_decode_sinks_{cpu,gpu}.py: window_ref.decode_window_ref and chunk_window_ref.chunk_window_ref with `sinks`, adapters
over tests/serving_model.py like those.

An attention sink is one more key of every softmax of query head h, with logit sinks[h] (natural-log units, NOT
multiplied by the softmax scale) and a zero value row:

    o[h] = sum_j exp(s_j) V_j / (exp(sinks[h]) + sum_j exp(s_j)),   j over the row's window [lo, pos]

With every sink -inf (or sinks None) the model performs the operations of the call without sinks and returns the same
numbers, exactly.  Each reference also returns the row's log-sum-exp WITHOUT the sink, from which the tests build sinks of a
known weight:

    sinks[h] = lse[anchor, h] + delta_h   =>   the sink's share of the anchor row's softmax is sigmoid(delta_h)

The problem builders, layout converters and TOL of window_ref.py / chunk_window_ref.py are reused by import.
"""
import numpy as np

from window_ref import TOL, decode_window_model, window_lo  # noqa: F401
from chunk_window_ref import chunk_window_model

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


def decode_window_sinks_ref(q, k, v, k_cache, v_cache, seq_len, idx_layer, rot_dim, window, sinks, dtype="fp16",
                            q_bias=None, k_bias=None, v_bias=None, cos_table=None, sin_table=None, scale=None):
    """window_ref.decode_window_ref with sinks [H] (None = all -inf).  Returns dict(o [B, H, D] float32 unrounded,
    k_row, v_row [B, Hkv, D] float32, lse [B, H] float64 = log sum_j exp(s_j) over [lo, pos], without the sink, o64 = o
    before it is rounded to float32)."""
    return decode_window_model(q, k, v, k_cache, v_cache, seq_len, idx_layer, rot_dim, window, sinks, dtype, q_bias, k_bias,
                               v_bias, cos_table, sin_table, scale)


def chunk_sinks_ref(prob, window, sinks, scale=None):
    """chunk_window_ref.chunk_window_ref with sinks [H] (None = all -inf); prob.ns may be ragged, which makes this the
    reference of the varlen call as well.  Returns per sequence b (o [n_b, H, D] float32 unrounded, k_rows, v_rows
    [n_b, Hkv, D] float32, lse [n_b, H] float64 without the sink, o in float64)."""
    return chunk_window_model(prob, window, sinks, scale)


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
