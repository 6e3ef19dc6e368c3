"""References of sfa_decode_kv8_window_sinks / sfa_decode_chunk_kv8_window_sinks / sfa_decode_varlen_kv8_window_sinks
(attention sinks in the three windowed decode calls over an fp8 e4m3 KV cache) for tests/test_decode_kv8_sinks_{cpu,gpu}.py.

An attention sink is one more key of every softmax of query head h, with logit sinks[h] (natural-log units, multiplied
NEITHER by the softmax scale NOR by k_scale) and a zero value row.  With s_j = q16 . (k_scale[hk] K8_j) * scale over the
row's key range [lo, pos]:

    o[h] = v_scale[hk] sum_j exp(s_j) V8_j / (exp(sinks[h]) + sum_j exp(s_j))

The functions here are adapters over tests/serving_model.py, which holds this arithmetic, as kv8_window_ref.
decode_kv8_window_ref and chunk_kv8_window_ref.chunk_kv8_window_ref are: with every sink -inf (or sinks None) the model
performs the operations of the call without sinks and returns the same numbers, exactly.  Each reference also returns the
row's log-sum-exp WITHOUT the sink, from which the tests build sinks of a known weight (sinks_ref.make_sinks):

    sinks[h] = lse[anchor, h] + delta_h   =>   the sink's share of the anchor row's softmax is sigmoid(delta_h)

How the device is checked is how the twins are checked: (a) the appended bytes against the reference quantiser, by the
twins' own rules (chunk_kv8_ref.check_bytes; the single-token rules of tests/test_decode_kv8_window_gpu.py), (b) o against
attend_sinks() over the bytes the device stored, at window_ref.TOL.  The frames, problems, layouts and run() harnesses of
kv8_window_ref.py / chunk_kv8_window_ref.py are reused by import; WithSinks makes those harnesses drive the sinks calls.
"""
import functools

import numpy as np

import chunk_kv8_ref as ckr
import chunk_kv8_window_ref as ckw
import kv8_ref
import kv8_window_ref as kwr
from sinks_ref import deltas, make_sinks, sigmoid  # noqa: F401  (re-exported for the two test files)
from window_ref import TOL, window_lo  # noqa: F401

B, HKV, L, M, LAYER, LENS = ckw.B, ckw.HKV, ckw.L, ckw.M, ckw.LAYER, ckw.LENS
assert (kwr.B, kwr.HKV, kwr.L, kwr.M, kwr.LAYER, kwr.LENS) == (B, HKV, L, M, LAYER, LENS)


def attend_sinks(q16, k8, v8, pos, window, sinks, k_scale=None, v_scale=None, scale=None):
    """chunk_kv8_window_ref.attend with a sink column: q16 [n, H, D] float64 rotated, rounded queries of the tokens at
    pos .. pos + n - 1 of one sequence; k8 / v8 [M, Hkv, D] uint8, one (sequence, layer) of the cache after the append;
    sinks [H] (None = all -inf).  Returns (o [n, H, D] float64, lse [n, H] float64 = log sum_j exp(s_j) over the row's
    key range, without the sink)."""
    return ckr.attend_bytes(q16, k8, v8, pos, window, sinks, k_scale, v_scale, scale)


def decode_kv8_sinks_ref(qkv, k8, v8, seq_len, idx_layer, rot_dim, dtype, window, sinks, k_scale=None, v_scale=None,
                         q_bias=None, k_bias=None, v_bias=None, cos_table=None, sin_table=None, scale=None):
    """kv8_window_ref.decode_kv8_window_ref with sinks [H] (None = all -inf); k8 / v8 are MUTATED at the appended rows.
    Returns its dict (o float32, unrounded) plus o64, lse [B, H] float64 without the sink and q16 [B, H, D] float64 = the
    rotated, rounded queries."""
    return kv8_ref.decode_kv8_model(qkv, k8, v8, seq_len, idx_layer, rot_dim, dtype, window, sinks, k_scale, v_scale, q_bias,
                                    k_bias, v_bias, cos_table, sin_table, scale)


def chunk_kv8_sinks_ref(p, window, sinks, lens=None, base=None):
    """chunk_kv8_window_ref.reference(p, window) with sinks [H] (None = all -inf); p.ns may be ragged, which makes this the
    reference of the varlen call as well.  Returns (dict(o, q16, lse = per sequence [n_b, H] float64 without the sink), k8
    after, v8 after).  base: reference(p, window, lens) when the caller has it already."""
    ref, k_ref, v_ref = ckw.reference(p, window, lens) if base is None else base
    lens = p.lens if lens is None else lens
    o, lse = [], []
    for b, q16 in enumerate(ref["q16"]):
        ob, lb = attend_sinks(q16, k_ref[b, LAYER], v_ref[b, LAYER], int(lens[b]), window, sinks, p.ks, p.vs, p.scale)
        o.append(ob)
        lse.append(lb)
    return dict(o=o, q16=ref["q16"], lse=lse), k_ref, v_ref


varlen_kv8_sinks_ref = chunk_kv8_sinks_ref      # the packed call gives each token what the chunk call gives it


def anchor_sinks(p, window, anchor, shift=None, base=None, token=0):
    """float32 sinks [H] = the log-sum-exp of token `token` of sequence `anchor` (without a sink) + delta (None:
    linspace(-3, 3, H); a number: that delta for every head)"""
    ref, k_ref, v_ref = ckw.reference(p, window) if base is None else base
    q16 = ref["q16"][anchor][token:token + 1]
    _, lse = attend_sinks(q16, k_ref[anchor, LAYER], v_ref[anchor, LAYER], int(p.lens[anchor]) + token, window, None, p.ks,
                          p.vs, p.scale)
    return make_sinks(lse[0], shift).astype(np.float32)


# ---- the frames' references: made once, never modified.  The sinks the device gets are the float32 roundings, and the
# ---- references are computed from those ------------------------------------------------------------------------------------

def _single_args(dtype, D, G, tables, k_factors):
    t, c = kwr.tokens(dtype, D, G), kwr.caches(D, k_factors)
    cos, sin = kwr.rotary_tables(dtype, t.rot) if tables else (None, None)
    return t, c, dict(q_bias=t.qb, k_bias=t.kb, v_bias=t.vb, cos_table=cos, sin_table=sin)


def single_with(dtype, D, G, window, sinks, tables=False, scale=None, k_factors=(1.0, 1.0)):
    """decode_kv8_sinks_ref on the single-token frame with the given sinks; adds k8 / v8 = the caches after the step"""
    t, c, kw = _single_args(dtype, D, G, tables, k_factors)
    k8, v8 = c.k8.copy(), c.v8.copy()
    ref = decode_kv8_sinks_ref(t.qkv, k8, v8, LENS, LAYER, t.rot, dtype, window, sinks, c.ks, c.vs, scale=scale, **kw)
    return dict(ref, k8=k8, v8=v8)


@functools.lru_cache(maxsize=None)
def single_ref(dtype, D, G, window, tables=False, anchor=None, shift=None, scale=None, k_factors=(1.0, 1.0)):
    """(sinks float32 [H] or None, the reference): anchor None = no sink (every sink -inf)"""
    if anchor is None:
        return None, single_with(dtype, D, G, window, None, tables, scale, k_factors)
    lse = single_ref(dtype, D, G, window, tables, scale=scale, k_factors=k_factors)[1]["lse"][anchor]
    sinks = make_sinks(lse, shift).astype(np.float32)
    return sinks, single_with(dtype, D, G, window, sinks, tables, scale, k_factors)


@functools.lru_cache(maxsize=None)
def chunk_ref(dtype, D, G, n, window, tables=False, anchor=None, shift=None):
    """(sinks float32 [H] or None, (ref, k8 after, v8 after)) on chunk_kv8_window_ref.problem; the anchor row is token 0
    of sequence `anchor`"""
    p = ckw.problem(dtype, D, G, n, tables)
    base = ckw.frame_reference(dtype, D, G, n, window, tables)
    sinks = None if anchor is None else anchor_sinks(p, window, anchor, shift, base)
    return sinks, chunk_kv8_sinks_ref(p, window, sinks, base=base)


# ---- problems the CPU and the GPU file share: the bars the GPU tests lean on are asserted on the references alone --------

# "the sink binds": a window of 4 rows keeps |o| of the order of a V row, so that half of it is many tolerances
BINDS = dict(D=128, G=4, n=8, window=4, anchor=2)

# "the sink is unscaled": Hkv = 2, G = 8, k_scale / v_scale factors (0.5, 2) per kv head -- four distinct scales
SCALED = dict(dtype="bf16", D=64, G=8, n=5, window=4, anchor=2, k_factors=(0.5, 2.0))


def wrongly_scaled(sinks, ks, D, G):
    """the sinks a kernel that multiplied them by k_scale[hk], or by head_dim_inv, would in effect use"""
    return {"k_scale": sinks * np.repeat(np.asarray(ks, np.float64), G), "head_dim_inv": sinks / np.sqrt(float(D))}


@functools.lru_cache(maxsize=None)
def scaled_problem():
    s = SCALED
    p = ckw.make_problem(s["dtype"], s["D"], s["G"], LENS, (s["n"],) * 4, seed=12, k_factors=s["k_factors"])
    assert len(set(p.ks.tolist()) | set(p.vs.tolist())) == 4 and p.ks[1] / p.ks[0] > 3.9
    return p


# ---- the device ------------------------------------------------------------------------------------------------------------

class WithSinks:
    """The package `sfa` with the three windowed fp8 operators replaced by their _sinks twins at fixed `sinks` (a float32
    device tensor [H], or None = NULL): the run() harnesses of chunk_kv8_window_ref and of the single-token fp8-window
    tests then drive the sinks calls as they are."""

    def __init__(self, sfa, sinks, **extra):
        self._sfa, self._sinks, self._extra = sfa, sinks, extra     # extra: keyword arguments added to every call

    def __getattr__(self, name):
        return getattr(self._sfa, name)

    def flash_decode_kv8_window(self, *args, **kw):
        return self._sfa.flash_decode_kv8_window_sinks(*args, self._sinks, **{**kw, **self._extra})

    def flash_decode_chunk_kv8_window(self, *args, **kw):
        return self._sfa.flash_decode_chunk_kv8_window_sinks(*args, self._sinks, **{**kw, **self._extra})

    def flash_decode_varlen_kv8_window(self, *args, **kw):
        return self._sfa.flash_decode_varlen_kv8_window_sinks(*args, self._sinks, **{**kw, **self._extra})


def check_chunk(r, p, window, sinks, ref3, k_before=None, v_before=None, lens=None, k_bytes=True):
    """chunk_kv8_window_ref.check with the sink in (b): (a) the appended bytes by chunk_kv8_ref.check_bytes, unchanged
    (k_bytes=False: K only where the reference's bytes are the device's own, as there); (b) o of every sequence against
    attend_sinks() over the bytes the device stored, with q16 from the reference, at TOL, elementwise, nothing exempt.
    ref3 = chunk_kv8_sinks_ref(p, window, sinks)."""
    ref, k_ref, v_ref = ref3
    k_true = k_ref
    lens = p.lens if lens is None else lens
    if not k_bytes:
        k_ref = k_ref.copy()
        k_ref[~ckw.append_mask(p, lens)] = r.k8[~ckw.append_mask(p, lens)]
    ckr.check_bytes(lens, p.ns, r.k8, r.v8, p.k8 if k_before is None else k_before, p.v8 if v_before is None else v_before,
                    k_ref, v_ref)
    tol = TOL[p.dtype]
    for b, n in enumerate(p.ns):
        if n == 0:
            assert r.of[b].shape[0] == 0
            continue
        if np.array_equal(r.k8[b, LAYER], k_true[b, LAYER]) and np.array_equal(r.v8[b, LAYER], v_ref[b, LAYER]):
            want = ref["o"][b]                  # the device stored the reference's bytes
        else:
            want = attend_sinks(ref["q16"][b], r.k8[b, LAYER], r.v8[b, LAYER], lens[b], window, sinks, p.ks, p.vs, p.scale)[0]
        assert np.isfinite(r.of[b]).all(), b
        print("sequence %d: max |o - ref| = %.3e (tol %.1e)" % (b, np.abs(r.of[b] - want).max(), tol))
        np.testing.assert_allclose(r.of[b], want, atol=tol, rtol=tol, err_msg=f"sequence {b}")


def check_single_o(r, ref, dtype, window, sinks, ks, vs, lens=LENS, scale=None):
    """(b) for the single-token call: r.of [B, H, D] against attend_sinks() over the bytes the device stored (r.kc / r.vc
    canonical), with q16 from the reference, at TOL"""
    tol = TOL[dtype]
    for b, pos in enumerate(lens):
        if np.array_equal(r.kc[b, LAYER], ref["k8"][b, LAYER]) and np.array_equal(r.vc[b, LAYER], ref["v8"][b, LAYER]):
            want = ref["o64"][b]
        else:
            want = attend_sinks(ref["q16"][b][None], r.kc[b, LAYER], r.vc[b, LAYER], int(pos), window, sinks, ks, vs, scale)[0][0]
        assert np.isfinite(r.of[b]).all(), b
        print("sequence %d: max |o - ref| = %.3e (tol %.1e)" % (b, np.abs(r.of[b] - want).max(), tol))
        np.testing.assert_allclose(r.of[b], want, atol=tol, rtol=tol, err_msg=f"sequence {b}")
