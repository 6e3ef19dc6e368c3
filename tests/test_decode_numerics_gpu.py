"""Adversarial numerics of the five decode entry points (sfa_decode and its three kernels, sfa_decode_kv8,
sfa_decode_chunk, sfa_decode_varlen, sfa_decode_window) against the fp64 oracle, on the problems of
tests/decode_cases.py:

  A  softmax stress: a dominating key in a chosen tile / wave share / split, among the new tokens, nowhere; running
     maxima that move in every tile or never; all keys equal; all scores far below zero; logits in the hundreds
  W  the edges of a sliding window: the same structures placed on the first row of the window, on its last cached row
     and on the row just below it, for every alignment of lo to the 32-row tile, its 16-row halves and the pages
  B  softmax_scale (head_dim_inv of the C ABI), which no other decode test passes
  C  what the kernels must not read: NaN / Inf bit patterns in every cache byte outside rows 0 .. pos + n - 1 of
     idx_layer (a window: outside rows lo .. pos), -1 in the block_table entries past a sequence's last page (and of the
     pages wholly below lo), NaN in the workspace

Tolerances are the project's (tests/test_decode_gpu.py): kernel against fp64 on identical inputs, atol = rtol = 2e-3
(fp16) / 1.6e-2 (bf16), elementwise, nothing exempt.  Sections A and C run with rotary_embedding_dim = 0 and no bias, so
the q and k of the device are the input bits and the appended rows are compared bit for bit.  tests/
test_decode_numerics_cpu.py checks, without a GPU, that each problem has the structure it is named for.
"""
import numpy as np
import pytest
import torch

import decode_cases as dc
from oracle.numerics import from_bits16, to_bits16

pytestmark = pytest.mark.gpu

SPLITS = (1, 3)


@pytest.fixture(scope="module")
def sfa():
    assert torch.cuda.is_available(), "GPU tests need a GPU (run with -m gpu on the MI355X box)"
    import starflashattention_amd as m
    m._lib.load()                  # fail loudly if the HIP library is missing
    m.check_decode_status()
    return m


_cache = {}


def cached(key, make):
    """problems and their oracle results: computed once, shared by the tests that follow, never modified (the most
    recent 16: a spike batch with its oracle is 25 MB)"""
    if key not in _cache:
        while len(_cache) >= 16:
            del _cache[next(iter(_cache))]
        _cache[key] = make()
    return _cache[key]


def stress(entry, dtype, G, D, kind):
    def make():
        p = dc.softmax_stress(entry, dtype, G, D, kind)
        return p, dc.oracle(p)
    return cached(("A", entry, dtype, G, D, kind), make)


def edges(dtype, G, D, kind, window):
    def make():
        p = dc.window_edges(dtype, G, D, kind, window)
        return p, dc.oracle(p)
    return cached(("W", dtype, G, D, kind, window), make)


def assert_close(p, res, ref, what):
    o = from_bits16(res["o"], p.dtype)
    assert np.isfinite(o).all(), what
    tol = dc.TOL[p.dtype]
    np.testing.assert_allclose(o, ref["o"], atol=tol, rtol=tol, err_msg=str(what))


def assert_caches(p, res, ref, what):
    """rot = 0, no bias: the appended rows are the input bits (kv8: their codes), and no other byte of either cache,
    the spare pages of a pool included, has changed"""
    np.testing.assert_array_equal(res["kc"], ref["kc"], err_msg=f"{what}: k cache")
    np.testing.assert_array_equal(res["vc"], ref["vc"], err_msg=f"{what}: v cache")
    for s in (res["spare_k"], res["spare_v"]):
        assert s is None or np.all(s == p.spare_fill), f"{what}: a page no sequence owns was written"


# ---------------------------------------------------------------------------------------------------------------------
# A. softmax stress
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cfg,kind", [(c, k) for c in dc.CONFIGS for k in dc.stress_kinds(c[0])],
                         ids=lambda x: x if isinstance(x, str) else dc.config_id(x))
def test_softmax_stress(sfa, cfg, kind):
    """One batch per kind, a sequence per case (decode_cases.softmax_stress), at num_splits 1 and 3: o against the
    oracle; where a new token carries all the weight (1.0 in fp32), o is the bits of its v."""
    entry, G, D, layout, dtype, knobs = cfg
    p, ref = stress(entry, dtype, G, D, kind)
    for S in SPLITS:
        what = (dc.config_id(cfg), kind, f"num_splits={S}")
        res = dc.run(sfa, p, layout, S, knobs=knobs)
        sfa.check_decode_status()
        assert_close(p, res, ref, what)
        assert_caches(p, res, ref, what)
        for r in np.flatnonzero(p.exact):
            b, _ = p.seq_of(r)
            v = p.v_new[p.cu[b] + p.hot[r] - p.lens[b]]                       # [Hkv, D], representable in dtype
            np.testing.assert_array_equal(res["o"][r], np.repeat(to_bits16(v, p.dtype), G, axis=0),
                                          err_msg=f"{what}: token {r} must return v of key {p.hot[r]} exactly")


# ---------------------------------------------------------------------------------------------------------------------
# W. the edges of a sliding window
# ---------------------------------------------------------------------------------------------------------------------

_WINDOW_CONFIGS = [c for c in dc.CONFIGS if c[0] == "window"]


@pytest.mark.parametrize("window", dc.WINDOWS, ids=lambda w: f"w{w}")
@pytest.mark.parametrize("kind", dc.EDGE_KINDS)
@pytest.mark.parametrize("cfg", _WINDOW_CONFIGS, ids=dc.config_id)
def test_window_edges(sfa, cfg, kind, window):
    """One batch per (kind, window), a sequence per lo with pos = lo + window - 1 (decode_cases.window_edges): a key that
    carries all the weight on row lo or on row pos - 1; one just as large on row lo - 1, which nobody may see; a ramp that
    peaks at lo and goes on rising below it, and one that rises in every tile of the window; all keys equal with rows
    lo - 1, lo and pos - 1 of V so large that one row dropped, added or counted twice is far outside the tolerance
    (tests/test_decode_numerics_cpu.py).  At num_splits 1, 3 and 4 (window 17: splits and waves without rows): o against
    the oracle, elementwise; the appended rows and every other cache byte; a clean status."""
    entry, G, D, layout, dtype, knobs = cfg
    p, ref = edges(dtype, G, D, kind, window)
    for S in (1, 3, 4):
        what = (dc.config_id(cfg), kind, f"window={window}", f"num_splits={S}")
        res = dc.run(sfa, p, layout, S, knobs=knobs)
        sfa.check_decode_status()
        assert_close(p, res, ref, what)
        assert_caches(p, res, ref, what)


# ---------------------------------------------------------------------------------------------------------------------
# B. softmax_scale
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cfg", dc.CONFIGS, ids=dc.config_id)
def test_softmax_scale(sfa, cfg):
    """N(0,1) data (rotation on for the 16-bit caches; kv8 with k_scale = amax / 448 times [0.5, 2.0] per head; the
    window: 40) at softmax_scale 0.03 and 0.5 against the oracle with scale=; the call without the argument gives
    another result."""
    entry, G, D, layout, dtype, knobs = cfg
    p = cached(("B", entry, dtype, G, D), lambda: dc.normal_problem(entry, dtype, G, D, rot=0 if entry == "kv8" else D,
                                                                    amax_scales=True))
    if entry == "kv8":
        assert p.ks[0] != p.ks[1] and not np.any(np.log2(p.ks) % 1 == 0)
    default = dc.run(sfa, p, layout, 1, knobs=knobs)
    for scale in (0.03, 0.5):
        ref = cached(("B", entry, dtype, G, D, scale), lambda: dc.oracle(p, scale=scale))
        for S in SPLITS:
            what = (dc.config_id(cfg), f"softmax_scale={scale}", f"num_splits={S}")
            res = dc.run(sfa, p, layout, S, softmax_scale=scale, knobs=knobs)
            sfa.check_decode_status()
            assert_close(p, res, ref, what)
            d = np.abs(from_bits16(res["o"], dtype) - from_bits16(default["o"], dtype))
            assert d.max() > 2 * dc.TOL[dtype], f"{what}: the same as without softmax_scale"


# ---------------------------------------------------------------------------------------------------------------------
# C. unread memory is not read
# ---------------------------------------------------------------------------------------------------------------------

_UNREAD = ([(c, "nan") for c in dc.CONFIGS] + [(c, "inf") for c in dc.CONFIGS if c[0] != "kv8"] +
           [(c, "nan_table-1") for c in dc.CONFIGS if c[3] == "paged"])
# the window: each mode at every window of decode_cases.UNREAD_WINDOWS; "nan" is window 40, "nan_w16" window 16, ...
_UNREAD += [(c, f"{mode}_w{w}") for c, mode in _UNREAD if c[0] == "window" for w in dc.UNREAD_WINDOWS[1:]]


@pytest.mark.parametrize("cfg,mode", _UNREAD, ids=lambda x: x if isinstance(x, str) else dc.config_id(x))
def test_unread_memory_is_not_read(sfa, cfg, mode):
    """The same call on a clean problem (zeros in every cache byte the contract does not name) and on a poisoned one (NaN
    patterns there -- 0x7FFF, e4m3 0x7F -- or +Inf; in the pages nobody owns as well; "table-1": and -1 in the block_table
    entries past the last page a sequence needs): o and the appended rows bit-identical, the status clean, every poisoned
    byte still in place.  num_splits 4 leaves splits without keys at the small positions.
    A window: the rows below lo are poisoned as well (in the clean problem they hold the sequence's data), "table-1" also
    puts -1 into the entries of the pages wholly below lo, and "_w16" / "_w1" run window 16 (at pos = 15, 31, 63 the window
    begins exactly on a page boundary) and window 1 (no cached row is read; lo = pos, mostly on no tile boundary)
    instead of 40."""
    entry, G, D, layout, dtype, knobs = cfg
    mode, _, window = mode.partition("_w")
    window = (int(window) if window else dc.STRESS_WINDOW) if entry == "window" else None
    clean = cached(("C", entry, dtype, G, D, window), lambda: dc.normal_problem(entry, dtype, G, D, window=window))
    ref = cached(("C", entry, dtype, G, D, window, "oracle"), lambda: dc.oracle(clean))
    bad = clean.poisoned(dc.INF16[dtype] if mode == "inf" else None)
    m = clean.unread_mask()
    for S in (1, 3, 4):
        what = (dc.config_id(cfg), mode, f"num_splits={S}")
        a = dc.run(sfa, clean, layout, S, knobs=knobs)
        sfa.check_decode_status()
        minus = -1 if mode.endswith("table-1") else None
        z = dc.run(sfa, bad, layout, S, table_beyond=minus, table_below=minus, knobs=knobs)
        sfa.check_decode_status()                                           # clean, the -1 entries included
        assert np.isfinite(from_bits16(z["o"], dtype)).all(), what
        np.testing.assert_array_equal(z["o"], a["o"], err_msg=f"{what}: o depends on bytes outside the contract")
        for k in ("kc", "vc"):
            np.testing.assert_array_equal(z[k][~m], a[k][~m], err_msg=f"{what}: appended rows of {k}")
            np.testing.assert_array_equal(z[k][m], getattr(bad, k)[m], err_msg=f"{what}: a poisoned byte of {k} changed")
        assert_caches(clean, a, ref, what)
        for s in (z["spare_k"], z["spare_v"]):
            assert s is None or np.all(s == bad.spare_fill), f"{what}: a page no sequence owns was written"
        assert_close(clean, a, ref, what)


_STALE = [c for c in dc.CONFIGS if (c[0], c[1], c[2], c[3]) in
          {("decode", 1, 128, "blmhd"), ("decode", 2, 128, "blmhd"), ("decode", 4, 128, "blmhd"), ("kv8", 4, 128, "blmhd"),
           ("chunk", 8, 128, "blmhd"), ("varlen", 8, 128, "paged")}]


@pytest.mark.parametrize("cfg", _STALE, ids=dc.config_id)
def test_stale_workspace_is_not_read(sfa, cfg):
    """Through the C ABI with a workspace of exactly the size the library asks for, every byte of it 0xFF (fp32 NaN) before
    the call, num_splits = 4 and a batch with pos = 0 (splits without keys; varlen: and a sequence without tokens):
    bit-identical to the operator on its own cached workspace."""
    entry, G, D, layout, dtype, _ = cfg
    assert len(_STALE) == 6
    p = dc.normal_problem(entry, dtype, G, D, stale=True)
    assert 0 in p.lens and (entry != "varlen" or 0 in p.ns)
    a = dc.Run(p, layout).call(sfa, 4).result()
    sfa.check_decode_status()
    z = dc.Run(p, layout).call_exact_workspace(4, fill=0xFF).result()
    assert np.isfinite(from_bits16(z["o"], dtype)).all()
    for k in ("o", "kc", "vc"):
        np.testing.assert_array_equal(z[k], a[k], err_msg=k)
    ref = dc.oracle(p)
    assert_close(p, z, ref, dc.config_id(cfg))
    assert_caches(p, z, ref, dc.config_id(cfg))
