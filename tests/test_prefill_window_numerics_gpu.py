"""Adversarial numerics of the windowed prefill forward (sfa_prefill_window_fwd, all eight instances of
prefill_window_kernel<type, head_dim, SINK>) against the fp64 reference of tests/prefill_window_ref.py, on the problems of
tests/prefill_window_cases.py:

  A  softmax stress under the windows 1, 40, 65 and 150: a key that carries all the weight inside the window, one key
     below its lower bound and one above its limit; staircases rising and falling over the key tiles (falling: the keys
     just below a lower bound on a tile edge outweigh everything the row sees, and the row max drops as the window slides);
     ramps; all keys equal; all scores far below zero -- without sinks and with sinks of material weight
  B  softmax_scale, which the sink is not multiplied by
  C  what the result must not depend on: NaN / Inf outside strided views, past Sq and Sk and in the rows below lo_0;
     nothing written outside O's view or behind lse; K / V with a batch or head stride of 0; empty problems

Tolerances are the project's (tests/test_prefill_gpu.py): o atol = rtol = 2e-3 (fp16) / 1.6e-2 (bf16), elementwise, nothing
exempt; lse 2e-3 (the windowed kernel is an exact-scale kernel).  A row without a key is all zero bits with lse = -inf.
tests/test_prefill_window_numerics_cpu.py proves, without a GPU, that each problem has the structure it is named for;
profiles/prefill_window_numerics_mutations.txt records which one-line mutants fail here.
"""
import contextlib

import numpy as np
import pytest
import torch

import prefill_cases as pc
import prefill_window_cases as wc
from prefill_window_ref import prefill_window_ref

pytestmark = pytest.mark.gpu

MARKER_IMPL = pc.IMPLS["rows256"]            # forced: the library's own choice never reports this id


@pytest.fixture(scope="module")
def sfa():
    assert torch.cuda.is_available(), "GPU tests need a GPU (run with -m gpu on the MI355X box)"
    import starflashattention_amd as m
    m._lib.load()
    return m


_cache = {}


def cached(key, make):
    """problems (with their references and device copies): made once, shared by the tests that follow, never modified (the
    most recent 6)"""
    if key not in _cache:
        while len(_cache) >= 6:
            del _cache[next(iter(_cache))]
        _cache[key] = make()
    return _cache[key]


def stress(kind, cfg, shape):
    D, dtype, G = cfg
    return cached(("A", kind, cfg, shape), lambda: wc.stress_w(kind, dtype, D, G, *shape))


def normal(cfg, shape):
    D, dtype, G = cfg
    return cached(("N", cfg, shape), lambda: wc.normal_problem(dtype, D, G, *shape))


def mark(sfa):
    """a one-row full-attention call on the forced 8-wave kernel -> what last_prefill_kernel says after it"""
    q = torch.zeros(1, 1, 1, 64, dtype=torch.bfloat16, device="cuda:0")
    sfa.debug_set("prefill_impl", MARKER_IMPL)
    try:
        assert pc.call(sfa, q, q, q, torch.empty_like(q), None, False) == 0
    finally:
        sfa.debug_set("prefill_impl", -1)
    torch.cuda.synchronize()
    ran = sfa.debug_get("last_prefill_kernel")
    assert ran == MARKER_IMPL
    return ran


@contextlib.contextmanager
def only_the_windowed_kernel(sfa):
    """the windowed kernel leaves last_prefill_kernel alone: unchanged after the block, no causal kernel ran in it"""
    ran = mark(sfa)
    yield
    assert sfa.debug_get("last_prefill_kernel") == ran, "a call of the block went to the causal kernels"


def assert_matches(p, res, ref, what):
    o_want, lse_want = ref
    o = wc.values(p, res["o"])
    assert np.isfinite(o).all(), what
    tol = wc.TOL[p.dtype]
    print(f"{what}: max |o - ref| = {np.abs(o - o_want).max():.3e}")
    np.testing.assert_allclose(o, o_want, atol=tol, rtol=tol, err_msg=str(what))
    fin = np.isfinite(lse_want)
    ltol = wc.LSE_TOL[p.dtype]
    np.testing.assert_allclose(res["lse"][fin], lse_want[fin], atol=ltol, rtol=ltol, err_msg=f"{what}: lse")
    assert np.all(res["lse"][~fin] == -np.inf), f"{what}: lse of a row without a key"
    assert np.all(res["o"][~fin] == 0), f"{what}: o of a row without a key must be all zero bits"
    assert np.all(res["lse_tail"] == wc.LSE_SENTINEL), f"{what}: lse written past B * Hq * Sq floats"


def _id(x):
    return x if isinstance(x, str) else ("sinks" if x else "nosink") if isinstance(x, bool) else wc.config_id(x)


def test_the_marker_is_no_kernel_the_library_chooses(sfa):
    """what only_the_windowed_kernel rests on: a windowed call without sinks whose window covers every key goes to the
    causal kernels and changes last_prefill_kernel; one with a shorter window does not"""
    p = normal(wc.CONFIGS_W[0], (100, 299))
    ran = mark(sfa)
    wc.run_window(sfa, p, p.Sk - 1)
    assert sfa.debug_get("last_prefill_kernel") == ran
    wc.run_window(sfa, p, p.Sk)
    assert sfa.debug_get("last_prefill_kernel") not in (ran, -1)


# ---------------------------------------------------------------------------------------------------------------------
# A. softmax stress
# ---------------------------------------------------------------------------------------------------------------------

_STRESS = sorted([(c, s, k) for c in wc.CONFIGS_W for s in wc.SINKS for k in wc.KINDS_W],
                 key=lambda x: (x[2], wc.CONFIGS_W.index(x[0]), x[1]))            # the two sink settings of a problem follow


@pytest.mark.parametrize("cfg,sinks,kind", _STRESS, ids=_id)
def test_softmax_stress(sfa, cfg, sinks, kind):
    """One batch per kind and shape, a case per (batch, kv head), at the three alignments of the causal mask and every
    admitted window: o and lse against the reference.  Where a key inside the window carries all the weight (1.0 in fp32,
    every other weight at most 2^-40: tests/test_prefill_window_numerics_cpu.py), o is the bits of its V row -- with sinks
    in the rows where the sink's share is at most 2^-25 (prefill_window_cases.exact_rows_w); every other row is the
    reference's, the rows with that key one below their lower bound or one above their limit among them."""
    with only_the_windowed_kernel(sfa):
        for shape, window in wc.stress_runs(sinks):
            p = stress(kind, cfg, shape)
            s = wc.sinks_for(p, window) if sinks else None
            what = (wc.config_id(cfg), _id(sinks), kind, f"Sq={shape[0]} Sk={shape[1]} window={window}")
            res = wc.run_window(sfa, p, window, s)
            assert_matches(p, res, wc.oracle_w(p, window, s), what)
            if kind in ("spike", "alone"):
                exact = wc.exact_rows_w(p, window, s)
                want = np.repeat(wc.v_bits(p)[np.arange(p.B)[:, None], np.arange(p.Hkv)[None, :], p.spike], p.G, axis=1)
                np.testing.assert_array_equal(res["o"][exact], np.broadcast_to(want[:, :, None, :], res["o"].shape)[exact],
                                              err_msg=f"{what}: a row that sees key j* must return V[j*] exactly")
                assert exact.any() or sinks, what


# ---------------------------------------------------------------------------------------------------------------------
# B. softmax_scale
# ---------------------------------------------------------------------------------------------------------------------

_CS = [(c, s) for c in wc.CONFIGS_W for s in wc.SINKS]


@pytest.mark.parametrize("cfg,sinks", _CS, ids=_id)
def test_softmax_scale(sfa, cfg, sinks):
    """N(0,1) data, Sq = Sk = 299, windows 40 and 150, softmax_scale 0.03 and 0.5: o and lse against the reference with
    scale= (the sinks are the default-scale problem's, and no scale multiplies them), and another result than the call
    without the argument."""
    p = normal(cfg, wc.SCALE_SHAPE)
    with only_the_windowed_kernel(sfa):
        for window in wc.GUARD_WINDOWS:
            s = wc.sinks_for(p, window) if sinks else None
            default = wc.values(p, wc.run_window(sfa, p, window, s)["o"])
            for scale in wc.SCALES:
                what = (wc.config_id(cfg), _id(sinks), f"window={window} softmax_scale={scale}")
                res = wc.run_window(sfa, p, window, s, scale=scale)
                assert_matches(p, res, wc.oracle_w(p, window, s, scale), what)
                d = np.abs(wc.values(p, res["o"]) - default)
                assert d.max() > 2 * wc.TOL[p.dtype], f"{what}: the same as without softmax_scale"


# ---------------------------------------------------------------------------------------------------------------------
# C. what the result must not depend on
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cfg,sinks", _CS, ids=_id)
def test_result_does_not_depend_on_what_no_row_sees(sfa, cfg, sinks):
    """Q, K, V and O are views base[:, :, g : g + S, :D] of allocations [B, H, g + S + g, D + 8] (g = 256 rows for Q and O,
    64 for K and V), run with zeros, with 0x7FFF (NaN) and with +Inf in every element outside the views and in the K and V
    rows [0, lo_0) inside them: o and lse bit-identical across the three, finite where the reference is, the clean run
    matches the reference, every element of O's allocation outside its view still holds what it was filled with, and so do
    the 64 floats behind lse."""
    with only_the_windowed_kernel(sfa):
        for shape, window in wc.guard_runs(sinks):
            p = normal(cfg, shape)
            s = wc.sinks_for(p, window) if sinks else None
            ref = wc.oracle_w(p, window, s)
            what = (wc.config_id(cfg), _id(sinks), f"Sq={shape[0]} Sk={shape[1]} window={window}")
            clean = None
            for name, fill in zip(wc.FILLS, (0, pc.NAN16, pc.INF16[p.dtype])):
                res = wc.run_window(sfa, p, window, s, fill_bits=fill)
                assert np.all(res["o_outside"] == fill), f"{what} {name}: O's allocation was written outside its view"
                assert np.all(res["lse_tail"] == wc.LSE_SENTINEL), f"{what} {name}: lse written past B * Hq * Sq floats"
                if clean is None:
                    clean = res
                    assert_matches(p, res, ref, what)
                else:
                    assert np.isfinite(wc.values(p, res["o"])).all(), f"{what} {name}"
                    assert np.isfinite(res["lse"][np.isfinite(ref[1])]).all(), f"{what} {name}"
                    np.testing.assert_array_equal(res["o"], clean["o"], err_msg=f"{what} {name}: o depends on it")
                    np.testing.assert_array_equal(res["lse"], clean["lse"], err_msg=f"{what} {name}: lse depends on it")


@pytest.mark.parametrize("cfg,sinks", _CS, ids=_id)
def test_stride_zero_is_the_expanded_tensor(sfa, cfg, sinks):
    """K and V shared across the batch (batch stride 0), and one stored head shared by every kv head (head stride 0):
    bit-identical to the same call on .contiguous() copies; once per problem, the batch-shared call against the reference
    of the expanded problem."""
    with only_the_windowed_kernel(sfa):
        for shape in wc.STRIDE0_SHAPES:
            p = normal(cfg, shape)
            _, k, v = pc.device_inputs(p)
            for name, ex in (("batch", lambda t: t[:1].expand(p.B, -1, -1, -1)), ("head", lambda t: t[:, :1].expand(-1, p.Hkv, -1, -1))):
                ke, ve = ex(k), ex(v)
                assert 0 in ke.stride() and 0 in ve.stride()
                for window in wc.GUARD_WINDOWS:
                    s = wc.sinks_for(p, window) if sinks else None
                    a = wc.run_window(sfa, p, window, s, kv=(ke, ve))
                    z = wc.run_window(sfa, p, window, s, kv=(ke.contiguous(), ve.contiguous()))
                    what = (wc.config_id(cfg), _id(sinks), name, f"Sq={shape[0]} Sk={shape[1]} window={window}")
                    assert np.isfinite(wc.values(p, a["o"])).all(), what
                    np.testing.assert_array_equal(a["o"], z["o"], err_msg=str(what))
                    np.testing.assert_array_equal(a["lse"], z["lse"], err_msg=str(what))
            window = wc.GUARD_WINDOWS[0]
            s = wc.sinks_for(p, window) if sinks else None
            ref = prefill_window_ref(p.q, np.broadcast_to(p.k[:1], p.k.shape), np.broadcast_to(p.v[:1], p.v.shape), window,
                                     sinks=None if s is None else s.astype(np.float64))
            res = wc.run_window(sfa, p, window, s, kv=(k[:1].expand(p.B, -1, -1, -1), v[:1].expand(p.B, -1, -1, -1)))
            assert_matches(p, res, ref, (wc.config_id(cfg), _id(sinks), f"expanded Sq={shape[0]} Sk={shape[1]} window={window}"))


@pytest.mark.parametrize("cfg,sinks", _CS, ids=_id)
def test_empty_problems(sfa, cfg, sinks):
    """seqlen_k = 0, sinks or not: o is zeros and lse -inf in every row, nothing written outside the views.  batch = 0 or
    seqlen_q = 0: SFA_OK, and o and lse untouched.  (Under the window with Sq > Sk the rows without a key give zeros and
    -inf: test_softmax_stress and the guarded runs at (299, 100) and (299, 1), through the reference.)"""
    D, dtype, G = cfg
    p = normal(cfg, (100, 299))
    q, k, v = pc.device_inputs(p)
    ts = torch.from_numpy(wc.sinks_for(p, 40)).to(q.device) if sinks else None
    fill = 0x3C00 if dtype == "fp16" else 0x3F80                                             # 1.0
    n = p.B * p.Hq * p.Sq
    with only_the_windowed_kernel(sfa):
        for name, sizes in zip(wc.EMPTY, ((p.B, p.Hq, p.Hkv, p.Sq, 0, D), (0, p.Hq, p.Hkv, p.Sq, p.Sk, D),
                                          (p.B, p.Hq, p.Hkv, 0, p.Sk, D))):
            o_base, o = wc.guarded(q, wc.GUARD_Q, fill, copy=False)
            lse = torch.full((n + wc.LSE_TAIL,), wc.LSE_SENTINEL, dtype=torch.float32, device=q.device)
            st = wc.call_window(sfa, q, k, v, o, lse, 40, ts, sizes=sizes)
            torch.cuda.synchronize()
            what = (wc.config_id(cfg), _id(sinks), name)
            assert st == 0, what
            assert np.all(wc.outside(o_base, wc.GUARD_Q, p.Sq, D) == fill), what
            ob, l = wc._bits_of(o), lse.cpu().numpy()
            if name == "Sk=0":
                assert np.all(ob == 0), what
                assert np.all(l[:n] == -np.inf) and np.all(l[n:] == wc.LSE_SENTINEL), what
            else:
                assert np.all(ob == fill) and np.all(l == wc.LSE_SENTINEL), what
