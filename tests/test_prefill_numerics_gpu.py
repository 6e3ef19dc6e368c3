"""Adversarial numerics of the prefill forward (sfa_prefill_fwd, every selectable kernel) against the fp64 oracle, on the
problems of tests/prefill_cases.py:

  A  softmax stress: a key that carries all the weight on every tile, wave and page edge and on the causal diagonal; the
     same with one aligned query row per 32-row block; staircases whose steps straddle the lazy-rescale threshold; ramps;
     all keys equal with a marker in the last V row (the row-clamped ragged tile); all scores far below zero; chained
     q-tiles of the persistent kernels with row maxima of alternating sign
  B  softmax_scale, for o and lse
  C  what the result must not depend on: NaN / Inf between the rows, heads and batches of strided views and past Sq and
     Sk; nothing written outside O's view or past lse's B * Hq * Sq floats; K / V with a batch or head stride of 0; empty
     problems

Tolerances are the project's (tests/test_prefill_gpu.py): o atol = rtol = 2e-3 (fp16) / 1.6e-2 (bf16), elementwise, nothing
exempt; lse that file's LSE_TOL by flavour.  tests/test_prefill_numerics_cpu.py proves, without a GPU, that each problem
has the structure it is named for; profiles/prefill_numerics_mutations.txt records that one-line mutants fail here.
"""
import numpy as np
import pytest
import torch

import prefill_cases as pc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sfa():
    assert torch.cuda.is_available(), "GPU tests need a GPU (run with -m gpu on the MI355X box)"
    import starflashattention_amd as m
    m._lib.load()
    return m


@pytest.fixture
def knobs(sfa):
    """kernel selection through sfa_debug_set; back on the library's own choice after the test"""
    yield sfa.debug_set
    for n in ("prefill_impl", "prefill_pairs"):
        sfa.debug_set(n, -1)


_cache = {}


def cached(key, make):
    """problems (with their oracle results and device copies): made once, shared by the tests that follow, never modified
    (the most recent 6: a spike batch of 84 query heads with both oracles is 80 MB)"""
    if key not in _cache:
        while len(_cache) >= 6:
            del _cache[next(iter(_cache))]
        _cache[key] = make()
    return _cache[key]


def by_data(params, key):
    """parameters ordered so that tests on the same problem follow one another (the cache is small)"""
    return sorted(params, key=key)


def assert_kernel(sfa, cfg):
    """the configuration ran the kernel it is named for (the coverage of this file rests on it)"""
    assert sfa.last_prefill_kernel() == pc.expected_kernel(cfg[0], cfg[1]), (pc.config_id(cfg), sfa.last_prefill_kernel())


def assert_matches(p, res, causal, impl, what, scale=None, ref=None):
    o_want, lse_want = ref or p.oracle(causal, scale)
    o = pc.values(p, res["o"])
    assert np.isfinite(o).all(), what
    tol = pc.TOL[p.dtype]
    np.testing.assert_allclose(o, o_want, atol=tol, rtol=tol, err_msg=str(what))
    fin = np.isfinite(lse_want)
    ltol = pc.LSE_TOL[pc.flavour(impl)][p.dtype]
    np.testing.assert_allclose(res["lse"][fin], lse_want[fin], atol=ltol, rtol=ltol, err_msg=f"{what}: lse")
    assert np.all(res["lse"][~fin] == -np.inf), f"{what}: lse of a row without a key"
    assert np.all(res["o"][~fin] & 0x7FFF == 0), f"{what}: o of a row without a key must be zeros"
    assert np.all(res["lse_tail"] == pc.LSE_SENTINEL), f"{what}: lse written past B * Hq * Sq floats"


# ---------------------------------------------------------------------------------------------------------------------
# A. softmax stress
# ---------------------------------------------------------------------------------------------------------------------

_STRESS = by_data([(c, k) for c in pc.CONFIGS for k in pc.stress_kinds(c[0], c[1])],
                  key=lambda ck: (ck[1], ck[0][1], ck[0][2], ck[0][3]))


@pytest.mark.parametrize("cfg,kind", _STRESS, ids=lambda x: x if isinstance(x, str) else pc.config_id(x))
def test_softmax_stress(sfa, knobs, cfg, kind):
    """One batch per kind and shape, a case per (batch, kv head), at the three alignments of the causal mask, full and
    causal: o and lse against the oracle.  Where a key carries all the weight (1.0 in fp32: tests/
    test_prefill_numerics_cpu.py), o is the bits of its V row in every kernel: a rise of 46 to 92 log2 units is far above
    the threshold of 8, so the reference moves to the row's own max (exact flavours: mnew = max(msc, mx); prescaled:
    d = max(mx, 0)), the weight is 2^(fma(s, c2, -round(s c2))) = 1 +- 3e-6 (exact) or 2^0 (prescaled), which packs to 1.0
    in 16 bit, every other weight is at most 2^-40 of it, and o / lsum = V (1 +- 3e-6) rounds back to V.
    All kinds run on the prescaled flavours too (prefill_cases.PRESCALED_KINDS: none is left out)."""
    impl, D, dtype, G = cfg
    pc.select_impl(knobs, impl)
    for Sq, Sk in pc.SHAPES:
        p = cached(("A", kind, dtype, D, G, Sq, Sk), lambda: pc.softmax_stress(kind, dtype, D, G, Sq, Sk))
        for causal in (False, True):
            what = (pc.config_id(cfg), kind, f"Sq={Sq} Sk={Sk} causal={causal}")
            res = pc.run(sfa, p, causal)
            assert_kernel(sfa, cfg)
            assert_matches(p, res, causal, impl, what)
            if kind in ("spike", "alone"):
                sees = np.repeat(p.sees(causal), G, axis=1)                                 # [B, Hq, Sq]
                want = np.repeat(pc.v_bits(p)[np.arange(p.B)[:, None], np.arange(p.Hkv)[None, :], p.spike], G, axis=1)
                got = res["o"][sees]
                np.testing.assert_array_equal(got, np.broadcast_to(want[:, :, None, :], res["o"].shape)[sees],
                                              err_msg=f"{what}: a row that sees key j* must return V[j*] exactly")
                assert sees.any() or (kind == "alone" and causal)


_W4 = [c for c in pc.CONFIGS if c[0].endswith("w4") and c[3] == 1]


@pytest.mark.parametrize("shape", pc.CHAINED, ids=lambda s: "b%d_hq%d_hkv%d_sq%d_sk%d" % s)
@pytest.mark.parametrize("cfg", _W4, ids=pc.config_id)
def test_chained_q_tiles_keep_no_state(sfa, knobs, cfg, shape):
    """More units than persistent workgroups: consecutive q-tiles of a workgroup have row maxima more than 100 log2 units
    apart and of opposite sign (prefill_cases.chained), so a reference max, row sum or O left over from the previous
    q-tile shows in either order of traversal.  The shapes carry their own group size (1 and 4)."""
    impl, D, dtype, _ = cfg
    pc.select_impl(knobs, impl)
    p = cached(("chained", dtype, shape), lambda: pc.chained(dtype, shape))
    for causal in (False, True):
        res = pc.run(sfa, p, causal)
        assert "prefill_w4_kernel" in sfa.last_prefill_kernel()
        assert_matches(p, res, causal, impl, (pc.config_id(cfg), shape, f"causal={causal}"))


# ---------------------------------------------------------------------------------------------------------------------
# B. softmax_scale
# ---------------------------------------------------------------------------------------------------------------------

_BY_DATA = by_data(pc.CONFIGS, key=lambda c: (c[1], c[2], c[3]))


@pytest.mark.parametrize("cfg", _BY_DATA, ids=pc.config_id)
def test_softmax_scale(sfa, knobs, cfg):
    """N(0,1) data, Sq = Sk = 299, softmax_scale 0.03 and 0.5: o and lse against the oracle with scale=, and another
    result than the call without the argument.  The prescaled flavours at 0.5: against the fp64 result from the Q they
    round (prefill_cases.PRESCALED_SCALES says why: that result alone is 0.95 to 2.3 tolerances away from the oracle), at
    the same tolerance."""
    impl, D, dtype, G = cfg
    pc.select_impl(knobs, impl)
    p = cached(("N", dtype, D, G, 299, 299), lambda: pc.normal_problem(dtype, D, G, 299, 299))
    for causal in (False, True):
        default = pc.values(p, pc.run(sfa, p, causal)["o"])
        for scale in pc.SCALES:
            what = (pc.config_id(cfg), f"softmax_scale={scale} causal={causal}")
            res = pc.run(sfa, p, causal, scale=scale)
            assert_kernel(sfa, cfg)
            own = pc.flavour(impl) == "prescaled" and scale not in pc.PRESCALED_SCALES
            assert_matches(p, res, causal, impl, what, scale=scale, ref=p.prescaled(causal, scale) if own else None)
            d = np.abs(pc.values(p, res["o"]) - default)
            assert d.max() > 2 * pc.TOL[dtype], f"{what}: the same as without softmax_scale"


# ---------------------------------------------------------------------------------------------------------------------
# C. what the result must not depend on
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cfg", _BY_DATA, ids=pc.config_id)
def test_result_does_not_depend_on_what_lies_outside_the_views(sfa, knobs, cfg):
    """Q, K, V and O are views base[:, :, g : g + S, :D] of allocations [B, H, g + S + g, D + 8] (g = 256 rows for Q and O,
    64 for K and V), run with zeros, with 0x7FFF (NaN) and with +Inf in every element outside the views: o and lse
    bit-identical across the three, finite where the oracle is, the clean run matches the oracle, every element of O's
    allocation outside its view still holds what it was filled with, and so do the 64 floats behind lse."""
    impl, D, dtype, G = cfg
    pc.select_impl(knobs, impl)
    for Sq, Sk in pc.SHAPES + pc.ONE_ROW_SHAPES:
        p = cached(("N", dtype, D, G, Sq, Sk), lambda: pc.normal_problem(dtype, D, G, Sq, Sk))
        for causal in (False, True):
            what = (pc.config_id(cfg), f"Sq={Sq} Sk={Sk} causal={causal}")
            clean = None
            for name, fill in (("zeros", 0), ("nan", pc.NAN16), ("inf", pc.INF16[dtype])):
                res = pc.run(sfa, p, causal, fill_bits=fill)
                assert_kernel(sfa, cfg)
                assert np.all(res["o_outside"] == fill), f"{what} {name}: O's allocation was written outside its view"
                assert np.all(res["lse_tail"] == pc.LSE_SENTINEL), f"{what} {name}: lse written past B * Hq * Sq floats"
                if clean is None:
                    clean = res
                    assert_matches(p, res, causal, impl, what)
                else:
                    assert np.isfinite(pc.values(p, res["o"])).all(), f"{what} {name}"
                    np.testing.assert_array_equal(res["o"], clean["o"], err_msg=f"{what} {name}: o depends on it")
                    np.testing.assert_array_equal(res["lse"], clean["lse"], err_msg=f"{what} {name}: lse depends on it")


@pytest.mark.parametrize("cfg", _BY_DATA, ids=pc.config_id)
def test_stride_zero_is_the_expanded_tensor(sfa, knobs, cfg):
    """K and V shared across the batch (batch stride 0), and one stored head shared by every kv head (head stride 0):
    bit-identical to the same call on .contiguous() copies."""
    impl, D, dtype, G = cfg
    pc.select_impl(knobs, impl)
    for Sq, Sk in ((299, 299), (100, 299)):
        p = cached(("N", dtype, D, G, Sq, Sk), lambda: pc.normal_problem(dtype, D, G, Sq, Sk))
        _, k, v = pc.device_inputs(p)
        for name, ex in (("batch", lambda t: t[:1].expand(p.B, -1, -1, -1)), ("head", lambda t: t[:, :1].expand(-1, p.Hkv, -1, -1))):
            ke, ve = ex(k), ex(v)
            assert 0 in ke.stride() and 0 in ve.stride()
            for causal in (False, True):
                a = pc.run(sfa, p, causal, kv=(ke, ve))
                assert_kernel(sfa, cfg)
                z = pc.run(sfa, p, causal, kv=(ke.contiguous(), ve.contiguous()))
                what = (pc.config_id(cfg), name, f"Sq={Sq} Sk={Sk} causal={causal}")
                assert np.isfinite(pc.values(p, a["o"])).all(), what
                np.testing.assert_array_equal(a["o"], z["o"], err_msg=str(what))
                np.testing.assert_array_equal(a["lse"], z["lse"], err_msg=str(what))
        # and the shared tensors are what the oracle says for the expanded problem (once, full attention)
        want = pc.sdpa_ref(p.q, np.broadcast_to(p.k[:1], p.k.shape), np.broadcast_to(p.v[:1], p.v.shape))
        got = pc.values(p, pc.run(sfa, p, False, kv=(k[:1].expand(p.B, -1, -1, -1), v[:1].expand(p.B, -1, -1, -1)))["o"])
        np.testing.assert_allclose(got, want, atol=pc.TOL[dtype], rtol=pc.TOL[dtype])


@pytest.mark.parametrize("cfg", [c for c in _BY_DATA if c[0] in ("auto", "rows128")], ids=pc.config_id)
def test_empty_problems(sfa, knobs, cfg):
    """seqlen_k = 0: o is zeros and lse -inf in every row, nothing written outside the views.  batch = 0 or seqlen_q = 0:
    SFA_OK, and o and lse untouched.  No prefill kernel runs, so one configuration per head_dim, type and group size.
    (Under the causal mask with Sq > Sk the rows without a key give zeros and -inf: test_softmax_stress and section C
    at (299, 100) and (299, 1), through the oracle and the exact checks of assert_matches.)"""
    impl, D, dtype, G = cfg
    pc.select_impl(knobs, impl)
    p = cached(("N", dtype, D, G, 100, 299), lambda: pc.normal_problem(dtype, D, G, 100, 299))
    q, k, v = pc.device_inputs(p)
    fill = 0x3C00 if dtype == "fp16" else 0x3F80                                             # 1.0
    n = p.B * p.Hq * p.Sq
    for causal in (False, True):
        for name, sizes in (("Sk=0", (p.B, p.Hq, p.Hkv, p.Sq, 0, D)), ("batch=0", (0, p.Hq, p.Hkv, p.Sq, p.Sk, D)),
                            ("Sq=0", (p.B, p.Hq, p.Hkv, 0, p.Sk, D))):
            o_base, o = pc.guarded(q, pc.GUARD_Q, fill, copy=False)
            lse = torch.full((n + pc.LSE_TAIL,), pc.LSE_SENTINEL, dtype=torch.float32, device=q.device)
            st = pc.call(sfa, q, k, v, o, lse, causal, sizes=sizes)
            torch.cuda.synchronize()
            what = (pc.config_id(cfg), name, f"causal={causal}")
            assert st == 0, what
            assert np.all(pc.outside(o_base, pc.GUARD_Q, p.Sq, D) == fill), what
            ob, l = pc._bits_of(o), lse.cpu().numpy()
            if name == "Sk=0":
                assert np.all(ob == 0), what
                assert np.all(l[:n] == -np.inf) and np.all(l[n:] == pc.LSE_SENTINEL), what
            else:
                assert np.all(ob == fill) and np.all(l == pc.LSE_SENTINEL), what
