"""The problems of tests/prefill_cases.py have the structure they are named for -- proved from the fp64 oracle alone, no
GPU.  What tests/test_prefill_numerics_gpu.py relies on:

  - the key of every "spike" and "alone" case carries weight 1.0 in fp32 in every row that sees it, so o is the bits of
    its V row and lse its score; under the causal mask the first row that sees it is row j* - (Sk - Sq)
  - the staircases rise per key tile alternately by 6.5-7.5 and by 8.5-9.5 log2 units: below and above the lazy-rescale
    threshold of 8; their coefficients are exact in fp16 and bf16
  - the ascending ramp moves the row max in every tile, the descending one never after the first
  - the marker row of "equal" moves every element of o by more than five times the bf16 atol if the last key row is
    dropped or counted twice (more than 4.5 units of atol + rtol |o| everywhere, more than 5 in 99 elements of 100)
  - consecutive 256-row q-tiles (and neighbouring heads) of the chained problem have row maxima more than 100 log2 units
    apart
  - every kind the GPU test runs on a prescaled flavour passes the admission rule: the fp64 result from Q * scale * log2(e)
    rounded to 16 bit stays within a quarter of the tolerance of the oracle
"""
import warnings

import numpy as np
import pytest

import prefill_cases as pc
from oracle import round_to

DTYPES = ["fp16", "bf16"]
DIMS = [64, 128, 256]


def weights(p, b, h, causal):
    sc = pc.scores_log2(p, b, h, causal)
    m = sc.max(axis=1, keepdims=True)
    w = np.exp2(sc - np.where(np.isfinite(m), m, 0.0))
    return sc, w / np.maximum(w.sum(axis=1, keepdims=True), 1e-300)


@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ["spike", "alone"])
def test_spike_carries_all_the_weight(kind, dtype, D):
    for Sq, Sk in pc.SHAPES:
        p = pc.softmax_stress(kind, dtype, D, 1, Sq, Sk)
        assert sorted(set(p.spike.ravel())) == [j for j in pc.SPIKE_ROWS if j < Sk]
        vb = pc.v_bits(p)
        for causal in (False, True):
            o, lse = p.oracle(causal)
            sees = p.sees(causal)
            assert sees.any(axis=2).all() or (causal and Sq < Sk) or kind == "alone"
            for b in range(p.B):
                for h in range(p.Hkv):
                    j = int(p.spike[b, h])
                    sc, w = weights(p, b, h, causal)
                    rows = np.flatnonzero(sees[b, h])
                    assert np.all(w[rows, j].astype(np.float32) == np.float32(1.0)), (Sq, Sk, causal, j)
                    assert np.all(1.0 - w[rows, j] < 2.0 ** -25)
                    # the oracle itself rounds to the bits of V[j*], and its lse is the score of j*
                    got = pc.to_bits16(round_to(o[b, h, rows], dtype), dtype)
                    np.testing.assert_array_equal(got, np.broadcast_to(vb[b, h, j], got.shape))
                    np.testing.assert_allclose(lse[b, h, rows], sc[rows, j] / pc.LOG2E, rtol=1e-6)
                    if causal and kind == "spike":
                        first = j - p.coff                  # the diagonal: row first - 1 must not see j*, row first must
                        if 0 <= first < Sq:
                            assert sees[b, h, first] and np.isfinite(sc[first, j])
                        if 0 <= first - 1 < Sq:
                            assert not sees[b, h, first - 1] and sc[first - 1, j] == -np.inf
                    # every other row: an ordinary softmax (nothing near one-hot) wherever it sees 32 keys or more
                    other = np.flatnonzero(~sees[b, h])
                    other = other[np.isfinite(sc[other]).sum(axis=1) >= 32]
                    assert other.size == 0 or w[other].max() < 0.9


def test_alone_rows_are_alone_in_their_blocks():
    rows = pc.ALONE_ROWS
    assert len({r // 32 for r in rows}) == len(rows)                        # different 32-row blocks
    assert {r % 32 for r in rows} >= {0, 31} and any(0 < r % 32 < 31 for r in rows)      # first, last, middle
    p = pc.softmax_stress("alone", "bf16", 128, 4, 299, 299)
    # a jump of tens of log2 units in the hot rows against neighbours whose scores stay within a few units
    sc = pc.scores_log2(p, 0, 0, False)
    j = int(p.spike[0, 0])
    assert np.all(sc[p.hot, j] - np.delete(sc[p.hot], j, axis=1).max(axis=1) > 40)
    cold = np.setdiff1d(np.arange(p.Sq), p.hot)
    assert np.abs(sc[cold]).max() < 8


@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("tile", [64, 32])
def test_staircase_rises_straddle_the_rescale_threshold(D, tile):
    for dtype in DTYPES:
        p = pc.softmax_stress(f"staircase{tile}", dtype, D, 1, 299, 299)
        c = np.asarray(pc.STAIR64[D] if tile == 64 else pc.stair32(D))
        assert np.array_equal(round_to(c, dtype), c.astype(np.float32))     # exact in 16 bit
        assert np.array_equal(np.abs(p.k[0, 0, :, 0]), c[np.arange(299) // tile].astype(np.float32))
        sc = pc.scores_log2(p, 0, 0, False)[0]
        tmax = np.array([sc[t:t + tile].max() for t in range(0, 299, tile)])
        rise = np.diff(tmax)
        assert len(rise) == (4 if tile == 64 else 9)
        assert np.all((rise[0::2] > 6.5) & (rise[0::2] < 7.5)), rise        # below the threshold of 8
        assert np.all((rise[1::2] > 8.5) & (rise[1::2] < 9.5)), rise        # above it
    if tile == 64:
        want = {64: (7.03, 9.02), 128: (6.89, 8.93), 256: (6.85, 9.02)}[D]
        np.testing.assert_allclose([rise[0], rise[1]], want, atol=0.006)


@pytest.mark.parametrize("D", DIMS)
def test_ramp_moves_the_max_in_every_tile_or_never(D):
    p = pc.softmax_stress("ramp", "bf16", D, 1, 299, 299)
    for h, asc in enumerate([True, False, True, False]):
        sc = pc.scores_log2(p, 0, h, False)
        for tile in (32, 64):
            tmax = np.stack([sc[:, t:t + tile].max(axis=1) for t in range(0, 299, tile)], axis=1)
            run = np.maximum.accumulate(tmax, axis=1)
            if asc:
                assert np.all(np.diff(run, axis=1) > 0)
            else:
                assert np.all(run == tmax[:, :1])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", DIMS)
def test_equal_marks_every_one_row_error(dtype, D):
    """o = the mean of V over the visible rows; the last key row dropped, or counted twice (what a row-clamped load of the
    ragged tile does if the mask lets one duplicate through), moves every element of every row that sees it by
    |+-32 - o| / (Sk +- 1) >= 0.105: more than five times the bf16 atol of 0.016 (the A / Sk = 0.107 against 0.08 that the
    marker was sized by) everywhere.  Counted in whole units atol + rtol |o| the margin is thinner, because |o| itself
    reaches 0.107 + 4 sigma = 0.34 where the marker and the mean of the other rows have the same sign: more than 4.5 units
    in every element (0.0965 at |o| = 0.34) and more than 5 in at least 99 of 100 elements of every row."""
    tol = pc.TOL["bf16"]
    for Sq, Sk in pc.SHAPES:
        p = pc.softmax_stress("equal", dtype, D, 1, Sq, Sk)
        assert np.all(np.abs(p.v[:, :, Sk - 1]) == pc.EQUAL_A)
        for causal in (False, True):
            o, _ = p.oracle(causal)
            n = np.minimum(np.arange(Sq) + p.coff + 1, Sk) if causal else np.full(Sq, Sk)      # visible keys per row
            rows = np.flatnonzero(n == Sk)
            assert rows.size >= 1
            csum = np.cumsum(p.v.astype(np.float64), axis=2)
            assert np.abs(o[:, :, rows] - (csum[:, :, Sk - 1] / Sk)[:, :, None, :]).max() < 1e-6
            last = p.v[:, :, Sk - 1].astype(np.float64)
            for wrong in ((csum[:, :, Sk - 1] - last) / max(Sk - 1, 1), (csum[:, :, Sk - 1] + last) / (Sk + 1)):
                d = np.abs(wrong[:, :, None, :] - o[:, :, rows])
                unit = tol + tol * np.abs(o[:, :, rows])
                assert np.all(d > 5 * tol)
                assert np.all(d > 4.5 * unit)
                assert np.all((d > 5 * unit).mean(axis=-1) >= 0.99)


@pytest.mark.parametrize("shape", pc.CHAINED, ids=lambda s: "b%d_hq%d_hkv%d_sq%d_sk%d" % s)
def test_chained_q_tiles_alternate(shape):
    p = pc.chained("bf16", shape)
    nq = p.Sq // 256
    for causal in (False, True):
        tops = np.full((p.Hq, nq), np.nan)
        for h in range(p.Hq):
            m = pc.scores_log2(p, 0, h, causal).max(axis=1).reshape(nq, 256)
            m = np.where(np.isfinite(m), m, np.nan)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", RuntimeWarning)                 # q-tiles without a key: all NaN
                lo, hi = np.nanmin(m, axis=1), np.nanmax(m, axis=1)
            seen = ~np.isnan(hi)
            assert np.all(np.sign(lo[seen]) == np.sign(hi[seen])) and np.all(np.sign(hi[seen]) == p.sign[h, ::256][seen])
            tops[h] = np.where(p.sign[h, ::256] > 0, lo, hi)                # the row max nearest to zero
        assert np.isfinite(tops).any()
        d = np.concatenate([np.abs(tops[:, 1:] - tops[:, :-1]).ravel(), np.abs(tops[1:] - tops[:-1]).ravel()])
        d = d[np.isfinite(d)]                                               # next q-tile, next head: where both see a key
        assert d.size >= p.Hq - 1 and d.min() > 100, d.min()


_PRESCALED = sorted({(dt, D) for impl, D, dt, _ in pc.CONFIGS if pc.flavour(impl) == "prescaled"})


def admission_excess(p, causal):
    """max over o and lse of |prescaled_reference - oracle| / (tol + tol |oracle|): the admission rule wants <= 0.25"""
    o, lse = p.oracle(causal)
    po, plse = pc.prescaled_reference(p, causal)
    fin = np.isfinite(lse)
    assert np.array_equal(fin, np.isfinite(plse))
    t, lt = pc.TOL[p.dtype], pc.LSE_TOL["prescaled"][p.dtype]
    eo = (np.abs(po - o) / (t + t * np.abs(o))).max()
    el = (np.abs(plse[fin] - lse[fin]) / (lt + lt * np.abs(lse[fin]))).max() if fin.any() else 0.0
    return max(eo, el)


@pytest.mark.parametrize("dtype,D", _PRESCALED)
@pytest.mark.parametrize("kind", pc.PRESCALED_KINDS)
def test_prescaled_admission(kind, dtype, D):
    """(at group size 1: a larger group adds query heads of the same distribution)"""
    assert set(pc.PRESCALED_KINDS) | set(pc.PRESCALED_LEFT_OUT) == set(pc.KINDS) and not set(pc.PRESCALED_KINDS) & set(pc.PRESCALED_LEFT_OUT)
    for Sq, Sk in pc.SHAPES:
        p = pc.softmax_stress(kind, dtype, D, 1, Sq, Sk)
        for causal in (False, True):
            assert admission_excess(p, causal) <= 0.25, (Sq, Sk, causal)


@pytest.mark.parametrize("dtype,D", _PRESCALED)
def test_prescaled_admission_of_softmax_scale(dtype, D):
    """Section B's problem: admitted at softmax_scale 0.03, full and causal.  At 0.5 it is not, at either group size, full
    or causal: the fp64 result from the rounded Q is by itself 0.95 to 2.3 tolerances away from the oracle, more than one
    whole tolerance in every full-attention case."""
    assert pc.SCALES == (0.03, 0.5) and pc.PRESCALED_SCALES == (0.03,)
    for G in (1, 4):
        p = pc.normal_problem(dtype, D, G, 299, 299)
        for causal in (False, True):
            o, lse = p.oracle(causal, 0.03)
            po, plse = pc.prescaled_reference(p, causal, 0.03)
            t, lt = pc.TOL[dtype], pc.LSE_TOL["prescaled"][dtype]
            assert (np.abs(po - o) / (t + t * np.abs(o))).max() <= 0.25
            assert (np.abs(plse - lse) / (lt + lt * np.abs(lse))).max() <= 0.25
        for causal in (False, True):
            o, _ = p.oracle(causal, 0.5)
            po, _ = pc.prescaled_reference(p, causal, 0.5)
            excess = (np.abs(po - o) / (t + t * np.abs(o))).max()
            assert excess > 0.25 and (causal or excess > 1.0), (G, causal, excess)


def test_prescaled_admission_of_the_chained_problem():
    dtypes = {dt for impl, D, dt, _ in pc.CONFIGS if impl == "prescaled_w4"}
    for dtype in dtypes:
        for shape in pc.CHAINED:
            p = pc.chained(dtype, shape)
            for causal in (False, True):
                assert admission_excess(p, causal) <= 0.25, (shape, causal)


def test_configurations_cover_the_issue():
    impls = {(i, D) for i, D, _, _ in pc.CONFIGS}
    assert impls == {(i, 128) for i in ("w4", "prescaled_w4", "rows256", "rows256x2", "rows128", "prescaled256",
                                        "prescaled128", "auto")} | {(i, 64) for i in ("rows256", "rows128", "prescaled128")} | \
        {("auto", 256), ("d256_fallback", 256)}
    family = lambda i, D: "d256" + i if D == 256 else "w4" if i.endswith("w4") else "128" if i.endswith("128") else \
        "auto" if i == "auto" else "8w"
    for fam in {family(i, D) for i, D in impls} - {"auto"}:
        seen = {(dt, G) for i, D, dt, G in pc.CONFIGS if family(i, D) == fam}
        assert {dt for dt, _ in seen} == {"fp16", "bf16"} and {G for _, G in seen} == {1, 4}, fam
    for i, D, _, _ in pc.CONFIGS:
        ks = pc.stress_kinds(i, D)
        assert ("staircase32" in ks) == (pc.key_tile(i, D) == 32)
