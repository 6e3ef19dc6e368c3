"""The problems of tests/prefill_window_cases.py have the structure tests/test_prefill_window_numerics_gpu.py relies on --
proved from the fp64 reference alone, no GPU.  Every item is a condition on the inputs:

  - spike / alone: under every window some row sees the spike; in every such row the spike's weight without a sink is 1.0
    in fp32 and every other weight at most 2^-40; for every window below Sk some row has the spike one key below its lower
    bound and some row one key above its limit, and letting the key below in (window + 1) moves the row by more than ten
    tolerances, so a leak cannot hide
  - staircase64_down: the same for every row whose lower bound lies on a tile edge; the ascending staircase shows that leak
    in no row at all at windows 65 and 150 (it is no lower-mask test)
  - the sinks of sinks_for are material -- a share of 0.05 to 0.95 -- in at least a tenth of the rows that have a key, for
    every kind, configuration, shape and window; the rows of "spike" and "alone" that must still return V[spike] under
    these sinks are those where the sink's share is at most 2^-25, and there the reference itself rounds to V[spike]
  - CONFIGS_W x {no sink, sinks} are the eight template instances, a window >= Sk runs only with sinks, and no parametrized
    GPU case launches more than 40 kernels
"""
import numpy as np
import pytest

import prefill_cases as pc
import prefill_window_cases as wc
from oracle import round_to
from oracle.numerics import to_bits16
from prefill_window_ref import prefill_window_ref, window_mask

CFG = pytest.mark.parametrize("cfg", wc.CONFIGS_W, ids=wc.config_id)
_problems = {}


def problem(kind, cfg, shape):
    """shared by the tests of this file (the most recent 4: the references live in the problems)"""
    key = (kind, cfg, shape)
    if key not in _problems:
        while len(_problems) >= 4:
            del _problems[next(iter(_problems))]
        D, dtype, G = cfg
        _problems[key] = wc.stress_w(kind, dtype, D, G, *shape)
    return _problems[key]


def slot_ref(p, b, hk, window):
    """o [G, Sq, D] of the query heads of one (batch, kv head) slot under `window`, no sink"""
    o, _ = prefill_window_ref(p.q[b:b + 1, hk * p.G:(hk + 1) * p.G], p.k[b:b + 1, hk:hk + 1], p.v[b:b + 1, hk:hk + 1], window)
    return o[0].astype(np.float64)


def leak_shows(p, b, hk, window, rows):
    """[G, len(rows)] bool: the key one below the lower bound, let in (window + 1), moves some element of the row by more
    than 10 TOL (1 + |o|)"""
    o, o1 = slot_ref(p, b, hk, window)[:, rows], slot_ref(p, b, hk, window + 1)[:, rows]
    return (np.abs(o1 - o) > 10 * wc.TOL[p.dtype] * (1 + np.abs(o))).any(axis=-1)


@CFG
@pytest.mark.parametrize("kind", ["spike", "alone"])
def test_spike_carries_all_the_weight_of_the_rows_that_see_it(kind, cfg):
    for shape in wc.SHAPES:
        p = problem(kind, cfg, shape)
        assert sorted(set(p.spike.ravel())) == wc.spike_rows_w(*shape)
        for b in range(p.B):
            for hk in range(p.Hkv):
                j = int(p.spike[b, hk])
                for h in range(hk * p.G, (hk + 1) * p.G):
                    full = pc.scores_log2(p, b, h, False)
                    for window in wc.WINDOWS:
                        rows = np.flatnonzero(wc.sees_w(p, window)[b, hk])
                        if rows.size == 0:
                            continue
                        sc = np.where(window_mask(p.Sq, p.Sk, window), full, -np.inf)[rows]
                        w = np.exp2(sc - sc.max(axis=1, keepdims=True))
                        w /= w.sum(axis=1, keepdims=True)
                        assert np.all(w[:, j].astype(np.float32) == np.float32(1.0)), (shape, window, j)
                        assert np.delete(w, j, axis=1).max() <= 2.0 ** -40, (shape, window, j)
        for window in wc.WINDOWS:
            assert wc.sees_w(p, window).any(), (shape, window)


@CFG
@pytest.mark.parametrize("kind", ["spike", "alone"])
def test_some_row_has_the_spike_one_key_outside_its_window(kind, cfg):
    for shape in wc.SHAPES:
        p = problem(kind, cfg, shape)
        hot = np.ones(p.Sq, bool) if p.hot is None else np.isin(np.arange(p.Sq), p.hot)
        for window in wc.windows_for(p.Sk, False):
            lo, lim = wc.lo_lim(p, window)
            below = (p.spike[:, :, None] == lo - 1) & hot          # (a spike is >= 0, so lo_i > 0 in these rows)
            above = (p.spike[:, :, None] == lim + 1) & hot & (lim >= 0)
            assert below.any() and above.any(), (shape, window)
            assert not (wc.sees_w(p, window) & (below | above)).any()
            for b, hk in zip(*np.nonzero(below.any(axis=2))):
                assert leak_shows(p, b, hk, window, np.flatnonzero(below[b, hk])).all(), (shape, window, b, hk)


@CFG
def test_descending_staircase_shows_a_key_below_the_window_and_the_ascending_one_does_not(cfg):
    seen = {w: [] for w in (65, 150)}
    for shape in wc.SHAPES:
        down, up = problem("staircase64_down", cfg, shape), problem("staircase64", cfg, shape)
        c = np.asarray(pc.STAIR64[cfg[0]])
        for b, hk in np.ndindex(down.B, down.Hkv):
            assert np.array_equal(np.abs(down.k[b, hk, :, 0]), c[::-1][np.arange(down.Sk) // 64].astype(np.float32))
        for window in wc.windows_for(down.Sk, False):
            lo, lim = wc.lo_lim(down, window)
            edge = np.flatnonzero((lo > 0) & (lo % 64 == 0) & (lim >= 0))
            if edge.size:
                sc = pc.scores_log2(down, 0, 0, False)
                vis = np.where(window_mask(down.Sq, down.Sk, window), sc, -np.inf)[edge].max(axis=1)
                rise = sc[edge, lo[edge] - 1] - vis
                assert np.all((rise > 6.5) & (rise < 9.5)), rise
                for b, hk in np.ndindex(down.B, down.Hkv):
                    assert leak_shows(down, b, hk, window, edge).all(), (shape, window)
            if window in seen:
                rows = np.flatnonzero((lo > 0) & (lim >= 0))
                seen[window] += [leak_shows(up, b, hk, window, rows).ravel() for b, hk in np.ndindex(up.B, up.Hkv)]
        assert any(((lo > 0) & (lo % 64 == 0) & (lim >= 0)).any() for lo, lim in
                   (wc.lo_lim(down, w) for w in wc.windows_for(down.Sk, False)))
    for window, s in seen.items():
        s = np.concatenate(s)
        assert s.size > 100 and not s.any(), (window, s.mean())         # blind: the ascending kind is no lower-mask test


@CFG
@pytest.mark.parametrize("kind", wc.KINDS_W)
def test_sinks_are_material(kind, cfg):
    lowest = 1.0
    for shape in wc.SHAPES:
        p = problem(kind, cfg, shape)
        for window in wc.windows_for(p.Sk, True):
            sinks = wc.sinks_for(p, window)
            assert sinks.dtype == np.float32 and sinks.shape == (p.Hq,) and np.isfinite(sinks).all()
            share = wc.sink_share(p, window, sinks)
            has = np.isfinite(share)
            assert np.array_equal(has, np.broadcast_to((wc.lo_lim(p, window)[1] >= 0), has.shape))
            frac = ((share[has] >= 0.05) & (share[has] <= 0.95)).mean()
            lowest = min(lowest, frac)
            assert frac >= 0.10, (shape, window, frac)
            if kind in ("spike", "alone"):
                # the rows held to the bits of V[spike] under these sinks: the reference itself rounds to them
                exact = wc.exact_rows_w(p, window, sinks)
                sees = np.repeat(wc.sees_w(p, window), p.G, axis=1)
                assert not (exact & ~sees).any()
                assert np.all(share[sees & ~exact] > wc.EXACT_SHARE)
                o, _ = wc.oracle_w(p, window, sinks)
                want = np.repeat(pc.v_bits(p)[np.arange(p.B)[:, None], np.arange(p.Hkv)[None, :], p.spike], p.G, axis=1)
                got = to_bits16(round_to(o, p.dtype), p.dtype)
                np.testing.assert_array_equal(got[exact], np.broadcast_to(want[:, :, None, :], got.shape)[exact])
        if kind in ("spike", "alone"):
            # ... and under the shortest window they are there at every shape
            assert wc.exact_rows_w(p, wc.WINDOWS[0], wc.sinks_for(p, wc.WINDOWS[0])).any(), shape
    print(f"{kind} {wc.config_id(cfg)}: lowest material fraction {lowest:.2f}")


def test_sinks_of_the_normal_problems_are_material():
    """sections B and C: N(0,1) data, the windows of GUARD_WINDOWS.  At the one-row shapes one row per head has a key, and
    the sink's share of it in batch 0 is sigmoid(delta_h) itself, 0.047 to 0.953."""
    for D, dtype, G in wc.CONFIGS_W:
        for shape in wc.SHAPES + wc.ONE_ROW_SHAPES:
            p = wc.normal_problem(dtype, D, G, *shape)
            for window in wc.windows_for(p.Sk, True, wc.GUARD_WINDOWS):
                share = wc.sink_share(p, window, wc.sinks_for(p, window))
                has = np.isfinite(share)
                if shape in wc.ONE_ROW_SHAPES:
                    np.testing.assert_allclose(share[0, :, -1], wc.sigmoid(wc.deltas(p.Hq)), atol=1e-5)
                else:
                    assert ((share[has] >= 0.05) & (share[has] <= 0.95)).mean() >= 0.10, (shape, window)


def test_sinks_for_anchors_on_a_row():
    """The anchor is the lse of a row (np.median of an even number of rows is the mean of two, and between two steps of a
    staircase lies no row).  On the ascending staircase at head_dim 128, (100, 299), window 1 -- 57 rows on one step, 43 on
    the next, each row its one key -- the sink's share of a row on the anchor's step is sigmoid(delta_h) exactly: with the
    two heads of prefill_cases' staircase that is 0.047 or 0.953 and material nowhere, hence the four slots of stress_w."""
    p = wc.stress_w("staircase64", "bf16", 128, 1, 100, 299)
    assert p.Hq == 4
    two = pc.softmax_stress("staircase64", "bf16", 128, 1, 100, 299)
    assert np.array_equal(p.k[:, :2], two.k) and np.array_equal(p.q[:, :2], two.q) and np.array_equal(p.v[:, :2], two.v)
    _, lse = wc.oracle_w(p, 1)
    sinks = wc.sinks_for(p, 1)
    anchors = sinks.astype(np.float64) - wc.deltas(p.Hq)
    for h in range(p.Hq):
        fin = np.sort(lse[0, h].astype(np.float64))
        assert abs(fin[fin.size // 2] - anchors[h]) < 1e-5 and np.abs(lse[0, h] - anchors[h]).min() < 1e-5
    share = wc.sink_share(two, 1, wc.sinks_for(two, 1))
    assert not ((share >= 0.05) & (share <= 0.95)).any()
    assert np.isclose(share[0, 0], wc.sigmoid(-3.0), atol=1e-3).sum() >= 43         # the rows of the anchor's step
    assert np.isclose(share[0, 1], wc.sigmoid(3.0), atol=1e-3).sum() >= 43


def test_configurations_reach_every_instance():
    inst = {wc.instance(c, s) for c in wc.CONFIGS_W for s in wc.SINKS}
    assert inst == {(dt, D, s) for dt in ("fp16", "bf16") for D in (64, 128) for s in (False, True)}
    assert {G for _, _, G in wc.CONFIGS_W} == {1, 4}
    assert wc.WINDOWS == (1, 40, 65, 150) and set(wc.GUARD_WINDOWS) <= set(wc.WINDOWS)
    assert wc.KINDS_W == ["spike", "alone", "staircase64", "staircase64_down", "ramp", "equal", "below"]
    for sinks in wc.SINKS:
        for (Sq, Sk), window in wc.stress_runs(sinks) + wc.guard_runs(sinks):
            assert window < Sk or sinks
        assert {s for s, _ in wc.stress_runs(sinks)} == set(wc.SHAPES)
    assert {s for s, _ in wc.guard_runs(True)} == set(wc.SHAPES + wc.ONE_ROW_SHAPES)
    # every admitted pair is there: all windows with sinks, those below Sk without
    assert len(wc.stress_runs(True)) == len(wc.SHAPES) * len(wc.WINDOWS)
    assert len(wc.stress_runs(False)) == sum(w < Sk for _, Sk in wc.SHAPES for w in wc.WINDOWS)


def test_launch_budget():
    for section in ("A", "B", "guarded", "stride0", "empty"):
        for sinks in wc.SINKS:
            assert wc.launches(section, sinks) <= wc.MAX_LAUNCHES, (section, sinks, wc.launches(section, sinks))
