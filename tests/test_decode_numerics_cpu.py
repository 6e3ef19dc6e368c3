"""The structured problems of tests/decode_cases.py have the structure they are named for -- checked against the fp64
oracle alone, so that a pass of tests/test_decode_numerics_gpu.py means what it says.  No GPU."""
import numpy as np
import pytest

import decode_cases as dc
import kv8_ref

# every (entry, G, D, dtype) the GPU file runs
SHAPES = sorted({(c[0], c[1], c[2], c[4]) for c in dc.CONFIGS})
ids = lambda s: f"{s[0]}-G{s[1]}-D{s[2]}-{s[3]}"


@pytest.fixture(scope="module")
def built():
    cache = {}

    def get(entry, G, D, dtype, kind):
        key = (entry, G, D, dtype, kind)
        if key not in cache:
            p = dc.softmax_stress(entry, dtype, G, D, kind)
            cache[key] = (p, dc.oracle(p))
        return cache[key]
    return get


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_spikes_carry_the_weight(built, shape):
    """Every token that is meant to see a spike gives it >= 0.99 of the weight in every head (all but 2^-30 of it where
    the GPU test asks for the bits of v: that is 1.0 in fp32); a token in front of a spike among the new tokens gives it
    less than 1e-6 -- and would give it >= 0.99 if the causal mask let it through, so a leak cannot hide."""
    entry = shape[0]
    kinds = [k for k in dc.stress_kinds(entry) if k in ("spike", "below", "chunk_spike")]
    seen_hot = seen_front = 0
    for kind in kinds:
        p, ref = built(*shape, kind)
        assert np.isfinite(ref["o"]).all()
        for r in range(p.T):
            b, t = p.seq_of(r)
            if p.spike[b] < 0:
                assert p.hot[r] < 0
                continue
            w = dc.weights(p, ref, r)[:, p.spike[b]]
            if p.hot[r] >= 0:
                assert p.hot[r] == p.spike[b] <= p.lens[b] + t
                assert w.min() >= 0.99, (kind, r, w.min())
                if p.exact[r]:
                    assert 1.0 - w.min() <= 2.0 ** -30, (kind, r, 1.0 - w.min())
                seen_hot += 1
            else:
                assert p.spike[b] > p.lens[b] + t and w.max() < 1e-6
                assert dc.weights(p, ref, r, causal=False)[:, p.spike[b]].min() >= 0.99
                seen_front += 1
    assert seen_hot > 0 and (entry in ("decode", "kv8", "window") or seen_front > 0)


@pytest.mark.parametrize("shape", [s for s in SHAPES if s[0] != "window"], ids=ids)     # (window: the window-edge ramps)
def test_ramps_move_the_max_as_named(built, shape):
    """Ascending: the row max over 32-key tiles strictly increases from tile to tile (every tile rescales); descending:
    it is attained in tile 0 (no later tile rescales).  Seen from the last token of each sequence, in every head."""
    p, ref = built(*shape, "ramp")
    seen = set()
    for b in range(p.B):
        if p.ramp[b] == 0:
            continue
        sc = dc.scores_log2(p, ref, p.cu[b + 1] - 1)                       # [H, pos + n]
        nk = sc.shape[1]
        tiles = np.stack([sc[:, t:t + 32].max(axis=1) for t in range(0, nk, 32)], axis=1)
        if p.ramp[b] > 0:
            assert np.all(np.diff(tiles, axis=1) > 0), (b, tiles)
            assert nk <= 32 or np.all(tiles[:, -1] - tiles[:, 0] > 8)       # by far more than one unit a tile
        else:
            assert np.all(tiles.argmax(axis=1) == 0), (b, tiles)
        seen.add(p.ramp[b])
    assert seen == {1, -1}


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_extreme_logits_are_extreme(built, shape):
    p, ref = built(*shape, "extreme")
    assert np.isfinite(ref["o"]).all()
    for b in range(p.B):
        if p.ns[b]:
            sc = dc.scores_log2(p, ref, p.cu[b + 1] - 1)[:, p.lo[b]:]         # (the keys its last token sees)
            assert np.abs(sc).max() >= 100.0


@pytest.mark.parametrize("shape", [s for s in SHAPES if s[0] not in ("varlen", "window")], ids=ids)
def test_equal_keys_give_the_mean_of_v(built, shape):
    p, ref = built(*shape, "equal")
    for r in range(p.T):
        b, t = p.seq_of(r)
        V = np.repeat(p.values(ref["vc"][b, dc.LAYER, :p.lens[b] + t + 1], p.vs), p.G, axis=1)
        np.testing.assert_allclose(ref["o"][r], V.mean(axis=0), atol=1e-6, rtol=1e-6)


@pytest.mark.parametrize("shape", [s for s in SHAPES if s[0] == "kv8"], ids=ids)
def test_e4m3_new_tokens_survive_quantisation(built, shape):
    """The cached rows reach the oracle as codes; of the new token, v (multiples of 1/8 in [-2, 2] over a power-of-two
    scale) always survives q8 and back unchanged, and so does k where the output must be exact."""
    for kind in dc.stress_kinds("kv8"):
        p, ref = built(*shape, kind)
        assert np.all(np.log2(p.ks) % 1 == 0) and np.all(np.log2(p.vs) % 1 == 0) and p.ks[0] != p.ks[1]
        np.testing.assert_array_equal(kv8_ref.dequantize(kv8_ref.quantize(p.v_new, p.vs), p.vs), p.v_new)
        if p.exact.any():
            k = p.k_new[p.exact]
            np.testing.assert_array_equal(kv8_ref.dequantize(kv8_ref.quantize(k, p.ks), p.ks), k)
        for b in range(p.B):                       # what the oracle appended is what the problem said
            np.testing.assert_array_equal(p.values(ref["vc"][b, dc.LAYER, p.lens[b]], p.vs), p.v_new[b])


@pytest.mark.parametrize("shape,pattern", [(s, pat) for s in SHAPES for pat in ("nan", "inf") if (s[0], pat) != ("kv8", "inf")],
                         ids=lambda x: x if isinstance(x, str) else ids(x))          # (e4m3 has no infinity)
def test_poison_is_outside_the_contract(shape, pattern):
    """The poisoned problem differs from the clean one in every byte outside rows 0 .. pos + n - 1 of idx_layer and in
    no other; the oracle does not see the difference.  A window: rows lo .. pos, at each window of section C; the rows
    below lo hold the sequence's N(0,1) data in the clean problem, every other byte outside the contract zeros."""
    entry = shape[0]
    for window in dc.UNREAD_WINDOWS if entry == "window" else (None,):
        _poison_is_outside_the_contract(shape, pattern, window)


def _poison_is_outside_the_contract(shape, pattern, window):
    entry, G, D, dtype = shape
    clean = dc.normal_problem(entry, dtype, G, D, window=window)
    bad = clean.poisoned(None if pattern == "nan" else dc.INF16[dtype])
    m = clean.unread_mask()
    zeros = m.copy()
    for b in range(clean.B):
        zeros[b, dc.LAYER, :clean.lo[b]] = False
    assert entry != "window" or (m != zeros).any()
    for c, x in ((clean.kc, bad.kc), (clean.vc, bad.vc)):
        assert np.all(c[zeros] == 0) and np.all(x[m] != c[m]) and np.array_equal(x[~m], c[~m])
        assert not np.isfinite(bad.values(x[m])).any()
    for b in range(clean.B):
        lo, end = clean.lo[b], clean.lens[b] + clean.ns[b]
        assert lo == (0 if window is None else max(0, clean.lens[b] + 1 - window))
        assert not m[b, dc.LAYER, lo:end].any() and m[b, dc.LAYER, end:].all() and m[b, dc.LAYER, :lo].all()
        assert m[b, 1 - dc.LAYER].all()
    a, z = dc.oracle(clean), dc.oracle(bad)
    assert np.isfinite(z["o"]).all()
    np.testing.assert_array_equal(z["o"], a["o"])
    np.testing.assert_array_equal(z["kc"][~m], a["kc"][~m])
    np.testing.assert_array_equal(z["vc"][~m], a["vc"][~m])
    np.testing.assert_array_equal(z["kc"][m], bad.kc[m])


def test_the_issue_s_coverage_table():
    have = {(c[0], c[1], c[2], c[3]) for c in dc.CONFIGS}
    want = [("decode", 1, 64, "blmhd"), ("decode", 1, 128, "blmhd"), ("decode", 1, 128, "blhmd"), ("decode", 1, 128, "paged"),
            ("decode", 1, 256, "blmhd"), ("decode", 2, 128, "blmhd"), ("kv8", 1, 128, "blmhd"), ("kv8", 16, 128, "blmhd"),
            ("kv8", 2, 64, "blmhd")]
    want += [("decode", G, D, lay) for G, D in ((4, 128), (8, 64), (8, 256), (16, 128)) for lay in ("blhmd", "blmhd", "paged")]
    want += [("kv8", 4, 128, lay) for lay in ("blhmd", "blmhd", "paged")]
    want += [(e, G, D, lay) for e in ("chunk", "varlen") for D in (64, 128) for G in (1, 8) for lay in ("blmhd", "paged")]
    assert set(want) <= have
    assert any(c[:3] == ("decode", 4, 64) for c in dc.CONFIGS)
    assert any(c[:3] == ("decode", 8, 128) and c[5].get("decode_gqa_mfma") == 0 for c in dc.CONFIGS)
    for entry in ("decode", "kv8", "chunk", "varlen", "window"):
        mine = [c for c in dc.CONFIGS if c[0] == entry]
        assert {c[4] for c in mine} == {"fp16", "bf16"}
    for kernel in ([c for c in dc.CONFIGS if c[0] == "kv8"], [c for c in dc.CONFIGS if c[:2] == ("decode", 1)],
                   [c for c in dc.CONFIGS if c[:3] == ("decode", 8, 64)], [c for c in dc.CONFIGS if c[:3] == ("decode", 4, 64)]):
        assert any(c[5].get("decode_nt") == 1 for c in kernel)          # (the chunk body has no non-temporal loads)
    assert dc.SPIKE_ROWS[-1] == 199 and dc.VARLEN_NS == [1, 3, 40, 0, 17]


# ---------------------------------------------------------------------------------------------------------------------
# the sliding window: the window-edge problems, from the oracle alone
# ---------------------------------------------------------------------------------------------------------------------

WINDOW_SHAPES = [s for s in SHAPES if s[0] == "window"]
EDGES = [(s, w) for s in WINDOW_SHAPES for w in dc.WINDOWS]
edge_ids = lambda x: ids(x) if isinstance(x, tuple) else f"w{x}"


@pytest.fixture(scope="module")
def edges():
    cache = {}

    def get(shape, kind, window):
        key = (shape, kind, window)
        if key not in cache:
            p = dc.window_edges(shape[3], shape[1], shape[2], kind, window)
            cache[key] = (p, dc.oracle(p))
        return cache[key]
    return get


def elementwise_tol(p, want):
    """what the GPU file allows per element: atol = rtol"""
    return dc.TOL[p.dtype] * (1.0 + np.abs(want))


def test_window_edge_sequences_cover_the_alignments():
    """pos = lo + window - 1 for every sequence (row lo - 1 is the first one outside); per window, a sequence for each
    of lo & 31 in {0 with lo != 0, 1, 15, 16, 17, 31} (no masked key in the first tile; masked rows that end on or beside
    the 16-row half that decides the two page offsets), a non-zero lo on a page boundary, and lo = 0."""
    assert dc.WINDOWS == (17, 32, 40, 100) and dc.EDGE_KINDS == ["edge_in", "edge_last", "edge_out", "ramp_through", "equal"]
    assert dc.WINDOW_LOS == [0, 1, 15, 16, 17, 31, 32, 33, 48, 63, 64, 65, 96, 127, 128, 129, 156]
    for window in dc.WINDOWS:
        for kind in dc.EDGE_KINDS:
            los = dc.window_los(window, kind)
            assert los == [lo for lo in dc.WINDOW_LOS if lo + window <= dc.M and (kind != "edge_out" or lo > 0)]
            for r in (0, 1, 15, 16, 17, 31):
                assert any(lo & 31 == r and lo > 0 for lo in los), (window, kind, r)
            assert any(lo > 0 and lo % dc.PS == 0 for lo in los) and (kind == "edge_out" or 0 in los)
            p = dc.window_edges("fp16", 1, 64, kind, window)
            per_lo = 2 if kind == "ramp_through" else 1
            assert p.window == window and p.lo == [lo for lo in los for _ in range(per_lo)]
            assert p.lens == [lo + window - 1 for lo in p.lo] and max(p.lens) <= dc.M - 1 and p.ns == [1] * p.B


@pytest.mark.parametrize("shape,window", EDGES, ids=edge_ids)
def test_window_edge_spikes_carry_the_weight(edges, shape, window):
    """edge_in: row lo, edge_last: row pos - 1 (a cached row) has all but 1e-6 of the fp64 weight in every head."""
    for kind, row_of in (("edge_in", lambda lo, pos: lo), ("edge_last", lambda lo, pos: pos - 1)):
        p, ref = edges(shape, kind, window)
        assert np.isfinite(ref["o"]).all()
        for b in range(p.B):
            row = row_of(p.lo[b], p.lens[b])
            assert p.hot[b] == p.spike[b] == row and p.lo[b] <= row < p.lens[b]
            assert dc.weights(p, ref, b)[:, row].min() >= 1.0 - 1e-6, (kind, b)
            v = np.repeat(p.values(p.vc[b, dc.LAYER, row]), p.G, axis=0)
            assert np.all(np.abs(ref["o"][b] - v) <= 0.01 * elementwise_tol(p, v))       # o is that row of V


@pytest.mark.parametrize("shape,window", EDGES, ids=edge_ids)
def test_window_edge_out_would_show(edges, shape, window):
    """edge_out: row lo - 1 holds finite bits, has no weight, and a kernel that saw it would be wrong by more than 10
    times the elementwise tolerance in at least half of the elements of every sequence."""
    p, ref = edges(shape, "edge_out", window)
    seen = dc.oracle(p, window=window + 1)["o"]                                # the oracle over [lo - 1, pos]
    for b in range(p.B):
        lo = p.lo[b]
        assert lo >= 1 and p.spike[b] == lo - 1 and p.hot[b] == -1
        for c in (p.kc, p.vc):
            assert np.isfinite(p.values(c[b, dc.LAYER, lo - 1])).all()
        assert dc.weights(p, ref, b)[:, lo - 1].max() == 0.0
        assert dc.weights(p, ref, b, causal=False)[:, lo - 1].min() >= 0.99
        far = np.abs(seen[b] - ref["o"][b]) > 10 * elementwise_tol(p, ref["o"][b])
        assert far.mean() >= 0.5, (b, far.mean())


@pytest.mark.parametrize("shape,window", EDGES, ids=edge_ids)
def test_window_equal_marks_every_one_row_error(edges, shape, window):
    """equal: o is the mean of V over exactly rows lo .. pos, and each one-row error -- row lo dropped, row lo counted
    twice, row lo - 1 added, row pos - 1 dropped -- differs from it by more than 5 times the elementwise tolerance in at
    least half of the elements, for every sequence.  A condition on the inputs (decode_cases.equal_magnitude)."""
    p, ref = edges(shape, "equal", window)
    seen = 0
    for b in range(p.B):
        lo, pos = p.lo[b], p.lens[b]
        V = np.repeat(p.values(ref["vc"][b, dc.LAYER, :pos + 1]), p.G, axis=1)             # [pos + 1, H, D]
        want = ref["o"][b]
        np.testing.assert_allclose(want, V[lo:].mean(axis=0), atol=1e-6, rtol=1e-6)
        rows = list(range(lo, pos + 1))
        wrong = {"lo dropped": rows[1:], "lo twice": [lo] + rows, "pos - 1 dropped": rows[:-2] + rows[-1:]}
        if lo >= 1:
            wrong["lo - 1 added"] = [lo - 1] + rows
        for name, rr in wrong.items():
            far = np.abs(V[rr].mean(axis=0) - want) > 5 * elementwise_tol(p, want)
            assert far.mean() >= 0.5, (name, b, far.mean())
            seen += 1
    assert seen == 4 * p.B - 1                                                   # (lo = 0 has no row below it)


@pytest.mark.parametrize("shape,window", EDGES, ids=edge_ids)
def test_window_ramps_are_as_named(edges, shape, window):
    """ramp_through, the ramp that goes on below lo: the largest score of [lo, pos] is at row lo in every head, and every
    row below lo scores higher than row lo.  The ascending one: the row max over the 32-key tiles of the window
    (measured from lo & ~31, as the kernel cuts them) strictly increases, and the rows below lo are zeros."""
    p, ref = edges(shape, "ramp_through", window)
    seen = set()
    for b in range(p.B):
        lo, pos = p.lo[b], p.lens[b]
        sc = dc.scores_log2(p, ref, b, causal=False)                           # [H, pos + 1], nothing masked
        if p.ramp[b] < 0:
            assert np.all(sc[:, lo:].argmax(axis=1) == 0)
            assert np.all(sc[:, :lo] > sc[:, lo:lo + 1])
            assert np.all(np.diff(sc[:, lo:], axis=1) < 0)                     # (far below lo, bf16 steps tie)
        else:
            assert not p.kc[b, dc.LAYER, :lo].any()
            masked = dc.scores_log2(p, ref, b)
            base = lo & ~31
            tiles = np.stack([masked[:, t:t + 32].max(axis=1) for t in range(base, pos + 1, 32)], axis=1)
            assert tiles.shape[1] >= 2 or window <= 32 - (lo & 31)
            assert np.all(np.diff(tiles, axis=1) > 0), (b, tiles)
        seen.add(p.ramp[b])
    assert seen == {1, -1}


def test_window_configurations_cover_the_kernel():
    """decode_window_kernel's instantiations: every (head_dim, layout) pair, every group size at least twice (1 and 2,
    the padded query columns, on each load path), both dtypes, non-temporal loads forced once per load path."""
    w = [c for c in dc.CONFIGS if c[0] == "window"]
    assert 12 <= len(w) <= 18 and len({c[:5] for c in w}) == len(w)
    assert {(c[2], c[3]) for c in w} == {(D, lay) for D in (64, 128, 256) for lay in ("blhmd", "blmhd", "paged")}
    for G in (1, 2, 4, 8, 16):
        assert sum(c[1] == G for c in w) >= 2
    for G in (1, 2):
        assert {c[3] for c in w if c[1] == G} == {"blhmd", "blmhd", "paged"}
    assert {c[4] for c in w} == {"fp16", "bf16"} and all(a[4] != b[4] for a, b in zip(w, w[1:]))
    nt = [c for c in w if c[5].get("decode_nt") == 1]
    assert len(nt) == 3 and {c[3] for c in nt} == {"blhmd", "blmhd", "paged"}
    assert all(c[5] in ({}, {"decode_nt": 1}) for c in w)
    assert dc.stress_kinds("window") == ["below", "extreme"] and dc.STRESS_WINDOW == 40 and dc.UNREAD_WINDOWS == (40, 16, 1)
    assert (dc.M, dc.L, dc.PS) == (256, 2, 16)
    for window, at in ((16, (15, 31, 63)), (1, (1, 15, 33))):       # section C: lo on a page boundary; lo = pos off a tile boundary
        p = dc.normal_problem("window", "fp16", 1, 64, window=window)
        for pos in at:
            lo = p.lo[p.lens.index(pos)]
            assert lo == pos + 1 - window and (lo % dc.PS == 0 if window == 16 else lo % 32 != 0)


# ---------------------------------------------------------------------------------------------------------------------
# a model of decode_window_kernel's addressing, and what one-line slips of it do to the window-edge problems
# ---------------------------------------------------------------------------------------------------------------------

def window_model(p, slip=None, paged=False):
    """fp64 attention over the key slots as decode_window_kernel addresses them at num_splits = 1: tiles of 32 keys from
    lo & ~31 up to pos, a slot is real if key < pos - t and key >= lo - t, its row is min(max(row, lo), pos - 1), and
    (paged, page size 16) its page index min(max(index of the tile's 16-row half, lo's page), the last page).  slip:
    "narrow" / "wide" = the lower mask key > nlo / key >= nlo - 1, "long" = lo one row lower, "page" = the first page one
    too high where lo is not page-aligned -- mutants (a) to (d) of profiles/decode_window_numerics_mutations.txt."""
    o = np.zeros((p.B, p.H, p.D))
    for b in range(p.B):
        pos = p.lens[b]
        lo = max(0, pos - p.window) if slip == "long" else p.lo[b]
        rows = []
        for t in range(lo & ~31, pos, 32):
            nlo = lo - t
            for key in range(min(32, pos - t)):
                if not {"narrow": key > nlo, "wide": key >= nlo - 1}.get(slip, key >= nlo):
                    continue
                row = min(max(t + key, lo), pos - 1)
                if paged:
                    first = (lo >> 4) + (1 if slip == "page" and lo & 15 else 0)
                    row = 16 * min(max((t + 16 * (key >> 4)) >> 4, first), (pos - 1) >> 4) + (row & 15)
                rows.append(row)
        K = np.concatenate([p.values(p.kc[b, dc.LAYER, rows]), p.k_new[b][None].astype(np.float64)])
        V = np.concatenate([p.values(p.vc[b, dc.LAYER, rows]), p.v_new[b][None].astype(np.float64)])
        sc = np.einsum("kgd,tkd->kgt", p.q[b].astype(np.float64).reshape(p.Hkv, p.G, p.D), K) * p.D ** -0.5
        w = np.exp(sc - sc.max(axis=2, keepdims=True))
        o[b] = np.einsum("kgt,tkd->kgd", w / w.sum(axis=2, keepdims=True), V).reshape(p.H, p.D)
    return o


@pytest.mark.parametrize("window", dc.WINDOWS, ids=lambda w: f"w{w}")
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_window_edge_problems_tell_one_row_slips_apart(edges, dtype, window):
    """The model without a slip is the oracle on every window-edge problem.  With one, the sequences it puts outside the
    GPU file's elementwise tolerance are exactly: mask too narrow -- every sequence of edge_in, edge_out, equal and of the
    ramp that peaks at lo; mask too wide -- every lo that is no multiple of 32 in edge_out, equal and that ramp (the
    doubled row already has all the weight in edge_in); window too long -- every lo >= 1 of the same three; first page one
    too high (paged) -- every lo that is no multiple of 16 in edge_in, edge_out, equal and the ramp that peaks at lo (the
    ascending ramp leaves the tolerance under it at some windows only and is not asserted).  edge_last sees none of them."""
    shape = ("window", 2, 64, dtype)
    off32, off16, pos1 = (lambda lo: lo % 32 != 0), (lambda lo: lo % 16 != 0), (lambda lo: lo >= 1)
    all_, none = (lambda lo: True), (lambda lo: False)
    want = {None: dict(edge_in=none, edge_out=none, equal=none, ramp_through=none),
            "narrow": dict(edge_in=all_, edge_out=all_, equal=all_, ramp_through=all_),
            "wide": dict(edge_in=none, edge_out=off32, equal=off32, ramp_through=off32),
            "long": dict(edge_in=none, edge_out=pos1, equal=pos1, ramp_through=pos1),
            "page": dict(edge_in=off16, edge_out=off16, equal=off16, ramp_through=off16)}
    for kind in dc.EDGE_KINDS:
        p, ref = edges(shape, kind, window)
        for slip, kinds in want.items():
            for paged in (False, True) if slip != "page" else (True,):
                got = window_model(p, slip, paged)
                out = (np.abs(got - ref["o"]) > elementwise_tol(p, ref["o"])).any(axis=(1, 2))
                if slip is None:
                    np.testing.assert_allclose(got, ref["o"], atol=1e-6, rtol=1e-6)
                if kind == "edge_last":
                    assert not out.any(), (slip, paged)
                elif kind in kinds:
                    hit = [kinds[kind](lo) and (kind != "ramp_through" or p.ramp[b] < 0) for b, lo in enumerate(p.lo)]
                    if kind == "ramp_through" and slip == "page":       # (the ascending ramp: at some windows only)
                        out, hit = out[::2], hit[::2]
                        assert all(r < 0 for r in p.ramp[::2])
                    assert out.tolist() == hit, (kind, slip, paged, out.tolist())
