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
    assert seen_hot > 0 and (entry in ("decode", "kv8") or seen_front > 0)


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
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
            assert np.abs(dc.scores_log2(p, ref, p.cu[b + 1] - 1)).max() >= 100.0


@pytest.mark.parametrize("shape", [s for s in SHAPES if s[0] != "varlen"], ids=ids)
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
    no other; the oracle does not see the difference."""
    entry, G, D, dtype = shape
    clean = dc.normal_problem(entry, dtype, G, D)
    bad = clean.poisoned(None if pattern == "nan" else dc.INF16[dtype])
    m = clean.unread_mask()
    for c, x in ((clean.kc, bad.kc), (clean.vc, bad.vc)):
        assert np.all(c[m] == 0) and np.all(x[m] != c[m]) and np.array_equal(x[~m], c[~m])
        assert not np.isfinite(bad.values(x[m])).any()
    for b in range(clean.B):
        assert not m[b, dc.LAYER, :clean.lens[b] + clean.ns[b]].any() and m[b, dc.LAYER, clean.lens[b] + clean.ns[b]:].all()
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
    for entry in ("decode", "kv8", "chunk", "varlen"):
        mine = [c for c in dc.CONFIGS if c[0] == entry]
        assert {c[4] for c in mine} == {"fp16", "bf16"}
    for kernel in ([c for c in dc.CONFIGS if c[0] == "kv8"], [c for c in dc.CONFIGS if c[:2] == ("decode", 1)],
                   [c for c in dc.CONFIGS if c[:3] == ("decode", 8, 64)], [c for c in dc.CONFIGS if c[:3] == ("decode", 4, 64)]):
        assert any(c[5].get("decode_nt") == 1 for c in kernel)          # (the chunk body has no non-temporal loads)
    assert dc.SPIKE_ROWS[-1] == 199 and dc.VARLEN_NS == [1, 3, 40, 0, 17]
