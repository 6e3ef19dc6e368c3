"""CPU twin of tests/test_far_memory_prefill_gpu.py and tests/test_far_memory_decode_gpu.py: every case of their tables
has the structure it is named for, and is safe to run.

For every placement: the named term really exceeds 2^31 elements and its byte offset 2^32; every other term stays below
2^24 elements -- but for the terms a table marks "bounded", which share the far term's stride and are limited by the
entry points instead (checked here against that limit); and the four addresses a truncating implementation would form in
place of any offset of the call (tests/far_memory.py) stay inside the arena, as does the true one.  Needs no GPU.
"""
import numpy as np
import pytest

import far_memory as fm

PLACEMENTS = fm.prefill_placements()


def test_truncations_are_the_four_cuts():
    x = np.array([0, 5, 2 ** 31 - 1, 2 ** 31, 2 ** 31 + 2 ** 20, 2 ** 32 - 8, 2 ** 32, 2 ** 32 + 24, 3 * 2 ** 31 + 8])
    t = fm.truncations(x, 2)
    assert t[0].tolist() == [0, 10, 2 ** 32 - 2, -2 ** 32, -2 ** 32 + 2 ** 21, -16, 0, 48, -2 ** 32 + 16]
    assert t[1].tolist() == [0, 10, 2 ** 32 - 2, 2 ** 32, 2 ** 32 + 2 ** 21, 2 ** 33 - 16, 0, 48, 2 ** 32 + 16]
    assert t[2].tolist() == [0, 10, -2, 0, 2 ** 21, -16, 0, 48, 16]
    assert t[3].tolist() == [0, 10, 2 ** 32 - 2, 0, 2 ** 21, 2 ** 32 - 16, 0, 48, 16]
    # one-byte elements (the fp8 caches): the element and the byte cuts coincide
    t = fm.truncations(x, 1)
    assert np.array_equal(t[0], t[2]) and np.array_equal(t[1], t[3])


def test_the_tables_cover_what_the_issue_names():
    ids = set(PLACEMENTS)
    for Sq, Sk in ((100, 299), (299, 100)):
        for D in (64, 128, 256):
            for op, terms in (("q", ("batch", "head", "row")), ("o", ("batch", "head", "row")),
                              ("k", ("batch", "head", "tile")), ("v", ("batch", "head", "tile"))):
                for t in terms:
                    assert "rect-%dx%d-D%d-%s-%s" % (Sq, Sk, D, op, t) in ids
    for D in (64, 128):
        for op in "qkvo":
            assert {"packed-D%d-%s-token" % (D, op), "packed-D%d-%s-head" % (D, op)} <= ids
    # packed: four sequences, a ragged one, an empty one, one with more rows than keys
    assert len(fm.PACKED_LENS) == 4 and (0, 5) in fm.PACKED_LENS and any(a > b for a, b in fm.PACKED_LENS)
    assert any(b % 64 for _, b in fm.PACKED_LENS)
    from prefill_varlen_split_ref import LENS
    assert set(fm.PACKED_LENS) <= set(LENS)


@pytest.mark.parametrize("name", list(PLACEMENTS))
def test_placement_has_the_structure_it_is_named_for(name):
    p = PLACEMENTS[name]
    kinds = [k for _, k in p.terms.values()]
    if p.term == "limit":
        assert kinds.count("far") == 0
    else:
        assert kinds.count("far") == 1
    for term, (value, kind) in p.terms.items():
        if kind == "far":
            assert value >= fm.FAR > 2 ** 31 and value * p.itemsize > 2 ** 32, (term, value)
        elif kind == "near":
            assert 0 <= value < fm.NEAR, (term, value)
        else:
            assert p.bound, term
    # the terms are the view's: they add up to its last row
    if p.term == "limit":
        pass
    elif "bounded" not in kinds:
        assert sum(v for v, _ in p.terms.values()) == int(p.row_offsets().max())
    else:       # (the last tile or sequence is ragged: the far term plus the bounded one reaches at least the last row)
        assert sum(v for v, _ in p.terms.values()) >= int(p.row_offsets().max()) >= max(v for v, _ in p.terms.values())
    assert all(s % 8 == 0 for s in p.strides)
    # a K / V pitch is one the entry points admit (the tile and token cases sit inside the limit on purpose)
    if p.operand in "kv" and p.D != 256:
        pitch = p.strides[0] if len(p.shape) == 2 else p.strides[2]
        assert pitch <= fm.pitch_limit(64, p.D) or name.startswith("limit32"), pitch
        assert not fm.wraps_at(pitch, 32 if name.startswith("limit32") else 64, p.D)
    if p.term == "limit":
        T = 32 if name.startswith("limit32") else 64
        pitch = p.strides[-1] if len(p.shape) == 3 else p.strides[0]
        assert pitch == fm.pitch_limit(T, p.D) and fm.wraps_at(pitch + 8, T, p.D)
        # one full tile and a ragged one (packed: in the last sequence)
        assert (p.shape[2] if len(p.shape) == 3 else fm.LIMIT_PACKED_LENS[-1][1]) == fm.LIMIT_SK[T] > T


@pytest.mark.parametrize("name", list(PLACEMENTS))
def test_no_truncated_address_leaves_the_arena(name):
    p = PLACEMENTS[name]
    need = p.arena_bytes()
    assert need <= fm.CAP - 2 ** 20
    assert p.safe_in(need) and p.safe_in(need + 2 ** 20, fm.GUARD + 4096)
    x = p.offsets()
    t = fm.truncations(x, p.itemsize) + fm.GUARD * p.itemsize
    assert t.shape == (4, x.size) and t.min() >= 0 and t.max() + p.D * p.itemsize <= need
    assert not p.safe_in(fm.GUARD * p.itemsize + (p.extent() - 1) * p.itemsize)         # (the check can fail)
    if p.term != "limit":
        assert (t != (x * p.itemsize + fm.GUARD * p.itemsize)).any(), "no offset of the case is cut by 32 bits"
    # the sentinel bands lie in the gaps: none of their elements belongs to a row
    bands = p.bands()
    rows = p.row_offsets().ravel()
    assert bands.size and np.intersect1d(bands // p.D * p.D, rows).size == 0
    assert bands.min() + fm.GUARD >= 0 and (bands.max() + 1 + fm.GUARD) * p.itemsize <= need + 2 ** 20
    runs = p.written()
    assert sum(hi - lo for lo, hi in runs) == rows.size * p.D


# ---- the decode tables -------------------------------------------------------------------------------------------------

CACHES = fm.decode_cache_maps()


@pytest.mark.parametrize("name", list(CACHES))
def test_far_cache_has_the_structure_it_is_named_for(name):
    cm = CACHES[name]
    terms = cm.terms()
    assert [k for _, k in terms.values()].count("far") == 1
    for term, (value, kind) in terms.items():
        if kind == "far":
            assert value >= fm.FAR and value > 2 ** 31, (term, value)
            assert cm.itemsize == 1 or value * cm.itemsize > 2 ** 32        # (e4m3: elements are bytes)
        else:
            assert 0 <= value < fm.NEAR, (term, value)
    x = cm.row_offsets()
    assert x.shape == (fm.DEC_B, fm.DEC_M, fm.DEC_HKV)
    used = x[x >= 0]
    assert used.max() + cm.D <= cm.elems and np.unique(used).size == used.size
    last = fm.DEC_B - 1                                 # every row of the last sequence is far
    assert x[last][x[last] >= 0].min() >= fm.FAR
    if cm.layout == "paged":
        assert cm.elems > 2 ** 31 and cm.shape[2] == 16
        for b, pos in enumerate(fm.DEC_LENS):           # mapped: the history, the new tokens, the sentinel rows; then -1
            need = -(-(pos + fm.DEC_N + fm.DEC_TAIL) // 16)
            assert np.all(cm.table[b, :need] >= 0) and np.all(cm.table[b, need:] == -1) and need < cm.table.shape[1]
        assert cm.table.max() == cm.num_pages - 1 and int(cm.table[cm.table >= 0].min()) * cm.page_stride >= fm.FAR
    else:
        assert cm.layer == cm.L - 1 and ((fm.DEC_B - 1) * (cm.L - 1) + cm.layer - 1) * fm.DEC_M * fm.DEC_HKV * cm.D < fm.FAR * 2
    # the compact twin holds the same rows in a small cache
    small = fm.CacheMap(cm.layout, cm.D, cm.itemsize, False)
    assert small.elems * small.itemsize < 2 ** 24 and all(k == "near" for _, k in small.terms().values())
    if cm.layout == "paged":
        assert np.array_equal(small.table >= 0, cm.table >= 0)


@pytest.mark.parametrize("name", list(CACHES))
def test_no_truncated_cache_address_leaves_the_arena(name):
    cm = CACHES[name]
    need = fm.decode_arena_bytes(cm)
    assert need <= fm.CAP - 2 ** 20
    for base in (fm.GUARD, fm.GUARD + cm.elems):        # K, and V behind it: K is V's guard
        assert cm.safe_in(need, base)
        t = fm.truncations(cm.offsets(), cm.itemsize) + base * cm.itemsize
        assert t.min() >= 0 and t.max() + cm.D * cm.itemsize <= need
        assert (t != cm.offsets() * cm.itemsize + base * cm.itemsize).any()
    assert not cm.safe_in(need, fm.GUARD // 2) or cm.itemsize == 1 and not cm.safe_in(need, 0)
    assert not cm.safe_in(need - 4096, fm.GUARD + cm.elems)


@pytest.mark.parametrize("name", list(fm.QKV_CASES))
def test_far_qkv_strides(name):
    p = fm.qkv_placement(name)
    c = fm.QKV_CASES[name]
    (value, kind), = p.terms.values()
    # args->stride is an int: 2^30 is the largest power of two it holds, so the third row sits at exactly 2^31 elements
    assert kind == "far" and value >= 2 ** 31 and value * 2 >= 2 ** 32 and fm.QKV_STRIDE == 2 ** 30 < 2 ** 31
    assert max(c["ns"]) * len(c["ns"]) >= 3 and c["B"] == len(c["lens"]) == len(c["ns"])
    need = p.arena_bytes()
    assert need <= fm.CAP and p.safe_in(need)
    t = fm.truncations(p.offsets(), 2) + fm.GUARD * 2
    assert t.min() >= 0 and (t != p.offsets() * 2 + fm.GUARD * 2).any()
