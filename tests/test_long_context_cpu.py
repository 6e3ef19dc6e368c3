"""tests/long_context_cases.py on the CPU: the structure of the cases (the coverage table, the geometry caps, the header's
preconditions), the conditions on the inputs under which a long softmax test bites (held on the fp64 model alone), the split
counts the library picks at these lengths (its exported host functions), and the justification of the far-position RoPE
envelope against two independent fp32 evaluations."""
import numpy as np
import pytest
import torch

import long_context_cases as lc
import serving_cases as sc
import serving_model as sm
from oracle import round_to
from oracle.decode_ref import _inv_freq

BY_ID = {c["id"]: c for c in lc.CASES}

# item -> the id of a case that reaches it
COVERAGE = {
    'G:16:M:32768': 12,
    'G:1:M:131072': 0,
    'G:1:M:32768': 60,
    'G:2:M:131072': 1,
    'G:2:M:32768': 75,
    'G:4:M:131072': 14,
    'G:4:M:32768': 2,
    'G:8:M:131072': 27,
    'G:8:M:32768': 3,
    'M:131072:D:128:16bit': 1,
    'M:131072:D:128:kv8': 36,
    'M:131072:D:64:16bit': 0,
    'M:131072:D:64:kv8': 39,
    'M:131072:blhmd16': 1,
    'M:131072:blmhd16': 0,
    'M:131072:paged128': 7,
    'M:131072:paged16': 10,
    'M:32768:D:128:16bit': 2,
    'M:32768:D:128:kv8': 37,
    'M:32768:D:256:16bit': 72,
    'M:32768:D:64:16bit': 3,
    'M:32768:D:64:kv8': 38,
    'M:32768:blhmd16': 5,
    'M:32768:blmhd16': 8,
    'M:32768:paged128': 3,
    'M:32768:paged16': 2,
    'cold_alone:S:0:flash_decode': 0,
    'cold_alone:S:0:flash_decode_chunk': 12,
    'cold_alone:S:1:flash_decode': 78,
    'cold_alone:S:1:flash_decode_chunk_window': 16,
    'cold_alone:S:1:flash_decode_window': 4,
    'cold_alone:S:32:flash_decode': 76,
    'cold_alone:S:32:flash_decode_chunk_window': 18,
    'cold_alone:S:32:flash_decode_varlen_window': 30,
    'cold_alone:S:32:flash_decode_window': 6,
    'cold_alone:S:7:flash_decode': 2,
    'cold_alone:S:7:flash_decode_chunk': 14,
    'cold_alone:S:7:flash_decode_varlen': 26,
    'far:65535:bf16': 7,
    'far:65535:fp16': 4,
    'far:65536:bf16': 11,
    'far:65536:fp16': 10,
    'far:65537:bf16': 14,
    'far:65537:fp16': 13,
    'far:98321:bf16': 16,
    'far:98321:fp16': 17,
    'far:M-1:bf16': 1,
    'far:M-1:fp16': 0,
    'far:M-n:bf16': 12,
    'far:M-n:fp16': 15,
    'flash_decode:blhmd0': 1,
    'flash_decode:blmhd0': 0,
    'flash_decode:decode_gqa_kernel:M:131072': 1,
    'flash_decode:decode_gqa_kernel:M:32768': 75,
    'flash_decode:decode_gqa_kernel:table_row>=65536': 1,
    'flash_decode:decode_kernel:M:131072': 0,
    'flash_decode:decode_kernel:M:32768': 72,
    'flash_decode:decode_kernel:table_row>=65536': 77,
    'flash_decode:matrix-core:M:131072': 76,
    'flash_decode:matrix-core:M:32768': 2,
    'flash_decode:matrix-core:table_row>=65536': 76,
    'flash_decode:paged128': 3,
    'flash_decode:paged16': 2,
    'flash_decode_chunk:blhmd0': 13,
    'flash_decode_chunk:blmhd0': 12,
    'flash_decode_chunk:paged128': 15,
    'flash_decode_chunk:paged16': 14,
    'flash_decode_chunk_kv8:blhmd0': 49,
    'flash_decode_chunk_kv8:blmhd0': 48,
    'flash_decode_chunk_kv8:paged128': 51,
    'flash_decode_chunk_kv8:paged16': 50,
    'flash_decode_chunk_kv8_window:blhmd0': 53,
    'flash_decode_chunk_kv8_window:blmhd0': 52,
    'flash_decode_chunk_kv8_window:paged128': 55,
    'flash_decode_chunk_kv8_window:paged16': 54,
    'flash_decode_chunk_kv8_window_sinks:blhmd0': 57,
    'flash_decode_chunk_kv8_window_sinks:blmhd0': 56,
    'flash_decode_chunk_kv8_window_sinks:paged128': 59,
    'flash_decode_chunk_kv8_window_sinks:paged16': 58,
    'flash_decode_chunk_window:blhmd0': 17,
    'flash_decode_chunk_window:blmhd0': 16,
    'flash_decode_chunk_window:paged128': 19,
    'flash_decode_chunk_window:paged16': 18,
    'flash_decode_chunk_window_sinks:blhmd0': 21,
    'flash_decode_chunk_window_sinks:blmhd0': 20,
    'flash_decode_chunk_window_sinks:paged128': 23,
    'flash_decode_chunk_window_sinks:paged16': 22,
    'flash_decode_kv8:blhmd0': 37,
    'flash_decode_kv8:blmhd0': 36,
    'flash_decode_kv8:paged128': 39,
    'flash_decode_kv8:paged16': 38,
    'flash_decode_kv8_window:blhmd0': 41,
    'flash_decode_kv8_window:blmhd0': 40,
    'flash_decode_kv8_window:paged128': 43,
    'flash_decode_kv8_window:paged16': 42,
    'flash_decode_kv8_window_sinks:blhmd0': 45,
    'flash_decode_kv8_window_sinks:blmhd0': 44,
    'flash_decode_kv8_window_sinks:paged128': 47,
    'flash_decode_kv8_window_sinks:paged16': 46,
    'flash_decode_varlen:blhmd0': 25,
    'flash_decode_varlen:blmhd0': 24,
    'flash_decode_varlen:paged128': 27,
    'flash_decode_varlen:paged16': 26,
    'flash_decode_varlen_kv8:blhmd0': 61,
    'flash_decode_varlen_kv8:blmhd0': 60,
    'flash_decode_varlen_kv8:paged128': 63,
    'flash_decode_varlen_kv8:paged16': 62,
    'flash_decode_varlen_kv8_window:blhmd0': 65,
    'flash_decode_varlen_kv8_window:blmhd0': 64,
    'flash_decode_varlen_kv8_window:paged128': 67,
    'flash_decode_varlen_kv8_window:paged16': 66,
    'flash_decode_varlen_kv8_window_sinks:blhmd0': 69,
    'flash_decode_varlen_kv8_window_sinks:blmhd0': 68,
    'flash_decode_varlen_kv8_window_sinks:paged128': 71,
    'flash_decode_varlen_kv8_window_sinks:paged16': 70,
    'flash_decode_varlen_window:blhmd0': 29,
    'flash_decode_varlen_window:blmhd0': 28,
    'flash_decode_varlen_window:paged128': 31,
    'flash_decode_varlen_window:paged16': 30,
    'flash_decode_varlen_window_sinks:blhmd0': 33,
    'flash_decode_varlen_window_sinks:blmhd0': 32,
    'flash_decode_varlen_window_sinks:paged128': 35,
    'flash_decode_varlen_window_sinks:paged16': 34,
    'flash_decode_window:blhmd0': 5,
    'flash_decode_window:blmhd0': 4,
    'flash_decode_window:paged128': 7,
    'flash_decode_window:paged16': 6,
    'flash_decode_window_sinks:blhmd0': 9,
    'flash_decode_window_sinks:blmhd0': 8,
    'flash_decode_window_sinks:paged128': 11,
    'flash_decode_window_sinks:paged16': 10,
    'n:40:_chunk': 18,
    'n:40:_varlen': 31,
    'order:012': 0,
    'order:021': 4,
    'order:102': 5,
    'order:120': 2,
    'order:201': 1,
    'order:210': 3,
    'section:A:rot:0:16bit': 0,
    'section:A:rot:0:kv8': 37,
    'section:B:rot:D/2:16bit': 1,
    'section:B:rot:D/2:kv8': 36,
    'section:B:rot:D:16bit': 3,
    'section:B:rot:D:kv8': 38,
    'short:0': 0,
    'short:3': 1,
    'splits:0:_chunk:16bit': 12,
    'splits:0:_chunk:kv8': 48,
    'splits:0:_single:16bit': 0,
    'splits:0:_single:kv8': 36,
    'splits:0:_varlen:16bit': 24,
    'splits:0:_varlen:kv8': 60,
    'splits:1:_chunk:16bit': 13,
    'splits:1:_chunk:kv8': 49,
    'splits:1:_single:16bit': 1,
    'splits:1:_single:kv8': 37,
    'splits:1:_varlen:16bit': 25,
    'splits:1:_varlen:kv8': 61,
    'splits:32:_chunk:16bit': 15,
    'splits:32:_chunk:kv8': 51,
    'splits:32:_single:16bit': 3,
    'splits:32:_single:kv8': 39,
    'splits:32:_varlen:16bit': 27,
    'splits:32:_varlen:kv8': 63,
    'splits:7:_chunk:16bit': 14,
    'splits:7:_chunk:kv8': 50,
    'splits:7:_single:16bit': 2,
    'splits:7:_single:kv8': 38,
    'splits:7:_varlen:16bit': 26,
    'splits:7:_varlen:kv8': 62,
    'table_row>=65536:flash_decode': 1,
    'table_row>=65536:flash_decode_chunk': 14,
    'table_row>=65536:flash_decode_chunk_kv8': 49,
    'table_row>=65536:flash_decode_chunk_kv8_window': 52,
    'table_row>=65536:flash_decode_chunk_kv8_window_sinks': 59,
    'table_row>=65536:flash_decode_chunk_window': 17,
    'table_row>=65536:flash_decode_chunk_window_sinks': 20,
    'table_row>=65536:flash_decode_kv8': 36,
    'table_row>=65536:flash_decode_kv8_window': 43,
    'table_row>=65536:flash_decode_kv8_window_sinks': 80,
    'table_row>=65536:flash_decode_varlen': 27,
    'table_row>=65536:flash_decode_varlen_kv8': 62,
    'table_row>=65536:flash_decode_varlen_kv8_window': 65,
    'table_row>=65536:flash_decode_varlen_kv8_window_sinks': 68,
    'table_row>=65536:flash_decode_varlen_window': 30,
    'table_row>=65536:flash_decode_varlen_window_sinks': 33,
    'table_row>=65536:flash_decode_window': 79,
    'table_row>=65536:flash_decode_window_sinks': 11,
    'varlen:empty_sequence': 24,
    'window:1:M:131072': 7,
    'window:1:M:32768': 6,
    'window:2M:M:131072': 29,
    'window:2M:M:32768': 73,
    'window:4096:M:131072': 4,
    'window:4096:M:32768': 19,
    'window:65536+17:M:131072': 16,
    'window:M:M:131072': 55,
    'window:M:M:32768': 5,
}

ITEMS = (["%s:%s" % (e, l) for e in sc.ENTRIES for l in ("blmhd0", "blhmd0", "paged16", "paged128")] +
         ["splits:%d:%s:%s" % (S, s, c) for S in lc.SPLITS for s in ("_single", "_chunk", "_varlen") for c in ("16bit", "kv8")] +
         ["far:%s:%s" % (f, d) for f in ("M-1", "M-n", 65535, 65536, 65537, 98304 + 17) for d in ("fp16", "bf16")] +
         ["flash_decode:%s:M:%d" % (k, M) for k in ("decode_kernel", "decode_gqa_kernel", "matrix-core") for M in lc.M_VALUES] +
         ["window:%s:M:%d" % (w, M) for M in lc.M_VALUES for w in ("1", "4096", "M", "2M")] + ["window:65536+17:M:131072"] +
         ["G:%d:M:%d" % (g, M) for M in lc.M_VALUES for g in (1, 2, 4, 8)] + ["G:16:M:32768", "short:0", "short:3"] +
         ["section:%s:rot:%s:%s" % (s, r, c) for c in ("16bit", "kv8") for s, r in (("A", "0"), ("B", "D/2"), ("B", "D"))] +
         ["order:%d%d%d" % o for o in ((0, 1, 2), (2, 0, 1), (1, 2, 0), (2, 1, 0), (0, 2, 1), (1, 0, 2))] +
         ["M:%d:%s" % (M, l) for M in lc.M_VALUES for l in ("blmhd16", "blhmd16", "paged16", "paged128")] +
         ["cold_alone:S:32:flash_decode", "cold_alone:S:32:flash_decode_window", "cold_alone:S:7:flash_decode"] +
         ["cold_alone:S:0:flash_decode_chunk", "cold_alone:S:7:flash_decode_chunk", "cold_alone:S:32:flash_decode_chunk_window",
          "cold_alone:S:7:flash_decode_varlen", "cold_alone:S:32:flash_decode_varlen_window"] +
         ["table_row>=65536:" + e for e in sc.ENTRIES] +
         ["flash_decode:%s:table_row>=65536" % k for k in ("decode_kernel", "decode_gqa_kernel", "matrix-core")] +
         ["M:32768:D:256:16bit", "n:40:_chunk", "n:40:_varlen", "varlen:empty_sequence"])


def test_the_coverage_table_names_every_item():
    assert set(ITEMS) <= set(COVERAGE), sorted(set(ITEMS) - set(COVERAGE))


@pytest.mark.parametrize("item", sorted(COVERAGE))
def test_a_case_reaches(item):
    assert item in lc.case_items(BY_ID[COVERAGE[item]])


def test_the_cases_keep_the_geometry_caps():
    assert [c["id"] for c in sorted(lc.CASES, key=lambda c: c["id"])] == list(range(len(lc.CASES)))
    for c in lc.CASES:
        M, D, H = c["M"], c["D"], c["Hkv"] * c["G"]
        assert M in lc.M_VALUES and c["Hkv"] in (1, 2) and H <= 32 and D in (64, 128, 256)
        assert c["L"] == 1 and c["layer"] == 0 if M == 131072 else c["L"] in (1, 2) and c["layer"] == c["L"] - 1
        assert lc.B * c["L"] * M * c["Hkv"] * D * 2 <= 201326592                  # one cache, 16 bit
        assert M * H * D <= 131072 * 1024                                           # the fp64 model's K and V per sequence
        assert D < 256 or (c["shape"] == "" and not c["kv8"])
        assert sorted(c["order"]) == [0, 1, 2]
        assert all(c["n"][b] > 0 for b in range(lc.B) if c["order"][b] == 0)       # the far sequence always has tokens
        small = c["window"] is not None and c["window"] <= 4096
        assert max(c["n"]) <= (40 if small else 4)
        for b, role in enumerate(c["order"]):
            pos, n = c["pos"][b], c["n"][b]
            assert 0 <= pos and pos + n <= M
            if role == 0:
                assert pos == (M - n if c["far"] == "last" else c["far"])
            elif role == 1:
                assert pos % 2 == 1 and pos >= (40000 if M == 131072 else 20000) and pos % 16 not in (0, 15)
            else:
                assert pos in (0, 3)
        assert c["rot"] == 0 and not c["tables"] if c["section"] == "A" else c["rot"] in (D // 2, D) and c["tables"]


def test_head_dim_256_is_for_the_single_token_16_bit_calls():
    c = next(c for c in lc.CASES if c["D"] == 256)
    m = lc.materialise(c)
    with pytest.raises(AssertionError):
        lc.check_preconditions(m["trace"]["geo"], dict(m["call"], shape="_chunk", entry="flash_decode_chunk"), m["trace"]["table"])
    with pytest.raises(AssertionError):
        lc.check_preconditions(dict(m["trace"]["geo"], kv8=True), m["call"], m["trace"]["table"])
    with pytest.raises(AssertionError):             # and everything else is still serving_cases' rule
        lc.check_preconditions(m["trace"]["geo"], dict(m["call"], pos=[c["M"]] * lc.B), m["trace"]["table"])


def test_the_rotation_invariant_cases_cover_their_product_at_far_positions():
    """three shapes x both cache types x windowed or not, each with tokens on a far sequence at a row >= 65535, and every far
    position at least once"""
    cells = set()
    for c in lc.INVARIANT_CASES:
        far = [c["pos"][b] for b in range(lc.B) if c["order"][b] == 0 and c["n"][b] > 0]
        assert len(far) == 1 and far[0] >= 65535 and c["M"] == 131072 and c["rot"] == c["D"] // 2 and not c["tables"], c
        assert far[0] == (c["M"] - max(c["n"]) if c["far"] == "last" else c["far"])
        cells.add((c["shape"], c["kv8"], c["window"] is not None))
    assert len(cells) == 12 == len(lc.INVARIANT_CASES)
    assert {c["far"] for c in lc.INVARIANT_CASES} == set(lc.far_positions(131072))
    for rot in (32, 64, 128):
        assert len({lc.own_pair(t, rot) for t in range(4)}) == 4


def test_planted_rows():
    vis, below = lc.planted_rows(131071, 1, None)
    assert below is None and {0, 131070, 65535, 65536, 4095 - 1, 4095 + 1, 4095 + 32, 18724 * 3 - 64} <= set(vis)
    vis, below = lc.planted_rows(127000 + 4095, 4, 4096)
    assert below == 126999 and vis[0] == 127000 and 127003 in vis and vis[-1] == 131094 and 65536 not in vis
    vis, below = lc.planted_rows(3, 1, 1)
    assert vis == [] and below == 2
    assert lc.planted_rows(0, 2, None) == ([], None)


@pytest.fixture(scope="module")
def lib():
    from starflashattention_amd import _lib
    return _lib.load()


def test_the_library_splits_the_key_range_at_these_lengths(lib):
    """num_splits = 0: what the exported host functions say the library picks.  Above 1 in every case but a window of one
    row; 32 for sfa_decode at 131072 rows with one kv head, the count clamp_splits reaches only from 65536 rows on."""
    for c in lc.CASES:
        S = lc.auto_splits(lib, c)
        assert 1 <= S <= 32 and (S == 1) == (c["window"] == 1), (c["id"], S)
    assert lib.sfa_decode_auto_splits(lc.B, 1, 128, 131072) == 32 and lib.sfa_decode_auto_splits(lc.B, 1, 128, 32768) == 16


@pytest.mark.parametrize("case", lc.CASES, ids=lc.case_id)
def test_a_case_keeps_the_preconditions_and_bites(case):
    """The header's preconditions; background scores within +-1; and the mutation conditions: dropping any single planted
    visible row (cached or new) from the model's attention, or admitting the planted row below the window, moves the
    model's o by at least 10 x TOL (atol = rtol) in some element."""
    m = lc.materialise(case)
    geo, call, data = m["trace"]["geo"], m["call"], m["data"]
    lc.check_preconditions(geo, call, m["trace"]["table"], data["k_scale"], data["v_scale"])
    assert geo["stride"] > geo["M"] // geo["ps"]
    bg = lc.background(lc.bg_key(case))
    for b, (pos, n) in enumerate(zip(case["pos"], case["n"])):       # the planted rows, and nothing else, differ from the background
        rows = m["visible"][b] + ([m["below"][b]] if m["below"][b] is not None else [])
        diff = np.flatnonzero((data["kc"][b] != bg["kc"][b]).any(axis=(0, 2, 3)))
        assert set(diff) <= set(rows if n else []) and all(r < pos for r in rows)
        for t in m["tokens"]:
            assert np.array_equal(round_to(t, geo["dtype"]), t)
    if call["sinks"] is not None and geo["H"] > 1:
        assert sum(s == float("-inf") for s in call["sinks"]) == 1
    if data["k_scale"] is not None:                                     # no planted byte saturates
        assert np.all((data["kc"] & 0x7F) < 0x7E) and np.all((data["vc"] & 0x7F) < 0x7E)
    for r in lc.mutation_margins(m):
        print(r)
        assert r["background"] <= 1.0, r
        assert r["drop"] >= 10.0 and r["admit"] >= 10.0, r


@pytest.mark.parametrize("cid", (7, 16, 35, 57))
def test_the_weights_are_the_models(cid):
    """lc.weights(), which the mutation conditions are computed from, reproduces serving_model.attend_rows"""
    m = lc.materialise(BY_ID[cid])
    mc = sc.model_call(m["trace"]["geo"], m["call"], m["data"], m["tokens"])
    cache = (m["data"]["kc"], m["data"]["vc"])
    app, attend = sm.step(cache, mc)
    after = sm.apply(cache, mc, app)
    want = attend(*after)
    for b, n in enumerate(mc["n"]):
        if n:
            np.testing.assert_allclose(lc.weights(mc, after, b)[0], want[b], rtol=1e-12, atol=1e-13)


@pytest.mark.parametrize("case", lc.INVARIANT_CASES, ids=lc.case_id)
def test_a_rotation_invariant_case_is_invariant_and_bites(case):
    """Section C: the preconditions and the mutation conditions as above; the model's o over the bits a device stores hardly depends on that device's inv_freq
    within the envelope (two thirds of TOL at the most: bf16's rounding of a rotated q of magnitude 4); and rotating q at pos for every token of a chunk, instead of pos + t, moves o by 10 x TOL."""
    from oracle import rope_interleaved
    m = lc.materialise(case)
    geo, call, data = m["trace"]["geo"], m["call"], m["data"]
    lc.check_preconditions(geo, call, m["trace"]["table"], data["k_scale"], data["v_scale"])
    rot, dtype, H, Hkv, tol = geo["rot"], geo["dtype"], geo["H"], geo["Hkv"], lc.TOL[geo["dtype"]]
    assert rot == geo["D"] // 2 and not geo["tables"] and not np.any(data["kc"][..., :rot])
    for r in lc.mutation_margins(m):
        assert r["background"] <= 1.0 and r["drop"] >= 10.0 and r["admit"] >= 10.0, r
    mc = sc.model_call(geo, call, data, m["tokens"])
    cache = (data["kc"], data["vc"])
    after = sm.apply(cache, mc, sm.step(cache, mc)[0])
    for b, (pos, n) in enumerate(zip(call["pos"], call["n"])):
        if n == 0:
            continue
        o = lc.weights(mc, after, b)[0]
        tok = np.asarray(m["tokens"][b], np.float64)
        # (1) the device's inv_freq at either end of the envelope: what the GPU test compares with (the model's own q over
        # the k bits such a device stores) against what such a device computes (q rotated by its own angle too)
        for d in (0, 2 * lc.ENVELOPE_ULPS):
            kb = after[0].copy()
            q16 = np.empty((n, H, geo["D"]))
            for t in range(n):
                ang = lc.envelope(pos + t, rot)[d]
                rope = lambda x: round_to(rope_interleaved(x, pos + t, rot, cos=np.cos(ang), sin=np.sin(ang)), dtype)
                q16[t] = rope(tok[t, :H])
                kb[b, geo["layer"], pos + t] = sm.store(rope(tok[t, H:H + Hkv]), dtype, geo["kv8"], data["k_scale"])
            o_test = lc.weights(mc, (kb, after[1]), b)[0]
            o_device = lc.weights(mc, (kb, after[1]), b, q16=q16)[0]
            err = np.abs(o_test - o_device) / (tol + tol * np.abs(o_device))
            print("sequence %d, %+d ulps: the reference moves by %.3f of the tolerance" % (b, d - lc.ENVELOPE_ULPS, err.max()))
            assert err.max() <= 2.0 / 3.0               # (the reference's own uncertainty leaves the kernel a third of TOL)
        # (2) q rotated at pos for t > 0
        if n > 1:
            q16 = np.stack([round_to(rope_interleaved(tok[t, :H], pos, rot), dtype) for t in range(n)]).astype(np.float64)
            o2 = lc.weights(mc, after, b, q16=q16)[0]
            wrong = (np.abs(o2 - o) / (tol + tol * np.abs(o)))[1:].max()
            print("sequence %d: q rotated at pos moves o by %.1f tolerances" % (b, wrong))
            assert wrong >= 10.0


# ---- the far-position RoPE envelope ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("rot", (32, 64, 128, 256))
def test_two_fp32_evaluations_of_inv_freq_agree_within_the_envelope(rot):
    """torch.pow on the CPU against numpy's: independent fp32 powers, then the same reciprocal"""
    e = torch.arange(0, rot, 2, dtype=torch.float32) / rot
    t = (1.0 / torch.pow(torch.tensor(10000.0, dtype=torch.float32), e)).numpy()
    d = lc.ulps_between(t, _inv_freq(rot))
    print("ulps between torch's and numpy's inv_freq:", d.tolist())
    assert np.abs(d).max() <= lc.ENVELOPE_ULPS
    exact = (10000.0 ** (-np.arange(0, rot, 2, dtype=np.float64) / rot))
    assert np.abs(_inv_freq(rot).astype(np.float64) / exact - 1.0).max() <= lc.ENVELOPE_ULPS * 2.0 ** -23


@pytest.mark.parametrize("dtype", ("fp16", "bf16"))
@pytest.mark.parametrize("rot", (32, 64, 128))
def test_numpys_float32_rope_lies_in_the_envelope(rot, dtype):
    k = np.zeros(rot + 2)
    k[0::2] = 1.0
    for pos in lc.PROBE_POSITIONS + (65535, 98304 + 17):
        row = round_to(sc.rope_float32(k, pos, rot), dtype).astype(np.float64)
        ok = lc.check_probe_row(row, pos, rot, dtype)
        assert ok[lc.ENVELOPE_ULPS].all()                   # numpy's own inv_freq is the envelope's middle
        for scale in lc.K_SCALE:
            import kv8_ref
            s = np.asarray([scale], np.float32)
            lc.check_probe_bytes(kv8_ref.quantize(row[None].astype(np.float32), s), pos, rot, dtype, s)


def test_the_envelope_is_narrow_where_it_matters():
    """the probe can tell the deviations apart at far positions: at 131071 and rot 64 at least ten pairs are consistent with
    fewer than all five candidates in fp16 (the sensitivity the issue quotes), and a pair rotated at the neighbouring
    position is outside the envelope"""
    k = np.zeros(64)
    k[0::2] = 1.0
    row = round_to(sc.rope_float32(k, 131071, 64), "fp16").astype(np.float64)
    ok = lc.consistent_deviations(row, 131071, 64, "fp16")
    assert (ok.sum(axis=0) < 5).sum() >= 10
    with pytest.raises(AssertionError):
        lc.check_probe_row(row, 131070, 64, "fp16")
    assert lc.envelope(65536, 64).shape == (5, 32) and np.all(lc.envelope(0, 64) == 0.0)
    assert np.all(np.diff(lc.envelope(131071, 64), axis=0) >= 0.0)
