"""CPU tests of tests/serving_model.py (the geometry-free fp64 model of a decode call) and tests/serving_cases.py (the
seeded generators of the serving traces and of the prefill fuzz).

1. Anchors.  The model against oracle.decode_ref, computed here.  The reference functions of the *_ref.py files, which are
   adapters over the model, against what each of them returned while it had arithmetic of its own, recorded in
   tests/golden/decode_ref_anchors.npz (decode_ref_anchor_cases.py and make_decode_ref_anchors.py beside it): o to 1e-9
   where the function keeps fp64, to the bit after rounding to float32 where it returns float32; appended rows, bytes and
   the hashes of the caches identical.
2. Coverage: every item the traces and the prefill cases must reach is listed with a seed that reaches it, so that a change
   to a generator cannot silently drop one.
3. The generators are deterministic, every generated call satisfies the header's preconditions, and the reference alone
   meets the conditions the fp8 byte checks lean on at every committed seed.
"""
import functools
import importlib.util
import os

import numpy as np
import pytest

import serving_cases as sc
import serving_model as sm
from conftest import GOLDEN, load_golden
from oracle import decode_ref, round_to, rotary_table_ref, to_bits16

RECORDED = load_golden("decode_ref_anchors.npz")
_spec = importlib.util.spec_from_file_location("decode_ref_anchor_cases", os.path.join(GOLDEN, "decode_ref_anchor_cases.py"))
anchors = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(anchors)


def same_f32(model_o, ref_o):
    np.testing.assert_array_equal(np.asarray(model_o).astype(np.float32), np.asarray(ref_o, np.float32))


# ---- 1. anchors ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,rot,tables,bias", [("fp16", 64, False, False), ("bf16", 32, True, True), ("fp16", 0, False, True)])
def test_anchor_decode_ref(dtype, rot, tables, bias):
    """oracle.decode_ref at the frame of tests/test_fuzz_gpu.py: one kv head per query head, [B, 3, H, D]"""
    rng = np.random.default_rng([1, rot])
    B, H, D, L, M, layer = 3, 3, 64, 2, 96, 1
    lens = [0, 37, 95]
    qkv = round_to(rng.standard_normal((B, 3, H, D)), dtype)
    kc, vc = round_to(rng.standard_normal((B, L, M, H, D)), dtype), round_to(rng.standard_normal((B, L, M, H, D)), dtype)
    qb, kb, vb = (round_to(rng.standard_normal((H, D)), dtype) if bias else None for _ in range(3))
    cos, sin = rotary_table_ref(M, rot, dtype) if tables else (None, None)
    kr, vr = kc.copy(), vc.copy()
    ref = decode_ref(qkv, kr, vr, lens, layer, rot, dtype=dtype, q_bias=qb, k_bias=kb, v_bias=vb, cos_table=cos, sin_table=sin)
    call = sm.make_call(dtype, H, lens, [1] * B, [qkv[b].reshape(1, 3 * H, D) for b in range(B)], layer, rot, q_bias=qb,
                        k_bias=kb, v_bias=vb, cos=cos, sin=sin)
    cache = (to_bits16(kc, dtype), to_bits16(vc, dtype))
    app, attend = sm.step(cache, call)
    after = sm.apply(cache, call, app)
    np.testing.assert_array_equal(after[0], to_bits16(kr, dtype))           # the whole cache after the step, bit for bit
    np.testing.assert_array_equal(after[1], to_bits16(vr, dtype))
    o = attend(*after)
    for b in range(B):
        np.testing.assert_array_equal(app["k16"][b][0], ref["k_row"][b])
        np.testing.assert_array_equal(app["v16"][b][0], ref["v_row"][b])
        same_f32(o[b][0], ref["o"][b])


def test_the_fixture_records_every_case_and_nothing_else():
    assert {k.rsplit("/", 1)[0] for k in RECORDED.files if k != "commit"} == set(anchors.CASES)
    assert len(str(RECORDED["commit"])) == 40
    functions = {name.split("/")[0] for name in anchors.CASES}
    assert len(functions) == 11 and all(sum(n.startswith(f + "/") for n in anchors.CASES) >= 2 for f in functions)


@pytest.mark.parametrize("name", list(anchors.CASES))
def test_anchor_recorded(name):
    """one case of the fixture on today's reference function: every field it returned, by the type it was returned in"""
    got = anchors.CASES[name]()
    assert {name + "/" + field for field in got} == {k for k in RECORDED.files if k.startswith(name + "/")}
    for field, value in got.items():
        want, value = RECORDED[name + "/" + field], np.asarray(value)
        assert value.dtype == want.dtype and value.shape == want.shape, field
        if want.dtype == np.float64:
            np.testing.assert_allclose(value, want, atol=1e-9, rtol=0, err_msg=field)
        elif want.dtype == np.float32:
            same_f32(value, want)
        else:                                                   # appended bytes, the hashes of the caches
            np.testing.assert_array_equal(value, want, err_msg=field)


# ---- 2. coverage -----------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def trace(seed, kv8):
    return sc.make_trace(seed, kv8)


def trace_items(tr):
    """what a trace reaches, as strings"""
    g = tr["geo"]
    paged = g["layout"] == "paged"
    it = {"layout:" + g["layout"], "Hkv:%d" % g["Hkv"], "G:%d" % g["G"], "L:%d" % g["L"], "bias:" + ("yes" if g["bias"] else "no"),
          "rot:" + {0: "0", g["D"] // 2: "half", g["D"]: "full"}[g["rot"]]}
    if g["rot"] > 0:
        it.add("tables:" + ("yes" if g["tables"] else "no"))
    if g["L"] > 1:
        it.add("layer:" + ("first" if g["layer"] == 0 else "last" if g["layer"] == g["L"] - 1 else "middle"))
    if paged:
        it |= {"page_size:%d" % g["ps"], "stride:" + ("equal" if g["stride"] == -(-g["M"] // g["ps"]) else "wide")}
    for c in tr["calls"]:
        it |= {"entry:" + c["entry"], "num_splits:%d" % c["num_splits"]}
        live = [(p, n) for p, n in zip(c["pos"], c["n"]) if n > 0]
        if any(p == 0 for p, _ in live):
            it.add("pos:0")
        if any(p + n == g["M"] for p, n in live):
            it.add("ends_at_memory_max_len")
        if c["shape"] == "_varlen" and live and len(live) < g["B"]:
            it.add("varlen:n_b=0")
        if paged and any(p // g["ps"] != (p + n - 1) // g["ps"] for p, n in live):
            it.add("append_crosses_page_edge")
        if c["window"] is not None and live:
            it.add("window:binds" if any(c["window"] < p + n for p, n in live) else "window:does_not_bind")
            if c["window"] == 1:
                it.add("window:1")
        if c["sinks"] is not None and float("-inf") in c["sinks"]:
            it.add("sink:-inf")
    # an entry point names its cache type; everything else is listed once per cache type
    return {i if i.startswith("entry:") else ("kv8:" if g["kv8"] else "16bit:") + i for i in it}


# item -> (kv8, seed): the first seed of the committed ones that reaches it; every item but the entry points is pinned once
# for the 16-bit traces and once for the fp8 traces ("kv8:tables:no" = an fp8 trace that rotates with in-kernel trigonometry)
TRACE_COVERAGE = {
    'entry:flash_decode': (False, 3),
    'entry:flash_decode_window': (False, 0),
    'entry:flash_decode_window_sinks': (False, 0),
    'entry:flash_decode_chunk': (False, 0),
    'entry:flash_decode_chunk_window': (False, 3),
    'entry:flash_decode_chunk_window_sinks': (False, 1),
    'entry:flash_decode_varlen': (False, 0),
    'entry:flash_decode_varlen_window': (False, 2),
    'entry:flash_decode_varlen_window_sinks': (False, 1),
    'entry:flash_decode_kv8': (True, 0),
    'entry:flash_decode_kv8_window': (True, 1),
    'entry:flash_decode_kv8_window_sinks': (True, 0),
    'entry:flash_decode_chunk_kv8': (True, 0),
    'entry:flash_decode_chunk_kv8_window': (True, 0),
    'entry:flash_decode_chunk_kv8_window_sinks': (True, 7),
    'entry:flash_decode_varlen_kv8': (True, 0),
    'entry:flash_decode_varlen_kv8_window': (True, 1),
    'entry:flash_decode_varlen_kv8_window_sinks': (True, 1),
    '16bit:layout:blmhd': (False, 2),
    '16bit:layout:blhmd': (False, 3),
    '16bit:layout:paged': (False, 0),
    '16bit:page_size:16': (False, 0),
    '16bit:page_size:32': (False, 17),
    '16bit:page_size:64': (False, 10),
    '16bit:page_size:128': (False, 1),
    '16bit:Hkv:1': (False, 2),
    '16bit:Hkv:2': (False, 8),
    '16bit:Hkv:3': (False, 0),
    '16bit:Hkv:4': (False, 1),
    '16bit:G:1': (False, 6),
    '16bit:G:2': (False, 1),
    '16bit:G:4': (False, 7),
    '16bit:G:8': (False, 0),
    '16bit:G:16': (False, 18),
    '16bit:L:1': (False, 8),
    '16bit:L:2': (False, 0),
    '16bit:L:3': (False, 1),
    '16bit:layer:first': (False, 4),
    '16bit:layer:middle': (False, 9),
    '16bit:layer:last': (False, 0),
    '16bit:stride:equal': (False, 0),
    '16bit:stride:wide': (False, 10),
    '16bit:pos:0': (False, 0),
    '16bit:ends_at_memory_max_len': (False, 2),
    '16bit:varlen:n_b=0': (False, 0),
    '16bit:append_crosses_page_edge': (False, 0),
    '16bit:window:binds': (False, 0),
    '16bit:window:does_not_bind': (False, 0),
    '16bit:window:1': (False, 0),
    '16bit:sink:-inf': (False, 1),
    '16bit:num_splits:0': (False, 0),
    '16bit:num_splits:1': (False, 0),
    '16bit:num_splits:2': (False, 0),
    '16bit:num_splits:3': (False, 1),
    '16bit:rot:0': (False, 0),
    '16bit:rot:half': (False, 4),
    '16bit:rot:full': (False, 2),
    '16bit:tables:yes': (False, 2),
    '16bit:tables:no': (False, 7),
    '16bit:bias:yes': (False, 1),
    '16bit:bias:no': (False, 0),
    'kv8:layout:blmhd': (True, 0),
    'kv8:layout:blhmd': (True, 1),
    'kv8:layout:paged': (True, 2),
    'kv8:page_size:16': (True, 4),
    'kv8:page_size:32': (True, 11),
    'kv8:page_size:64': (True, 2),
    'kv8:page_size:128': (True, 6),
    'kv8:Hkv:1': (True, 7),
    'kv8:Hkv:2': (True, 6),
    'kv8:Hkv:3': (True, 1),
    'kv8:Hkv:4': (True, 0),
    'kv8:G:1': (True, 0),
    'kv8:G:2': (True, 6),
    'kv8:G:4': (True, 1),
    'kv8:G:8': (True, 4),
    'kv8:G:16': (True, 9),
    'kv8:L:1': (True, 0),
    'kv8:L:2': (True, 3),
    'kv8:L:3': (True, 1),
    'kv8:layer:first': (True, 1),
    'kv8:layer:middle': (True, 5),
    'kv8:layer:last': (True, 12),
    'kv8:stride:equal': (True, 2),
    'kv8:stride:wide': (True, 5),
    'kv8:pos:0': (True, 0),
    'kv8:ends_at_memory_max_len': (True, 2),
    'kv8:varlen:n_b=0': (True, 2),
    'kv8:append_crosses_page_edge': (True, 2),
    'kv8:window:binds': (True, 0),
    'kv8:window:does_not_bind': (True, 0),
    'kv8:window:1': (True, 2),
    'kv8:sink:-inf': (True, 1),
    'kv8:num_splits:0': (True, 0),
    'kv8:num_splits:1': (True, 0),
    'kv8:num_splits:2': (True, 0),
    'kv8:num_splits:3': (True, 0),
    'kv8:rot:0': (True, 0),
    'kv8:rot:half': (True, 3),
    'kv8:rot:full': (True, 2),
    'kv8:tables:yes': (True, 3),
    'kv8:tables:no': (True, 2),
    'kv8:bias:yes': (True, 0),
    'kv8:bias:no': (True, 1),
}

COMMON_ITEMS = (["layout:blmhd", "layout:blhmd", "layout:paged"] +
               ["page_size:%d" % p for p in sc.PAGE_SIZES] + ["Hkv:%d" % h for h in (1, 2, 3, 4)] +
               ["G:%d" % g for g in sc.GROUPS] + ["L:1", "L:2", "L:3", "layer:first", "layer:middle", "layer:last",
                                                  "stride:equal", "stride:wide", "pos:0", "ends_at_memory_max_len",
                                                  "varlen:n_b=0", "append_crosses_page_edge", "window:binds",
                                                  "window:does_not_bind", "window:1", "sink:-inf"] +
               ["num_splits:%d" % s for s in (0, 1, 2, 3)] +       # 0: the library's choice
               ["rot:0", "rot:half", "rot:full", "tables:yes", "tables:no", "bias:yes", "bias:no"])
TRACE_ITEMS = ["entry:" + e for e in sc.ENTRIES] + [t + i for t in ("16bit:", "kv8:") for i in COMMON_ITEMS]


def prefill_items(c):
    it = {"%s:G:%d" % (c["kind"], c["G"])}
    if "Sq" in c:
        it.add("Sq>Sk" if c["Sq"] > c["Sk"] else "Sq<=Sk")
    else:
        if any(a == 0 or b == 0 for a, b in c["lens"]):
            it.add("empty_sequence")
        if any(a > b for a, b in c["lens"]):
            it.add("n_q>n_k")
        if c["invalid"]:
            it.add("invalid:" + c["invalid"])
        if c.get("low_hint"):
            it.add("low_hint")
            if c["max_seqlen_k"] == 1:
                it.add("low_hint:1")
    if c["sinks"] is not None and float("-inf") in c["sinks"]:
        it.add("sink:-inf")
    if c["num_splits"] is not None:
        it.add("num_splits:%d" % c["num_splits"])
    if c["packed"]:
        it.add("packed_allocation")
    return it


# item -> (kind, seed)
PREFILL_COVERAGE = {
    'window:G:1': ('window', 5),
    'window:G:2': ('window', 2),
    'window:G:3': ('window', 8),
    'window:G:4': ('window', 3),
    'window:G:6': ('window', 9),
    'window:G:8': ('window', 0),
    'split:G:1': ('split', 0),
    'split:G:2': ('split', 2),
    'split:G:3': ('split', 4),
    'split:G:4': ('split', 7),
    'split:G:6': ('split', 3),
    'split:G:8': ('split', 1),
    'varlen:G:1': ('varlen', 9),
    'varlen:G:2': ('varlen', 0),
    'varlen:G:3': ('varlen', 13),
    'varlen:G:4': ('varlen', 2),
    'varlen:G:6': ('varlen', 1),
    'varlen:G:8': ('varlen', 5),
    'varlen_window:G:1': ('varlen_window', 8),
    'varlen_window:G:2': ('varlen_window', 9),
    'varlen_window:G:3': ('varlen_window', 3),
    'varlen_window:G:4': ('varlen_window', 0),
    'varlen_window:G:6': ('varlen_window', 6),
    'varlen_window:G:8': ('varlen_window', 7),
    'varlen_split:G:1': ('varlen_split', 1),
    'varlen_split:G:2': ('varlen_split', 0),
    'varlen_split:G:3': ('varlen_split', 2),
    'varlen_split:G:4': ('varlen_split', 20),
    'varlen_split:G:6': ('varlen_split', 3),
    'varlen_split:G:8': ('varlen_split', 5),
    'Sq>Sk': ('window', 0),
    'Sq<=Sk': ('window', 2),
    'empty_sequence': ('varlen', 0),
    'n_q>n_k': ('varlen', 0),
    'invalid:backwards': ('varlen', 8),
    'invalid:past_total_k': ('varlen', 16),
    'low_hint': ('varlen_split', 2),
    'sink:-inf': ('window', 4),
    'packed_allocation': ('window', 0),
    'num_splits:0': ('split', 2),
    'num_splits:1': ('split', 1),
    'num_splits:2': ('split', 3),
    'num_splits:3': ('split', 8),
    'num_splits:5': ('split', 13),
    'num_splits:9': ('split', 0),
}

PREFILL_ITEMS = (["%s:G:%d" % (k, g) for k in sc.PREFILL_KINDS for g in sc.PREFILL_GROUPS] + ["Sq>Sk", "Sq<=Sk", "empty_sequence", "n_q>n_k",
                                                            "invalid:backwards", "invalid:past_total_k", "low_hint",
                                                            "sink:-inf", "packed_allocation"] +
                 ["num_splits:%d" % s for s in sc.PREFILL_SPLITS])


def test_the_coverage_tables_name_every_item():
    assert set(TRACE_COVERAGE) == set(TRACE_ITEMS)
    assert set(PREFILL_COVERAGE) == set(PREFILL_ITEMS)
    assert all(seed in sc.TRACE_SEEDS for _, seed in TRACE_COVERAGE.values())
    assert all(kind in sc.PREFILL_KINDS and seed in sc.PREFILL_SEEDS for kind, seed in PREFILL_COVERAGE.values())
    assert len(sc.TRACE_SEEDS) == 32 and len(sc.PREFILL_SEEDS) == 24 and len(sc.ENTRIES) == 18


@pytest.mark.parametrize("item", TRACE_ITEMS)
def test_a_trace_reaches(item):
    kv8, seed = TRACE_COVERAGE[item]
    assert kv8 == ("kv8" in item.split(":")[0] or "_kv8" in item)
    assert item in trace_items(trace(seed, kv8)), (item, kv8, seed)


@pytest.mark.parametrize("item", PREFILL_ITEMS)
def test_a_prefill_case_reaches(item):
    kind, seed = PREFILL_COVERAGE[item]
    assert item in prefill_items(sc.prefill_case(kind, seed)), (item, kind, seed)


# ---- 3. determinism, preconditions, the conditions on the reference ---------------------------------------------------------

def test_the_generators_are_deterministic():
    for kv8 in (False, True):
        for seed in (0, 5, 31):
            a, b = sc.make_trace(seed, kv8), sc.make_trace(seed, kv8)
            assert repr((a["geo"], a["calls"])) == repr((b["geo"], b["calls"])) and np.array_equal(a["table"], b["table"])
    tr = trace(3, True)
    da, db = sc.trace_data(tr), sc.trace_data(tr)
    assert all(np.array_equal(da[k], db[k]) if da[k] is not None else db[k] is None for k in da)
    ta, tb = sc.call_tokens(tr["geo"], tr["calls"][2]), sc.call_tokens(tr["geo"], tr["calls"][2])
    assert all(np.array_equal(x, y) for x, y in zip(ta, tb))
    for kind in sc.PREFILL_KINDS:
        assert repr(sc.prefill_case(kind, 7)) == repr(sc.prefill_case(kind, 7))
        assert all(np.array_equal(x, y) for x, y in zip(sc.prefill_inputs(sc.prefill_case(kind, 7)),
                                                        sc.prefill_inputs(sc.prefill_case(kind, 7))))


@pytest.mark.parametrize("kv8", [False, True])
def test_every_generated_call_satisfies_the_preconditions(kv8):
    for seed in sc.TRACE_SEEDS:
        tr = trace(seed, kv8)
        g = tr["geo"]
        assert g["dtype"] == ("fp16", "bf16")[seed % 2] and 1 <= g["B"] <= 6 and g["H"] <= sc.H_MAX and g["M"] <= sc.M_MAX
        assert len(tr["calls"]) == sc.STEPS
        pos = tr["calls"][0]["pos"]
        for i, c in enumerate(tr["calls"]):
            assert c["step"] == i and c["pos"] == pos           # seq_len advances by what was appended
            sc.check_preconditions(g, c, tr["table"])
            assert all(n <= sc.N_MAX for n in c["n"]) and (c["window"] is None or c["window"] <= 2 * g["M"])
            pos = [p + n for p, n in zip(pos, c["n"])]
        if kv8 and g["rot"] > 0 and not g["tables"]:
            assert g["M"] <= sc.KV8_TRIG_M_MAX


def test_the_preconditions_reject_what_the_library_would():
    tr = sc.make_trace(0, False)
    g, c = tr["geo"], tr["calls"][0]
    sc.check_preconditions(g, c, tr["table"])
    with pytest.raises(AssertionError):
        sc.check_preconditions(g, dict(c, pos=[g["M"]] * g["B"], n=[1] * g["B"]), tr["table"])
    with pytest.raises(AssertionError):
        sc.check_preconditions(g, c, np.zeros_like(tr["table"]))            # pages shared between sequences
    with pytest.raises(AssertionError):
        sc.check_preconditions(dict(g, G=3, H=3 * g["Hkv"]), c, tr["table"])
    with pytest.raises(AssertionError):
        sc.check_preconditions(dict(g, D=256), c, tr["table"])
    with pytest.raises(AssertionError):
        sc.check_preconditions(g, c, tr["table"], k_scale=np.zeros(g["Hkv"], np.float32))


@pytest.mark.parametrize("seed", sc.TRACE_SEEDS)
def test_the_reference_alone_keeps_the_kv8_byte_conditions(seed):
    """more than 98 % of the K bytes a trace appends are identical, and every one is within one e4m3 step,
    when the reference quantiser is applied to the reference's own rotated k computed in float32 arithmetic.  A seed that
    cannot keep this is replaced in serving_cases.TRACE_SEEDS (with the reason); the cap stays."""
    tr = trace(seed, True)
    data = sc.trace_data(tr)
    sc.check_preconditions(tr["geo"], tr["calls"][0], tr["table"], data["k_scale"], data["v_scale"])
    same, total, worst = sc.kv8_k_bytes_float32(tr, data)
    if total:
        assert same / total > 0.98, (same, total)
        assert worst <= 1.0, worst


def test_the_prefill_cases_stay_inside_their_allocations():
    for kind in sc.PREFILL_KINDS:
        for seed in sc.PREFILL_SEEDS:
            c = sc.prefill_case(kind, seed)
            assert c["Hq"] == c["Hkv"] * c["G"] and 1 <= c["Hkv"] <= 5 and c["G"] in sc.PREFILL_GROUPS
            if "Sq" in c:
                assert 1 <= c["Sq"] <= 700 and 1 <= c["Sk"] <= 700 and 1 <= c["B"] <= 3
                assert c["window"] is None or 1 <= c["window"] <= 2 * c["Sk"]
                continue
            cu_q, cu_k = c["cu_q"], c["cu_k"]
            assert all(0 <= a <= b for a, b in zip(cu_q, cu_q[1:])) and cu_q[-1] == c["total_q"]    # query rows: always ranges
            assert all(0 <= x <= c["alloc_k"] for x in cu_k) and c["total_k"] <= c["alloc_k"]
            bad = [b for b in range(c["B"]) if not 0 <= cu_k[b] <= cu_k[b + 1] <= c["total_k"]]
            assert (len(bad) >= 1) == (c["invalid"] is not None)
            if kind == "varlen_split":
                assert c["max_seqlen_k"] >= 1
