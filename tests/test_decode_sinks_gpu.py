"""GPU checks of sfa_decode_window_sinks / sfa_decode_chunk_window_sinks / sfa_decode_varlen_window_sinks (attention sinks
in the three windowed decode calls) through the Python operators: parity with the fp64 references of tests/sinks_ref.py
over the twins' own pairwise-covering sweeps, that the sink binds and is indexed by query head, that it is counted once
whatever the split count, bit-identity with the _window twin where the sink has no weight, the extremes, unread memory,
rejection, graph replay and the operators' argument checks.

The frame is the window tests': B = 4 sequences at seq_len = (0, 5, 130, 1000), 2 kv heads, 2 layers, memory_max_len
1408, q / k / v bias and a partial rotary embedding; their run() harnesses drive the sinks calls through
sinks_ref.WithSinks.  Tolerance: window_ref.TOL (fp16 2e-3, bf16 1.6e-2, atol = rtol, elementwise, nothing exempt) -- a
sink multiplies the output by a factor in (0, 1], so the bound that holds for the twins holds here.

Sinks: sinks[h] = lse_ref[anchor, h] + delta_h with delta = linspace(-3, 3, H): on the anchor row (chunk / varlen: token
0 of the anchor sequence) the sink's share of the softmax is sigmoid(delta_h), 0.047 .. 0.953, different for every head.
"""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import chunk_window_ref as cw
import sinks_ref
import test_decode_chunk_window_gpu as cwg
import test_decode_window_gpu as w1
import window_ref
from sinks_ref import WithSinks
from window_ref import TOL

pytestmark = pytest.mark.gpu

LENS, HKV, L, M, LAYER = cw.LENS, cw.HKV, cw.L, cw.M, cw.LAYER
assert w1.LENS == LENS and (w1.HKV, w1.L, w1.M, w1.LAYER) == (HKV, L, M, LAYER)
CALLS = ("single", "chunk", "varlen")


@pytest.fixture(scope="module")
def sfa():
    assert torch.cuda.is_available(), "GPU tests need a GPU (run with -m gpu on the MI355X box)"
    import starflashattention_amd as m
    m._lib.load()                  # fail loudly if the HIP library is missing
    return m


def on_device(sinks):
    """float32 [H] on the GPU (None stays None = NULL)"""
    return None if sinks is None else torch.from_numpy(np.asarray(sinks, np.float32)).to("cuda:0")


# ---- references (made once, never modified).  `shift`: None = delta_h = linspace(-3, 3, H), a number = that delta for
# ---- every head; the sinks the device gets are the float32 roundings, and the references are computed from those ---------

def _single_args(dtype, D, G, window, tables):
    t, c = w1.tokens(dtype, D, G), w1.caches(dtype, D)
    f = lambda x: x.float().numpy()
    qkv = f(t.qkv)
    cos, sin = w1.rotary_tables(dtype, t.rot) if tables else (None, None)
    return ((qkv[:, :t.H], qkv[:, t.H:t.H + HKV], qkv[:, t.H + HKV:], c.kf, c.vf, LENS, LAYER, t.rot, window),
            dict(q_bias=f(t.qb), k_bias=f(t.kb), v_bias=f(t.vb), cos_table=cos, sin_table=sin))


@functools.lru_cache(maxsize=None)
def single_ref(dtype, D, G, window, tables=False, anchor=None, shift=None, scale=None):
    """(sinks float32 [H] or None, the reference): anchor None = no sink (every sink -inf)"""
    args, kw = _single_args(dtype, D, G, window, tables)
    if anchor is None:
        return None, sinks_ref.decode_window_sinks_ref(*args, None, dtype, scale=scale, **kw)
    lse = single_ref(dtype, D, G, window, tables, scale=scale)[1]["lse"][anchor]
    sinks = sinks_ref.make_sinks(lse, shift).astype(np.float32)
    return sinks, sinks_ref.decode_window_sinks_ref(*args, sinks, dtype, scale=scale, **kw)


@functools.lru_cache(maxsize=None)
def chunk_ref(dtype, D, G, n, window, tables=False, anchor=None, shift=None, scale=None):
    prob = cw.problem(dtype, D, G, n, tables)
    if anchor is None:
        return None, sinks_ref.chunk_sinks_ref(prob, window, None, scale=scale)
    lse = chunk_ref(dtype, D, G, n, window, tables, scale=scale)[1][anchor][3][0]      # token 0 of the anchor sequence
    sinks = sinks_ref.make_sinks(lse, shift).astype(np.float32)
    return sinks, sinks_ref.chunk_sinks_ref(prob, window, sinks, scale=scale)


def three(ref):
    """the (o, k_rows, v_rows) of chunk_window_ref.check_against_reference"""
    return [x[:3] for x in ref]


def run_call(sfa, call, dtype, D, G, n, layout, window, sinks, num_splits=0, tables=False, **extra):
    """One call of `call` in CALLS with `sinks` (float32 array, device tensor or None) -- or, sinks="window", its
    _window twin.  Returns the harness result with o as a list per sequence."""
    s = sfa if isinstance(sinks, str) else WithSinks(sfa, sinks if isinstance(sinks, torch.Tensor) else on_device(sinks),
                                                     **extra)
    if call == "single":
        r = w1.run(s, dtype, D, G, layout, window, num_splits, tables=tables)
        r.o = [r.o[b] for b in range(w1.B)]
        return r
    return cw.run(s, cw.problem(dtype, D, G, n, tables), layout, window, num_splits, varlen=call == "varlen")


def reference_of(call, dtype, D, G, n, window, tables=False, anchor=None, shift=None, scale=None):
    """(sinks, o per sequence as [rows, H, D] float32, the full reference)"""
    if call == "single":
        sinks, ref = single_ref(dtype, D, G, window, tables, anchor, shift, scale)
        return sinks, [ref["o"][b][None] for b in range(w1.B)], ref
    sinks, ref = chunk_ref(dtype, D, G, n, window, tables, anchor, shift, scale)
    return sinks, [x[0] for x in ref], ref


def rows_of(o_bits, call):
    """[rows, H, D] bits of one sequence's output"""
    return o_bits[None] if call == "single" else o_bits


def assert_o(r, o_ref, dtype, call):
    tol = TOL[dtype]
    for b in range(len(o_ref)):
        np.testing.assert_allclose(cw.as_float(rows_of(r.o[b], call), dtype), o_ref[b], atol=tol, rtol=tol,
                                   err_msg=f"sequence {b}")


def same_bits(r, other):
    return (all(torch.equal(a, b) for a, b in zip(r.o, other.o)) and torch.equal(r.kc, other.kc)
            and torch.equal(r.vc, other.vc))


# ---- 1. parity sweeps: the twins' own ------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", list(enumerate(window_ref.SWEEP)), ids=lambda c: "-".join(str(x) for x in c[1]))
def test_sinks_parity_sweep_single(sfa, case):
    i, (dtype, D, layout, G, num_splits, window) = case
    tables, anchor = bool(i & 1), i % 4
    sinks, ref = single_ref(dtype, D, G, window, tables, anchor)
    r = w1.run(WithSinks(sfa, on_device(sinks)), dtype, D, G, layout, window, num_splits, tables=tables)
    sfa.check_decode_status()
    np.testing.assert_allclose(w1.as_float(r.o, dtype), ref["o"], atol=TOL[dtype], rtol=TOL[dtype])
    c = w1.caches(dtype, D)
    w1.check_appended_and_untouched(r, c.kc, c.vc, ref, dtype, like=w1._full_decode(dtype, D, G, tables))
    if r.spare_k is not None:
        assert not bool(r.spare_k.any()) and not bool(r.spare_v.any())


def chunk_parity_case(sfa, case, varlen):
    i, (dtype, D, layout, G, num_splits, window) = case
    tables, anchor = bool(i & 1), (i + 1) % 4
    n = cw.sweep_tokens(G)
    prob = cw.problem(dtype, D, G, n, tables)
    sinks, ref = chunk_ref(dtype, D, G, n, window, tables, anchor)
    r = cw.run(WithSinks(sfa, on_device(sinks)), prob, layout, window, num_splits, varlen=varlen)
    sfa.check_decode_status()
    cw.check_against_reference(r, prob, three(ref))
    plain = cw.run(sfa, prob, "blmhd", None, 1, varlen=varlen)      # the appended rows are the plain call's, bit for bit
    assert cwg.same_appends(r, plain, prob)
    if r.spare_k is not None:
        assert not bool(r.spare_k.any()) and not bool(r.spare_v.any())


@pytest.mark.parametrize("case", list(enumerate(cw.SWEEP)), ids=lambda c: "-".join(str(x) for x in c[1]))
def test_sinks_parity_sweep_chunk(sfa, case):
    chunk_parity_case(sfa, case, False)


@pytest.mark.parametrize("case", list(enumerate(cw.SWEEP)), ids=lambda c: "-".join(str(x) for x in c[1]))
def test_sinks_parity_sweep_varlen(sfa, case):
    chunk_parity_case(sfa, case, True)


# ---- 2. the sink binds ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("call", CALLS)
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_sink_binds(sfa, dtype, call):
    """On the anchor row the heads with delta >= 0 (a sink share of at least one half) differ from the _window call's
    output by more than 10 tol (1 + max |o|), and still match the reference: a kernel that ignores `sinks` cannot pass.
    A window of 4 rows keeps |o| of the order of a V row, so that half of it is many tolerances."""
    D, G, n, window, anchor = 128, 4, 8, 4, 2
    H, tol = HKV * G, TOL[dtype]
    sinks, o_ref, _ = reference_of(call, dtype, D, G, n, window, anchor=anchor)
    r = run_call(sfa, call, dtype, D, G, n, "blmhd", window, sinks)
    plain = run_call(sfa, call, dtype, D, G, n, "blmhd", window, "window")
    sfa.check_decode_status()
    assert_o(r, o_ref, dtype, call)
    got = cw.as_float(rows_of(r.o[anchor], call), dtype)[0]                # [H, D]: the anchor row
    base = cw.as_float(rows_of(plain.o[anchor], call), dtype)[0]
    heads = [h for h in range(H) if sinks_ref.deltas(H)[h] >= 0]
    assert len(heads) == H // 2
    for h in heads:
        gap = np.abs(got[h] - base[h]).max()
        assert gap > 10 * tol * (1.0 + np.abs(base[h]).max()), (h, gap)


# ---- 3. bit identity with the _window twin where the sink has no weight --------------------------------------------------

IDENTITY_SHAPES = {"blmhd": ("bf16", 128, 8), "blhmd": ("fp16", 64, 1), "paged16": ("fp16", 128, 2), "paged64": ("bf16", 64, 16)}


@pytest.mark.parametrize("call", CALLS)
@pytest.mark.parametrize("num_splits", [1, 3])
@pytest.mark.parametrize("layout", list(IDENTITY_SHAPES))
def test_weightless_sink_is_the_window_call_bit_for_bit(sfa, layout, num_splits, call):
    """sinks = NULL, all -inf and all -1e30 each give the _window call's o and caches as bits"""
    dtype, D, G = IDENTITY_SHAPES[layout]
    n, window = cw.sweep_tokens(G), 100
    H = HKV * G
    plain = run_call(sfa, call, dtype, D, G, n, layout, window, "window", num_splits)
    for sinks in (None, np.full(H, -np.inf, np.float32), np.full(H, -1e30, np.float32)):
        r = run_call(sfa, call, dtype, D, G, n, layout, window, sinks, num_splits)
        sfa.check_decode_status()
        assert same_bits(r, plain), (call, sinks if sinks is None else float(sinks[0]))


# ---- 4. the sink is indexed by query head --------------------------------------------------------------------------------

@pytest.mark.parametrize("h", [0, 7, 8, 15])
def test_sink_is_indexed_by_query_head(sfa, h):
    """Hkv = 2, G = 8: every sink -inf but head h's.  Exactly head h's rows differ from the _window call, the other
    heads are bit-identical, and head h matches the reference."""
    dtype, D, G, n, window, anchor = "bf16", 64, 8, 5, 33, 3
    H = HKV * G
    for call, num_splits in (("single", 1), ("chunk", 2), ("varlen", 0)):
        full, _, _ = reference_of(call, dtype, D, G, n, window, anchor=anchor, shift=0.0)
        sinks = np.full(H, -np.inf, np.float32)
        sinks[h] = full[h]
        if call == "single":
            args, kw = _single_args(dtype, D, G, window, False)
            o_ref = [x[None] for x in sinks_ref.decode_window_sinks_ref(*args, sinks, dtype, **kw)["o"]]
        else:
            o_ref = [x[0] for x in sinks_ref.chunk_sinks_ref(cw.problem(dtype, D, G, n), window, sinks)]
        r = run_call(sfa, call, dtype, D, G, n, "paged16", window, sinks, num_splits)
        plain = run_call(sfa, call, dtype, D, G, n, "paged16", window, "window", num_splits)
        sfa.check_decode_status()
        assert_o(r, o_ref, dtype, call)
        assert torch.equal(r.kc, plain.kc) and torch.equal(r.vc, plain.vc)
        for b in range(len(LENS)):
            a, p = rows_of(r.o[b], call), rows_of(plain.o[b], call)        # [rows, H, D]
            others = [x for x in range(H) if x != h]
            assert torch.equal(a[:, others], p[:, others]), (call, b)
            assert not bool((a[:, h] == p[:, h]).all(dim=-1).any()), (call, b)     # every row of head h moved


# ---- 5. counted once, whatever the split count ---------------------------------------------------------------------------

@pytest.mark.parametrize("call", CALLS)
@pytest.mark.parametrize("num_splits", [1, 2, 3, 4])
def test_sink_counted_once_at_every_split_count(sfa, num_splits, call):
    """More splits than key tiles included: the seq_len 0 and 5 sequences leave split 0 nothing but the sink (single
    token, S > 1: no cached tile at all at seq_len 0; chunk: one 64-key tile for up to four splits)."""
    for dtype, D, G, layout, window, anchor in (("bf16", 64, 8, "paged16", 33, 0), ("fp16", 128, 2, "blmhd", 5000, 1)):
        n = 9
        sinks, o_ref, _ = reference_of(call, dtype, D, G, n, window, anchor=anchor)
        r = run_call(sfa, call, dtype, D, G, n, layout, window, sinks, num_splits)
        sfa.check_decode_status()
        assert_o(r, o_ref, dtype, call)


def _named_problem(dtype):
    """D = 64, Hkv = 1, G = 16, one sequence at seq_len 1000, n = 72 tokens: 1152 query rows = five 256-row q-tiles"""
    D, G, n, pos = 64, 16, 72, 1000
    rng = np.random.default_rng([31, dtype == "bf16"])
    rt = lambda *s: torch.from_numpy(rng.standard_normal(s, dtype=np.float32)).to(cw.TDT[dtype])
    kc, vc = rt(1, L, M, 1, D), rt(1, L, M, 1, D)
    return SimpleNamespace(dtype=dtype, D=D, G=G, H=G, Hkv=1, B=1, lens=(pos,), ns=(n,), qkv=rt(1, n, G + 2, D), kc=kc, vc=vc,
                           kf=kc.float().numpy(), vf=vc.float().numpy(), rot=D // 2, tables=False,
                           qb=rt(G, D), kb=rt(1, D), vb=rt(1, D))


@pytest.mark.parametrize("varlen", [False, True], ids=["chunk", "varlen"])
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_sink_is_there_when_split_zero_stages_no_tile(sfa, dtype, varlen):
    """The named case: window 33, num_splits 2.  Key tiles are 64 rows: the window of the sequence's first token starts
    in tile 15 (row 968) and the keys end in tile 16, so split 0 has tile 15 and split 1 tile 16.  The last q-tile holds
    the tokens 64 .. 71, whose windows start at row 1032 or later: in tile 16.  Its split-0 workgroup stages no tile, and
    the sink must still be in its rows' partials -- once."""
    p, window, S = _named_problem(dtype), 33, 2
    lo0, last = 1000 + 1 - window, 1000 + 64 + 1 - window
    assert lo0 // 64 == 15 and (1000 + p.ns[0] - 1) // 64 == 16 and last // 64 == 16 and 64 * p.G == 4 * 256
    base = sinks_ref.chunk_sinks_ref(p, window, None)
    sinks = sinks_ref.make_sinks(base[0][3][p.ns[0] - 1]).astype(np.float32)      # anchor: the last token, in that q-tile
    ref = sinks_ref.chunk_sinks_ref(p, window, sinks)
    dev = torch.device("cuda:0")
    n, H, D = p.ns[0], p.H, p.D
    kd, vd = p.kc.clone().to(dev), p.vc.clone().to(dev)
    sl = torch.tensor([1000], dtype=torch.int32, device=dev)
    lead = (n,) if varlen else (1, n)
    o = torch.full(lead + (H, D), 7.0, dtype=cw.TDT[dtype], device=dev)
    qkv = p.qkv.reshape(lead + (H + 2, D)).contiguous().to(dev)
    common = (p.qb.to(dev), p.kb.to(dev), p.vb.to(dev), kd, vd, sl, o)
    tail = (1, M, H, D, p.rot, M, L, LAYER, window, on_device(sinks))
    kw = dict(num_splits=S, num_heads_kv=1)
    if varlen:
        cu = torch.tensor([0, n], dtype=torch.int32, device=dev)
        sfa.flash_decode_varlen_window_sinks(qkv, *common, cu, *tail, **kw)
    else:
        sfa.flash_decode_chunk_window_sinks(qkv, *common, *tail, **kw)
    torch.cuda.synchronize()
    sfa.check_decode_status()
    tol = TOL[dtype]
    got = o.float().cpu().numpy().reshape(n, H, D)
    np.testing.assert_allclose(got, ref[0][0], atol=tol, rtol=tol)
    # and the sink is material in those rows: without it they are many tolerances away
    gap = np.abs(base[0][0][64:] - ref[0][0][64:]).max()
    assert gap > 10 * tol, gap
    np.testing.assert_array_equal(cw.as_float(cw.bits(vd.cpu())[0, LAYER, 1000:1000 + n], dtype), ref[0][2])


# ---- 6. extremes ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("call", CALLS)
@pytest.mark.parametrize("num_splits", [1, 3])
def test_sink_extremes(sfa, num_splits, call):
    """delta = +100 on every head: a finite output within tolerance of the reference (about e^-100 of the windowed one),
    no NaN, no overflow.  delta = -100: the sink's weight is below half an ulp of the row sum, the _window output bit
    for bit."""
    dtype, D, G, n, layout, window, anchor = "fp16", 64, 4, 9, "paged64", 100, 2
    plain = run_call(sfa, call, dtype, D, G, n, layout, window, "window", num_splits)
    sinks, o_ref, _ = reference_of(call, dtype, D, G, n, window, anchor=anchor, shift=100.0)
    assert max(np.abs(x).max() for x in o_ref) < 1e-30
    r = run_call(sfa, call, dtype, D, G, n, layout, window, sinks, num_splits)
    sfa.check_decode_status()
    for a in r.o:
        assert bool(torch.isfinite(a.view(cw.TDT[dtype]).float()).all())
    assert_o(r, o_ref, dtype, call)
    assert torch.equal(r.kc, plain.kc) and torch.equal(r.vc, plain.vc)
    sinks, o_ref, _ = reference_of(call, dtype, D, G, n, window, anchor=anchor, shift=-100.0)
    r = run_call(sfa, call, dtype, D, G, n, layout, window, sinks, num_splits)
    sfa.check_decode_status()
    assert same_bits(r, plain)
    assert_o(r, o_ref, dtype, call)


@pytest.mark.parametrize("call", CALLS)
def test_sink_is_not_scaled_by_the_softmax_scale(sfa, call):
    """softmax_scale = 0.25 / sqrt(D): the scores shrink fourfold, the sink does not; parity still holds"""
    for dtype, D, G, layout, num_splits in (("bf16", 64, 8, "blhmd", 2), ("fp16", 128, 1, "paged16", 1)):
        n, window, anchor, scale = 9, 100, 3, 0.25 / np.sqrt(D)
        sinks, o_ref, _ = reference_of(call, dtype, D, G, n, window, anchor=anchor, scale=scale)
        unscaled, o_other, _ = reference_of(call, dtype, D, G, n, window, anchor=anchor)
        assert np.abs(sinks - unscaled).max() > 1.0             # (the two problems really differ)
        r = run_call(sfa, call, dtype, D, G, n, layout, window, sinks, num_splits, softmax_scale=scale)
        sfa.check_decode_status()
        assert_o(r, o_ref, dtype, call)


# ---- 7. unread memory ----------------------------------------------------------------------------------------------------

def sinks_inside_nan(sinks):
    """the same values as a view into a larger device buffer with NaN on both sides"""
    H = len(sinks)
    buf = torch.full((3 * H + 5,), float("nan"), dtype=torch.float32, device="cuda:0")
    view = buf[H + 3:2 * H + 3]
    view.copy_(on_device(sinks))
    assert view.is_contiguous() and view.data_ptr() % 4 == 0 and view.data_ptr() != buf.data_ptr()
    return view


@pytest.mark.parametrize("num_splits", [1, 3])
@pytest.mark.parametrize("window", [17, 100])
def test_sinks_read_nothing_around_them_or_below_the_window(sfa, window, num_splits):
    """`sinks` as a view between NaNs gives the bits of a tensor of its own; and with that view the twins' unread-memory
    cases hold: NaN / Inf in every cache row below lo_0 and at or beyond pos + n, in the other layer and the spare pages,
    -1 in the freed block_table entries."""
    dtype, D, G, n, ps = "bf16", 128, 4, 40, 16                 # (the shapes of the twins' cases)
    for call in CALLS:
        sinks, o_ref, _ = reference_of(call, dtype, D, G, n, window, anchor=1)
        view = sinks_inside_nan(sinks)
        r = run_call(sfa, call, dtype, D, G, n, f"paged{ps}", window, view, num_splits)
        own = run_call(sfa, call, dtype, D, G, n, f"paged{ps}", window, sinks, num_splits)
        sfa.check_decode_status()
        assert same_bits(r, own)
        assert_o(r, o_ref, dtype, call)
        shim = WithSinks(sfa, view)
        if call == "single":
            w1.test_window_reads_nothing_below_it(shim, window, ps, num_splits)
        else:
            cwg.unread_memory_case(shim, window, ps, num_splits, call == "varlen")


# ---- 8. rejection --------------------------------------------------------------------------------------------------------

def test_sinks_reject_like_the_window_calls(sfa):
    """seq_len out of range and a bad append page: NaN rows in o, an untouched cache and the twins' status bits -- the
    twins' own cases, run through the sinks calls (bf16, D 128, G 4, window 100)"""
    sinks, _ = single_ref("bf16", 128, 4, 100, False, 3)
    shim = WithSinks(sfa, on_device(sinks))
    w1.test_window_rejects_like_decode(shim)
    cwg.rejection_case(shim, False)
    cwg.rejection_case(shim, True)


@pytest.mark.parametrize("num_splits", [1, 3])
def test_sinks_bad_read_page_gives_nan(sfa, num_splits):
    """a bad entry on a page the window reads: the sequence's outputs are NaN -- the NaN survives the sink fold -- and
    the status is raised; the same entry below the window is never looked at (fp16, D 128, G 8, window 100)"""
    sinks, _ = single_ref("fp16", 128, 8, 100, False, 3)
    shim = WithSinks(sfa, on_device(sinks))
    w1.test_window_bad_table_entry_inside_and_below_the_window(shim, num_splits)
    cwg.bad_read_page_case(shim, num_splits, False)
    cwg.bad_read_page_case(shim, num_splits, True)


# ---- 9. graph replay -----------------------------------------------------------------------------------------------------

def test_chunk_window_sinks_graph_replay(sfa):
    """One captured flash_decode_chunk_window_sinks call, replayed with other sinks contents and other seq_len: both are
    read on the device, so each replay matches its own reference."""
    dtype, D, G, n, window = "fp16", 128, 2, 40, 33
    dev = torch.device("cuda:0")
    probs = [cw.make_problem(dtype, D, G, lens, (n,) * 4, seed=s) for s, lens in ((1, (3, 700, 64, 31)), (2, (1300, 0, 97, 500)))]
    p0 = probs[0]
    dt = cw.TDT[dtype]
    qkv = torch.zeros(p0.B, n, p0.H + 2 * HKV, D, dtype=dt, device=dev)
    kd = torch.zeros(p0.B, L, M, HKV, D, dtype=dt, device=dev)
    vd = torch.zeros_like(kd)
    o = torch.zeros(p0.B, n, p0.H, D, dtype=dt, device=dev)
    sl = torch.zeros(p0.B, dtype=torch.int32, device=dev)
    sk = torch.zeros(p0.H, dtype=torch.float32, device=dev)
    qb, kb, vb = (torch.zeros_like(x).to(dev) for x in (p0.qb, p0.kb, p0.vb))
    call = lambda: sfa.flash_decode_chunk_window_sinks(qkv, qb, kb, vb, kd, vd, sl, o, p0.B, M, p0.H, D, p0.rot, M, L,
                                                       LAYER, window, sk, num_splits=2, num_heads_kv=HKV)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    outs = []
    with torch.cuda.stream(side):
        call()                                              # warm-up: the stream's workspace exists before the capture
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            call()
        for i, p in enumerate(probs):
            base = sinks_ref.chunk_sinks_ref(p, window, None)
            sinks = sinks_ref.make_sinks(base[i + 1][3][0]).astype(np.float32)     # another anchor, other contents
            for dst, src in ((qkv, p.qkv), (kd, p.kc), (vd, p.vc), (qb, p.qb), (kb, p.kb), (vb, p.vb)):
                dst.copy_(src.to(dev))
            sk.copy_(torch.from_numpy(sinks))
            o.fill_(7.0)
            sl.copy_(torch.tensor(list(p.lens), dtype=torch.int32))
            graph.replay()
            side.synchronize()
            sfa.check_decode_status(dev)
            ob = cw.bits(o.cpu())
            r = SimpleNamespace(o=[ob[b] for b in range(p.B)], kc=cw.bits(kd.cpu()), vc=cw.bits(vd.cpu()))
            cw.check_against_reference(r, p, three(sinks_ref.chunk_sinks_ref(p, window, sinks)))
            outs.append(ob)
            # the sink of this replay is material: the windowed reference is many tolerances away in the anchor's row
            gap = np.abs(cw.as_float(ob[i + 1][0], dtype) - base[i + 1][0][0]).max()
            assert gap > 10 * TOL[dtype], gap
    assert not torch.equal(outs[0], outs[1])


# ---- 10. bad arguments through Python ------------------------------------------------------------------------------------

@pytest.mark.parametrize("call", CALLS)
def test_sinks_bad_arguments(sfa, call):
    dtype, D, G, n, window = "fp16", 64, 2, 5, 8
    H = HKV * G
    good = torch.zeros(H, dtype=torch.float32, device="cuda:0")
    bad = {"dtype": good.half(), "shape": torch.zeros(H + 1, dtype=torch.float32, device="cuda:0"),
           "rank": good[None], "device": good.cpu(),
           "contiguous": torch.zeros(2 * H, dtype=torch.float32, device="cuda:0")[::2], "tensor": [0.0] * H}
    for what, sinks in bad.items():
        with pytest.raises(RuntimeError, match="sinks"):
            s = WithSinks(sfa, sinks)
            if call == "single":
                w1.run(s, dtype, D, G, "blmhd", window)
            else:
                cw.run(s, cw.problem(dtype, D, G, n), "blmhd", window, varlen=call == "varlen")
    for w in (0, -3):
        with pytest.raises(RuntimeError, match="window"):
            run_call(sfa, call, dtype, D, G, n, "blmhd", w, good)
    run_call(sfa, call, dtype, D, G, n, "blmhd", window, good)       # and the good one is accepted
    sfa.check_decode_status()
