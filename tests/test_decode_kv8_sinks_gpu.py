"""GPU checks of sfa_decode_kv8_window_sinks / sfa_decode_chunk_kv8_window_sinks / sfa_decode_varlen_kv8_window_sinks
(attention sinks in the three windowed decode calls over an fp8 e4m3 KV cache) through the Python operators: parity with
the fp64 references of tests/kv8_sinks_ref.py over the twins' own pairwise-covering sweeps, that the sink binds, is indexed
by query head and is scaled by nothing, that it is counted once whatever the split count, bit-identity with the
_kv8_window twin where the sink has no weight, the extremes, unread memory, rejection, graph replay, the operators'
argument checks and a two-layer stack fed the way a server feeds it.

The device is checked as the twins are: (a) the appended bytes against the reference quantiser by the twins' own rules
(chunk_kv8_ref.check_bytes; check_appended_and_untouched of tests/test_decode_kv8_window_gpu.py), (b) o against the fp64
sink attention over the bytes the device stored, at window_ref.TOL (fp16 2e-3, bf16 1.6e-2, atol = rtol, elementwise,
nothing exempt) -- a sink multiplies the output by a factor in (0, 1], so the bound that holds for the twins holds here.

The frame is the fp8 window tests': B = 4 sequences at seq_len = (0, 5, 130, 1000), 2 kv heads, 2 layers, memory_max_len
1408, q / k / v bias and a partial rotary embedding; their run() harnesses drive the sinks calls through
kv8_sinks_ref.WithSinks.  Sinks: sinks[h] = lse_ref[anchor, h] + delta_h with delta = linspace(-3, 3, H): on the anchor
row (chunk / varlen: token 0 of the anchor sequence) the sink's share of the softmax is sigmoid(delta_h), 0.047 .. 0.953.
"""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import chunk_kv8_ref as ckr
import chunk_kv8_window_ref as ckw
import kv8_ref
import kv8_sinks_ref as ksr
import kv8_window_ref as kwr
import test_decode_chunk_kv8_window_gpu as tcw
import test_decode_kv8_window_gpu as tkw
from chunk_window_ref import TDT, as_float, bits
from kv8_sinks_ref import BINDS, HKV, L, LAYER, LENS, M, SCALED, TOL, WithSinks, window_lo
from oracle import round_to

pytestmark = pytest.mark.gpu

CALLS = ("single", "chunk", "varlen")


@pytest.fixture(scope="module")
def sfa():
    assert torch.cuda.is_available(), "GPU tests need a GPU (run with -m gpu on the MI355X box)"
    import starflashattention_amd as m
    m._lib.load()                  # fail loudly if the HIP library is missing
    m.check_decode_status()
    return m


def on_device(sinks):
    """float32 [H] on the GPU (None stays None = NULL)"""
    return None if sinks is None else torch.from_numpy(np.asarray(sinks, np.float32)).to("cuda:0")


def shim_of(sfa, sinks, **extra):
    """`sfa` itself for sinks="twin", else the package with the sinks calls in the twins' places"""
    if isinstance(sinks, str):
        return sfa
    return WithSinks(sfa, sinks if isinstance(sinks, torch.Tensor) else on_device(sinks), **extra)


def run_call(sfa, call, dtype, D, G, n, layout, window, sinks, num_splits=0, tables=False, k_factors=(1.0, 1.0), p=None,
             softmax_scale=None):
    """One call of `call` in CALLS with `sinks` (float32 array, device tensor or None = NULL) -- or, sinks="twin", its
    _kv8_window twin -- on the frame (p: another chunk / varlen problem).  Returns o as a list per sequence of [rows, H, D]
    bits (.o) and float32 (.of), and the canonical caches .k8 / .v8."""
    s = shim_of(sfa, sinks)
    if call == "single":
        r = tkw.run(s, dtype, D, G, layout, window, num_splits, softmax_scale, tables=tables, k_factors=k_factors)
        return SimpleNamespace(o=[r.o[b][None] for b in range(len(LENS))], of=[r.of[b][None] for b in range(len(LENS))],
                               k8=r.kc, v8=r.vc, spare_k=r.spare_k, spare_v=r.spare_v, raw=r)
    p = ckw.problem(dtype, D, G, n, tables) if p is None else p
    assert softmax_scale is None or p.scale == softmax_scale
    r = ckw.run(s, p, layout, window, num_splits, varlen=call == "varlen")
    r.o = [x.numpy() for x in r.o]
    return r


def same_bits(r, other):
    return (all(np.array_equal(a, b) for a, b in zip(r.o, other.o)) and np.array_equal(r.k8, other.k8)
            and np.array_equal(r.v8, other.v8))


def check_call(r, call, dtype, D, G, n, window, sinks, ref, tables=False, k_factors=(1.0, 1.0), p=None, k_bytes=True,
               scale=None):
    """(a) and (b) for one run; ref = ksr.single_ref(...)[1] or ksr.chunk_ref(...)[1] / ksr.chunk_kv8_sinks_ref(...)"""
    if call == "single":
        c = kwr.caches(D, k_factors)
        tkw.check_appended_and_untouched(r.raw, ref, D, k_before=c.k8, v_before=c.v8)
        ksr.check_single_o(r.raw, ref, dtype, window, sinks, c.ks, c.vs, scale=scale)
    else:
        p = ckw.problem(dtype, D, G, n, tables) if p is None else p
        ksr.check_chunk(r, p, window, sinks, ref, k_bytes=k_bytes)


def reference_of(call, dtype, D, G, n, window, tables=False, anchor=None, shift=None):
    """(sinks, the reference) on the frame"""
    if call == "single":
        return ksr.single_ref(dtype, D, G, window, tables, anchor, shift)
    return ksr.chunk_ref(dtype, D, G, n, window, tables, anchor, shift)


def run_and_check(sfa, call, dtype, D, G, n, layout, window, num_splits=0, tables=False, anchor=0, shift=None):
    sinks, ref = reference_of(call, dtype, D, G, n, window, tables, anchor, shift)
    r = run_call(sfa, call, dtype, D, G, n, layout, window, sinks, num_splits, tables)
    sfa.check_decode_status()
    check_call(r, call, dtype, D, G, n, window, sinks, ref, tables, k_bytes=tables)
    return r, sinks, ref


def spare_untouched(r, fill):
    return r.spare_k is None or (bool((torch.as_tensor(r.spare_k) == fill).all()) and bool((torch.as_tensor(r.spare_v) == fill).all()))


# ---- 1. parity sweeps: the twins' own, with material sinks; the anchors cover seq_len 0, 5, 130 and 1000 -----------------

@pytest.mark.parametrize("case", list(enumerate(kwr.SWEEP)), ids=lambda c: "-".join(str(x) for x in c[1]))
def test_kv8_sinks_parity_sweep_single(sfa, case):
    i, (dtype, D, layout, G, num_splits, window) = case
    tables, anchor = bool(i & 1), i % 4
    sinks, ref = ksr.single_ref(dtype, D, G, window, tables, anchor)
    r = run_call(sfa, "single", dtype, D, G, 1, layout, window, sinks, num_splits, tables)
    sfa.check_decode_status()
    ksr.check_single_o(r.raw, ref, dtype, window, sinks, kwr.caches(D).ks, kwr.caches(D).vs)
    # the appended bytes are sfa_decode_kv8's, bit for bit, whatever the sink
    tkw.check_appended_and_untouched(r.raw, ref, D, like=tkw._plain_kv8(dtype, D, G, tables))
    assert spare_untouched(r, 0)


def chunk_parity_case(sfa, case, varlen):
    i, (dtype, D, layout, G, num_splits, window, n) = case
    call, anchor = "varlen" if varlen else "chunk", (i + 1) % 4
    # the rotary tables, as in the twins' sweep (criterion (a) at the frame's long positions); every fourth case a second
    # time with the trigonometry computed in the kernel, its appended K bytes held against the plain call's instead
    for tables in (True, False) if i % 4 == 0 else (True,):
        p = ckw.problem(dtype, D, G, n, tables)
        sinks, ref = ksr.chunk_ref(dtype, D, G, n, window, tables, anchor)
        r = run_call(sfa, call, dtype, D, G, n, layout, window, sinks, num_splits, tables)
        sfa.check_decode_status()
        ksr.check_chunk(r, p, window, sinks, ref, k_bytes=tables)
        plain = ckw.run(sfa, p, "blmhd", None, 1, varlen=varlen)
        assert tcw.same_appends(r, plain, p)
        assert spare_untouched(r, ckw.FILL)


@pytest.mark.parametrize("case", list(enumerate(ckw.SWEEP)), ids=lambda c: "-".join(str(x) for x in c[1]))
def test_kv8_sinks_parity_sweep_chunk(sfa, case):
    chunk_parity_case(sfa, case, False)


@pytest.mark.parametrize("case", list(enumerate(ckw.SWEEP)), ids=lambda c: "-".join(str(x) for x in c[1]))
def test_kv8_sinks_parity_sweep_varlen(sfa, case):
    chunk_parity_case(sfa, case, True)


# ---- 2. the sink binds ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("call", CALLS)
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_kv8_sink_binds(sfa, dtype, call):
    """On the anchor row the heads with delta >= 0 (a sink share of at least one half) leave the _kv8_window call's output
    by more than 10 tol (1 + max |o|), and still match the reference: a kernel that ignores `sinks` cannot pass.  (The
    references alone meet the bar: tests/test_decode_kv8_sinks_cpu.py.)"""
    D, G, n, window, anchor = (BINDS[k] for k in ("D", "G", "n", "window", "anchor"))
    H, tol = HKV * G, TOL[dtype]
    r, sinks, _ = run_and_check(sfa, call, dtype, D, G, n, "blmhd", window, anchor=anchor)
    plain = run_call(sfa, call, dtype, D, G, n, "blmhd", window, "twin")
    sfa.check_decode_status()
    got, base = r.of[anchor][0], plain.of[anchor][0]            # [H, D]: the anchor row
    heads = [h for h in range(H) if ksr.deltas(H)[h] >= 0]
    assert len(heads) == H // 2
    for h in heads:
        gap = np.abs(got[h] - base[h]).max()
        assert gap > 10 * tol * (1.0 + np.abs(base[h]).max()), (h, gap)


# ---- 3. bit identity with the _kv8_window twin where the sink has no weight ------------------------------------------------

IDENTITY_SHAPES = {"blmhd": ("bf16", 128, 8), "blhmd": ("fp16", 64, 1), "paged16": ("fp16", 128, 2)}


@pytest.mark.parametrize("call", CALLS)
@pytest.mark.parametrize("num_splits", [1, 3])
@pytest.mark.parametrize("layout", list(IDENTITY_SHAPES))
def test_weightless_kv8_sink_is_the_twin_bit_for_bit(sfa, layout, num_splits, call):
    """sinks = NULL, all -inf and all -1e30 each give the _kv8_window call's o and both caches as bits"""
    dtype, D, G = IDENTITY_SHAPES[layout]
    n, window = {8: 45, 1: 70, 2: 5}[G], 100
    H = HKV * G
    plain = run_call(sfa, call, dtype, D, G, n, layout, window, "twin", num_splits)
    for sinks in (None, np.full(H, -np.inf, np.float32), np.full(H, -1e30, np.float32)):
        r = run_call(sfa, call, dtype, D, G, n, layout, window, sinks, num_splits)
        sfa.check_decode_status()
        assert all(np.isfinite(x).all() for x in r.of)
        assert same_bits(r, plain), (call, sinks if sinks is None else float(sinks[0]))


# ---- 4. the sink is indexed by query head and scaled by nothing ----------------------------------------------------------------

@pytest.mark.parametrize("h", [0, 7, 8, 15])
def test_kv8_sink_is_indexed_by_query_head(sfa, h):
    """Hkv = 2, G = 8: every sink -inf but head h's.  Exactly head h's rows differ from the _kv8_window call, the other
    heads are bit-identical, the caches are the twin's, and head h matches the reference."""
    dtype, D, G, n, window, anchor = "bf16", 64, 8, 5, 33, 3
    H = HKV * G
    for call, num_splits in (("single", 1), ("chunk", 2), ("varlen", 0)):
        full, _ = reference_of(call, dtype, D, G, n, window, anchor=anchor, shift=0.0)
        sinks = np.full(H, -np.inf, np.float32)
        sinks[h] = full[h]
        ref = (ksr.single_with(dtype, D, G, window, sinks) if call == "single"
               else ksr.chunk_kv8_sinks_ref(ckw.problem(dtype, D, G, n), window, sinks))
        r = run_call(sfa, call, dtype, D, G, n, "paged16", window, sinks, num_splits)
        plain = run_call(sfa, call, dtype, D, G, n, "paged16", window, "twin", num_splits)
        sfa.check_decode_status()
        check_call(r, call, dtype, D, G, n, window, sinks, ref, k_bytes=False)
        assert np.array_equal(r.k8, plain.k8) and np.array_equal(r.v8, plain.v8)
        others = [x for x in range(H) if x != h]
        for b in range(len(LENS)):
            a, q = r.o[b], plain.o[b]                           # [rows, H, D] bits
            assert np.array_equal(a[:, others], q[:, others]), (call, b)
            assert not (a[:, h] == q[:, h]).all(axis=-1).any(), (call, b)      # every row of head h moved


@pytest.mark.parametrize("call", CALLS)
def test_kv8_sink_is_not_scaled_by_k_scale_or_head_dim_inv(sfa, call):
    """k_scale / v_scale with factors (0.5, 2) per kv head -- four distinct scales -- at Hkv = 2, G = 8: the device matches
    the reference, and misses the reference whose sink is multiplied by k_scale[hk] and the one whose sink is multiplied by
    head_dim_inv (either is more than 2 tol (1 + |o|) from the right one: tests/test_decode_kv8_sinks_cpu.py)."""
    s = SCALED
    dtype, D, G, n, window, anchor, kf = (s[k] for k in ("dtype", "D", "G", "n", "window", "anchor", "k_factors"))
    tol = TOL[dtype]
    if call == "single":
        sinks, ref = ksr.single_ref(dtype, D, G, window, anchor=anchor, k_factors=kf)
        ks, p = kwr.caches(D, kf).ks, None
        o_of = lambda sk: ksr.single_with(dtype, D, G, window, sk, k_factors=kf)["o64"][anchor]
    else:
        p = ksr.scaled_problem()
        sinks = ksr.anchor_sinks(p, window, anchor)
        ref, ks = ksr.chunk_kv8_sinks_ref(p, window, sinks), p.ks
        o_of = lambda sk: ksr.chunk_kv8_sinks_ref(p, window, sk)[0]["o"][anchor][0]
    for layout, num_splits in (("blmhd", 1), ("paged16", 3)):
        r = run_call(sfa, call, dtype, D, G, n, layout, window, sinks, num_splits, k_factors=kf, p=p)
        sfa.check_decode_status()
        check_call(r, call, dtype, D, G, n, window, sinks, ref, k_factors=kf, p=p, k_bytes=False)
        got = r.of[anchor][0]
        for what, wrong in ksr.wrongly_scaled(sinks.astype(np.float64), ks, D, G).items():
            o = o_of(wrong)
            assert not np.all(np.abs(got - o) <= tol * (1.0 + np.abs(o))), what
            for hk in range(HKV):                               # under either kv head, with its own scale
                h = slice(hk * G, (hk + 1) * G)
                assert (np.abs(got[h] - o[h]) > tol * (1.0 + np.abs(o[h]))).any(), (what, hk)


# ---- 5. counted once, whatever the split count ---------------------------------------------------------------------------

@pytest.mark.parametrize("call", CALLS)
@pytest.mark.parametrize("num_splits", [1, 2, 3, 4])
def test_kv8_sink_counted_once_at_every_split_count(sfa, num_splits, call):
    """More splits than key tiles included: the seq_len 0 and 5 sequences leave split 0 nothing but the sink (single
    token, S > 1: no cached tile at all at seq_len 0; chunk: one 64-key tile for up to four splits)."""
    for dtype, D, G, layout, window, anchor in (("bf16", 64, 8, "paged16", 33, 0), ("fp16", 128, 2, "blmhd", 5000, 1)):
        run_and_check(sfa, call, dtype, D, G, 9, layout, window, num_splits, anchor=anchor)


@pytest.mark.parametrize("num_splits", [2, 3, 4])
def test_kv8_sink_with_more_splits_than_tiles_single_token(sfa, num_splits):
    """The single-token equivalent of the named case below: at seq_len 5 the five cached rows are one 32-row tile of one
    wave of one split, at seq_len 0 there is none; the other splits merge nothing but, in split 0, the sink.  Anchored on
    the seq_len 5 sequence, where the sink is material: without it the rows are many tolerances away."""
    dtype, D, G, window, anchor = "fp16", 64, 16, 100, 1
    r, sinks, ref = run_and_check(sfa, "single", dtype, D, G, 1, "blhmd", window, num_splits, anchor=anchor)
    base = ksr.single_ref(dtype, D, G, window)[1]
    assert np.abs(base["o64"][anchor] - ref["o64"][anchor]).max() > 10 * TOL[dtype]


def _named_problem(dtype):
    """D = 64, Hkv = 1, G = 16, one sequence at seq_len 1000, n = 72 tokens: 1152 query rows = five 256-row q-tiles"""
    D, G, n, pos = 64, 16, 72, 1000
    rng = np.random.default_rng([31, dtype == "bf16"])
    kc, vc = (rng.standard_normal((1, L, M, 1, D)).astype(np.float32) for _ in range(2))
    ks, vs = kwr.amax_scale(kc), kwr.amax_scale(vc)
    r = lambda *s: round_to(rng.standard_normal(s), dtype).astype(np.float32)
    return SimpleNamespace(dtype=dtype, D=D, G=G, H=G, B=1, lens=(pos,), ns=(n,), tok=[r(n, G + 2, D)], ks=ks, vs=vs,
                           k8=kv8_ref.quantize(kc, ks), v8=kv8_ref.quantize(vc, vs), rot=D // 2, biases=(r(G, D), r(1, D), r(1, D)))


@pytest.mark.parametrize("varlen", [False, True], ids=["chunk", "varlen"])
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_kv8_sink_is_there_when_split_zero_stages_no_tile(sfa, dtype, varlen):
    """The named case: window 33, num_splits 2.  Key tiles are 64 rows: the window of the sequence's first token starts
    in tile 15 (row 968) and the keys end in tile 16, so split 0 has tile 15 and split 1 tile 16.  The last q-tile holds
    the tokens 64 .. 71, whose windows start at row 1032 or later: in tile 16.  Its split-0 workgroup stages no tile, and
    the sink must still be in its rows' partials -- once, and before v_scale meets them."""
    p, window, S = _named_problem(dtype), 33, 2
    pos, n, H, D = p.lens[0], p.ns[0], p.H, p.D
    lo0, last = pos + 1 - window, pos + 64 + 1 - window
    assert lo0 // 64 == 15 and (pos + n - 1) // 64 == 16 and last // 64 == 16 and 64 * p.G == 4 * 256
    cos, sin = ckw.rotary_tables(dtype, p.rot)
    k_ref, v_ref = p.k8.copy(), p.v8.copy()
    base = ckw.chunk_kv8_window_ref(p.tok, k_ref, v_ref, p.lens, LAYER, p.rot, dtype, window, p.ks, p.vs, q_bias=p.biases[0],
                                    k_bias=p.biases[1], v_bias=p.biases[2], cos_table=cos, sin_table=sin)
    q16 = base["q16"][0]
    _, lse = ksr.attend_sinks(q16[n - 1:], k_ref[0, LAYER], v_ref[0, LAYER], pos + n - 1, window, None, p.ks, p.vs)
    sinks = ksr.make_sinks(lse[0]).astype(np.float32)           # anchor: the last token, in that q-tile
    dev = torch.device("cuda:0")
    dt = TDT[dtype]
    t16 = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dt).to(dev)
    kd, vd = torch.from_numpy(p.k8).to(dev), torch.from_numpy(p.v8).to(dev)
    sl = torch.tensor([pos], dtype=torch.int32, device=dev)
    lead = (n,) if varlen else (1, n)
    o = torch.full(lead + (H, D), 7.0, dtype=dt, device=dev)
    qkv = t16(p.tok[0]).view(lead + (H + 2, D))
    common = (*(t16(x) for x in p.biases), kd, vd, sl, o)
    tail = (1, M, H, D, p.rot, M, L, LAYER, window, on_device(sinks))
    kw = dict(num_splits=S, num_heads_kv=1, k_scale=torch.from_numpy(p.ks).to(dev), v_scale=torch.from_numpy(p.vs).to(dev),
              rotary_cos_table=t16(cos), rotary_sin_table=t16(sin))
    if varlen:
        cu = torch.tensor([0, n], dtype=torch.int32, device=dev)
        sfa.flash_decode_varlen_kv8_window_sinks(qkv, *common, cu, *tail, **kw)
    else:
        sfa.flash_decode_chunk_kv8_window_sinks(qkv, *common, *tail, **kw)
    torch.cuda.synchronize()
    sfa.check_decode_status()
    k_out, v_out = kd.cpu().numpy(), vd.cpu().numpy()
    ckr.check_bytes(p.lens, p.ns, k_out, v_out, p.k8, p.v8, k_ref, v_ref)
    want, _ = ksr.attend_sinks(q16, k_out[0, LAYER], v_out[0, LAYER], pos, window, sinks, p.ks, p.vs)
    tol = TOL[dtype]
    got = o.float().cpu().numpy().reshape(n, H, D)
    assert np.isfinite(got).all()
    np.testing.assert_allclose(got, want, atol=tol, rtol=tol)
    # and the sink is material in those rows: without it they are many tolerances away
    plain, _ = ksr.attend_sinks(q16[64:], k_out[0, LAYER], v_out[0, LAYER], pos + 64, window, None, p.ks, p.vs)
    gap = np.abs(plain - want[64:]).max()
    assert gap > 10 * tol, gap


# ---- 6. extremes ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("call", CALLS)
@pytest.mark.parametrize("num_splits", [1, 3])
def test_kv8_sink_extremes(sfa, num_splits, call):
    """delta = +100 on every head: a finite output within tolerance of the reference (about e^-100 of the windowed one),
    no NaN, no overflow.  delta = -100: the sink's weight is below half an ulp of the row sum, the _kv8_window output bit
    for bit."""
    dtype, D, G, n, layout, window, anchor = "fp16", 64, 4, 9, "paged64", 100, 2
    plain = run_call(sfa, call, dtype, D, G, n, layout, window, "twin", num_splits)
    sinks, ref = reference_of(call, dtype, D, G, n, window, anchor=anchor, shift=100.0)
    r = run_call(sfa, call, dtype, D, G, n, layout, window, sinks, num_splits)
    sfa.check_decode_status()
    assert all(np.isfinite(x).all() for x in r.of)
    assert max(np.abs(x[0]).max() for x in r.of[anchor:anchor + 1]) < 1e-30
    check_call(r, call, dtype, D, G, n, window, sinks, ref, k_bytes=False)
    assert np.array_equal(r.k8, plain.k8) and np.array_equal(r.v8, plain.v8)
    sinks, ref = reference_of(call, dtype, D, G, n, window, anchor=anchor, shift=-100.0)
    r = run_call(sfa, call, dtype, D, G, n, layout, window, sinks, num_splits)
    sfa.check_decode_status()
    assert same_bits(r, plain)
    check_call(r, call, dtype, D, G, n, window, sinks, ref, k_bytes=False)


@pytest.mark.parametrize("call", CALLS)
def test_kv8_sink_is_not_scaled_by_the_softmax_scale(sfa, call):
    """softmax_scale = 0.25 / sqrt(D): the scores shrink fourfold, the sink does not; parity holds.  The argument matters:
    with the same sinks the reference at the default scale is more than 2 tol (1 + |o|) away, so a call that ignored
    softmax_scale, or applied it to the sink as well, would not pass."""
    for dtype, D, G, layout, num_splits in (("bf16", 64, 8, "blhmd", 2), ("fp16", 128, 1, "paged16", 1)):
        n, window, anchor, scale, tol = 9, 100, 3, 0.25 / float(np.sqrt(D)), TOL[dtype]
        if call == "single":
            sinks, ref = ksr.single_ref(dtype, D, G, window, anchor=anchor, scale=scale)
            p, mine = None, ref["o64"]
            other = ksr.single_with(dtype, D, G, window, sinks)["o64"]
            scaled_sink = ksr.single_with(dtype, D, G, window, 0.25 * sinks.astype(np.float64), scale=scale)["o64"]
        else:
            p = ckw.make_problem(dtype, D, G, LENS, (n,) * 4, scale=scale)
            sinks = ksr.anchor_sinks(p, window, anchor)
            ref = ksr.chunk_kv8_sinks_ref(p, window, sinks)
            mine = np.concatenate(ref[0]["o"])
            other = np.concatenate(ksr.chunk_kv8_sinks_ref(ckw.problem(dtype, D, G, n), window, sinks)[0]["o"])
            scaled_sink = np.concatenate(ksr.chunk_kv8_sinks_ref(p, window, 0.25 * sinks.astype(np.float64))[0]["o"])
        for wrong in (other, scaled_sink):                      # (asserted on the references alone)
            assert (np.abs(wrong - mine) > 2 * tol * (1.0 + np.abs(mine))).any()
        r = run_call(sfa, call, dtype, D, G, n, layout, window, sinks, num_splits, p=p, softmax_scale=scale)
        sfa.check_decode_status()
        check_call(r, call, dtype, D, G, n, window, sinks, ref, p=p, k_bytes=False, scale=scale)


# ---- 7. unread memory ----------------------------------------------------------------------------------------------------

def sinks_inside_nan(sinks):
    """the same values as a view into a larger device buffer with NaN on both sides"""
    H = len(sinks)
    buf = torch.full((3 * H + 5,), float("nan"), dtype=torch.float32, device="cuda:0")
    view = buf[H + 3:2 * H + 3]
    view.copy_(on_device(sinks))
    assert view.is_contiguous() and view.data_ptr() % 4 == 0 and view.data_ptr() != buf.data_ptr()
    return view


@pytest.mark.parametrize("call", CALLS)
@pytest.mark.parametrize("num_splits", [1, 3])
def test_kv8_sinks_view_between_nans_gives_the_bits_of_a_tensor_of_its_own(sfa, num_splits, call):
    dtype, D, G, n, window = "bf16", 128, 4, 40, 100
    sinks, ref = reference_of(call, dtype, D, G, n, window, anchor=1)
    r = run_call(sfa, call, dtype, D, G, n, "paged16", window, sinks_inside_nan(sinks), num_splits)
    own = run_call(sfa, call, dtype, D, G, n, "paged16", window, sinks, num_splits)
    sfa.check_decode_status()
    assert same_bits(r, own)
    check_call(r, call, dtype, D, G, n, window, sinks, ref, k_bytes=False)


@pytest.mark.parametrize("varlen", [False, True], ids=["chunk", "varlen"])
@pytest.mark.parametrize("num_splits", [1, 3])
@pytest.mark.parametrize("layout", ["blmhd", "paged16", "paged64"])
def test_kv8_sinks_read_nothing_outside_the_window(sfa, layout, num_splits, varlen):
    """The twins' unread-memory case (lo_0 on and beside a 64-row tile, a 32-row boundary and a page boundary; 0x7F in
    every byte outside [lo_0, pos + n), -1 in the table entries below the window and after the last page) with `sinks` a
    view between NaNs: the run demands the bits of the run on benign bytes and a clean status word; and the clean run is
    the right answer."""
    D, dtype = (64, "fp16") if layout != "paged64" else (128, "bf16")
    lens = tuple(lo + tcw.UNREAD_WINDOW - 1 for lo in tcw.UNREAD_LO0)
    p = ckw.make_problem(dtype, D, 4, lens, (tcw.UNREAD_N,) * len(lens), seed=9, tables=True)
    assert tuple(window_lo(pos, tcw.UNREAD_WINDOW) for pos in p.lens) == tcw.UNREAD_LO0
    sinks = ksr.anchor_sinks(p, tcw.UNREAD_WINDOW, 4)
    clean = tcw.unread_memory_case(WithSinks(sfa, sinks_inside_nan(sinks)), p, tcw.UNREAD_WINDOW, layout, num_splits, varlen)
    if num_splits == 1:
        ksr.check_chunk(clean, p, tcw.UNREAD_WINDOW, sinks, ksr.chunk_kv8_sinks_ref(p, tcw.UNREAD_WINDOW, sinks))


@pytest.mark.parametrize("window", tkw.dc.UNREAD_WINDOWS, ids=lambda w: f"w{w}")
@pytest.mark.parametrize("cfg", tkw.CONFIGS[1:4], ids=tkw.config_id)
def test_kv8_sinks_read_nothing_outside_the_window_single_token(sfa, cfg, window):
    """the single-token twin's unread-memory case (0x7F below lo and beyond pos, in the other layer and the spare pages,
    -1 in the table; num_splits 1, 3, 4) with zero sinks between NaNs: poisoned and benign runs give the same bits"""
    view = sinks_inside_nan(np.zeros(tkw.dc.HKV * cfg[0], np.float32))
    shim = WithSinks(sfa, view)
    G, D, layout, dtype, knobs = cfg
    clean = tkw.cached(("C", dtype, G, D, window), lambda: kwr.normal_problem(dtype, G, D, window))
    bad = clean.poisoned()
    m = clean.unread_mask()
    for S in (1, 3, 4):
        a = tkw.run_problem(shim, clean, layout, S, knobs=knobs)
        sfa.check_decode_status()
        z = tkw.run_problem(shim, bad, layout, S, table_beyond=-1, table_below=-1, knobs=knobs)
        sfa.check_decode_status()                               # clean, the -1 entries included
        assert np.isfinite(tkw.from_bits16(z["o"], dtype)).all()
        np.testing.assert_array_equal(z["o"], a["o"])
        for k in ("kc", "vc"):
            np.testing.assert_array_equal(z[k][~m], a[k][~m])
            np.testing.assert_array_equal(z[k][m], getattr(bad, k)[m])
        # a zero sink is material here (the scores are of order 1): the twin's output is elsewhere
        twin = tkw.run_problem(sfa, clean, layout, S, knobs=knobs)
        assert not np.array_equal(twin["o"], a["o"])
        np.testing.assert_array_equal(twin["kc"], a["kc"])


# ---- 8. rejection --------------------------------------------------------------------------------------------------------

def test_kv8_sinks_reject_like_the_twins(sfa):
    """seq_len out of range and a bad append page: NaN rows in o, an untouched cache and the twins' status bits -- the
    twins' own cases, run through the sinks calls (bf16, D 128, G 4, window 100)"""
    sinks, _ = ksr.single_ref("bf16", 128, 4, 100, False, 3)
    shim = WithSinks(sfa, on_device(sinks))
    tkw.test_kv8_window_rejects_like_kv8(shim)
    tcw.rejection_case(shim, False)
    tcw.rejection_case(shim, True)


@pytest.mark.parametrize("num_splits", [1, 3])
def test_kv8_sinks_bad_read_page_gives_nan(sfa, num_splits):
    """a bad entry on a page the window reads: the sequence's outputs are NaN -- the NaN survives the sink fold and
    v_scale -- and the status is raised; the same entry below the window is never looked at (fp16, D 128, G 8, window 100)"""
    sinks, _ = ksr.single_ref("fp16", 128, 8, 100, False, 3)
    shim = WithSinks(sfa, on_device(sinks))
    tkw.test_kv8_window_bad_table_entry_inside_and_below_the_window(shim, num_splits)
    tcw.bad_read_page_case(shim, num_splits, False)
    tcw.bad_read_page_case(shim, num_splits, True)


# ---- 9. graph replay -----------------------------------------------------------------------------------------------------

def test_varlen_kv8_window_sinks_graph_replay(sfa):
    """One captured flash_decode_varlen_kv8_window_sinks call, replayed with other sinks, cu_tokens, seq_len, scales and
    tensor contents under the same total_tokens bound: all are read on the device, so each replay matches its own
    reference."""
    dtype, D, G, window, T = "fp16", 128, 2, 33, 48
    dev = torch.device("cuda:0")
    probs = [ckw.make_problem(dtype, D, G, (3, 700, 64, 31), (3, 0, 40, 5), seed=1, tables=True),
             ckw.make_problem(dtype, D, G, (1300, 0, 97, 500), (1, 20, 0, 10), seed=2, k_factors=(0.5, 2.0), tables=True)]
    dt = TDT[dtype]
    t16 = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dt)
    cos, sin = (t16(x).to(dev) for x in ckw.rotary_tables(dtype, probs[0].rot))
    p0 = probs[0]
    qkv = torch.zeros(T, p0.H + 2 * HKV, D, dtype=dt, device=dev)
    kd = torch.zeros(p0.B, L, M, HKV, D, dtype=torch.uint8, device=dev)
    vd = torch.zeros_like(kd)
    o = torch.zeros(T, p0.H, D, dtype=dt, device=dev)
    sl = torch.zeros(p0.B, dtype=torch.int32, device=dev)
    cu = torch.zeros(p0.B + 1, dtype=torch.int32, device=dev)  # all sequences idle during warm-up and capture
    sk = torch.zeros(p0.H, dtype=torch.float32, device=dev)
    qb, kb, vb = (torch.zeros(x.shape, dtype=dt, device=dev) for x in p0.biases)
    ks, vs = torch.ones(HKV, device=dev), torch.ones(HKV, device=dev)
    call = lambda: sfa.flash_decode_varlen_kv8_window_sinks(qkv, qb, kb, vb, kd, vd, sl, o, cu, p0.B, M, p0.H, D, p0.rot, M, L,
                                                            LAYER, window, sk, num_splits=2, num_heads_kv=HKV, k_scale=ks,
                                                            v_scale=vs, rotary_cos_table=cos, rotary_sin_table=sin)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        call()                                              # warm-up: the stream's workspace exists before the capture
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            call()
        for i, p in enumerate(probs):
            anchor = (2, 1)[i]                              # a sequence with tokens
            sinks = ksr.anchor_sinks(p, window, anchor)
            cu_h = np.concatenate([[0], np.cumsum(p.ns)]).astype(np.int32)
            packed = np.zeros((T, p.H + 2 * HKV, D), np.float32)
            for b, n in enumerate(p.ns):
                packed[cu_h[b]:cu_h[b + 1]] = p.tok[b]
            for dst, src in ((qkv, t16(packed)), (kd, torch.from_numpy(p.k8)), (vd, torch.from_numpy(p.v8)),
                             (qb, t16(p.biases[0])), (kb, t16(p.biases[1])), (vb, t16(p.biases[2])),
                             (ks, torch.from_numpy(p.ks)), (vs, torch.from_numpy(p.vs)), (sk, torch.from_numpy(sinks))):
                dst.copy_(src.to(dev))
            o.fill_(7.0)
            sl.copy_(torch.tensor(list(p.lens), dtype=torch.int32))
            cu.copy_(torch.from_numpy(cu_h))
            graph.replay()
            side.synchronize()
            sfa.check_decode_status(dev)
            ob = bits(o.cpu())
            o_list = [ob[cu_h[b]:cu_h[b + 1]] for b in range(p.B)]
            r = SimpleNamespace(o=o_list, of=[as_float(x, dtype) for x in o_list], k8=kd.cpu().numpy(), v8=vd.cpu().numpy())
            ref = ksr.chunk_kv8_sinks_ref(p, window, sinks)
            ksr.check_chunk(r, p, window, sinks, ref)
            assert bool((ob[cu_h[-1]:].view(dt) == 7.0).all())              # rows past cu_tokens[B] are not written
            # the sink of this replay is material: the twin's reference is many tolerances away in the anchor's row
            gap = np.abs(r.of[anchor][0] - ckw.reference(p, window)[0]["o"][anchor][0]).max()
            assert gap > 10 * TOL[dtype], gap


def test_kv8_window_sinks_graph_replay_single_token(sfa):
    """One captured flash_decode_kv8_window_sinks call, replayed on the frame's seq_len and again with other seq_len and
    other sinks: what a fresh call on those contents gives, bit for bit, and the second matches its reference."""
    dtype, D, G, window, S = "bf16", 128, 4, 100, 3
    lens2 = (700, 0, 99, 313)
    sinks1, _ = ksr.single_ref(dtype, D, G, window, anchor=2)
    c, t = kwr.caches(D), kwr.tokens(dtype, D, G)
    bias = dict(q_bias=t.qb, k_bias=t.kb, v_bias=t.vb)
    k8, v8 = c.k8.copy(), c.v8.copy()
    base = ksr.decode_kv8_sinks_ref(t.qkv, k8, v8, lens2, LAYER, t.rot, dtype, window, None, c.ks, c.vs, **bias)
    sinks2 = ksr.make_sinks(base["lse"][0]).astype(np.float32)
    k8, v8 = c.k8.copy(), c.v8.copy()
    ref2 = dict(ksr.decode_kv8_sinks_ref(t.qkv, k8, v8, lens2, LAYER, t.rot, dtype, window, sinks2, c.ks, c.vs, **bias),
                k8=k8, v8=v8)
    fresh = [tkw.run(WithSinks(sfa, on_device(s)), dtype, D, G, "paged16", window, S, lens=ln)
             for s, ln in ((sinks1, LENS), (sinks2, lens2))]
    sfa.check_decode_status()
    dv = tkw.Device(dtype, D, G, "paged16")
    sk = torch.zeros(HKV * G, dtype=torch.float32, device=dv.dev)
    shim = WithSinks(sfa, sk)
    side = torch.cuda.Stream(dv.dev)
    side.wait_stream(torch.cuda.current_stream(dv.dev))
    with torch.cuda.stream(side):
        dv.call(shim, window, S)                # warm-up: the stream's workspace exists before the capture
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            dv.call(shim, window, S)
        for s, ln, want in zip((sinks1, sinks2), (LENS, lens2), fresh):
            dv.kd.copy_(tkw.to_layout(c.k8, "paged16").to(dv.dev))
            dv.vd.copy_(tkw.to_layout(c.v8, "paged16").to(dv.dev))
            dv.sl.copy_(torch.tensor(ln, dtype=torch.int32))
            sk.copy_(torch.from_numpy(s))
            dv.o.fill_(7.0)
            graph.replay()
            side.synchronize()
            sfa.check_decode_status(dv.dev)
            r = dv.result()
            np.testing.assert_array_equal(r.o, want.o)
            np.testing.assert_array_equal(r.kc, want.kc)
            np.testing.assert_array_equal(r.vc, want.vc)
    assert not np.array_equal(fresh[0].o, fresh[1].o)
    ksr.check_single_o(fresh[1], ref2, dtype, window, sinks2, c.ks, c.vs, lens=lens2)


# ---- 10. bad arguments through Python ------------------------------------------------------------------------------------

@pytest.mark.parametrize("call", CALLS)
def test_kv8_sinks_bad_arguments(sfa, call):
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
                tkw.run(s, dtype, D, G, "blmhd", window)
            else:
                ckw.run(s, ckw.problem(dtype, D, G, n), "blmhd", window, varlen=call == "varlen")
    for w in (0, -3):
        with pytest.raises(RuntimeError, match="window"):
            run_call(sfa, call, dtype, D, G, n, "blmhd", w, good)
    run_call(sfa, call, dtype, D, G, n, "blmhd", window, good)       # and the good one is accepted
    sfa.check_decode_status()


# ---- 11. a layer stack, the way a server uses the calls --------------------------------------------------------------------

def test_kv8_sinks_layer_stack(sfa):
    """Two layers of one fp8 paged-16 cache, H = 16, Hkv = 2, D = 64: layer 0 with a 128-row window, layer 1 with
    window = memory_max_len (full attention), each with sinks of its own.  A ragged prompt goes in through the varlen
    call, then four single-token steps follow with seq_len incremented here; before every call of layer 0 the block_table
    entries of its pages wholly below the window are -1 (a server has freed them).  Every call's appended bytes (the
    twins' check_bytes rules) and o (the fp64 sink attention over the bytes the device stored) are checked, the host
    caches fed forward from the device's."""
    dtype, D, G, ps, nb = "bf16", 64, 8, 16, 3
    H, tol = HKV * G, TOL[dtype]
    windows = (128, M)
    lens, ns = [0, 40, 200], (140, 17, 5)
    p = ckw.make_problem(dtype, D, G, lens, ns, seed=31, k_factors=(0.5, 2.0), tables=True)
    rng = np.random.default_rng(77)
    r16 = lambda *s: round_to(rng.standard_normal(s), dtype).astype(np.float32)
    cos, sin = ckw.rotary_tables(dtype, p.rot)
    bias = dict(q_bias=p.biases[0], k_bias=p.biases[1], v_bias=p.biases[2], cos_table=cos, sin_table=sin)
    # scores have a standard deviation near 2, so a row's log-sum-exp over 128 keys is near 7: material sinks around it
    sinks = (np.linspace(4.0, 10.0, H).astype(np.float32), np.linspace(9.0, 3.0, H).astype(np.float32))
    dev = torch.device("cuda:0")
    dt = TDT[dtype]
    t16 = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dt).to(dev)
    kd, vd = ckw.to_layout(p.k8, "paged16").to(dev), ckw.to_layout(p.v8, "paged16").to(dev)
    table = ckw.page_table(ps, nb)[0]
    kw = dict(num_heads_kv=HKV, kv_layout="paged", k_scale=torch.from_numpy(p.ks).to(dev), v_scale=torch.from_numpy(p.vs).to(dev),
              rotary_cos_table=t16(cos), rotary_sin_table=t16(sin))
    qb, kb, vb = (t16(x) for x in p.biases)
    sk = [on_device(s) for s in sinks]
    k_host, v_host = p.k8.copy(), p.v8.copy()
    layer_view = lambda x, l: x if l == LAYER else x[:, ::-1]   # check_bytes looks at layer index LAYER
    freed = 0
    for step in range(5):
        counts = ns if step == 0 else (1,) * nb
        for l in (0, 1):
            window = windows[l]
            tok = [r16(n, H + 2 * HKV, D) for n in counts]
            tl = table.copy()
            for b, pos in enumerate(lens):                      # the pages wholly below lo_0 are gone
                tl[b, :window_lo(pos, window) // ps] = -1
            freed += int((tl == -1).sum()) if l == 0 else 0
            assert l == 0 or not (tl == -1).any()
            sl = torch.tensor(lens, dtype=torch.int32, device=dev)
            args = (qb, kb, vb, kd, vd, sl)
            tail = (nb, M, H, D, p.rot, M, L, l, window, sk[l])
            kwl = dict(kw, block_table=torch.from_numpy(tl).to(dev), num_splits=(0, 1, 3)[step % 3])
            k_ref, v_ref = k_host.copy(), v_host.copy()
            ref = ckw.chunk_kv8_window_ref(tok, k_ref, v_ref, lens, l, p.rot, dtype, window, p.ks, p.vs, **bias)
            if step == 0:
                cu_h = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
                o = torch.full((int(cu_h[-1]), H, D), 7.0, dtype=dt, device=dev)
                sfa.flash_decode_varlen_kv8_window_sinks(t16(np.concatenate(tok)), *args, o, torch.from_numpy(cu_h).to(dev),
                                                         *tail, **kwl)
                got = [o.float().cpu().numpy()[cu_h[b]:cu_h[b + 1]] for b in range(nb)]
            else:
                o = torch.full((nb, H, D), 7.0, dtype=dt, device=dev)
                sfa.flash_decode_kv8_window_sinks(t16(np.stack([x[0] for x in tok])), *args, o, *tail, **kwl)
                got = [o.float().cpu().numpy()[b][None] for b in range(nb)]
            torch.cuda.synchronize()
            sfa.check_decode_status()
            k_out, v_out = ckw.from_layout(kd, "paged16", nb)[0], ckw.from_layout(vd, "paged16", nb)[0]
            ckr.check_bytes(lens, counts, *(layer_view(x, l) for x in (k_out, v_out, k_host, v_host, k_ref, v_ref)))
            for b in range(nb):
                want, _ = ksr.attend_sinks(ref["q16"][b], k_out[b, l], v_out[b, l], lens[b], window, sinks[l], p.ks, p.vs)
                assert np.isfinite(got[b]).all()
                np.testing.assert_allclose(got[b], want, atol=tol, rtol=tol, err_msg=f"step {step} layer {l} sequence {b}")
                if step == 1:                                   # the sinks are material: the twin's answer is elsewhere
                    plain = ckw.attend(ref["q16"][b], k_out[b, l], v_out[b, l], lens[b], window, p.ks, p.vs)
                    assert np.abs(plain - want).max() > 10 * tol
            k_host, v_host = k_out.copy(), v_out.copy()         # the next call reads the bytes the device stored
        lens = [pos + n for pos, n in zip(lens, counts)]
    assert lens == [144, 61, 209] and freed > 20
