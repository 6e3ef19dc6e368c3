"""GPU checks of sfa_decode_kv8_window (sliding-window decode over an fp8 e4m3 KV cache) through the Python operator and
the C ABI: parity with the fp64 reference of tests/kv8_window_ref.py over a pairwise-covering sweep, the window's own edge
cases, bit-identity with sfa_decode_kv8 where the window does not bind, successive steps, the edges of the window for
every alignment of lo, softmax_scale, the promise that nothing below the window is read, the workspace, rejection, graph
capture and the non-temporal loads.

Tolerances are the project's decode tolerances (window_ref.TOL: fp16 2e-3, bf16 1.6e-2, atol = rtol, elementwise, nothing
exempt): the reference sees the same dequantised bytes as the device, so the quantisation error is on both sides.  The
appended V bytes are exact; the appended K bytes follow the fp8 criterion (tests/test_decode_kv8_gpu.py): every element
within one e4m3 step and more than 98 % of the bytes identical -- and are sfa_decode_kv8's bit for bit.

The window suite's problem (kv8_window_ref): B = 4 sequences at seq_len = [0, 5, 130, 1000], 2 kv heads, 2 layers,
memory_max_len 1408, q / k / v bias, a partial rotary embedding (head_dim / 2), scales amax / 448 per kv head.  The
structured problems (window edges, softmax_scale, unread memory) are decode_cases' with e4m3 caches: M = 256, no rotation.
"""
import ctypes
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import decode_cases as dc
import kv8_ref
import kv8_window_ref as kw
from kv8_window_ref import B, HKV, L, LAYER, LENS, M, SPARE, SWEEP, TOL, window_lo
from oracle.numerics import from_bits16

pytestmark = pytest.mark.gpu

TDT = {"fp16": torch.float16, "bf16": torch.bfloat16}
GROUPS = [1, 2, 4, 8, 16]
NAN8 = dc.NAN8                                  # 0x7F: the e4m3 NaN byte


@pytest.fixture(scope="module")
def sfa():
    assert torch.cuda.is_available(), "GPU tests need a GPU (run with -m gpu on the MI355X box)"
    import starflashattention_amd as m
    m._lib.load()                  # fail loudly if the HIP library is missing
    m.check_decode_status()
    return m


# ---- layouts of the window suite's problem (canonical uint8 [B, L, M, Hkv, D], numpy) --------------------------------

def page_size(layout):
    return int(layout[5:]) if layout.startswith("paged") else None


def page_table(ps):
    """(the table that lays the pools out, the number of pages): shuffled, SPARE pages nobody owns"""
    pps = M // ps
    n = B * pps + SPARE
    return np.random.default_rng(3).permutation(n)[:B * pps].astype(np.int32).reshape(B, pps), n


def to_layout(c, layout, spare_fill=0):
    t = torch.from_numpy(np.ascontiguousarray(c))
    D = t.shape[-1]
    if layout == "blmhd":
        return t.clone()
    if layout == "blhmd":
        return t.permute(0, 1, 3, 2, 4).contiguous()
    ps = page_size(layout)
    table, n = page_table(ps)
    pps = M // ps
    pool = torch.full((n, L, ps, HKV, D), spare_fill, dtype=torch.uint8)
    pool[torch.from_numpy(table.reshape(-1)).long()] = (
        t.view(B, L, pps, ps, HKV, D).permute(0, 2, 1, 3, 4, 5).reshape(B * pps, L, ps, HKV, D))
    return pool


def from_layout(t, layout):
    """(canonical bytes [B, L, M, Hkv, D], the bytes of the spare pages or None), numpy"""
    t = t.cpu()
    D = t.shape[-1]
    if layout == "blmhd":
        return t.numpy(), None
    if layout == "blhmd":
        return t.permute(0, 1, 3, 2, 4).contiguous().numpy(), None
    ps = page_size(layout)
    table, n = page_table(ps)
    pps = M // ps
    own = torch.from_numpy(table.reshape(-1)).long()
    rest = torch.from_numpy(np.setdiff1d(np.arange(n), table.reshape(-1))).long()
    canon = t[own].view(B, pps, L, ps, HKV, D).permute(0, 2, 1, 3, 4, 5).reshape(B, L, M, HKV, D).contiguous()
    return canon.numpy(), t[rest].contiguous().numpy()


class Device:
    """The device side of one call on the window suite's problem: fresh copies of everything, kept for re-use (graph
    replay, successive steps)."""

    def __init__(self, dtype, D, G, layout, k8=None, v8=None, lens=LENS, table=None, spare_fill=0, tables=False,
                 qkv=None, k_factors=(1.0, 1.0)):
        self.dev = dev = torch.device("cuda:0")
        self.dtype, self.D, self.G, self.layout = dtype, D, G, layout
        self.t, c = kw.tokens(dtype, D, G), kw.caches(D, k_factors)
        t = self.t
        t16 = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(TDT[dtype]).to(dev)
        self.kd = to_layout(c.k8 if k8 is None else k8, layout, spare_fill).to(dev)
        self.vd = to_layout(c.v8 if v8 is None else v8, layout, spare_fill).to(dev)
        q = t16(t.qkv if qkv is None else qkv)
        self.qkv = q.view(B, 3, t.H, D) if G == 1 else q
        self.o = torch.full((B, t.H, D), 7.0, dtype=TDT[dtype], device=dev)
        self.sl = torch.tensor(list(lens), dtype=torch.int32, device=dev)
        ps = page_size(layout)
        self.kw = dict(kv_layout="paged" if ps else layout, num_heads_kv=HKV,
                       k_scale=torch.from_numpy(c.ks).to(dev), v_scale=torch.from_numpy(c.vs).to(dev))
        if ps:
            self.kw["block_table"] = torch.from_numpy(page_table(ps)[0] if table is None else table).to(dev)
        if tables:
            cos, sin = kw.rotary_tables(dtype, t.rot)
            self.kw.update(rotary_cos_table=t16(cos), rotary_sin_table=t16(sin))
        self.bias = (t16(t.qb), t16(t.kb), t16(t.vb))

    def args(self):
        t = self.t
        return (self.qkv, *self.bias, self.kd, self.vd, self.sl, self.o, B, M, t.H, self.D, t.rot, M, L, LAYER)

    def call(self, sfa, window, num_splits=0, softmax_scale=None):
        """flash_decode_kv8_window, or flash_decode_kv8 for window None"""
        kwargs = dict(self.kw, num_splits=num_splits, softmax_scale=softmax_scale)
        if window is None:
            ret = sfa.flash_decode_kv8(*self.args(), **kwargs)
        else:
            ret = sfa.flash_decode_kv8_window(*self.args(), window, **kwargs)
        assert ret.data_ptr() == self.o.data_ptr()
        return self

    def result(self):
        torch.cuda.synchronize()
        k_out, spare_k = from_layout(self.kd, self.layout)
        v_out, spare_v = from_layout(self.vd, self.layout)
        o = self.o.cpu()
        return SimpleNamespace(o=o.view(torch.int16).numpy().copy(), of=o.float().numpy(), kc=k_out, vc=v_out,
                               spare_k=spare_k, spare_v=spare_v)


def run(sfa, dtype, D, G, layout, window, num_splits=0, softmax_scale=None, **kwargs):
    """One call on fresh device copies; o as bits (.o) and as float32 (.of), the caches canonical (bytes)"""
    return Device(dtype, D, G, layout, **kwargs).call(sfa, window, num_splits, softmax_scale).result()


def append_mask(lens):
    """[B, L, M] True on every row a call must leave alone"""
    m = np.ones((B, L, M), bool)
    for b, pos in enumerate(lens):
        if 0 <= pos < M:
            m[b, LAYER, pos] = False
    return m


def check_appended_and_untouched(r, ref, D, like=None, lens=LENS, k_before=None, v_before=None):
    """The appended rows against the reference's (V exact; K within one e4m3 step and > 98 % identical: the device's
    sincosf can move a 16-bit value by one ulp, which rarely crosses an e4m3 rounding boundary) and, bit for bit, against
    the rows `like` of another run; every other byte of the caches as it was."""
    c = kw.caches(D)
    same = []
    for b, pos in enumerate(lens):
        np.testing.assert_array_equal(r.vc[b, LAYER, pos], ref["v_row"][b])
        got, want = kv8_ref.E4M3[r.kc[b, LAYER, pos]], kv8_ref.E4M3[ref["k_row"][b]]
        assert np.all(np.abs(got - want) <= kv8_ref.step_at(np.maximum(np.abs(got), np.abs(want)))), (b, got, want)
        same.append(r.kc[b, LAYER, pos] == ref["k_row"][b])
        if like is not None:
            np.testing.assert_array_equal(r.kc[b, LAYER, pos], like.k_rows[b])
            np.testing.assert_array_equal(r.vc[b, LAYER, pos], like.v_rows[b])
    assert np.mean(same) > 0.98
    m = append_mask(lens)
    np.testing.assert_array_equal(r.kc[m], (c.k8 if k_before is None else k_before)[m])
    np.testing.assert_array_equal(r.vc[m], (c.v8 if v_before is None else v_before)[m])


@functools.lru_cache(maxsize=None)
def _plain_kv8(dtype, D, G, tables):
    """the rows sfa_decode_kv8 appends on the same problem"""
    import starflashattention_amd as m
    r = run(m, dtype, D, G, "blmhd", None, tables=tables)
    rows = lambda c: [c[b, LAYER, pos].copy() for b, pos in enumerate(LENS)]
    return SimpleNamespace(k_rows=rows(r.kc), v_rows=rows(r.vc))


# ---- parity ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", list(enumerate(SWEEP)), ids=lambda c: "-".join(str(x) for x in c[1]))
def test_kv8_window_parity_sweep(sfa, case):
    i, (dtype, D, layout, G, num_splits, window) = case
    tables = bool(i & 1)                        # every other case reads the rotary tables instead of computing cos / sin
    ref = kw.reference(dtype, D, G, window, tables)
    r = run(sfa, dtype, D, G, layout, window, num_splits, tables=tables)
    sfa.check_decode_status()
    np.testing.assert_allclose(r.of, ref["o"], atol=TOL[dtype], rtol=TOL[dtype])
    # the appended bytes are sfa_decode_kv8's, bit for bit, at every window
    check_appended_and_untouched(r, ref, D, like=_plain_kv8(dtype, D, G, tables))
    if r.spare_k is not None:
        assert not r.spare_k.any() and not r.spare_v.any()


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_kv8_window_binds(sfa, dtype):
    """pos = 1000, window = 100: the windowed and the full reference differ by more than ten tolerances, so a kernel that
    ignores `window` cannot pass; the device matches the windowed one."""
    D, G, window = 128, 4, 100
    ref, full = kw.reference(dtype, D, G, window), kw.reference(dtype, D, G, None)
    b = LENS.index(1000)
    tol = TOL[dtype]
    gap = np.abs(ref["o"][b] - full["o"][b])
    assert gap.max() > 10 * tol * (1.0 + np.abs(full["o"][b]).max()), gap.max()
    r = run(sfa, dtype, D, G, "blmhd", window)
    sfa.check_decode_status()
    np.testing.assert_allclose(r.of, ref["o"], atol=tol, rtol=tol)
    assert np.abs(r.of[b] - full["o"][b]).max() > 5 * tol


@pytest.mark.parametrize("G", GROUPS)
def test_kv8_window_of_one_returns_the_new_v_row(sfa, G):
    """window = 1: the token sees itself only; o is the dequantised appended V row times v_scale, rounded to the dtype"""
    for dtype, D, layout in (("bf16", 128, "blmhd"), ("fp16", 64, "paged16")):
        r = run(sfa, dtype, D, G, layout, 1)
        sfa.check_decode_status()
        vs = kw.caches(D).vs
        for b, pos in enumerate(LENS):
            v = kv8_ref.E4M3[r.vc[b, LAYER, pos]].astype(np.float32) * vs[:, None]          # fp32, as the epilogue
            want = torch.from_numpy(np.repeat(v, G, axis=0)).to(TDT[dtype])                 # [H, D], rounded to nearest even
            np.testing.assert_array_equal(r.o[b], want.view(torch.int16).numpy(), err_msg=str((dtype, D, layout, b)))
        assert not np.array_equal(r.vc[:, LAYER, list(LENS)], kw.caches(D).v8[:, LAYER, list(LENS)])


# every G on the three load paths (contiguous row-major, head-major, paged), both dtypes, num_splits 1 and 3
IDENTITY_CASES = [(G, layout, dtype, num_splits) for G in GROUPS for layout in ("blmhd", "blhmd", "paged16")
                  for dtype in ("fp16", "bf16") for num_splits in (1, 3)]


@pytest.mark.parametrize("case", IDENTITY_CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_kv8_window_bit_identical_to_kv8_where_it_does_not_bind(sfa, case):
    """One body (decode_kv8_body.h), and with lo = 0 the same tile partition: o and the caches are sfa_decode_kv8's bit
    for bit at the same explicit num_splits.  head_dim alternates with the group."""
    G, layout, dtype, num_splits = case
    D = 128 if GROUPS.index(G) % 2 == 0 else 64
    full = run(sfa, dtype, D, G, layout, None, num_splits)
    for window in (max(LENS) + 1, 5000):
        r = run(sfa, dtype, D, G, layout, window, num_splits)
        sfa.check_decode_status()
        np.testing.assert_array_equal(r.o, full.o)
        np.testing.assert_array_equal(r.kc, full.kc)
        np.testing.assert_array_equal(r.vc, full.vc)


@pytest.mark.parametrize("layout", ["blmhd", "paged16"])
def test_kv8_window_successive_steps(sfa, layout):
    """Eight steps that cross pos = window, the cache fed forward on the device, against the reference fed forward on the
    host (its K row taken from the device after each step, as in tests/test_decode_kv8_gpu.py: the next step reads the
    bytes the device stored)."""
    dtype, D, G, window = "bf16", 128, 4, 36
    lens = [0, 30, 33, 1000]                    # pos + 1 = window is crossed by sequences 1 and 2; 0 stays inside, 3 outside
    c, t = kw.caches(D), kw.tokens(dtype, D, G)
    rng = np.random.default_rng(81)
    k_ref, v_ref = c.k8.copy(), c.v8.copy()
    dv = Device(dtype, D, G, layout)
    from oracle import round_to
    for step in range(8):
        qkv = round_to(rng.standard_normal(t.qkv.shape), dtype).astype(np.float32)
        ref = kw.decode_kv8_window_ref(qkv, k_ref, v_ref, lens, LAYER, t.rot, dtype, window, c.ks, c.vs, q_bias=t.qb,
                                       k_bias=t.kb, v_bias=t.vb)
        q = torch.from_numpy(qkv).to(TDT[dtype]).to(dv.dev)
        dv.qkv.copy_(q.view(dv.qkv.shape))
        dv.sl.copy_(torch.tensor(lens, dtype=torch.int32))
        k_before, v_before = from_layout(dv.kd, layout)[0], from_layout(dv.vd, layout)[0]
        r = dv.call(sfa, window, 1 + step % 3).result()
        np.testing.assert_allclose(r.of, ref["o"], atol=TOL[dtype], rtol=TOL[dtype], err_msg=f"step {step}")
        check_appended_and_untouched(r, ref, D, lens=lens, k_before=k_before, v_before=v_before)
        k_ref = r.kc.copy()
        np.testing.assert_array_equal(r.vc, v_ref)
        lens = [n + 1 for n in lens]
    assert lens[1] > window > lens[1] - 8 and lens[0] < window
    sfa.check_decode_status()


# ---- the structured problems of decode_cases over e4m3 caches ---------------------------------------------------------

class Kv8WindowRun(dc.Run):
    """decode_cases.Run for a kv8 problem with a window (kv8_window_ref.with_window)"""

    def call(self, sfa, num_splits=0, softmax_scale=None):
        p = self.p
        (kc, vc, sl, o), sizes = self.positional()
        ret = sfa.flash_decode_kv8_window(self.qkv, None, None, None, kc, vc, sl, o, *sizes, p.window,
                                          **self.keywords(num_splits, softmax_scale))
        assert ret.data_ptr() == o.data_ptr()
        return self


def run_problem(sfa, p, layout, num_splits=0, softmax_scale=None, table_beyond=None, table_below=None, knobs=None):
    knobs = knobs or {}
    for k, v in knobs.items():
        sfa.debug_set(k, v)
    try:
        return Kv8WindowRun(p, layout, table_beyond, table_below).call(sfa, num_splits, softmax_scale).result()
    finally:
        for k in knobs:
            sfa.debug_set(k, -1)


_cache = {}


def cached(key, make):
    """problems and their oracle results: computed once, shared by the tests that follow, never modified"""
    if key not in _cache:
        while len(_cache) >= 16:
            del _cache[next(iter(_cache))]
        _cache[key] = make()
    return _cache[key]


def assert_close(p, res, ref, what):
    o = from_bits16(res["o"], p.dtype)
    assert np.isfinite(o).all(), what
    np.testing.assert_allclose(o, ref["o"], atol=TOL[p.dtype], rtol=TOL[p.dtype], err_msg=str(what))


def assert_caches(p, res, ref, what):
    """rot = 0, no bias: the appended rows are the codes of the input bits, and no other byte of either cache, the spare
    pages of a pool included, has changed"""
    np.testing.assert_array_equal(res["kc"], ref["kc"], err_msg=f"{what}: k cache")
    np.testing.assert_array_equal(res["vc"], ref["vc"], err_msg=f"{what}: v cache")
    for s in (res["spare_k"], res["spare_v"]):
        assert s is None or np.all(s == p.spare_fill), f"{what}: a page no sequence owns was written"


# (G, head_dim, layout, dtype, knobs): every (dtype, head_dim, contiguous / paged) kernel, every group size, both
# contiguous layouts, non-temporal loads forced once per load path
CONFIGS = [(1, 128, "blmhd", "bf16", {}), (2, 64, "paged", "fp16", {}), (4, 128, "blhmd", "fp16", {"decode_nt": 1}),
           (8, 64, "blmhd", "bf16", {}), (16, 128, "paged", "bf16", {"decode_nt": 1}), (1, 64, "blhmd", "fp16", {}),
           (2, 128, "paged", "fp16", {}), (4, 64, "paged", "bf16", {})]
config_id = lambda c: f"G{c[0]}-D{c[1]}-{c[2]}-{c[3]}" + "".join(f"-{k}{v}" for k, v in c[4].items())


@pytest.mark.parametrize("window", dc.WINDOWS, ids=lambda w: f"w{w}")
@pytest.mark.parametrize("kind", kw.EDGE_KINDS)
@pytest.mark.parametrize("cfg", CONFIGS, ids=config_id)
def test_kv8_window_edges(sfa, cfg, kind, window):
    """One batch per (kind, window), a sequence per lo with pos = lo + window - 1 (kv8_window_ref.window_edges): a key that
    carries the weight on row lo or on row pos - 1; one just as large on row lo - 1, which nobody may see; a ramp that
    peaks at lo and goes on below it, and one that rises through the tiles of the window; all keys equal with rows lo - 1,
    lo and pos - 1 of V so large that one row dropped, added or counted twice is far outside the tolerance
    (tests/test_decode_kv8_window_cpu.py).  At num_splits 1, 3 and 4 (window 17: splits and waves without rows): o against
    the oracle, elementwise; the appended bytes and every other cache byte; a clean status."""
    G, D, layout, dtype, knobs = cfg
    def make():
        p = kw.window_edges(dtype, G, D, kind, window)
        return p, kw.oracle(p)
    p, ref = cached(("W", dtype, G, D, kind, window), make)
    for S in (1, 3, 4):
        what = (config_id(cfg), kind, f"window={window}", f"num_splits={S}")
        res = run_problem(sfa, p, layout, S, knobs=knobs)
        sfa.check_decode_status()
        assert_close(p, res, ref, what)
        assert_caches(p, res, ref, what)


@pytest.mark.parametrize("cfg", CONFIGS[:4], ids=config_id)
def test_kv8_window_softmax_scale(sfa, cfg):
    """N(0,1) data with k_scale = amax / 448 times [0.5, 2.0] per head at window 40 and softmax_scale 0.03 and 0.5,
    against the oracle with scale=; the call without the argument gives another result."""
    G, D, layout, dtype, knobs = cfg
    p = cached(("B", dtype, G, D), lambda: kw.normal_problem(dtype, G, D, dc.STRESS_WINDOW, amax_scales=True))
    assert p.ks[0] != p.ks[1] and not np.any(np.log2(p.ks) % 1 == 0)
    default = run_problem(sfa, p, layout, 1, knobs=knobs)
    for scale in (0.03, 0.5):
        ref = cached(("B", dtype, G, D, scale), lambda: kw.oracle(p, scale=scale))
        for S in (1, 3):
            what = (config_id(cfg), f"softmax_scale={scale}", f"num_splits={S}")
            res = run_problem(sfa, p, layout, S, softmax_scale=scale, knobs=knobs)
            sfa.check_decode_status()
            assert_close(p, res, ref, what)
            d = np.abs(from_bits16(res["o"], dtype) - from_bits16(default["o"], dtype))
            assert d.max() > 2 * TOL[dtype], f"{what}: the same as without softmax_scale"


@pytest.mark.parametrize("window", dc.UNREAD_WINDOWS, ids=lambda w: f"w{w}")
@pytest.mark.parametrize("cfg", CONFIGS[:5], ids=config_id)
def test_kv8_window_unread_memory_is_not_read(sfa, cfg, window):
    """The same call on a clean problem and on a poisoned one: the NaN byte 0x7F in every cache byte below lo and beyond
    pos, in the other layer and in the pages nobody owns; (paged) -1 in every block_table entry of a page wholly below lo
    and past the last page a sequence needs.  o and the appended bytes bit-identical, the status clean, every poisoned
    byte still in place.  Windows 40, 16 (at pos = 15, 31, 63 the window begins exactly on a page boundary) and 1 (no
    cached row is read; lo = pos, mostly on no tile boundary); num_splits 4 leaves splits without keys."""
    G, D, layout, dtype, knobs = cfg
    clean = cached(("C", dtype, G, D, window), lambda: kw.normal_problem(dtype, G, D, window))
    ref = cached(("C", dtype, G, D, window, "oracle"), lambda: kw.oracle(clean))
    bad = clean.poisoned()
    assert bad.spare_fill == NAN8 and clean.spare_fill == 0
    m = clean.unread_mask()
    assert all(m[b, dc.LAYER, :lo].all() for b, lo in enumerate(clean.lo)) and (window == 1 or max(clean.lo) > 0)
    for S in (1, 3, 4):
        what = (config_id(cfg), f"window={window}", f"num_splits={S}")
        a = run_problem(sfa, clean, layout, S, knobs=knobs)
        sfa.check_decode_status()
        z = run_problem(sfa, bad, layout, S, table_beyond=-1, table_below=-1, knobs=knobs)
        sfa.check_decode_status()                                           # clean, the -1 entries included
        assert np.isfinite(from_bits16(z["o"], dtype)).all(), what
        np.testing.assert_array_equal(z["o"], a["o"], err_msg=f"{what}: o depends on bytes outside the contract")
        for k in ("kc", "vc"):
            np.testing.assert_array_equal(z[k][~m], a[k][~m], err_msg=f"{what}: appended rows of {k}")
            np.testing.assert_array_equal(z[k][m], getattr(bad, k)[m], err_msg=f"{what}: a poisoned byte of {k} changed")
        assert_caches(clean, a, ref, what)
        for s in (z["spare_k"], z["spare_v"]):
            assert s is None or np.all(s == NAN8), f"{what}: a page no sequence owns was written"
        assert_close(clean, a, ref, what)


# ---- workspace -------------------------------------------------------------------------------------------------------

def test_kv8_window_exact_workspace_with_empty_splits(sfa):
    """sfa_decode_kv8_window itself at num_splits = 4 with a workspace of exactly sfa_decode_window_workspace_bytes bytes,
    every fp32 of it a NaN beforehand, and a window so short (17 rows: at most two 32-row tiles) that splits are empty:
    bit-identical to the operator, nothing written past the end."""
    from exact_workspace import call_with_exact_workspace
    from starflashattention_amd import _lib, ops
    dtype, D, G, window, S = "bf16", 128, 4, 17, 4
    want = run(sfa, dtype, D, G, "blmhd", window, S)
    sfa.check_decode_status()
    dv = Device(dtype, D, G, "blmhd")
    t = dv.t
    a, *_ = ops._decode_args(dv.qkv, *dv.bias, dv.kd, dv.vd, dv.sl, dv.o, B, M, t.H, D, t.rot, M, L, LAYER, None, None, None,
                             "blmhd", None, HKV, kv8=True)
    lib = _lib.load()
    a.stride = (t.H + 2 * HKV) * D
    nbytes = lib.sfa_decode_window_workspace_bytes(B, t.H, HKV, D, M, window, S)
    assert nbytes == lib.sfa_decode_workspace_bytes(B, t.H, D, M, S) <= lib.sfa_decode_workspace_bytes_gqa(B, t.H, HKV, D, M, S)
    vp = lambda x: ctypes.c_void_p(x.data_ptr())
    ks, vs = dv.kw["k_scale"], dv.kw["v_scale"]
    call_with_exact_workspace(a, nbytes, S, lambda args, stream: lib.sfa_decode_kv8_window(args, vp(ks), vp(vs), window, stream),
                              dv.dev, fill=0xFF)
    r = dv.result()
    np.testing.assert_array_equal(r.o, want.o)
    np.testing.assert_array_equal(r.kc, want.kc)
    np.testing.assert_array_equal(r.vc, want.vc)
    assert np.isfinite(r.of).all()


# ---- rejection -------------------------------------------------------------------------------------------------------

def test_kv8_window_rejects_like_kv8(sfa):
    """seq_len out of range and a bad append page: NaN, the sequence's cache untouched, sfa_decode's status"""
    dtype, D, G, window = "bf16", 128, 4, 100
    c = kw.caches(D)
    good = run(sfa, dtype, D, G, "blmhd", window)
    sfa.check_decode_status()
    lens = (0, M, 130, -1)
    r = run(sfa, dtype, D, G, "blmhd", window, lens=lens)
    with pytest.raises(sfa.SfaError, match="seq_len") as e:
        sfa.check_decode_status()
    assert e.value.status == sfa._lib.SFA_ERR_SEQ_LEN_RANGE
    assert np.isnan(r.of[1]).all() and np.isnan(r.of[3]).all()
    m = append_mask(lens)
    np.testing.assert_array_equal(r.kc[m], c.k8[m])
    np.testing.assert_array_equal(r.vc[m], c.v8[m])
    np.testing.assert_array_equal(r.o[[0, 2]], good.o[[0, 2]])
    np.testing.assert_array_equal(r.kc[~m], good.kc[~m])
    # the append page of sequence 2 (pos 130) outside the pool
    ps = 16
    table = page_table(ps)[0].copy()
    table[2, 130 // ps] = -7
    goodp = run(sfa, dtype, D, G, "paged16", window)
    sfa.check_decode_status()
    r = run(sfa, dtype, D, G, "paged16", window, table=table)
    with pytest.raises(sfa.SfaError, match="block_table") as e:
        sfa.check_decode_status()
    assert e.value.status == sfa._lib.SFA_ERR_BLOCK_TABLE_RANGE
    assert np.isnan(r.of[2]).all()
    m = append_mask((0, 5, -1, 1000))           # nothing of sequence 2 was written, anywhere in the pools
    np.testing.assert_array_equal(r.kc[m], c.k8[m])
    np.testing.assert_array_equal(r.vc[m], c.v8[m])
    assert not r.spare_k.any() and not r.spare_v.any()
    np.testing.assert_array_equal(r.o[[0, 1, 3]], goodp.o[[0, 1, 3]])
    sfa.check_decode_status()


@pytest.mark.parametrize("num_splits", [1, 3])
def test_kv8_window_bad_table_entry_inside_and_below_the_window(sfa, num_splits):
    dtype, D, G, window, ps = "fp16", 128, 8, 100, 16
    b, lo = LENS.index(1000), window_lo(1000, window)
    _, n = page_table(ps)
    clean = run(sfa, dtype, D, G, "paged16", window, num_splits)
    sfa.check_decode_status()
    inside = page_table(ps)[0].copy()
    inside[b, lo // ps + 1] = n                 # a page the window reads
    r = run(sfa, dtype, D, G, "paged16", window, num_splits, table=inside)
    with pytest.raises(sfa.SfaError, match="block_table"):
        sfa.check_decode_status()
    assert np.isnan(r.of[b]).all()
    np.testing.assert_array_equal(r.o[:b], clean.o[:b])
    np.testing.assert_array_equal(r.kc, clean.kc)                               # reads only: the same appends
    np.testing.assert_array_equal(r.vc, clean.vc)
    below = page_table(ps)[0].copy()
    below[b, lo // ps - 1] = n                  # the same bad value on the last page wholly below lo: never looked at
    below[b, 0] = -1
    r = run(sfa, dtype, D, G, "paged16", window, num_splits, table=below)
    sfa.check_decode_status()
    np.testing.assert_array_equal(r.o, clean.o)
    np.testing.assert_array_equal(r.kc, clean.kc)
    np.testing.assert_array_equal(r.vc, clean.vc)


def test_kv8_window_must_be_positive(sfa):
    for w in (0, -3):
        with pytest.raises(sfa.SfaError, match="window") as e:
            run(sfa, "fp16", 64, 2, "blmhd", w)
        assert e.value.status == -2


# ---- graph capture ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", ["blmhd", "paged16"])
def test_kv8_window_graph_capture_and_replay(sfa, layout):
    """lo is computed on the device from seq_len: one captured call, replayed on the suite's seq_len and again after
    seq_len changed, gives what a fresh call on those contents gives."""
    dtype, D, G, window, S = "bf16", 128, 4, 100, 3
    lens2 = (700, 0, 99, 313)
    fresh = [run(sfa, dtype, D, G, layout, window, S, lens=ln) for ln in (LENS, lens2)]
    sfa.check_decode_status()
    dv = Device(dtype, D, G, layout)
    side = torch.cuda.Stream(dv.dev)
    side.wait_stream(torch.cuda.current_stream(dv.dev))
    with torch.cuda.stream(side):
        dv.call(sfa, window, S)                 # warm-up: the stream's workspace exists before the capture
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            dv.call(sfa, window, S)
        for ln, want in zip((LENS, lens2), fresh):
            dv.kd.copy_(to_layout(kw.caches(D).k8, layout).to(dv.dev))
            dv.vd.copy_(to_layout(kw.caches(D).v8, layout).to(dv.dev))
            dv.sl.copy_(torch.tensor(ln, dtype=torch.int32))
            dv.o.fill_(7.0)
            graph.replay()
            side.synchronize()
            sfa.check_decode_status(dv.dev)
            r = dv.result()
            np.testing.assert_array_equal(r.o, want.o)
            np.testing.assert_array_equal(r.kc, want.kc)
            np.testing.assert_array_equal(r.vc, want.vc)
    ref = kw.reference(dtype, D, G, window, lens=lens2)
    np.testing.assert_allclose(fresh[1].of, ref["o"], atol=TOL[dtype], rtol=TOL[dtype])


# ---- non-temporal loads ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", ["blmhd", "blhmd", "paged16"])
def test_kv8_window_non_temporal_loads(sfa, layout):
    """decode_nt forced on and off, once per load path: the same bits, and the reference's values"""
    dtype, D, G, window = "fp16", 128, 2, 100
    out = []
    for nt in (0, 1):
        sfa.debug_set("decode_nt", nt)
        try:
            out.append(run(sfa, dtype, D, G, layout, window, 2))
        finally:
            sfa.debug_set("decode_nt", -1)
    sfa.check_decode_status()
    np.testing.assert_array_equal(out[0].o, out[1].o)
    np.testing.assert_array_equal(out[0].kc, out[1].kc)
    np.testing.assert_allclose(out[1].of, kw.reference(dtype, D, G, window)["o"], atol=TOL[dtype], rtol=TOL[dtype])
