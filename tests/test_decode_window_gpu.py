"""GPU checks of sfa_decode_window (sliding-window decode) through the Python operator and the C ABI: parity with the
fp64 reference of tests/window_ref.py over a pairwise-covering sweep, the window's own edge cases, bit-identity with
sfa_decode where the window does not bind, the promise that nothing below the window is read, rejection, and the
workspace.

Tolerances are the project's decode tolerances (kernel vs fp64 reference on identically rounded inputs): fp16 2e-3,
bf16 1.6e-2, atol = rtol.  Every problem has B = 4 sequences at seq_len = [0, 5, 130, 1000] (lo = 0, inside the first
tile, on and beside multiples of 16 and 32, different per sequence), 2 kv heads, 2 layers, memory_max_len 1408, q / k / v
bias and a partial rotary embedding (head_dim / 2).
"""
import ctypes
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import rotary_table_ref
from window_ref import SWEEP, TOL, decode_window_ref, window_lo

pytestmark = pytest.mark.gpu

ULP = {"fp16": 2.0 ** -10, "bf16": 2.0 ** -7}
TDT = {"fp16": torch.float16, "bf16": torch.bfloat16}
B, HKV, L, M, LAYER, SPARE = 4, 2, 2, 1408, 1, 3
LENS = (0, 5, 130, 1000)
NAN16 = 0x7FFF                                  # NaN in fp16 and in bf16
GROUPS = [1, 2, 4, 8, 16]


@pytest.fixture(scope="module")
def sfa():
    assert torch.cuda.is_available(), "GPU tests need a GPU (run with -m gpu on the MI355X box)"
    import starflashattention_amd as m
    m._lib.load()                  # fail loudly if the HIP library is missing
    return m


# ---- problems (CPU, canonical layout [B, L, M, Hkv, D]) and their references: made once, never modified -------------

def _randn(rng, dtype, *shape):
    return torch.from_numpy(rng.standard_normal(shape, dtype=np.float32)).to(TDT[dtype])


@functools.lru_cache(maxsize=None)
def caches(dtype, D):
    rng = np.random.default_rng([1, D, dtype == "bf16"])
    kc, vc = _randn(rng, dtype, B, L, M, HKV, D), _randn(rng, dtype, B, L, M, HKV, D)
    return SimpleNamespace(kc=kc, vc=vc, kf=kc.float().numpy(), vf=vc.float().numpy())


@functools.lru_cache(maxsize=None)
def tokens(dtype, D, G):
    rng = np.random.default_rng([2, D, G, dtype == "bf16"])
    H = HKV * G
    t = SimpleNamespace(H=H, rot=D // 2, qkv=_randn(rng, dtype, B, H + 2 * HKV, D), qb=_randn(rng, dtype, H, D),
                        kb=_randn(rng, dtype, HKV, D), vb=_randn(rng, dtype, HKV, D))
    return t


@functools.lru_cache(maxsize=None)
def rotary_tables(dtype, rot):
    return rotary_table_ref(M, rot, dtype)


@functools.lru_cache(maxsize=None)
def reference(dtype, D, G, window, tables=False):
    """window_ref on the inputs the device gets; window None = sfa_decode"""
    t, c = tokens(dtype, D, G), caches(dtype, D)
    f = lambda x: x.float().numpy()
    qkv = f(t.qkv)
    cos, sin = rotary_tables(dtype, t.rot) if tables else (None, None)
    return decode_window_ref(qkv[:, :t.H], qkv[:, t.H:t.H + HKV], qkv[:, t.H + HKV:], c.kf, c.vf, LENS, LAYER, t.rot,
                             window, dtype, q_bias=f(t.qb), k_bias=f(t.kb), v_bias=f(t.vb), cos_table=cos, sin_table=sin)


def bits(t):
    return t.contiguous().view(torch.int16)


def poisoned(c, lens, window):
    """a copy of the canonical cache c with NaN in every row the windowed call must not read: the other layer, the
    rows below lo and the rows above pos"""
    p = c.clone()
    pb = p.view(torch.int16)
    pb[:, 1 - LAYER] = NAN16
    for b, pos in enumerate(lens):
        pb[b, LAYER, :window_lo(pos, window)] = NAN16
        pb[b, LAYER, pos + 1:] = NAN16
    return p


# ---- layouts ---------------------------------------------------------------------------------------------------------

def page_size(layout):
    return int(layout[5:]) if layout.startswith("paged") else None


def page_table(ps):
    """(the table that lays the pools out, the number of pages): shuffled, SPARE pages nobody owns"""
    pps = M // ps
    n = B * pps + SPARE
    return np.random.default_rng(3).permutation(n)[:B * pps].astype(np.int32).reshape(B, pps), n


def to_layout(c, layout, spare_bits=0):
    D = c.shape[-1]
    if layout == "blmhd":
        return c.clone()
    if layout == "blhmd":
        return c.permute(0, 1, 3, 2, 4).contiguous()
    ps = page_size(layout)
    table, n = page_table(ps)
    pps = M // ps
    pool = torch.full((n, L, ps, HKV, D), spare_bits, dtype=torch.int16).view(c.dtype)
    pool[torch.from_numpy(table.reshape(-1)).long()] = (
        c.view(B, L, pps, ps, HKV, D).permute(0, 2, 1, 3, 4, 5).reshape(B * pps, L, ps, HKV, D))
    return pool


def from_layout(t, layout):
    """(canonical bits [B, L, M, Hkv, D], the bits of the spare pages or None)"""
    t = bits(t.cpu())
    D = t.shape[-1]
    if layout == "blmhd":
        return t, None
    if layout == "blhmd":
        return t.permute(0, 1, 3, 2, 4).contiguous(), None
    ps = page_size(layout)
    table, n = page_table(ps)
    pps = M // ps
    own = torch.from_numpy(table.reshape(-1)).long()
    rest = torch.from_numpy(np.setdiff1d(np.arange(n), table.reshape(-1))).long()
    canon = t[own].view(B, pps, L, ps, HKV, D).permute(0, 2, 1, 3, 4, 5).reshape(B, L, M, HKV, D).contiguous()
    return canon, t[rest].contiguous()


def run(sfa, dtype, D, G, layout, window, num_splits=0, kc=None, vc=None, lens=LENS, table=None, spare_bits=0,
        tables=False):
    """One call on fresh device copies: flash_decode_window, or flash_decode for window None.  kc / vc: canonical caches
    instead of the problem's own; table: the block_table the call gets instead of the one the pools are laid out by.
    Returns o, kc, vc (canonical) as bits and the spare pages' bits."""
    dev = torch.device("cuda:0")
    t, c = tokens(dtype, D, G), caches(dtype, D)
    kd = to_layout(c.kc if kc is None else kc, layout, spare_bits).to(dev)
    vd = to_layout(c.vc if vc is None else vc, layout, spare_bits).to(dev)
    qkv = (t.qkv.view(B, 3, t.H, D) if G == 1 else t.qkv).to(dev)
    o = torch.full((B, t.H, D), 7.0, dtype=TDT[dtype], device=dev)
    sl = torch.tensor(list(lens), dtype=torch.int32, device=dev)
    ps = page_size(layout)
    kw = dict(num_splits=num_splits, kv_layout="paged" if ps else layout, num_heads_kv=HKV)
    if ps:
        kw["block_table"] = torch.from_numpy(page_table(ps)[0] if table is None else table).to(dev)
    if tables:
        cos, sin = rotary_tables(dtype, t.rot)
        td = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(TDT[dtype]).to(dev)
        kw.update(rotary_cos_table=td(cos), rotary_sin_table=td(sin))
    args = (qkv, t.qb.to(dev), t.kb.to(dev), t.vb.to(dev), kd, vd, sl, o, B, M, t.H, D, t.rot, M, L, LAYER)
    ret = sfa.flash_decode(*args, **kw) if window is None else sfa.flash_decode_window(*args, window, **kw)
    assert ret.data_ptr() == o.data_ptr()
    torch.cuda.synchronize()
    k_out, spare_k = from_layout(kd, layout)
    v_out, spare_v = from_layout(vd, layout)
    return SimpleNamespace(o=bits(o.cpu()), kc=k_out, vc=v_out, spare_k=spare_k, spare_v=spare_v)


def as_float(o_bits, dtype):
    return o_bits.view(TDT[dtype]).float().numpy()


def append_mask(lens):
    """[B, L, M] True on every row a call must leave alone"""
    m = torch.ones((B, L, M), dtype=torch.bool)
    for b, pos in enumerate(lens):
        if 0 <= pos < M:
            m[b, LAYER, pos] = False
    return m


def check_appended_and_untouched(r, src_k, src_v, ref, dtype, like=None):
    """The appended K / V rows against the reference (V exact, K to one storage ulp: the device's sincosf / powf and
    numpy's differ in the last fp32 bit of the angle) and, bit for bit, against the rows `like` of another run; every
    other row of the caches as it was."""
    for b, pos in enumerate(LENS):
        krow, vrow = as_float(r.kc[b, LAYER, pos], dtype), as_float(r.vc[b, LAYER, pos], dtype)
        np.testing.assert_array_equal(vrow, ref["v_row"][b])
        err = np.abs(krow - ref["k_row"][b])
        assert np.all(err <= ULP[dtype] * np.maximum(1.0, np.abs(krow)) * 1.01), err.max()
        if like is not None:
            assert torch.equal(r.kc[b, LAYER, pos], like.k_rows[b])
            assert torch.equal(r.vc[b, LAYER, pos], like.v_rows[b])
    m = append_mask(LENS)
    assert torch.equal(r.kc[m], bits(src_k)[m]) and torch.equal(r.vc[m], bits(src_v)[m])


@functools.lru_cache(maxsize=None)
def _full_decode(dtype, D, G, tables):
    """the rows sfa_decode appends on the same problem"""
    import starflashattention_amd as m
    r = run(m, dtype, D, G, "blmhd", None, tables=tables)
    rows = lambda c: [c[b, LAYER, pos].clone() for b, pos in enumerate(LENS)]
    return SimpleNamespace(k_rows=rows(r.kc), v_rows=rows(r.vc))


# ---- parity ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", list(enumerate(SWEEP)), ids=lambda c: "-".join(str(x) for x in c[1]))
def test_window_parity_sweep(sfa, case):
    i, (dtype, D, layout, G, num_splits, window) = case
    tables = bool(i & 1)                        # every other case reads the rotary tables instead of computing cos / sin
    ref = reference(dtype, D, G, window, tables)
    r = run(sfa, dtype, D, G, layout, window, num_splits, tables=tables)
    sfa.check_decode_status()
    np.testing.assert_allclose(as_float(r.o, dtype), ref["o"], atol=TOL[dtype], rtol=TOL[dtype])
    c = caches(dtype, D)
    # the appended rows are sfa_decode's, bit for bit
    check_appended_and_untouched(r, c.kc, c.vc, ref, dtype, like=_full_decode(dtype, D, G, tables))
    if r.spare_k is not None:
        assert not bool(r.spare_k.any()) and not bool(r.spare_v.any())


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_window_binds(sfa, dtype):
    """pos = 1000, window = 100: the windowed and the full result differ by far more than the tolerance, so a kernel that
    ignores `window` cannot pass."""
    D, G, window = 128, 4, 100
    ref, full = reference(dtype, D, G, window), reference(dtype, D, G, None)
    b = LENS.index(1000)
    tol = TOL[dtype]
    gap = np.abs(ref["o"][b] - full["o"][b])
    assert gap.max() > 10 * tol * (1.0 + np.abs(full["o"][b]).max()), gap.max()
    r = run(sfa, dtype, D, G, "blmhd", window)
    sfa.check_decode_status()
    np.testing.assert_allclose(as_float(r.o, dtype), ref["o"], atol=tol, rtol=tol)
    assert np.abs(as_float(r.o, dtype)[b] - full["o"][b]).max() > 5 * tol


@pytest.mark.parametrize("G", GROUPS)
def test_window_of_one_returns_the_new_v_row(sfa, G):
    """window = 1: the token sees itself only, o is the bits of the V row the call appends"""
    for dtype, D, layout in (("bf16", 128, "blmhd"), ("fp16", 64, "paged16")):
        r = run(sfa, dtype, D, G, layout, 1)
        sfa.check_decode_status()
        for b, pos in enumerate(LENS):
            want = r.vc[b, LAYER, pos].repeat_interleave(G, dim=0)          # [H, D]: query head h reads kv head h // G
            assert torch.equal(r.o[b], want), (dtype, D, layout, b)
        assert not torch.equal(r.vc[:, LAYER, list(LENS)], bits(caches(dtype, D).vc)[:, LAYER, list(LENS)])


@pytest.mark.parametrize("G", GROUPS)
def test_window_beyond_every_position_is_plain_decode(sfa, G):
    for dtype, D, layout in (("fp16", 128, "blmhd"), ("bf16", 256, "blhmd"), ("bf16", 64, "paged64")):
        full = run(sfa, dtype, D, G, layout, None)
        r = run(sfa, dtype, D, G, layout, max(LENS) + 1)
        sfa.check_decode_status()
        tol = TOL[dtype]
        np.testing.assert_allclose(as_float(r.o, dtype), as_float(full.o, dtype), atol=tol, rtol=tol)
        assert torch.equal(r.kc, full.kc) and torch.equal(r.vc, full.vc)


# the (head_dim, G) pairs sfa_decode sends to decode_gqa_mfma_kernel without a knob (decode_dispatch.hip), on each of its
# load paths: blmhd row-major through the K tile, blhmd in operand layout, paged
MFMA_PAIRS = [(128, 8), (128, 4), (128, 16), (64, 8), (256, 8)]
IDENTITY_CASES = [(D, G, num_splits, layout, dtype) for D, G in MFMA_PAIRS for dtype in ("fp16", "bf16")
                  for layout in ("blmhd", "blhmd", "paged16") for num_splits in (1, 3)]


def _identity_id(case):
    D, G, *rest = case
    return "-".join(str(x) for x in rest) + ("" if (D, G) == MFMA_PAIRS[0] else f"-D{D}-G{G}")


@pytest.mark.parametrize("case", IDENTITY_CASES, ids=_identity_id)
def test_window_bit_identical_to_decode_where_it_does_not_bind(sfa, case):
    """These groups are served by decode_gqa_mfma_kernel in sfa_decode: the same body (decode_mfma16.h), and with lo = 0
    the same tile partition"""
    D, G, num_splits, layout, dtype = case
    full = run(sfa, dtype, D, G, layout, None, num_splits)
    r = run(sfa, dtype, D, G, layout, 5000, num_splits)
    sfa.check_decode_status()
    assert torch.equal(r.o, full.o)
    assert torch.equal(r.kc, full.kc) and torch.equal(r.vc, full.vc)


# ---- what the window promises not to read ----------------------------------------------------------------------------

@pytest.mark.parametrize("window", [17, 100])
@pytest.mark.parametrize("ps", [16, 64])
@pytest.mark.parametrize("num_splits", [1, 3])
def test_window_reads_nothing_below_it(sfa, window, ps, num_splits):
    """The same call on a clean problem and on one with NaN in every cache row below lo and above pos, in the other
    layer and in the spare pages, and -1 in every block_table entry of a page wholly below lo: the same bits, a clean
    status, the poison still in place."""
    dtype, D, G, layout = "bf16", 128, 4, f"paged{ps}"
    c = caches(dtype, D)
    clean = run(sfa, dtype, D, G, layout, window, num_splits)
    sfa.check_decode_status()
    pk, pv = poisoned(c.kc, LENS, window), poisoned(c.vc, LENS, window)
    table = page_table(ps)[0].copy()
    for b, pos in enumerate(LENS):
        table[b, :window_lo(pos, window) // ps] = -1
    assert (table[LENS.index(1000)] == -1).sum() == (1001 - window) // ps > 0
    r = run(sfa, dtype, D, G, layout, window, num_splits, kc=pk, vc=pv, table=table, spare_bits=NAN16)
    sfa.check_decode_status()
    assert not bool(torch.isnan(r.o.view(TDT[dtype])).any())
    assert torch.equal(r.o, clean.o)
    m = append_mask(LENS)
    assert torch.equal(r.kc[~m], clean.kc[~m]) and torch.equal(r.vc[~m], clean.vc[~m])       # the appended rows
    assert torch.equal(r.kc[m], bits(pk)[m]) and torch.equal(r.vc[m], bits(pv)[m])           # the poison, and the rest
    assert bool((r.spare_k == NAN16).all()) and bool((r.spare_v == NAN16).all())
    # the contiguous layouts keep the same promise
    for lay in ("blmhd", "blhmd"):
        c2 = run(sfa, dtype, D, G, lay, window, num_splits)
        r2 = run(sfa, dtype, D, G, lay, window, num_splits, kc=pk, vc=pv)
        sfa.check_decode_status()
        assert torch.equal(r2.o, c2.o)
        assert torch.equal(r2.kc[~m], c2.kc[~m]) and torch.equal(r2.kc[m], bits(pk)[m])
        assert torch.equal(r2.vc[~m], c2.vc[~m]) and torch.equal(r2.vc[m], bits(pv)[m])


# ---- rejection -------------------------------------------------------------------------------------------------------

def test_window_rejects_like_decode(sfa):
    """seq_len out of range and a bad append page: NaN, the sequence's cache untouched, sfa_decode's status"""
    dtype, D, G, window = "bf16", 128, 4, 100
    c = caches(dtype, D)
    good = run(sfa, dtype, D, G, "blmhd", window)
    sfa.check_decode_status()
    lens = (0, M, 130, -1)
    for w in (window, None):
        r = run(sfa, dtype, D, G, "blmhd", w, lens=lens)
        with pytest.raises(RuntimeError, match="seq_len"):
            sfa.check_decode_status()
        o = r.o.view(TDT[dtype])
        assert bool(torch.isnan(o[1]).all()) and bool(torch.isnan(o[3]).all())
        m = append_mask(lens)
        assert torch.equal(r.kc[m], bits(c.kc)[m]) and torch.equal(r.vc[m], bits(c.vc)[m])
        if w is not None:
            assert torch.equal(r.o[0], good.o[0]) and torch.equal(r.o[2], good.o[2])
            assert torch.equal(r.kc[~m], good.kc[~m])
    # the append page of sequence 2 (pos 130) outside the pool
    ps = 16
    table = page_table(ps)[0].copy()
    table[2, 130 // ps] = -7
    goodp = run(sfa, dtype, D, G, "paged16", window)
    sfa.check_decode_status()
    for w in (window, None):
        r = run(sfa, dtype, D, G, "paged16", w, table=table)
        with pytest.raises(RuntimeError, match="block_table"):
            sfa.check_decode_status()
        assert bool(torch.isnan(r.o.view(TDT[dtype])[2]).all())
        m = append_mask((0, 5, -1, 1000))       # nothing of sequence 2 was written, anywhere in the pools
        assert torch.equal(r.kc[m], bits(c.kc)[m]) and torch.equal(r.vc[m], bits(c.vc)[m])
        assert not bool(r.spare_k.any()) and not bool(r.spare_v.any())
        if w is not None:
            for b in (0, 1, 3):
                assert torch.equal(r.o[b], goodp.o[b])


@pytest.mark.parametrize("num_splits", [1, 3])
def test_window_bad_table_entry_inside_and_below_the_window(sfa, num_splits):
    dtype, D, G, window, ps = "fp16", 128, 8, 100, 16
    b, lo = LENS.index(1000), window_lo(1000, window)
    _, n = page_table(ps)
    clean = run(sfa, dtype, D, G, "paged16", window, num_splits)
    sfa.check_decode_status()
    inside = page_table(ps)[0].copy()
    inside[b, lo // ps + 1] = n                 # a page the window reads
    r = run(sfa, dtype, D, G, "paged16", window, num_splits, table=inside)
    with pytest.raises(RuntimeError, match="block_table"):
        sfa.check_decode_status()
    assert bool(torch.isnan(r.o.view(TDT[dtype])[b]).all())
    assert torch.equal(r.o[:b], clean.o[:b])
    assert torch.equal(r.kc, clean.kc) and torch.equal(r.vc, clean.vc)          # reads only: the same appends
    below = page_table(ps)[0].copy()
    below[b, lo // ps - 1] = n                  # the same entry on the last page wholly below lo: never looked at
    below[b, 0] = -1
    r = run(sfa, dtype, D, G, "paged16", window, num_splits, table=below)
    sfa.check_decode_status()
    assert torch.equal(r.o, clean.o) and torch.equal(r.kc, clean.kc) and torch.equal(r.vc, clean.vc)


def test_window_must_be_positive(sfa):
    for w in (0, -3):
        with pytest.raises(RuntimeError, match="window"):
            run(sfa, "fp16", 64, 2, "blmhd", w)


# ---- workspace -------------------------------------------------------------------------------------------------------

def test_window_exact_workspace_with_empty_splits(sfa):
    """sfa_decode_window itself at num_splits = 4 with a workspace of exactly sfa_decode_window_workspace_bytes bytes,
    every fp32 of it a NaN beforehand, and a window so short (17 rows: at most two 32-row tiles) that splits are empty:
    bit-identical to the operator, nothing written past the end."""
    from exact_workspace import call_with_exact_workspace
    from starflashattention_amd import _lib, ops
    dtype, D, G, window, S = "bf16", 128, 4, 17, 4
    dev = torch.device("cuda:0")
    t, c = tokens(dtype, D, G), caches(dtype, D)
    want = run(sfa, dtype, D, G, "blmhd", window, S)
    sfa.check_decode_status()
    kd, vd = c.kc.clone().to(dev), c.vc.clone().to(dev)
    o = torch.full((B, t.H, D), 7.0, dtype=TDT[dtype], device=dev)
    sl = torch.tensor(list(LENS), dtype=torch.int32, device=dev)
    held = [x.to(dev) for x in (t.qkv, t.qb, t.kb, t.vb)]
    a, *_ = ops._decode_args(*held, kd, vd, sl, o, B, M, t.H, D, t.rot, M, L, LAYER, None, None, None, "blmhd", None, HKV)
    lib = _lib.load()
    a.stride = (t.H + 2 * HKV) * D
    nbytes = lib.sfa_decode_window_workspace_bytes(B, t.H, HKV, D, M, window, S)
    assert nbytes == lib.sfa_decode_workspace_bytes(B, t.H, D, M, S)
    call_with_exact_workspace(a, nbytes, S, lambda args, stream: lib.sfa_decode_window(args, window, stream), dev,
                              fill=0xFF)
    assert torch.equal(bits(o.cpu()), want.o)
    assert torch.equal(bits(kd.cpu()), want.kc) and torch.equal(bits(vd.cpu()), want.vc)
    assert bool(torch.isfinite(o.float()).all())
