"""GPU checks of sfa_decode_mla_chunk (n new tokens per sequence of latent-attention decode) through the Python operator.
Reference: the call's definition -- tests/mla_ref.py's fp64 single-token step applied n times to a copy of the cache, the
row each step returns written back before the next.  Tolerance: the project's decode tolerance (window_ref.TOL: fp16
2e-3, bf16 1.6e-2, atol = rtol); the appended latent bit-exact, the appended rope part within one storage ulp, every
other cache bit unchanged.  Geometry and layouts are test_decode_mla_gpu.py's: B = 3, layer 1 of 2, M = 256.

The rope part: one storage ulp of the reference's rounded value, plus what the fp32 recipe (sfa_decode_mla's, which this
call must reproduce bit for bit) carries whatever the result's size: a rotated element a cos - b sin moves by at most
hypot(a, b) times the error of the angle and of the fp32 arithmetic.  The arithmetic (two products, a sum, sincosf) is
bounded by 2^-22; in-kernel angles add (pos + t) 2^-23, the device's powf and numpy's differing in the last fp32 bit
of inv_freq.  Without that term a result that cancels fails the bare ulp: measured at fp16, H = 48, n = 1, pos 64, an
element of value -0.00522 stored 7.6e-6 = 2 ulp from the reference (the single-token call stores the same bits).
"""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from mla_ref import D, DV, mla_decode_ref
from oracle import rotary_table_ref
from test_decode_mla_gpu import B, L, LAYER, LENS, M, MANT, NAN16, TDT, from_layout, page_table, to_layout
from window_ref import TOL

pytestmark = pytest.mark.gpu

# (dtype, num_heads, n, layout, num_splits, rotary tables).  The row-block counts R = n H / 16 by name: 1, 2, 3 (NHB = 4
# with an idle wave), 4, 9 (a partial last group), 256.  Every H of {16, 32, 48, 64, 128} occurs, every n of {1, 2, 3, 8,
# 17, 32} twice, and each value of dtype, layout, splits and tables meets each value of the other three; a
# dozen cases cannot also pair every H with every n (30 pairs) or every n with every layout (18).
SWEEP = [
    ("fp16", 16, 1, "blmhd", 0, False), ("bf16", 16, 2, "paged16", 1, True), ("fp16", 16, 3, "paged64", 3, False),
    ("bf16", 64, 1, "paged16", 3, False), ("fp16", 48, 3, "blmhd", 1, True), ("bf16", 128, 32, "paged64", 0, True),
    ("fp16", 32, 8, "paged16", 0, True), ("bf16", 32, 17, "blmhd", 3, True), ("fp16", 128, 2, "paged64", 1, False),
    ("bf16", 64, 17, "paged64", 3, True), ("fp16", 128, 8, "blmhd", 3, False), ("bf16", 16, 32, "paged16", 0, False),
]


@pytest.fixture(scope="module")
def sfa():
    import starflashattention_amd as m
    m._lib.load()                  # fail loudly if the HIP library is missing
    return m


@functools.lru_cache(maxsize=None)
def base():
    """N(0, 1) for 32 tokens and 128 heads, and the canonical cache [B, L, M, 576]: drawn once for the whole module"""
    g = torch.Generator().manual_seed(11)
    return SimpleNamespace(q=torch.randn(B, 32, 128, D, generator=g), kvn=torch.randn(B, 32, D, generator=g),
                           cache=torch.randn(B, L, M, D, generator=g))


@functools.lru_cache(maxsize=None)
def problem(dtype, H):
    """q (the first H heads; a test takes the first n tokens), kv_new and the cache in `dtype`: never modified"""
    x = base()
    return SimpleNamespace(q=x.q[:, :, :H].to(TDT[dtype]), kvn=x.kvn.to(TDT[dtype]), cache=x.cache.to(TDT[dtype]))


f = lambda t: t.float().numpy()


def reference(q, kvn, layer, lens, good, dtype, cos, sin):
    """n single-token steps of the sequences in `good`: (o [B, n, H, 512] fp64, the rows stored [B, n, 576])"""
    layer, n = layer.copy(), q.shape[1]
    want, rows = np.zeros(q.shape[:3] + (DV,)), np.zeros(kvn.shape, np.float32)
    for t in range(n):
        at = [pos + t if b in good else 0 for b, pos in enumerate(lens)]
        want[:, t], rows[:, t] = mla_decode_ref(q[:, t], kvn[:, t], layer, at, dtype, cos_table=cos, sin_table=sin)
        for b in good:
            layer[b, at[b]] = rows[b, t]
    return want, rows


def run(sfa, dtype, H, n, layout, splits, tables, lens, kvn=None, cache=None, poison=False, spoil_table=None, good=None):
    """One call on a fresh device copy, checked against the reference: o and the appended rows of the sequences in
    `good` (default all), every other cache bit unchanged.  poison: NaN bits wherever the call must not read.
    Returns (o on the device, the device cache, the reference o, what the call was given)."""
    p = problem(dtype, H)
    q, kvn = p.q[:, :n].contiguous(), (p.kvn if kvn is None else kvn)[:, :n].contiguous()
    cache = (p.cache if cache is None else cache).clone()
    good = range(B) if good is None else good
    tbl = None
    if poison:
        cb = cache.view(torch.int16)
        cb[:, 1 - LAYER] = NAN16
        for b, pos in enumerate(lens):
            cb[b, LAYER, pos + n:] = NAN16
    dc = to_layout(cache, layout, NAN16 if poison else 0).cuda()
    if layout != "blmhd":
        ps = int(layout[5:])
        tbl, pages = page_table(ps)
        tbl = tbl.to(torch.int32)
        if poison:
            for b, pos in enumerate(lens):
                tbl[b, (pos + n - 1) // ps + 1:] = pages + 7       # entries past the last needed page: out of range
        if spoil_table:
            tbl[spoil_table] = pages
        tbl = tbl.cuda()
    cos, sin = rotary_table_ref(M, 64, dtype) if tables else (None, None)
    dev_tab = lambda t: None if t is None else torch.from_numpy(t).to(TDT[dtype]).cuda()
    kw = dict(idx_layer=LAYER, num_splits=splits, rotary_cos_table=dev_tab(cos), rotary_sin_table=dev_tab(sin),
              block_table=tbl)
    o = torch.zeros(B, n, H, DV, dtype=TDT[dtype], device="cuda")
    sfa.flash_decode_mla_chunk(q.cuda(), kvn.cuda(), dc, torch.tensor(lens, dtype=torch.int32, device="cuda"), o, **kw)
    want, rows = reference(f(q), f(kvn), f(cache[:, LAYER]), lens, good, dtype, cos, sin)
    got, after = f(o.cpu()), from_layout(dc, layout)
    expect = cache.clone()
    for b in good:
        new = slice(lens[b], lens[b] + n)
        np.testing.assert_allclose(got[b], want[b], atol=TOL[dtype], rtol=TOL[dtype], err_msg=f"o[{b}]")
        stored = f(after[b, LAYER, new])
        assert np.array_equal(stored[:, :DV], f(kvn[b, :, :DV])), "the appended latents are bit-exact copies"
        ulp = 2.0 ** (np.floor(np.log2(np.maximum(np.abs(rows[b, :, DV:]), 1e-30))) - MANT[dtype])
        pair = np.hypot(f(kvn[b, :, DV::2]), f(kvn[b, :, DV + 1::2])).repeat(2, axis=1)
        angle = 0 if tables else (lens[b] + np.arange(n))[:, None] * 2.0 ** -23
        err = np.abs(stored[:, DV:] - rows[b, :, DV:])
        assert np.all(err <= ulp + pair * (2.0 ** -22 + angle)), f"the appended rope parts: {(err / ulp).max()} ulp"
        expect[b, LAYER, new] = after[b, LAYER, new]
    assert torch.equal(after.view(torch.int16), expect.view(torch.int16)), "a cache row other than the appended ones changed"
    return o, dc, want, SimpleNamespace(q=q, kvn=kvn, cache=cache, kw=kw)


@pytest.mark.parametrize("dtype,H,n,layout,splits,tables", SWEEP)
def test_parity_sweep(sfa, dtype, H, n, layout, splits, tables):
    run(sfa, dtype, H, n, layout, splits, tables, tuple(min(pos, M - n) for pos in LENS))
    sfa.check_decode_status()


@pytest.mark.parametrize("H", [16, 128])
@pytest.mark.parametrize("n", [3, 17])
@pytest.mark.parametrize("pos", [0, 31, 32, 33, "M-n"])
def test_tile_split_and_page_edges(sfa, H, n, pos):
    """pos = 0 is the new tile alone; at 33 with 3 splits a split is empty; n = 17 at 31 appends across three pages"""
    pos, top = (M - n if pos == "M-n" else pos), M - n + 1
    run(sfa, "bf16", H, n, "paged16", 3, False, (pos, (pos + 97) % top, (pos + 180) % top))


@pytest.mark.parametrize("where", [0, 2, 3, "pos-1"])
def test_causality_inside_the_chunk(sfa, where, H=16, n=4):
    """one row -- new token `where`, or the last cached one -- gets 8 q of its own token's head 5 in its latent and a
    marked value: it dominates where it is visible, and a leak into the tokens before it fails by far more than TOL.
    H = 16, n = 4: the four tokens are the four waves of ONE workgroup, told apart by nvalid = t + 1 alone"""
    p = problem("bf16", H)
    kvn, cache = p.kvn.clone(), p.cache.clone()
    mark = (8 * p.q[:, 0 if where == "pos-1" else where, 5, :DV].float() + torch.arange(DV) % 7).to(torch.bfloat16)
    for b, pos in enumerate(LENS):
        if where == "pos-1":
            cache[b, LAYER, pos - 1, :DV] = mark[b]
        else:
            kvn[b, where, :DV] = mark[b]
    run(sfa, "bf16", H, n, "paged64", 3, True, tuple(min(pos, M - n) for pos in LENS), kvn=kvn, cache=cache)


def test_same_bytes_as_n_single_calls(sfa, dtype="fp16", H=16, n=4, layout="paged16"):
    lens = (31, 64, M - n)
    _, dc, want, x = run(sfa, dtype, H, n, layout, 3, False, lens)
    dc1 = to_layout(x.cache, layout).cuda()
    o1 = torch.zeros(n, B, H, DV, dtype=TDT[dtype], device="cuda")
    for t in range(n):
        seq = torch.tensor(lens, dtype=torch.int32, device="cuda") + t
        sfa.flash_decode_mla(x.q[:, t].contiguous().cuda(), x.kvn[:, t].contiguous().cuda(), dc1, seq, o1[t], **x.kw)
    assert torch.equal(dc.view(torch.int16), dc1.view(torch.int16)), "one chunk call and n single calls: the same cache bytes"
    np.testing.assert_allclose(f(o1.cpu()).transpose(1, 0, 2, 3), want, atol=TOL[dtype], rtol=TOL[dtype])


@pytest.mark.parametrize("layout", ["blmhd", "paged16"])
def test_unread_memory_may_hold_nan(sfa, layout):
    o, *_ = run(sfa, "fp16", 32, 5, layout, 3, False, (33, 100, 7), poison=True)
    assert torch.isfinite(o.float()).all()
    sfa.check_decode_status()


@pytest.mark.parametrize("what", ["seq_len", "block_table"])
def test_rejection(sfa, what):
    """sequence 1 is refused -- pos + n = M + 1, or a bad entry on the SECOND page of [pos, pos + n): every token of o[1]
    NaN, its cache untouched (run checks that), the others right, the status sticky, the next good call clean"""
    n = 3           # rows 62, 63, 64 of sequence 1 lie on pages 3 and 4
    lens, spoil, status = ((33, M + 1 - n, 200), None, -7) if what == "seq_len" else ((33, 62, 200), (1, 4), -8)
    o, *_ = run(sfa, "bf16", 32, n, "paged16", 3, False, lens, spoil_table=spoil, good=(0, 2))
    assert torch.isnan(o[1].float()).all()
    with pytest.raises(sfa.SfaError) as e:
        sfa.check_decode_status()
    assert e.value.status == status
    run(sfa, "bf16", 32, n, "paged16", 3, False, (33, 62, 200))
    sfa.check_decode_status()              # reset by the failed poll: the next good call is clean
