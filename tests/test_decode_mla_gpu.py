"""GPU checks of sfa_decode_mla (latent-attention decode) through the Python operator, against the fp64 reference of
tests/mla_ref.py: a pairwise-covering parity sweep, tile and split edges, which columns are key and which are value, a
dominant key at the tile seams, the promise about unread memory, rejection, and two steps on one stream.

Tolerance: the project's decode tolerance (window_ref.TOL: fp16 2e-3, bf16 1.6e-2, atol = rtol); the appended rope part
within one storage ulp of the reference's rounded value, the appended latent bit-exact.  Every problem has B = 3 sequences
at different positions, 2 layers of which layer 1 is used, and memory_max_len 256 = 8 tiles of 32 rows.
"""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from mla_ref import D, DV, mla_decode_ref
from oracle import rotary_table_ref
from window_ref import TOL

pytestmark = pytest.mark.gpu

TDT = {"fp16": torch.float16, "bf16": torch.bfloat16}
MANT = {"fp16": 10, "bf16": 7}
B, L, M, LAYER, SPARE = 3, 2, 256, 1, 3
LENS = (33, 64, M - 1)                          # one past a tile, a whole number of tiles, the last legal row
NAN16 = 0x7FFF                                  # NaN in fp16 and in bf16

# (dtype, num_heads, layout, num_splits, rotary tables): every value of every factor meets every value of every other one
SWEEP = [
    ("fp16", 16, "blmhd", 0, False), ("bf16", 16, "paged16", 1, False), ("fp16", 16, "paged64", 3, True),
    ("bf16", 32, "blmhd", 1, False), ("fp16", 32, "paged16", 3, True), ("bf16", 32, "paged64", 0, True),
    ("fp16", 64, "blmhd", 3, True), ("bf16", 64, "paged16", 0, True), ("fp16", 64, "paged64", 1, False),
    ("bf16", 128, "blmhd", 0, True), ("fp16", 128, "paged16", 1, False), ("bf16", 128, "paged64", 3, False),
    ("fp16", 128, "blmhd", 1, True), ("bf16", 16, "paged64", 1, True), ("bf16", 64, "blmhd", 3, False),
    ("fp16", 32, "paged64", 0, False),
]


@pytest.fixture(scope="module")
def sfa():
    import starflashattention_amd as m
    m._lib.load()                  # fail loudly if the HIP library is missing
    return m


@functools.lru_cache(maxsize=None)
def problem(dtype, H):
    """q, kv_new and the canonical cache [B, L, M, 576], N(0, 1): made once, never modified"""
    rng = np.random.default_rng([7, H, dtype == "bf16"])
    r = lambda *s: torch.from_numpy(rng.standard_normal(s, dtype=np.float32)).to(TDT[dtype])
    return SimpleNamespace(q=r(B, H, D), kvn=r(B, D), cache=r(B, L, M, D))


def page_table(ps):
    """(a shuffled table that lays the pool out, the number of pages: SPARE more than are used)"""
    n = B * (M // ps) + SPARE
    return torch.from_numpy(np.random.default_rng(3).permutation(n)[:B * (M // ps)].reshape(B, M // ps)), n


def to_layout(c, layout, spare_bits=0):
    if layout == "blmhd":
        return c.clone()
    ps = int(layout[5:])
    tbl, n = page_table(ps)
    pool = torch.full((n, L, ps, D), spare_bits, dtype=torch.int16).view(c.dtype)
    pool[tbl.reshape(-1)] = c.view(B, L, M // ps, ps, D).permute(0, 2, 1, 3, 4).reshape(-1, L, ps, D)
    return pool


def from_layout(dc, layout):
    if layout == "blmhd":
        return dc.cpu()
    ps = int(layout[5:])
    return dc.cpu()[page_table(ps)[0].reshape(-1)].view(B, M // ps, L, ps, D).permute(0, 2, 1, 3, 4).reshape(B, L, M, D)


def run(sfa, dtype, H, layout, splits, tables, lens, q=None, kvn=None, cache=None, poison=False, spoil_table=None,
        good=None):
    """One call on a fresh device copy, checked against the reference: o and the appended rows of the sequences in
    `good` (default all), every other cache bit unchanged.  poison: NaN bits wherever the call must not read.
    Returns (o on the device, the device cache) for what a test checks beyond that."""
    p = problem(dtype, H)
    q, kvn = p.q if q is None else q, p.kvn if kvn is None else kvn
    cache = (p.cache if cache is None else cache).clone()
    good = range(B) if good is None else good
    tbl = None
    if poison:
        cb = cache.view(torch.int16)
        cb[:, 1 - LAYER] = NAN16
        for b, pos in enumerate(lens):
            cb[b, LAYER, pos:] = NAN16
    dc = to_layout(cache, layout, NAN16 if poison else 0).cuda()
    if layout != "blmhd":
        ps = int(layout[5:])
        tbl, n = page_table(ps)
        tbl = tbl.to(torch.int32)
        if poison:
            for b, pos in enumerate(lens):
                tbl[b, pos // ps + 1:] = n + 7          # entries past the last needed page: out of range
        if spoil_table:
            tbl[spoil_table] = n
        tbl = tbl.cuda()
    cos, sin = rotary_table_ref(M, 64, dtype) if tables else (None, None)
    dev_tab = lambda t: None if t is None else torch.from_numpy(t).to(TDT[dtype]).cuda()
    o = torch.zeros(B, H, DV, dtype=TDT[dtype], device="cuda")
    sfa.flash_decode_mla(q.cuda(), kvn.cuda(), dc, torch.tensor(lens, dtype=torch.int32, device="cuda"), o,
                         idx_layer=LAYER, num_splits=splits, rotary_cos_table=dev_tab(cos), rotary_sin_table=dev_tab(sin),
                         block_table=tbl)
    f = lambda t: t.float().numpy()
    ref_lens = [pos if b in good else 0 for b, pos in enumerate(lens)]
    want, rows = mla_decode_ref(f(q), f(kvn), f(cache[:, LAYER]), ref_lens, dtype, cos_table=cos, sin_table=sin)
    got, after = f(o.cpu()), from_layout(dc, layout)
    expect = cache.clone()
    for b in good:
        np.testing.assert_allclose(got[b], want[b], atol=TOL[dtype], rtol=TOL[dtype], err_msg=f"o[{b}]")
        row = f(after[b, LAYER, lens[b]])
        assert np.array_equal(row[:DV], f(kvn[b, :DV])), "the appended latent is a bit-exact copy"
        ulp = 2.0 ** (np.floor(np.log2(np.maximum(np.abs(rows[b, DV:]), 1e-30))) - MANT[dtype])
        assert np.all(np.abs(row[DV:] - rows[b, DV:]) <= ulp), "the appended rope part"
        expect[b, LAYER, lens[b]] = after[b, LAYER, lens[b]]
    assert torch.equal(after.view(torch.int16), expect.view(torch.int16)), "a cache row other than the appended ones changed"
    return o, dc


@pytest.mark.parametrize("dtype,H,layout,splits,tables", SWEEP)
def test_parity_sweep(sfa, dtype, H, layout, splits, tables):
    run(sfa, dtype, H, layout, splits, tables, LENS)
    sfa.check_decode_status()


@pytest.mark.parametrize("H", [16, 128])
@pytest.mark.parametrize("pos", [0, 1, 31, 32, 33, 95, 200, M - 1])
def test_tile_and_split_edges(sfa, H, pos):
    """pos = 0 is the new token alone; at 33 with 3 splits a split is empty; M - 1 is the last legal row"""
    run(sfa, "bf16", H, "paged16", 3, False, (pos, (pos + 97) % M, (pos + 180) % M))


@pytest.mark.parametrize("case", ["rope_only", "latent_only", "rope_columns_x64"])
def test_which_columns_are_key_and_value(sfa, case):
    p = problem("fp16", 32)
    q, cache = p.q.clone(), p.cache.clone()
    if case == "rope_only":
        q[..., :DV] = 0
    elif case == "latent_only":
        q[..., DV:] = 0
    else:                       # large rope columns: a leak of column >= 512 into o would show
        cache[..., DV:] *= 64
        q[..., DV:] /= 64
    run(sfa, "fp16", 32, "blmhd", 1, False, LENS, q=q, cache=cache)


@pytest.mark.parametrize("where", [0, 31, 32, "pos-1", "new"])
def test_one_key_carries_the_weight(sfa, where):
    """one row gets 8 q in its latent, so it dominates every head's softmax a little differently, with a marked value"""
    p = problem("bf16", 64)
    kvn, cache = p.kvn.clone(), p.cache.clone()
    mark = (8 * p.q[:, 5, :DV].float() + torch.arange(DV) % 7).to(torch.bfloat16)
    for b, pos in enumerate(LENS):
        if where == "new":
            kvn[b, :DV] = mark[b]
        else:
            cache[b, LAYER, pos - 1 if where == "pos-1" else where, :DV] = mark[b]
    run(sfa, "bf16", 64, "paged64", 3, True, LENS, kvn=kvn, cache=cache)


@pytest.mark.parametrize("layout", ["blmhd", "paged16"])
def test_unread_memory_may_hold_nan(sfa, layout):
    o, _ = run(sfa, "fp16", 32, layout, 3, False, (33, 100, 7), poison=True)
    assert torch.isfinite(o.float()).all()
    sfa.check_decode_status()


@pytest.mark.parametrize("what", ["seq_len", "block_table"])
def test_rejection(sfa, what):
    """sequence 1 is refused: o[1] NaN, its cache untouched (run checks that), the others right, the status sticky"""
    lens, spoil, status = ((33, M, 200), None, -7) if what == "seq_len" else (LENS, (1, LENS[1] // 16), -8)
    o, _ = run(sfa, "bf16", 32, "paged16", 3, False, lens, spoil_table=spoil, good=(0, 2))
    assert torch.isnan(o[1].float()).all()
    with pytest.raises(sfa.SfaError) as e:
        sfa.check_decode_status()
    assert e.value.status == status
    run(sfa, "bf16", 32, "paged16", 3, False, LENS)
    sfa.check_decode_status()              # reset by the failed poll: the next good call is clean


def test_two_steps_on_one_stream(sfa):
    """the second call reads the row the first appended; two preallocated seq_len tensors, no synchronisation between"""
    dtype, H = "fp16", 64
    p = problem(dtype, H)
    f = lambda t: t.float().numpy()
    lens = [np.array(LENS) - 1, np.array(LENS)]
    kv2 = p.kvn.flip(0).contiguous()
    dc = p.cache.cuda()
    seq = [torch.tensor(x, dtype=torch.int32, device="cuda") for x in lens]
    o = [torch.zeros(B, H, DV, dtype=TDT[dtype], device="cuda") for _ in range(2)]
    qd, kd = p.q.cuda(), [p.kvn.cuda(), kv2.cuda()]
    for i in range(2):
        sfa.flash_decode_mla(qd, kd[i], dc, seq[i], o[i], idx_layer=LAYER, num_splits=3)
    cache = f(p.cache[:, LAYER]).copy()
    for i, kvn in enumerate((p.kvn, kv2)):
        want, rows = mla_decode_ref(f(p.q), f(kvn), cache, lens[i], dtype)
        np.testing.assert_allclose(f(o[i].cpu()), want, atol=TOL[dtype], rtol=TOL[dtype])
        cache[np.arange(B), lens[i]] = rows
