"""GPU checks of sfa_decode_chunk_window (the sliding window in the multi-token decode step) through the Python operator
and the C ABI: parity with the fp64 reference of tests/chunk_window_ref.py over a pairwise-covering sweep, bit-identity
with sfa_decode_chunk where the window does not bind, agreement with n successive sfa_decode_window calls, the window's
edges, the promise that nothing below lo_0 is read, rejection, the workspace and graph replay.

Tolerances are the project's decode tolerances (window_ref.TOL: kernel vs fp64 reference on identically rounded inputs,
fp16 2e-3, bf16 1.6e-2, atol = rtol), elementwise, nothing exempt.  The common frame: B = 4 sequences at seq_len =
[0, 5, 130, 1000], 2 kv heads, 2 layers, memory_max_len 1408, q / k / v bias and a partial rotary embedding.
"""
import numpy as np
import pytest
import torch

from chunk_window_ref import (EDGE_N, EDGE_WINDOWS, HKV, INF16, L, LAYER, LENS, M, NAN16, SWEEP, TDT, TOL, append_mask,
                              as_float, bits, check_against_reference, chunk_window_ref, edge_problem, make_problem,
                              page_table, problem, reference, run, spike_rows, sweep_tokens, window_lo)

pytestmark = pytest.mark.gpu

VARLEN = False                                   # tests/test_decode_varlen_window_gpu.py runs these through the packed call


@pytest.fixture(scope="module")
def sfa():
    assert torch.cuda.is_available(), "GPU tests need a GPU (run with -m gpu on the MI355X box)"
    import starflashattention_amd as m
    m._lib.load()                  # fail loudly if the HIP library is missing
    return m


def same_appends(r, other, prob):
    m = append_mask(prob)
    return torch.equal(r.kc[~m], other.kc[~m]) and torch.equal(r.vc[~m], other.vc[~m])


# ---- parity ------------------------------------------------------------------------------------------------------------

def parity_case(sfa, case, varlen):
    i, (dtype, D, layout, G, num_splits, window) = case
    tables = bool(i & 1)                        # every other case reads the rotary tables instead of computing cos / sin
    n = sweep_tokens(G)
    prob, ref = problem(dtype, D, G, n, tables), reference(dtype, D, G, n, window, tables)
    r = run(sfa, prob, layout, window, num_splits, varlen=varlen)
    sfa.check_decode_status()
    check_against_reference(r, prob, ref)
    # the prologue is shared: the appended rows are the plain call's, bit for bit, at every window
    plain = run(sfa, prob, "blmhd", None, 1, varlen=varlen)
    assert same_appends(r, plain, prob)
    if r.spare_k is not None:
        assert not bool(r.spare_k.any()) and not bool(r.spare_v.any())


@pytest.mark.parametrize("case", list(enumerate(SWEEP)), ids=lambda c: "-".join(str(x) for x in c[1]))
def test_chunk_window_parity_sweep(sfa, case):
    parity_case(sfa, case, VARLEN)


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_chunk_window_binds(sfa, dtype):
    """pos = 1000, window = 100: the windowed and the full reference differ by many tolerances (the factor is asserted on
    the CPU as well), and the device sides with the windowed one."""
    D, G, n, window = 128, 4, 40, 100
    prob = problem(dtype, D, G, n)
    ref, full = reference(dtype, D, G, n, window), reference(dtype, D, G, n, None)
    b = LENS.index(1000)
    tol = TOL[dtype]
    gap = np.abs(ref[b][0] - full[b][0])
    assert gap.max() > 10 * tol * (1.0 + np.abs(full[b][0]).max()), gap.max()
    r = run(sfa, prob, "blmhd", window, varlen=VARLEN)
    sfa.check_decode_status()
    check_against_reference(r, prob, ref)
    assert np.abs(as_float(r.o[b], dtype) - full[b][0]).max() > 5 * tol


@pytest.mark.parametrize("num_splits", [1, 3])
@pytest.mark.parametrize("layout", ["blmhd", "blhmd", "paged16", "paged64"])
def test_chunk_window_bit_identical_to_chunk_where_it_does_not_bind(sfa, layout, num_splits):
    """window >= pos + n for every sequence: lo = 0 everywhere, the same tile partition, the same bits"""
    for dtype, D, G in (("bf16", 128, 8), ("fp16", 64, 1), ("fp16", 128, 2)):
        n = sweep_tokens(G)
        prob = problem(dtype, D, G, n)
        full = run(sfa, prob, layout, None, num_splits, varlen=VARLEN)
        for window in (max(LENS) + n, 5000):
            r = run(sfa, prob, layout, window, num_splits, varlen=VARLEN)
            sfa.check_decode_status()
            assert all(torch.equal(a, b) for a, b in zip(r.o, full.o)), (dtype, D, G, window)
            assert torch.equal(r.kc, full.kc) and torch.equal(r.vc, full.vc)


@pytest.mark.parametrize("window", [1, 33, 100])
def test_chunk_window_against_successive_decode_window_calls(sfa, window):
    """n successive sfa_decode_window calls on the device, seq_len advanced by one each time: the same outputs within
    tolerance (both are within it of the same reference) and the same appended rows bit for bit"""
    dtype, D, G, n, layout = "bf16", 128, 4, 40, "paged16"
    prob = problem(dtype, D, G, n)
    r = run(sfa, prob, layout, window, varlen=VARLEN)
    sfa.check_decode_status()
    dev = torch.device("cuda:0")
    from chunk_window_ref import from_layout, to_layout
    kd, vd = to_layout(prob.kc, layout).to(dev), to_layout(prob.vc, layout).to(dev)
    table = torch.from_numpy(page_table(16, prob.B)[0]).to(dev)
    o = torch.empty(prob.B, n, prob.H, D, dtype=TDT[dtype], device=dev)
    held = [x.to(dev) for x in (prob.qb, prob.kb, prob.vb)]
    for t in range(n):
        sl = torch.tensor([pos + t for pos in LENS], dtype=torch.int32, device=dev)
        ot = torch.empty(prob.B, prob.H, D, dtype=TDT[dtype], device=dev)
        sfa.flash_decode_window(prob.qkv[:, t].contiguous().to(dev), *held, kd, vd, sl, ot, prob.B, M, prob.H, D, prob.rot,
                                M, L, LAYER, window, kv_layout="paged", block_table=table, num_heads_kv=HKV)
        o[:, t] = ot
    torch.cuda.synchronize()
    sfa.check_decode_status()
    tol = TOL[dtype]
    for b in range(prob.B):
        np.testing.assert_allclose(as_float(r.o[b], dtype), o[b].float().cpu().numpy(), atol=tol, rtol=tol)
    assert torch.equal(from_layout(kd, layout, prob.B)[0], r.kc) and torch.equal(from_layout(vd, layout, prob.B)[0], r.vc)


# ---- the window's edges ------------------------------------------------------------------------------------------------

EDGE_LAYOUTS = {17: "paged16", 32: "blmhd", 40: "blhmd", 100: "paged64"}


@pytest.mark.parametrize("num_splits", [1, 3, 4])
@pytest.mark.parametrize("window", EDGE_WINDOWS)
def test_chunk_window_edges(sfa, window, num_splits):
    """rotary_embedding_dim = 0 and no bias, one sequence per lo_0 in {0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128,
    129}, G = 1 and 300 tokens (two q-tiles):
      (a) a key that carries all the weight at row j*: every token that sees it returns the bits of V[j*], the first
          token with lo_t = j* + 1 does not (it is the first / last row of a wave, the first row of the second q-tile,
          or has lo_t on a 64-key / 32-key boundary);
      (b) all keys equal, V rows of alternating, marked magnitude: one row dropped, added or counted twice at either edge
          of any token's window leaves the tolerance (asserted on the CPU from the reference alone);
      (c) a ramp of scores that keeps rising below lo_t."""
    layout = EDGE_LAYOUTS[window]
    for dtype in ("fp16", "bf16"):
        spike = edge_problem(dtype, window, "spike")
        ref = chunk_window_ref(spike, window)
        r = run(sfa, spike, layout, window, num_splits, varlen=VARLEN)
        sfa.check_decode_status()
        check_against_reference(r, spike, ref)
        for b, (pos, jstar) in enumerate(spike_rows(window)):
            vstar = r.vc[b, LAYER, jstar]                                       # [Hkv, D] bits, G = 1
            seen = 0
            for t in range(EDGE_N):
                if window_lo(pos + t, window) <= jstar <= pos + t:
                    assert torch.equal(r.o[b][t], vstar), (dtype, b, t)
                    seen += 1
                else:
                    assert not torch.equal(r.o[b][t], vstar), (dtype, b, t)
            assert seen >= min(window, 17)
        for kind in ("equal", "ramp"):
            prob = edge_problem(dtype, window, kind)
            r = run(sfa, prob, layout, window, num_splits, varlen=VARLEN)
            sfa.check_decode_status()
            check_against_reference(r, prob, chunk_window_ref(prob, window))


# ---- what the window promises not to read ------------------------------------------------------------------------------

def poisoned(c, prob, window, dtype, word):
    """a copy of the canonical cache c with NaN / +Inf in every row the call must not read: the other layer, the rows
    below lo_0 and the rows at or beyond pos + n"""
    p = c.clone()
    pb = p.view(torch.int16)
    pb[:, 1 - LAYER] = word
    for b, (pos, n) in enumerate(zip(prob.lens, prob.ns)):
        pb[b, LAYER, :window_lo(pos, window)] = word
        pb[b, LAYER, pos + n:] = word
    return p


def unread_memory_case(sfa, window, ps, num_splits, varlen, prob=None):
    dtype, D, G, n = "bf16", 128, 4, 40
    prob = problem(dtype, D, G, n) if prob is None else prob
    layout = f"paged{ps}"
    clean = run(sfa, prob, layout, window, num_splits, varlen=varlen)
    sfa.check_decode_status()
    m = append_mask(prob)
    for word in (NAN16, INF16[dtype]):
        pk, pv = poisoned(prob.kc, prob, window, dtype, word), poisoned(prob.vc, prob, window, dtype, word)
        table = page_table(ps, prob.B)[0].copy()
        for b, (pos, nb) in enumerate(zip(prob.lens, prob.ns)):
            table[b, :window_lo(pos, window) // ps] = -1                    # wholly below lo_0
            table[b, (pos + nb - 1) // ps + 1:] = -1                        # past the last page
        b1000 = prob.lens.index(1000)
        assert (table[b1000] == -1).sum() >= (1001 - window) // ps > 0
        r = run(sfa, prob, layout, window, num_splits, varlen=varlen, kc=pk, vc=pv, table=table, spare_bits=word)
        sfa.check_decode_status()
        for a, c in zip(r.o, clean.o):
            assert bool(torch.isfinite(a.view(TDT[dtype]).float()).all())
            assert torch.equal(a, c)
        assert same_appends(r, clean, prob)
        assert torch.equal(r.kc[m], bits(pk)[m]) and torch.equal(r.vc[m], bits(pv)[m])       # the poison, and the rest
        assert bool((r.spare_k == word).all()) and bool((r.spare_v == word).all())
        # the contiguous layouts keep the same promise
        for lay in ("blmhd", "blhmd"):
            c2 = run(sfa, prob, lay, window, num_splits, varlen=varlen)
            r2 = run(sfa, prob, lay, window, num_splits, varlen=varlen, kc=pk, vc=pv)
            sfa.check_decode_status()
            assert all(torch.equal(a, c) for a, c in zip(r2.o, c2.o))
            assert same_appends(r2, c2, prob)
            assert torch.equal(r2.kc[m], bits(pk)[m]) and torch.equal(r2.vc[m], bits(pv)[m])


@pytest.mark.parametrize("window", [1, 16, 17, 100])
@pytest.mark.parametrize("ps", [16, 64])
@pytest.mark.parametrize("num_splits", [1, 3])
def test_chunk_window_reads_nothing_below_it(sfa, window, ps, num_splits):
    """The same call on a clean problem and on one with NaN (0x7FFF) / +Inf in every cache row below lo_0 and at or beyond
    pos + n, in the other layer and in the spare pages, and -1 in every block_table entry wholly below lo_0 and past the
    last page: o and the appended rows bit-identical, the status clean, every poisoned byte still in place."""
    unread_memory_case(sfa, window, ps, num_splits, VARLEN)


def test_chunk_window_exact_workspace_with_empty_splits(sfa):
    """sfa_decode_chunk_window itself at num_splits = 4 with a workspace of exactly
    sfa_decode_chunk_window_workspace_bytes bytes, every fp32 of it a NaN beforehand, and a window so short (17 rows
    over 40 tokens: two key tiles) that splits are empty: bit-identical to the operator, nothing written past the end."""
    from exact_workspace import call_with_exact_workspace
    from starflashattention_amd import _lib, ops
    dtype, D, G, n, window, S = "bf16", 128, 4, 40, 17, 4
    prob = problem(dtype, D, G, n)
    dev = torch.device("cuda:0")
    want = run(sfa, prob, "blmhd", window, S)
    sfa.check_decode_status()
    kd, vd = prob.kc.clone().to(dev), prob.vc.clone().to(dev)
    o = torch.full((prob.B, n, prob.H, D), 7.0, dtype=TDT[dtype], device=dev)
    sl = torch.tensor(list(LENS), dtype=torch.int32, device=dev)
    held = [x.to(dev) for x in (prob.qkv, prob.qb, prob.kb, prob.vb)]
    a, *_ = ops._decode_args(*held, kd, vd, sl, o, prob.B, M, prob.H, D, prob.rot, M, L, LAYER, None, None, None, "blmhd",
                             None, HKV, tokens=n)
    lib = _lib.load()
    nbytes = lib.sfa_decode_chunk_window_workspace_bytes(prob.B, prob.H, HKV, D, M, n, window, S)
    assert nbytes == lib.sfa_decode_chunk_workspace_bytes(prob.B, prob.H, HKV, D, M, n, S)
    call_with_exact_workspace(a, nbytes, S, lambda args, stream: lib.sfa_decode_chunk_window(args, n, 0, window, stream),
                              dev, fill=0xFF)
    ob = bits(o.cpu())
    assert all(torch.equal(ob[b], want.o[b]) for b in range(prob.B))
    assert torch.equal(bits(kd.cpu()), want.kc) and torch.equal(bits(vd.cpu()), want.vc)
    assert bool(torch.isfinite(o.float()).all())


# ---- rejection ---------------------------------------------------------------------------------------------------------

def rejection_case(sfa, varlen):
    """pos + n > M and a bad append page: NaN, the sequence's cache untouched, the chunk call's status; the others as
    they were"""
    dtype, D, G, n, window = "bf16", 128, 4, 40, 100
    prob = problem(dtype, D, G, n)
    good = run(sfa, prob, "blmhd", window, varlen=varlen)
    sfa.check_decode_status()
    lens = (0, M - n + 1, 130, -1)
    r = run(sfa, prob, "blmhd", window, varlen=varlen, lens=lens)
    with pytest.raises(RuntimeError, match="seq_len"):
        sfa.check_decode_status()
    for b in (1, 3):
        assert bool(torch.isnan(r.o[b].view(TDT[dtype])).all())
    m = append_mask(prob, (0, -1, 130, -1))
    assert torch.equal(r.kc[m], bits(prob.kc)[m]) and torch.equal(r.vc[m], bits(prob.vc)[m])
    assert torch.equal(r.o[0], good.o[0]) and torch.equal(r.o[2], good.o[2])
    assert torch.equal(r.kc[~m], good.kc[~m])
    # an append page of sequence 2 (rows 130 .. 169) outside the pool
    ps = 16
    table = page_table(ps, prob.B)[0].copy()
    table[2, 150 // ps] = -7
    goodp = run(sfa, prob, "paged16", window, varlen=varlen)
    sfa.check_decode_status()
    r = run(sfa, prob, "paged16", window, varlen=varlen, table=table)
    with pytest.raises(RuntimeError, match="block_table"):
        sfa.check_decode_status()
    assert bool(torch.isnan(r.o[2].view(TDT[dtype])).all())
    m = append_mask(prob, (0, 5, -1, 1000))     # nothing of sequence 2 was written, anywhere in the pools
    assert torch.equal(r.kc[m], bits(prob.kc)[m]) and torch.equal(r.vc[m], bits(prob.vc)[m])
    assert not bool(r.spare_k.any()) and not bool(r.spare_v.any())
    for b in (0, 1, 3):
        assert torch.equal(r.o[b], goodp.o[b])


def bad_read_page_case(sfa, num_splits, varlen):
    """a bad entry on a read page inside the window: NaN for that sequence and the status; the same entry on a page
    wholly below lo_0: nothing"""
    dtype, D, G, n, window, ps = "fp16", 128, 8, 40, 100, 16
    prob = problem(dtype, D, G, n)
    b, lo = LENS.index(1000), window_lo(1000, window)
    _, npages = page_table(ps, prob.B)
    clean = run(sfa, prob, "paged16", window, num_splits, varlen=varlen)
    sfa.check_decode_status()
    inside = page_table(ps, prob.B)[0].copy()
    inside[b, lo // ps + 1] = npages            # a page the window reads and no token appends to
    r = run(sfa, prob, "paged16", window, num_splits, varlen=varlen, table=inside)
    with pytest.raises(RuntimeError, match="block_table"):
        sfa.check_decode_status()
    assert bool(torch.isnan(r.o[b].view(TDT[dtype])).all())
    assert all(torch.equal(r.o[i], clean.o[i]) for i in range(b))
    assert torch.equal(r.kc, clean.kc) and torch.equal(r.vc, clean.vc)          # reads only: the same appends
    below = page_table(ps, prob.B)[0].copy()
    below[b, lo // ps - 1] = npages             # the last page wholly below lo_0: never looked at
    below[b, 0] = -1
    r = run(sfa, prob, "paged16", window, num_splits, varlen=varlen, table=below)
    sfa.check_decode_status()
    assert all(torch.equal(x, y) for x, y in zip(r.o, clean.o))
    assert torch.equal(r.kc, clean.kc) and torch.equal(r.vc, clean.vc)


def test_chunk_window_rejects_like_chunk(sfa):
    rejection_case(sfa, VARLEN)


@pytest.mark.parametrize("num_splits", [1, 3])
def test_chunk_window_bad_table_entry_inside_and_below_the_window(sfa, num_splits):
    bad_read_page_case(sfa, num_splits, VARLEN)


def test_chunk_window_bad_arguments(sfa):
    prob = problem("fp16", 64, 2, 40)
    for w in (0, -3):
        with pytest.raises(RuntimeError, match="window"):
            run(sfa, prob, "blmhd", w, varlen=VARLEN)
    # head_dim 256: SFA_ERR_UNSUPPORTED_HEAD_DIM (-4)
    dev = torch.device("cuda:0")
    B, H, D, n = 1, 2, 256, 2
    z = torch.zeros(0, dtype=torch.float16, device=dev)
    qkv = torch.zeros(B, n, 3, H, D, dtype=torch.float16, device=dev)
    kc = torch.zeros(B, 1, 64, H, D, dtype=torch.float16, device=dev)
    o = torch.zeros(B, n, H, D, dtype=torch.float16, device=dev)
    sl = torch.zeros(B, dtype=torch.int32, device=dev)
    with pytest.raises(sfa.SfaError) as e:
        sfa.flash_decode_chunk_window(qkv, z, z, z, kc, kc.clone(), sl, o, B, 64, H, D, 0, 64, 1, 0, 8)
    assert e.value.status == -4


# ---- graph replay ------------------------------------------------------------------------------------------------------

def test_chunk_window_graph_replay(sfa):
    """One captured flash_decode_chunk_window call, replayed with two different seq_len contents: lo is computed on the
    device, so both replays are correct."""
    dtype, D, G, n, window = "fp16", 128, 2, 40, 33
    dev = torch.device("cuda:0")
    probs = [make_problem(dtype, D, G, lens, (n,) * 4, seed=s) for s, lens in ((1, (3, 700, 64, 31)), (2, (1300, 0, 97, 500)))]
    p0 = probs[0]
    dt = TDT[dtype]
    qkv = torch.zeros(p0.B, n, p0.H + 2 * HKV, D, dtype=dt, device=dev)
    kd = torch.zeros(p0.B, L, M, HKV, D, dtype=dt, device=dev)
    vd = torch.zeros_like(kd)
    o = torch.zeros(p0.B, n, p0.H, D, dtype=dt, device=dev)
    sl = torch.zeros(p0.B, dtype=torch.int32, device=dev)
    qb, kb, vb = (torch.zeros_like(x).to(dev) for x in (p0.qb, p0.kb, p0.vb))
    call = lambda: sfa.flash_decode_chunk_window(qkv, qb, kb, vb, kd, vd, sl, o, p0.B, M, p0.H, D, p0.rot, M, L, LAYER,
                                                 window, num_splits=2, num_heads_kv=HKV)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        call()                                              # warm-up: the stream's workspace exists before the capture
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            call()
        for p in probs:
            for dst, src in ((qkv, p.qkv), (kd, p.kc), (vd, p.vc), (qb, p.qb), (kb, p.kb), (vb, p.vb)):
                dst.copy_(src.to(dev))
            o.fill_(7.0)
            sl.copy_(torch.tensor(list(p.lens), dtype=torch.int32))
            graph.replay()
            side.synchronize()
            sfa.check_decode_status(dev)
            ob = bits(o.cpu())
            from types import SimpleNamespace
            r = SimpleNamespace(o=[ob[b] for b in range(p.B)], kc=bits(kd.cpu()), vc=bits(vd.cpu()))
            check_against_reference(r, p, chunk_window_ref(p, window))
