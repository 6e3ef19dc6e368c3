"""GPU checks of sfa_decode_varlen_window (the sliding window over a ragged, packed batch of new tokens): the checks of
tests/test_decode_chunk_window_gpu.py through the packed call, one mixed batch, bit-identity with
sfa_decode_chunk_window at uniform lengths and with sfa_decode_varlen where the window does not bind, rejection and
graph replay.  Reference, tolerances and frame: tests/chunk_window_ref.py."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from chunk_window_ref import (HKV, L, LAYER, LENS, M, SWEEP, TDT, bits, check_against_reference, chunk_window_ref,
                              make_problem, problem, run, sweep_tokens)
from test_decode_chunk_window_gpu import (bad_read_page_case, parity_case, rejection_case, sfa,  # noqa: F401
                                          unread_memory_case)

pytestmark = pytest.mark.gpu

MIXED_LENS, MIXED_NS = (700, 64, 0, 100, 1000), (0, 1, 7, 300, 40)


@pytest.mark.parametrize("case", list(enumerate(SWEEP)), ids=lambda c: "-".join(str(x) for x in c[1]))
def test_varlen_window_parity_sweep(sfa, case):
    parity_case(sfa, case, True)


def mixed_problem(dtype, D, G):
    return make_problem(dtype, D, G, MIXED_LENS, MIXED_NS, seed=5)


@pytest.mark.parametrize("case", [("bf16", 128, 1, "paged16", 0, 100), ("fp16", 64, 1, "blmhd", 3, 33),
                                  ("fp16", 128, 4, "blhmd", 1, 17), ("bf16", 64, 8, "paged64", 3, 129),
                                  ("bf16", 128, 2, "blmhd", 1, 1)], ids=lambda c: "-".join(str(x) for x in c))
def test_varlen_window_mixed_batch(sfa, case):
    """n_b = [0, 1, 7, 300, 40]: an idle sequence, a decode step, a verify step, a prompt chunk of several q-tiles, and
    a chunk at a long history, in one call"""
    dtype, D, G, layout, num_splits, window = case
    prob = mixed_problem(dtype, D, G)
    r = run(sfa, prob, layout, window, num_splits, varlen=True)
    sfa.check_decode_status()
    check_against_reference(r, prob, chunk_window_ref(prob, window))
    if r.spare_k is not None:
        assert not bool(r.spare_k.any()) and not bool(r.spare_v.any())


@pytest.mark.parametrize("num_splits", [1, 3])
@pytest.mark.parametrize("window", [1, 17, 100, 5000])
def test_varlen_window_uniform_lengths_reproduce_chunk_window(sfa, window, num_splits):
    for dtype, D, G, layout in (("bf16", 128, 8, "paged16"), ("fp16", 64, 1, "blhmd")):
        prob = problem(dtype, D, G, sweep_tokens(G))
        c = run(sfa, prob, layout, window, num_splits)
        v = run(sfa, prob, layout, window, num_splits, varlen=True)
        sfa.check_decode_status()
        assert all(torch.equal(a, b) for a, b in zip(v.o, c.o))
        assert torch.equal(v.kc, c.kc) and torch.equal(v.vc, c.vc)


@pytest.mark.parametrize("num_splits", [1, 3])
def test_varlen_window_bit_identical_to_varlen_where_it_does_not_bind(sfa, num_splits):
    for dtype, D, G, layout in (("bf16", 128, 4, "paged64"), ("fp16", 64, 1, "blmhd")):
        prob = mixed_problem(dtype, D, G)
        full = run(sfa, prob, layout, None, num_splits, varlen=True)
        r = run(sfa, prob, layout, max(p + n for p, n in zip(MIXED_LENS, MIXED_NS)), num_splits, varlen=True)
        sfa.check_decode_status()
        assert all(torch.equal(a, b) for a, b in zip(r.o, full.o))
        assert torch.equal(r.kc, full.kc) and torch.equal(r.vc, full.vc)


@pytest.mark.parametrize("window", [1, 16, 100])
@pytest.mark.parametrize("num_splits", [1, 4])
def test_varlen_window_reads_nothing_below_it(sfa, window, num_splits):
    unread_memory_case(sfa, window, 16, num_splits, True)


def test_varlen_window_rejects_like_varlen(sfa):
    rejection_case(sfa, True)


def test_varlen_window_bad_table_entry_inside_and_below_the_window(sfa):
    bad_read_page_case(sfa, 3, True)


def test_varlen_window_bad_arguments(sfa):
    prob = problem("fp16", 64, 2, 40)
    for w in (0, -3):
        with pytest.raises(RuntimeError, match="window"):
            run(sfa, prob, "blmhd", w, varlen=True)
    dev = torch.device("cuda:0")
    B, H, D, T = 1, 2, 256, 2
    z = torch.zeros(0, dtype=torch.float16, device=dev)
    qkv = torch.zeros(T, 3, H, D, dtype=torch.float16, device=dev)
    kc = torch.zeros(B, 1, 64, H, D, dtype=torch.float16, device=dev)
    o = torch.zeros(T, H, D, dtype=torch.float16, device=dev)
    sl = torch.zeros(B, dtype=torch.int32, device=dev)
    cu = torch.tensor([0, T], dtype=torch.int32, device=dev)
    with pytest.raises(sfa.SfaError) as e:
        sfa.flash_decode_varlen_window(qkv, z, z, z, kc, kc.clone(), sl, o, cu, B, 64, H, D, 0, 64, 1, 0, 8)
    assert e.value.status == -4


def test_varlen_window_graph_replay(sfa):
    """One captured flash_decode_varlen_window call, replayed with two different cu_tokens / seq_len contents under the
    same total_tokens bound: lo and the lengths are read on the device, so both replays are correct."""
    dtype, D, G, window, T = "fp16", 128, 2, 33, 48
    dev = torch.device("cuda:0")
    probs = [make_problem(dtype, D, G, (3, 700, 64, 31), (3, 0, 40, 5), seed=1),
             make_problem(dtype, D, G, (1300, 0, 97, 500), (1, 20, 0, 10), seed=2)]
    p0 = probs[0]
    dt = TDT[dtype]
    qkv = torch.zeros(T, p0.H + 2 * HKV, D, dtype=dt, device=dev)
    kd = torch.zeros(p0.B, L, M, HKV, D, dtype=dt, device=dev)
    vd = torch.zeros_like(kd)
    o = torch.zeros(T, p0.H, D, dtype=dt, device=dev)
    sl = torch.zeros(p0.B, dtype=torch.int32, device=dev)
    cu = torch.zeros(p0.B + 1, dtype=torch.int32, device=dev)  # all sequences idle during warm-up and capture
    qb, kb, vb = (torch.zeros_like(x).to(dev) for x in (p0.qb, p0.kb, p0.vb))
    call = lambda: sfa.flash_decode_varlen_window(qkv, qb, kb, vb, kd, vd, sl, o, cu, p0.B, M, p0.H, D, p0.rot, M, L, LAYER,
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
            cu_h = np.concatenate([[0], np.cumsum(p.ns)]).astype(np.int32)
            packed = torch.zeros(T, p.H + 2 * HKV, D, dtype=dt)
            for b, n in enumerate(p.ns):
                packed[cu_h[b]:cu_h[b + 1]] = p.qkv[b, :n]
            for dst, src in ((qkv, packed), (kd, p.kc), (vd, p.vc), (qb, p.qb), (kb, p.kb), (vb, p.vb)):
                dst.copy_(src.to(dev))
            o.fill_(7.0)
            sl.copy_(torch.tensor(list(p.lens), dtype=torch.int32))
            cu.copy_(torch.from_numpy(cu_h))
            graph.replay()
            side.synchronize()
            sfa.check_decode_status(dev)
            ob = bits(o.cpu())
            r = SimpleNamespace(o=[ob[cu_h[b]:cu_h[b + 1]] for b in range(p.B)], kc=bits(kd.cpu()), vc=bits(vd.cpu()))
            check_against_reference(r, p, chunk_window_ref(p, window))
            assert bool((ob[cu_h[-1]:].view(dt) == 7.0).all())              # rows past cu_tokens[B] are not written
