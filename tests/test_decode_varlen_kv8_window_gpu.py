"""GPU checks of sfa_decode_varlen_kv8_window (the sliding window over a ragged, packed batch of new tokens and an fp8
e4m3 KV cache): the cases of tests/test_decode_chunk_kv8_window_gpu.py through the packed call, ragged counts, a sequence
without tokens, bit-identity with sfa_decode_chunk_kv8_window at uniform lengths and with sfa_decode_varlen_kv8 where the
window does not bind, a bad cu_tokens range and graph replay.  Reference, tolerances and frame:
tests/chunk_kv8_window_ref.py."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import chunk_kv8_window_ref as ref
from chunk_kv8_window_ref import (EDGE_WINDOWS, HKV, L, LAYER, LENS, M, SWEEP, append_mask, check, make_problem, poisoned,
                                  poisoned_table, problem, run, same_bits)
from chunk_window_ref import TDT, bits
from test_decode_chunk_kv8_window_gpu import (UNREAD_LO0, UNREAD_WINDOW, bad_read_page_case, edges_case,  # noqa: F401
                                              not_binding_case, null_scales_case, parity_case, rejection_case, scales_case,
                                              sfa, status_word, unread_memory_case, unread_problems, variants_case,
                                              window_binds_case, workspace_case)

pytestmark = pytest.mark.gpu

RAGGED = ((0, 1, 45, 300), (300, 45, 1, 0), (45, 0, 300, 1))       # token counts at seq_len = LENS, and two permutations


@pytest.mark.parametrize("case", list(enumerate(SWEEP)), ids=lambda c: "-".join(str(x) for x in c[1]))
def test_varlen_kv8_window_parity_sweep(sfa, case):
    parity_case(sfa, case, True)


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_varlen_kv8_window_binds(sfa, dtype):
    window_binds_case(sfa, dtype, True)


@pytest.mark.parametrize("num_splits", [1, 3])
@pytest.mark.parametrize("layout", ["blmhd", "blhmd", "paged16", "paged64"])
def test_varlen_kv8_window_bit_identical_to_varlen_kv8_where_it_does_not_bind(sfa, layout, num_splits):
    not_binding_case(sfa, layout, num_splits, True)


@pytest.mark.parametrize("num_splits", [1, 3, 4])
@pytest.mark.parametrize("window", EDGE_WINDOWS)
def test_varlen_kv8_window_edges(sfa, window, num_splits):
    edges_case(sfa, window, num_splits, True)


@pytest.mark.parametrize("num_splits", [1, 3])
@pytest.mark.parametrize("layout", ["blmhd", "blhmd", "paged16", "paged64"])
@pytest.mark.parametrize("D", [64, 128])
def test_varlen_kv8_window_reads_nothing_outside_it(sfa, unread_problems, D, layout, num_splits):
    unread_memory_case(sfa, unread_problems[D], UNREAD_WINDOW, layout, num_splits, True)


def test_varlen_kv8_window_distinct_scales_per_head(sfa):
    scales_case(sfa, True)


@pytest.mark.parametrize("num_splits", [1, 3])
def test_varlen_kv8_window_null_scales_equal_ones(sfa, num_splits):
    null_scales_case(sfa, num_splits, True)


@pytest.mark.parametrize("variant", ["softmax_scale", "bias", "tables", "partial_rotary", "partial_rotary_tables", "rot0"])
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_varlen_kv8_window_variants(sfa, variant, dtype):
    variants_case(sfa, variant, dtype, True)


def test_varlen_kv8_window_rejects_like_varlen_kv8(sfa):
    rejection_case(sfa, True)


def test_varlen_kv8_window_bad_table_entry_inside_and_below_the_window(sfa):
    bad_read_page_case(sfa, 3, True)


def test_varlen_kv8_window_workspaces_through_the_c_abi(sfa):
    workspace_case(sfa, True)


# ---- what only the packed call has -----------------------------------------------------------------------------------------

def ragged_problem(dtype, D, G, ns):
    return make_problem(dtype, D, G, LENS, ns, seed=5, k_factors=(0.5, 2.0), tables=True)


@pytest.mark.parametrize("ns", RAGGED, ids=lambda ns: "-".join(str(n) for n in ns))
@pytest.mark.parametrize("case", [("bf16", 128, 1, "paged16", 0, 100), ("fp16", 64, 1, "blmhd", 3, 33),
                                  ("fp16", 128, 4, "blhmd", 1, 17), ("bf16", 64, 8, "paged64", 3, 129),
                                  ("bf16", 128, 2, "blmhd", 1, 1)], ids=lambda c: "-".join(str(x) for x in c))
def test_varlen_kv8_window_ragged_batch(sfa, case, ns):
    """n_b = [0, 1, 45, 300] and the same counts permuted: an idle sequence, a decode step, a verify step and a prompt
    chunk of several q-tiles in one call, each of them at every history length of the frame in turn"""
    dtype, D, G, layout, num_splits, window = case
    p = ragged_problem(dtype, D, G, ns)
    r = run(sfa, p, layout, window, num_splits, varlen=True)
    sfa.check_decode_status()
    check(r, p, window, ref.reference(p, window))
    if r.spare_k is not None:
        assert bool((r.spare_k == ref.FILL).all()) and bool((r.spare_v == ref.FILL).all())


@pytest.mark.parametrize("layout", ["blmhd", "paged16"])
def test_varlen_kv8_window_sequence_without_tokens_is_not_touched(sfa, layout):
    """n_b = 0: nothing of the sequence is read or written and seq_len[b] is not looked at -- its cache rows, the other
    layer and (paged) its whole row of the block_table are poison, its seq_len is out of range, and the call gives the
    bits of the call on benign bytes with no status raised"""
    window = 33
    for ns, idle in ((RAGGED[0], 0), (RAGGED[1], 3)):
        p = ragged_problem("bf16", 128, 4, ns)
        sfa.check_decode_status()
        clean = run(sfa, p, layout, window, 3, varlen=True)
        assert status_word(sfa) == 0
        pk, pv = poisoned(p.k8, p, window), poisoned(p.v8, p, window)
        assert (pk[idle] == 0x7F).all()
        lens = list(LENS)
        lens[idle] = -12345
        ps = ref.page_size(layout)
        r = run(sfa, p, layout, window, 3, varlen=True, k8=pk, v8=pv, lens=lens, fill=0x7F,
                table=poisoned_table(p, window, ps) if ps else None)
        assert status_word(sfa) == 0
        sfa.check_decode_status()
        assert all(torch.equal(a, c) for a, c in zip(r.o, clean.o)) and r.o[idle].shape[0] == 0
        m = append_mask(p)
        assert np.array_equal(r.k8[~m], clean.k8[~m]) and np.array_equal(r.v8[~m], clean.v8[~m])
        assert np.array_equal(r.k8[m], pk[m]) and np.array_equal(r.v8[m], pv[m])


@pytest.mark.parametrize("num_splits", [1, 3])
@pytest.mark.parametrize("window", [1, 17, 100, 5000])
def test_varlen_kv8_window_uniform_lengths_reproduce_chunk_kv8_window(sfa, window, num_splits):
    for dtype, D, G, n, layout in (("bf16", 128, 8, 45, "paged16"), ("fp16", 64, 1, 70, "blhmd")):
        p = problem(dtype, D, G, n)
        c = run(sfa, p, layout, window, num_splits)
        v = run(sfa, p, layout, window, num_splits, varlen=True)
        sfa.check_decode_status()
        assert same_bits(v, c)


@pytest.mark.parametrize("num_splits", [1, 3])
def test_varlen_kv8_window_ragged_bit_identical_to_varlen_kv8_where_it_does_not_bind(sfa, num_splits):
    for dtype, D, G, layout in (("bf16", 128, 4, "paged64"), ("fp16", 64, 1, "blmhd")):
        p = ragged_problem(dtype, D, G, RAGGED[0])
        full = run(sfa, p, layout, None, num_splits, varlen=True)
        r = run(sfa, p, layout, max(pos + n for pos, n in zip(p.lens, p.ns)), num_splits, varlen=True)
        sfa.check_decode_status()
        assert same_bits(r, full)


def test_varlen_kv8_window_bad_cu_tokens_range(sfa):
    """cu_tokens[b+1] < cu_tokens[b], or a range that leaves [0, total_tokens): the sequence is skipped with nothing
    written, o included, SFA_ERR_SEQ_LEN_RANGE is raised, and the other sequences get the bits of the clean call"""
    window = 33
    p = problem("bf16", 128, 4, 5)                              # true cu_tokens = [0, 5, 10, 15, 20]
    sfa.check_decode_status()
    clean = run(sfa, p, "blmhd", window, 3, varlen=True)
    assert status_word(sfa) == 0
    for cu, skipped in (([0, 5, 10, 15, 14], 3), ([0, 5, 10, 15, 25], 3), ([-2, 5, 10, 15, 20], 0)):
        r = run(sfa, p, "blmhd", window, 3, varlen=True, cu=cu)
        assert status_word(sfa) == 1
        with pytest.raises(sfa.SfaError, match="seq_len") as e:
            sfa.check_decode_status()
        assert e.value.status == sfa._lib.SFA_ERR_SEQ_LEN_RANGE
        for b in range(p.B):
            if b == skipped:
                assert bool((r.o[b].view(TDT[p.dtype]) == 7.0).all())       # still the fill value
                np.testing.assert_array_equal(r.k8[b], p.k8[b])
                np.testing.assert_array_equal(r.v8[b], p.v8[b])
            else:
                assert torch.equal(r.o[b], clean.o[b])
                np.testing.assert_array_equal(r.k8[b], clean.k8[b])
                np.testing.assert_array_equal(r.v8[b], clean.v8[b])
    sfa.check_decode_status()


def test_varlen_kv8_window_bad_arguments(sfa):
    p = problem("fp16", 64, 2, 5)
    for w in (0, -3):
        with pytest.raises(sfa.SfaError, match="window") as e:
            run(sfa, p, "blmhd", w, varlen=True)
        assert e.value.status == -2
    dev = torch.device("cuda:0")
    B, H, D, T = 1, 2, 256, 2
    qkv = torch.zeros(T, 3, H, D, dtype=torch.float16, device=dev)
    kc = torch.zeros(B, 1, 64, H, D, dtype=torch.uint8, device=dev)
    o = torch.zeros(T, H, D, dtype=torch.float16, device=dev)
    sl = torch.zeros(B, dtype=torch.int32, device=dev)
    cu = torch.tensor([0, T], dtype=torch.int32, device=dev)
    with pytest.raises(sfa.SfaError) as e:
        sfa.flash_decode_varlen_kv8_window(qkv, None, None, None, kc, kc.clone(), sl, o, cu, B, 64, H, D, 0, 64, 1, 0, 8)
    assert e.value.status == -4


def test_varlen_kv8_window_graph_replay(sfa):
    """One captured flash_decode_varlen_kv8_window call, replayed with two different cu_tokens / seq_len contents under the
    same total_tokens bound: lo and the lengths are read on the device, so both replays are correct."""
    dtype, D, G, window, T = "fp16", 128, 2, 33, 48
    dev = torch.device("cuda:0")
    probs = [make_problem(dtype, D, G, (3, 700, 64, 31), (3, 0, 40, 5), seed=1, tables=True),
             make_problem(dtype, D, G, (1300, 0, 97, 500), (1, 20, 0, 10), seed=2, k_factors=(0.5, 2.0), tables=True)]
    cos, sin = (torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(TDT[dtype]).to(dev)
                for x in ref.rotary_tables(dtype, probs[0].rot))
    p0 = probs[0]
    dt = TDT[dtype]
    t16 = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dt)
    qkv = torch.zeros(T, p0.H + 2 * HKV, D, dtype=dt, device=dev)
    kd = torch.zeros(p0.B, L, M, HKV, D, dtype=torch.uint8, device=dev)
    vd = torch.zeros_like(kd)
    o = torch.zeros(T, p0.H, D, dtype=dt, device=dev)
    sl = torch.zeros(p0.B, dtype=torch.int32, device=dev)
    cu = torch.zeros(p0.B + 1, dtype=torch.int32, device=dev)  # all sequences idle during warm-up and capture
    qb, kb, vb = (torch.zeros(x.shape, dtype=dt, device=dev) for x in p0.biases)
    ks, vs = torch.ones(HKV, device=dev), torch.ones(HKV, device=dev)
    call = lambda: sfa.flash_decode_varlen_kv8_window(qkv, qb, kb, vb, kd, vd, sl, o, cu, p0.B, M, p0.H, D, p0.rot, M, L,
                                                      LAYER, window, num_splits=2, num_heads_kv=HKV, k_scale=ks, v_scale=vs,
                                                      rotary_cos_table=cos, rotary_sin_table=sin)
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
            packed = np.zeros((T, p.H + 2 * HKV, D), np.float32)
            for b, n in enumerate(p.ns):
                packed[cu_h[b]:cu_h[b + 1]] = p.tok[b]
            for dst, src in ((qkv, t16(packed)), (kd, torch.from_numpy(p.k8)), (vd, torch.from_numpy(p.v8)),
                             (qb, t16(p.biases[0])), (kb, t16(p.biases[1])), (vb, t16(p.biases[2])),
                             (ks, torch.from_numpy(p.ks)), (vs, torch.from_numpy(p.vs))):
                dst.copy_(src.to(dev))
            o.fill_(7.0)
            sl.copy_(torch.tensor(list(p.lens), dtype=torch.int32))
            cu.copy_(torch.from_numpy(cu_h))
            graph.replay()
            side.synchronize()
            sfa.check_decode_status(dev)
            ob = bits(o.cpu())
            o_list = [ob[cu_h[b]:cu_h[b + 1]] for b in range(p.B)]
            r = SimpleNamespace(o=o_list, of=[ref.cw.as_float(x, dtype) for x in o_list], k8=kd.cpu().numpy(),
                                v8=vd.cpu().numpy())
            check(r, p, window, ref.reference(p, window))
            assert bool((ob[cu_h[-1]:].view(dt) == 7.0).all())              # rows past cu_tokens[B] are not written
