"""GPU parity of sfa_decode_varlen_kv8 (a ragged, packed batch of new tokens over an fp8 e4m3 KV cache) against the CPU
reference of tests/chunk_kv8_ref.py, checked the way tests/test_decode_chunk_kv8_gpu.py describes: (a) the appended bytes
against the reference quantiser and every other byte against the bytes before, (b) o against attend() over the bytes the
device stored, at the project's decode tolerances."""
import ctypes

import numpy as np
import pytest
import torch

import chunk_kv8_ref as ckr
from chunk_kv8_ref import L, LAYER, M
from oracle import rotary_table_ref, round_to

pytestmark = pytest.mark.gpu

TDT = {"fp16": torch.float16, "bf16": torch.bfloat16}
COUNTS = [0, 1, 70, 5]
LENS = [17, 255, M - 70, 63]                    # the single token takes the last row; sequence 2 ends at M (186 + 70)


@pytest.fixture(scope="module")
def sfa():
    assert torch.cuda.is_available(), "GPU tests need a GPU (run with -m gpu on the MI355X box)"
    import starflashattention_amd as m
    m._lib.load()                  # fail loudly if the HIP library is missing
    return m


@pytest.mark.parametrize("dtype,D,layout,G,splits", [
    ("bf16", 128, "blmhd", 4, 1), ("bf16", 128, "paged16", 4, 3), ("fp16", 64, "blhmd", 1, 3), ("fp16", 64, "paged64", 8, 1),
    ("bf16", 64, "paged16", 16, 3), ("fp16", 128, "blmhd", 8, 0), ("fp16", 128, "blhmd", 16, 1), ("bf16", 128, "paged64", 1, 3),
])
def test_varlen_kv8_mixed_batch(sfa, dtype, D, layout, G, splits):
    """n_b = [0, 1, 70, 5]: a sequence with no tokens, a decode step, a chunk that crosses a 64-key tile and ends at
    memory_max_len (G = 8 / 16: two and five q-tiles), and a short verify"""
    pr = ckr.make_problem(3000 + G, COUNTS, 1 if G == 16 else 2, G, D, dtype)
    lay, ps = ckr.split_layout(layout)
    ckr.check(sfa, pr, LENS, lay, ps, varlen=True, num_splits=splits)


@pytest.mark.parametrize("variant", ["bias_tables", "partial_rotary", "null_scales"])
def test_varlen_kv8_variants(sfa, variant):
    dtype = "bf16"
    pr = ckr.make_problem(3100, COUNTS, 2, 4, 128, dtype, scale_factors=[0.3, 1.7], with_scales=variant != "null_scales")
    rng = np.random.default_rng(3101)
    kw = {}
    if variant == "bias_tables":
        kw["biases"] = [round_to(rng.standard_normal((h, 128)) * 0.5, dtype) for h in (pr["H"], pr["Hkv"], pr["Hkv"])]
        kw["tables"] = rotary_table_ref(M, 128, dtype)
    elif variant == "partial_rotary":
        kw["rot"] = 64
    ckr.check(sfa, pr, LENS, "paged", varlen=True, num_splits=3, **kw)
    ckr.check(sfa, pr, LENS, "blmhd", varlen=True, num_splits=1, **kw)


@pytest.mark.parametrize("layout", ["blmhd", "paged"])
@pytest.mark.parametrize("splits", [1, 3])
def test_varlen_kv8_uniform_counts_reproduce_the_chunk_call(sfa, layout, splits):
    """A uniform cu_tokens gives flash_decode_chunk_kv8's o and cache bytes, bit for bit at the same explicit num_splits"""
    pr = ckr.make_problem(3200, [45] * 3, 2, 4, 128, "bf16")
    lens = [0, 63, 130]
    table, num_pages = ckr.page_table(3, 16) if layout == "paged" else (None, 0)
    a = ckr.run(sfa, pr, lens, pr["k8"], pr["v8"], layout, table=table, num_pages=num_pages, num_splits=splits)
    b = ckr.run(sfa, pr, lens, pr["k8"], pr["v8"], layout, table=table, num_pages=num_pages, num_splits=splits, varlen=True)
    sfa.check_decode_status()
    for x, y in zip(a[0] + [a[1], a[2]], b[0] + [b[1], b[2]]):
        np.testing.assert_array_equal(x, y)
    assert not np.array_equal(a[1], pr["k8"])


@pytest.mark.parametrize("splits", [1, 3])
def test_varlen_kv8_unread_memory(sfa, splits):
    """0x7F in every row at and beyond pos + n_b, in the other layer and the spare pages, -1 in every block_table entry past
    a sequence's last page (all of them for the sequence without tokens)"""
    counts, lens = [0, 1, 70, 5], [17, 100, 131, 63]            # pos + n = 17, 101, 201, 68
    pr = ckr.make_problem(3300, counts, 2, 4, 128, "bf16")
    ckr.poison(pr, lens)
    table = ckr.page_table(4, 16)[0]
    bad = table.clone()
    for b, (pos, n) in enumerate(zip(lens, counts)):
        bad[b, ((pos + n - 1) // 16 + 1 if n else 0):] = -1
    o, *_ = ckr.check(sfa, pr, lens, "paged", varlen=True, num_splits=splits, fill=0x7F, call_table=bad)
    assert all(np.isfinite(x).all() for x in o)
    ckr.check(sfa, pr, lens, "blmhd", varlen=True, num_splits=splits)


def test_varlen_kv8_bad_cu_tokens_range_is_skipped(sfa):
    """A cu_tokens range that exceeds total_tokens: the sequence is skipped, the status raised, nothing of it written;
    the others are served."""
    from starflashattention_amd import ops
    counts, lens = [5, 1, 9], [3, 100, 10]
    pr = ckr.make_problem(3400, counts, 2, 4, 128, "bf16")
    T = sum(counts)
    cu = [0, 5, 6, T + 7]                                       # sequence 2 claims rows past the end of qkv / o
    sfa.check_decode_status()                                   # a cleared status word
    o, k_out, v_out, _ = ckr.run(sfa, pr, lens, pr["k8"], pr["v8"], varlen=True, num_splits=3, cu=cu)
    dev = torch.device("cuda:0")
    ws = ops._workspaces[(dev.index, torch.cuda.current_stream(dev).cuda_stream)]
    assert int(ws[:4].view(torch.int32).item()) == 1
    with pytest.raises(sfa.SfaError, match="seq_len") as e:
        sfa.check_decode_status()
    assert e.value.status == sfa._lib.SFA_ERR_SEQ_LEN_RANGE
    assert np.all(o[2] == 7.0)                                  # skipped: o keeps its fill
    np.testing.assert_array_equal(k_out[2], pr["k8"][2])
    np.testing.assert_array_equal(v_out[2], pr["v8"][2])
    served = dict(pr, counts=[5, 1, 0], tok=pr["tok"][:2] + [pr["tok"][2][:0]])
    ref, k_ref, v_ref = ckr.reference(served, lens)
    ckr.check_bytes(lens, served["counts"], k_out, v_out, pr["k8"], pr["v8"], k_ref, v_ref)
    ckr.check_o(served, lens, o, k_out, v_out, ref)


def test_varlen_kv8_rejection(sfa):
    """pos + n_b > M and an append page outside the pool: NaN rows, both status bits, nothing of the two sequences
    stored; the good sequences correct"""
    from starflashattention_amd import ops
    counts, lens, ps = [5, 20, 4, 33], [3, M - 20 + 1, 100, 50], 16
    pr = ckr.make_problem(3500, counts, 2, 4, 128, "bf16")
    table, num_pages = ckr.page_table(4, ps)
    bad = table.clone()
    bad[3, (50 + 33 - 1) // ps] = num_pages + 1                  # the last append page of sequence 3
    sfa.check_decode_status()
    o, k_out, v_out, _ = ckr.run(sfa, pr, lens, pr["k8"], pr["v8"], "paged", varlen=True, num_splits=3, table=table,
                                 call_table=bad, num_pages=num_pages)
    dev = torch.device("cuda:0")
    ws = ops._workspaces[(dev.index, torch.cuda.current_stream(dev).cuda_stream)]
    assert int(ws[:4].view(torch.int32).item()) == 3
    with pytest.raises(sfa.SfaError) as e:
        sfa.check_decode_status()
    assert e.value.status == sfa._lib.SFA_ERR_BLOCK_TABLE_RANGE  # (the poll reports the block-table bit first)
    for b in (1, 3):
        assert np.isnan(o[b]).all()
        np.testing.assert_array_equal(k_out[b], pr["k8"][b])
        np.testing.assert_array_equal(v_out[b], pr["v8"][b])
    served = dict(pr, counts=[5, 0, 4, 0], tok=[pr["tok"][0], pr["tok"][1][:0], pr["tok"][2], pr["tok"][3][:0]])
    ref, k_ref, v_ref = ckr.reference(served, lens)
    ckr.check_bytes(lens, served["counts"], k_out, v_out, pr["k8"], pr["v8"], k_ref, v_ref)
    ckr.check_o(served, lens, o, k_out, v_out, ref)


def test_varlen_kv8_exact_workspace_through_the_c_abi(sfa):
    """sfa_decode_varlen_kv8 itself at num_splits = 3 with a workspace of exactly sfa_decode_varlen_workspace_bytes bytes,
    every fp32 of it a NaN beforehand: the bits of the operator, nothing written past the end."""
    from exact_workspace import call_with_exact_workspace
    from starflashattention_amd import _lib, ops
    dev = torch.device("cuda:0")
    S = 3
    pr = ckr.make_problem(3600, COUNTS, 2, 4, 128, "bf16")
    want_o, want_k, want_v, _ = ckr.run(sfa, pr, LENS, pr["k8"], pr["v8"], varlen=True, num_splits=S)
    sfa.check_decode_status()
    B, H, Hkv, D, T = 4, pr["H"], pr["Hkv"], 128, sum(COUNTS)
    kd, vd = ckr.to_layout(pr["k8"], "blmhd"), ckr.to_layout(pr["v8"], "blmhd")
    qkv = torch.from_numpy(np.concatenate(pr["tok"])).to(torch.bfloat16).to(dev)
    o = torch.full((T, H, D), 7.0, dtype=torch.bfloat16, device=dev)
    sl = torch.tensor(LENS, dtype=torch.int32, device=dev)
    cu = torch.tensor(np.concatenate([[0], np.cumsum(COUNTS)]), dtype=torch.int32, device=dev)
    ks, vs = torch.from_numpy(pr["ks"]).to(dev), torch.from_numpy(pr["vs"]).to(dev)
    a, *_ = ops._decode_args(qkv, None, None, None, kd, vd, sl, o, B, M, H, D, D, M, L, LAYER, None, None, None, "blmhd",
                             None, Hkv, packed=T, kv8=True)
    lib = _lib.load()
    a.stride = 0
    call_with_exact_workspace(a, lib.sfa_decode_varlen_workspace_bytes(B, H, Hkv, D, M, T, S), S,
                              lambda args, stream: lib.sfa_decode_varlen_kv8(args, ctypes.c_void_p(ks.data_ptr()),
                                                                             ctypes.c_void_p(vs.data_ptr()),
                                                                             ctypes.c_void_p(cu.data_ptr()), T, 0, stream),
                              dev, fill=0xFF)
    np.testing.assert_array_equal(o.float().cpu().numpy(), np.concatenate(want_o))
    np.testing.assert_array_equal(kd.cpu().numpy(), want_k)
    np.testing.assert_array_equal(vd.cpu().numpy(), want_v)
    assert bool(torch.isfinite(o.float()).all())


def test_varlen_kv8_graph_replay(sfa):
    """One flash_decode_varlen_kv8 call captured on a single stream and replayed with two different cu_tokens / seq_len
    contents under the same token total."""
    dev = torch.device("cuda:0")
    dtype, D, G, Hkv, T = "fp16", 128, 2, 2, 40
    H = Hkv * G
    probs = [(ckr.make_problem(3700 + i, counts, Hkv, G, D, dtype), lens)
             for i, (counts, lens) in enumerate((([30, 0, 10], [3, 200, 64]), ([1, 38, 1], [255, 100, 0])))]
    dt = TDT[dtype]
    qkv = torch.zeros(T, H + 2 * Hkv, D, dtype=dt, device=dev)
    kd = torch.zeros(3, L, M, Hkv, D, dtype=torch.uint8, device=dev)
    vd = torch.zeros_like(kd)
    o = torch.zeros(T, H, D, dtype=dt, device=dev)
    sl = torch.zeros(3, dtype=torch.int32, device=dev)
    cu = torch.zeros(4, dtype=torch.int32, device=dev)
    ks, vs = torch.ones(Hkv, device=dev), torch.ones(Hkv, device=dev)
    call = lambda: sfa.flash_decode_varlen_kv8(qkv, None, None, None, kd, vd, sl, o, cu, 3, M, H, D, D, M, L, LAYER,
                                               num_splits=2, num_heads_kv=Hkv, k_scale=ks, v_scale=vs)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        call()                                                  # warm-up: the stream's workspace exists before the capture
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            call()
        for pr, lens in probs:
            true_cu = np.concatenate([[0], np.cumsum(pr["counts"])]).astype(np.int32)
            qkv.copy_(torch.from_numpy(np.concatenate(pr["tok"])).to(dt))
            kd.copy_(torch.from_numpy(pr["k8"]))
            vd.copy_(torch.from_numpy(pr["v8"]))
            ks.copy_(torch.from_numpy(pr["ks"]))
            vs.copy_(torch.from_numpy(pr["vs"]))
            o.fill_(7.0)
            sl.copy_(torch.tensor(lens, dtype=torch.int32))
            cu.copy_(torch.from_numpy(true_cu))
            graph.replay()
            side.synchronize()
            sfa.check_decode_status(dev)
            ref, k_ref, v_ref = ckr.reference(pr, lens)
            k_out, v_out = kd.cpu().numpy(), vd.cpu().numpy()
            of = o.float().cpu().numpy()
            ckr.check_bytes(lens, pr["counts"], k_out, v_out, pr["k8"], pr["v8"], k_ref, v_ref)
            ckr.check_o(pr, lens, [of[true_cu[b]:true_cu[b + 1]] for b in range(3)], k_out, v_out, ref)
