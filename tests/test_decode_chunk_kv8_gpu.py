"""GPU parity of sfa_decode_chunk_kv8 (n new tokens per sequence over an fp8 e4m3 KV cache) against the CPU reference of
tests/chunk_kv8_ref.py.

How o is checked.  On-device sincosf can move a K byte across an e4m3 rounding boundary, and one e4m3
step on a key that carries half the weight of a two-key row is outside the fp16 tolerance.  So every case checks
(a) the appended bytes against the reference quantiser -- V exact, K within one e4m3 step and > 98 % identical per call,
    every other byte of both caches (the other layer and the spare pages included) equal to the bytes before -- and
(b) o against chunk_kv8_ref.attend() over THE BYTES THE DEVICE STORED, with q16 from the reference, at the project's
    decode tolerances unchanged (fp16 2e-3, bf16 1.6e-2, atol = rtol): the output is a function of the cache after the call.

Shapes are those of tests/test_decode_kv8_gpu.py: L = 2, M = 256, LAYER = 1, page size 16 (and 64)."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import chunk_kv8_ref as ckr
import kv8_ref
from chunk_kv8_ref import L, LAYER, M, TOL
from oracle import rope_interleaved, rotary_table_ref, round_to

pytestmark = pytest.mark.gpu

TDT = {"fp16": torch.float16, "bf16": torch.bfloat16}
POS = [0, 63, 130]


@pytest.fixture(scope="module")
def sfa():
    assert torch.cuda.is_available(), "GPU tests need a GPU (run with -m gpu on the MI355X box)"
    import starflashattention_amd as m
    m._lib.load()                  # fail loudly if the HIP library is missing
    return m


def hkv_of(G):
    return 1 if G == 16 else 2


# ---- 1. parity ---------------------------------------------------------------------------------------------------------

FACTORS = (("fp16", "bf16"), (64, 128), ("blmhd", "blhmd", "paged16", "paged64"), (1, 4, 8, 16), (1, 5, 45, 70), (1, 3))


def pairwise_cases(total=40, seed=7):
    """A subset of the full factorial (dtype, D, layout, G, n, splits) that covers every pair of values of every two
    factors: greedy, each step takes the candidate that covers the most pairs still missing; then random further
    cases up to `total`.  G = 8 with n = 45 (360 query rows: two q-tiles) is in by construction."""
    rng = np.random.default_rng(seed)
    every = list(itertools.product(*FACTORS))
    pairs = lambda c: {(i, c[i], j, c[j]) for i in range(len(c)) for j in range(i + 1, len(c))}
    missing = set().union(*(pairs(c) for c in every))
    cases = [("bf16", 128, "paged16", 8, 45, 3)]
    missing -= pairs(cases[0])
    while missing:
        best = max(every, key=lambda c: (len(pairs(c) & missing), -every.index(c)))
        cases.append(best)
        missing -= pairs(best)
    rest = [c for c in every if c not in cases]
    for i in rng.permutation(len(rest))[:max(0, total - len(cases))]:
        cases.append(rest[i])
    return cases


PARITY = pairwise_cases()


def test_parity_cases_cover_every_pair():
    seen = {(i, c[i], j, c[j]) for c in PARITY for i in range(6) for j in range(i + 1, 6)}
    want = {(i, a, j, b) for i in range(6) for j in range(i + 1, 6) for a in FACTORS[i] for b in FACTORS[j]}
    assert seen == want and len(PARITY) == 40 and len(set(PARITY)) == 40
    assert any(c[3] == 8 and c[4] == 45 for c in PARITY) and any(c[4] == 70 for c in PARITY)


@pytest.mark.parametrize("dtype,D,layout,G,n,splits", PARITY)
def test_chunk_kv8_parity(sfa, dtype, D, layout, G, n, splits):
    pr = ckr.make_problem(1000 + PARITY.index((dtype, D, layout, G, n, splits)), [n] * 3, hkv_of(G), G, D, dtype)
    lay, ps = ckr.split_layout(layout)
    ckr.check(sfa, pr, POS, lay, ps, num_splits=splits)


@pytest.mark.parametrize("layout,splits", [("blmhd", 1), ("paged16", 3), ("blhmd", 3), ("paged64", 1)])
def test_chunk_kv8_ends_at_memory_max_len(sfa, layout, splits):
    """pos + n == M for the last sequence (186 + 70), with a 64-key tile boundary inside the chunk"""
    pr = ckr.make_problem(1100, [70] * 3, 2, 4, 128, "bf16")
    lay, ps = ckr.split_layout(layout)
    ckr.check(sfa, pr, [0, 63, M - 70], lay, ps, num_splits=splits)


def test_chunk_kv8_library_split_count_and_float8_tensors(sfa):
    """num_splits = 0 (the library's choice), and torch.float8_e4m3fn caches: the bits of the uint8 call"""
    pr = ckr.make_problem(1101, [5] * 3, 2, 4, 128, "bf16")
    ckr.check(sfa, pr, POS, num_splits=0)
    a = ckr.run(sfa, pr, POS, pr["k8"], pr["v8"], num_splits=2)
    b = ckr.run(sfa, pr, POS, pr["k8"], pr["v8"], num_splits=2, as_fp8=True)
    for x, y in zip(a[0] + [a[1], a[2]], b[0] + [b[1], b[2]]):
        np.testing.assert_array_equal(x, y)


# ---- 2. variants -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", ["bias", "tables", "partial_rotary", "rot0", "softmax_scale"])
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_chunk_kv8_variants(sfa, variant, dtype):
    pr = ckr.make_problem(1200, [5] * 3, 2, 4, 128, dtype)
    rng = np.random.default_rng(1201)
    kw = {}
    if variant == "bias":
        kw["biases"] = [round_to(rng.standard_normal((h, 128)) * 0.5, dtype) for h in (pr["H"], pr["Hkv"], pr["Hkv"])]
    elif variant == "tables":
        kw["tables"] = rotary_table_ref(M, 128, dtype)
    elif variant == "partial_rotary":
        kw.update(rot=64, tables=rotary_table_ref(M, 64, dtype))
        ckr.check(sfa, pr, POS, "paged", num_splits=3, rot=64)      # and the trigonometry on the device
    elif variant == "rot0":
        kw["rot"] = 0
    else:
        kw["softmax_scale"] = 0.05
    ckr.check(sfa, pr, POS, num_splits=1, **kw)
    ckr.check(sfa, pr, POS, "paged", num_splits=3, **kw)


def test_chunk_kv8_distinct_scales_per_head(sfa):
    pr = ckr.make_problem(1210, [45] * 3, 4, 2, 128, "bf16", scale_factors=[0.5, 0.037, 2.0, 1.3])
    assert len(set(pr["ks"].tolist())) == 4 and len(set(pr["vs"].tolist())) == 4
    ckr.check(sfa, pr, POS, num_splits=1)
    ckr.check(sfa, pr, POS, "blhmd", num_splits=3)


@pytest.mark.parametrize("splits", [1, 3])
def test_chunk_kv8_null_scales_equal_ones(sfa, splits):
    pr = ckr.make_problem(1211, [5] * 3, 2, 4, 128, "bf16", with_scales=False)
    ckr.check(sfa, pr, POS, num_splits=splits)
    a = ckr.run(sfa, pr, POS, pr["k8"], pr["v8"], num_splits=splits)
    pr1 = dict(pr, ks=np.ones(2, np.float32), vs=np.ones(2, np.float32))
    b = ckr.run(sfa, pr1, POS, pr["k8"], pr["v8"], num_splits=splits)
    for x, y in zip(a[0] + [a[1], a[2]], b[0] + [b[1], b[2]]):
        np.testing.assert_array_equal(x, y)                     # bit for bit


def test_chunk_kv8_new_tokens_saturate(sfa):
    """|v16 / v_scale| beyond 448 stores the largest finite code, never NaN."""
    pr = ckr.make_problem(1212, [5] * 3, 2, 2, 128, "bf16")
    pr["vs"] = np.array([1e-4, 2e-4], np.float32)               # v ~ N(0,1): |v / scale| > 448 for all but a few
    pr["v8"] = kv8_ref.quantize(np.random.default_rng(1213).standard_normal(pr["v8"].shape).astype(np.float32) * 1e-2, pr["vs"])
    _, _, v_out, _ = ckr.check(sfa, pr, POS, num_splits=1)
    rows = np.stack([v_out[b, LAYER, POS[b]:POS[b] + 5] for b in range(3)])
    assert np.mean((rows == 0x7E) | (rows == 0xFE)) > 0.9 and not np.any((rows & 0x7F) == 0x7F)


# ---- 3. equals n successive flash_decode_kv8 calls -----------------------------------------------------------------------

def successive_kv8(sfa, pr, lens, k8, v8, layout, table, num_pages, tables):
    """n flash_decode_kv8 steps over device caches laid out from k8 / v8; returns (o [B][n, H, D], k8 after, v8 after)"""
    dev = torch.device("cuda:0")
    dt = TDT[pr["dtype"]]
    B, H, Hkv, D, n = pr["B"], pr["H"], pr["Hkv"], pr["D"], pr["counts"][0]
    t16 = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dt).to(dev)
    kd, vd = ckr.to_layout(k8, layout, table, num_pages), ckr.to_layout(v8, layout, table, num_pages)
    kw = dict(kv_layout=layout, num_heads_kv=Hkv, k_scale=torch.from_numpy(pr["ks"]).to(dev),
              v_scale=torch.from_numpy(pr["vs"]).to(dev))
    if layout == "paged":
        kw["block_table"] = table.to(dev)
    if tables is not None:
        kw.update(rotary_cos_table=t16(tables[0]), rotary_sin_table=t16(tables[1]))
    tok = t16(np.stack(pr["tok"]))                              # [B, n, H + 2 Hkv, D]
    out = torch.empty((B, n, H, D), dtype=dt, device=dev)
    for t in range(n):
        o = torch.empty((B, H, D), dtype=dt, device=dev)
        sfa.flash_decode_kv8(tok[:, t].contiguous(), None, None, None, kd, vd,
                             torch.tensor([p + t for p in lens], dtype=torch.int32, device=dev), o, B, M, H, D, D, M, L,
                             LAYER, **kw)
        out[:, t] = o
    torch.cuda.synchronize()
    return list(out.float().cpu().numpy()), ckr.from_layout(kd, layout, B, table), ckr.from_layout(vd, layout, B, table)


@pytest.mark.parametrize("layout", ["blmhd", "paged"])
@pytest.mark.parametrize("with_tables", [True, False])
def test_chunk_kv8_equals_successive_decode_kv8_calls(sfa, layout, with_tables):
    pr = ckr.make_problem(1300, [5] * 3, 2, 4, 128, "bf16")
    table, num_pages = ckr.page_table(3, 16) if layout == "paged" else (None, 0)
    tables = rotary_table_ref(M, 128, "bf16") if with_tables else None
    o1, k1, v1 = successive_kv8(sfa, pr, POS, pr["k8"], pr["v8"], layout, table, num_pages, tables)
    o2, k2, v2, _ = ckr.run(sfa, pr, POS, pr["k8"], pr["v8"], layout, table=table, num_pages=num_pages, tables=tables)
    sfa.check_decode_status()
    np.testing.assert_array_equal(v2, v1)
    if with_tables:
        np.testing.assert_array_equal(k2, k1)                   # the same cos / sin: byte-identical caches
    else:                                                       # in-kernel trigonometry: criterion (a) between the two
        ckr.check_bytes(POS, pr["counts"], k2, v2, pr["k8"], pr["v8"], k1, v1)
    tol = 2 * TOL["bf16"]
    for b in range(3):
        np.testing.assert_allclose(o2[b], o1[b], atol=tol, rtol=tol)


# ---- 4. exact-value cross-check with flash_decode_chunk --------------------------------------------------------------------

@pytest.mark.parametrize("dtype,G,layout,n,splits", [("fp16", 1, "blmhd", 5, 1), ("bf16", 8, "blhmd", 45, 3),
                                                     ("fp16", 4, "paged", 70, 1), ("bf16", 16, "paged", 5, 3)])
def test_chunk_kv8_against_flash_decode_chunk_on_exact_values(sfa, dtype, G, layout, n, splits):
    """Scale 1, no rotation, and cache / new-token values that e4m3 holds exactly (the multiples of 1/8 in [-2, 2]: e4m3's
    spacing is 1/8 only up to 2): both calls see the same numbers."""
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(1400 + G)
    B, Hkv, D = 3, hkv_of(G), 128
    H = Hkv * G
    draw = lambda *s: rng.integers(-16, 17, size=s).astype(np.float32) / 8.0
    kc, vc = draw(B, L, M, Hkv, D), draw(B, L, M, Hkv, D)
    k8, v8 = kv8_ref.quantize(kc), kv8_ref.quantize(vc)
    np.testing.assert_array_equal(kv8_ref.E4M3[k8], kc)
    pr = dict(tok=[draw(n, H + 2 * Hkv, D) for _ in range(B)], k8=k8, v8=v8, ks=None, vs=None, B=B, H=H, Hkv=Hkv, D=D,
              dtype=dtype, counts=[n] * B)
    table, num_pages = ckr.page_table(B, 16) if layout == "paged" else (None, 0)
    o8, k8_out, v8_out, _ = ckr.run(sfa, pr, POS, k8, v8, layout, rot=0, num_splits=splits, table=table, num_pages=num_pages)
    dt = TDT[dtype]
    t16 = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dt).to(dev)
    kc_d, vc_d = t16(kc), t16(vc)                               # blmhd: the layout is not what this test is about
    o16 = torch.empty((B, n, H, D), dtype=dt, device=dev)
    sfa.flash_decode_chunk(t16(np.stack(pr["tok"])).view((B, n, 3, H, D) if G == 1 else (B, n, H + 2 * Hkv, D)), None, None,
                           None, kc_d, vc_d, torch.tensor(POS, dtype=torch.int32, device=dev), o16, B, M, H, D, 0, M, L,
                           LAYER, num_splits=splits, num_heads_kv=Hkv)
    sfa.check_decode_status()
    tol = 2 * TOL[dtype]
    np.testing.assert_allclose(np.stack(o8), o16.float().cpu().numpy(), atol=tol, rtol=tol)
    np.testing.assert_array_equal(kv8_ref.E4M3[k8_out], kc_d.float().cpu().numpy())     # the same cache after the call
    np.testing.assert_array_equal(kv8_ref.E4M3[v8_out], vc_d.float().cpu().numpy())


# ---- 5. prompt, then decode ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", ["blmhd", "paged"])
def test_chunk_kv8_prompt_then_decode_steps(sfa, layout):
    """A flash_decode_chunk_kv8 prompt at pos = 0 (n = 45) into an fp8 cache, then three flash_decode_kv8 steps over it,
    each against the reference over the bytes the device holds."""
    n = 45
    pr = ckr.make_problem(1500, [n] * 2, 2, 4, 128, "bf16")
    table, num_pages = ckr.page_table(2, 16) if layout == "paged" else (None, 0)
    _, k_gpu, v_gpu, _ = ckr.check(sfa, pr, [0, 0], layout, num_splits=0)
    rng = np.random.default_rng(1501)
    dev = torch.device("cuda:0")
    lens = [n, n]
    for step in range(3):
        qkv = round_to(rng.standard_normal((2, pr["H"] + 2 * pr["Hkv"], 128)), "bf16")
        k_ref, v_ref = k_gpu.copy(), v_gpu.copy()
        ref = kv8_ref.decode_kv8_ref(qkv, k_ref, v_ref, lens, LAYER, 128, "bf16", pr["ks"], pr["vs"])
        kd, vd = ckr.to_layout(k_gpu, layout, table, num_pages), ckr.to_layout(v_gpu, layout, table, num_pages)
        o = torch.empty((2, pr["H"], 128), dtype=torch.bfloat16, device=dev)
        kw = dict(block_table=table.to(dev)) if layout == "paged" else {}
        sfa.flash_decode_kv8(torch.from_numpy(qkv).to(torch.bfloat16).to(dev), None, None, None, kd, vd,
                             torch.tensor(lens, dtype=torch.int32, device=dev), o, 2, M, pr["H"], 128, 128, M, L, LAYER,
                             kv_layout=layout, num_heads_kv=pr["Hkv"], k_scale=torch.from_numpy(pr["ks"]).to(dev),
                             v_scale=torch.from_numpy(pr["vs"]).to(dev), **kw)
        sfa.check_decode_status()
        k_new, v_new = ckr.from_layout(kd, layout, 2, table), ckr.from_layout(vd, layout, 2, table)
        ckr.check_bytes(lens, [1, 1], k_new, v_new, k_gpu, v_gpu, k_ref, v_ref)
        # the step's output over the bytes the device stored (its own row included)
        q16 = [np.asarray(round_to(rope_interleaved(qkv[b, :pr["H"]].astype(np.float64), lens[b], 128), "bf16"),
                          np.float64)[None] for b in range(2)]
        for b in range(2):
            want = ckr.attend(q16[b], k_new[b, LAYER], v_new[b, LAYER], lens[b], pr["ks"], pr["vs"])[0]
            np.testing.assert_allclose(o[b].float().cpu().numpy(), want, atol=TOL["bf16"], rtol=TOL["bf16"])
        k_gpu, v_gpu = k_new, v_new
        lens = [x + 1 for x in lens]


# ---- 6. unread memory ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", ["blmhd", "paged"])
@pytest.mark.parametrize("splits", [1, 3])
@pytest.mark.parametrize("D,dtype", [(128, "bf16"), (64, "fp16")])
def test_chunk_kv8_unread_memory(sfa, layout, splits, D, dtype):
    """NaN bytes in everything the call may not read, pos + n no multiple of 16: a masked key has weight 0, but 0 x NaN is
    NaN in P V, so the ragged last tile must re-address its rows instead of only masking them."""
    n, lens = 5, [0, 63, 130]                                   # pos + n = 5, 68, 135
    pr = ckr.make_problem(1600, [n] * 3, 2, 4, D, dtype)
    ckr.poison(pr, lens)
    kw = {}
    if layout == "paged":
        kw["call_table"] = ckr.poisoned_table(ckr.page_table(3, 16)[0], lens, pr["counts"], 16)
        assert int((kw["call_table"] == -1).sum()) > 20
    o, *_ = ckr.check(sfa, pr, lens, layout, num_splits=splits, fill=0x7F, **kw)
    assert all(np.isfinite(x).all() for x in o)


# ---- 7. rejection: the library's handled paths ---------------------------------------------------------------------------------

def status_word(sfa):
    from starflashattention_amd import ops
    dev = torch.device("cuda:0")
    ws = ops._workspaces[(dev.index, torch.cuda.current_stream(dev).cuda_stream)]
    torch.cuda.synchronize()
    return int(ws[:4].view(torch.int32).item())


@pytest.mark.parametrize("splits", [1, 3])
def test_chunk_kv8_rejects_rows_beyond_memory_max_len(sfa, splits):
    n = 5
    pr = ckr.make_problem(1700, [n] * 3, 2, 4, 128, "bf16")
    sfa.check_decode_status()                                   # a cleared status word
    good, *_ = ckr.run(sfa, pr, [40, 41, 129], pr["k8"], pr["v8"], num_splits=splits)
    assert status_word(sfa) == 0
    lens = [40, M - n + 1, 129]
    o, k_out, v_out, _ = ckr.run(sfa, pr, lens, pr["k8"], pr["v8"], num_splits=splits)
    assert status_word(sfa) == 1
    with pytest.raises(sfa.SfaError, match="seq_len") as e:
        sfa.check_decode_status()
    assert e.value.status == sfa._lib.SFA_ERR_SEQ_LEN_RANGE
    assert np.isnan(o[1]).all()
    for b in (0, 2):
        np.testing.assert_array_equal(o[b], good[b])            # the other sequences: the bits of the clean run
    np.testing.assert_array_equal(k_out[1], pr["k8"][1])        # nothing of the rejected sequence was stored
    np.testing.assert_array_equal(v_out[1], pr["v8"][1])
    sfa.check_decode_status()                                   # the flag was cleared by the raise


@pytest.mark.parametrize("splits", [1, 3])
def test_chunk_kv8_rejects_bad_pages(sfa, splits):
    n, lens, ps = 5, [40, 44, 129], 16                          # sequence 1 appends rows 44 .. 48: pages 2 and 3
    pr = ckr.make_problem(1701, [n] * 3, 2, 4, 128, "bf16")
    table, num_pages = ckr.page_table(3, ps)
    sfa.check_decode_status()
    good, kg, vg, _ = ckr.run(sfa, pr, lens, pr["k8"], pr["v8"], "paged", table=table, num_pages=num_pages, num_splits=splits)
    assert status_word(sfa) == 0
    # an append page outside the pool: the sequence is rejected, nothing of it stored anywhere in the pools
    bad = table.clone()
    bad[1, 48 // ps] = num_pages
    o, _, _, raw = ckr.run(sfa, pr, lens, pr["k8"], pr["v8"], "paged", table=table, call_table=bad, num_pages=num_pages,
                           num_splits=splits)
    assert status_word(sfa) == 2
    with pytest.raises(sfa.SfaError, match="block_table") as e:
        sfa.check_decode_status()
    assert e.value.status == sfa._lib.SFA_ERR_BLOCK_TABLE_RANGE
    assert np.isnan(o[1]).all()
    want_k, want_v = pr["k8"].copy(), pr["v8"].copy()
    for b in (0, 2):
        np.testing.assert_array_equal(o[b], good[b])
        rows = slice(lens[b], lens[b] + n)
        want_k[b, LAYER, rows], want_v[b, LAYER, rows] = kg[b, LAYER, rows], vg[b, LAYER, rows]
    assert torch.equal(raw[0].cpu(), ckr.to_layout(want_k, "paged", table, num_pages).cpu())
    assert torch.equal(raw[1].cpu(), ckr.to_layout(want_v, "paged", table, num_pages).cpu())
    # a bad page that is only read: reported, never dereferenced, that sequence's outputs NaN; its rows are appended,
    # as the 16-bit call appends them
    bad = table.clone()
    bad[2, 0] = -5
    o, k_out, v_out, _ = ckr.run(sfa, pr, lens, pr["k8"], pr["v8"], "paged", table=table, call_table=bad,
                                 num_pages=num_pages, num_splits=splits)
    assert status_word(sfa) == 2
    with pytest.raises(sfa.SfaError, match="block_table"):
        sfa.check_decode_status()
    assert np.isnan(o[2]).all() and not np.isnan(np.stack([o[0], o[1]])).any()
    for b in (0, 1):
        np.testing.assert_array_equal(o[b], good[b])
    np.testing.assert_array_equal(k_out, kg)
    np.testing.assert_array_equal(v_out, vg)
    sfa.check_decode_status()


# ---- 9. exact workspace through the C ABI ------------------------------------------------------------------------------------

def test_chunk_kv8_exact_workspace_through_the_c_abi(sfa):
    """sfa_decode_chunk_kv8 itself at num_splits = 3 with a workspace of exactly sfa_decode_chunk_workspace_bytes bytes,
    every fp32 of it a NaN beforehand: the bits of the operator, nothing written past the end."""
    from exact_workspace import call_with_exact_workspace
    from starflashattention_amd import _lib, ops
    dev = torch.device("cuda:0")
    n, S = 45, 3
    pr = ckr.make_problem(1900, [n] * 3, 2, 4, 128, "bf16")
    want_o, want_k, want_v, _ = ckr.run(sfa, pr, POS, pr["k8"], pr["v8"], num_splits=S)
    sfa.check_decode_status()
    B, H, Hkv, D = 3, pr["H"], pr["Hkv"], 128
    kd, vd = ckr.to_layout(pr["k8"], "blmhd"), ckr.to_layout(pr["v8"], "blmhd")
    qkv = torch.from_numpy(np.stack(pr["tok"])).to(torch.bfloat16).to(dev)
    o = torch.full((B, n, H, D), 7.0, dtype=torch.bfloat16, device=dev)
    sl = torch.tensor(POS, dtype=torch.int32, device=dev)
    ks, vs = torch.from_numpy(pr["ks"]).to(dev), torch.from_numpy(pr["vs"]).to(dev)
    a, *_ = ops._decode_args(qkv, None, None, None, kd, vd, sl, o, B, M, H, D, D, M, L, LAYER, None, None, None, "blmhd",
                             None, Hkv, tokens=n, kv8=True)
    lib = _lib.load()
    a.stride = 0
    call_with_exact_workspace(a, lib.sfa_decode_chunk_workspace_bytes(B, H, Hkv, D, M, n, S), S,
                              lambda args, stream: lib.sfa_decode_chunk_kv8(args, ctypes.c_void_p(ks.data_ptr()),
                                                                            ctypes.c_void_p(vs.data_ptr()), n, 0, stream),
                              dev, fill=0xFF)
    np.testing.assert_array_equal(o.float().cpu().numpy(), np.stack(want_o))
    np.testing.assert_array_equal(kd.cpu().numpy(), want_k)
    np.testing.assert_array_equal(vd.cpu().numpy(), want_v)
    assert bool(torch.isfinite(o.float()).all())


# ---- 10. graph replay ------------------------------------------------------------------------------------------------------------

def test_chunk_kv8_graph_replay(sfa):
    """One flash_decode_chunk_kv8 call captured on a single stream and replayed with two different seq_len (and tensor)
    contents: everything the kernels need is read on the device, so both replays are correct."""
    dev = torch.device("cuda:0")
    dtype, D, G, n, Hkv = "fp16", 128, 2, 40, 2
    H = Hkv * G
    probs = [(ckr.make_problem(2000 + i, [n] * 3, Hkv, G, D, dtype), lens) for i, lens in enumerate(([3, 200, 64], [130, 0, 97]))]
    dt = TDT[dtype]
    qkv = torch.zeros(3, n, H + 2 * Hkv, D, dtype=dt, device=dev)
    kd = torch.zeros(3, L, M, Hkv, D, dtype=torch.uint8, device=dev)
    vd = torch.zeros_like(kd)
    o = torch.zeros(3, n, H, D, dtype=dt, device=dev)
    sl = torch.zeros(3, dtype=torch.int32, device=dev)
    ks, vs = torch.ones(Hkv, device=dev), torch.ones(Hkv, device=dev)
    call = lambda: sfa.flash_decode_chunk_kv8(qkv, None, None, None, kd, vd, sl, o, 3, M, H, D, D, M, L, LAYER,
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
            qkv.copy_(torch.from_numpy(np.stack(pr["tok"])).to(dt))
            kd.copy_(torch.from_numpy(pr["k8"]))
            vd.copy_(torch.from_numpy(pr["v8"]))
            ks.copy_(torch.from_numpy(pr["ks"]))
            vs.copy_(torch.from_numpy(pr["vs"]))
            o.fill_(7.0)
            sl.copy_(torch.tensor(lens, dtype=torch.int32))
            graph.replay()
            side.synchronize()
            sfa.check_decode_status(dev)
            ref, k_ref, v_ref = ckr.reference(pr, lens)
            k_out, v_out = kd.cpu().numpy(), vd.cpu().numpy()
            ckr.check_bytes(lens, pr["counts"], k_out, v_out, pr["k8"], pr["v8"], k_ref, v_ref)
            ckr.check_o(pr, lens, list(o.float().cpu().numpy()), k_out, v_out, ref)
