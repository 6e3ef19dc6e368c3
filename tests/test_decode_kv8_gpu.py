"""GPU parity of sfa_decode_kv8 (decode attention over an fp8 e4m3 KV cache) and sfa_kv8_quantize against the CPU
reference of tests/kv8_ref.py.

Tolerances: the project's decode tolerances (tests/test_decode_gpu.py: kernel vs fp64 reference on identical inputs,
fp16 atol = rtol = 2e-3, bf16 1.6e-2).  They carry over because the reference sees the identical dequantised cache: the
quantisation error is in both.  The appended V bytes are exact; the appended K bytes follow the 16-bit criterion carried
over (on-device sincosf can move a 16-bit value by one ulp, which rarely crosses an e4m3 rounding boundary): every
element within one e4m3 step, more than 98 % of the bytes identical.

Shapes: M = 256 rows, two layers (idx_layer = 1), lengths on the 32-key tile, wave-share and split edges and the last row.
"""
import numpy as np
import pytest
import torch

import kv8_ref
from oracle import rotary_table_ref, round_to

pytestmark = pytest.mark.gpu

TOL = {"fp16": 2e-3, "bf16": 1.6e-2}
TDT = {"fp16": torch.float16, "bf16": torch.bfloat16}
L, M, LAYER, PS = 2, 256, 1, 16


@pytest.fixture(scope="module")
def sfa():
    assert torch.cuda.is_available(), "GPU tests need a GPU (run with -m gpu on the MI355X box)"
    import starflashattention_amd as m
    m._lib.load()                  # fail loudly if the HIP library is missing
    return m


def amax_scale(x):
    """amax / 448 per kv head of x [B, L, M, Hkv, D]"""
    return (np.abs(x).max(axis=(0, 1, 2, 4)) / 448.0).astype(np.float32)


def make_problem(seed, B, Hkv, G, D, dtype, scale_factors=None, with_scales=True):
    """N(0,1) caches quantised with scale = factor * amax / 448 per kv head, and an N(0,1) qkv row rounded to dtype."""
    rng = np.random.default_rng(seed)
    H = Hkv * G
    kc = rng.standard_normal((B, L, M, Hkv, D)).astype(np.float32)
    vc = rng.standard_normal((B, L, M, Hkv, D)).astype(np.float32)
    ks = vs = None
    if with_scales:
        f = np.ones(Hkv, np.float32) if scale_factors is None else np.asarray(scale_factors, np.float32)
        ks, vs = amax_scale(kc) * f, amax_scale(vc) * f[::-1]
    qkv = round_to(rng.standard_normal((B, H + 2 * Hkv, D)), dtype)
    return dict(qkv=qkv, k8=kv8_ref.quantize(kc, ks), v8=kv8_ref.quantize(vc, vs), ks=ks, vs=vs, B=B, H=H, Hkv=Hkv,
                D=D, dtype=dtype)


def page_table(B, seed=3):
    """a shuffled block table over a pool with a few pages to spare"""
    pps = M // PS
    num_pages = B * pps + 3
    g = torch.Generator().manual_seed(seed)
    return torch.randperm(num_pages, generator=g)[:B * pps].to(torch.int32).view(B, pps), num_pages


def to_layout(c, layout, table=None, num_pages=0):
    """canonical uint8 [B, L, M, Hkv, D] (numpy) -> the device tensor of `layout`"""
    t = torch.from_numpy(np.ascontiguousarray(c))
    if layout == "blhmd":
        t = t.permute(0, 1, 3, 2, 4).contiguous()
    elif layout == "paged":
        B, _, _, Hkv, D = c.shape
        pool = torch.full((num_pages, L, PS, Hkv, D), 0x33, dtype=torch.uint8)
        pool[table.long().view(-1)] = t.view(B, L, M // PS, PS, Hkv, D).permute(0, 2, 1, 3, 4, 5).reshape(-1, L, PS, Hkv, D)
        t = pool
    return t.cuda()


def from_layout(t, layout, B, table=None):
    t = t.cpu()
    if layout == "blhmd":
        t = t.permute(0, 1, 3, 2, 4)
    elif layout == "paged":
        Hkv, D = t.shape[3], t.shape[4]
        t = t[table.long().view(-1)].view(B, M // PS, L, PS, Hkv, D).permute(0, 2, 1, 3, 4, 5).reshape(B, L, M, Hkv, D)
    return t.contiguous().numpy()


def run_kv8(sfa, pr, lens, k8, v8, layout="blmhd", num_splits=0, rot=None, biases=None, tables=None, table=None,
            num_pages=0, as_fp8=False, call_table=None):
    """One flash_decode_kv8 call on canonical numpy caches; returns (o fp32, k8 after, v8 after, raw device caches).
    Paged: `table` lays the pools out and reads them back; the call gets call_table when given (a damaged copy)."""
    dev = torch.device("cuda:0")
    dt = TDT[pr["dtype"]]
    B, H, Hkv, D = pr["B"], pr["H"], pr["Hkv"], pr["D"]
    t16 = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dt).to(dev)
    kd, vd = to_layout(k8, layout, table, num_pages), to_layout(v8, layout, table, num_pages)
    if as_fp8:
        kd, vd = kd.view(torch.float8_e4m3fn), vd.view(torch.float8_e4m3fn)
    o = torch.full((B, H, D), 7.0, dtype=dt, device=dev)
    kw = dict(num_splits=num_splits, kv_layout=layout, num_heads_kv=Hkv)
    if layout == "paged":
        kw["block_table"] = (table if call_table is None else call_table).to(dev)
    if tables is not None:
        kw.update(rotary_cos_table=t16(tables[0]), rotary_sin_table=t16(tables[1]))
    if pr["ks"] is not None:
        kw.update(k_scale=torch.from_numpy(pr["ks"]).to(dev), v_scale=torch.from_numpy(pr["vs"]).to(dev))
    bq, bk, bv = (None, None, None) if biases is None else (t16(x) for x in biases)
    qkv = t16(pr["qkv"]).view((B, 3, H, D) if Hkv == H else (B, H + 2 * Hkv, D))   # one query head per kv head: [B, 3, H, D]
    ret = sfa.flash_decode_kv8(qkv, bq, bk, bv, kd, vd, torch.tensor(list(lens), dtype=torch.int32, device=dev),
                               o, B, M, H, D, D if rot is None else rot, M, L, LAYER, **kw)
    assert ret.data_ptr() == o.data_ptr()
    torch.cuda.synchronize()
    kd, vd = kd.view(torch.uint8), vd.view(torch.uint8)
    return o.float().cpu().numpy(), from_layout(kd, layout, B, table), from_layout(vd, layout, B, table), (kd, vd)


def check_bytes(lens, k_out, v_out, k_before, v_before, ref):
    """The appended rows against the reference's (V exact; K within one e4m3 step, > 98 % identical) and every other
    byte of both caches against the caches before the step."""
    B = len(lens)
    for b in range(B):
        np.testing.assert_array_equal(v_out[b, LAYER, lens[b]], ref["v_row"][b])                # exact
        got, want = kv8_ref.E4M3[k_out[b, LAYER, lens[b]]], kv8_ref.E4M3[ref["k_row"][b]]
        assert np.all(np.abs(got - want) <= kv8_ref.step_at(np.maximum(np.abs(got), np.abs(want)))), (b, got, want)
        assert np.mean(k_out[b, LAYER, lens[b]] == ref["k_row"][b]) > 0.98
    mask = np.ones(k_before.shape[:3], bool)
    for b in range(B):
        mask[b, LAYER, lens[b]] = False
    np.testing.assert_array_equal(k_out[mask], k_before[mask])
    np.testing.assert_array_equal(v_out[mask], v_before[mask])


def check(sfa, pr, lens, layout="blmhd", **kw):
    """Parity of o, the appended bytes, and every other byte of both caches (the other layer and, paged, the pages no
    sequence owns included)."""
    table = num_pages = None
    if layout == "paged":
        table, num_pages = page_table(pr["B"])
    k_ref, v_ref = pr["k8"].copy(), pr["v8"].copy()
    okw = {}
    if kw.get("biases") is not None:
        okw = dict(q_bias=kw["biases"][0], k_bias=kw["biases"][1], v_bias=kw["biases"][2])
    if kw.get("tables") is not None:
        okw.update(cos_table=kw["tables"][0], sin_table=kw["tables"][1])
    rot = pr["D"] if kw.get("rot") is None else kw["rot"]
    ref = kv8_ref.decode_kv8_ref(pr["qkv"], k_ref, v_ref, lens, LAYER, rot, pr["dtype"], pr["ks"], pr["vs"], **okw)
    o, k_out, v_out, raw = run_kv8(sfa, pr, lens, pr["k8"], pr["v8"], layout, table=table, num_pages=num_pages, **kw)
    sfa.check_decode_status()
    tol = TOL[pr["dtype"]]
    np.testing.assert_allclose(o, ref["o"], atol=tol, rtol=tol)
    check_bytes(lens, k_out, v_out, pr["k8"], pr["v8"], ref)
    if layout == "paged":           # the spare pages of the pool
        spare = torch.from_numpy(np.setdiff1d(np.arange(num_pages), table.numpy().ravel())).to(raw[0].device)
        assert bool((raw[0][spare] == 0x33).all()) and bool((raw[1][spare] == 0x33).all())
    return o, ref


# ---- 1. parity of o (and 2. the appended bytes and the untouched rest, in every case) ----

@pytest.mark.parametrize("G", [1, 2, 4, 8, 16])
def test_kv8_group_sizes(sfa, G):
    pr = make_problem(10 + G, 3, 1 if G == 16 else 2, G, 128, "bf16")
    check(sfa, pr, [129, 33, 255])
    check(sfa, pr, [0, 128, 31])


@pytest.mark.parametrize("layout", ["blmhd", "blhmd", "paged"])
@pytest.mark.parametrize("G", [1, 8])
def test_kv8_layouts(sfa, layout, G):
    pr = make_problem(30 + G, 3, 2, G, 128, "bf16")
    for lens in ([1, 127, 32], [255, 0, 129], [33, 128, 31]):
        check(sfa, pr, lens, layout)


@pytest.mark.parametrize("layout", ["blmhd", "paged"])
@pytest.mark.parametrize("G", [1, 4])
def test_kv8_fp16_head_dim_64(sfa, layout, G):
    pr = make_problem(50 + G, 3, 3, G, 64, "fp16")
    for lens in ([1, 127, 32], [255, 0, 129], [33, 128, 31]):
        check(sfa, pr, lens, layout)


@pytest.mark.parametrize("num_splits", [0, 1, 3, 4])
@pytest.mark.parametrize("layout", ["blmhd", "paged"])
def test_kv8_num_splits(sfa, num_splits, layout):
    pr = make_problem(60, 2, 2, 4, 128, "bf16")
    check(sfa, pr, [129, 129], layout, num_splits=num_splits)
    check(sfa, pr, [2, 255], layout, num_splits=num_splits)     # splits with no keys at all


@pytest.mark.parametrize("nt", [0, 1])
def test_kv8_non_temporal_loads(sfa, nt):
    pr = make_problem(61, 2, 2, 2, 128, "fp16")
    sfa.debug_set("decode_nt", nt)
    try:
        check(sfa, pr, [129, 32], num_splits=2)
    finally:
        sfa.debug_set("decode_nt", -1)


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_kv8_bias_rotary_tables_partial_rotary(sfa, dtype):
    pr = make_problem(62, 2, 2, 4, 128, dtype)
    rng = np.random.default_rng(63)
    rot = 64
    biases = [round_to(rng.standard_normal((h, 128)) * 0.5, dtype) for h in (pr["H"], pr["Hkv"], pr["Hkv"])]
    check(sfa, pr, [129, 33], rot=rot, biases=biases, tables=rotary_table_ref(M, rot, dtype))
    check(sfa, pr, [129, 33], rot=rot, biases=biases)           # partial rotary, trigonometry on the device


def test_kv8_accepts_float8_tensors(sfa):
    pr = make_problem(64, 2, 2, 2, 128, "bf16")
    a = run_kv8(sfa, pr, [40, 129], pr["k8"], pr["v8"])
    b = run_kv8(sfa, pr, [40, 129], pr["k8"], pr["v8"], as_fp8=True)
    for x, y in zip(a[:3], b[:3]):
        np.testing.assert_array_equal(x, y)


# ---- 3. scales ----

def test_kv8_distinct_scales_per_head(sfa):
    pr = make_problem(70, 2, 4, 2, 128, "bf16", scale_factors=[0.5, 0.037, 2.0, 1.3])
    assert len(set(pr["ks"].tolist())) == 4
    check(sfa, pr, [129, 255])
    check(sfa, pr, [129, 255], "blhmd", num_splits=3)


def test_kv8_null_scales_equal_ones(sfa):
    pr = make_problem(71, 2, 2, 4, 128, "bf16", with_scales=False)
    lens = [129, 31]
    check(sfa, pr, lens)
    a = run_kv8(sfa, pr, lens, pr["k8"], pr["v8"], num_splits=2)
    pr1 = dict(pr, ks=np.ones(2, np.float32), vs=np.ones(2, np.float32))
    b = run_kv8(sfa, pr1, lens, pr["k8"], pr["v8"], num_splits=2)
    for x, y in zip(a[:3], b[:3]):
        np.testing.assert_array_equal(x, y)                     # bit for bit


def test_kv8_new_token_saturates(sfa):
    """|v16 / v_scale| beyond 448 stores the largest finite code, not NaN."""
    pr = make_problem(72, 2, 2, 2, 128, "bf16")
    pr["vs"] = np.array([1e-4, 2e-4], np.float32)               # v ~ N(0,1): |v / scale| > 448 for all but a few
    pr["v8"] = kv8_ref.quantize(np.random.default_rng(73).standard_normal(pr["v8"].shape).astype(np.float32) * 1e-2, pr["vs"])
    lens = [33, 129]
    _, ref = check(sfa, pr, lens)
    rows = ref["v_row"]
    assert np.mean((rows == 0x7E) | (rows == 0xFE)) > 0.9 and not np.any((rows & 0x7F) == 0x7F)


# ---- 4. successive steps read the appended rows back ----

@pytest.mark.parametrize("layout", ["blmhd", "paged"])
def test_kv8_three_successive_steps(sfa, layout):
    pr = make_problem(80, 2, 2, 4, 128, "bf16")
    table, num_pages = page_table(pr["B"]) if layout == "paged" else (None, 0)
    rng = np.random.default_rng(81)
    k_ref, v_ref = pr["k8"].copy(), pr["v8"].copy()
    k_gpu, v_gpu = pr["k8"].copy(), pr["v8"].copy()
    lens = [31, 126]
    for step in range(3):
        pr["qkv"] = round_to(rng.standard_normal(pr["qkv"].shape), "bf16")
        ref = kv8_ref.decode_kv8_ref(pr["qkv"], k_ref, v_ref, lens, LAYER, 128, "bf16", pr["ks"], pr["vs"])
        k_before, v_before = k_gpu, v_gpu
        o, k_gpu, v_gpu, _ = run_kv8(sfa, pr, lens, k_gpu, v_gpu, layout, table=table, num_pages=num_pages)
        np.testing.assert_allclose(o, ref["o"], atol=TOL["bf16"], rtol=TOL["bf16"])
        check_bytes(lens, k_gpu, v_gpu, k_before, v_before, ref)
        k_ref = k_gpu.copy()        # the next step of the reference reads the bytes the device stored
        lens = [n + 1 for n in lens]
    sfa.check_decode_status()


# ---- 5. cross-check with sfa_decode on the 16-bit copy of the same cache ----

@pytest.mark.parametrize("dtype,G,layout", [("fp16", 1, "blmhd"), ("bf16", 1, "blhmd"), ("bf16", 8, "blmhd"), ("fp16", 4, "paged")])
def test_kv8_against_sfa_decode_on_exact_values(sfa, dtype, G, layout):
    """Scale 1, no rotation, and cache / new-token values that e4m3 holds exactly: both calls see the same numbers.
    The values are the multiples of 1/8 in [-2, 2]: e4m3's spacing is 1/8 only up to 2 (1/4 from 2 to 4), so the
    multiples of 1/8 beyond 2 would not be exact."""
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(90 + G)
    B, Hkv, D = 3, 2, 128
    H = Hkv * G
    draw = lambda *s: rng.integers(-16, 17, size=s).astype(np.float32) / 8.0
    kc, vc, qkv = draw(B, L, M, Hkv, D), draw(B, L, M, Hkv, D), draw(B, H + 2 * Hkv, D)
    k8, v8 = kv8_ref.quantize(kc), kv8_ref.quantize(vc)
    np.testing.assert_array_equal(kv8_ref.E4M3[k8], kc)
    pr = dict(qkv=qkv, k8=k8, v8=v8, ks=None, vs=None, B=B, H=H, Hkv=Hkv, D=D, dtype=dtype)
    lens = [129, 32, 255]
    table, num_pages = page_table(B) if layout == "paged" else (None, 0)
    o8, k8_out, v8_out, _ = run_kv8(sfa, pr, lens, k8, v8, layout, rot=0, table=table, num_pages=num_pages)
    dt = TDT[dtype]
    t16 = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dt).to(dev)
    kc_d, vc_d = t16(kc), t16(vc)
    o16 = torch.empty((B, H, D), dtype=dt, device=dev)
    sfa.flash_decode(t16(qkv).view((B, 3, H, D) if G == 1 else (B, H + 2 * Hkv, D)), None, None, None, kc_d, vc_d, torch.tensor(lens, dtype=torch.int32, device=dev), o16,
                     B, M, H, D, 0, M, L, LAYER, num_heads_kv=Hkv)
    sfa.check_decode_status()
    np.testing.assert_allclose(o8, o16.float().cpu().numpy(), atol=2 * TOL[dtype], rtol=2 * TOL[dtype])
    np.testing.assert_array_equal(kv8_ref.E4M3[k8_out], kc_d.float().cpu().numpy())     # the same cache after the step
    np.testing.assert_array_equal(kv8_ref.E4M3[v8_out], vc_d.float().cpu().numpy())


# ---- 6. rejection: the library's handled paths ----

@pytest.mark.parametrize("num_splits", [1, 2])
def test_kv8_rejects_seq_len_out_of_range(sfa, num_splits):
    pr = make_problem(100, 3, 2, 4, 128, "bf16")
    sfa.check_decode_status()                                   # clean slate
    good, _, _, _ = run_kv8(sfa, pr, [40, 41, 129], pr["k8"], pr["v8"], num_splits=num_splits)
    o, k_out, v_out, _ = run_kv8(sfa, pr, [40, M, 129], pr["k8"], pr["v8"], num_splits=num_splits)
    with pytest.raises(sfa.SfaError, match="seq_len") as e:
        sfa.check_decode_status()
    assert e.value.status == sfa._lib.SFA_ERR_SEQ_LEN_RANGE
    assert np.isnan(o[1]).all()
    np.testing.assert_array_equal(o[[0, 2]], good[[0, 2]])      # the other sequences: the bits of the clean run
    ref = kv8_ref.decode_kv8_ref(pr["qkv"][[0, 2]], pr["k8"][[0, 2]].copy(), pr["v8"][[0, 2]].copy(), [40, 129], LAYER,
                                 128, "bf16", pr["ks"], pr["vs"])
    np.testing.assert_allclose(o[[0, 2]], ref["o"], atol=TOL["bf16"], rtol=TOL["bf16"])
    np.testing.assert_array_equal(k_out[1], pr["k8"][1])
    np.testing.assert_array_equal(v_out[1], pr["v8"][1])
    sfa.check_decode_status()                                   # the flag was cleared by the raise


def test_kv8_rejects_append_page_outside_the_pool(sfa):
    pr = make_problem(101, 3, 2, 4, 128, "bf16")
    table, num_pages = page_table(pr["B"])
    lens = [40, 41, 129]
    sfa.check_decode_status()
    good, kg, vg, _ = run_kv8(sfa, pr, lens, pr["k8"], pr["v8"], "paged", table=table, num_pages=num_pages)
    bad = table.clone()
    bad[1, lens[1] // PS] = num_pages
    o, _, _, raw = run_kv8(sfa, pr, lens, pr["k8"], pr["v8"], "paged", table=table, call_table=bad, num_pages=num_pages)
    with pytest.raises(sfa.SfaError, match="block_table") as e:
        sfa.check_decode_status()
    assert e.value.status == sfa._lib.SFA_ERR_BLOCK_TABLE_RANGE
    assert np.isnan(o[1]).all()
    np.testing.assert_array_equal(o[[0, 2]], good[[0, 2]])
    # nothing of sequence 1 was stored anywhere: the pools hold the original bytes plus the two healthy appends
    want_k, want_v = pr["k8"].copy(), pr["v8"].copy()
    for b in (0, 2):
        want_k[b, LAYER, lens[b]], want_v[b, LAYER, lens[b]] = kg[b, LAYER, lens[b]], vg[b, LAYER, lens[b]]
    assert torch.equal(raw[0].cpu(), to_layout(want_k, "paged", table, num_pages).cpu())
    assert torch.equal(raw[1].cpu(), to_layout(want_v, "paged", table, num_pages).cpu())
    # a bad page that is only read: reported, never dereferenced, that sequence's output NaN
    bad = table.clone()
    bad[2, 0] = num_pages + 5
    o, k_out, v_out, _ = run_kv8(sfa, pr, lens, pr["k8"], pr["v8"], "paged", table=table, call_table=bad, num_pages=num_pages)
    with pytest.raises(sfa.SfaError, match="block_table"):
        sfa.check_decode_status()
    assert np.isnan(o[2]).all() and not np.isnan(o[[0, 1]]).any()
    np.testing.assert_array_equal(o[[0, 1]], good[[0, 1]])
    sfa.check_decode_status()


# ---- 7. quantize_kv8 ----

@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("with_scale", [True, False])
def test_quantize_kv8(sfa, dtype, with_scale):
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(110)
    B, Hkv, D, rows = 2, 3, 128, 77
    x = round_to(rng.standard_normal((B, L, M, Hkv, D)) * 3.0, dtype)
    scale = amax_scale(x) * np.array([1.0, 0.3, 2.0], np.float32) if with_scale else None
    x[1, LAYER, 5, 1, 7] = np.nan
    x[1, LAYER, 6, 2, :4] = [10000.0, -10000.0, np.inf, -np.inf]   # beyond +-448 * scale: saturate
    sc_d = torch.from_numpy(scale).to(dev) if with_scale else None
    src = torch.from_numpy(x).to(TDT[dtype]).to(dev)
    want = kv8_ref.quantize(x[1, LAYER, :rows], scale)
    assert want[5, 1, 7] == 0x7F and list(want[6, 2, :4]) == [0x7E, 0xFE, 0x7E, 0xFE]
    # a blmhd slice into a blmhd cache
    dst = torch.full((B, L, M, Hkv, D), 0x33, dtype=torch.uint8, device=dev)
    out = sfa.quantize_kv8(src[1, LAYER, :rows], sc_d, out=dst[1, LAYER, :rows])
    assert out.data_ptr() == dst[1, LAYER].data_ptr()
    np.testing.assert_array_equal(dst[1, LAYER, :rows].cpu().numpy(), want)
    dst[1, LAYER, :rows] = 0x33
    assert bool((dst == 0x33).all())                            # nothing else was written
    # a blhmd slice (other strides) into a blhmd fp8 cache, from the blmhd source
    dst_h = torch.full((B, L, Hkv, M, D), 0x33, dtype=torch.uint8, device=dev).view(torch.float8_e4m3fn)
    sfa.quantize_kv8(src[1, LAYER, :rows], sc_d, out=dst_h[1, LAYER, :, :rows].permute(1, 0, 2))
    np.testing.assert_array_equal(dst_h.view(torch.uint8)[1, LAYER, :, :rows].permute(1, 0, 2).cpu().numpy(), want)
    assert bool((dst_h.view(torch.uint8)[1, LAYER, :, rows:] == 0x33).all()) and bool((dst_h.view(torch.uint8)[0] == 0x33).all())
    # a blhmd source slice, a new contiguous result; no rows: nothing happens
    src_h = src.permute(0, 1, 3, 2, 4).contiguous()
    got = sfa.quantize_kv8(src_h[1, LAYER, :, :rows].permute(1, 0, 2), sc_d)
    assert got.dtype == torch.uint8 and got.is_contiguous()
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    assert sfa.quantize_kv8(src[1, LAYER, :0], sc_d).shape == (0, Hkv, D)
    torch.cuda.synchronize()


def test_kv8_prompt_through_a_staging_cache(sfa):
    """The documented prompt flow: flash_decode_chunk on one 16-bit staging layer, quantize_kv8 into the fp8 cache, then
    a decode step over it, against the reference on the same bytes."""
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(120)
    B, Hkv, G, D, n = 2, 2, 4, 128, 45
    H = Hkv * G
    dt = torch.bfloat16
    prompt = torch.from_numpy(round_to(rng.standard_normal((B, n, H + 2 * Hkv, D)), "bf16")).to(dt).to(dev)
    stage_k, stage_v = (torch.zeros((B, 1, M, Hkv, D), dtype=dt, device=dev) for _ in range(2))
    zero = torch.zeros(B, dtype=torch.int32, device=dev)
    sfa.flash_decode_chunk(prompt, None, None, None, stage_k, stage_v, zero, torch.empty((B, n, H, D), dtype=dt, device=dev),
                           B, M, H, D, D, M, 1, 0, num_heads_kv=Hkv)
    ks = (stage_k[:, 0, :n].float().abs().amax(dim=(0, 1, 3)) / 448.0).contiguous()
    vs = (stage_v[:, 0, :n].float().abs().amax(dim=(0, 1, 3)) / 448.0).contiguous()
    k8 = torch.zeros((B, L, M, Hkv, D), dtype=torch.uint8, device=dev)
    v8 = torch.zeros_like(k8)
    for b in range(B):
        sfa.quantize_kv8(stage_k[b, 0, :n], ks, out=k8[b, LAYER, :n])
        sfa.quantize_kv8(stage_v[b, 0, :n], vs, out=v8[b, LAYER, :n])
    torch.cuda.synchronize()
    np.testing.assert_array_equal(k8[:, LAYER, :n].cpu().numpy(),
                                  kv8_ref.quantize(stage_k[:, 0, :n].float().cpu().numpy(), ks.cpu().numpy()))
    pr = dict(qkv=round_to(rng.standard_normal((B, H + 2 * Hkv, D)), "bf16"), k8=k8.cpu().numpy(), v8=v8.cpu().numpy(),
              ks=ks.cpu().numpy(), vs=vs.cpu().numpy(), B=B, H=H, Hkv=Hkv, D=D, dtype="bf16")
    check(sfa, pr, [n, n])
