"""GPU parity of the HIP decode path (through the C ABI) against the CPU oracle and the
reference-generated golden vectors.

Tolerances: kernel vs fp64 oracle on identically rounded inputs --
fp16 atol=rtol=2e-3, bf16 atol=rtol=1.6e-2.  The appended K row is compared to one storage ulp
(on-device sincosf/powf vs numpy differ in the last fp32 bit of the angle); the appended V row
and everything that is pure data movement must be bit-exact.
"""
import numpy as np
import pytest
import torch

from conftest import bf16bits_to_f32
from oracle import decode_ref, rotary_table_ref, round_to

pytestmark = pytest.mark.gpu

TOL = {"fp16": 2e-3, "bf16": 1.6e-2}
ULP = {"fp16": 2.0 ** -10, "bf16": 2.0 ** -7}
TDT = {"fp16": torch.float16, "bf16": torch.bfloat16}


@pytest.fixture(scope="module")
def sfa():
    assert torch.cuda.is_available(), "GPU tests need a GPU (run with -m gpu on the MI355X box)"
    import starflashattention_amd as m
    m._lib.load()                  # fail loudly if the HIP library is missing
    return m


def run_decode(sfa, qkv, kc, vc, lens, layer, rot, dtype, num_splits=0, biases=None, tables=None):
    """numpy fp32 (representable) in -> (o, kc_after, vc_after) numpy fp32 out."""
    dev = torch.device("cuda:0")
    dt = TDT[dtype]
    B, _, H, D = qkv.shape
    L, M = kc.shape[1], kc.shape[2]
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dt).to(dev)
    qkv_d, kc_d, vc_d = t(qkv), t(kc), t(vc)
    o = torch.full((B, H, D), 7.0, dtype=dt, device=dev)
    if biases is None:
        bq = bk = bv = torch.zeros(0, dtype=dt, device=dev)
    else:
        bq, bk, bv = (t(b) for b in biases)
    kw = {}
    if tables is not None:
        kw = dict(rotary_cos_table=t(tables[0]), rotary_sin_table=t(tables[1]))
    ret = sfa.flash_decode(qkv_d, bq, bk, bv, kc_d, vc_d,
                           torch.tensor(list(lens), dtype=torch.int32, device=dev), o,
                           B, M, H, D, rot, M, L, layer, num_splits=num_splits, **kw)
    assert ret.data_ptr() == o.data_ptr()          # returns the tensor it was given (api:67)
    torch.cuda.synchronize()
    return o.float().cpu().numpy(), kc_d.float().cpu().numpy(), vc_d.float().cpu().numpy()


def check_against_oracle(sfa, qkv, kc, vc, lens, layer, rot, dtype, **kw):
    kc_ref, vc_ref = kc.copy(), vc.copy()
    okw = {}
    if kw.get("biases") is not None:
        okw = dict(q_bias=kw["biases"][0], k_bias=kw["biases"][1], v_bias=kw["biases"][2])
    if kw.get("tables") is not None:
        okw.update(cos_table=kw["tables"][0], sin_table=kw["tables"][1])
    ref = decode_ref(qkv, kc_ref, vc_ref, lens, layer, rot, dtype=dtype, **okw)
    o, kc_out, vc_out = run_decode(sfa, qkv, kc, vc, lens, layer, rot, dtype, **kw)
    tol = TOL[dtype]
    np.testing.assert_allclose(o, ref["o"], atol=tol, rtol=tol)
    B = qkv.shape[0]
    for b in range(B):
        krow, vrow = kc_out[b, layer, lens[b]], vc_out[b, layer, lens[b]]
        np.testing.assert_array_equal(vrow, ref["v_row"][b])                 # data movement: exact
        err = np.abs(krow - ref["k_row"][b])
        assert np.all(err <= ULP[dtype] * np.maximum(1.0, np.abs(krow)) * 1.01), err.max()
        assert np.mean(krow == ref["k_row"][b]) > 0.98
    # nothing else in the caches may change
    mask = np.ones(kc.shape[:3], bool)
    for b in range(B):
        mask[b, layer, lens[b]] = False
    np.testing.assert_array_equal(kc_out[mask], kc[mask])
    np.testing.assert_array_equal(vc_out[mask], vc[mask])
    return o, ref


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("num_splits", [0, 1, 3, 4])
@pytest.mark.parametrize("nt", ["0", "1"])
def test_decode_golden_reference_vectors(sfa, decode_golden, dtype, num_splits, nt):
    """Every golden case (seq_len around the 32/128 block and split boundaries), against the
    reference's own outputs; with default and with non-temporal cache-row loads (the launcher picks
    the latter for caches beyond the Infinity Cache -- bench sizes)."""
    sfa.debug_set("decode_nt", int(nt))
    try:
        _golden_reference_vectors(sfa, decode_golden, dtype, num_splits)
    finally:
        sfa.debug_set("decode_nt", -1)


def _golden_reference_vectors(sfa, decode_golden, dtype, num_splits):
    g = decode_golden
    qkv = bf16bits_to_f32(g["qkv_bf16bits"])
    kc = bf16bits_to_f32(g["k_cache_bf16bits"])
    vc = bf16bits_to_f32(g["v_cache_bf16bits"])
    layer = int(g["idx_layer"])
    B, H, D, L, M = (int(x) for x in g["dims"])
    tag = {"fp16": "f16", "bf16": "bf16"}[dtype]
    for case, s in enumerate(g["seq_lens"]):
        lens = [int(s)] * B
        o, ref = check_against_oracle(sfa, qkv, kc, vc, lens, layer, D, dtype, num_splits=num_splits)
        # reference evaluated in fp32 on the same 16-bit inputs (it does not round q/k after RoPE)
        np.testing.assert_allclose(o, g["o_f32"][case], atol=TOL[dtype], rtol=TOL[dtype])
        # reference evaluated natively in the 16-bit dtype
        np.testing.assert_allclose(o, g[f"o_{tag}"][case], atol=2 * TOL[dtype], rtol=2 * TOL[dtype])


def test_decode_golden_ragged_batch(sfa, decode_golden):
    g = decode_golden
    qkv = bf16bits_to_f32(g["qkv_bf16bits"])
    kc = bf16bits_to_f32(g["k_cache_bf16bits"])
    vc = bf16bits_to_f32(g["v_cache_bf16bits"])
    layer = int(g["idx_layer"])
    D = int(g["dims"][2])
    lens = [int(g["seq_lens"][3]), int(g["seq_lens"][7])]       # 32 and 129
    o, _ = check_against_oracle(sfa, qkv, kc, vc, lens, layer, D, "fp16", num_splits=2)
    np.testing.assert_allclose(o[0], g["o_f32"][3][0], atol=2e-3, rtol=2e-3)
    np.testing.assert_allclose(o[1], g["o_f32"][7][1], atol=2e-3, rtol=2e-3)


def test_decode_partial_rotary_golden(sfa, decode_golden):
    g = decode_golden
    qkv = bf16bits_to_f32(g["qkv_bf16bits"])
    kc = bf16bits_to_f32(g["k_cache_bf16bits"])
    vc = bf16bits_to_f32(g["v_cache_bf16bits"])
    layer, rot = int(g["idx_layer"]), int(g["partial_rot_dim"])
    B, H, D, L, M = (int(x) for x in g["dims"])
    for case in (0, 4, 8):
        s = int(g["seq_lens"][case])
        _, kc_out, _ = run_decode(sfa, qkv, kc, vc, [s] * B, layer, rot, "fp16")
        want = round_to(g["partial_k_rot_f32"][case], "fp16")
        got = kc_out[:, layer, s]
        assert np.all(np.abs(got - want) <= ULP["fp16"] * np.maximum(1.0, np.abs(want)) * 1.01)
        np.testing.assert_array_equal(got[..., rot:], qkv[:, 1, :, rot:])
        check_against_oracle(sfa, qkv, kc, vc, [s] * B, layer, rot, "fp16")


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("D,H", [(128, 5), (64, 3), (256, 2)])
def test_decode_random_shapes(sfa, dtype, D, H):
    rng = np.random.default_rng(11 + D + H)
    B, L, M = 3, 2, 700
    qkv = round_to(rng.standard_normal((B, 3, H, D)), dtype)
    kc = round_to(rng.standard_normal((B, L, M, H, D)), dtype)
    vc = round_to(rng.standard_normal((B, L, M, H, D)), dtype)
    for lens, splits in (([0, 699, 333], 0), ([1, 15, 16], 1), ([64, 65, 63], 5), ([511, 512, 513], 7)):
        check_against_oracle(sfa, qkv, kc, vc, lens, 0, D, dtype, num_splits=splits)
        check_against_oracle(sfa, qkv, kc, vc, lens, 1, D // 2, dtype, num_splits=splits)
        check_against_oracle(sfa, qkv, kc, vc, lens, 1, 0, dtype, num_splits=splits)


def test_decode_bias_and_rotary_table(sfa):
    rng = np.random.default_rng(5)
    B, H, D, L, M = 2, 4, 128, 1, 300
    qkv = round_to(rng.standard_normal((B, 3, H, D)), "fp16")
    kc = round_to(rng.standard_normal((B, L, M, H, D)), "fp16")
    vc = round_to(rng.standard_normal((B, L, M, H, D)), "fp16")
    biases = [round_to(0.5 * rng.standard_normal((H, D)), "fp16") for _ in range(3)]
    check_against_oracle(sfa, qkv, kc, vc, [200, 299], 0, D, "fp16", biases=biases, num_splits=2)
    # LUT path (the C++ harness's compute_rotary_table): device table == oracle table, then decode
    cos_d, sin_d = sfa.compute_rotary_table(M, D, torch.float16)
    cos_r, sin_r = rotary_table_ref(M, D, "fp16")
    assert np.max(np.abs(cos_d.float().cpu().numpy() - cos_r)) <= 2.0 ** -10
    assert np.max(np.abs(sin_d.float().cpu().numpy() - sin_r)) <= 2.0 ** -10
    assert np.mean(cos_d.float().cpu().numpy() == cos_r) > 0.98
    check_against_oracle(sfa, qkv, kc, vc, [17, 250], 0, D, "fp16", tables=(cos_r, sin_r))


def test_decode_ones_known_answer_reference_shapes(sfa, ones_kat):
    """The reference's only known answer (cc:63-78, 116-129): all ones -> all 1.0, at its own
    shapes B=2,H=32,D=128,L=4 and (max_seq_len, seq_len) pairs (cc:138-146), fp16, splits=4."""
    dev = torch.device("cuda:0")
    B, H, D, L = (int(x) for x in ones_kat["dims_BHDL"])
    for M, s in ones_kat["max_seq_len__seq_len"]:
        M, s = int(M), int(s)
        qkv = torch.ones(B, 3, H, D, dtype=torch.float16, device=dev)
        kc = torch.ones(B, L, M, H, D, dtype=torch.float16, device=dev)
        vc = torch.ones(B, L, M, H, D, dtype=torch.float16, device=dev)
        o = torch.zeros(B, H, D, dtype=torch.float16, device=dev)
        z = torch.zeros(H, D, dtype=torch.float16, device=dev)
        sl = torch.full((B,), s, dtype=torch.int32, device=dev)
        sfa.flash_decode(qkv, z, z, z, kc, vc, sl, o, B, M, H, D, D, M, L, 0, num_splits=4)
        torch.cuda.synchronize()
        assert torch.all(o == float(ones_kat["expect"])), (M, s, o.flatten()[:4])


def test_decode_rejects_out_of_range_seq_len(sfa, ones_kat):
    """cc:141-142 pair (4096, 4096) overruns the cache in the reference; here the row is rejected
    on the device: caches untouched, NaN output, sticky status -> RuntimeError when polled."""
    dev = torch.device("cuda:0")
    M, s = (int(x) for x in ones_kat["must_raise"][0])
    B, H, D, L = 2, 4, 128, 1
    M = 64
    qkv = torch.ones(B, 3, H, D, dtype=torch.float16, device=dev)
    kc = torch.ones(B, L, M, H, D, dtype=torch.float16, device=dev)
    vc = torch.ones(B, L, M, H, D, dtype=torch.float16, device=dev)
    guard_k = kc.clone()
    o = torch.zeros(B, H, D, dtype=torch.float16, device=dev)
    z = torch.zeros(H, D, dtype=torch.float16, device=dev)
    sl = torch.tensor([M, 5], dtype=torch.int32, device=dev)       # sample 0 is out of range
    sfa.check_decode_status(dev)                                    # clean slate
    for splits in (1, 2):
        sfa.flash_decode(qkv, z, z, z, kc, vc, sl, o, B, M, H, D, D, M, L, 0, num_splits=splits)
        with pytest.raises(RuntimeError, match="seq_len"):
            sfa.check_decode_status(dev)
        assert torch.isnan(o[0]).all() and torch.all(o[1] == 1.0)
        assert torch.equal(kc[0], guard_k[0])
    sfa.check_decode_status(dev)                                    # flag was cleared by the raise


def test_decode_argument_errors(sfa):
    dev = torch.device("cuda:0")
    B, H, D, L, M = 1, 2, 128, 1, 16
    mk = lambda *s, dt=torch.float16: torch.zeros(*s, dtype=dt, device=dev)
    args = lambda **kw: dict(dict(qkv=mk(B, 3, H, D), kc=mk(B, L, M, H, D), vc=mk(B, L, M, H, D),
                                  sl=mk(B, dt=torch.int32), o=mk(B, H, D)), **kw)

    def call(a, D_=D):
        z = mk(0)
        return sfa.flash_decode(a["qkv"], z, z, z, a["kc"], a["vc"], a["sl"], a["o"], B, M, H, D_, D_, M, L, 0)

    call(args())
    with pytest.raises(RuntimeError, match="dtype"):
        call(args(o=mk(B, H, D, dt=torch.bfloat16)))
    with pytest.raises(RuntimeError, match="shape"):
        call(args(kc=mk(B, L, M + 1, H, D)))
    with pytest.raises(RuntimeError, match="float16 or bfloat16"):
        call(args(qkv=mk(B, 3, H, D, dt=torch.float32)))
    with pytest.raises(RuntimeError, match="HIP device"):
        call(args(sl=torch.zeros(B, dtype=torch.int32)))
    with pytest.raises(RuntimeError, match="contiguous"):
        call(args(o=mk(B, H, 2 * D)[..., ::2]))


def test_decode_roundtrip_multi_step_append(sfa):
    """Size-independent property: decoding T tokens one by one (each step appends its K/V) gives,
    at the last step, the same output as one causal-attention row computed from scratch."""
    from oracle import sdpa_ref, rope_interleaved
    rng = np.random.default_rng(21)
    dev = torch.device("cuda:0")
    B, H, D, L, M, T = 2, 2, 128, 1, 40, 24
    toks = round_to(rng.standard_normal((T, B, 3, H, D)), "bf16")
    kc = torch.zeros(B, L, M, H, D, dtype=torch.bfloat16, device=dev)
    vc = torch.zeros_like(kc)
    o = torch.zeros(B, H, D, dtype=torch.bfloat16, device=dev)
    z = torch.zeros(0, dtype=torch.bfloat16, device=dev)
    for t in range(T):
        sl = torch.full((B,), t, dtype=torch.int32, device=dev)
        sfa.flash_decode(torch.from_numpy(toks[t]).bfloat16().to(dev), z, z, z, kc, vc, sl, o,
                         B, M, H, D, D, M, L, 0)
    torch.cuda.synchronize()
    # from scratch on the CPU: rope every token at its own position, attend with the last query
    K = np.stack([round_to(rope_interleaved(toks[t][:, 1], t, D), "bf16") for t in range(T)], 2)  # [B,H,T,D]
    V = np.stack([toks[t][:, 2] for t in range(T)], 2)
    q = round_to(rope_interleaved(toks[T - 1][:, 0], T - 1, D), "bf16")[:, :, None, :]
    want = sdpa_ref(q, K, V)[:, :, 0]
    np.testing.assert_allclose(o.float().cpu().numpy(), want, atol=1.6e-2, rtol=1.6e-2)
    np.testing.assert_array_equal(vc[:, 0, :T].float().cpu().numpy(), V.transpose(0, 2, 1, 3))


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("num_splits", [0, 1, 3])
def test_decode_head_major_kv_layout(sfa, dtype, num_splits):
    """kv_layout="blhmd" (SURVEY.md 8f-2): the same decode step on [B, L, H, M, D] caches -- output
    bit-identical to the reference layout's, the appended row lands at [b, layer, h, seq_len[b], :],
    nothing else is touched."""
    rng = np.random.default_rng(5)
    B, H, D, L, M, layer = 3, 4, 128, 2, 96, 1
    tdt = {"fp16": torch.float16, "bf16": torch.bfloat16}[dtype]
    dev = torch.device("cuda:0")
    qkv = torch.from_numpy(rng.standard_normal((B, 3, H, D)).astype(np.float32)).to(tdt).to(dev)
    kc = torch.from_numpy(rng.standard_normal((B, L, M, H, D)).astype(np.float32)).to(tdt).to(dev)
    vc = torch.from_numpy(rng.standard_normal((B, L, M, H, D)).astype(np.float32)).to(tdt).to(dev)
    lens = [0, 37, M - 1]
    sl = torch.tensor(lens, dtype=torch.int32, device=dev)
    z = torch.zeros(0, dtype=tdt, device=dev)
    kc_a, vc_a = kc.clone(), vc.clone()
    kc_h, vc_h = (t.permute(0, 1, 3, 2, 4).contiguous() for t in (kc, vc))
    o_a = torch.empty((B, H, D), dtype=tdt, device=dev)
    o_h = torch.empty_like(o_a)
    sfa.flash_decode(qkv, z, z, z, kc_a, vc_a, sl, o_a, B, M, H, D, D, M, L, layer, num_splits=num_splits)
    sfa.flash_decode(qkv, z, z, z, kc_h, vc_h, sl, o_h, B, M, H, D, D, M, L, layer, num_splits=num_splits,
                     kv_layout="blhmd")
    torch.cuda.synchronize()
    assert torch.equal(o_a, o_h)
    assert torch.equal(kc_h.permute(0, 1, 3, 2, 4), kc_a)
    assert torch.equal(vc_h.permute(0, 1, 3, 2, 4), vc_a)
    for b in range(B):      # the appended rows really changed, everything else did not
        assert not torch.equal(kc_a[b, layer, lens[b]], kc[b, layer, lens[b]])
    mask = torch.ones((B, L, M), dtype=torch.bool, device=dev)
    for b in range(B):
        mask[b, layer, lens[b]] = False
    assert torch.equal(kc_a[mask], kc[mask]) and torch.equal(vc_a[mask], vc[mask])
    with pytest.raises(RuntimeError, match="kv_layout"):
        sfa.flash_decode(qkv, z, z, z, kc_h, vc_h, sl, o_h, B, M, H, D, D, M, L, layer, kv_layout="paged")
    with pytest.raises(RuntimeError, match="k_cache_table"):       # shape is checked against the layout
        sfa.flash_decode(qkv, z, z, z, kc_a, vc_a, sl, o_h, B, M, H, D, D, M, L, layer, kv_layout="blhmd")


@pytest.mark.parametrize("dtype,D", [("fp16", 128), ("bf16", 128), ("bf16", 64), ("fp16", 256)])
@pytest.mark.parametrize("num_splits", [0, 1, 3])
@pytest.mark.parametrize("page_size", [16, 64])
def test_decode_paged_kv_cache(sfa, dtype, D, num_splits, page_size):
    """kv_layout="paged" (SURVEY.md 8f-2): the contiguous caches cut into pages and scattered through
    a shuffled pool.  Output bit-identical to the contiguous run; the new row lands in the right page;
    no other pool byte changes; a table entry outside the pool raises the sticky status."""
    rng = np.random.default_rng(7)
    B, H, L, M, layer = 3, 4, 2, 192, 1
    tdt = {"fp16": torch.float16, "bf16": torch.bfloat16}[dtype]
    dev = torch.device("cuda:0")
    qkv = torch.from_numpy(rng.standard_normal((B, 3, H, D)).astype(np.float32)).to(tdt).to(dev)
    kc = torch.from_numpy(rng.standard_normal((B, L, M, H, D)).astype(np.float32)).to(tdt).to(dev)
    vc = torch.from_numpy(rng.standard_normal((B, L, M, H, D)).astype(np.float32)).to(tdt).to(dev)
    lens = [0, 77, M - 1]
    sl = torch.tensor(lens, dtype=torch.int32, device=dev)
    z = torch.zeros(0, dtype=tdt, device=dev)
    pps = M // page_size                                   # pages per sequence
    num_pages = B * pps + 5                                 # a few pages nobody owns
    perm = torch.from_numpy(rng.permutation(num_pages)[:B * pps].astype(np.int32)).view(B, pps)
    table = perm.to(dev)

    def to_pool(c):
        pool = torch.from_numpy(rng.standard_normal((num_pages, L, page_size, H, D)).astype(np.float32)).to(tdt).to(dev)
        # [B, L, pps, page_size, H, D] -> pool[table[b, i]] = c[b, :, i*ps:(i+1)*ps]
        pool[table.long().view(-1)] = c.view(B, L, pps, page_size, H, D).permute(0, 2, 1, 3, 4, 5).reshape(
            B * pps, L, page_size, H, D)
        return pool
    kp, vp = to_pool(kc), to_pool(vc)
    kp0, vp0 = kp.clone(), vp.clone()
    kc_a, vc_a = kc.clone(), vc.clone()
    o_a = torch.empty((B, H, D), dtype=tdt, device=dev)
    o_p = torch.empty_like(o_a)
    sfa.flash_decode(qkv, z, z, z, kc_a, vc_a, sl, o_a, B, M, H, D, D, M, L, layer, num_splits=num_splits)
    sfa.flash_decode(qkv, z, z, z, kp, vp, sl, o_p, B, M, H, D, D, M, L, layer, num_splits=num_splits,
                     kv_layout="paged", block_table=table)
    sfa.check_decode_status()
    if D >= 128:            # same rows per step as the contiguous kernel: bit-identical
        assert torch.equal(o_a, o_p)
    else:                   # D=64 pages in 16-row steps, the contiguous kernel in 32-row steps
        np.testing.assert_allclose(o_p.float().cpu().numpy(), o_a.float().cpu().numpy(), atol=TOL[dtype] / 4,
                                   rtol=TOL[dtype] / 4)
    changed_k = (kp != kp0).flatten(2).any(-1)             # [num_pages, L]
    for b in range(B):
        pg, row = int(perm[b, lens[b] // page_size]), lens[b] % page_size
        assert torch.equal(kp[pg, layer, row], kc_a[b, layer, lens[b]])
        assert torch.equal(vp[pg, layer, row], vc_a[b, layer, lens[b]])
        kp0[pg, layer, row] = kp[pg, layer, row]
        vp0[pg, layer, row] = vp[pg, layer, row]
    assert torch.equal(kp, kp0) and torch.equal(vp, vp0)   # nothing but the three appended rows changed
    assert int(changed_k.sum()) == B
    # a table entry outside the pool: reported, not dereferenced
    bad = table.clone()
    bad[1, 0] = num_pages + 3
    sfa.flash_decode(qkv, z, z, z, kp, vp, sl, o_p, B, M, H, D, D, M, L, layer, kv_layout="paged", block_table=bad)
    with pytest.raises(RuntimeError, match="block_table"):
        sfa.check_decode_status()
    assert torch.isnan(o_p[1].float()).all() and not torch.isnan(o_p[0].float()).any()     # the sequence that read it
    assert torch.equal(kp, kp0) and torch.equal(vp, vp0)   # (the appended rows were simply written again)
    with pytest.raises(RuntimeError, match="page_size"):
        sfa.flash_decode(qkv, z, z, z, kp[:, :, :8].contiguous(), vp[:, :, :8].contiguous(), sl, o_p, B, M, H, D, D,
                         M, L, layer, kv_layout="paged", block_table=table)


@pytest.mark.parametrize("group", [1, 2, 8])          # multi-head, VALU grouped-query and matrix-core kernels
@pytest.mark.parametrize("num_splits", [1, 3])
@pytest.mark.parametrize("where", ["append_page", "read_page"])
def test_decode_paged_bad_table_entry(sfa, group, num_splits, where):
    """A block_table entry outside the pool: on the page the new token goes to, the sequence is
    rejected like a bad seq_len -- NOTHING is stored through a substituted page, o[b] is NaN, the sticky
    status is raised; on a page that is only read, page 0 is read in its place and o[b] is NaN as well.
    The other sequences of the batch are served normally."""
    rng = np.random.default_rng(23)
    B, Hkv, L, M, layer, D, ps = 3, 2, 1, 128, 0, 128, 16
    H = Hkv * group
    dev = torch.device("cuda:0")
    mk = lambda *shape: torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).to(torch.bfloat16).to(dev)
    qkv = mk(B, 3, H, D) if group == 1 else mk(B, H + 2 * Hkv, D)
    pps = M // ps
    num_pages = B * pps
    table = torch.from_numpy(rng.permutation(num_pages).astype(np.int32)).view(B, pps).to(dev)
    kp, vp = mk(num_pages, L, ps, Hkv, D), mk(num_pages, L, ps, Hkv, D)
    lens = [40, 77, 100]
    sl = torch.tensor(lens, dtype=torch.int32, device=dev)
    z = torch.zeros(0, dtype=torch.bfloat16, device=dev)
    kw = dict(kv_layout="paged", num_splits=num_splits, num_heads_kv=Hkv)
    good = torch.empty((B, H, D), dtype=torch.bfloat16, device=dev)
    kg, vg = kp.clone(), vp.clone()
    sfa.flash_decode(qkv, z, z, z, kg, vg, sl, good, B, M, H, D, D, M, L, layer, block_table=table, **kw)
    sfa.check_decode_status()
    bad = table.clone()
    victim = 1
    bad[victim, lens[victim] // ps if where == "append_page" else 0] = -7 if where == "append_page" else num_pages
    kb, vb = kp.clone(), vp.clone()
    o = torch.full((B, H, D), 3.0, dtype=torch.bfloat16, device=dev)
    sfa.flash_decode(qkv, z, z, z, kb, vb, sl, o, B, M, H, D, D, M, L, layer, block_table=bad, **kw)
    with pytest.raises(RuntimeError, match="block_table"):
        sfa.check_decode_status()
    assert torch.isnan(o[victim].float()).all()
    for b in (0, 2):                                        # the healthy sequences: same bits as the clean run
        assert torch.equal(o[b], good[b])
    if where == "append_page":
        # the victim's row was not written anywhere: the pools differ from the originals only by the two healthy appends
        kb2, vb2 = kp.clone(), vp.clone()
        for b in (0, 2):
            pg, row = int(table[b, lens[b] // ps]), lens[b] % ps
            kb2[pg, layer, row], vb2[pg, layer, row] = kg[pg, layer, row], vg[pg, layer, row]
        assert torch.equal(kb, kb2) and torch.equal(vb, vb2)
    else:
        assert torch.equal(kb, kg) and torch.equal(vb, vg)     # reads only: same appends as the clean run
    sfa.check_decode_status()                               # the flag was reset by the raise above


@pytest.mark.parametrize("dtype,D", [("fp16", 128), ("bf16", 128), ("bf16", 64), ("fp16", 64), ("bf16", 256), ("fp16", 256)])
@pytest.mark.parametrize("group", [2, 4, 8, 16])
@pytest.mark.parametrize("num_splits", [0, 1, 3])
def test_decode_grouped_queries(sfa, dtype, D, group, num_splits):
    """Grouped-query decode (num_heads_kv): one workgroup serves the G query heads of a
    kv head from one pass over the cache (the matrix-core kernel: G = 16, G = 8, and G = 4 at head_dim 128; the VALU
    kernel otherwise).  Checked against the (oracle-validated) multi-head kernel on
    the expanded problem -- kv heads repeated G times -- and against the fp64 oracle on it."""
    rng = np.random.default_rng(11)
    B, Hkv, L, M, layer = 3, 2, 2, 160, 0
    H = Hkv * group
    tdt = {"fp16": torch.float16, "bf16": torch.bfloat16}[dtype]
    dev = torch.device("cuda:0")
    mk = lambda *shape: torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).to(tdt).to(dev)
    qkv = mk(B, H + 2 * Hkv, D)
    kc, vc = mk(B, L, M, Hkv, D), mk(B, L, M, Hkv, D)
    qb, kb_, vb_ = mk(H, D), mk(Hkv, D), mk(Hkv, D)
    lens = [0, 53, M - 1]
    sl = torch.tensor(lens, dtype=torch.int32, device=dev)
    rot = D // 2
    # the expanded multi-head problem
    rep = lambda t, dim: t.repeat_interleave(group, dim)
    qkv_x = torch.stack([qkv[:, :H], rep(qkv[:, H:H + Hkv], 1), rep(qkv[:, H + Hkv:], 1)], 1).contiguous()
    kc_x, vc_x = rep(kc, 3).contiguous(), rep(vc, 3).contiguous()
    o = torch.empty((B, H, D), dtype=tdt, device=dev)
    o_x = torch.empty_like(o)
    kc_g, vc_g = kc.clone(), vc.clone()
    sfa.flash_decode(qkv, qb, kb_, vb_, kc_g, vc_g, sl, o, B, M, H, D, rot, M, L, layer, num_splits=num_splits,
                     num_heads_kv=Hkv)
    sfa.flash_decode(qkv_x, qb, rep(kb_, 0).contiguous(), rep(vb_, 0).contiguous(), kc_x, vc_x, sl, o_x, B, M, H, D,
                     rot, M, L, layer, num_splits=num_splits)
    sfa.check_decode_status()
    tol = TOL[dtype]
    np.testing.assert_allclose(o.float().cpu().numpy(), o_x.float().cpu().numpy(), atol=tol / 2, rtol=tol / 2)
    f = lambda t: t.float().cpu().numpy()
    ref = decode_ref(f(qkv_x), f(rep(kc, 3)), f(rep(vc, 3)), lens, layer, rot, dtype=dtype, q_bias=f(qb),
                     k_bias=f(rep(kb_, 0)), v_bias=f(rep(vb_, 0)))
    np.testing.assert_allclose(f(o), ref["o"], atol=tol, rtol=tol)         # the fp64 oracle on the expanded problem
    if group == 2:
        # Same row grouping as the multi-head kernel (four row groups a step, the same lane groups, the same split
        # merge): bit-identical -- measured on MI355X for every (dtype, head_dim) here but fp16 at head_dim 256, where
        # isolated elements differ by ONE fp16 ulp (max |diff| 1.5e-5 at all three num_splits; bf16 at 256 is identical,
        # its ulp being 8 x coarser).  The two kernels' source arithmetic is the same; the cause was not isolated further
        # (hipcc contracting a multiply-add differently in one of the two instantiations is the candidate).
        if (dtype, D) == ("fp16", 256):
            ulps = (o.view(torch.int16).int() - o_x.view(torch.int16).int()).abs()
            assert int(ulps.max()) <= 1
        else:
            assert torch.equal(o, o_x)
    # appended rows: identical to the expanded run's, everything else untouched
    assert torch.equal(rep(kc_g, 3), kc_x) and torch.equal(rep(vc_g, 3), vc_x)
    mask = torch.ones((B, L, M), dtype=torch.bool, device=dev)
    for b in range(B):
        mask[b, layer, lens[b]] = False
        assert not torch.equal(kc_g[b, layer, lens[b]], kc[b, layer, lens[b]])
    assert torch.equal(kc_g[mask], kc[mask]) and torch.equal(vc_g[mask], vc[mask])
    # head-major caches work for grouped queries too
    kc_h, vc_h = (t.permute(0, 1, 3, 2, 4).contiguous() for t in (kc, vc))
    o_h = torch.empty_like(o)
    sfa.flash_decode(qkv, qb, kb_, vb_, kc_h, vc_h, sl, o_h, B, M, H, D, rot, M, L, layer, num_splits=num_splits,
                     num_heads_kv=Hkv, kv_layout="blhmd")
    assert torch.equal(o_h, o)
    # ... and so do paged pools
    ps = 16
    pps = M // ps
    table = torch.from_numpy(rng.permutation(B * pps + 3)[:B * pps].astype(np.int32)).view(B, pps).to(dev)
    def to_pool(c):
        pool = torch.zeros((B * pps + 3, L, ps, Hkv, D), dtype=tdt, device=dev)
        pool[table.long().view(-1)] = c.view(B, L, pps, ps, Hkv, D).permute(0, 2, 1, 3, 4, 5).reshape(B * pps, L, ps, Hkv, D)
        return pool
    kp, vp = to_pool(kc), to_pool(vc)
    o_p = torch.empty_like(o)
    sfa.flash_decode(qkv, qb, kb_, vb_, kp, vp, sl, o_p, B, M, H, D, rot, M, L, layer, num_splits=num_splits,
                     num_heads_kv=Hkv, kv_layout="paged", block_table=table)
    sfa.check_decode_status()
    if D >= 128:
        assert torch.equal(o_p, o)
    else:   # D=64 pages in shorter steps than the contiguous kernel
        np.testing.assert_allclose(o_p.float().cpu().numpy(), o.float().cpu().numpy(), atol=tol / 2, rtol=tol / 2)
    for b in range(B):
        pg, row = int(table[b, lens[b] // ps]), lens[b] % ps
        assert torch.equal(kp[pg, layer, row], kc_g[b, layer, lens[b]])
    with pytest.raises(RuntimeError, match="num_heads"):
        sfa.flash_decode(qkv, qb, kb_, vb_, kc_g, vc_g, sl, o, B, M, H, D, rot, M, L, layer, num_heads_kv=H + 1)


def test_decode_gqa_workspace_sized_by_query_heads(sfa):
    """The older contract of the C ABI: num_splits <= 0 and a workspace sized with sfa_decode_workspace_bytes(..., 0),
    which knows the query-head count only.  With grouped queries the library's own split count (by KV heads) can be
    larger than that size allows -- sfa_decode then takes the largest count that fits instead of failing (round-2
    advisor item).  B * Hkv = 8 < 128 and M = 8192 (4 splits by KV heads, 1 by query heads): the case that used to return
    SFA_ERR_WORKSPACE_TOO_SMALL."""
    rng = np.random.default_rng(5)
    B, Hkv, group, D, L, M, layer = 4, 2, 16, 128, 1, 8192, 0
    H = Hkv * group
    dev = torch.device("cuda:0")
    mk = lambda *shape: torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).to(torch.bfloat16).to(dev)
    qkv = mk(B, H + 2 * Hkv, D)
    kc, vc = mk(B, L, M, Hkv, D), mk(B, L, M, Hkv, D)
    sl = torch.tensor([M - 1, 777, 0, 4099], dtype=torch.int32, device=dev)
    o_new, o_old = (torch.empty((B, H, D), dtype=torch.bfloat16, device=dev) for _ in range(2))
    lib = sfa._lib.load()
    assert lib.sfa_decode_auto_splits(B, Hkv, D, M) > lib.sfa_decode_auto_splits(B, H, D, M)
    sfa.flash_decode(qkv, None, None, None, kc.clone(), vc.clone(), sl, o_new, B, M, H, D, D, M, L, layer, num_heads_kv=Hkv)
    sfa.flash_decode(qkv, None, None, None, kc.clone(), vc.clone(), sl, o_old, B, M, H, D, D, M, L, layer, num_heads_kv=Hkv,
                     _sized_by_query_heads=True)
    sfa.check_decode_status()
    tol = TOL["bf16"]
    np.testing.assert_allclose(o_old.float().cpu().numpy(), o_new.float().cpu().numpy(), atol=tol, rtol=tol)


def test_decode_exact_workspace_through_the_c_abi(sfa):
    """sfa_decode itself, with a workspace of exactly sfa_decode_workspace_bytes(..., 3) bytes and a canary behind it:
    bit-identical to the operator (which uses its roomy cached workspace) and nothing written past the end."""
    from exact_workspace import call_with_exact_workspace, decode_problem
    from starflashattention_amd import _lib, ops
    dev = torch.device("cuda:0")
    B, H, Hkv, D, L, M, S = 3, 4, 2, 64, 1, 128, 3
    qkv, kc0, vc0, o0 = decode_problem((B,), B, H, Hkv, D, L, M, 71, dev)
    sl = torch.tensor([0, 70, 127], dtype=torch.int32, device=dev)
    z = torch.zeros(0, dtype=torch.float16, device=dev)
    kc1, vc1, o1 = kc0.clone(), vc0.clone(), o0.clone()
    sfa.flash_decode(qkv, z, z, z, kc1, vc1, sl, o1, B, M, H, D, D, M, L, 0, num_splits=S, num_heads_kv=Hkv)
    sfa.check_decode_status(dev)
    kc2, vc2, o2 = kc0.clone(), vc0.clone(), o0.clone()
    a, *_ = ops._decode_args(qkv, z, z, z, kc2, vc2, sl, o2, B, M, H, D, D, M, L, 0, None, None, None, "blmhd", None, Hkv)
    lib = _lib.load()
    a.stride = (H + 2 * Hkv) * D
    call_with_exact_workspace(a, lib.sfa_decode_workspace_bytes(B, H, D, M, S), S, lib.sfa_decode, dev)
    assert torch.equal(o2, o1) and torch.equal(kc2, kc1) and torch.equal(vc2, vc1)
    assert bool(torch.isfinite(o2.float()).all()) and not torch.equal(o2, o0) and not torch.equal(kc2, kc0)


def test_decode_layouts_agree_at_scale(sfa):
    """BASELINE config 4's sequence length and head count at a batch the box can hold thrice: the
    reference layout, the head-major layout and a randomly paged pool (non-temporal loads kick in:
    the caches exceed the Infinity Cache) give bit-identical outputs and appended rows; one (b, h) slice
    against the fp64 oracle."""
    dev = torch.device("cuda:0")
    torch.manual_seed(4)
    B, H, D, L, M, ps = 12, 32, 128, 1, 8192, 64
    tdt = torch.bfloat16
    kc = torch.empty((B, L, M, H, D), dtype=tdt, device=dev).normal_()
    vc = torch.empty((B, L, M, H, D), dtype=tdt, device=dev).normal_()
    qkv = torch.randn((B, 3, H, D), device=dev).to(tdt)
    lens = torch.randint(4000, M - 1, (B,), dtype=torch.int32)
    lens[0], lens[1] = M - 1, 0
    sl = lens.to(dev)
    z = torch.zeros(0, dtype=tdt, device=dev)
    outs = {}
    # reference layout
    k_a, v_a = kc.clone(), vc.clone()
    outs["blmhd"] = torch.empty((B, H, D), dtype=tdt, device=dev)
    sfa.flash_decode(qkv, z, z, z, k_a, v_a, sl, outs["blmhd"], B, M, H, D, D, M, L, 0)
    # head-major
    k_h, v_h = (t.permute(0, 1, 3, 2, 4).contiguous() for t in (kc, vc))
    outs["blhmd"] = torch.empty_like(outs["blmhd"])
    sfa.flash_decode(qkv, z, z, z, k_h, v_h, sl, outs["blhmd"], B, M, H, D, D, M, L, 0, kv_layout="blhmd")
    # paged: the same rows scattered through a shuffled pool
    pps = M // ps
    table = torch.randperm(B * pps, device=dev).to(torch.int32).view(B, pps)
    def to_pool(c):
        pool = torch.empty((B * pps, L, ps, H, D), dtype=tdt, device=dev)
        pool[table.long().view(-1)] = c.view(B, L, pps, ps, H, D).permute(0, 2, 1, 3, 4, 5).reshape(B * pps, L, ps, H, D)
        return pool
    k_p, v_p = to_pool(kc), to_pool(vc)
    outs["paged"] = torch.empty_like(outs["blmhd"])
    sfa.flash_decode(qkv, z, z, z, k_p, v_p, sl, outs["paged"], B, M, H, D, D, M, L, 0, kv_layout="paged",
                     block_table=table)
    sfa.check_decode_status()
    assert torch.equal(outs["blmhd"], outs["blhmd"]) and torch.equal(outs["blmhd"], outs["paged"])
    assert torch.equal(k_h.permute(0, 1, 3, 2, 4), k_a) and torch.equal(v_h.permute(0, 1, 3, 2, 4), v_a)
    for b in (0, 1, 5):
        pos = int(lens[b])
        pg = int(table[b, pos // ps])
        assert torch.equal(k_p[pg, 0, pos % ps], k_a[b, 0, pos]) and torch.equal(v_p[pg, 0, pos % ps], v_a[b, 0, pos])
    # one (b, h) slice against the oracle
    b, h = 5, 7
    f = lambda t: t.float().cpu().numpy()
    ref = decode_ref(f(qkv[b:b + 1, :, h:h + 1]), f(kc[b:b + 1, :, :, h:h + 1]), f(vc[b:b + 1, :, :, h:h + 1]),
                     [int(lens[b])], 0, D, dtype="bf16")
    np.testing.assert_allclose(f(outs["blmhd"][b:b + 1, h:h + 1]), ref["o"], atol=TOL["bf16"], rtol=TOL["bf16"])
