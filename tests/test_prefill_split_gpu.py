"""GPU tests of sfa_prefill_split_fwd / flash_attn_split_fwd / mha_fwd_split: the prefill forward with each q-tile's key
range split over several workgroups and a combine over their fp32 partials, against oracle.sdpa_ref (which
tests/prefill_split_ref.py equals: tests/test_prefill_split_cpu.py) on identically rounded inputs.

Tolerances: o within the project's TOL (fp16 2e-3, bf16 1.6e-2: tests/test_prefill_gpu.py::TOL), lse within 2e-3
(LSE_TOL["exact"] of tests/test_prefill_gpu.py; the split kernel is an exact-scale kernel).  After every call
sfa_debug_get("last_prefill_splits") must hold the resolved count: that the split kernels ran, and with how many splits.
The shapes are the smallest that reach each edge of the partition (the table at SHAPES)."""
import functools

import numpy as np
import pytest
import torch

import prefill_cases as pc
from oracle import round_to, sdpa_ref
from prefill_split_ref import key_tiles, prefill_split_ref, resolved_splits

pytestmark = pytest.mark.gpu

TOL = {"fp16": 2e-3, "bf16": 1.6e-2}            # tests/test_prefill_gpu.py::TOL
LSE_TOL = 2e-3                                  # tests/test_prefill_gpu.py::LSE_TOL["exact"]
TDT = {"fp16": torch.float16, "bf16": torch.bfloat16}
NAN16 = {"fp16": 0x7E00, "bf16": 0x7FC0}
DEV = "cuda:0"


@pytest.fixture(scope="module")
def sfa():
    assert torch.cuda.is_available(), "GPU tests need a GPU (run with -m gpu on the MI355X box)"
    import starflashattention_amd as m
    m._lib.load()
    return m


def dev16(x, dtype):
    return torch.from_numpy(np.array(x, order="C")).to(TDT[dtype]).to(DEV)          # (a copy: the shared problems are read-only)


def split_call(sfa, tq, tk, tv, causal, S, **kw):
    """flash_attn_split_fwd(return_lse=True) on device tensors; asserts that the call resolved S as documented"""
    o, lse = sfa.flash_attn_split_fwd(tq, tk, tv, causal=causal, num_splits=S, return_lse=True, **kw)
    torch.cuda.synchronize()
    assert sfa.debug_get("last_prefill_splits") == resolved_splits(tk.shape[2], S), (S, sfa.debug_get("last_prefill_splits"))
    return o, lse


def run(sfa, q, k, v, dtype, causal, S, **kw):
    """numpy in -> (o float32 numpy, lse float32 numpy, o as the 16-bit device tensor)"""
    o, lse = split_call(sfa, dev16(q, dtype), dev16(k, dtype), dev16(v, dtype), causal, S, **kw)
    return o.float().cpu().numpy(), lse.cpu().numpy(), o


@functools.lru_cache(maxsize=None)
def problem(shape, dtype, scale=None):
    """(q, k, v) rounded to dtype and the fp64 reference (o, lse): computed once per (shape, dtype, scale), shared, never
    written to"""
    B, Hq, Hkv, Sq, Sk, D, causal = shape
    rng = np.random.default_rng(abs(hash(shape)) % (2 ** 31))
    q = round_to(rng.standard_normal((B, Hq, Sq, D)), dtype)
    k = round_to(rng.standard_normal((B, Hkv, Sk, D)), dtype)
    v = round_to(rng.standard_normal((B, Hkv, Sk, D)), dtype)
    o, lse = sdpa_ref(q, k, v, causal=causal, scale=scale, return_lse=True)
    for a in (q, k, v, o, lse):
        a.setflags(write=False)
    return q, k, v, o, lse


def check(o, lse, want, lse_want, dtype):
    np.testing.assert_allclose(o, want, atol=TOL[dtype], rtol=TOL[dtype])
    fin = np.isfinite(lse_want)
    np.testing.assert_allclose(lse[fin], lse_want[fin], atol=LSE_TOL, rtol=LSE_TOL)
    assert np.all(lse[~fin] == -np.inf)
    assert np.all(o[~fin] == 0)


# ---- 1. parity ----
# (B, Hq, Hkv, Sq, Sk, D, causal), the split counts
SHAPES = [
    ((1, 1, 1, 1, 1, 128, True), (2,)),             # one tile, fewer tiles than splits
    ((1, 2, 1, 64, 257, 64, False), (2, 3, 5)),     # five tiles, the last holds one key, alone in a split at S = 5
    ((1, 2, 2, 300, 300, 128, True), (2, 4, 8)),    # two q-tiles of 4 and 5 tiles; rows 0-31 see tile 0 only: later splits
                                                    # are empty for some waves of a non-empty workgroup
    ((2, 4, 2, 100, 1000, 128, True), (4, 7)),      # Sq < Sk, 16 tiles, 7 does not divide
    ((1, 1, 1, 333, 100, 128, True), (2,)),         # 233 rows without a key
    ((1, 8, 1, 513, 513, 64, True), (3,)),          # GQA 8, a one-row third q-tile
    ((1, 2, 1, 257, 1025, 128, False), (4,)),       # 17 tiles, ragged by one key, a one-row second q-tile
]
SHAPE3, SHAPE_SQ_GT_SK = SHAPES[2][0], SHAPES[4][0]
PARITY = [(shape, S) for shape, counts in SHAPES for S in counts]


def shape_id(x):
    return "x".join(map(str, x[:6])) + ("-causal" if x[6] else "-full") if isinstance(x, tuple) else str(x)


@pytest.mark.parametrize("shape,S", PARITY, ids=shape_id)
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_parity(sfa, shape, S, dtype):
    q, k, v, want, lse_want = problem(shape, dtype)
    o, lse, _ = run(sfa, q, k, v, dtype, shape[6], S)
    check(o, lse, want, lse_want, dtype)
    Sq, Sk = shape[3], shape[4]
    if shape[6] and Sq > Sk:
        assert np.all(lse[:, :, :Sq - Sk] == -np.inf)


def test_reference_of_the_partition_agrees(sfa):
    """prefill_split_ref -- partials over exactly the documented tile ranges, merged by the combine's formula -- is what
    the parity above compares against, to fp64 rounding (one shape here; all of them in tests/test_prefill_split_cpu.py)"""
    q, k, v, want, lse_want = problem(SHAPE3, "bf16")
    o, lse = prefill_split_ref(q, k, v, True, 4)
    np.testing.assert_allclose(o, want, rtol=0, atol=1e-6)
    np.testing.assert_allclose(lse, lse_want, rtol=0, atol=1e-5)
    got, got_lse, _ = run(sfa, q, k, v, "bf16", True, 4)
    check(got, got_lse, o, lse, "bf16")


# ---- 2. exact count at the seams ----
ULP2 = {"bf16": 2.0 ** -7, "fp16": 2.0 ** -10}  # 2 ulp of the 16-bit type


@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
@pytest.mark.parametrize("Sq,Sk", [(300, 300), (100, 333)])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_exact_count_at_the_seams(sfa, causal, Sq, Sk, D, dtype):
    """The construction of tests/test_prefill_window_gpu.py::test_exact_window_count without a window: q = 0, so every
    score is 0 and every weight 1; V row j is the unit vector of j % D.  Every partial sum is an exact integer, every
    reference max is 0 and every merge weight 2^0, so o[i, d] = c_i(d) / cnt_i is one fp32 division of exact integers
    (as a product with the reciprocal) rounded once to 16 bit, and lse = log cnt_i: a tile dropped or counted twice at a
    split seam moves an element by a whole 1 / cnt.  rtol 2 ulp of the type, atol 1e-6; lse to 1e-5."""
    Hq, Hkv = 2, 1
    rng = np.random.default_rng(11)
    q = np.zeros((1, Hq, Sq, D))
    k = round_to(rng.standard_normal((1, Hkv, Sk, D)), dtype)
    v = np.zeros((1, Hkv, Sk, D))
    v[0, 0, np.arange(Sk), np.arange(Sk) % D] = 1.0
    tq, tk, tv = dev16(q, dtype), dev16(k, dtype), dev16(v, dtype)
    onehot = np.zeros((Sk, D))
    onehot[np.arange(Sk), np.arange(Sk) % D] = 1.0
    mask = np.ones((Sq, Sk), bool)
    if causal:
        mask = np.arange(Sk)[None, :] <= np.arange(Sq)[:, None] + (Sk - Sq)
    cnt = mask.sum(axis=1).astype(np.float64)
    assert cnt.min() >= 1
    want = (mask.astype(np.float64) @ onehot) / cnt[:, None]           # [Sq, D]
    for S in (2, 3, 5, 6):
        o, lse = split_call(sfa, tq, tk, tv, causal, S)
        o, lse = o.float().cpu().numpy(), lse.cpu().numpy()
        print(f"causal={causal} Sq={Sq} Sk={Sk} D={D} {dtype} S={S}: max |o - want| = {np.abs(o - want[None, None]).max():.3e}, "
              f"max |lse - want| = {np.abs(lse - np.log(cnt)[None, None]).max():.3e}")
        for h in range(Hq):
            np.testing.assert_allclose(o[0, h], want, rtol=ULP2[dtype], atol=1e-6, err_msg=f"S {S} head {h}")
            np.testing.assert_allclose(lse[0, h], np.log(cnt), rtol=0, atol=1e-5, err_msg=f"S {S} head {h}")


# ---- 3. a dominant key per split ----
@pytest.mark.parametrize("kind", ["spike", "alone"])
@pytest.mark.parametrize("Sq,Sk", [(299, 299), (100, 299)])
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_dominant_key_in_a_later_split(sfa, kind, Sq, Sk, dtype):
    """prefill_cases.softmax_stress: one key j* carries all the weight of the rows that see it, a case per (batch, kv
    head) with j* on every tile edge -- for S = 2 (tiles [0, 3) and [3, 5)) and S = 5 (a tile each) most of them in a split
    other than the first.  Within its split the key's weight packs to 1.0 and every other is at most 2^-40 of it
    (tests/test_prefill_numerics_gpu.py::test_softmax_stress); the other splits' maxima lie 46 or more log2 units below,
    so their merge weights are at most 2^-46 and the row returns the bits of V[j*]."""
    D, G = 128, 1
    p = pc.softmax_stress(kind, dtype, D, G, Sq, Sk)
    tq, tk, tv = pc.device_inputs(p)
    assert (p.spike >= 192).any() and (p.spike >= 64).sum() > (p.spike < 64).sum()
    for causal in (False, True):
        want, lse_want = p.oracle(causal)
        sees = np.repeat(p.sees(causal), G, axis=1)                                 # [B, Hq, Sq]
        vrow = np.repeat(pc.v_bits(p)[np.arange(p.B)[:, None], np.arange(p.Hkv)[None, :], p.spike], G, axis=1)
        for S in (2, 5):
            o, lse = split_call(sfa, tq, tk, tv, causal, S)
            check(o.float().cpu().numpy(), lse.cpu().numpy(), want, lse_want, dtype)
            bits = o.view(torch.int16).cpu().numpy().view(np.uint16)
            np.testing.assert_array_equal(bits[sees], np.broadcast_to(vrow[:, :, None, :], bits.shape)[sees],
                                          err_msg=f"{kind} causal={causal} S={S}: a row that sees key j* must return V[j*]")
            assert sees.any() or (kind == "alone" and causal)


@pytest.mark.parametrize("Sq,Sk", [(299, 299), (100, 299)])
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_staircase_between_splits(sfa, Sq, Sk, dtype):
    """staircase64: the row maxima rise by tens of log2 units from one 64-key tile to the next, so the splits' reference
    maxima differ by that much and all but the last merge weight underflow towards 0: parity at TOL."""
    p = pc.softmax_stress("staircase64", dtype, 128, 1, Sq, Sk)
    tq, tk, tv = pc.device_inputs(p)
    for causal in (False, True):
        want, lse_want = p.oracle(causal)
        for S in (2, 5):
            o, lse = split_call(sfa, tq, tk, tv, causal, S)
            check(o.float().cpu().numpy(), lse.cpu().numpy(), want, lse_want, dtype)


# ---- 4. the contents of the workspace never matter ----
@pytest.mark.parametrize("shape,S", [(SHAPE3, 2), (SHAPE3, 4), (SHAPE3, 8), (SHAPE_SQ_GT_SK, 2)], ids=shape_id)
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_workspace_contents_never_matter(sfa, shape, S, dtype):
    """The same call over a workspace of 0x00 bytes and one of 0xFF bytes (NaN in every float): bit-identical o and lse.
    A partial that nobody wrote must not be read, and an empty one must be skipped, not multiplied by 0 (0 * NaN is NaN)."""
    B, Hq, Hkv, Sq, Sk, D, causal = shape
    q, k, v, want, lse_want = problem(shape, dtype)
    tq, tk, tv = dev16(q, dtype), dev16(k, dtype), dev16(v, dtype)
    need = sfa.prefill_split_workspace_bytes(B, Hq, Sq, Sk, D, causal=causal, num_splits=S)
    assert need > 0
    outs = []
    for fill in (0x00, 0xFF):
        ws = torch.full((need,), fill, dtype=torch.uint8, device=DEV)
        o, lse = split_call(sfa, tq, tk, tv, causal, S, workspace=ws)
        outs.append((o.view(torch.int16).cpu(), lse.cpu()))
    assert torch.equal(outs[0][0], outs[1][0])
    assert torch.equal(outs[0][1], outs[1][1])          # (-inf == -inf; a NaN would differ from itself)
    check(outs[1][0].view(TDT[dtype]).float().numpy(), outs[1][1].numpy(), want, lse_want, dtype)
    # one byte short of the sizing function's answer: refused, nothing launched
    with pytest.raises(sfa.SfaError, match="sfa_prefill_split_fwd: workspace has") as e:
        sfa.flash_attn_split_fwd(tq, tk, tv, causal=causal, num_splits=S, workspace=ws[:need - 1])
    assert e.value.status == -5


# ---- 5. never read, never written ----
@pytest.mark.parametrize("shape,S", [(SHAPE3, 4), (SHAPES[1][0], 5), (SHAPES[6][0], 4), (SHAPES[3][0], 7)], ids=shape_id)
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_guarded_views(sfa, shape, S, dtype):
    """q, K, V are views inside NaN-filled allocations (prefill_cases.guarded: NaN between the rows, in guard rows before
    row 0 and past Sk, between heads and batches); o is a view inside a NaN-filled one.  The result is the contiguous
    call's bit for bit, and nothing outside o's view changes."""
    B, Hq, Hkv, Sq, Sk, D, causal = shape
    q, k, v, want, lse_want = problem(shape, dtype)
    tq, tk, tv = dev16(q, dtype), dev16(k, dtype), dev16(v, dtype)
    o0, lse0 = split_call(sfa, tq, tk, tv, causal, S)
    nan = NAN16[dtype]
    _, gq = pc.guarded(tq, pc.GUARD_Q, nan)
    _, gk = pc.guarded(tk, pc.GUARD_K, nan)
    _, gv = pc.guarded(tv, pc.GUARD_K, nan)
    o_base, go = pc.guarded(tq, pc.GUARD_Q, nan, copy=False)
    o, lse = split_call(sfa, gq, gk, gv, causal, S, out=go)
    assert o.data_ptr() == go.data_ptr()
    assert torch.equal(o.contiguous().view(torch.int16), o0.view(torch.int16))
    assert torch.equal(lse, lse0)
    assert np.all(pc.outside(o_base, pc.GUARD_Q, Sq, D) == nan)
    check(o0.float().cpu().numpy(), lse0.cpu().numpy(), want, lse_want, dtype)


def test_permuted_inputs_and_head_stride_zero(sfa):
    """q, k, v as permuted views of [B, S, H, D] storage; then K / V with a head stride of 0 (one kv head's rows serving
    every kv head)."""
    torch.manual_seed(3)
    B, Hq, Hkv, Sq, Sk, D, S = 2, 4, 2, 200, 333, 128, 3
    q = torch.randn(B, Sq, Hq, D, device=DEV).bfloat16()
    k = torch.randn(B, Sk, Hkv, D, device=DEV).bfloat16()
    v = torch.randn(B, Sk, Hkv, D, device=DEV).bfloat16()
    qt, kt, vt = q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2)
    o, lse = split_call(sfa, qt, kt, vt, True, S)
    o2, lse2 = split_call(sfa, qt.contiguous(), kt.contiguous(), vt.contiguous(), True, S)
    assert torch.equal(o.view(torch.int16), o2.view(torch.int16)) and torch.equal(lse, lse2)
    want, lse_want = sdpa_ref(*(t.float().cpu().numpy() for t in (qt, kt, vt)), causal=True, return_lse=True)
    check(o.float().cpu().numpy(), lse.cpu().numpy(), want, lse_want, "bf16")
    # head stride 0
    k0, v0 = kt[:, :1].contiguous(), vt[:, :1].contiguous()
    ke, ve = k0.expand(B, Hkv, Sk, D), v0.expand(B, Hkv, Sk, D)
    assert ke.stride(1) == 0 and ve.stride(1) == 0
    for causal in (False, True):
        o3, lse3 = split_call(sfa, qt, ke, ve, causal, S)
        o4, lse4 = split_call(sfa, qt, ke.contiguous(), ve.contiguous(), causal, S)
        assert torch.equal(o3.view(torch.int16), o4.view(torch.int16)) and torch.equal(lse3, lse4)
    want, lse_want = sdpa_ref(qt.float().cpu().numpy(), k0.float().cpu().numpy(), v0.float().cpu().numpy(), causal=True,
                              return_lse=True)
    check(o3.float().cpu().numpy(), lse3.cpu().numpy(), want, lse_want, "bf16")


# ---- 6. forwarding and the resolved count ----
@pytest.mark.parametrize("shape", [(1, 8, 8, 1024, 1024, 128), (1, 2, 1, 257, 257, 64)], ids=lambda c: "x".join(map(str, c)))
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
def test_one_split_is_the_unsplit_call(sfa, shape, causal):
    B, Hq, Hkv, Sq, Sk, D = shape
    torch.manual_seed(5)
    q = torch.randn(B, Hq, Sq, D, device=DEV).bfloat16()
    k = torch.randn(B, Hkv, Sk, D, device=DEV).bfloat16()
    v = torch.randn(B, Hkv, Sk, D, device=DEV).bfloat16()
    for fast in (False, True):
        want = sfa.flash_attn_fwd(q, k, v, causal=causal, fast_scale=fast)
        torch.cuda.synchronize()
        ran = sfa.debug_get("last_prefill_kernel")
        assert ran > 0
        sfa.flash_attn_fwd(q[:, :, :1], k[:, :, :1], v[:, :, :1], causal=not causal, fast_scale=not fast)   # another kernel in between
        o = sfa.flash_attn_split_fwd(q, k, v, causal=causal, num_splits=1, fast_scale=fast, workspace=None)
        torch.cuda.synchronize()
        assert sfa.debug_get("last_prefill_splits") == 1
        assert sfa.debug_get("last_prefill_kernel") == ran, fast
        assert torch.equal(o.view(torch.int16), want.view(torch.int16)), fast
    want, lse_want = sfa.flash_attn_fwd(q, k, v, causal=causal, return_lse=True)
    torch.cuda.synchronize()
    ran = sfa.debug_get("last_prefill_kernel")
    o, lse = sfa.flash_attn_split_fwd(q, k, v, causal=causal, num_splits=1, return_lse=True,
                                      workspace=torch.empty(0, dtype=torch.uint8, device=DEV))
    torch.cuda.synchronize()
    assert sfa.debug_get("last_prefill_splits") == 1 and sfa.debug_get("last_prefill_kernel") == ran
    assert torch.equal(o.view(torch.int16), want.view(torch.int16)) and torch.equal(lse, lse_want)
    # the split kernels leave last_prefill_kernel alone
    sfa.flash_attn_split_fwd(q, k, v, causal=causal, num_splits=2)
    torch.cuda.synchronize()
    assert sfa.debug_get("last_prefill_splits") == 2 and sfa.debug_get("last_prefill_kernel") == ran


def test_resolved_counts(sfa):
    # an explicit count above the number of key tiles resolves to that number
    shape = SHAPES[1][0]
    q, k, v, want, lse_want = problem(shape, "bf16")
    assert key_tiles(shape[4]) == 5
    for S in (6, 9, 1000):
        o, lse, _ = run(sfa, q, k, v, "bf16", False, S)
        assert sfa.debug_get("last_prefill_splits") == 5
        check(o, lse, want, lse_want, "bf16")
    # auto on a grid of 256 q-tiles (the smallest: B * Hq = 256, Sq = 1): 1, the unsplit call
    B, Hq, Sk, D = 2, 128, 1024, 64
    assert sfa.prefill_auto_splits(B, Hq, 1, Sk, D) == 1
    torch.manual_seed(9)
    tq = torch.randn(B, Hq, 1, D, device=DEV).half()
    tk = torch.randn(B, Hq, Sk, D, device=DEV).half()
    tv = torch.randn(B, Hq, Sk, D, device=DEV).half()
    o = sfa.flash_attn_split_fwd(tq, tk, tv, num_splits=0)
    o1 = sfa.flash_attn_fwd(tq, tk, tv)
    torch.cuda.synchronize()
    assert sfa.debug_get("last_prefill_splits") == 1
    assert torch.equal(o.view(torch.int16), o1.view(torch.int16))
    # auto on a small grid with a long key range splits, and a workspace that holds fewer splits gets what it holds
    B, Hq, Sq, Sk, D = 1, 2, 64, 8192, 64
    auto = sfa.prefill_auto_splits(B, Hq, Sq, Sk, D)
    assert 2 < auto <= key_tiles(Sk)
    shape = (B, Hq, 1, Sq, Sk, D, False)
    q, k, v, want, lse_want = problem(shape, "fp16")
    tq, tk, tv = dev16(q, "fp16"), dev16(k, "fp16"), dev16(v, "fp16")
    o, lse = sfa.flash_attn_split_fwd(tq, tk, tv, num_splits=0, return_lse=True)
    torch.cuda.synchronize()
    assert sfa.debug_get("last_prefill_splits") == auto
    check(o.float().cpu().numpy(), lse.cpu().numpy(), want, lse_want, "fp16")
    ws = torch.empty(sfa.prefill_split_workspace_bytes(B, Hq, Sq, Sk, D, num_splits=2), dtype=torch.uint8, device=DEV)
    o, lse = sfa.flash_attn_split_fwd(tq, tk, tv, num_splits=-1, return_lse=True, workspace=ws)
    torch.cuda.synchronize()
    assert sfa.debug_get("last_prefill_splits") == 2
    check(o.float().cpu().numpy(), lse.cpu().numpy(), want, lse_want, "fp16")
    o = sfa.flash_attn_split_fwd(tq, tk, tv, num_splits=0, workspace=ws[:256])
    torch.cuda.synchronize()
    assert sfa.debug_get("last_prefill_splits") == 1


def test_no_keys(sfa):
    """seqlen_k == 0 through the C ABI (an empty torch tensor has no data pointer to pass): every row is empty, zeros
    and lse = -inf, whatever the split count; the workspace may be NULL."""
    import ctypes
    lib = sfa._lib.load()
    q = torch.randn(1, 2, 40, 64, device=DEV).half()
    kv = torch.randn(1, 1, 8, 64, device=DEV).half()
    for S in (4, 0):
        o = torch.full_like(q, 7.0)
        lse = torch.full((1, 2, 40), 7.0, dtype=torch.float32, device=DEV)
        a = sfa._lib.PrefillArgs()
        a.q, a.k, a.v, a.o, a.lse = q.data_ptr(), kv.data_ptr(), kv.data_ptr(), o.data_ptr(), lse.data_ptr()
        a.batch, a.heads_q, a.heads_kv, a.seqlen_q, a.seqlen_k, a.head_dim = 1, 2, 1, 40, 0, 64
        for dst, t in ((a.q_stride, q), (a.k_stride, kv), (a.v_stride, kv), (a.o_stride, o)):
            dst[0], dst[1], dst[2] = t.stride(0), t.stride(1), t.stride(2)
        a.causal, a.dtype = 1, sfa._lib.DTYPE_FP16
        st = lib.sfa_prefill_split_fwd(ctypes.byref(a), S, None, 0, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert st == 0, lib.sfa_last_error()
        torch.cuda.synchronize()
        assert sfa.debug_get("last_prefill_splits") == 1
        assert torch.all(o == 0) and torch.all(lse == -float("inf"))


# ---- 7. softmax_scale ----
@pytest.mark.parametrize("scale", pc.SCALES)
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_softmax_scale(sfa, scale, dtype):
    shape = SHAPES[3][0]
    q, k, v, want, lse_want = problem(shape, dtype, scale)
    for S in (4, 7):
        o, lse, _ = run(sfa, q, k, v, dtype, shape[6], S, softmax_scale=scale)
        check(o, lse, want, lse_want, dtype)


# ---- 8. graph ----
def test_graph_replay(sfa):
    """One captured split call (S = 3) on a side stream -- two launches, no parallel branches -- replayed with new
    contents of q, k, v."""
    dtype, S = "bf16", 3
    B, Hq, Hkv, Sq, Sk, D, causal = SHAPE3
    tq = torch.zeros(B, Hq, Sq, D, dtype=TDT[dtype], device=DEV)
    tk = torch.zeros(B, Hkv, Sk, D, dtype=TDT[dtype], device=DEV)
    tv = torch.zeros_like(tk)
    out = torch.zeros_like(tq)
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        sfa.flash_attn_split_fwd(tq, tk, tv, causal=causal, num_splits=S, out=out)     # warm-up: the stream's workspace exists
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            _, lse = sfa.flash_attn_split_fwd(tq, tk, tv, causal=causal, num_splits=S, out=out, return_lse=True)
        assert sfa.debug_get("last_prefill_splits") == S
        for seed in (1, 2):
            rng = np.random.default_rng(seed)
            q = round_to(rng.standard_normal((B, Hq, Sq, D)), dtype)
            k = round_to(rng.standard_normal((B, Hkv, Sk, D)), dtype)
            v = round_to(rng.standard_normal((B, Hkv, Sk, D)), dtype)
            want, lse_want = sdpa_ref(q, k, v, causal=causal, return_lse=True)
            for dst, src in ((tq, q), (tk, k), (tv, v)):
                dst.copy_(dev16(src, dtype))
            out.fill_(7.0)
            graph.replay()
            side.synchronize()
            check(out.float().cpu().numpy(), lse.cpu().numpy(), want, lse_want, dtype)


# ---- 9. the operator's argument errors, and the pybind surface ----
def test_argument_errors(sfa):
    q = torch.zeros(1, 4, 16, 128, device=DEV, dtype=torch.bfloat16)
    kv = torch.zeros(1, 2, 300, 128, device=DEV, dtype=torch.bfloat16)
    sfa.flash_attn_split_fwd(q, kv, kv, num_splits=2)
    with pytest.raises(RuntimeError, match="num_splits"):
        sfa.flash_attn_split_fwd(q, kv, kv, num_splits=2.5)
    with pytest.raises(RuntimeError, match="workspace"):
        sfa.flash_attn_split_fwd(q, kv, kv, num_splits=2, workspace=torch.zeros(1 << 20, dtype=torch.float32, device=DEV))
    with pytest.raises(RuntimeError, match="workspace"):
        sfa.flash_attn_split_fwd(q, kv, kv, num_splits=2, workspace=torch.zeros(1 << 20, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="dtype"):
        sfa.flash_attn_split_fwd(q, kv.half(), kv, num_splits=2)
    ws = torch.zeros((1 << 20) + 256, dtype=torch.uint8, device=DEV)
    with pytest.raises(sfa.SfaError, match="sfa_prefill_split_fwd: workspace must be 256-byte aligned") as e:
        sfa.flash_attn_split_fwd(q, kv, kv, num_splits=2, workspace=ws[16:])
    assert e.value.status == -2
    with pytest.raises(sfa.SfaError, match="sfa_prefill_split_fwd: workspace is NULL") as e:
        sfa.flash_attn_split_fwd(q, kv, kv, num_splits=2, workspace=ws[:0])
    assert e.value.status == -1
    z = torch.zeros(1, 2, 16, 256, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(sfa.SfaError, match="sfa_prefill_split_fwd: head_dim 256") as e:
        sfa.flash_attn_split_fwd(z, z, z, num_splits=2)
    assert e.value.status == -4
    torch.cuda.synchronize()


def test_pybind_mha_fwd_split(sfa):
    import star_flash_attn as ext
    dtype = "bf16"
    q, k, v, want, lse_want = problem(SHAPE3, dtype)
    tq, tk, tv = dev16(q, dtype), dev16(k, dtype), dev16(v, dtype)
    out, lse = ext.mha_fwd_split(tq, tk, tv, causal=True, num_splits=4, return_lse=True)
    torch.cuda.synchronize()
    assert sfa.debug_get("last_prefill_splits") == resolved_splits(300, 4) == 3        # five tiles in chunks of two
    check(out.float().cpu().numpy(), lse.cpu().numpy(), want, lse_want, dtype)
    o2 = sfa.flash_attn_split_fwd(tq, tk, tv, causal=True, num_splits=4)
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int16), o2.view(torch.int16))
    (o3,) = ext.mha_fwd_split(tq, tk, tv, causal=True)          # the library's choice
    torch.cuda.synchronize()
    assert sfa.debug_get("last_prefill_splits") == sfa.prefill_auto_splits(1, 2, 300, 300, 128, causal=True)
    check(o3.float().cpu().numpy(), lse_want, want, lse_want, dtype)
    with pytest.raises(RuntimeError, match="head_dim 256"):
        z = torch.zeros(1, 2, 16, 256, device=DEV, dtype=torch.bfloat16)
        ext.mha_fwd_split(z, z, z, num_splits=2)
