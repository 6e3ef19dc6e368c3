"""GPU tests of sfa_prefill_window_fwd / flash_attn_window_fwd / mha_fwd_window: the prefill forward with a sliding window
and attention sinks, against the fp64 reference of tests/prefill_window_ref.py on identically rounded inputs.

Tolerances: o within the project's TOL (fp16 2e-3, bf16 1.6e-2: tests/test_prefill_gpu.py::TOL), lse within 2e-3
(LSE_TOL["exact"] of tests/test_prefill_gpu.py; the windowed kernel is an exact-scale kernel).  The shapes are the smallest
that reach each edge of a 64-key tile, a 32-row wave block and the 256-row q-tile."""
import functools

import numpy as np
import pytest
import torch

from oracle import round_to
from prefill_window_ref import prefill_window_ref, visible_counts, window_mask
from sinks_ref import deltas

pytestmark = pytest.mark.gpu

TOL = {"fp16": 2e-3, "bf16": 1.6e-2}            # tests/test_prefill_gpu.py::TOL
LSE_TOL = 2e-3                                  # tests/test_prefill_gpu.py::LSE_TOL["exact"]
TDT = {"fp16": torch.float16, "bf16": torch.bfloat16}
DEV = "cuda:0"
INT_MAX = 2 ** 31 - 1


@pytest.fixture(scope="module")
def sfa():
    assert torch.cuda.is_available(), "GPU tests need a GPU (run with -m gpu on the MI355X box)"
    import starflashattention_amd as m
    m._lib.load()
    return m


def dev16(x, dtype):
    return torch.from_numpy(np.array(x, order="C")).to(TDT[dtype]).to(DEV)          # (a copy: the shared problems are read-only)


def dev_sinks(sinks):
    return None if sinks is None else torch.from_numpy(np.array(sinks, np.float32)).to(DEV)


def run(sfa, q, k, v, dtype, window, sinks=None):
    """numpy in -> (o float32 numpy, lse float32 numpy, o as the 16-bit device tensor)"""
    o, lse = sfa.flash_attn_window_fwd(dev16(q, dtype), dev16(k, dtype), dev16(v, dtype), window, sinks=dev_sinks(sinks),
                                       return_lse=True)
    torch.cuda.synchronize()
    return o.float().cpu().numpy(), lse.cpu().numpy(), o


@functools.lru_cache(maxsize=None)
def problem(case, dtype):
    """(q, k, v) rounded to dtype, the no-sink reference (o, lse) and sinks of material weight for every head:
    sinks[h] = lse_nosink[anchor, h] + delta_h, delta spread over [-3, 3], anchor = the last row of batch 0.  Computed once
    per (case, dtype) and shared; nobody writes to it."""
    B, Hq, Hkv, Sq, Sk, D, window = case
    rng = np.random.default_rng(abs(hash(case)) % (2 ** 31))
    q = round_to(rng.standard_normal((B, Hq, Sq, D)), dtype)
    k = round_to(rng.standard_normal((B, Hkv, Sk, D)), dtype)
    v = round_to(rng.standard_normal((B, Hkv, Sk, D)), dtype)
    o0, lse0 = prefill_window_ref(q, k, v, window)
    sinks = (lse0[0, :, Sq - 1].astype(np.float64) + deltas(Hq)).astype(np.float32)
    for a in (q, k, v, o0, lse0, sinks):
        a.setflags(write=False)
    return q, k, v, o0, lse0, sinks


def check(o, lse, want, lse_want, dtype):
    np.testing.assert_allclose(o, want, atol=TOL[dtype], rtol=TOL[dtype])
    fin = np.isfinite(lse_want)
    np.testing.assert_allclose(lse[fin], lse_want[fin], atol=LSE_TOL, rtol=LSE_TOL)
    assert np.all(lse[~fin] == -np.inf)
    assert np.all(o[~fin] == 0)


# ---- 1. parity ----
CASES = [
    (1, 1, 1, 1, 1, 128, 1),
    (2, 3, 3, 64, 64, 128, 17),
    (1, 2, 1, 257, 257, 128, 64),
    (1, 2, 1, 257, 257, 128, 65),
    (1, 4, 2, 300, 300, 64, 63),
    (2, 2, 2, 513, 513, 64, 200),
    (1, 2, 2, 100, 333, 128, 150),
    (1, 2, 2, 100, 333, 128, 500),
    (1, 1, 1, 333, 100, 128, 40),      # the first 233 rows see no key: zeros and lse = -inf
    (1, 8, 1, 600, 600, 64, 128),
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("with_sinks", [False, True], ids=["nosink", "sinks"])
def test_parity(sfa, case, dtype, with_sinks):
    q, k, v, o0, lse0, sinks = problem(case, dtype)
    window = case[6]
    if with_sinks:
        want, lse_want = prefill_window_ref(q, k, v, window, sinks=sinks.astype(np.float64))
    else:
        want, lse_want, sinks = o0, lse0, None
    o, lse, _ = run(sfa, q, k, v, dtype, window, sinks)
    check(o, lse, want, lse_want, dtype)
    if case[3] > case[4]:
        assert np.all(lse[:, :, :case[3] - case[4]] == -np.inf)


# ---- 2. exact window count ----
WINDOWS = [1, 2, 63, 64, 65, 127, 128, 129, 300]
ULP2 = {"bf16": 2.0 ** -7, "fp16": 2.0 ** -10}  # 2 ulp of the 16-bit type


@pytest.mark.parametrize("Sq,Sk", [(300, 300), (100, 333)])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("with_sink", [True, False], ids=["sink0", "nosink"])
def test_exact_window_count(sfa, Sq, Sk, D, dtype, with_sink):
    """q = 0, so every score is 0 and every weight 1; V row j is the unit vector of j % D.  Then o[i, d] =
    c_i(d) / (cnt_i + 1) with a sink of logit 0 (weight exactly 1), c_i(d) / cnt_i without, and lse = log of the
    denominator: one key too many or too few at either edge of any row moves an element by a whole 1 / denominator.  The
    value is one fp32 division of exact integers, rounded once to 16 bit: rtol 2 ulp of the type, atol 1e-6."""
    Hq, Hkv = 2, 1
    rng = np.random.default_rng(11)
    q = np.zeros((1, Hq, Sq, D))
    k = round_to(rng.standard_normal((1, Hkv, Sk, D)), dtype)
    v = np.zeros((1, Hkv, Sk, D))
    v[0, 0, np.arange(Sk), np.arange(Sk) % D] = 1.0
    tq, tk, tv = dev16(q, dtype), dev16(k, dtype), dev16(v, dtype)
    sinks = torch.zeros(Hq, dtype=torch.float32, device=DEV) if with_sink else None
    onehot = np.zeros((Sk, D))
    onehot[np.arange(Sk), np.arange(Sk) % D] = 1.0
    for window in WINDOWS:
        o, lse = sfa.flash_attn_window_fwd(tq, tk, tv, window, sinks=sinks, return_lse=True)
        torch.cuda.synchronize()
        o, lse = o.float().cpu().numpy(), lse.cpu().numpy()
        mask = window_mask(Sq, Sk, window)
        cnt = visible_counts(Sq, Sk, window).astype(np.float64)
        assert cnt.min() >= 1
        den = cnt + (1.0 if with_sink else 0.0)
        want = (mask.astype(np.float64) @ onehot) / den[:, None]           # [Sq, D]
        print(f"Sq={Sq} Sk={Sk} D={D} {dtype} window={window}: max |o - want| = {np.abs(o - want[None, None]).max():.3e}, "
              f"max |lse - want| = {np.abs(lse - np.log(den)[None, None]).max():.3e}")
        for h in range(Hq):
            np.testing.assert_allclose(o[0, h], want, rtol=ULP2[dtype], atol=1e-6, err_msg=f"window {window} head {h}")
            np.testing.assert_allclose(lse[0, h], np.log(den), rtol=0, atol=1e-5, err_msg=f"window {window} head {h}")


# ---- 3. never read ----
@pytest.mark.parametrize("case", [(1, 2, 1, 100, 333, 128, 150), (1, 2, 1, 100, 333, 128, 64), (1, 2, 2, 256, 1024, 64, 64)],
                         ids=lambda c: "x".join(map(str, c)))
@pytest.mark.parametrize("with_sinks", [False, True], ids=["nosink", "sinks"])
def test_rows_below_the_window_are_never_read(sfa, case, with_sinks):
    """The K and V rows [0, lo_0) hold NaN in one run and Inf in another: the output is the run's with zeros there, bit
    for bit (a masked key has weight 0, but 0 * NaN is NaN in P.V: the rows must not be staged at all)."""
    B, Hq, Hkv, Sq, Sk, D, window = case
    dtype = "bf16"
    q, k, v, _, _, sinks = problem(case, dtype)
    lo0 = max(0, Sk - Sq + 1 - window)
    assert lo0 > 0 and (case != (1, 2, 2, 256, 1024, 64, 64) or lo0 == 705)
    tq, ts = dev16(q, dtype), dev_sinks(sinks if with_sinks else None)
    outs = []
    for fill in (0.0, float("nan"), float("inf")):
        tk, tv = dev16(k, dtype), dev16(v, dtype)
        tk[:, :, :lo0] = fill
        tv[:, :, :lo0] = fill
        o, lse = sfa.flash_attn_window_fwd(tq, tk, tv, window, sinks=ts, return_lse=True)
        torch.cuda.synchronize()
        outs.append((o.view(torch.int16).cpu(), lse.cpu()))
    assert torch.isfinite(outs[0][1]).all()
    for o, lse in outs[1:]:
        assert torch.equal(o, outs[0][0])
        assert torch.equal(lse, outs[0][1])
    want, lse_want = prefill_window_ref(q, k, v, window, sinks=sinks.astype(np.float64) if with_sinks else None)
    check(outs[0][0].view(torch.bfloat16).float().numpy(), outs[0][1].numpy(), want, lse_want, dtype)


# ---- 4. sink numerics ----
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("window", [100, 300, INT_MAX])
def test_underflowing_sinks_change_nothing(sfa, dtype, window):
    """Sinks whose weight underflows in fp32 (-inf, -1e30) give bit-identical outputs; under a window < Sk they equal the
    same kernel's no-sink output (sinks = None), with window >= Sk (where sinks = None forwards to the causal kernels) the
    reference within TOL."""
    case = (1, 4, 2, 300, 300, 64, 100)
    q, k, v, _, _, _ = problem(case, dtype)
    Hq, Sk = case[1], case[4]
    o_inf, lse_inf, t_inf = run(sfa, q, k, v, dtype, window, np.full(Hq, -np.inf))
    o_big, lse_big, t_big = run(sfa, q, k, v, dtype, window, np.full(Hq, -1e30))
    assert torch.equal(t_inf.view(torch.int16), t_big.view(torch.int16))
    assert np.array_equal(lse_inf, lse_big)
    if window < Sk:
        o_none, lse_none, t_none = run(sfa, q, k, v, dtype, window, None)
        assert torch.equal(t_inf.view(torch.int16), t_none.view(torch.int16))
        assert np.array_equal(lse_inf, lse_none)
    want, lse_want = prefill_window_ref(q, k, v, window)
    check(o_inf, lse_inf, want, lse_want, dtype)


def test_sink_far_above_the_scores(sfa):
    """A sink 80 above every score: finite output, no overflow.  fp16 at head_dim 64, where an fp32 overflow would show.
    The reference's values are tiny (weights <= e^-80): the output sits within rtol 1e-2 of them where their magnitude is at
    least 1e-30, and is 0 elsewhere."""
    case = (1, 4, 2, 300, 300, 64, 100)
    dtype = "fp16"
    q, k, v, _, _, _ = problem(case, dtype)
    B, Hq, Hkv, Sq, Sk, D, window = case
    smax = max(float(np.max(q[0, h].astype(np.float64) @ k[0, h // 2].astype(np.float64).T)) for h in range(Hq)) / np.sqrt(D)
    sinks = np.full(Hq, smax + 80.0)
    want, lse_want = prefill_window_ref(q, k, v, window, sinks=sinks)
    o, lse, _ = run(sfa, q, k, v, dtype, window, sinks)
    assert np.all(np.isfinite(o)) and np.all(np.isfinite(lse))
    big = np.abs(want) >= 1e-30
    print(f"sink = {sinks[0]:.2f}: max |want| = {np.abs(want).max():.3e}, elements >= 1e-30: {int(big.sum())}, "
          f"max |o| = {np.abs(o).max():.3e}")
    np.testing.assert_allclose(o[big], want[big], rtol=1e-2, atol=0)
    assert np.all(o[~big] == 0)
    np.testing.assert_allclose(lse, lse_want, atol=LSE_TOL, rtol=LSE_TOL)


# ---- 5. forwarding ----
@pytest.mark.parametrize("case", [(1, 8, 8, 1024, 1024, 128), (1, 2, 1, 257, 257, 64)], ids=lambda c: "x".join(map(str, c)))
def test_no_sink_and_full_window_is_the_causal_call(sfa, case):
    B, Hq, Hkv, Sq, Sk, D = case
    torch.manual_seed(5)
    q = torch.randn(B, Hq, Sq, D, device=DEV).bfloat16()
    k = torch.randn(B, Hkv, Sk, D, device=DEV).bfloat16()
    v = torch.randn(B, Hkv, Sk, D, device=DEV).bfloat16()
    want, lse_want = sfa.flash_attn_fwd(q, k, v, causal=True, return_lse=True)
    torch.cuda.synchronize()
    ran = sfa.debug_get("last_prefill_kernel")
    assert ran > 0
    for window in (Sk, Sk + 1, INT_MAX):
        sfa.flash_attn_fwd(q[:, :, :1], k[:, :, :1], v[:, :, :1])          # another kernel in between (full attention)
        o, lse = sfa.flash_attn_window_fwd(q, k, v, window, return_lse=True)
        torch.cuda.synchronize()
        assert sfa.debug_get("last_prefill_kernel") == ran, window
        assert torch.equal(o.view(torch.int16), want.view(torch.int16)), window
        assert torch.equal(lse, lse_want), window
    # the windowed kernel leaves last_prefill_kernel alone
    sfa.flash_attn_window_fwd(q, k, v, Sk - 1)
    sfa.flash_attn_window_fwd(q, k, v, INT_MAX, sinks=torch.zeros(Hq, dtype=torch.float32, device=DEV))
    torch.cuda.synchronize()
    assert sfa.debug_get("last_prefill_kernel") == ran


# ---- 6. strided views and out ----
def test_strided_views_and_out(sfa):
    """q, k, v are permuted views of [B, S, H, D] storage; out is a strided view into a larger NaN-filled buffer, outside
    of which nothing changes."""
    torch.manual_seed(3)
    B, Hq, Hkv, Sq, Sk, D, window = 2, 4, 2, 200, 333, 128, 70
    q = torch.randn(B, Sq, Hq, D, device=DEV).bfloat16()
    k = torch.randn(B, Sk, Hkv, D, device=DEV).bfloat16()
    v = torch.randn(B, Sk, Hkv, D, device=DEV).bfloat16()
    sinks = torch.linspace(-1.0, 4.0, Hq, device=DEV)
    store = torch.full((B, Sq + 3, Hq + 1, D), float("nan"), device=DEV, dtype=torch.bfloat16)
    out = store[:, 2:2 + Sq, :Hq].transpose(1, 2)
    o = sfa.flash_attn_window_fwd(q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2), window, sinks=sinks, out=out)
    o2, lse2 = sfa.flash_attn_window_fwd(q.transpose(1, 2).contiguous(), k.transpose(1, 2).contiguous(),
                                         v.transpose(1, 2).contiguous(), window, sinks=sinks, return_lse=True)
    torch.cuda.synchronize()
    assert o.data_ptr() == out.data_ptr()
    assert torch.equal(o.view(torch.int16), o2.view(torch.int16))
    assert torch.isnan(store[:, :2]).all() and torch.isnan(store[:, 2 + Sq:]).all() and torch.isnan(store[:, :, Hq]).all()
    assert not torch.isnan(store[:, 2:2 + Sq, :Hq]).any()
    want, lse_want = prefill_window_ref(*(t.transpose(1, 2).float().cpu().numpy() for t in (q, k, v)), window,
                                        sinks=sinks.double().cpu().numpy())
    check(o2.float().cpu().numpy(), lse2.cpu().numpy(), want, lse_want, "bf16")


# ---- 7. argument errors through ops.py ----
def test_argument_errors(sfa):
    q = torch.zeros(1, 4, 16, 128, device=DEV, dtype=torch.bfloat16)
    kv = torch.zeros(1, 2, 16, 128, device=DEV, dtype=torch.bfloat16)
    good = torch.zeros(4, dtype=torch.float32, device=DEV)
    sfa.flash_attn_window_fwd(q, kv, kv, 4, sinks=good)
    with pytest.raises(RuntimeError, match="HIP device"):
        sfa.flash_attn_window_fwd(q, kv, kv, 4, sinks=good.cpu())
    with pytest.raises(RuntimeError, match="dtype"):
        sfa.flash_attn_window_fwd(q, kv, kv, 4, sinks=good.half())
    with pytest.raises(RuntimeError, match="shape"):
        sfa.flash_attn_window_fwd(q, kv, kv, 4, sinks=torch.zeros(2, dtype=torch.float32, device=DEV))
    with pytest.raises(RuntimeError, match="window"):
        sfa.flash_attn_window_fwd(q, kv, kv, 0)
    with pytest.raises(RuntimeError, match="dtype"):
        sfa.flash_attn_window_fwd(q, kv.half(), kv, 4)
    z = torch.zeros(1, 2, 16, 256, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(sfa.SfaError, match="sfa_prefill_window_fwd: head_dim 256") as e:
        sfa.flash_attn_window_fwd(z, z, z, 4)
    assert e.value.status == -4
    torch.cuda.synchronize()


# ---- 8. pybind ----
def test_pybind_mha_fwd_window(sfa):
    import star_flash_attn as ext
    case = (1, 4, 2, 300, 300, 64, 63)
    dtype = "bf16"
    q, k, v, o0, lse0, sinks = problem(case, dtype)
    window = case[6]
    tq, tk, tv = dev16(q, dtype), dev16(k, dtype), dev16(v, dtype)
    out, lse = ext.mha_fwd_window(tq, tk, tv, window, sinks=dev_sinks(sinks), return_lse=True)
    torch.cuda.synchronize()
    want, lse_want = prefill_window_ref(q, k, v, window, sinks=sinks.astype(np.float64))
    check(out.float().cpu().numpy(), lse.cpu().numpy(), want, lse_want, dtype)
    (out2,) = ext.mha_fwd_window(tq, tk, tv, window)
    torch.cuda.synchronize()
    check(out2.float().cpu().numpy(), lse0, o0, lse0, dtype)
    o3 = sfa.flash_attn_window_fwd(tq, tk, tv, window, sinks=dev_sinks(sinks))
    assert torch.equal(out.view(torch.int16), o3.view(torch.int16))
    with pytest.raises(RuntimeError, match="window"):
        ext.mha_fwd_window(tq, tk, tv, 0)
    with pytest.raises(RuntimeError, match="sinks"):
        ext.mha_fwd_window(tq, tk, tv, 4, sinks=torch.zeros(3, dtype=torch.float32, device=DEV))
