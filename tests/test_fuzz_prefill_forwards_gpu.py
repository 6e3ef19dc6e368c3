"""Randomised sweep of the five newer prefill forwards -- flash_attn_window_fwd, flash_attn_split_fwd,
flash_attn_varlen_fwd, flash_attn_varlen_window_fwd, flash_attn_varlen_split_fwd -- 24 seeded cases each, against their
existing fp64 references on identically rounded inputs.  tests/serving_cases.py draws the cases: any
heads_q % heads_kv == 0 with group sizes 1, 2, 3, 4, 6, 8 and 1 .. 5 kv heads, Sq > Sk, empty sequences, n_q > n_k, one
invalid (backwards, or past total_k) pair, windows up to 2 Sk, sinks with an occasional -inf, every split request, a
max_seqlen_k hint that is exact or deliberately low, q / k / v contiguous or slices of one packed allocation.
tests/test_serving_model_cpu.py lists which seed reaches what.

Tolerances: o within tests/test_prefill_gpu.py::TOL, lse within its LSE_TOL["exact"] (none of these calls prescales q); a
row with no visible key holds exactly 0 and -inf; the rows of an invalid pair keep what o and lse held before the call.
"""
import ctypes

import numpy as np
import pytest
import torch

import serving_cases as sc
from prefill_split_ref import prefill_split_ref
from prefill_varlen_ref import prefill_varlen_ref
from prefill_varlen_split_ref import prefill_varlen_split_ref
from prefill_varlen_window_ref import prefill_varlen_window_ref
from prefill_window_ref import prefill_window_ref

pytestmark = pytest.mark.gpu
TOL = {"fp16": 2e-3, "bf16": 1.6e-2}            # tests/test_prefill_gpu.py::TOL
LSE_TOL = 2e-3                                  # tests/test_prefill_gpu.py::LSE_TOL["exact"]
TDT = {"fp16": torch.float16, "bf16": torch.bfloat16}
DEV = "cuda:0"
FILL = 7.0                                      # what o and lse hold before a packed call


@pytest.fixture(scope="module")
def sfa():
    assert torch.cuda.is_available(), "GPU tests need a GPU (run with -m gpu on the MI355X box)"
    import starflashattention_amd as m
    m._lib.load()
    return m


def t16(x, dtype):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(TDT[dtype]).to(DEV)


def sinks_dev(c):
    return None if c["sinks"] is None else torch.tensor(c["sinks"], dtype=torch.float32, device=DEV)


def check(c, o, lse, want, lse_want, rows=None):
    """o and lse against the reference where a row has a key, exactly 0 and -inf where it has none; rows (packed calls):
    the query rows of valid sequences, every other row holds FILL.  o [..., Hq, D]-last layouts as the references give
    them: rectangular [B, Hq, Sq, D] / [B, Hq, Sq], packed [Tq, Hq, D] / [Hq, Tq]."""
    tol = TOL[c["dtype"]]
    want, lse_want = np.asarray(want, np.float64), np.asarray(lse_want, np.float64)
    if rows is None:
        has = np.isfinite(lse_want)
        o_has, o_none, l_has, l_none = o[has], o[~has], lse[has], lse[~has]
        w_has, lw_has = want[has], lse_want[has]
    else:
        has = np.isfinite(lse_want) & rows[None, :]             # [Hq, Tq]
        none = ~np.isfinite(lse_want) & rows[None, :]
        ot, wt = o.transpose(1, 0, 2), want.transpose(1, 0, 2)  # [Hq, Tq, D]
        o_has, o_none, l_has, l_none = ot[has], ot[none], lse[has], lse[none]
        w_has, lw_has = wt[has], lse_want[has]
        assert np.all(o[~rows] == FILL) and np.all(lse[:, ~rows] == FILL), "rows of no valid sequence were written"
    assert np.isfinite(o_has).all()
    if o_has.size:
        print("max |o - ref| = %.3e (tol %.1e), max |lse - ref| = %.3e (tol %.1e)"
              % (np.abs(o_has - w_has).max(), tol, np.abs(l_has - lw_has).max(), LSE_TOL))
    np.testing.assert_allclose(o_has, w_has, atol=tol, rtol=tol)
    np.testing.assert_allclose(l_has, lw_has, atol=LSE_TOL, rtol=LSE_TOL)
    assert np.all(l_none == -np.inf) and np.all(o_none == 0), "a row with no visible key must hold 0 and -inf"


def described(c, fn):
    try:
        fn()
    except AssertionError as e:
        raise AssertionError(f"{c!r}\n{e}") from None


# ---- the rectangular calls ---------------------------------------------------------------------------------------------

def rect_tensors(c, q, k, v):
    """contiguous [B, H, S, D] tensors, or views of one [B, T, Hq + 2 Hkv, D] allocation (NaN where no operand lies)"""
    if not c["packed"]:
        return t16(q, c["dtype"]), t16(k, c["dtype"]), t16(v, c["dtype"])
    B, Hq, Hkv, Sq, Sk = c["B"], c["Hq"], c["Hkv"], c["Sq"], c["Sk"]
    buf = np.full((B, max(Sq, Sk), Hq + 2 * Hkv, c["D"]), np.nan, np.float32)
    buf[:, :Sq, :Hq] = q.transpose(0, 2, 1, 3)
    buf[:, :Sk, Hq:Hq + Hkv] = k.transpose(0, 2, 1, 3)
    buf[:, :Sk, Hq + Hkv:] = v.transpose(0, 2, 1, 3)
    t = t16(buf, c["dtype"])
    return (t[:, :Sq, :Hq].permute(0, 2, 1, 3), t[:, :Sk, Hq:Hq + Hkv].permute(0, 2, 1, 3),
            t[:, :Sk, Hq + Hkv:].permute(0, 2, 1, 3))


@pytest.mark.parametrize("seed", sc.PREFILL_SEEDS)
def test_fuzz_window_fwd(sfa, seed):
    c = sc.prefill_case("window", seed)
    q, k, v = sc.prefill_inputs(c)

    def body():
        want, lse_want = prefill_window_ref(q, k, v, c["window"], c["sinks"], c["softmax_scale"])
        o, lse = sfa.flash_attn_window_fwd(*rect_tensors(c, q, k, v), c["window"], sinks=sinks_dev(c),
                                           softmax_scale=c["softmax_scale"], return_lse=True)
        torch.cuda.synchronize()
        check(c, o.float().cpu().numpy(), lse.cpu().numpy(), want, lse_want)
    described(c, body)


@pytest.mark.parametrize("seed", sc.PREFILL_SEEDS)
def test_fuzz_split_fwd(sfa, seed):
    c = sc.prefill_case("split", seed)
    q, k, v = sc.prefill_inputs(c)

    def body():
        # the reference follows the partition of the count the call resolves to: its own choice for a request of 0
        S = c["num_splits"] or sfa.prefill_auto_splits(c["B"], c["Hq"], c["Sq"], c["Sk"], c["D"], c["causal"])
        want, lse_want = prefill_split_ref(q, k, v, c["causal"], max(S, 1), c["softmax_scale"])
        o, lse = sfa.flash_attn_split_fwd(*rect_tensors(c, q, k, v), causal=c["causal"], num_splits=c["num_splits"],
                                          softmax_scale=c["softmax_scale"], return_lse=True)
        torch.cuda.synchronize()
        check(c, o.float().cpu().numpy(), lse.cpu().numpy(), want, lse_want)
    described(c, body)


# ---- the packed calls --------------------------------------------------------------------------------------------------

def packed_tensors(c, q, k, v):
    """contiguous [T, H, D] tensors, or views of one [T, Hq + 2 Hkv, D] allocation (NaN where no operand lies)"""
    if not c["packed"]:
        return t16(q, c["dtype"]), t16(k, c["dtype"]), t16(v, c["dtype"])
    Hq, Hkv = c["Hq"], c["Hkv"]
    buf = np.full((max(q.shape[0], k.shape[0]), Hq + 2 * Hkv, c["D"]), np.nan, np.float32)
    buf[:q.shape[0], :Hq], buf[:k.shape[0], Hq:Hq + Hkv], buf[:k.shape[0], Hq + Hkv:] = q, k, v
    t = t16(buf, c["dtype"])
    return t[:q.shape[0], :Hq], t[:k.shape[0], Hq:Hq + Hkv], t[:k.shape[0], Hq + Hkv:]


def packed_call(sfa, c, q, k, v):
    """The packed call of c["kind"] with o and lse prefilled with FILL and total_k = c["total_k"] (which may be less than
    the key rows allocated: a sequence past it is skipped without leaving the allocation).  ops.py checks the tensors and
    fills the argument struct; the lse buffer and the totals are this function's own.  Returns (o, lse) as numpy."""
    ops, lib = sfa.ops, sfa._lib.load()
    tq, tk, tv = packed_tensors(c, q, k, v)
    out = torch.full(tq.shape, FILL, dtype=tq.dtype, device=DEV)
    cu_q = torch.tensor(c["cu_q"], dtype=torch.int32, device=DEV)
    cu_k = torch.tensor(c["cu_k"], dtype=torch.int32, device=DEV)
    _, a, out, _, ws, dev, W = ops._prefill_varlen_args(tq, tk, tv, cu_q, cu_k, c["causal"], c["softmax_scale"], out, False,
                                                        None, c["window"])
    lse = torch.full((c["Hq"], tq.shape[0]), FILL, dtype=torch.float32, device=DEV)
    a.lse = lse.data_ptr()
    assert a.total_k == c["alloc_k"] and c["total_k"] <= c["alloc_k"]
    a.total_k = c["total_k"]
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    ptr = lambda w: (ctypes.c_void_p(w.data_ptr()) if w is not None else None, w.numel() if w is not None else 0)
    if c["kind"] == "varlen":
        st = lib.sfa_prefill_varlen_fwd(ctypes.byref(a), *ptr(ws), stream)
    elif c["kind"] == "varlen_window":
        sinks = sinks_dev(c)
        st = lib.sfa_prefill_varlen_window_fwd(ctypes.byref(a), W, None if sinks is None else ctypes.c_void_p(sinks.data_ptr()),
                                               *ptr(ws), stream)
    else:
        need = lib.sfa_prefill_varlen_split_workspace_bytes(a.batch, a.heads_q, a.total_q, c["max_seqlen_k"], a.head_dim,
                                                            c["num_splits"])
        ws = ops._workspace(dev, ops._STATUS_BYTES + need)[ops._STATUS_BYTES:] if need else None
        st = lib.sfa_prefill_varlen_split_fwd(ctypes.byref(a), c["max_seqlen_k"], c["num_splits"], *ptr(ws), stream)
    sfa._lib.check(st)
    torch.cuda.synchronize()
    return out.float().cpu().numpy(), lse.cpu().numpy()


def packed_case(sfa, kind, seed):
    c = sc.prefill_case(kind, seed)
    q, k, v = sc.prefill_inputs(c)

    def body():
        kr, vr = k[:c["total_k"]], v[:c["total_k"]]             # the reference judges validity by the totals the call gets
        if kind == "varlen":
            want, lse_want, rows = prefill_varlen_ref(q, kr, vr, c["cu_q"], c["cu_k"], c["causal"], c["softmax_scale"])
        elif kind == "varlen_window":
            want, lse_want, rows = prefill_varlen_window_ref(q, kr, vr, c["cu_q"], c["cu_k"], c["window"], c["sinks"],
                                                             c["softmax_scale"])
        else:
            S = c["num_splits"] or sfa.prefill_varlen_auto_splits(c["B"], c["Hq"], c["total_q"], c["max_seqlen_k"], c["D"],
                                                                  c["causal"])
            want, lse_want, rows = prefill_varlen_split_ref(q, kr, vr, c["cu_q"], c["cu_k"], c["causal"], c["max_seqlen_k"],
                                                            max(S, 1), c["softmax_scale"])
        o, lse = packed_call(sfa, c, q, k, v)
        check(c, o, lse, want, lse_want, rows)
    described(c, body)


@pytest.mark.parametrize("seed", sc.PREFILL_SEEDS)
def test_fuzz_varlen_fwd(sfa, seed):
    packed_case(sfa, "varlen", seed)


@pytest.mark.parametrize("seed", sc.PREFILL_SEEDS)
def test_fuzz_varlen_window_fwd(sfa, seed):
    packed_case(sfa, "varlen_window", seed)


@pytest.mark.parametrize("seed", sc.PREFILL_SEEDS)
def test_fuzz_varlen_split_fwd(sfa, seed):
    packed_case(sfa, "varlen_split", seed)
