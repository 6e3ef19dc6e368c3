"""GPU tests of sfa_prefill_varlen_window_fwd / flash_attn_varlen_window_fwd / mha_varlen_fwd_window: the packed prefill
forward under a sliding window with attention sinks, against tests/prefill_varlen_window_ref.py (prefill_window_ref per
sequence: tests/test_prefill_varlen_window_cpu.py) on identically rounded inputs, and against the rectangular windowed
call's bits.

Tolerances are the project's: o within TOL (fp16 2e-3, bf16 1.6e-2: tests/test_prefill_gpu.py::TOL), lse within 2e-3
(LSE_TOL["exact"]; the packed windowed kernel is an exact-scale kernel), exact counts to 2 ulp of the type and 1e-5.  The
batches P, Q, R and S are the smallest that reach each edge (prefill_varlen_window_ref.BATCHES)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import prefill_cases as pc
import prefill_window_cases as wc
from oracle import round_to
from prefill_varlen_ref import cu_of
from prefill_varlen_window_ref import (BATCHES, INT_MAX, anchor_sinks, batch_cu, inputs, lo0, prefill_varlen_window_ref,
                                       reference)
from prefill_window_ref import visible_counts, window_mask

pytestmark = pytest.mark.gpu

TOL = {"fp16": 2e-3, "bf16": 1.6e-2}            # tests/test_prefill_gpu.py::TOL
LSE_TOL = 2e-3                                  # tests/test_prefill_gpu.py::LSE_TOL["exact"]
ULP2 = {"bf16": 2.0 ** -7, "fp16": 2.0 ** -10}  # 2 ulp of the 16-bit type
TDT = {"fp16": torch.float16, "bf16": torch.bfloat16}
DEV = "cuda:0"
FILL = 7.0                                      # what o and lse hold before a call that must leave rows alone
PARITY_WINDOWS = (1, 40, 65, 128, 300)
SINKS = (False, True)
CONFIGS = [(dt, D) for dt in ("fp16", "bf16") for D in (64, 128)]      # with SINKS: all 8 instances of the kernel


@pytest.fixture(scope="module")
def sfa():
    assert torch.cuda.is_available(), "GPU tests need a GPU (run with -m gpu on the MI355X box)"
    import starflashattention_amd as m
    m._lib.load()
    return m


def dev16(x, dtype):
    return torch.from_numpy(np.array(x, order="C")).to(TDT[dtype]).to(DEV)          # (a copy: the shared problems are read-only)


def cu_dev(cu):
    return torch.tensor(list(cu), dtype=torch.int32, device=DEV)


def sinks_dev(sinks):
    return None if sinks is None else torch.from_numpy(np.array(sinks, np.float32)).to(DEV)


def call(sfa, tq, tk, tv, cu_q, cu_k, window, sinks=None, **kw):
    """flash_attn_varlen_window_fwd with lse; sinks: None, a numpy [Hq] array or a device tensor.  Returns (o, lse)."""
    ts = sinks if isinstance(sinks, torch.Tensor) else sinks_dev(sinks)
    o, lse = sfa.flash_attn_varlen_window_fwd(tq, tk, tv, cu_dev(cu_q), cu_dev(cu_k), window, sinks=ts, return_lse=True, **kw)
    torch.cuda.synchronize()
    return o, lse


def raw_call(sfa, tq, tk, tv, cu_q, cu_k, window, sinks=None, fill=FILL, total_q=None, total_k=None, softmax_scale=None):
    """sfa_prefill_varlen_window_fwd on torch views as they are, with o and lse buffers of the test's own holding `fill`
    and, if given, totals smaller than the tensors.  Returns (o, lse [Hq, total_q])."""
    lib = sfa._lib.load()
    Tq = tq.shape[0] if total_q is None else total_q
    Tk = tk.shape[0] if total_k is None else total_k
    Hq, D = tq.shape[1], tq.shape[2]
    B = len(cu_q) - 1
    cq, ck = cu_dev(cu_q), cu_dev(cu_k)
    out = torch.full(tq.shape, fill, dtype=tq.dtype, device=DEV)
    lse = torch.full((Hq, Tq), fill, dtype=torch.float32, device=DEV)
    ws = torch.empty(sfa.prefill_varlen_workspace_bytes(B, Tq), dtype=torch.uint8, device=DEV)
    ts = sinks_dev(sinks)
    a = sfa._lib.PrefillVarlenArgs()
    a.q, a.k, a.v, a.o, a.lse = tq.data_ptr(), tk.data_ptr(), tv.data_ptr(), out.data_ptr(), lse.data_ptr()
    a.cu_seqlens_q, a.cu_seqlens_k = cq.data_ptr(), ck.data_ptr()
    a.batch, a.heads_q, a.heads_kv, a.total_q, a.total_k, a.head_dim = B, Hq, tk.shape[1], Tq, Tk, D
    for dst, t in ((a.q_stride, tq), (a.k_stride, tk), (a.v_stride, tv), (a.o_stride, out)):
        dst[0], dst[1] = t.stride(0), t.stride(1)
    a.softmax_scale = float(softmax_scale) if softmax_scale else 0.0
    a.causal = 1
    a.dtype = sfa._lib.DTYPE_FP16 if tq.dtype == torch.float16 else sfa._lib.DTYPE_BF16
    st = lib.sfa_prefill_varlen_window_fwd(ctypes.byref(a), int(window), ctypes.c_void_p(ts.data_ptr()) if ts is not None else None,
                                           ctypes.c_void_p(ws.data_ptr()), ws.numel(),
                                           ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))
    assert st == 0, (st, lib.sfa_last_error())
    torch.cuda.synchronize()
    return out, lse


def same_bits(o1, lse1, o0, lse0, what=""):
    assert torch.equal(o1.contiguous().view(torch.int16), o0.contiguous().view(torch.int16)), what
    assert torch.equal(lse1.contiguous().view(torch.int32), lse0.contiguous().view(torch.int32)), what


def check(o, lse, want, lse_want, rows, dtype, fill=None):
    """o [Tq, Hq, D], lse [Hq, Tq] numpy against the reference on the rows of valid sequences; the others hold `fill`"""
    np.testing.assert_allclose(o[rows], want[rows], atol=TOL[dtype], rtol=TOL[dtype])
    fin = np.isfinite(lse_want) & rows[None, :]
    none = ~np.isfinite(lse_want) & rows[None, :]
    np.testing.assert_allclose(lse[fin], lse_want[fin], atol=LSE_TOL, rtol=LSE_TOL)
    assert np.all(lse[none] == -np.inf)                         # a row that sees no key: exactly 0 and -inf
    assert np.all(o.transpose(1, 0, 2)[none] == 0)
    if fill is not None:
        assert np.all(o[~rows] == fill) and np.all(lse[:, ~rows] == fill)


def check_ref(o, lse, ref, dtype, fill=None):
    check(o.float().cpu().numpy(), lse.cpu().numpy(), ref[0], ref[1], ref[2], dtype, fill)


@functools.lru_cache(maxsize=None)
def device_inputs(name, dtype, D, pad=0):
    """the device copies of inputs(...): made once, never written to"""
    return tuple(dev16(x, dtype) for x in inputs(name, dtype, D, pad))


@functools.lru_cache(maxsize=None)
def packed(sfa, name, dtype, D, window, with_sinks):
    """(o, lse) of the packed call on a batch: run once per key, shared by the tests that compare against it"""
    tq, tk, tv = device_inputs(name, dtype, D)
    cu_q, cu_k = batch_cu(name)
    return call(sfa, tq, tk, tv, cu_q, cu_k, window, reference(name, dtype, D, window, with_sinks)[3])


def sequences(name):
    """(b, q0, q1, k0, k1) of a batch's sequences with rows"""
    cu_q, cu_k = batch_cu(name)
    return [(b, cu_q[b], cu_q[b + 1], cu_k[b], cu_k[b + 1]) for b in range(len(cu_q) - 1) if cu_q[b + 1] > cu_q[b]]


def ids3(name, dtype, D):
    return f"{name}-{dtype}-D{D}"


def cases(names):
    return [pytest.param(n, dt, D, id=ids3(n, dt, D)) for n in names for dt, D in CONFIGS]


# ---- 1. parity ----
@pytest.mark.parametrize("name,dtype,D", cases("PQRS"))
def test_parity(sfa, name, dtype, D):
    for window in PARITY_WINDOWS:
        for with_sinks in SINKS:
            ref = reference(name, dtype, D, window, with_sinks)
            assert ref[2].all()
            o, lse = packed(sfa, name, dtype, D, window, with_sinks)
            assert o.shape == ref[0].shape and lse.shape == ref[1].shape
            check_ref(o, lse, ref, dtype)
            if name == "Q":
                lse = lse.cpu().numpy()
                assert np.all(lse[:, 100:100 + 233] == -np.inf) and np.all(np.isfinite(lse[:, 100 + 233:100 + 333]))
                assert np.all(lse[:, 433:438] == -np.inf)           # the sequence with no keys
                assert np.all(o[100:100 + 233].float().cpu().numpy() == 0) and np.all(o[433:438].float().cpu().numpy() == 0)


@pytest.mark.parametrize("dtype,D", CONFIGS)
def test_rows_beyond_the_last_sequence_keep_their_fill(sfa, dtype, D):
    """batch Q with total_q and total_k 40 rows beyond cu[batch], o and lse prefilled: the padding rows keep their fill (the
    q, k, v rows there are NaN: nothing reads them either)"""
    cu_q, cu_k = batch_cu("Q")
    q, k, v = inputs("Q", dtype, D, 40)
    assert q.shape[0] == cu_q[-1] + 40 and k.shape[0] == cu_k[-1] + 40
    tq, tk, tv = dev16(q, dtype), dev16(k, dtype), dev16(v, dtype)
    tq[cu_q[-1]:] = float("nan")
    tk[cu_k[-1]:] = float("nan")
    tv[cu_k[-1]:] = float("nan")
    for with_sinks in SINKS:
        ref = reference("Q", dtype, D, 128, with_sinks, None, 40)
        assert not ref[2][cu_q[-1]:].any() and ref[2][:cu_q[-1]].all()
        o, lse = raw_call(sfa, tq, tk, tv, cu_q, cu_k, 128, ref[3])
        check_ref(o, lse, ref, dtype, fill=FILL)


# ---- 2. the bits of the rectangular kernel ----
@pytest.mark.parametrize("name,dtype,D", cases("PQRS"))
def test_bits_of_the_rectangular_kernel(sfa, name, dtype, D):
    """Every sequence against flash_attn_window_fwd on its own [1, H, n, D] view, wherever that call runs the windowed
    kernel (sinks given, or window < n_k): equal bit for bit in o and lse."""
    tq, tk, tv = device_inputs(name, dtype, D)
    compared = 0
    for window in PARITY_WINDOWS:
        for with_sinks in SINKS:
            ts = sinks_dev(reference(name, dtype, D, window, with_sinks)[3])
            o, lse = packed(sfa, name, dtype, D, window, with_sinks)
            for b, q0, q1, k0, k1 in sequences(name):
                if k1 == k0 or not (with_sinks or window < k1 - k0):
                    continue
                o4, lse4 = sfa.flash_attn_window_fwd(tq[q0:q1].transpose(0, 1)[None], tk[k0:k1].transpose(0, 1)[None],
                                                     tv[k0:k1].transpose(0, 1)[None], window, sinks=ts, return_lse=True)
                torch.cuda.synchronize()
                same_bits(o4[0].transpose(0, 1), lse4[0], o[q0:q1], lse[:, q0:q1], (window, with_sinks, b))
                compared += 1
    assert compared >= len(PARITY_WINDOWS) * len(sequences(name)) // 2


# ---- 3. alone equals batched ----
@pytest.mark.parametrize("name,dtype,D", cases("QR"))
def test_alone_equals_batched(sfa, name, dtype, D):
    tq, tk, tv = device_inputs(name, dtype, D)
    for window in (40, 128):
        for with_sinks in SINKS:
            sinks = reference(name, dtype, D, window, with_sinks)[3]
            o, lse = packed(sfa, name, dtype, D, window, with_sinks)
            for b, q0, q1, k0, k1 in sequences(name):
                # its own slices; a sequence with no keys still needs a K / V pointer: one row it does not own
                ks, vs = (tk[k0:k1], tv[k0:k1]) if k1 > k0 else (tk[:1], tv[:1])
                o1, lse1 = call(sfa, tq[q0:q1], ks, vs, [0, q1 - q0], [0, k1 - k0], window, sinks)
                same_bits(o1, lse1, o[q0:q1], lse[:, q0:q1], (window, with_sinks, b))


# ---- 4. poisoned neighbours and never-read rows ----
@pytest.mark.parametrize("name,dtype,D", cases("QR"))
def test_poisoned_neighbours_and_never_read_rows(sfa, name, dtype, D):
    """NaN in q, K and V of every other sequence, in the sequence's own K and V rows below lo_0(b) and in the padding rows:
    the sequence's rows are the clean call's bit for bit.  A masked key that is read still reaches P.V as 0 * NaN."""
    cu_q, cu_k = batch_cu(name)
    q, k, v = inputs(name, dtype, D, 40)
    tq, tk, tv = dev16(q, dtype), dev16(k, dtype), dev16(v, dtype)
    nan = float("nan")
    for window in (1, 65, 128):
        for with_sinks in SINKS:
            ref = reference(name, dtype, D, window, with_sinks, None, 40)
            o, lse = raw_call(sfa, tq, tk, tv, cu_q, cu_k, window, ref[3])
            check_ref(o, lse, ref, dtype, fill=FILL)
            for b, q0, q1, k0, k1 in sequences(name):
                low = lo0(q1 - q0, k1 - k0, window)
                pq, pk, pv = (torch.full_like(t, nan) for t in (tq, tk, tv))
                pq[q0:q1], pk[k0 + low:k1], pv[k0 + low:k1] = tq[q0:q1], tk[k0 + low:k1], tv[k0 + low:k1]
                o1, lse1 = raw_call(sfa, pq, pk, pv, cu_q, cu_k, window, ref[3])
                same_bits(o1[q0:q1], lse1[:, q0:q1], o[q0:q1], lse[:, q0:q1], (window, with_sinks, b, low))
                assert np.all(o1[cu_q[-1]:].float().cpu().numpy() == FILL) and np.all(lse1[:, cu_q[-1]:].cpu().numpy() == FILL)
    if name == "Q":
        assert lo0(100, 1000, 128) == 773
    else:
        assert lo0(64, 769, 1) == 705 and lo0(64, 769, 65) == 641


# ---- 5. the exact window count ----
COUNT_WINDOWS = (1, 2, 63, 64, 65, 127, 128, 129, 300)


@pytest.mark.parametrize("name,dtype,D", cases("RS"))
def test_exact_window_count(sfa, name, dtype, D):
    """q = 0, so every score is 0 and every weight 1; V row j -- j the index within the sequence -- is the unit vector of
    j % D; the sink logit is 0, one more weight of 1.  Then o[i, d] = c_i(d) / (cnt_i + 1) and lse = log(cnt_i + 1) (cnt_i
    without sinks): a key beyond either edge of the window, or taken from the neighbour, moves an element by a whole
    1 / cnt.  rtol 2 ulp of the type, atol 1e-6; lse to 1e-5."""
    lens, Hq, Hkv = BATCHES[name]
    cu_q, cu_k = batch_cu(name)
    rng = np.random.default_rng(11)
    k = round_to(rng.standard_normal((cu_k[-1], Hkv, D)), dtype)
    v = np.zeros((cu_k[-1], Hkv, D))
    for b, (nq, nk) in enumerate(lens):
        v[cu_k[b] + np.arange(nk), :, np.arange(nk) % D] = 1.0
    tq = torch.zeros((cu_q[-1], Hq, D), dtype=TDT[dtype], device=DEV)
    tk, tv = dev16(k, dtype), dev16(v, dtype)
    for window in COUNT_WINDOWS:
        for with_sinks in SINKS:
            o, lse = call(sfa, tq, tk, tv, cu_q, cu_k, window, np.zeros(Hq, np.float32) if with_sinks else None)
            o, lse = o.float().cpu().numpy(), lse.cpu().numpy()
            for b, (nq, nk) in enumerate(lens):
                onehot = np.zeros((nk, D))
                onehot[np.arange(nk), np.arange(nk) % D] = 1.0
                mask = window_mask(nq, nk, window)
                cnt = mask.sum(axis=1).astype(np.float64)
                assert np.array_equal(cnt, visible_counts(nq, nk, window)) and cnt.min() >= 1 and cnt.max() <= window
                den = cnt + (1.0 if with_sinks else 0.0)
                want = (mask.astype(np.float64) @ onehot) / den[:, None]           # [nq, D]
                got, got_lse = o[cu_q[b]:cu_q[b + 1]], lse[:, cu_q[b]:cu_q[b + 1]]
                print(f"{name} seq {b} window={window} sinks={with_sinks} D={D} {dtype}: max |o - want| = "
                      f"{np.abs(got - want[:, None]).max():.3e}, max |lse - want| = {np.abs(got_lse - np.log(den)[None]).max():.3e}")
                for h in range(Hq):
                    what = f"window {window} sinks {with_sinks} seq {b} head {h}"
                    np.testing.assert_allclose(got[:, h], want, rtol=ULP2[dtype], atol=1e-6, err_msg=what)
                    np.testing.assert_allclose(got_lse[h], np.log(den), rtol=0, atol=1e-5, err_msg=what)


# ---- 6. sinks without weight ----
@pytest.mark.parametrize("dtype,D", CONFIGS)
def test_sinks_without_weight_are_no_sinks(sfa, dtype, D):
    """sinks of -inf, of -1e30 and None give the same bits under a window below some n_k (40: every sequence of Q with
    keys): the SINK instance with a weight that underflows, and the instance without the flag."""
    tq, tk, tv = device_inputs("Q", dtype, D)
    cu_q, cu_k = batch_cu("Q")
    Hq = BATCHES["Q"][1]
    o0, lse0 = packed(sfa, "Q", dtype, D, 40, False)
    for value in (-np.inf, -1e30):
        o1, lse1 = call(sfa, tq, tk, tv, cu_q, cu_k, 40, np.full(Hq, value, np.float32))
        same_bits(o1, lse1, o0, lse0, value)
    check_ref(o0, lse0, reference("Q", dtype, D, 40, False), dtype)


# ---- 7. forwarding ----
@pytest.mark.parametrize("name,dtype,D", cases("PQ"))
def test_forwarding(sfa, name, dtype, D):
    """window = total_k, total_k + 1 and INT_MAX without sinks: flash_attn_varlen_fwd(causal=True), bit for bit.  The same
    windows with sinks run the windowed kernel and match the reference."""
    tq, tk, tv = device_inputs(name, dtype, D)
    cu_q, cu_k = batch_cu(name)
    total_k = tk.shape[0]
    assert total_k == cu_k[-1]
    o0, lse0 = sfa.flash_attn_varlen_fwd(tq, tk, tv, cu_dev(cu_q), cu_dev(cu_k), causal=True, return_lse=True)
    torch.cuda.synchronize()
    ref = reference(name, dtype, D, INT_MAX, True)          # (every window >= max n_k has the same reference and sinks)
    for window in (total_k, total_k + 1, INT_MAX):
        o1, lse1 = call(sfa, tq, tk, tv, cu_q, cu_k, window)
        same_bits(o1, lse1, o0, lse0, window)
        o2, lse2 = call(sfa, tq, tk, tv, cu_q, cu_k, window, ref[3])
        check_ref(o2, lse2, ref, dtype)
        assert not torch.equal(lse2, lse0)                  # the sinks took part
    check_ref(o0, lse0, reference(name, dtype, D, INT_MAX, False), dtype)


# ---- 8. adversarial numerics, packed ----
STRESS_KINDS = ("spike", "alone", "staircase64_down")
STRESS_WINDOWS = (40, 65)
STRESS_CONFIGS = wc.CONFIGS_W                   # with SINKS: all 8 instances of the kernel


@pytest.mark.parametrize("cfg", STRESS_CONFIGS, ids=wc.config_id)
@pytest.mark.parametrize("kind", STRESS_KINDS)
def test_adversarial_numerics_packed(sfa, kind, cfg):
    """prefill_window_cases.stress_w problems of the three prefill_cases.SHAPES, batch b of each as one sequence of a packed
    batch of three (a problem with fewer batches repeats them): held to oracle_w, the rows of exact_rows_w to V's bits, as
    tests/test_prefill_window_numerics_gpu.py does, and to the rectangular call's bits.  The sinks are sinks_for of the
    first shape, for all three sequences."""
    D, dtype, G = cfg
    probs = [wc.stress_w(kind, dtype, D, G, Sq, Sk) for Sq, Sk in wc.SHAPES]
    Hq = probs[0].Hq
    assert all(p.Hq == Hq and p.Hkv == probs[0].Hkv for p in probs)
    cu_q, cu_k = cu_of([p.Sq for p in probs]), cu_of([p.Sk for p in probs])
    dev = [pc.device_inputs(p) for p in probs]                                  # [B, H, S, D] each
    exact_seen = 0
    for window in STRESS_WINDOWS:
        for with_sinks in SINKS:
            sinks = wc.sinks_for(probs[0], window) if with_sinks else None
            rect = [wc.run_window(sfa, p, window, sinks) for p in probs]        # the rectangular call: bits of o, lse
            for rnd in range(max(p.B for p in probs)):
                bs = [rnd % p.B for p in probs]
                tq = torch.cat([d[0][b].transpose(0, 1) for d, b in zip(dev, bs)]).contiguous()
                tk = torch.cat([d[1][b].transpose(0, 1) for d, b in zip(dev, bs)]).contiguous()
                tv = torch.cat([d[2][b].transpose(0, 1) for d, b in zip(dev, bs)]).contiguous()
                o, lse = call(sfa, tq, tk, tv, cu_q, cu_k, window, sinks)
                for s, (p, b) in enumerate(zip(probs, bs)):
                    want, lse_want = wc.oracle_w(p, window, sinks)
                    got = o[cu_q[s]:cu_q[s + 1]].transpose(0, 1).contiguous()   # [Hq, Sq, D]
                    got_lse = lse[:, cu_q[s]:cu_q[s + 1]].contiguous().cpu().numpy()
                    g = got.float().cpu().numpy()
                    np.testing.assert_allclose(g, want[b], atol=TOL[dtype], rtol=TOL[dtype])
                    fin = np.isfinite(lse_want[b])
                    np.testing.assert_allclose(got_lse[fin], lse_want[b][fin], atol=LSE_TOL, rtol=LSE_TOL)
                    assert np.all(got_lse[~fin] == -np.inf) and np.all(g[~fin] == 0)
                    gb = got.view(torch.int16).cpu().numpy().view(np.uint16)
                    ex = wc.exact_rows_w(p, window, sinks)[b]                   # [Hq, Sq]
                    if ex.any():
                        vrow = np.repeat(wc.v_bits(p)[b][np.arange(p.Hkv), p.spike[b]], G, axis=0)      # [Hq, D]
                        np.testing.assert_array_equal(gb[ex], np.broadcast_to(vrow[:, None, :], gb.shape)[ex])
                        exact_seen += int(ex.sum())
                    np.testing.assert_array_equal(gb, rect[s]["o"][b], err_msg=f"{kind} window {window} shape {s}")
                    np.testing.assert_array_equal(got_lse.view(np.uint32), rect[s]["lse"][b].view(np.uint32))
    assert exact_seen > 0 or kind == "staircase64_down"


# ---- 9. scale and views ----
@pytest.mark.parametrize("scale", pc.SCALES)
@pytest.mark.parametrize("dtype,D", CONFIGS)
def test_softmax_scale(sfa, scale, dtype, D):
    """softmax_scale 0.03 and 0.5; the sinks are not scaled"""
    tq, tk, tv = device_inputs("Q", dtype, D)
    cu_q, cu_k = batch_cu("Q")
    for with_sinks in SINKS:
        ref = reference("Q", dtype, D, 128, with_sinks, scale)
        o, lse = call(sfa, tq, tk, tv, cu_q, cu_k, 128, ref[3], softmax_scale=scale)
        check_ref(o, lse, ref, dtype)


@pytest.mark.parametrize("dtype,D", CONFIGS)
def test_strided_views(sfa, dtype, D):
    """q, k and v as the three slices of one packed [T, Hq + 2 Hkv, D] tensor (n_q = n_k), then o as a view inside a
    NaN-filled allocation: each equals the contiguous call's bits, and the allocation outside the view stays NaN."""
    lens, Hq, Hkv, window = [300, 0, 1, 257, 64], 4, 2, 65
    cu = cu_of(lens)
    T = cu[-1]
    rng = np.random.default_rng(D + 3)
    qkv = dev16(round_to(rng.standard_normal((T, Hq + 2 * Hkv, D)), dtype), dtype)
    tq, tk, tv = qkv[:, :Hq], qkv[:, Hq:Hq + Hkv], qkv[:, Hq + Hkv:]
    assert tq.stride(0) == (Hq + 2 * Hkv) * D == tk.stride(0) and not tk.is_contiguous()
    q, k, v = (t.float().cpu().numpy() for t in (tq, tk, tv))
    want, lse_want, rows = prefill_varlen_window_ref(q, k, v, cu, cu, window)
    sinks = anchor_sinks(lse_want, rows)
    ref = prefill_varlen_window_ref(q, k, v, cu, cu, window, sinks=sinks.astype(np.float64))
    o0, lse0 = call(sfa, tq.contiguous(), tk.contiguous(), tv.contiguous(), cu, cu, window, sinks)
    check_ref(o0, lse0, ref, dtype)
    o1, lse1 = call(sfa, tq, tk, tv, cu, cu, window, sinks)
    same_bits(o1, lse1, o0, lse0)
    base = torch.full((T + 16, Hq + 1, D + 8), float("nan"), dtype=TDT[dtype], device=DEV)
    view = base[8:8 + T, :Hq, :D]
    o2, lse2 = call(sfa, tq, tk, tv, cu, cu, window, sinks, out=view)
    assert o2.data_ptr() == view.data_ptr()
    same_bits(o2, lse2, o0, lse0)
    inside = torch.zeros(base.shape, dtype=torch.bool, device=DEV)
    inside[8:8 + T, :Hq, :D] = True
    assert torch.isnan(base[~inside]).all() and not torch.isnan(base[inside]).any()


# ---- 10. bad cu_seqlens ----
@pytest.mark.parametrize("dtype,D", CONFIGS)
def test_a_sequence_that_runs_backwards_is_skipped(sfa, dtype, D):
    cu_q, cu_k = [0, 10, 20, 30], [0, 100, 50, 300]
    rng = np.random.default_rng(D + 1)
    q = round_to(rng.standard_normal((30, 4, D)), dtype)
    k = round_to(rng.standard_normal((300, 2, D)), dtype)
    v = round_to(rng.standard_normal((300, 2, D)), dtype)
    sinks = np.linspace(-1.0, 2.0, 4).astype(np.float32)
    for s in (None, sinks):
        ref = prefill_varlen_window_ref(q, k, v, cu_q, cu_k, 40, sinks=None if s is None else s.astype(np.float64))
        assert ref[2][:10].all() and not ref[2][10:20].any() and ref[2][20:].all()
        o, lse = raw_call(sfa, dev16(q, dtype), dev16(k, dtype), dev16(v, dtype), cu_q, cu_k, 40, s)
        check_ref(o, lse, ref, dtype, fill=FILL)


@pytest.mark.parametrize("dtype,D", CONFIGS)
def test_a_sequence_past_total_k_is_skipped(sfa, dtype, D):
    """cu_k[batch] = 300 is above the total_k = 260 passed but inside the allocation of 300 rows, so that not even a wrong
    implementation leaves valid memory: the last sequence is skipped, the others are correct."""
    cu_q, cu_k = [0, 10, 20, 30], [0, 100, 200, 300]
    rng = np.random.default_rng(D + 2)
    q = round_to(rng.standard_normal((30, 4, D)), dtype)
    k = round_to(rng.standard_normal((300, 2, D)), dtype)
    v = round_to(rng.standard_normal((300, 2, D)), dtype)
    sinks = np.linspace(-1.0, 2.0, 4).astype(np.float32)
    for s in (None, sinks):
        ref = prefill_varlen_window_ref(q, k[:260], v[:260], cu_q, cu_k, 40, sinks=None if s is None else s.astype(np.float64))
        assert ref[2][:20].all() and not ref[2][20:].any()
        o, lse = raw_call(sfa, dev16(q, dtype), dev16(k, dtype), dev16(v, dtype), cu_q, cu_k, 40, s, total_k=260)
        check_ref(o, lse, ref, dtype, fill=FILL)


# ---- 11. the workspace ----
@pytest.mark.parametrize("dtype,D", CONFIGS)
def test_workspace(sfa, dtype, D):
    tq, tk, tv = device_inputs("P", dtype, D)
    cu_q, cu_k = batch_cu("P")
    need = sfa.prefill_varlen_workspace_bytes(len(cu_q) - 1, tq.shape[0])
    assert need == 256
    ref = reference("P", dtype, D, 65, True)
    outs = []
    for fill in (0x00, 0xFF):
        ws = torch.full((need,), fill, dtype=torch.uint8, device=DEV)
        outs.append(call(sfa, tq, tk, tv, cu_q, cu_k, 65, ref[3], workspace=ws))
    same_bits(*outs[0], *outs[1])
    check_ref(*outs[1], ref, dtype)
    same_bits(*outs[1], *packed(sfa, "P", dtype, D, 65, True))
    cq, ck, ts = cu_dev(cu_q), cu_dev(cu_k), sinks_dev(ref[3])
    f = sfa.flash_attn_varlen_window_fwd
    with pytest.raises(sfa.SfaError, match="sfa_prefill_varlen_window_fwd: workspace has") as e:       # one byte short
        f(tq, tk, tv, cq, ck, 65, sinks=ts, workspace=ws[:need - 1])
    assert e.value.status == -5
    big = torch.zeros(need + 256, dtype=torch.uint8, device=DEV)
    with pytest.raises(sfa.SfaError, match="sfa_prefill_varlen_window_fwd: workspace must be 256-byte aligned") as e:
        f(tq, tk, tv, cq, ck, 65, sinks=ts, workspace=big[16:])
    assert e.value.status == -2
    with pytest.raises(sfa.SfaError, match="sfa_prefill_varlen_window_fwd: workspace is NULL") as e:
        f(tq, tk, tv, cq, ck, 65, workspace=big[:0])
    assert e.value.status == -1
    torch.cuda.synchronize()


# ---- 12. the debug knobs ----
def test_debug_knobs_keep_their_values(sfa):
    x = torch.randn(1, 2, 300, 128, device=DEV).bfloat16()
    sfa.flash_attn_split_fwd(x, x, x, causal=True, num_splits=2)
    sfa.flash_attn_fwd(x, x, x, causal=True)
    torch.cuda.synchronize()
    ran, splits = sfa.debug_get("last_prefill_kernel"), sfa.debug_get("last_prefill_splits")
    assert ran > 0 and splits == 2
    tq, tk, tv = device_inputs("P", "bf16", 128)
    cu_q, cu_k = batch_cu("P")
    for window, with_sinks in ((65, True), (65, False), (INT_MAX, False)):      # the kernel with and without SINK; forwarded
        ref = reference("P", "bf16", 128, window, with_sinks)
        o, lse = call(sfa, tq, tk, tv, cu_q, cu_k, window, ref[3])
        check_ref(o, lse, ref, "bf16")
        assert sfa.debug_get("last_prefill_kernel") == ran and sfa.debug_get("last_prefill_splits") == splits


# ---- 13. graph ----
def test_graph_replay_with_new_contents(sfa):
    """One captured call on a side stream -- two launches, no parallel branches -- replayed three times with new q, k, v,
    new contents of both cu arrays (the same batch and totals, other lengths, one of them 0, one sequence without keys) and
    new contents of sinks."""
    dtype, D, Hq, Hkv, B, Tq, Tk, window = "bf16", 64, 4, 2, 4, 700, 900, 128
    tq = torch.zeros(Tq, Hq, D, dtype=TDT[dtype], device=DEV)
    tk = torch.zeros(Tk, Hkv, D, dtype=TDT[dtype], device=DEV)
    tv = torch.zeros_like(tk)
    out = torch.zeros_like(tq)
    ts = torch.zeros(Hq, dtype=torch.float32, device=DEV)
    cq, ck = cu_dev([0] * (B + 1)), cu_dev([0] * (B + 1))
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        sfa.flash_attn_varlen_window_fwd(tq, tk, tv, cq, ck, window, sinks=ts, out=out)     # warm-up: the stream's workspace exists
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            _, lse = sfa.flash_attn_varlen_window_fwd(tq, tk, tv, cq, ck, window, sinks=ts, out=out, return_lse=True)
        replays = [([(300, 300), (1, 1), (257, 257), (64, 64)], 1),
                   ([(100, 400), (0, 0), (333, 100), (256, 256)], 2),
                   ([(5, 0), (600, 890), (0, 0), (1, 2)], 3)]
        for lens, seed in replays:
            cu_q, cu_k = cu_of([a for a, _ in lens]), cu_of([b for _, b in lens])
            assert cu_q[-1] <= Tq and cu_k[-1] <= Tk
            rng = np.random.default_rng(seed)
            q = round_to(rng.standard_normal((Tq, Hq, D)), dtype)
            k = round_to(rng.standard_normal((Tk, Hkv, D)), dtype)
            v = round_to(rng.standard_normal((Tk, Hkv, D)), dtype)
            _, lse_ns, rows = prefill_varlen_window_ref(q, k, v, cu_q, cu_k, window)
            sinks = anchor_sinks(lse_ns, rows)
            ref = prefill_varlen_window_ref(q, k, v, cu_q, cu_k, window, sinks=sinks.astype(np.float64))
            assert not ref[2][cu_q[-1]:].any()
            for dst, src in ((tq, q), (tk, k), (tv, v)):
                dst.copy_(dev16(src, dtype))
            cq.copy_(cu_dev(cu_q))
            ck.copy_(cu_dev(cu_k))
            ts.copy_(sinks_dev(sinks))
            out.fill_(FILL)
            lse.fill_(FILL)
            graph.replay()
            side.synchronize()
            check_ref(out, lse, ref, dtype, fill=FILL)


# ---- 14. the pybind surface ----
def test_pybind_mha_varlen_fwd_window(sfa):
    import star_flash_attn as ext
    dtype, D = "bf16", 128
    tq, tk, tv = device_inputs("P", dtype, D)
    cu_q, cu_k = batch_cu("P")
    cq, ck = cu_dev(cu_q), cu_dev(cu_k)
    for with_sinks in SINKS:
        ref = reference("P", dtype, D, 65, with_sinks)
        ts = sinks_dev(ref[3])
        out, lse = ext.mha_varlen_fwd_window(tq, tk, tv, cq, ck, 65, sinks=ts, return_lse=True)
        torch.cuda.synchronize()
        check_ref(out, lse, ref, dtype)
        same_bits(out, lse, *packed(sfa, "P", dtype, D, 65, with_sinks))
        (o3,) = ext.mha_varlen_fwd_window(tq, tk, tv, cq, ck, 65, ts)
        torch.cuda.synchronize()
        assert torch.equal(o3.view(torch.int16), out.view(torch.int16))
    with pytest.raises(RuntimeError, match="head_dim 256"):
        z = torch.zeros(16, 2, 256, device=DEV, dtype=torch.bfloat16)
        ext.mha_varlen_fwd_window(z, z, z, cu_dev([0, 16]), cu_dev([0, 16]), 8)
    with pytest.raises(RuntimeError, match="window must be in"):
        ext.mha_varlen_fwd_window(tq, tk, tv, cq, ck, 0)
