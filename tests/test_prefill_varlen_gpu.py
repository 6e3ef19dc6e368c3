"""GPU tests of sfa_prefill_varlen_fwd / flash_attn_varlen_fwd / mha_varlen_fwd: the prefill forward over packed
sequences of different lengths, against tests/prefill_varlen_ref.py (oracle.sdpa_ref per sequence:
tests/test_prefill_varlen_cpu.py) on identically rounded inputs.

Tolerances: o within the project's TOL (fp16 2e-3, bf16 1.6e-2: tests/test_prefill_gpu.py::TOL), lse within 2e-3
(LSE_TOL["exact"] of tests/test_prefill_gpu.py; the packed kernel is an exact-scale kernel).  The batches are the smallest
that reach each edge (the table at BATCHES)."""
import functools

import numpy as np
import pytest
import torch

import prefill_cases as pc
from oracle import round_to
from prefill_varlen_ref import cu_of, items, plan_bound, prefill_varlen_ref

pytestmark = pytest.mark.gpu

TOL = {"fp16": 2e-3, "bf16": 1.6e-2}            # tests/test_prefill_gpu.py::TOL
LSE_TOL = 2e-3                                  # tests/test_prefill_gpu.py::LSE_TOL["exact"]
TDT = {"fp16": torch.float16, "bf16": torch.bfloat16}
NAN16 = {"fp16": 0x7E00, "bf16": 0x7FC0}
DEV = "cuda:0"
FILL = 7.0                                      # what o and lse hold before a call that must leave rows alone

# name -> (the (n_q, n_k) of each sequence, Hq, Hkv, causal values, head dims)
BATCHES = {
    "A": ([(1, 1)], 2, 2, (True, False), (64, 128)),                            # one row, one key
    "B": ([(300, 300), (0, 0), (1, 1), (257, 257), (64, 64)], 4, 2, (True,), (64, 128)),    # an empty sequence inside; a one-row
    #                                                     second q-tile; 6 items in 7 slots (one marker)
    "C": ([(100, 1000), (333, 100), (5, 0), (256, 256)], 2, 2, (True,), (64, 128)),     # n_q < n_k; 233 rows without a key; a
    #                                                     sequence with no keys; exactly one full q-tile
    "D": ([(64, 257), (257, 65), (1, 129)], 8, 1, (False,), (64,)),             # a last key tile of one key next to another
    #                                                     sequence's rows; n_q > n_k without a mask
    "E": ([(300, 321), (100, 383), (64, 65), (1, 128)], 2, 1, (True, False), (64, 128)),    # key lengths = 1, 63, 1, 0 mod 64
    #                                                     side by side; 5 items in 5 slots
}


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


def bits(t):
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


@functools.lru_cache(maxsize=None)
def problem(name, dtype, D, causal, scale=None, pad=0):
    """(q [Tq, Hq, D], k, v [Tk, Hkv, D] rounded to dtype, cu_q, cu_k, the fp64 reference o [Tq, Hq, D], lse [Hq, Tq] and the
    mask of the rows of valid sequences): computed once per key, shared, never written to.  pad: rows of the tensors
    beyond cu[batch]."""
    lens, Hq, Hkv, _, _ = BATCHES[name]
    cu_q, cu_k = cu_of([a for a, _ in lens]), cu_of([b for _, b in lens])
    rng = np.random.default_rng([ord(name), D, pad])
    q = round_to(rng.standard_normal((cu_q[-1] + pad, Hq, D)), dtype)
    k = round_to(rng.standard_normal((cu_k[-1] + pad, Hkv, D)), dtype)
    v = round_to(rng.standard_normal((cu_k[-1] + pad, Hkv, D)), dtype)
    o, lse, rows = prefill_varlen_ref(q, k, v, cu_q, cu_k, causal, scale)
    for a in (q, k, v, o, lse, rows):
        a.setflags(write=False)
    return q, k, v, tuple(cu_q), tuple(cu_k), o, lse, rows


def varlen_call(sfa, tq, tk, tv, cu_q, cu_k, causal, prefill=None, **kw):
    """flash_attn_varlen_fwd through the C ABI's lse layout; prefill = FILL: o and lse hold it before the call.  Returns
    (o, lse) device tensors."""
    out = kw.pop("out", None)
    if prefill is not None and out is None:
        out = torch.full(tq.shape, prefill, dtype=tq.dtype, device=DEV)
    if prefill is None:
        o, lse = sfa.flash_attn_varlen_fwd(tq, tk, tv, cu_dev(cu_q), cu_dev(cu_k), causal=causal, out=out, return_lse=True, **kw)
    else:
        o, lse = call_with_lse(sfa, tq, tk, tv, out, cu_dev(cu_q), cu_dev(cu_k), causal, prefill, **kw)
    torch.cuda.synchronize()
    return o, lse


def call_with_lse(sfa, tq, tk, tv, out, cu_q, cu_k, causal, fill, softmax_scale=None, total_q=None, total_k=None):
    """sfa_prefill_varlen_fwd on torch views as they are, with an lse buffer of the test's own (prefilled) and, if given,
    totals smaller than the tensors.  Returns (out, lse [Hq, total_q])."""
    import ctypes
    lib = sfa._lib.load()
    Tq = tq.shape[0] if total_q is None else total_q
    Tk = tk.shape[0] if total_k is None else total_k
    Hq, D = tq.shape[1], tq.shape[2]
    B = cu_q.numel() - 1
    lse = torch.full((Hq, Tq), fill, dtype=torch.float32, device=DEV)
    ws = torch.empty(sfa.prefill_varlen_workspace_bytes(B, Tq), dtype=torch.uint8, device=DEV)
    a = sfa._lib.PrefillVarlenArgs()
    a.q, a.k, a.v, a.o, a.lse = tq.data_ptr(), tk.data_ptr(), tv.data_ptr(), out.data_ptr(), lse.data_ptr()
    a.cu_seqlens_q, a.cu_seqlens_k = cu_q.data_ptr(), cu_k.data_ptr()
    a.batch, a.heads_q, a.heads_kv, a.total_q, a.total_k, a.head_dim = B, Hq, tk.shape[1], Tq, Tk, D
    for dst, t in ((a.q_stride, tq), (a.k_stride, tk), (a.v_stride, tv), (a.o_stride, out)):
        dst[0], dst[1] = t.stride(0), t.stride(1)
    a.softmax_scale = float(softmax_scale) if softmax_scale else 0.0
    a.causal = 1 if causal else 0
    a.dtype = sfa._lib.DTYPE_FP16 if tq.dtype == torch.float16 else sfa._lib.DTYPE_BF16
    st = lib.sfa_prefill_varlen_fwd(ctypes.byref(a), ctypes.c_void_p(ws.data_ptr()), ws.numel(),
                                    ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))
    assert st == 0, (st, lib.sfa_last_error())
    torch.cuda.synchronize()
    return out, lse


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


def cases(names, dtypes=("fp16", "bf16")):
    return [pytest.param(n, dt, D, c, id=f"{n}-{dt}-D{D}-{'causal' if c else 'full'}")
            for n in names for dt in dtypes for D in BATCHES[n][4] for c in BATCHES[n][3]]


def test_the_batches_reach_their_edges():
    q = lambda n: [a for a, _ in BATCHES[n][0]]
    assert items(cu_of(q("B"))) == 6 and plan_bound(5, sum(q("B"))) == 7
    assert items(cu_of(q("E"))) == 5 == plan_bound(4, sum(q("E")))
    assert [b % 64 for _, b in BATCHES["E"][0]] == [1, 63, 1, 0]
    assert all(b - a + 1 >= 2 for a, b in BATCHES["E"][0])      # every causal row of E sees at least 2 keys


# ---- 1. parity ----
@pytest.mark.parametrize("name,dtype,D,causal", cases("ABCD"))
def test_parity(sfa, name, dtype, D, causal):
    q, k, v, cu_q, cu_k, want, lse_want, rows = problem(name, dtype, D, causal)
    o, lse = varlen_call(sfa, dev16(q, dtype), dev16(k, dtype), dev16(v, dtype), cu_q, cu_k, causal)
    assert lse.shape == (q.shape[1], q.shape[0]) and o.shape == q.shape
    assert rows.all()
    check(o.float().cpu().numpy(), lse.cpu().numpy(), want, lse_want, rows, dtype)
    if name == "C":
        lse = lse.cpu().numpy()
        assert np.all(lse[:, 100:100 + 233] == -np.inf) and np.all(np.isfinite(lse[:, 100 + 233:100 + 333]))
        assert np.all(lse[:, 433:438] == -np.inf)               # the sequence with no keys


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("D", [64, 128])
def test_rows_beyond_the_last_sequence_keep_their_fill(sfa, dtype, D):
    """batch C with total_q and total_k 40 rows beyond cu[batch], o and lse prefilled: the padding rows keep their fill bit
    for bit (the q, k, v rows there are NaN: nothing reads them either)"""
    q, k, v, cu_q, cu_k, want, lse_want, rows = problem("C", dtype, D, True, None, 40)
    assert q.shape[0] == cu_q[-1] + 40 and k.shape[0] == cu_k[-1] + 40 and not rows[cu_q[-1]:].any()
    tq, tk, tv = dev16(q, dtype), dev16(k, dtype), dev16(v, dtype)
    tq[cu_q[-1]:] = float("nan")
    tk[cu_k[-1]:] = float("nan")
    tv[cu_k[-1]:] = float("nan")
    o, lse = varlen_call(sfa, tq, tk, tv, cu_q, cu_k, True, prefill=FILL)
    check(o.float().cpu().numpy(), lse.cpu().numpy(), want, lse_want, rows, dtype, fill=FILL)


# ---- 2. alone equals batched ----
@pytest.mark.parametrize("name,dtype,D,causal", cases("BC"))
def test_alone_equals_batched(sfa, name, dtype, D, causal):
    q, k, v, cu_q, cu_k, want, lse_want, rows = problem(name, dtype, D, causal)
    tq, tk, tv = dev16(q, dtype), dev16(k, dtype), dev16(v, dtype)
    o, lse = varlen_call(sfa, tq, tk, tv, cu_q, cu_k, causal)
    for b in range(len(cu_q) - 1):
        q0, q1, k0, k1 = cu_q[b], cu_q[b + 1], cu_k[b], cu_k[b + 1]
        if q1 == q0:
            continue
        # its own slices; a sequence with no keys still needs a K / V pointer: one row it does not own
        ks, vs = (tk[k0:k1], tv[k0:k1]) if k1 > k0 else (tk[:1], tv[:1])
        o1, lse1 = varlen_call(sfa, tq[q0:q1], ks, vs, [0, q1 - q0], [0, k1 - k0], causal)
        assert torch.equal(o1.view(torch.int16), o[q0:q1].view(torch.int16)), b
        assert torch.equal(lse1, lse[:, q0:q1]), b


# ---- 3. poisoned neighbours ----
@pytest.mark.parametrize("name,dtype,D,causal", cases("BD"))
def test_poisoned_neighbours(sfa, name, dtype, D, causal):
    """q, K and V of every other sequence are NaN: sequence b's rows are the clean call's bit for bit.  A key read from the
    neighbour at a ragged last tile, even under a mask, would turn the row into NaN (0 * NaN)."""
    q, k, v, cu_q, cu_k, want, lse_want, rows = problem(name, dtype, D, causal)
    tq, tk, tv = dev16(q, dtype), dev16(k, dtype), dev16(v, dtype)
    o, lse = varlen_call(sfa, tq, tk, tv, cu_q, cu_k, causal)
    check(o.float().cpu().numpy(), lse.cpu().numpy(), want, lse_want, rows, dtype)
    for b in range(len(cu_q) - 1):
        q0, q1, k0, k1 = cu_q[b], cu_q[b + 1], cu_k[b], cu_k[b + 1]
        if q1 == q0:
            continue
        pq, pk, pv = (torch.full_like(t, float("nan")) for t in (tq, tk, tv))
        pq[q0:q1], pk[k0:k1], pv[k0:k1] = tq[q0:q1], tk[k0:k1], tv[k0:k1]
        o1, lse1 = varlen_call(sfa, pq, pk, pv, cu_q, cu_k, causal)
        assert torch.equal(o1[q0:q1].view(torch.int16), o[q0:q1].view(torch.int16)), b
        assert torch.equal(lse1[:, q0:q1], lse[:, q0:q1]), b


# ---- 4. exact count at the seams ----
ULP2 = {"bf16": 2.0 ** -7, "fp16": 2.0 ** -10}  # 2 ulp of the 16-bit type


@pytest.mark.parametrize("name,dtype,D,causal", cases("E"))
def test_exact_count_at_the_seams(sfa, name, dtype, D, causal):
    """The construction of tests/test_prefill_split_gpu.py::test_exact_count_at_the_seams per sequence: q = 0, so every
    score is 0 and every weight 1; V row j -- j the index within the sequence -- is the unit vector of j % D.  Then
    o[i, d] = c_i(d) / cnt_i and lse = log cnt_i: a key taken from the neighbour or dropped at a ragged tile moves an
    element by a whole 1 / cnt.  rtol 2 ulp of the type, atol 1e-6; lse to 1e-5."""
    lens, Hq, Hkv, _, _ = BATCHES[name]
    cu_q, cu_k = cu_of([a for a, _ in lens]), cu_of([b for _, b in lens])
    rng = np.random.default_rng(11)
    q = np.zeros((cu_q[-1], Hq, D))
    k = round_to(rng.standard_normal((cu_k[-1], Hkv, D)), dtype)
    v = np.zeros((cu_k[-1], Hkv, D))
    for b, (nq, nk) in enumerate(lens):
        v[cu_k[b] + np.arange(nk), :, np.arange(nk) % D] = 1.0
    o, lse = varlen_call(sfa, dev16(q, dtype), dev16(k, dtype), dev16(v, dtype), cu_q, cu_k, causal)
    o, lse = o.float().cpu().numpy(), lse.cpu().numpy()
    for b, (nq, nk) in enumerate(lens):
        onehot = np.zeros((nk, D))
        onehot[np.arange(nk), np.arange(nk) % D] = 1.0
        mask = np.ones((nq, nk), bool)
        if causal:
            mask = np.arange(nk)[None, :] <= np.arange(nq)[:, None] + (nk - nq)
        cnt = mask.sum(axis=1).astype(np.float64)
        assert cnt.min() >= (2 if causal else 1)
        want = (mask.astype(np.float64) @ onehot) / cnt[:, None]           # [nq, D]
        got, got_lse = o[cu_q[b]:cu_q[b + 1]], lse[:, cu_q[b]:cu_q[b + 1]]
        print(f"{name} seq {b} causal={causal} D={D} {dtype}: max |o - want| = {np.abs(got - want[:, None]).max():.3e}, "
              f"max |lse - want| = {np.abs(got_lse - np.log(cnt)[None]).max():.3e}")
        for h in range(Hq):
            np.testing.assert_allclose(got[:, h], want, rtol=ULP2[dtype], atol=1e-6, err_msg=f"seq {b} head {h}")
            np.testing.assert_allclose(got_lse[h], np.log(cnt), rtol=0, atol=1e-5, err_msg=f"seq {b} head {h}")


# ---- 5. a dominant key ----
def pack_cases(p):
    """every (batch, kv head) case of a prefill_cases problem as a sequence of its own: q [B * Hkv * Sq, G, D], k / v
    [B * Hkv * Sk, 1, D] device tensors, cu_q, cu_k"""
    tq, tk, tv = pc.device_inputs(p)
    n = p.B * p.Hkv
    q = tq.reshape(p.B, p.Hkv, p.G, p.Sq, p.D).permute(0, 1, 3, 2, 4).reshape(n * p.Sq, p.G, p.D).contiguous()
    k = tk.reshape(n * p.Sk, 1, p.D).contiguous()
    v = tv.reshape(n * p.Sk, 1, p.D).contiguous()
    return q, k, v, [i * p.Sq for i in range(n + 1)], [i * p.Sk for i in range(n + 1)]


def unpack(p, o, lse):
    """o [n * Sq, G, D], lse [G, n * Sq] of the packed call -> [B, Hq, Sq, D], [B, Hq, Sq]"""
    o = o.reshape(p.B, p.Hkv, p.Sq, p.G, p.D).permute(0, 1, 3, 2, 4).reshape(p.B, p.Hq, p.Sq, p.D)
    lse = lse.reshape(p.G, p.B, p.Hkv, p.Sq).permute(1, 2, 0, 3).reshape(p.B, p.Hq, p.Sq)
    return o, lse


def check4(o, lse, want, lse_want, dtype):
    np.testing.assert_allclose(o, want, atol=TOL[dtype], rtol=TOL[dtype])
    fin = np.isfinite(lse_want)
    np.testing.assert_allclose(lse[fin], lse_want[fin], atol=LSE_TOL, rtol=LSE_TOL)
    assert np.all(lse[~fin] == -np.inf) and np.all(o[~fin] == 0)


@pytest.mark.parametrize("Sq,Sk", [(299, 299), (100, 299)])
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_dominant_key(sfa, Sq, Sk, dtype):
    """prefill_cases.softmax_stress("spike"): one key j* carries all the weight of the rows that see it, a case per
    (batch, kv head) with j* on every tile edge; here every case is a sequence of its own.  The key's weight packs to 1.0
    and every other is at most 2^-40 of it (tests/test_prefill_numerics_gpu.py::test_softmax_stress): the row returns the
    bits of V[j*]."""
    D, G = 128, 1
    p = pc.softmax_stress("spike", dtype, D, G, Sq, Sk)
    q, k, v, cu_q, cu_k = pack_cases(p)
    for causal in (False, True):
        want, lse_want = p.oracle(causal)
        sees = np.repeat(p.sees(causal), G, axis=1)                                 # [B, Hq, Sq]
        vrow = np.repeat(pc.v_bits(p)[np.arange(p.B)[:, None], np.arange(p.Hkv)[None, :], p.spike], G, axis=1)
        o, lse = varlen_call(sfa, q, k, v, cu_q, cu_k, causal)
        o, lse = unpack(p, o, lse)
        check4(o.float().cpu().numpy(), lse.cpu().numpy(), want, lse_want, dtype)
        b16 = bits(o)
        np.testing.assert_array_equal(b16[sees], np.broadcast_to(vrow[:, :, None, :], b16.shape)[sees],
                                      err_msg=f"causal={causal}: a row that sees key j* must return V[j*]")
        assert sees.any()


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_staircase(sfa, dtype):
    """staircase64: the row maxima rise by tens of log2 units from one 64-key tile to the next: parity at TOL."""
    p = pc.softmax_stress("staircase64", dtype, 128, 1, 299, 299)
    q, k, v, cu_q, cu_k = pack_cases(p)
    for causal in (False, True):
        want, lse_want = p.oracle(causal)
        o, lse = unpack(p, *varlen_call(sfa, q, k, v, cu_q, cu_k, causal))
        check4(o.float().cpu().numpy(), lse.cpu().numpy(), want, lse_want, dtype)


# ---- 6. strided views ----
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("D", [64, 128])
def test_strided_views(sfa, dtype, D):
    """q, k and v as the three slices of one packed [T, Hq + 2 Hkv, D] tensor (n_q = n_k); then guarded views
    (prefill_cases.guarded: NaN between rows and heads, guard rows before the first and past the last) with o a view inside a
    NaN-filled allocation; then K and V with a head stride of 0.  Each equals the contiguous call's bits."""
    lens, Hq, Hkv, causal = [300, 0, 1, 257, 64], 4, 2, True
    cu = cu_of(lens)
    T = cu[-1]
    rng = np.random.default_rng(D)
    qkv = dev16(round_to(rng.standard_normal((T, Hq + 2 * Hkv, D)), dtype), dtype)
    tq, tk, tv = qkv[:, :Hq], qkv[:, Hq:Hq + Hkv], qkv[:, Hq + Hkv:]
    assert tq.stride(0) == (Hq + 2 * Hkv) * D == tk.stride(0) and not tk.is_contiguous()
    o0, lse0 = varlen_call(sfa, tq.contiguous(), tk.contiguous(), tv.contiguous(), cu, cu, causal)
    want, lse_want, rows = prefill_varlen_ref(*(t.float().cpu().numpy() for t in (tq, tk, tv)), cu, cu, causal)
    check(o0.float().cpu().numpy(), lse0.cpu().numpy(), want, lse_want, rows, dtype)
    o1, lse1 = varlen_call(sfa, tq, tk, tv, cu, cu, causal)
    assert torch.equal(o1.view(torch.int16), o0.view(torch.int16)) and torch.equal(lse1, lse0)
    # guarded: prefill_cases.guarded takes [B, H, S, D]; its view [0] transposed is [S, H, D] with NaN between rows and heads
    nan = NAN16[dtype]
    g = lambda t, guard, copy=True: tuple(x[0].transpose(0, 1) if i else x for i, x in
                                          enumerate(pc.guarded(t.transpose(0, 1)[None], guard, nan, copy=copy)))
    _, gq = g(tq, pc.GUARD_Q)
    _, gk = g(tk, pc.GUARD_K)
    _, gv = g(tv, pc.GUARD_K)
    o_base, go = g(tq, pc.GUARD_Q, copy=False)
    assert gq.shape == tq.shape and gq.stride(2) == 1 and gq.stride(0) == D + pc.PAD_D
    o2, lse2 = varlen_call(sfa, gq, gk, gv, cu, cu, causal, out=go)
    assert o2.data_ptr() == go.data_ptr()
    assert torch.equal(o2.contiguous().view(torch.int16), o0.view(torch.int16)) and torch.equal(lse2, lse0)
    assert np.all(pc.outside(o_base, pc.GUARD_Q, T, D) == nan)
    # head stride 0: one kv head's rows serving every kv head
    k0, v0 = tk[:, :1].contiguous(), tv[:, :1].contiguous()
    ke, ve = k0.expand(T, Hkv, D), v0.expand(T, Hkv, D)
    assert ke.stride(1) == 0 and ve.stride(1) == 0
    o3, lse3 = varlen_call(sfa, tq, ke, ve, cu, cu, causal)
    o4, lse4 = varlen_call(sfa, tq, ke.contiguous(), ve.contiguous(), cu, cu, causal)
    assert torch.equal(o3.view(torch.int16), o4.view(torch.int16)) and torch.equal(lse3, lse4)
    want, lse_want, rows = prefill_varlen_ref(tq.float().cpu().numpy(), k0.float().cpu().numpy(), v0.float().cpu().numpy(),
                                              cu, cu, causal)
    check(o3.float().cpu().numpy(), lse3.cpu().numpy(), want, lse_want, rows, dtype)


# ---- 7. bad cu_seqlens ----
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("D", [64, 128])
def test_a_sequence_that_runs_backwards_is_skipped(sfa, dtype, D):
    cu_q, cu_k = [0, 10, 20, 30], [0, 100, 50, 300]
    rng = np.random.default_rng(D + 1)
    q = round_to(rng.standard_normal((30, 4, D)), dtype)
    k = round_to(rng.standard_normal((300, 2, D)), dtype)
    v = round_to(rng.standard_normal((300, 2, D)), dtype)
    want, lse_want, rows = prefill_varlen_ref(q, k, v, cu_q, cu_k, True)
    assert rows[:10].all() and not rows[10:20].any() and rows[20:].all()
    o, lse = varlen_call(sfa, dev16(q, dtype), dev16(k, dtype), dev16(v, dtype), cu_q, cu_k, True, prefill=FILL)
    check(o.float().cpu().numpy(), lse.cpu().numpy(), want, lse_want, rows, dtype, fill=FILL)


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("D", [64, 128])
def test_a_sequence_past_total_k_is_skipped(sfa, dtype, D):
    """cu_k[batch] = 300 is above the total_k = 260 passed but inside the allocation of 300 rows, so that not even a wrong
    implementation leaves valid memory: the last sequence is skipped, the others are correct."""
    cu_q, cu_k = [0, 10, 20, 30], [0, 100, 200, 300]
    rng = np.random.default_rng(D + 2)
    q = round_to(rng.standard_normal((30, 4, D)), dtype)
    k = round_to(rng.standard_normal((300, 2, D)), dtype)
    v = round_to(rng.standard_normal((300, 2, D)), dtype)
    want, lse_want, rows = prefill_varlen_ref(q, k[:260], v[:260], cu_q, cu_k, False)
    assert rows[:20].all() and not rows[20:].any()
    tq = dev16(q, dtype)
    out = torch.full(tq.shape, FILL, dtype=tq.dtype, device=DEV)
    o, lse = call_with_lse(sfa, tq, dev16(k, dtype), dev16(v, dtype), out, cu_dev(cu_q), cu_dev(cu_k), False, FILL,
                           total_k=260)
    check(o.float().cpu().numpy(), lse.cpu().numpy(), want, lse_want, rows, dtype, fill=FILL)


# ---- 8. the contents of the workspace never matter ----
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("D", [64, 128])
def test_workspace_contents_never_matter(sfa, dtype, D):
    q, k, v, cu_q, cu_k, want, lse_want, rows = problem("B", dtype, D, True)
    tq, tk, tv = dev16(q, dtype), dev16(k, dtype), dev16(v, dtype)
    need = sfa.prefill_varlen_workspace_bytes(len(cu_q) - 1, q.shape[0])
    assert need == 256
    outs = []
    for fill in (0x00, 0xFF):
        ws = torch.full((need,), fill, dtype=torch.uint8, device=DEV)
        o, lse = varlen_call(sfa, tq, tk, tv, cu_q, cu_k, True, workspace=ws)
        outs.append((o.view(torch.int16).cpu(), lse.cpu()))
    assert torch.equal(outs[0][0], outs[1][0])
    assert torch.equal(outs[0][1], outs[1][1])
    check(outs[1][0].view(TDT[dtype]).float().numpy(), outs[1][1].numpy(), want, lse_want, rows, dtype)
    cq, ck = cu_dev(cu_q), cu_dev(cu_k)
    with pytest.raises(sfa.SfaError, match="sfa_prefill_varlen_fwd: workspace has") as e:       # one byte short
        sfa.flash_attn_varlen_fwd(tq, tk, tv, cq, ck, causal=True, workspace=ws[:need - 1])
    assert e.value.status == -5
    big = torch.zeros(need + 256, dtype=torch.uint8, device=DEV)
    with pytest.raises(sfa.SfaError, match="sfa_prefill_varlen_fwd: workspace must be 256-byte aligned") as e:
        sfa.flash_attn_varlen_fwd(tq, tk, tv, cq, ck, causal=True, workspace=big[16:])
    assert e.value.status == -2
    with pytest.raises(sfa.SfaError, match="sfa_prefill_varlen_fwd: workspace is NULL") as e:
        sfa.flash_attn_varlen_fwd(tq, tk, tv, cq, ck, causal=True, workspace=big[:0])
    assert e.value.status == -1
    torch.cuda.synchronize()


# ---- 9. softmax_scale ----
@pytest.mark.parametrize("scale", pc.SCALES)
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("D", [64, 128])
def test_softmax_scale(sfa, scale, dtype, D):
    q, k, v, cu_q, cu_k, want, lse_want, rows = problem("C", dtype, D, True, scale)
    o, lse = varlen_call(sfa, dev16(q, dtype), dev16(k, dtype), dev16(v, dtype), cu_q, cu_k, True, softmax_scale=scale)
    check(o.float().cpu().numpy(), lse.cpu().numpy(), want, lse_want, rows, dtype)


# ---- 10. the debug knobs ----
def test_debug_knobs_keep_their_values(sfa):
    x = torch.randn(1, 2, 300, 128, device=DEV).bfloat16()
    sfa.flash_attn_split_fwd(x, x, x, causal=True, num_splits=2)
    sfa.flash_attn_fwd(x, x, x, causal=True)
    torch.cuda.synchronize()
    ran, splits = sfa.debug_get("last_prefill_kernel"), sfa.debug_get("last_prefill_splits")
    assert ran > 0 and splits == 2
    q, k, v, cu_q, cu_k, want, lse_want, rows = problem("B", "bf16", 128, True)
    o, lse = varlen_call(sfa, dev16(q, "bf16"), dev16(k, "bf16"), dev16(v, "bf16"), cu_q, cu_k, True)
    check(o.float().cpu().numpy(), lse.cpu().numpy(), want, lse_want, rows, "bf16")
    assert sfa.debug_get("last_prefill_kernel") == ran and sfa.debug_get("last_prefill_splits") == splits


# ---- 11. graph ----
def test_graph_replay_with_new_cu_seqlens(sfa):
    """One captured call on a side stream -- two launches, no parallel branches -- replayed with new q, k, v and new
    contents of both cu arrays: the same batch and totals, other lengths, one of them 0."""
    dtype, D, Hq, Hkv, B, Tq, Tk, causal = "bf16", 128, 4, 2, 4, 700, 900, True
    tq = torch.zeros(Tq, Hq, D, dtype=TDT[dtype], device=DEV)
    tk = torch.zeros(Tk, Hkv, D, dtype=TDT[dtype], device=DEV)
    tv = torch.zeros_like(tk)
    out = torch.zeros_like(tq)
    cq, ck = cu_dev([0] * (B + 1)), cu_dev([0] * (B + 1))
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        sfa.flash_attn_varlen_fwd(tq, tk, tv, cq, ck, causal=causal, out=out)      # warm-up: the stream's workspace exists
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            _, lse = sfa.flash_attn_varlen_fwd(tq, tk, tv, cq, ck, causal=causal, out=out, return_lse=True)
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
            want, lse_want, rows = prefill_varlen_ref(q, k, v, cu_q, cu_k, causal)
            assert not rows[cu_q[-1]:].any()
            for dst, src in ((tq, q), (tk, k), (tv, v)):
                dst.copy_(dev16(src, dtype))
            cq.copy_(cu_dev(cu_q))
            ck.copy_(cu_dev(cu_k))
            out.fill_(FILL)
            lse.fill_(FILL)
            graph.replay()
            side.synchronize()
            check(out.float().cpu().numpy(), lse.cpu().numpy(), want, lse_want, rows, dtype, fill=FILL)


# ---- 12. the pybind surface ----
def test_pybind_mha_varlen_fwd(sfa):
    import star_flash_attn as ext
    dtype = "bf16"
    q, k, v, cu_q, cu_k, want, lse_want, rows = problem("B", dtype, 128, True)
    tq, tk, tv = dev16(q, dtype), dev16(k, dtype), dev16(v, dtype)
    cq, ck = cu_dev(cu_q), cu_dev(cu_k)
    out, lse = ext.mha_varlen_fwd(tq, tk, tv, cq, ck, causal=True, return_lse=True)
    torch.cuda.synchronize()
    check(out.float().cpu().numpy(), lse.cpu().numpy(), want, lse_want, rows, dtype)
    o2, lse2 = sfa.flash_attn_varlen_fwd(tq, tk, tv, cq, ck, causal=True, return_lse=True)
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int16), o2.view(torch.int16)) and torch.equal(lse, lse2)
    (o3,) = ext.mha_varlen_fwd(tq, tk, tv, cq, ck, causal=True)
    torch.cuda.synchronize()
    assert torch.equal(o3.view(torch.int16), o2.view(torch.int16))
    with pytest.raises(RuntimeError, match="head_dim 256"):
        z = torch.zeros(16, 2, 256, device=DEV, dtype=torch.bfloat16)
        ext.mha_varlen_fwd(z, z, z, cu_dev([0, 16]), cu_dev([0, 16]))
