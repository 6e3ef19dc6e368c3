"""GPU tests of sfa_prefill_varlen_split_fwd / flash_attn_varlen_split_fwd / mha_varlen_split_fwd: the packed prefill
forward with each q-tile's key range split over several workgroups and a combine over their fp32 partials, against
tests/prefill_varlen_split_ref.py on identically rounded inputs.  The reference is computed once per problem, at the
first request of its batch: the references of different requests differ by reassociation in fp64 only
(tests/test_prefill_varlen_split_cpu.py, 1e-9).

Tolerances: o within the project's TOL (fp16 2e-3, bf16 1.6e-2: tests/test_prefill_gpu.py::TOL), lse within 2e-3
(LSE_TOL["exact"] of tests/test_prefill_gpu.py; the split kernels are exact-scale kernels).  After every call
sfa_debug_get("last_prefill_splits") must hold the resolved count.  The batches are those of the reference module: the
smallest that reach each edge of the partition."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import prefill_cases as pc
from oracle import round_to
from prefill_split_ref import key_tiles, resolved_splits, tiles_per_split
from prefill_varlen_ref import cu_of, plan_bound
from prefill_varlen_split_ref import BATCHES, HEADS, LENS, partition, prefill_varlen_split_ref
from test_prefill_varlen_gpu import check4, pack_cases, unpack

pytestmark = pytest.mark.gpu

TOL = {"fp16": 2e-3, "bf16": 1.6e-2}            # tests/test_prefill_gpu.py::TOL
LSE_TOL = 2e-3                                  # tests/test_prefill_gpu.py::LSE_TOL["exact"]
TDT = {"fp16": torch.float16, "bf16": torch.bfloat16}
DEV = "cuda:0"
FILL = 7.0                                      # what o and lse hold before a call that must leave rows alone
CU_Q, CU_K = tuple(cu_of([a for a, _ in LENS])), tuple(cu_of([b for _, b in LENS]))
PAD = 40                                        # rows of the tensors beyond cu[batch]


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


@functools.lru_cache(maxsize=None)
def problem(heads, dtype, D, causal, scale=None):
    """The lengths of batches T and U with PAD rows beyond cu[batch]: (q [Tq, Hq, D], k, v [Tk, Hkv, D] rounded to dtype, the
    fp64 reference o [Tq, Hq, D], lse [Hq, Tq] and the mask of the rows of valid sequences): computed once per key, shared,
    never written to"""
    Hq, Hkv = heads
    rng = np.random.default_rng([Hq, D, 5])
    q = round_to(rng.standard_normal((CU_Q[-1] + PAD, Hq, D)), dtype)
    k = round_to(rng.standard_normal((CU_K[-1] + PAD, Hkv, D)), dtype)
    v = round_to(rng.standard_normal((CU_K[-1] + PAD, Hkv, D)), dtype)
    o, lse, rows = prefill_varlen_split_ref(q, k, v, CU_Q, CU_K, causal, BATCHES["T"][1], BATCHES["T"][2][0], scale)
    for a in (q, k, v, o, lse, rows):
        a.setflags(write=False)
    return q, k, v, o, lse, rows


def split_call(sfa, tq, tk, tv, cu_q, cu_k, max_k, causal, S, fill=None, total_q=None, total_k=None, workspace=None,
               softmax_scale=None, want_status=0):
    """sfa_prefill_varlen_split_fwd through the C ABI on torch views as they are, with o and lse buffers of the test's own
    (prefilled with `fill`) and, if given, totals smaller than the tensors and a workspace tensor.  Asserts the status and
    that the call resolved S as documented.  Returns (o, lse [Hq, total_q])."""
    lib = sfa._lib.load()
    Tq = tq.shape[0] if total_q is None else total_q
    Tk = tk.shape[0] if total_k is None else total_k
    Hq, D = tq.shape[1], tq.shape[2]
    cq, ck = (c if isinstance(c, torch.Tensor) else cu_dev(c) for c in (cu_q, cu_k))
    B = cq.numel() - 1
    out = torch.full(tq.shape, 0.0 if fill is None else fill, dtype=tq.dtype, device=DEV)
    lse = torch.full((Hq, Tq), 0.0 if fill is None else fill, dtype=torch.float32, device=DEV)
    if workspace is None:
        workspace = torch.empty(sfa.prefill_varlen_split_workspace_bytes(B, Hq, Tq, max_k, D, S), dtype=torch.uint8, device=DEV)
    a = sfa._lib.PrefillVarlenArgs()
    a.q, a.k, a.v, a.o, a.lse = tq.data_ptr(), tk.data_ptr(), tv.data_ptr(), out.data_ptr(), lse.data_ptr()
    a.cu_seqlens_q, a.cu_seqlens_k = cq.data_ptr(), ck.data_ptr()
    a.batch, a.heads_q, a.heads_kv, a.total_q, a.total_k, a.head_dim = B, Hq, tk.shape[1], Tq, Tk, D
    for dst, t in ((a.q_stride, tq), (a.k_stride, tk), (a.v_stride, tv), (a.o_stride, out)):
        dst[0], dst[1] = t.stride(0), t.stride(1)
    a.softmax_scale = float(softmax_scale) if softmax_scale else 0.0
    a.causal = 1 if causal else 0
    a.dtype = sfa._lib.DTYPE_FP16 if tq.dtype == torch.float16 else sfa._lib.DTYPE_BF16
    st = lib.sfa_prefill_varlen_split_fwd(ctypes.byref(a), max_k, S, ctypes.c_void_p(workspace.data_ptr()) if workspace.numel() else None,
                                          workspace.numel(), ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))
    assert st == want_status, (st, lib.sfa_last_error())
    torch.cuda.synchronize()
    if st == 0 and S >= 1:
        assert sfa.debug_get("last_prefill_splits") == resolved_splits(max_k, S), (S, sfa.debug_get("last_prefill_splits"))
    return out, lse


def check(o, lse, want, lse_want, rows, dtype, fill=None):
    """o [Tq, Hq, D], lse [Hq, Tq] device tensors against the reference on the rows of valid sequences; the others hold
    `fill`"""
    o, lse = o.float().cpu().numpy(), lse.cpu().numpy()
    np.testing.assert_allclose(o[rows], want[rows], atol=TOL[dtype], rtol=TOL[dtype])
    fin = np.isfinite(lse_want) & rows[None, :]
    none = ~np.isfinite(lse_want) & rows[None, :]
    np.testing.assert_allclose(lse[fin], lse_want[fin], atol=LSE_TOL, rtol=LSE_TOL)
    assert np.all(lse[none] == -np.inf)                         # a row that sees no key: exactly 0 and -inf
    assert np.all(o.transpose(1, 0, 2)[none] == 0)
    if fill is not None:
        assert np.all(o[~rows] == fill) and np.all(lse[:, ~rows] == fill)


def same(a, b):
    return torch.equal(a[0].view(torch.int16), b[0].view(torch.int16)) and torch.equal(a[1], b[1])


def cases(names=("T", "U128", "U64"), heads=HEADS, dtypes=("fp16", "bf16"), Ds=(64, 128), causals=(True, False)):
    return [pytest.param(n, h, dt, D, c, id=f"{n}-{h[0]}over{h[1]}-{dt}-D{D}-{'causal' if c else 'full'}")
            for n in names for h in heads for dt in dtypes for D in Ds for c in causals]


def test_the_batches_reach_their_edges():
    assert key_tiles(520) == 9 and [nk <= 520 for _, nk in LENS] == [True] * 6 + [False]
    assert CU_Q[-1] == 927 and plan_bound(len(LENS), CU_Q[-1] + PAD) == 10
    assert partition(128, 2) == (1, 2) and key_tiles(1100) - 1 == 17       # the last split of the long sequence: 17 tiles
    assert partition(64, 2) == (1, 1)


# ---- 1. parity ----
@pytest.mark.parametrize("name,heads,dtype,D,causal", cases())
def test_parity(sfa, name, heads, dtype, D, causal):
    """o and lse at the project's tolerances for every request of the batch; exact zeros and -inf where no key is visible
    (the sequence without keys; under the causal mask the first 200 rows of (300, 100)); the 40 padding rows beyond
    cu[batch] -- NaN in q, k, v -- keep their fill."""
    _, max_k, requests = BATCHES[name]
    q, k, v, want, lse_want, rows = problem(heads, dtype, D, causal)
    assert not rows[CU_Q[-1]:].any() and rows[:CU_Q[-1]].all()
    tq, tk, tv = dev16(q, dtype), dev16(k, dtype), dev16(v, dtype)
    tq[CU_Q[-1]:] = float("nan")
    tk[CU_K[-1]:] = float("nan")
    tv[CU_K[-1]:] = float("nan")
    for S in requests:
        o, lse = split_call(sfa, tq, tk, tv, CU_Q, CU_K, max_k, causal, S, fill=FILL)
        check(o, lse, want, lse_want, rows, dtype, fill=FILL)
        lse = lse.cpu().numpy()
        assert np.all(lse[:, CU_Q[3]:CU_Q[4]] == -np.inf)                   # (5, 0)
        if causal:
            assert np.all(lse[:, CU_Q[5]:CU_Q[5] + 200] == -np.inf) and np.all(np.isfinite(lse[:, CU_Q[5] + 200:CU_Q[6]]))


# ---- 2. bits ----
def same_chunk_request(n_k, C):
    """a request under which sfa_prefill_split_fwd on a sequence of n_k keys cuts chunks of C tiles, or None"""
    for S in range(1, key_tiles(n_k) + 1):
        if tiles_per_split(n_k, S) == C:
            return S
    return None


@pytest.mark.parametrize("name,heads,dtype,D,causal", cases(("T",), Ds=(128,)) + cases(("T",), HEADS[:1], ("bf16",), (64,)))
def test_a_sequence_gets_the_bits_of_the_rectangular_split_call(sfa, name, heads, dtype, D, causal):
    """Every sequence of T inside the hint, every request: where a request exists under which flash_attn_split_fwd on the
    sequence's own [1, H, n, D] view cuts the same C (then it covers the same tiles per split), the packed call returns
    that call's o and lse bit for bit."""
    _, max_k, requests = BATCHES[name]
    q, k, v, _, _, _ = problem(heads, dtype, D, causal)
    tq, tk, tv = dev16(q, dtype), dev16(k, dtype), dev16(v, dtype)
    assert (partition(520, 3)[0], same_chunk_request(300, 3)) == (3, 2)         # the example of the issue
    met = 0
    for S in requests:
        C, _ = partition(max_k, S)
        o, lse = split_call(sfa, tq, tk, tv, CU_Q, CU_K, max_k, causal, S)
        for b, (nq, nk) in enumerate(LENS):
            S1 = same_chunk_request(nk, C) if 0 < nk <= max_k and nq > 0 else None
            if S1 is None:
                continue
            q0, k0 = CU_Q[b], CU_K[b]
            view = lambda t, r0, n: t[r0:r0 + n].transpose(0, 1)[None]
            o1, lse1 = sfa.flash_attn_split_fwd(view(tq, q0, nq), view(tk, k0, nk), view(tv, k0, nk), causal=causal,
                                                num_splits=S1, return_lse=True)
            torch.cuda.synchronize()
            if resolved_splits(nk, S1) == 1:
                continue                        # that call forwarded to the unsplit kernel: another walk
            met += 1
            assert torch.equal(o1[0].transpose(0, 1).contiguous().view(torch.int16), o[q0:q0 + nq].view(torch.int16)), (S, b)
            assert torch.equal(lse1[0], lse[:, q0:q0 + nq]), (S, b)
    assert met >= 10


@pytest.mark.parametrize("name,heads,dtype,D,causal", cases(("U64", "T")))
def test_one_split_is_the_unsplit_packed_call(sfa, name, heads, dtype, D, causal):
    """A resolved count of 1 -- the hint of one tile under any request, request 1 under any hint -- is
    flash_attn_varlen_fwd, bit for bit, over the plan-only workspace; the padding rows keep their fill."""
    _, max_k, requests = BATCHES[name]
    S = requests[0] if name == "U64" else 1
    q, k, v, want, lse_want, rows = problem(heads, dtype, D, causal)
    tq, tk, tv = dev16(q, dtype), dev16(k, dtype), dev16(v, dtype)
    ref = sfa.flash_attn_varlen_fwd(tq, tk, tv, cu_dev(CU_Q), cu_dev(CU_K), causal=causal, return_lse=True)
    torch.cuda.synchronize()
    ws = torch.full((sfa.prefill_varlen_workspace_bytes(len(LENS), tq.shape[0]),), 0xFF, dtype=torch.uint8, device=DEV)
    o, lse = split_call(sfa, tq, tk, tv, CU_Q, CU_K, max_k, causal, S, fill=FILL, workspace=ws)
    assert sfa.debug_get("last_prefill_splits") == 1
    n = CU_Q[-1]
    assert same((o[:n], lse[:, :n]), (ref[0][:n], ref[1][:, :n]))
    check(o, lse, want, lse_want, rows, dtype, fill=FILL)


@pytest.mark.parametrize("name,heads,dtype,D,causal", cases(("T", "U128"), Ds=(128,)) + cases(("T",), HEADS[:1], ("fp16",), (64,)))
def test_alone_equals_batched(sfa, name, heads, dtype, D, causal):
    _, max_k, requests = BATCHES[name]
    q, k, v, _, _, _ = problem(heads, dtype, D, causal)
    tq, tk, tv = dev16(q, dtype), dev16(k, dtype), dev16(v, dtype)
    for S in requests[:3]:
        o, lse = split_call(sfa, tq, tk, tv, CU_Q, CU_K, max_k, causal, S)
        for b, (nq, nk) in enumerate(LENS):
            if nq == 0:
                continue
            q0, k0 = CU_Q[b], CU_K[b]
            # its own slices; a sequence with no keys still needs a K / V pointer: one row it does not own
            ks, vs = (tk[k0:k0 + nk], tv[k0:k0 + nk]) if nk else (tk[:1], tv[:1])
            o1, lse1 = split_call(sfa, tq[q0:q0 + nq], ks, vs, [0, nq], [0, nk], max_k, causal, S, total_k=nk)
            assert same((o1, lse1), (o[q0:q0 + nq], lse[:, q0:q0 + nq])), (S, b)


# ---- 3. unread memory ----
@pytest.mark.parametrize("name,heads,dtype,D,causal", cases(("T", "U128"), Ds=(128,)) + cases(("T",), HEADS[1:], ("bf16",), (64,)))
def test_poisoned_neighbours(sfa, name, heads, dtype, D, causal):
    """q, K and V of every other sequence and of the padding rows are NaN: sequence b's rows are the clean call's bit for
    bit.  A key read from the neighbour at a ragged last tile or past a split's end, even under a mask, would turn the row
    into NaN (0 * NaN)."""
    _, max_k, requests = BATCHES[name]
    q, k, v, _, _, _ = problem(heads, dtype, D, causal)
    tq, tk, tv = dev16(q, dtype), dev16(k, dtype), dev16(v, dtype)
    for S in (requests[0], requests[-1]):
        o, lse = split_call(sfa, tq, tk, tv, CU_Q, CU_K, max_k, causal, S)
        for b, (nq, nk) in enumerate(LENS):
            if nq == 0:
                continue
            q0, k0 = CU_Q[b], CU_K[b]
            pq, pk, pv = (torch.full_like(t, float("nan")) for t in (tq, tk, tv))
            pq[q0:q0 + nq], pk[k0:k0 + nk], pv[k0:k0 + nk] = tq[q0:q0 + nq], tk[k0:k0 + nk], tv[k0:k0 + nk]
            o1, lse1 = split_call(sfa, pq, pk, pv, CU_Q, CU_K, max_k, causal, S)
            assert same((o1[q0:q0 + nq], lse1[:, q0:q0 + nq]), (o[q0:q0 + nq], lse[:, q0:q0 + nq])), (S, b)


@pytest.mark.parametrize("name,heads,dtype,D,causal", cases(("T", "U128"), Ds=(128,)) + cases(("T",), HEADS[:1], ("fp16",), (64,)))
def test_workspace_contents_never_matter(sfa, name, heads, dtype, D, causal):
    """The same call over workspaces of 0x00 bytes, 0xFF bytes (NaN in every float, -1 in every index) and float NaN:
    bit-identical o and lse.  A partial that nobody wrote must not be read, and an empty one must be skipped, not
    multiplied by 0."""
    _, max_k, requests = BATCHES[name]
    q, k, v, want, lse_want, rows = problem(heads, dtype, D, causal)
    tq, tk, tv = dev16(q, dtype), dev16(k, dtype), dev16(v, dtype)
    for S in (requests[0], requests[-1]):
        need = sfa.prefill_varlen_split_workspace_bytes(len(LENS), heads[0], tq.shape[0], max_k, D, S)
        outs = []
        for fill in (0x00, 0xFF, None):
            if fill is None:
                ws = torch.full((need // 4,), float("nan"), dtype=torch.float32, device=DEV).view(torch.uint8)
            else:
                ws = torch.full((need,), fill, dtype=torch.uint8, device=DEV)
            outs.append(split_call(sfa, tq, tk, tv, CU_Q, CU_K, max_k, causal, S, fill=FILL, workspace=ws))
        assert same(outs[0], outs[1]) and same(outs[0], outs[2])        # (-inf == -inf; a NaN would differ from itself)
        check(*outs[2], want, lse_want, rows, dtype, fill=FILL)


# ---- 4. exact count at the seams ----
ULP2 = {"bf16": 2.0 ** -7, "fp16": 2.0 ** -10}  # 2 ulp of the 16-bit type
# under the hint of 520 keys the requests cut chunks of 5, 3, 2 and 1 tiles: seams at keys 320 / 192 / 128 / every 64.
# Key ranges that end at a seam, one key past it and well inside the next chunk; 577 keys are one past the hint's nine
# tiles and 1100 far past them (the open-ended last split)
SEAM_LENS = [(64, 192), (100, 193), (300, 320), (257, 321), (1, 129), (30, 250), (64, 577), (40, 1100)]


@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_exact_count_at_the_seams(sfa, causal, D, dtype):
    """The construction of tests/test_prefill_varlen_gpu.py::test_exact_count_at_the_seams under every explicit request:
    q = 0, so every score is 0 and every weight 1; V row j -- j the index within the sequence -- is the unit vector of
    j % D.  Every partial sum is an exact integer, every reference max 0 and every merge weight 2^0, so
    o[i, d] = c_i(d) / cnt_i and lse = log cnt_i: a tile counted twice or dropped at a seam, the open-ended last split's
    included, moves an element by a whole 1 / cnt.  rtol 2 ulp of the type, atol 1e-6; lse to 1e-5."""
    Hq, Hkv, max_k = 2, 1, 520
    cu_q, cu_k = cu_of([a for a, _ in SEAM_LENS]), cu_of([b for _, b in SEAM_LENS])
    rng = np.random.default_rng(11)
    q = np.zeros((cu_q[-1], Hq, D))
    k = round_to(rng.standard_normal((cu_k[-1], Hkv, D)), dtype)
    v = np.zeros((cu_k[-1], Hkv, D))
    for b, (nq, nk) in enumerate(SEAM_LENS):
        v[cu_k[b] + np.arange(nk), :, np.arange(nk) % D] = 1.0
    tq, tk, tv = dev16(q, dtype), dev16(k, dtype), dev16(v, dtype)
    for S in BATCHES["T"][2]:
        o, lse = split_call(sfa, tq, tk, tv, cu_q, cu_k, max_k, causal, S)
        o, lse = o.float().cpu().numpy(), lse.cpu().numpy()
        for b, (nq, nk) in enumerate(SEAM_LENS):
            onehot = np.zeros((nk, D))
            onehot[np.arange(nk), np.arange(nk) % D] = 1.0
            mask = np.ones((nq, nk), bool)
            if causal:
                mask = np.arange(nk)[None, :] <= np.arange(nq)[:, None] + (nk - nq)
            cnt = mask.sum(axis=1).astype(np.float64)
            assert cnt.min() >= 1
            want = (mask.astype(np.float64) @ onehot) / cnt[:, None]           # [nq, D]
            got, got_lse = o[cu_q[b]:cu_q[b + 1]], lse[:, cu_q[b]:cu_q[b + 1]]
            print(f"S={S} seq {b} causal={causal} D={D} {dtype}: max |o - want| = {np.abs(got - want[:, None]).max():.3e}, "
                  f"max |lse - want| = {np.abs(got_lse - np.log(cnt)[None]).max():.3e}")
            for h in range(Hq):
                np.testing.assert_allclose(got[:, h], want, rtol=ULP2[dtype], atol=1e-6, err_msg=f"S {S} seq {b} head {h}")
                np.testing.assert_allclose(got_lse[h], np.log(cnt), rtol=0, atol=1e-5, err_msg=f"S {S} seq {b} head {h}")


# ---- 5. adversarial numerics ----
@pytest.mark.parametrize("kind", ["spike", "alone"])
@pytest.mark.parametrize("Sq,Sk", [(299, 299), (100, 299)])
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_dominant_key_in_the_first_a_middle_and_the_last_split(sfa, kind, Sq, Sk, dtype):
    """tests/test_prefill_split_gpu.py::test_dominant_key_in_a_later_split with every (batch, kv head) case a sequence of
    its own: one key j* carries all the weight of the rows that see it, j* on every tile edge -- under the hint of 299 keys
    and request 3 (tiles [0, 2), [2, 4), [4, 5)) in the first, the middle and the last split, under request 5 a tile each.
    The other splits' merge weights are at most 2^-46: the row returns the bits of V[j*]."""
    D, G = 128, 1
    p = pc.softmax_stress(kind, dtype, D, G, Sq, Sk)
    q, k, v, cu_q, cu_k = pack_cases(p)
    spl = p.spike // 128
    assert (spl == 0).any() and (spl == 1).any() and (spl == 2).any()
    for causal in (False, True):
        want, lse_want = p.oracle(causal)
        sees = np.repeat(p.sees(causal), G, axis=1)                                 # [B, Hq, Sq]
        vrow = np.repeat(pc.v_bits(p)[np.arange(p.B)[:, None], np.arange(p.Hkv)[None, :], p.spike], G, axis=1)
        for S in (2, 3, 5):
            o, lse = unpack(p, *split_call(sfa, q, k, v, cu_q, cu_k, Sk, causal, S))
            check4(o.float().cpu().numpy(), lse.cpu().numpy(), want, lse_want, dtype)
            b16 = o.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)
            np.testing.assert_array_equal(b16[sees], np.broadcast_to(vrow[:, :, None, :], b16.shape)[sees],
                                          err_msg=f"{kind} causal={causal} S={S}: a row that sees key j* must return V[j*]")
            assert sees.any() or (kind == "alone" and causal)


@pytest.mark.parametrize("Sq,Sk", [(299, 299), (100, 299)])
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_staircase_across_seams(sfa, Sq, Sk, dtype):
    """staircase64: the row maxima rise by tens of log2 units from one 64-key tile to the next, so the splits' reference
    maxima differ by that much and all but the last merge weight underflow towards 0: parity at TOL."""
    p = pc.softmax_stress("staircase64", dtype, 128, 1, Sq, Sk)
    q, k, v, cu_q, cu_k = pack_cases(p)
    for causal in (False, True):
        want, lse_want = p.oracle(causal)
        for S in (2, 3, 5):
            o, lse = unpack(p, *split_call(sfa, q, k, v, cu_q, cu_k, Sk, causal, S))
            check4(o.float().cpu().numpy(), lse.cpu().numpy(), want, lse_want, dtype)


# ---- 6. invalid sequences ----
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("D", [64, 128])
def test_invalid_sequences_are_skipped(sfa, dtype, D):
    """A sequence that runs backwards in cu_k; then one whose cu_k[batch] = 300 is above the total_k = 260 passed but inside
    the allocation of 300 rows, so that not even a wrong implementation leaves valid memory.  The invalid sequence's rows
    keep their fill in o and lse; the others are correct."""
    rng = np.random.default_rng(D + 1)
    q = round_to(rng.standard_normal((30, 4, D)), dtype)
    k = round_to(rng.standard_normal((300, 2, D)), dtype)
    v = round_to(rng.standard_normal((300, 2, D)), dtype)
    tq, tk, tv = dev16(q, dtype), dev16(k, dtype), dev16(v, dtype)
    for cu_q, cu_k, total_k, causal, valid in (([0, 10, 20, 30], [0, 100, 50, 300], 300, True, [0, 2]),
                                               ([0, 10, 20, 30], [0, 100, 200, 300], 260, False, [0, 1])):
        for S in (2, 4):
            want, lse_want, rows = prefill_varlen_split_ref(q, k[:total_k], v[:total_k], cu_q, cu_k, causal, 128, S)
            assert [b for b in range(3) if rows[10 * b]] == valid
            o, lse = split_call(sfa, tq, tk, tv, cu_q, cu_k, 128, causal, S, fill=FILL, total_k=total_k)
            check(o, lse, want, lse_want, rows, dtype, fill=FILL)


# ---- 7. the workspace checks ----
def test_workspace_errors_and_the_count_a_workspace_holds(sfa):
    dtype, D, heads, causal = "bf16", 128, HEADS[0], True
    q, k, v, want, lse_want, rows = problem(heads, dtype, D, causal)
    tq, tk, tv = dev16(q, dtype), dev16(k, dtype), dev16(v, dtype)
    B, Tq, max_k = len(LENS), tq.shape[0], 520
    size = lambda S: sfa.prefill_varlen_split_workspace_bytes(B, heads[0], Tq, max_k, D, S)
    need, plan = size(4), sfa.prefill_varlen_workspace_bytes(B, Tq)
    assert need > size(2) > plan == size(1)
    big = torch.zeros(need + 256, dtype=torch.uint8, device=DEV)
    lib = sfa._lib.load()
    split_call(sfa, tq, tk, tv, CU_Q, CU_K, max_k, causal, 4, workspace=big[:need - 1], want_status=-5)     # one byte short
    assert lib.sfa_last_error().startswith(b"sfa_prefill_varlen_split_fwd: workspace has")
    split_call(sfa, tq, tk, tv, CU_Q, CU_K, max_k, causal, 4, workspace=big[16:], want_status=-2)
    assert lib.sfa_last_error().startswith(b"sfa_prefill_varlen_split_fwd: workspace must be 256-byte aligned")
    split_call(sfa, tq, tk, tv, CU_Q, CU_K, max_k, causal, 4, workspace=big[:0], want_status=-1)            # NULL, S' = 3
    assert lib.sfa_last_error().startswith(b"sfa_prefill_varlen_split_fwd: workspace is NULL")
    with pytest.raises(sfa.SfaError, match="sfa_prefill_varlen_split_fwd: workspace has") as e:
        sfa.flash_attn_varlen_split_fwd(tq, tk, tv, cu_dev(CU_Q), cu_dev(CU_K), max_k, causal=causal, num_splits=4,
                                        workspace=big[:need - 1])
    assert e.value.status == -5
    # the library's choice: 4 heads and 6 q-tiles against 32768 keys split; a plan-only workspace runs with 1, one that
    # holds 2 with 2
    hint = 32768
    auto = sfa.prefill_varlen_auto_splits(B, heads[0], Tq, hint, D, causal=causal)
    assert auto > 2
    ref = sfa.flash_attn_varlen_fwd(tq, tk, tv, cu_dev(CU_Q), cu_dev(CU_K), causal=causal, return_lse=True)
    for S in (0, -1):
        o, lse = split_call(sfa, tq, tk, tv, CU_Q, CU_K, hint, causal, S, workspace=big[:plan])
        assert sfa.debug_get("last_prefill_splits") == 1
        assert same((o[:CU_Q[-1]], lse[:, :CU_Q[-1]]), (ref[0][:CU_Q[-1]], ref[1][:, :CU_Q[-1]]))
    two = torch.zeros(sfa.prefill_varlen_split_workspace_bytes(B, heads[0], Tq, hint, D, 2), dtype=torch.uint8, device=DEV)
    o, lse = split_call(sfa, tq, tk, tv, CU_Q, CU_K, hint, causal, 0, fill=FILL, workspace=two)
    assert sfa.debug_get("last_prefill_splits") == 2
    check(o, lse, want, lse_want, rows, dtype, fill=FILL)
    o, lse = sfa.flash_attn_varlen_split_fwd(tq, tk, tv, cu_dev(CU_Q), cu_dev(CU_K), hint, causal=causal, return_lse=True)
    torch.cuda.synchronize()
    assert sfa.debug_get("last_prefill_splits") == auto
    o[CU_Q[-1]:], lse[:, CU_Q[-1]:] = FILL, FILL
    check(o, lse, want, lse_want, rows, dtype, fill=FILL)


# ---- 8. softmax_scale, strided views, the debug knobs ----
@pytest.mark.parametrize("scale", pc.SCALES)
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("D", [64, 128])
def test_softmax_scale(sfa, scale, dtype, D):
    q, k, v, want, lse_want, rows = problem(HEADS[0], dtype, D, True, scale)
    tq, tk, tv = dev16(q, dtype), dev16(k, dtype), dev16(v, dtype)
    for S in (3, 9):
        o, lse = split_call(sfa, tq, tk, tv, CU_Q, CU_K, 520, True, S, fill=FILL, softmax_scale=scale)
        check(o, lse, want, lse_want, rows, dtype, fill=FILL)


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("D", [64, 128])
def test_strided_views(sfa, dtype, D):
    """q, k and v as the three slices of one packed [T, Hq + 2 Hkv, D] tensor (n_q = n_k): the contiguous call's bits."""
    lens, Hq, Hkv, causal, max_k = [300, 0, 1, 257, 64], 4, 2, True, 300
    cu = cu_of(lens)
    rng = np.random.default_rng(D)
    qkv = dev16(round_to(rng.standard_normal((cu[-1], Hq + 2 * Hkv, D)), dtype), dtype)
    tq, tk, tv = qkv[:, :Hq], qkv[:, Hq:Hq + Hkv], qkv[:, Hq + Hkv:]
    assert tq.stride(0) == (Hq + 2 * Hkv) * D == tk.stride(0) and not tk.is_contiguous()
    want, lse_want, rows = prefill_varlen_split_ref(*(t.float().cpu().numpy() for t in (tq, tk, tv)), cu, cu, causal, max_k, 3)
    for S in (3, 5):
        o0, lse0 = split_call(sfa, tq.contiguous(), tk.contiguous(), tv.contiguous(), cu, cu, max_k, causal, S)
        check(o0, lse0, want, lse_want, rows, dtype)
        o1, lse1 = split_call(sfa, tq, tk, tv, cu, cu, max_k, causal, S)
        assert same((o1, lse1), (o0, lse0))
        o2, lse2 = sfa.flash_attn_varlen_split_fwd(tq, tk, tv, cu_dev(cu), cu_dev(cu), max_k, causal=causal, num_splits=S,
                                                   return_lse=True)
        torch.cuda.synchronize()
        assert same((o2, lse2), (o0, lse0))


def test_debug_knobs(sfa):
    """last_prefill_splits is set to the resolved count (1 when the call forwards); last_prefill_kernel keeps its value"""
    x = torch.randn(1, 2, 300, 128, device=DEV).bfloat16()
    sfa.flash_attn_fwd(x, x, x, causal=True)
    torch.cuda.synchronize()
    ran = sfa.debug_get("last_prefill_kernel")
    assert ran > 0
    q, k, v, want, lse_want, rows = problem(HEADS[0], "bf16", 128, True)
    tq, tk, tv = dev16(q, "bf16"), dev16(k, "bf16"), dev16(v, "bf16")
    for max_k, S, resolved in ((520, 4, 3), (520, 100, 9), (64, 4, 1), (520, 1, 1), (128, 7, 2)):
        sfa.flash_attn_varlen_split_fwd(tq, tk, tv, cu_dev(CU_Q), cu_dev(CU_K), max_k, causal=True, num_splits=S)
        torch.cuda.synchronize()
        assert sfa.debug_get("last_prefill_splits") == resolved and sfa.debug_get("last_prefill_kernel") == ran


# ---- 9. graph ----
def test_graph_replay_with_new_cu_seqlens(sfa):
    """One captured call (request 3 under the hint of 400 keys: C = 3, S' = 3) on a side stream -- four launches, no
    parallel branches -- replayed three times with new q, k, v and new contents of both cu arrays under the same batch and
    totals: other lengths, a sequence that becomes empty and one that grows past the hint."""
    dtype, D, Hq, Hkv, B, Tq, Tk, causal, max_k, S = "bf16", 128, 4, 2, 4, 700, 1300, True, 400, 3
    tq = torch.zeros(Tq, Hq, D, dtype=TDT[dtype], device=DEV)
    tk = torch.zeros(Tk, Hkv, D, dtype=TDT[dtype], device=DEV)
    tv = torch.zeros_like(tk)
    out = torch.zeros_like(tq)
    cq, ck = cu_dev([0] * (B + 1)), cu_dev([0] * (B + 1))
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        sfa.flash_attn_varlen_split_fwd(tq, tk, tv, cq, ck, max_k, causal=causal, num_splits=S, out=out)    # warm-up: the stream's workspace exists
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            _, lse = sfa.flash_attn_varlen_split_fwd(tq, tk, tv, cq, ck, max_k, causal=causal, num_splits=S, out=out,
                                                     return_lse=True)
        assert sfa.debug_get("last_prefill_splits") == 3
        replays = [([(300, 300), (1, 1), (257, 400), (64, 64)], 1),
                   ([(100, 400), (0, 0), (333, 100), (256, 256)], 2),           # the second sequence became empty
                   ([(5, 0), (600, 1200), (0, 0), (1, 2)], 3)]                  # ... and now holds 1200 keys, past the hint
        for lens, seed in replays:
            cu_q, cu_k = cu_of([a for a, _ in lens]), cu_of([b for _, b in lens])
            assert cu_q[-1] <= Tq and cu_k[-1] <= Tk
            rng = np.random.default_rng(seed)
            q = round_to(rng.standard_normal((Tq, Hq, D)), dtype)
            k = round_to(rng.standard_normal((Tk, Hkv, D)), dtype)
            v = round_to(rng.standard_normal((Tk, Hkv, D)), dtype)
            want, lse_want, rows = prefill_varlen_split_ref(q, k, v, cu_q, cu_k, causal, max_k, S)
            assert not rows[cu_q[-1]:].any()
            for dst, src in ((tq, q), (tk, k), (tv, v)):
                dst.copy_(dev16(src, dtype))
            cq.copy_(cu_dev(cu_q))
            ck.copy_(cu_dev(cu_k))
            out.fill_(FILL)
            lse.fill_(FILL)
            graph.replay()
            side.synchronize()
            check(out, lse, want, lse_want, rows, dtype, fill=FILL)


# ---- 10. the pybind surface ----
def test_pybind_mha_varlen_split_fwd(sfa):
    import star_flash_attn as ext
    dtype = "bf16"
    q, k, v, want, lse_want, rows = problem(HEADS[0], dtype, 128, True)
    tq, tk, tv = dev16(q, dtype), dev16(k, dtype), dev16(v, dtype)
    cq, ck = cu_dev(CU_Q), cu_dev(CU_K)
    out, lse = ext.mha_varlen_split_fwd(tq, tk, tv, cq, ck, 520, causal=True, num_splits=4, return_lse=True)
    torch.cuda.synchronize()
    assert sfa.debug_get("last_prefill_splits") == 3
    o2, lse2 = sfa.flash_attn_varlen_split_fwd(tq, tk, tv, cq, ck, 520, causal=True, num_splits=4, return_lse=True)
    torch.cuda.synchronize()
    n = CU_Q[-1]
    assert same((out[:n], lse[:, :n]), (o2[:n], lse2[:, :n]))
    check(out[:n], lse[:, :n], want[:n], lse_want[:, :n], rows[:n], dtype)
    (o3,) = ext.mha_varlen_split_fwd(tq, tk, tv, cq, ck, 32768, causal=True)          # the library's choice
    torch.cuda.synchronize()
    assert sfa.debug_get("last_prefill_splits") == sfa.prefill_varlen_auto_splits(7, 4, tq.shape[0], 32768, 128, causal=True)
    np.testing.assert_allclose(o3[:n].float().cpu().numpy(), want[:n], atol=TOL[dtype], rtol=TOL[dtype])
    with pytest.raises(RuntimeError, match="max_seqlen_k"):
        ext.mha_varlen_split_fwd(tq, tk, tv, cq, ck, 0)
    with pytest.raises(RuntimeError, match="head_dim 256"):
        z = torch.zeros(16, 2, 256, device=DEV, dtype=torch.bfloat16)
        ext.mha_varlen_split_fwd(z, z, z, cu_dev([0, 16]), cu_dev([0, 16]), 16, num_splits=2)
