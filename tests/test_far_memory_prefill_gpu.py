"""Far-address tests of the six prefill forwards: one operand of a call is a view whose offsets do not fit 32 bits
(tests/far_memory.py: the tables, the arena and why running them is safe; tests/test_far_memory_cpu.py: the proof, without
a GPU), and the call must give what the same call gives on compact copies of the same operands -- bit for bit, since only
addresses differ.

Every case asserts
  1. o and lse bit-identical to the compact call's, under the same kernel (last_prefill_kernel; the compact call is
     forced to the kernel the far call reported) and the same split count (last_prefill_splits);
  2. the compact call within TOL / LSE_TOL of the fp64 reference (once per compact call, shared by its cases);
  3. 64 rows of sentinel on either side of every run of memory that O's view covers, intact after the call.
Where the 4-wave kernel is forced onto a view its descriptors do not cover, the refusal is the assertion.

At the end: the seven 8-wave kernels at the largest K / V row pitch their entry points admit (section "pitch limit"),
where one more notch would wrap the 32-bit row offset of the second half of every key tile.

Covered by inspection only: two index terms cannot be pushed past 2^31 at a shape that runs in seconds -- the lse index
(long long in every kernel: ((b * Hq + h) * Sq + row, h * total_q + row) and the index of the fp32 partials in the split
workspaces (size_t on the host, long long on the device).
"""
import functools

import numpy as np
import pytest
import torch

import far_memory as fm
from oracle import round_to, sdpa_ref
from prefill_varlen_ref import prefill_varlen_ref
from prefill_varlen_split_ref import prefill_varlen_split_ref
from prefill_varlen_window_ref import prefill_varlen_window_ref
from prefill_window_ref import prefill_window_ref

pytestmark = pytest.mark.gpu

TOL = {"fp16": 2e-3, "bf16": 1.6e-2}            # tests/test_prefill_gpu.py::TOL
LSE_TOL = 2e-3                                  # tests/test_prefill_gpu.py::LSE_TOL["exact"]
TDT = {"fp16": torch.float16, "bf16": torch.bfloat16}
DTYPES = ("fp16", "bf16")
DEV = torch.device("cuda:0")
IMPLS = {"auto": -1, "rows256": 10, "rows128": 22, "w4": 42, "d256_fallback": 61, "w4d": -1}
WINDOW, SPLITS, MAX_K = 40, 3, 520
PLACEMENTS = fm.prefill_placements()


@pytest.fixture(scope="module")
def sfa():
    assert torch.cuda.is_available(), "GPU tests need a GPU (run with -m gpu on the MI355X box)"
    import starflashattention_amd as m
    m._lib.load()
    return m


@pytest.fixture(scope="module")
def arena(sfa):
    """one arena for the module: the largest any of its placements needs, and room for the last band"""
    a = fm.Arena(max(p.arena_bytes() for p in PLACEMENTS.values()) + 2 ** 20, DEV)
    yield a
    compact.cache_clear()
    a.free()


def dev16(x, dtype):
    return torch.from_numpy(np.array(x, order="C")).to(TDT[dtype]).to(DEV)


def sinks_of(with_sinks):
    return np.linspace(-1.0, 2.0, fm.HQ).astype(np.float32) if with_sinks else None


# ---- the problems and the calls ----------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def rect_problem(Sq, Sk, D, dtype):
    rng = np.random.default_rng(Sq * 7 + Sk * 3 + D)
    q, k, v = (round_to(rng.standard_normal(s), dtype) for s in ((fm.B, fm.HQ, Sq, D), (fm.B, fm.HKV, Sk, D), (fm.B, fm.HKV, Sk, D)))
    return q, k, v


@functools.lru_cache(maxsize=None)
def packed_problem(lens, D, dtype):
    cu_q, cu_k = fm.cu_of([a for a, _ in lens]), fm.cu_of([b for _, b in lens])
    rng = np.random.default_rng(cu_q[-1] + D)
    q, k, v = (round_to(rng.standard_normal(s), dtype) for s in ((cu_q[-1], fm.HQ, D), (cu_k[-1], fm.HKV, D), (cu_k[-1], fm.HKV, D)))
    return q, k, v, tuple(cu_q), tuple(cu_k)


def reference(call, opt, causal, arrays):
    """(o float, lse float) of the fp64 reference of the call"""
    if call in ("fwd", "split"):
        return sdpa_ref(*arrays, causal=causal, return_lse=True)
    if call == "window":
        return prefill_window_ref(*arrays, WINDOW, sinks_of(opt))
    q, k, v, cu_q, cu_k = arrays
    if call == "varlen":
        return prefill_varlen_ref(q, k, v, cu_q, cu_k, causal)[:2]
    if call == "varlen_window":
        return prefill_varlen_window_ref(q, k, v, cu_q, cu_k, WINDOW, sinks_of(opt))[:2]
    return prefill_varlen_split_ref(q, k, v, cu_q, cu_k, causal, MAX_K, SPLITS)[:2]


def launch(sfa, call, opt, causal, t, out, impl=None):
    """the call on device tensors t = (q, k, v[, cu_q, cu_k]) into out: (o, lse, kernel id, split count)"""
    sinks = sinks_of(opt) if call.endswith("window") else None
    sinks = None if sinks is None else torch.from_numpy(sinks).to(DEV)
    get = sfa._lib.debug_get
    sfa.debug_set("prefill_impl", IMPLS[opt] if impl is None and call == "fwd" else -1 if impl is None else impl)
    try:
        if call == "fwd":
            o, lse = sfa.flash_attn_fwd(*t, causal=causal, out=out, return_lse=True)
        elif call == "window":
            o, lse = sfa.flash_attn_window_fwd(*t, WINDOW, sinks=sinks, out=out, return_lse=True)
        elif call == "split":
            o, lse = sfa.flash_attn_split_fwd(*t, causal=causal, num_splits=SPLITS, out=out, return_lse=True)
        elif call == "varlen":
            o, lse = sfa.flash_attn_varlen_fwd(*t, causal=causal, out=out, return_lse=True)
        elif call == "varlen_window":
            o, lse = sfa.flash_attn_varlen_window_fwd(*t, WINDOW, sinks=sinks, out=out, return_lse=True)
        else:
            o, lse = sfa.flash_attn_varlen_split_fwd(*t, MAX_K, causal=causal, num_splits=SPLITS, out=out, return_lse=True)
        torch.cuda.synchronize()
    finally:
        sfa.debug_set("prefill_impl", -1)
    assert o.data_ptr() == out.data_ptr()
    return o, lse, get("last_prefill_kernel") if call == "fwd" else None, get("last_prefill_splits") if "split" in call else None


def padded_out(shape, dtype):
    """a compact O inside an allocation with fm.BAND rows of sentinel on either side: (view, the whole allocation)"""
    D, n = shape[-1], int(np.prod(shape))
    whole = torch.full((n + 2 * fm.BAND * D,), fm.SENTINEL, dtype=torch.int16, device=DEV)
    return whole[fm.BAND * D:fm.BAND * D + n].view(TDT[dtype]).view(shape), whole


def bands_intact(whole, shape):
    D, n = shape[-1], int(np.prod(shape))
    return bool((whole[:fm.BAND * D] == fm.SENTINEL).all() and (whole[fm.BAND * D + n:] == fm.SENTINEL).all())


def device_operands(arrays, dtype):
    t = [dev16(x, dtype) for x in arrays[:3]]
    if len(arrays) == 5:
        t += [torch.tensor(list(c), dtype=torch.int32, device=DEV) for c in arrays[3:]]
    return t


@functools.lru_cache(maxsize=None)
def compact(sfa, call, opt, causal, key, dtype, impl):
    """the call on compact contiguous operands under kernel `impl` (None: as the variant says), checked against the fp64
    reference at the project's tolerances: (o, lse, kernel id, split count), computed once and left unchanged"""
    arrays = rect_problem(*key, dtype) if len(key) == 3 else packed_problem(key[0], key[1], dtype)
    t = device_operands(arrays, dtype)
    out, whole = padded_out(t[0].shape, dtype)
    o, lse, kernel, splits = launch(sfa, call, opt, causal, t, out, impl)
    assert bands_intact(whole, t[0].shape)
    want, lse_want = reference(call, opt, causal, arrays)
    want, lse_want = np.asarray(want, np.float64), np.asarray(lse_want, np.float64)
    np.testing.assert_allclose(o.float().cpu().numpy(), want, atol=TOL[dtype], rtol=TOL[dtype])
    got = lse.cpu().numpy()
    fin = np.isfinite(lse_want)
    np.testing.assert_allclose(got[fin], lse_want[fin], atol=LSE_TOL, rtol=LSE_TOL)
    assert np.all(got[~fin] == -np.inf) and fin.any()
    return o.clone(), lse.clone(), kernel, splits


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


def run_far(sfa, arena, call, opt, causal, key, dtype, placed, refused=False):
    """placed: {operand: (Placement, base)} -- those operands of the call are views into the arena, the others compact"""
    arrays = rect_problem(*key, dtype) if len(key) == 3 else packed_problem(key[0], key[1], dtype)
    t = device_operands(arrays, dtype)
    for op, (p, base) in placed.items():
        if op != "o":
            view = arena.view(p, TDT[dtype], base)
            view.copy_(t["qkv".index(op)])
            t["qkv".index(op)] = view
    if "o" in placed:
        p, base = placed["o"]
        out, idx = arena.view(p, TDT[dtype], base), arena.paint(p, TDT[dtype], base)
        intact = lambda: arena.intact(idx)
    else:
        out, whole = padded_out(t[0].shape, dtype)
        intact = lambda: bands_intact(whole, t[0].shape)
    if refused:
        # (as test_prefill_auto_falls_back_when_a_head_spans_2gib: forcing the 4-wave kernel on this view is refused)
        with pytest.raises(sfa.SfaError):
            launch(sfa, call, opt, causal, t, out)
        return
    o, lse, kernel, splits = launch(sfa, call, opt, causal, t, out)
    assert intact(), "a row outside O's view was written"
    if call == "fwd" and opt in ("rows256", "rows128", "w4", "d256_fallback"):
        assert kernel == IMPLS[opt]
    want_o, want_lse, want_kernel, want_splits = compact(sfa, call, opt, causal, key, dtype, kernel)
    assert (kernel, splits) == (want_kernel, want_splits)
    assert same_bits(o, want_o), "o differs from the compact call's"
    assert torch.equal(lse, want_lse), "lse differs from the compact call's"


# ---- one far term per case ---------------------------------------------------------------------------------------------

RECT_VARIANTS = [("fwd", "auto", (64, 128)), ("fwd", "rows256", (64, 128)), ("fwd", "rows128", (64, 128)),
                 ("fwd", "w4", (128,)), ("fwd", "d256_fallback", (256,)), ("fwd", "w4d", (256,)),
                 ("window", False, (64, 128)), ("window", True, (64, 128)), ("split", None, (64, 128))]
PACKED_VARIANTS = [("varlen", None), ("varlen_window", False), ("varlen_window", True), ("varlen_split", None)]


def rect_cases():
    """every (variant, operand, term); shape, head_dim, dtype and mask alternate so that each variant meets all of them"""
    out = []
    for vi, (call, opt, dims) in enumerate(RECT_VARIANTS):
        i = vi
        for op, terms in fm.RECT_TERMS.items():
            for term in terms:
                (Sq, Sk), D, dtype = fm.SHAPES[i % 2], dims[(i >> 1) % len(dims)], DTYPES[(i + (i >> 2)) % 2]
                causal = True if call == "window" else bool((i >> 1) & 1)
                name = "%s-%s-%dx%d-D%d-%s-%s-%s-%s" % (call, opt, Sq, Sk, D, dtype, "causal" if causal else "full", op, term)
                out.append(pytest.param(call, opt, causal, (Sq, Sk, D), dtype, op, term, id=name))
                i += 1
    return out


@pytest.mark.parametrize("call,opt,causal,key,dtype,op,term", rect_cases())
def test_rectangular_call_with_one_far_term(sfa, arena, call, opt, causal, key, dtype, op, term):
    Sq, Sk, D = key
    p = PLACEMENTS["rect-%dx%d-D%d-%s-%s" % (Sq, Sk, D, op, term)]
    pitch = {x: D for x in "qkv"}
    if op in pitch:
        pitch[op] = p.strides[2]
    refused = opt == "w4" and not fm.w4_serves(D, Sq, Sk, pitch["q"], pitch["k"], pitch["v"])
    run_far(sfa, arena, call, opt, causal, key, dtype, {op: (p, fm.GUARD)}, refused)
    if opt == "w4d":        # the persistent kernel wherever its descriptors cover the view, the 64-bit fallback elsewhere
        assert sfa._lib.debug_get("last_prefill_kernel") == (60 if fm.w4_serves(D, Sq, Sk, pitch["q"], pitch["k"], pitch["v"]) else 61)


def packed_cases():
    out = []
    for vi, (call, opt) in enumerate(PACKED_VARIANTS):
        i = vi
        for op in "qkvo":
            for term in fm.PACKED_TERMS:
                D, dtype = fm.PACKED_DIMS[i % 2], DTYPES[(i >> 1) % 2]
                causal = True if call == "varlen_window" else bool((i >> 2) & 1)
                name = "%s-%s-D%d-%s-%s-%s-%s" % (call, opt, D, dtype, "causal" if causal else "full", op, term)
                out.append(pytest.param(call, opt, causal, D, dtype, op, term, id=name))
                i += 1
    return out


@pytest.mark.parametrize("call,opt,causal,D,dtype,op,term", packed_cases())
def test_packed_call_with_one_far_term(sfa, arena, call, opt, causal, D, dtype, op, term):
    p = PLACEMENTS["packed-D%d-%s-%s" % (D, op, term)]
    run_far(sfa, arena, call, opt, causal, (fm.PACKED_LENS, D), dtype, {op: (p, fm.GUARD)})


# ---- pitch limit: K and V at the largest row pitch the entry points admit ---------------------------------------------------

LIMIT_CASES = [("fwd", "rows256", 64), ("fwd", "rows128", 32), ("window", True, 64), ("split", None, 64)]
LIMIT_PACKED = [("varlen", None), ("varlen_window", True), ("varlen_split", None)]


@pytest.mark.parametrize("D,dtype", [(64, "bf16"), (128, "fp16")])
@pytest.mark.parametrize("call,opt,T", LIMIT_CASES, ids=["prefill_kernel", "prefill_kernel_bm128", "prefill_window_kernel",
                                                          "prefill_split_kernel"])
def test_kv_at_the_pitch_limit(sfa, arena, call, opt, T, D, dtype):
    """One full key tile and a ragged one at pitch_limit(T, D): rows T/2 .. T-1 of the full tile are the ones whose 32-bit
    offset wraps at limit + 8 (tests/test_prefill_pitch_cpu.py), so a limit one notch too high fails here."""
    key = (fm.LIMIT_SQ, fm.LIMIT_SK[T], D)
    pk, pv = PLACEMENTS["limit%d-D%d-k" % (T, D)], PLACEMENTS["limit%d-D%d-v" % (T, D)]
    assert pk.strides[2] == fm.pitch_limit(T, D) == pv.strides[2]
    # V's rows sit in the gaps of K's, right behind them
    run_far(sfa, arena, call, opt, True, key, dtype, {"k": (pk, fm.GUARD), "v": (pv, fm.GUARD + fm.B * fm.HKV * D)})


@pytest.mark.parametrize("D,dtype", [(64, "fp16"), (128, "bf16")])
@pytest.mark.parametrize("call,opt", LIMIT_PACKED, ids=["prefill_varlen_kernel", "prefill_varlen_window_kernel",
                                                        "prefill_varlen_split_kernel"])
def test_packed_kv_at_the_pitch_limit(sfa, arena, call, opt, D, dtype):
    pk, pv = PLACEMENTS["limit64-packed-D%d-k" % D], PLACEMENTS["limit64-packed-D%d-v" % D]
    assert pk.strides[0] == fm.pitch_limit(64, D) == pv.strides[0]
    run_far(sfa, arena, call, opt, True, (fm.LIMIT_PACKED_LENS, D), dtype,
            {"k": (pk, fm.GUARD), "v": (pv, fm.GUARD + fm.HKV * D)})


def test_one_notch_above_the_limit_is_refused_on_real_tensors(sfa, arena):
    """the rejection as a caller meets it: a view one notch above the limit raises, under the call's name"""
    D, dtype = 128, "bf16"
    pk = PLACEMENTS["limit64-D128-k"]
    q, k, v = device_operands(rect_problem(fm.LIMIT_SQ, fm.LIMIT_SK[64], D, dtype), dtype)
    wide = torch.as_strided(arena.typed(TDT[dtype]), k.shape, (pk.strides[0], pk.strides[1], pk.strides[2] + 8, 1), fm.GUARD)
    for fn, name in ((lambda: sfa.flash_attn_window_fwd(q, wide, v, WINDOW), "sfa_prefill_window_fwd"),
                     (lambda: sfa.flash_attn_split_fwd(q, k, wide, num_splits=2), "sfa_prefill_split_fwd")):
        with pytest.raises(sfa.SfaError, match=name + ": [kv] seq stride 34087048 exceeds 34087040 elements"):
            fn()
    sfa.debug_set("prefill_impl", 10)
    try:
        with pytest.raises(sfa.SfaError, match="sfa_prefill_fwd: k seq stride 34087048 exceeds 34087040 elements"):
            sfa.flash_attn_fwd(q, wide, v)
    finally:
        sfa.debug_set("prefill_impl", -1)
