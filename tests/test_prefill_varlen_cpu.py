"""CPU-only checks of sfa_prefill_varlen_fwd: the reference of tests/prefill_varlen_ref.py against per-sequence
oracle.sdpa_ref, the plan bound, the symbols, the struct mirror, the sizing function, the argument validation of the C ABI
(fake pointers: every case returns before a launch) and the Python operator's argument errors that need no device."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from oracle import sdpa_ref
from prefill_varlen_ref import ENTRY_BYTES, cu_of, items, plan_bound, prefill_varlen_ref, valid_sequences
from starflashattention_amd import _lib

HEADER = os.path.join(ROOT, "include", "star_flash_attn.h")
NAME = b"sfa_prefill_varlen_fwd:"


# ---- the reference ----

@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
def test_reference_is_per_sequence_sdpa_ref(causal):
    lens = [(300, 300), (0, 0), (1, 1), (100, 333), (37, 5), (5, 0)]
    Hq, Hkv, D, pad = 4, 2, 64, 7
    cu_q, cu_k = cu_of([a for a, _ in lens]), cu_of([b for _, b in lens])
    rng = np.random.default_rng(3)
    q = rng.standard_normal((cu_q[-1] + pad, Hq, D))
    k = rng.standard_normal((cu_k[-1] + pad, Hkv, D))
    v = rng.standard_normal((cu_k[-1] + pad, Hkv, D))
    o, lse, rows = prefill_varlen_ref(q, k, v, cu_q, cu_k, causal)
    assert o.shape == (cu_q[-1] + pad, Hq, D) and lse.shape == (Hq, cu_q[-1] + pad)
    assert rows[:cu_q[-1]].all() and not rows[cu_q[-1]:].any()
    assert np.all(o[~rows] == 0) and np.all(lse[:, ~rows] == 0)
    for b, (nq, nk) in enumerate(lens):
        q0, k0 = cu_q[b], cu_k[b]
        if nq == 0:
            continue
        if nk == 0:
            assert np.all(o[q0:q0 + nq] == 0) and np.all(lse[:, q0:q0 + nq] == -np.inf)
            continue
        want, lse_want = sdpa_ref(q[q0:q0 + nq].transpose(1, 0, 2)[None], k[k0:k0 + nk].transpose(1, 0, 2)[None],
                                  v[k0:k0 + nk].transpose(1, 0, 2)[None], causal=causal, return_lse=True)
        np.testing.assert_array_equal(o[q0:q0 + nq], want[0].transpose(1, 0, 2))
        np.testing.assert_array_equal(lse[:, q0:q0 + nq], lse_want[0])
        if causal and nq > nk:
            assert np.all(lse[:, q0:q0 + nq - nk] == -np.inf) and np.all(o[q0:q0 + nq - nk] == 0)
            assert np.all(np.isfinite(lse[:, q0 + nq - nk:q0 + nq]))


def test_reference_skips_invalid_sequences():
    cu_q, cu_k = [0, 10, 20, 30], [0, 100, 50, 300]
    assert [s[0] for s in valid_sequences(cu_q, cu_k, 30, 300)] == [0, 2]
    assert [s[0] for s in valid_sequences(cu_q, cu_k, 30, 299)] == [0]         # cu_k[3] above total_k
    assert [s[0] for s in valid_sequences([0, -1, 5], [0, 0, 0], 5, 0)] == []   # both neighbours of a negative entry
    rng = np.random.default_rng(5)
    q, k, v = rng.standard_normal((30, 2, 64)), rng.standard_normal((300, 2, 64)), rng.standard_normal((300, 2, 64))
    o, lse, rows = prefill_varlen_ref(q, k, v, cu_q, cu_k, True)
    assert rows[:10].all() and not rows[10:20].any() and rows[20:].all()
    assert np.all(o[10:20] == 0)


def test_items_fit_the_plan_bound():
    rng = np.random.default_rng(7)
    assert items([0, 256]) == 1 and items([0, 257]) == 2 and items([0, 0, 1]) == 1
    assert items(cu_of([300, 0, 1, 257, 64])) == 6 and plan_bound(5, 622) == 7      # batch B of the GPU tests
    assert items(cu_of([300, 100, 64, 1])) == 5 == plan_bound(4, 465)               # batch E
    for trial in range(2000):
        B = int(rng.integers(1, 12))
        lens = rng.choice([0, 0, 1, 2, 255, 256, 257, 511, 512, 513, int(rng.integers(0, 2000))], size=B)
        cu = cu_of(lens)
        total = cu[-1] + int(rng.choice([0, 0, 1, 40, 255, 256, 1000]))     # trailing padding
        n = items(cu, total_q=total, cu_k=[0] * (B + 1), total_k=0)
        assert n == sum(-(-int(x) // 256) for x in lens)
        assert n <= plan_bound(B, cu[-1]) <= plan_bound(B, total), (lens, total)
    # entries that do not ascend: valid sequences may overlap and then claim more items than slots (the plan kernel drops
    # them); input that ascends never does
    assert items([0, 600, 0, 600, 0, 600], total_q=600, cu_k=[0] * 6, total_k=0) == 9 > plan_bound(5, 600) == 7


# ---- the C ABI ----

@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def test_symbols_exported_and_in_header(lib):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+sfa_prefill_varlen_fwd\s*\(\s*const\s+sfa_prefill_varlen_args\s*\*\s*args\s*,\s*void\s*\*\s*"
                     r"workspace\s*,\s*size_t\s+workspace_bytes\s*,\s*void\s*\*\s*stream\s*\)\s*;", text)
    assert re.search(r"\bsize_t\s+sfa_prefill_varlen_workspace_bytes\s*\(\s*int\s+batch\s*,\s*int\s+total_q\s*\)\s*;", text)
    for name in ("sfa_prefill_varlen_fwd", "sfa_prefill_varlen_workspace_bytes"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert lib.sfa_abi_version() == 4
    assert re.search(r"#define\s+SFA_ABI_VERSION\s+4\b", text)
    assert "prefill_varlen_kernel.hip" in __import__("starflashattention_amd.build", fromlist=["x"]).KERNEL_SOURCES
    assert os.path.exists(os.path.join(ROOT, "starflashattention_amd", "csrc", "prefill_varlen_kernel.hip"))


CTYPES_OF = {"const void *": ctypes.c_void_p, "void *": ctypes.c_void_p, "float *": ctypes.c_void_p, "int": ctypes.c_int,
             "float": ctypes.c_float, "int64_t[2]": ctypes.c_int64 * 2}


def test_ctypes_mirror_matches_the_header_struct():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef\s+struct\s+sfa_prefill_varlen_args\s*\{(.*?)\}\s*sfa_prefill_varlen_args\s*;", text, re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = " ".join(decl.split())
        if not decl:
            continue
        m = re.fullmatch(r"(const void \*|void \*|float \*|int64_t |int |float )(\w+)(\[2\])?", decl)
        assert m, decl
        fields.append((m.group(2), CTYPES_OF[m.group(1).strip() + (m.group(3) or "")]))
    assert fields == list(_lib.PrefillVarlenArgs._fields_)
    names = [n for n, _ in fields]
    assert names == ["q", "k", "v", "o", "lse", "cu_seqlens_q", "cu_seqlens_k", "batch", "heads_q", "heads_kv", "total_q",
                     "total_k", "head_dim", "q_stride", "k_stride", "v_stride", "o_stride", "softmax_scale", "causal", "dtype"]
    # 7 pointers, 6 ints, 4 x 2 int64, a float and 2 ints: 56 + 24 + 64 + 12 = 156, rounded up to the 8-byte alignment;
    # no hole before the end: every field starts where the one before it ends
    assert ctypes.sizeof(_lib.PrefillVarlenArgs) == 160
    off = 0
    for n, t in fields:
        assert getattr(_lib.PrefillVarlenArgs, n).offset == off, n
        off += ctypes.sizeof(t)
    assert off == 156
    # sfa_prefill_args is what it was
    assert ctypes.sizeof(_lib.PrefillArgs) == 5 * 8 + 6 * 4 + 12 * 8 + 4 * 4


def test_workspace_sizing(lib):
    size = lib.sfa_prefill_varlen_workspace_bytes
    assert ENTRY_BYTES == 8
    for B in (1, 2, 5, 31, 32, 33, 257, 10000):
        prev = 0
        for T in (1, 255, 256, 257, 622, 8191, 8192, 1 << 20, 2 ** 31 - 1):
            n = size(B, T)
            assert n % 256 == 0 and n >= ENTRY_BYTES * plan_bound(B, T) and n < ENTRY_BYTES * plan_bound(B, T) + 256
            assert n >= prev and n >= size(max(B - 1, 1), T)        # non-decreasing in both arguments
            prev = n
    assert size(5, 622) == 256 and size(2 ** 31 - 1, 2 ** 31 - 1) >= 8 * (2 ** 31 - 1)
    for B, T in ((0, 100), (-1, 100), (4, 0), (4, -7), (0, 0)):
        assert size(B, T) == 0
    import starflashattention_amd as m
    assert m.prefill_varlen_workspace_bytes(5, 622) == 256 and callable(m.flash_attn_varlen_fwd)


def _well_formed():
    p = _lib.PrefillVarlenArgs()
    p.q, p.k, p.v, p.o, p.cu_seqlens_q, p.cu_seqlens_k = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000
    p.batch, p.heads_q, p.heads_kv, p.total_q, p.total_k, p.head_dim = 3, 4, 2, 600, 640, 128
    for st, h in ((p.q_stride, 4), (p.o_stride, 4), (p.k_stride, 2), (p.v_stride, 2)):
        st[0], st[1] = h * 128, 128
    p.dtype = _lib.DTYPE_BF16
    p.causal = 1
    return p


WS, BIG = 0x100000, 1 << 30      # a fake, 256-byte aligned workspace
# steps 2-8 in the order of the checks: (what, fields, status).  Every case runs over a good, a NULL and a misaligned empty
# workspace, and with batch or total_q of 0: a check out of its place shows as a wrong status
STEPS = [
    ("q missing", dict(q=None), -1),
    ("k missing", dict(k=None), -1),
    ("v missing", dict(v=None), -1),
    ("o missing", dict(o=None), -1),
    ("cu_seqlens_q missing", dict(cu_seqlens_q=None), -1),
    ("cu_seqlens_k missing", dict(cu_seqlens_k=None), -1),
    ("negative batch", dict(batch=-1), -2),
    ("no query heads", dict(heads_q=0), -2),
    ("no kv heads", dict(heads_kv=0), -2),
    ("negative total_q", dict(total_q=-1), -2),
    ("negative total_k", dict(total_k=-1), -2),
    ("heads not a multiple", dict(heads_q=3), -2),
    ("head_dim 256", dict(head_dim=256), -4),
    ("head_dim 96", dict(head_dim=96), -4),
    ("bad dtype", dict(dtype=7), -3),
    ("negative stride", dict(k_stride=(-256, 128)), -2),
    ("stride not a multiple of 8", dict(o_stride=(516, 128)), -2),
    ("head stride not a multiple of 8", dict(q_stride=(512, 12)), -2),
    ("misaligned k", dict(k=0x2008), -2),
    ("misaligned cu_seqlens_q", dict(cu_seqlens_q=0x5002), -2),
    ("misaligned cu_seqlens_k", dict(cu_seqlens_k=0x6001), -2),
    ("misaligned lse", dict(lse=0x7002), -2),
]


def _set(p, fields):
    for f, val in fields.items():
        if isinstance(val, tuple):
            getattr(p, f)[0], getattr(p, f)[1] = val
        else:
            setattr(p, f, val)


def test_argument_validation_order(lib):
    lib.sfa_debug_get.restype = ctypes.c_int
    lib.sfa_debug_get.argtypes = [ctypes.c_char_p]
    last = lib.sfa_debug_get(b"last_prefill_kernel")
    splits = lib.sfa_debug_get(b"last_prefill_splits")
    fwd = lib.sfa_prefill_varlen_fwd
    assert fwd(None, WS, BIG, None) == -1                                    # 1. NULL args
    assert lib.sfa_last_error().startswith(NAME)
    assert fwd(None, None, 0, None) == -1
    for what, fields, want in STEPS:
        for ws, nbytes in ((WS, BIG), (None, 0), (WS + 1, 0)):              # steps 2-8 never look at the workspace
            p = _well_formed()
            _set(p, fields)
            st = fwd(ctypes.byref(p), ws, nbytes, None)
            err = lib.sfa_last_error()
            assert st == want, (what, st, err)
            assert err.startswith(NAME), (what, err)
        # ... and come before the empty-problem return
        for empty in ("batch", "total_q"):
            if empty in fields:
                continue
            p = _well_formed()
            _set(p, fields)
            setattr(p, empty, 0)
            assert fwd(ctypes.byref(p), WS, BIG, None) == want, (what, empty)
    # the order among steps 2-8: a case of step i together with one of every later step returns step i's status
    order =[("q missing", -1), ("negative batch", -2), ("heads not a multiple", -2), ("head_dim 96", -4), ("bad dtype", -3),
             ("negative stride", -2), ("misaligned k", -2)]
    by_name = {w: f for w, f, _ in STEPS}
    for i, (early, want) in enumerate(order):
        for late, late_status in order[i + 1:]:
            if want == late_status:
                continue                                                     # (the statuses would not tell them apart)
            p = _well_formed()
            _set(p, by_name[late])
            _set(p, by_name[early])
            assert fwd(ctypes.byref(p), None, 0, None) == want, (early, late)
    p = _well_formed()
    p.head_dim = 256
    assert fwd(ctypes.byref(p), WS, BIG, None) == -4
    msg = lib.sfa_last_error()
    assert b"sfa_prefill_fwd" in msg and msg.startswith(NAME)               # names the call that serves head_dim 256
    # 9. nothing to do: SFA_OK, nothing launched (the pointers are fake), the workspace not looked at
    for field in ("batch", "total_q"):
        for ws, nbytes in ((None, 0), (WS + 1, 5), (WS, BIG)):
            p = _well_formed()
            setattr(p, field, 0)
            assert fwd(ctypes.byref(p), ws, nbytes, None) == 0, field
    # 10. the workspace, in its order: NULL, alignment, size
    need = lib.sfa_prefill_varlen_workspace_bytes(3, 600)
    assert need == 256
    p = _well_formed()
    for ws, nbytes, want in ((None, 0, -1), (None, BIG, -1), (WS + 128, 0, -2), (WS + 128, BIG, -2), (WS, 0, -5),
                             (WS, need - 1, -5)):
        st = fwd(ctypes.byref(p), ws, nbytes, None)
        assert st == want, (ws, nbytes, st, lib.sfa_last_error())
        assert lib.sfa_last_error().startswith(NAME)
    # 11. the grid: (total_q / 256 + batch) * heads_q workgroups must fit 2^31 - 1 -- after the workspace checks
    p = _well_formed()
    p.batch, p.heads_q, p.heads_kv = 2 ** 27, 32, 8
    big_need = lib.sfa_prefill_varlen_workspace_bytes(p.batch, p.total_q)
    assert fwd(ctypes.byref(p), WS, big_need - 1, None) == -5
    assert fwd(ctypes.byref(p), WS, big_need, None) == -2
    assert b"grid" in lib.sfa_last_error()
    assert lib.sfa_debug_get(b"last_prefill_kernel") == last
    assert lib.sfa_debug_get(b"last_prefill_splits") == splits                # no call got as far as a launch


# ---- the Python operator's argument errors that need no device ----

def test_python_argument_errors(lib):
    import starflashattention_amd as m
    q = torch.zeros(10, 4, 64, dtype=torch.bfloat16)
    kv = torch.zeros(20, 2, 64, dtype=torch.bfloat16)
    cu = torch.tensor([0, 4, 10], dtype=torch.int32)
    cuk = torch.tensor([0, 8, 20], dtype=torch.int32)
    with pytest.raises(RuntimeError, match="float16 or bfloat16"):
        m.flash_attn_varlen_fwd(q.float(), kv, kv, cu, cuk)
    with pytest.raises(RuntimeError, match="k dtype"):
        m.flash_attn_varlen_fwd(q, kv.half(), kv, cu, cuk)
    with pytest.raises(RuntimeError, match=r"q must be \[tokens, heads, head_dim\]"):
        m.flash_attn_varlen_fwd(q[None], kv, kv, cu, cuk)
    with pytest.raises(RuntimeError, match="head_dim must be contiguous"):
        m.flash_attn_varlen_fwd(q, kv[:, :, ::2], kv, cu, cuk)
    with pytest.raises(RuntimeError, match="do not match"):
        m.flash_attn_varlen_fwd(q, kv, kv[:19], cu, cuk)
    with pytest.raises(RuntimeError, match="do not match"):
        m.flash_attn_varlen_fwd(q, torch.zeros(20, 2, 128, dtype=torch.bfloat16), torch.zeros(20, 2, 128, dtype=torch.bfloat16), cu, cuk)
    with pytest.raises(RuntimeError, match="cu_seqlens_q has dtype"):
        m.flash_attn_varlen_fwd(q, kv, kv, cu.long(), cuk)
    with pytest.raises(RuntimeError, match="cu_seqlens_k has dtype"):
        m.flash_attn_varlen_fwd(q, kv, kv, cu, cuk.float())
    with pytest.raises(RuntimeError, match="cu_seqlens_q must be a tensor"):
        m.flash_attn_varlen_fwd(q, kv, kv, [0, 4, 10], cuk)
    with pytest.raises(RuntimeError, match="cu_seqlens_k is on meta"):
        m.flash_attn_varlen_fwd(q, kv, kv, cu, cuk.to("meta"))
    with pytest.raises(RuntimeError, match=r"cu_seqlens_q must be a contiguous \[batch \+ 1\]"):
        m.flash_attn_varlen_fwd(q, kv, kv, cu[None], cuk)
    with pytest.raises(RuntimeError, match=r"cu_seqlens_k must be a contiguous \[batch \+ 1\]"):
        m.flash_attn_varlen_fwd(q, kv, kv, cu, cuk[:0])
    with pytest.raises(RuntimeError, match="cu_seqlens_q has 3 entries, cu_seqlens_k 2"):
        m.flash_attn_varlen_fwd(q, kv, kv, cu, cuk[:2])
    with pytest.raises(RuntimeError, match="out must match q"):
        m.flash_attn_varlen_fwd(q, kv, kv, cu, cuk, out=torch.zeros(10, 4, 128, dtype=torch.bfloat16))
    with pytest.raises(RuntimeError, match="workspace must be a contiguous 1-d uint8"):
        m.flash_attn_varlen_fwd(q, kv, kv, cu, cuk, workspace=torch.zeros(256, dtype=torch.float32))
    with pytest.raises(RuntimeError, match="must live on a HIP device"):       # ... and only then the device
        m.flash_attn_varlen_fwd(q, kv, kv, cu, cuk)
