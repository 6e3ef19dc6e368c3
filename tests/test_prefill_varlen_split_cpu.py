"""CPU-only checks of sfa_prefill_varlen_split_fwd: the reference of tests/prefill_varlen_split_ref.py against the unsplit
and the rectangular split references, the arithmetic of the item list, the symbols, the sizing function, the auto rule,
the argument validation of the C ABI (fake pointers: every case returns before a launch) and the Python operator's
argument errors that need no device.

The unsplit comparison: tests/prefill_varlen_ref.py returns float32 (oracle.sdpa_ref's fp64 math, rounded once), so the
1e-9 comparison -- reassociation only -- is against the same per-sequence unsplit softmax kept in fp64
(prefill_split_ref with one split, which is one partial over every tile), and prefill_varlen_ref itself is compared after
its own rounding, to one float32 ulp of values of magnitude <= 8 (1e-6)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from prefill_split_ref import key_tiles, prefill_split_ref, qtile_tiles, resolved_splits, tiles_per_split
from prefill_varlen_ref import cu_of, plan_bound, prefill_varlen_ref, valid_sequences
from prefill_varlen_split_ref import (BATCHES, HEADS, partition, plan_slots, prefill_varlen_split_ref, split_ranges,
                                      work_items, workspace_bytes)
from starflashattention_amd import _lib
from test_prefill_varlen_cpu import BIG, STEPS, WS, _set, _well_formed

HEADER = os.path.join(ROOT, "include", "star_flash_attn.h")
NAME = b"sfa_prefill_varlen_split_fwd:"


# ---- the reference ----

def _packed(lens, Hq, Hkv, D, seed, pad=0):
    cu_q, cu_k = cu_of([a for a, _ in lens]), cu_of([b for _, b in lens])
    rng = np.random.default_rng(seed)
    q = rng.standard_normal((cu_q[-1] + pad, Hq, D))
    k = rng.standard_normal((cu_k[-1] + pad, Hkv, D))
    v = rng.standard_normal((cu_k[-1] + pad, Hkv, D))
    return q, k, v, cu_q, cu_k


def _bhsd(x):
    return x.transpose(1, 0, 2)[None]


@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("name", list(BATCHES))
def test_reference_equals_the_unsplit_reference(name, causal):
    lens, max_k, requests = BATCHES[name]
    Hq, Hkv = HEADS[0]
    q, k, v, cu_q, cu_k = _packed(lens, Hq, Hkv, 64, 3, pad=9)
    want32, lse32, rows32 = prefill_varlen_ref(q, k, v, cu_q, cu_k, causal)
    for S in requests:
        o, lse, rows = prefill_varlen_split_ref(q, k, v, cu_q, cu_k, causal, max_k, S)
        assert o.dtype == np.float64 and np.array_equal(rows, rows32)
        assert np.all(o[~rows] == 0) and np.all(lse[:, ~rows] == 0)
        np.testing.assert_allclose(o.astype(np.float32), want32, rtol=0, atol=1e-6)
        fin = np.isfinite(lse32)
        assert np.array_equal(np.isfinite(lse), fin)
        np.testing.assert_allclose(lse[fin], lse32[fin], rtol=0, atol=1e-6)
        for b, (nq, nk) in enumerate(lens):
            q0, k0 = cu_q[b], cu_k[b]
            if nq == 0:
                continue
            if nk == 0:
                assert np.all(o[q0:q0 + nq] == 0) and np.all(lse[:, q0:q0 + nq] == -np.inf)
                continue
            w, lw = prefill_split_ref(_bhsd(q[q0:q0 + nq]), _bhsd(k[k0:k0 + nk]), _bhsd(v[k0:k0 + nk]), causal, 1)
            np.testing.assert_allclose(o[q0:q0 + nq], w[0].transpose(1, 0, 2), rtol=0, atol=1e-9)
            f = np.isfinite(lw[0])
            np.testing.assert_allclose(lse[:, q0:q0 + nq][f], lw[0][f], rtol=0, atol=1e-9)
            assert np.all(lse[:, q0:q0 + nq][~f] == -np.inf)


def same_chunk_request(n_k, C):
    """a request under which sfa_prefill_split_fwd on a sequence of n_k keys cuts chunks of C tiles, or None"""
    for S in range(1, key_tiles(n_k) + 1):
        if tiles_per_split(n_k, S) == C:
            return S
    return None


@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
def test_reference_equals_the_rectangular_split_reference_where_the_chunk_coincides(causal):
    """Per sequence of T inside the hint: where a request exists under which prefill_split_ref cuts the same C, the two
    references walk the same tile ranges and merge in the same order: equal to the last bit."""
    lens, max_k, requests = BATCHES["T"]
    Hq, Hkv = HEADS[0]
    q, k, v, cu_q, cu_k = _packed(lens, Hq, Hkv, 64, 4)
    assert (partition(520, 3), same_chunk_request(300, 3)) == ((3, 3), 2)      # the issue's example
    met = 0
    for S in requests:
        C, Sr = partition(max_k, S)
        o, lse, _ = prefill_varlen_split_ref(q, k, v, cu_q, cu_k, causal, max_k, S)
        for b, (nq, nk) in enumerate(lens):
            if nq == 0 or nk == 0 or nk > max_k:
                continue
            S1 = same_chunk_request(nk, C)
            if S1 is None:
                continue
            met += 1
            q0, k0 = cu_q[b], cu_k[b]
            w, lw = prefill_split_ref(_bhsd(q[q0:q0 + nq]), _bhsd(k[k0:k0 + nk]), _bhsd(v[k0:k0 + nk]), causal, S1)
            np.testing.assert_array_equal(o[q0:q0 + nq], w[0].transpose(1, 0, 2))
            np.testing.assert_array_equal(lse[:, q0:q0 + nq], lw[0])
    assert met >= 12


def test_partition_of_the_batches():
    assert [partition(520, S) for S in (2, 3, 4, 7, 9, 100)] == [(5, 2), (3, 3), (3, 3), (2, 5), (1, 9), (1, 9)]
    assert partition(128, 2) == partition(128, 100) == (1, 2) and partition(64, 7) == (1, 1)
    # the open-ended last split: 1100 keys are 18 tiles; under the hint of 128 split 1 carries tiles [1, 18)
    assert split_ranges(0, 64, 1100, False, 1, 2) == [(0, 0, 1), (1, 1, 18)]
    assert split_ranges(0, 64, 1100, True, 3, 3) == [(0, 0, 3), (1, 3, 6), (2, 6, 18)]
    # (257, 520) causal: q-tile 0 sees keys up to 255 + 263 = 518 -> 9 tiles, q-tile 1 the same; (300, 100) causal: q-tile 0
    # (rows 0..255) ends at key 55 -> 1 tile, so splits 1.. are empty; rows 0..199 see nothing
    assert qtile_tiles(0, 300, 100, True) == 1 and qtile_tiles(1, 300, 100, True) == 2
    assert split_ranges(0, 300, 100, True, 1, 9) == [(0, 0, 1)]
    assert split_ranges(0, 5, 0, True, 1, 9) == [] == split_ranges(0, 5, 0, False, 5, 2)


# ---- the plan arithmetic ----

def test_items_fit_the_list_and_cover_every_real_split_once():
    rng = np.random.default_rng(17)
    for trial in range(2000):
        B = int(rng.integers(1, 10))
        nq = rng.choice([0, 0, 1, 2, 255, 256, 257, 511, 512, 513, int(rng.integers(0, 1500))], size=B)
        nk = rng.choice([0, 0, 1, 63, 64, 65, 127, 128, 129, 1000, int(rng.integers(0, 5000))], size=B)
        cu_q, cu_k = cu_of(nq), cu_of(nk)
        total_q = cu_q[-1] + int(rng.choice([0, 0, 1, 40, 255, 256, 1000]))      # trailing padding
        total_k = cu_k[-1] + int(rng.choice([0, 7, 300]))
        max_k = int(rng.choice([1, 64, 65, 128, 520, 1000, 4096]))              # lengths above the hint included
        causal = bool(rng.integers(0, 2))
        C, S = partition(max_k, int(rng.integers(1, 20)))
        slots = plan_slots(cu_q, cu_k, total_q, total_k)
        bound = plan_bound(B, total_q)
        assert len(slots) <= bound
        its = work_items(cu_q, cu_k, total_q, total_k, causal, C, S)
        assert len(its) <= bound * S, (nq, nk, max_k, S)
        assert len(set(its)) == len(its)
        want = set()
        for slot, (b, qt) in enumerate(slots):
            ranges = split_ranges(qt, int(nq[b]), int(nk[b]), causal, C, S)
            # the non-empty splits are a prefix 0 .. n - 1, and together they cover [0, nkt) once
            assert [s for s, _, _ in ranges] == list(range(len(ranges)))
            tiles = [t for _, t0, t1 in ranges for t in range(t0, t1)]
            assert tiles == list(range(qtile_tiles(qt, int(nq[b]), int(nk[b]), causal)))
            want |= {(slot, s) for s, _, _ in ranges}
        assert set(its) == want


# ---- the C ABI ----

@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def test_symbols_exported_and_in_header(lib):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+sfa_prefill_varlen_split_fwd\s*\(\s*const\s+sfa_prefill_varlen_args\s*\*\s*args\s*,\s*int\s+"
                     r"max_seqlen_k\s*,\s*int\s+num_splits\s*,\s*void\s*\*\s*workspace\s*,\s*size_t\s+workspace_bytes\s*,\s*"
                     r"void\s*\*\s*stream\s*\)\s*;", text)
    assert re.search(r"\bsize_t\s+sfa_prefill_varlen_split_workspace_bytes\s*\(\s*int\s+batch\s*,\s*int\s+heads_q\s*,\s*int\s+"
                     r"total_q\s*,\s*int\s+max_seqlen_k\s*,\s*int\s+head_dim\s*,\s*int\s+num_splits\s*\)\s*;", text)
    assert re.search(r"\bint\s+sfa_prefill_varlen_auto_splits\s*\(\s*int\s+batch\s*,\s*int\s+heads_q\s*,\s*int\s+total_q\s*,\s*"
                     r"int\s+max_seqlen_k\s*,\s*int\s+head_dim\s*,\s*int\s+causal\s*\)\s*;", text)
    for name in ("sfa_prefill_varlen_split_fwd", "sfa_prefill_varlen_split_workspace_bytes", "sfa_prefill_varlen_auto_splits"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert lib.sfa_abi_version() == 4
    assert re.search(r"#define\s+SFA_ABI_VERSION\s+4\b", text)
    assert "prefill_varlen_split_kernel.hip" in __import__("starflashattention_amd.build", fromlist=["x"]).KERNEL_SOURCES
    assert os.path.exists(os.path.join(ROOT, "starflashattention_amd", "csrc", "prefill_varlen_split_kernel.hip"))
    assert ctypes.sizeof(_lib.PrefillVarlenArgs) == 160


def test_workspace_sizing(lib):
    size = lib.sfa_prefill_varlen_split_workspace_bytes
    plan_only = lib.sfa_prefill_varlen_workspace_bytes
    for B, Hq, T in ((1, 1, 1), (7, 4, 967), (7, 8, 967), (4, 32, 2048), (33, 2, 100000)):
        for max_k in (1, 64, 65, 128, 520, 8192, 100000):
            for D in (64, 128):
                prev = 0
                for S in (1, 2, 3, 4, 7, 9, 16, 100, 5000):
                    n = size(B, Hq, T, max_k, D, S)
                    Sr = resolved_splits(max_k, S)
                    assert n == workspace_bytes(B, Hq, T, D, Sr), (B, Hq, T, max_k, D, S)
                    assert n % 256 == 0 and n >= prev
                    assert n == size(B, Hq, T, max_k, D, Sr)                    # a request and the count it resolves to
                    if Sr == 1:
                        assert n == plan_only(B, T) > 0
                    else:
                        assert n > plan_only(B, T)
                    prev = n
                auto = lib.sfa_prefill_varlen_auto_splits(B, Hq, T, max_k, D, 1)
                assert size(B, Hq, T, max_k, D, 0) == size(B, Hq, T, max_k, D, -3) == size(B, Hq, T, max_k, D, auto)
    # batch T of the GPU tests (927 rows and 40 of padding) at 4 heads, head_dim 128, 9 splits: bound 3 + 7 = 10 slots
    assert plan_bound(7, 967) == 10
    assert size(7, 4, 967, 520, 128, 9) == 256 + 768 + 4 * 130 * 256 * 10 * 4 * 9
    for bad in ((0, 4, 100, 520, 128, 2), (-1, 4, 100, 520, 128, 2), (2, 0, 100, 520, 128, 2), (2, 4, 0, 520, 128, 2),
                (2, 4, -5, 520, 128, 2), (2, 4, 100, 0, 128, 2), (2, 4, 100, -1, 128, 2), (2, 4, 100, 520, 256, 2),
                (2, 4, 100, 520, 96, 0)):
        assert size(*bad) == 0, bad
    import starflashattention_amd as m
    assert m.prefill_varlen_split_workspace_bytes(7, 4, 967, 520, 128, num_splits=9) == size(7, 4, 967, 520, 128, 9)
    assert callable(m.flash_attn_varlen_split_fwd)


def test_auto_rule(lib):
    auto, rect = lib.sfa_prefill_varlen_auto_splits, lib.sfa_prefill_auto_splits
    for Hq in (1, 2, 8, 32, 64, 256):
        for T in (1, 256, 257, 2048, 4096, 8192, 65536):
            for max_k in (1, 64, 511, 512, 1024, 8192, 32768, 1 << 20):
                for D in (64, 128):
                    for causal in (0, 1):
                        a = auto(5, Hq, T, max_k, D, causal)
                        assert a == rect(1, Hq, T, max_k, D, causal), (Hq, T, max_k)
                        assert 1 <= a <= min(16, key_tiles(max_k))
                        if Hq * -(-T // 256) >= 256:
                            assert a == 1
    assert auto(8, 8, 4096, 8192, 128, 1) == 2 and auto(8, 32, 4096, 8192, 128, 1) == 1     # the sweep's two head counts
    assert auto(4, 8, 1024, 32768, 128, 1) == 8
    assert auto(0, 8, 1024, 32768, 128, 1) == 1 and auto(4, 8, 1024, 2 ** 31 - 1, 128, 0) == 8
    import starflashattention_amd as m
    assert m.prefill_varlen_auto_splits(4, 8, 1024, 32768, 128, causal=True) == 8


def test_argument_validation_order(lib):
    lib.sfa_debug_get.restype = ctypes.c_int
    lib.sfa_debug_get.argtypes = [ctypes.c_char_p]
    last = lib.sfa_debug_get(b"last_prefill_kernel")
    splits = lib.sfa_debug_get(b"last_prefill_splits")
    fwd = lib.sfa_prefill_varlen_split_fwd
    MAXK, S = 520, 3
    assert fwd(None, MAXK, S, WS, BIG, None) == -1                               # 1. NULL args
    assert lib.sfa_last_error().startswith(NAME)
    # 2-8: every step of the varlen order, under this call's name, never looking at the workspace or at max_seqlen_k
    for what, fields, want in STEPS:
        for ws, nbytes, max_k in ((WS, BIG, MAXK), (None, 0, MAXK), (WS + 1, 0, 0)):
            p = _well_formed()
            _set(p, fields)
            st = fwd(ctypes.byref(p), max_k, S, ws, nbytes, None)
            err = lib.sfa_last_error()
            assert st == want, (what, st, err)
            assert err.startswith(NAME), (what, err)
        for empty in ("batch", "total_q"):
            if empty in fields:
                continue
            p = _well_formed()
            _set(p, fields)
            setattr(p, empty, 0)
            assert fwd(ctypes.byref(p), MAXK, S, WS, BIG, None) == want, (what, empty)
    # 8b. max_seqlen_k < 1: after the alignment step (a misaligned k with the status -2 of its own message comes first, a
    # bad dtype's -3 too), before the empty-problem return and before the workspace
    for max_k in (0, -1, -2 ** 31):
        for ws, nbytes in ((WS, BIG), (None, 0), (WS + 1, 0)):
            for empty in (None, "batch", "total_q"):
                p = _well_formed()
                if empty:
                    setattr(p, empty, 0)
                assert fwd(ctypes.byref(p), max_k, S, ws, nbytes, None) == -2
                assert lib.sfa_last_error().startswith(NAME + b" max_seqlen_k="), lib.sfa_last_error()
    p = _well_formed()
    p.dtype = 7
    assert fwd(ctypes.byref(p), 0, S, WS, BIG, None) == -3
    p = _well_formed()
    p.k = 0x2008
    assert fwd(ctypes.byref(p), 0, S, WS, BIG, None) == -2 and b"16-byte aligned" in lib.sfa_last_error()
    # 9. nothing to do: SFA_OK, the workspace not looked at
    for field in ("batch", "total_q"):
        for ws, nbytes in ((None, 0), (WS + 1, 5), (WS, BIG)):
            p = _well_formed()
            setattr(p, field, 0)
            assert fwd(ctypes.byref(p), MAXK, S, ws, nbytes, None) == 0, field
    # 10. the workspace, against the resolved count: NULL, alignment, size
    p = _well_formed()
    need = lib.sfa_prefill_varlen_split_workspace_bytes(3, 4, 600, MAXK, 128, S)
    plan = lib.sfa_prefill_varlen_workspace_bytes(3, 600)
    assert need == workspace_bytes(3, 4, 600, 128, 3) > plan == 256
    for ws, nbytes, want in ((None, 0, -1), (None, BIG, -1), (WS + 128, 0, -2), (WS + 128, BIG, -2), (WS, 0, -5),
                             (WS, plan, -5), (WS, need - 1, -5)):
        st = fwd(ctypes.byref(p), MAXK, S, ws, nbytes, None)
        assert st == want, (ws, nbytes, st, lib.sfa_last_error())
        assert lib.sfa_last_error().startswith(NAME)
    # an explicit request that resolves to 1 needs the plan alone -- and still needs that
    for max_k, req in ((64, 5), (MAXK, 1)):
        for ws, nbytes, want in ((None, 0, -1), (WS + 128, BIG, -2), (WS, plan - 1, -5)):
            assert fwd(ctypes.byref(p), max_k, req, ws, nbytes, None) == want
    # the library's choice over a NULL workspace: 1 split, and the plan's NULL check
    assert lib.sfa_prefill_varlen_auto_splits(3, 4, 600, 32768, 128, 1) > 1
    assert fwd(ctypes.byref(p), 32768, 0, None, 0, None) == -1
    assert fwd(ctypes.byref(p), 32768, 0, WS, plan - 1, None) == -5             # fewer bytes than one split's plan
    # 11. the grids, after the workspace checks: bound * S' * heads_q attention workgroups, bound * heads_q * head_dim / 4
    # combine workgroups
    p = _well_formed()
    p.batch, p.heads_q, p.heads_kv = 2 ** 20, 32, 8
    big_need = lib.sfa_prefill_varlen_split_workspace_bytes(p.batch, p.heads_q, p.total_q, 8192, 128, 128)
    assert fwd(ctypes.byref(p), 8192, 128, WS, big_need - 1, None) == -5
    assert fwd(ctypes.byref(p), 8192, 128, WS, big_need, None) == -2            # 2^20 * 128 * 32 = 2^32 workgroups
    assert b"grid" in lib.sfa_last_error() and lib.sfa_last_error().startswith(NAME)
    p.batch = 2 ** 22                                                           # the combine grid: 2^22 * 32 * 32 = 2^32
    big_need = lib.sfa_prefill_varlen_split_workspace_bytes(p.batch, p.heads_q, p.total_q, 8192, 128, 2)
    assert fwd(ctypes.byref(p), 8192, 2, WS, big_need, None) == -2 and b"grid" in lib.sfa_last_error()
    assert lib.sfa_debug_get(b"last_prefill_kernel") == last
    assert lib.sfa_debug_get(b"last_prefill_splits") == splits                   # no call got as far as a launch
    # sfa_prefill_varlen_fwd keeps its own name
    p = _well_formed()
    assert lib.sfa_prefill_varlen_fwd(ctypes.byref(p), None, 0, None) == -1
    assert lib.sfa_last_error().startswith(b"sfa_prefill_varlen_fwd: workspace is NULL")
    p.head_dim = 96
    assert lib.sfa_prefill_varlen_fwd(ctypes.byref(p), WS, BIG, None) == -4
    assert lib.sfa_last_error().startswith(b"sfa_prefill_varlen_fwd: head_dim 96")


# ---- the Python operator's argument errors that need no device ----

def test_python_argument_errors(lib):
    import starflashattention_amd as m
    q = torch.zeros(10, 4, 64, dtype=torch.bfloat16)
    kv = torch.zeros(20, 2, 64, dtype=torch.bfloat16)
    cu = torch.tensor([0, 4, 10], dtype=torch.int32)
    cuk = torch.tensor([0, 8, 20], dtype=torch.int32)
    f = m.flash_attn_varlen_split_fwd
    with pytest.raises(RuntimeError, match="max_seqlen_k=12.5 must be an int"):
        f(q, kv, kv, cu, cuk, 12.5)
    with pytest.raises(RuntimeError, match="max_seqlen_k=True must be an int"):
        f(q, kv, kv, cu, cuk, True)
    with pytest.raises(RuntimeError, match="max_seqlen_k=0 must be >= 1"):
        f(q, kv, kv, cu, cuk, 0)
    with pytest.raises(RuntimeError, match="num_splits=2.0 must be an int"):
        f(q, kv, kv, cu, cuk, 12, num_splits=2.0)
    with pytest.raises(RuntimeError, match="float16 or bfloat16"):
        f(q.float(), kv, kv, cu, cuk, 12)
    with pytest.raises(RuntimeError, match="k dtype"):
        f(q, kv.half(), kv, cu, cuk, 12)
    with pytest.raises(RuntimeError, match="cu_seqlens_q has dtype"):
        f(q, kv, kv, cu.long(), cuk, 12)
    with pytest.raises(RuntimeError, match="cu_seqlens_q has 3 entries, cu_seqlens_k 2"):
        f(q, kv, kv, cu, cuk[:2], 12)
    with pytest.raises(RuntimeError, match="out must match q"):
        f(q, kv, kv, cu, cuk, 12, out=torch.zeros(10, 4, 128, dtype=torch.bfloat16))
    with pytest.raises(RuntimeError, match="workspace must be a contiguous 1-d uint8"):
        f(q, kv, kv, cu, cuk, 12, workspace=torch.zeros(256, dtype=torch.float32))
    with pytest.raises(RuntimeError, match="must live on a HIP device"):       # ... and only then the device
        f(q, kv, kv, cu, cuk, 12, num_splits=2)
