"""CPU-only checks of sfa_prefill_split_fwd: the partition and the fp64 reference of tests/prefill_split_ref.py against
oracle.sdpa_ref, the argument validation of the C ABI (fake pointers: every case returns before a launch), the sizing
function and the auto rule, and the symbols in the header."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from oracle import sdpa_ref
from prefill_split_ref import (key_tiles, prefill_split_ref, qtile_tiles, resolved_splits, split_range, tiles_per_split)
from starflashattention_amd import _lib

HEADER = os.path.join(ROOT, "include", "star_flash_attn.h")
NAME = b"sfa_prefill_split_fwd:"

# (B, Hq, Hkv, Sq, Sk, D, causal): the shapes of tests/test_prefill_split_gpu.py
SHAPES = [
    (1, 1, 1, 1, 1, 128, True),
    (1, 2, 1, 64, 257, 64, False),
    (1, 2, 2, 300, 300, 128, True),
    (2, 4, 2, 100, 1000, 128, True),
    (1, 1, 1, 333, 100, 128, True),
    (1, 8, 1, 513, 513, 64, True),
    (1, 2, 1, 257, 1025, 128, False),
]
IDS = ["x".join(map(str, s[:6])) + ("-causal" if s[6] else "-full") for s in SHAPES]


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_split_ranges_cover_each_visible_tile_once(shape):
    B, Hq, Hkv, Sq, Sk, D, causal = shape
    nkt = key_tiles(Sk)
    for S in range(1, 10):
        C, R = tiles_per_split(Sk, S), resolved_splits(Sk, S)
        assert C == -(-nkt // min(S, nkt)) and R == -(-nkt // C) and 1 <= R <= min(S, nkt)
        assert resolved_splits(Sk, R) == R and tiles_per_split(Sk, R) <= C
        for qt in range(-(-Sq // 256)):
            last = min(256 * (qt + 1), Sq) - 1
            lim = last + Sk - Sq if causal else Sk - 1
            visible = 0 if lim < 0 else lim // 64 + 1          # tiles the q-tile's last row sees
            assert qtile_tiles(qt, Sq, Sk, causal) == visible
            seen = np.zeros(nkt, int)
            for s in range(R):
                t0, t1 = split_range(qt, s, Sq, Sk, causal, S)
                assert t0 == s * C
                assert (t0 >= t1) == (s * C >= visible), (S, qt, s)         # emptiness follows the formula
                if t0 < t1:
                    assert t1 - t0 <= C
                    seen[t0:t1] += 1
            assert np.all(seen[:visible] == 1) and np.all(seen[visible:] == 0), (S, qt, seen)
    assert resolved_splits(5 * 64, 4) == 3 and tiles_per_split(5 * 64, 4) == 2          # the header's example


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
@pytest.mark.parametrize("S", [1, 2, 3, 5, 8])
def test_reference_is_sdpa_ref(shape, S):
    B, Hq, Hkv, Sq, Sk, D, causal = shape
    rng = np.random.default_rng(Sq * 1000 + Sk)
    q, k, v = (rng.standard_normal((B, Hq, Sq, D)), rng.standard_normal((B, Hkv, Sk, D)),
               rng.standard_normal((B, Hkv, Sk, D)))
    o, lse = prefill_split_ref(q, k, v, causal, S)
    want, lse_want = sdpa_ref(q, k, v, causal=causal, return_lse=True)
    fin = np.isfinite(lse_want)
    # (sdpa_ref returns float32: the fp64 results are compared after the same rounding)
    assert np.abs(o.astype(np.float32).astype(np.float64) - want).max() <= 1e-12
    assert np.abs(lse.astype(np.float32)[fin].astype(np.float64) - lse_want[fin]).max(initial=0.0) <= 1e-12
    assert np.all(lse[~fin] == -np.inf) and np.all(o[~fin] == 0)
    if causal and Sq > Sk:
        assert not fin[:, :, :Sq - Sk].any() and fin[:, :, Sq - Sk:].all()


# ---- the C ABI ----

@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def test_symbols_exported_and_in_header(lib):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+sfa_prefill_split_fwd\s*\(\s*const\s+sfa_prefill_args\s*\*\s*args\s*,\s*int\s+num_splits\s*,"
                     r"\s*void\s*\*\s*workspace\s*,\s*size_t\s+workspace_bytes\s*,\s*void\s*\*\s*stream\s*\)\s*;", text)
    assert re.search(r"\bsize_t\s+sfa_prefill_split_workspace_bytes\s*\(\s*int\s+batch\s*,\s*int\s+heads_q\s*,\s*int\s+seqlen_q"
                     r"\s*,\s*int\s+seqlen_k\s*,\s*int\s+head_dim\s*,\s*int\s+causal\s*,\s*int\s+num_splits\s*\)\s*;", text)
    assert re.search(r"\bint\s+sfa_prefill_auto_splits\s*\(\s*int\s+batch\s*,\s*int\s+heads_q\s*,\s*int\s+seqlen_q\s*,"
                     r"\s*int\s+seqlen_k\s*,\s*int\s+head_dim\s*,\s*int\s+causal\s*\)\s*;", text)
    for name in ("sfa_prefill_split_fwd", "sfa_prefill_split_workspace_bytes", "sfa_prefill_auto_splits"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert lib.sfa_abi_version() == 4
    assert "prefill_split_kernel.hip" in __import__("starflashattention_amd.build", fromlist=["x"]).KERNEL_SOURCES


def _well_formed():
    p = _lib.PrefillArgs()
    p.q, p.k, p.v, p.o = 0x1000, 0x2000, 0x3000, 0x4000
    p.batch, p.heads_q, p.heads_kv, p.seqlen_q, p.seqlen_k, p.head_dim = 1, 4, 2, 16, 640, 128
    for st, n in ((p.q_stride, 16), (p.o_stride, 16), (p.k_stride, 640), (p.v_stride, 640)):
        st[0], st[1], st[2] = 4 * n * 128, n * 128, 128
    p.dtype = _lib.DTYPE_BF16
    p.causal = 1
    return p


WS, BIG = 0x100000, 1 << 30      # a fake, 256-byte aligned workspace
# (what, fields, num_splits, workspace, workspace_bytes, status)
MALFORMED = [
    ("q missing", dict(q=None), 2, WS, BIG, -1),
    ("heads not a multiple", dict(heads_q=3), 2, WS, BIG, -2),
    ("misaligned k", dict(k=0x2008), 2, WS, BIG, -2),
    ("head_dim 256", dict(head_dim=256), 2, WS, BIG, -4),
    ("head_dim 96", dict(head_dim=96), 2, WS, BIG, -4),
    ("bad dtype", dict(dtype=7), 2, WS, BIG, -3),
    ("NULL workspace, 2 splits", dict(), 2, None, BIG, -1),
    ("NULL workspace, 10 splits", dict(), 10, None, 0, -1),
    ("unaligned workspace", dict(), 2, WS + 128, BIG, -2),
    ("workspace too small", dict(), 2, WS, 4096, -5),
    ("workspace one byte short", dict(), 4, WS, None, -5),
]


def test_argument_validation(lib):
    lib.sfa_debug_get.restype = ctypes.c_int
    lib.sfa_debug_get.argtypes = [ctypes.c_char_p]
    last = lib.sfa_debug_get(b"last_prefill_kernel")
    splits = lib.sfa_debug_get(b"last_prefill_splits")
    assert lib.sfa_prefill_split_fwd(None, 2, WS, BIG, None) == -1           # NULL args
    assert lib.sfa_last_error().startswith(NAME)
    for what, fields, S, ws, nbytes, want in MALFORMED:
        p = _well_formed()
        for f, val in fields.items():
            setattr(p, f, val)
        if nbytes is None:
            nbytes = lib.sfa_prefill_split_workspace_bytes(p.batch, p.heads_q, p.seqlen_q, p.seqlen_k, p.head_dim, 1, S) - 1
            assert nbytes > 0
        st = lib.sfa_prefill_split_fwd(ctypes.byref(p), S, ws, nbytes, None)
        err = lib.sfa_last_error()
        assert st == want, (what, st, err)
        assert err.startswith(NAME), (what, err)
    p = _well_formed()
    p.q_stride[2] = 132                                                     # bad strides
    assert lib.sfa_prefill_split_fwd(ctypes.byref(p), 2, WS, BIG, None) == -2
    assert lib.sfa_last_error().startswith(NAME)
    # the checks of args come before those of the workspace
    p = _well_formed()
    p.head_dim = 96
    assert lib.sfa_prefill_split_fwd(ctypes.byref(p), 2, None, 0, None) == -4
    # nothing to do: 0, and nothing is launched (the pointers are fake), whatever the workspace
    for field in ("batch", "seqlen_q"):
        p = _well_formed()
        setattr(p, field, 0)
        assert lib.sfa_prefill_split_fwd(ctypes.byref(p), 4, None, 0, None) == 0, field
        assert lib.sfa_prefill_split_fwd(ctypes.byref(p), 0, WS + 1, 5, None) == 0, field
    assert lib.sfa_debug_get(b"last_prefill_kernel") == last
    assert lib.sfa_debug_get(b"last_prefill_splits") == splits                # no call got as far as a launch
    assert lib.sfa_debug_get(b"no_such_knob") == -2 ** 31


DIMS = [(1, 32, 512, 32768, 128), (1, 8, 4096, 4096, 128), (4, 16, 1024, 1024, 64), (1, 2, 300, 300, 128),
        (2, 4, 100, 1000, 64), (1, 1, 1, 1, 128), (1, 4, 16384, 16384, 128), (1, 32, 256, 32768, 128)]


@pytest.mark.parametrize("dims", DIMS, ids=lambda d: "x".join(map(str, d)))
@pytest.mark.parametrize("causal", [0, 1])
def test_workspace_sizing(lib, dims, causal):
    B, Hq, Sq, Sk, D = dims
    size = lambda S: lib.sfa_prefill_split_workspace_bytes(B, Hq, Sq, Sk, D, causal, S)
    prev = 0
    for S in range(1, 40):
        n = size(S)
        R = resolved_splits(Sk, S)
        assert n % 256 == 0 and n >= prev, (S, n, prev)                      # a multiple of 256, non-decreasing
        assert n == size(R), (S, R)                                          # a request and what it resolves to
        if R > 1:       # holds every partial: 256 rows per q-tile and split, head_dim + 2 floats each
            assert n >= B * Hq * -(-Sq // 256) * R * 256 * (D + 2) * 4
        else:
            assert n == 0
        prev = n
    auto = lib.sfa_prefill_auto_splits(B, Hq, Sq, Sk, D, causal)
    assert size(0) == size(-3) == size(auto)
    assert lib.sfa_prefill_split_workspace_bytes(B, Hq, Sq, Sk, 256, causal, 4) == 0       # not served: nothing to size


def test_auto_splits(lib):
    auto = lib.sfa_prefill_auto_splits
    for B, Hq, Sq, Sk, D in DIMS + [(256, 1, 1, 4096, 128), (1, 256, 1, 65536, 64), (8, 32, 256, 32768, 128),
                                    (4, 32, 4096, 4096, 128), (1, 255, 1, 65536, 128), (1, 1, 256, 64 * 1000, 128)]:
        for causal in (0, 1):
            S = auto(B, Hq, Sq, Sk, D, causal)
            assert S >= 1
            assert S <= key_tiles(Sk)
            assert resolved_splits(Sk, S) == S                                # what it returns is a resolved count
            if B * Hq * -(-Sq // 256) >= 256:
                assert S == 1, (B, Hq, Sq, Sk)
    assert auto(1, 32, 512, 32768, 128, 1) > 1          # the shape the call exists for: 64 q-tiles, 512 key tiles
    assert auto(1, 32, 512, 64, 128, 1) == 1            # one key tile: nothing to split


def test_python_layer_exports_the_operator(lib):
    import starflashattention_amd as m
    assert callable(m.flash_attn_split_fwd) and callable(m.prefill_auto_splits) and callable(m.prefill_split_workspace_bytes)
    assert m.prefill_auto_splits(4, 32, 4096, 4096, 128, causal=True) == 1
    assert m.prefill_split_workspace_bytes(1, 2, 300, 300, 128, num_splits=2) == 2 * 2 * 2 * 256 * 130 * 4
    with pytest.raises(RuntimeError, match="float16 or bfloat16"):
        m.flash_attn_split_fwd(torch.zeros(1, 1, 4, 64), torch.zeros(1, 1, 4, 64), torch.zeros(1, 1, 4, 64), num_splits=2)
