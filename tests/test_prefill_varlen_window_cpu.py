"""CPU-only checks of sfa_prefill_varlen_window_fwd: the reference of tests/prefill_varlen_window_ref.py against
prefill_varlen_ref and per-sequence prefill_window_ref, the weight of the tests' sinks, the symbols, the argument
validation of the C ABI (fake pointers: every case returns before a launch) and the Python operator's argument errors that
need no device."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from prefill_varlen_ref import cu_of, prefill_varlen_ref
from prefill_varlen_window_ref import (BATCHES, INT_MAX, SHARE_HI, SHARE_LO, SHARE_ROWS, WINDOWS, batch_cu, inputs, lo0,
                                       prefill_varlen_window_ref, reference, sink_share)
from prefill_window_ref import prefill_window_ref
from starflashattention_amd import _lib
from test_prefill_varlen_cpu import BIG, STEPS, WS, _set, _well_formed

HEADER = os.path.join(ROOT, "include", "star_flash_attn.h")
NAME = b"sfa_prefill_varlen_window_fwd:"
SYMBOL = "sfa_prefill_varlen_window_fwd"


# ---- the reference ----

def _random_batch(lens, Hq, Hkv, D, pad, seed):
    cu_q, cu_k = cu_of([a for a, _ in lens]), cu_of([b for _, b in lens])
    rng = np.random.default_rng(seed)
    q = rng.standard_normal((cu_q[-1] + pad, Hq, D))
    k = rng.standard_normal((cu_k[-1] + pad, Hkv, D))
    v = rng.standard_normal((cu_k[-1] + pad, Hkv, D))
    return q, k, v, cu_q, cu_k


LENS = [(300, 300), (0, 0), (1, 1), (100, 333), (37, 5), (5, 0)]


@pytest.mark.parametrize("window", [333, 334, INT_MAX])
def test_reference_is_the_causal_varlen_reference_under_a_long_window(window):
    """window >= max n_k without sinks: exactly prefill_varlen_ref(causal=True)"""
    q, k, v, cu_q, cu_k = _random_batch(LENS, 4, 2, 64, 7, 3)
    assert window >= max(b for _, b in LENS)
    o, lse, rows = prefill_varlen_window_ref(q, k, v, cu_q, cu_k, window)
    want, lse_want, rows_want = prefill_varlen_ref(q, k, v, cu_q, cu_k, True)
    np.testing.assert_array_equal(o, want)
    np.testing.assert_array_equal(lse, lse_want)
    np.testing.assert_array_equal(rows, rows_want)


@pytest.mark.parametrize("with_sinks", [False, True], ids=["nosink", "sinks"])
@pytest.mark.parametrize("window", [1, 40, 65, 400])
def test_reference_is_per_sequence_window_ref(window, with_sinks):
    Hq, Hkv, D, pad = 4, 2, 64, 7
    q, k, v, cu_q, cu_k = _random_batch(LENS, Hq, Hkv, D, pad, 4)
    sinks = np.linspace(-1.0, 2.0, Hq) if with_sinks else None
    o, lse, rows = prefill_varlen_window_ref(q, k, v, cu_q, cu_k, window, sinks=sinks)
    assert o.shape == (cu_q[-1] + pad, Hq, D) and lse.shape == (Hq, cu_q[-1] + pad)
    assert rows[:cu_q[-1]].all() and not rows[cu_q[-1]:].any()
    assert np.all(o[~rows] == 0) and np.all(lse[:, ~rows] == 0)
    for b, (nq, nk) in enumerate(LENS):
        q0, k0 = cu_q[b], cu_k[b]
        if nq == 0:
            continue
        if nk == 0:
            assert np.all(o[q0:q0 + nq] == 0) and np.all(lse[:, q0:q0 + nq] == -np.inf)
            continue
        want, lse_want = prefill_window_ref(q[q0:q0 + nq].transpose(1, 0, 2)[None], k[k0:k0 + nk].transpose(1, 0, 2)[None],
                                            v[k0:k0 + nk].transpose(1, 0, 2)[None], window, sinks=sinks)
        np.testing.assert_array_equal(o[q0:q0 + nq], want[0].transpose(1, 0, 2))
        np.testing.assert_array_equal(lse[:, q0:q0 + nq], lse_want[0])
        if nq > nk:         # rows above the causal limit have no key, sink or not
            assert np.all(lse[:, q0:q0 + nq - nk] == -np.inf) and np.all(o[q0:q0 + nq - nk] == 0)
            assert np.all(np.isfinite(lse[:, q0 + nq - nk:q0 + nq]))


def test_reference_skips_invalid_sequences():
    cu_q, cu_k = [0, 10, 20, 30], [0, 100, 50, 300]
    rng = np.random.default_rng(5)
    q, k, v = rng.standard_normal((30, 2, 64)), rng.standard_normal((300, 2, 64)), rng.standard_normal((300, 2, 64))
    o, lse, rows = prefill_varlen_window_ref(q, k, v, cu_q, cu_k, 40, sinks=np.zeros(2))
    assert rows[:10].all() and not rows[10:20].any() and rows[20:].all()
    assert np.all(o[10:20] == 0) and np.all(lse[:, 10:20] == 0)


def test_lo0_and_what_the_batches_reach():
    assert lo0(100, 1000, 128) == 773 == 12 * 64 + 5            # Q: 12 whole tiles and 5 rows never read
    assert lo0(64, 769, 1) == 705 and lo0(64, 769, 65) == 641 == 10 * 64 + 1        # R
    assert lo0(64, 65, 1) == 1 and lo0(64, 65, 2) == 0 and lo0(333, 100, 1) == 0    # S; n_q > n_k
    assert lo0(300, 300, INT_MAX) == 0
    assert [b % 64 for _, b in BATCHES["S"][0]] == [1, 63, 1, 0]
    assert sum(-(-a // 256) for a, _ in BATCHES["P"][0]) == 6 and sum(a for a, _ in BATCHES["P"][0]) // 256 + 5 == 7
    assert BATCHES["R"][1] % 8 == 0 and all(BATCHES[n][1] % 8 for n in "PQS")       # the slices = 8 block map: R alone


@pytest.mark.parametrize("name", sorted(BATCHES))
def test_the_sinks_are_material(name):
    """The tests' sinks -- a_h + delta_h, a_h the no-sink lse of the row of median lse among the batch's rows with a key --
    take between 0.05 and 0.95 of the softmax in at least 0.2 of the rows with a key, for every head and window used."""
    for window in WINDOWS + (INT_MAX,):
        _, lse, rows, _ = reference(name, "bf16", 64, window, False)
        _, _, _, sinks = reference(name, "bf16", 64, window, True)
        share = sink_share(lse, sinks)
        for h in range(lse.shape[0]):
            has = np.isfinite(lse[h]) & rows
            frac = np.mean((share[h][has] >= SHARE_LO) & (share[h][has] <= SHARE_HI))
            assert frac >= SHARE_ROWS, (name, window, h, frac)


# ---- the C ABI ----

@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def test_symbol_exported_and_in_header(lib):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+sfa_prefill_varlen_window_fwd\s*\(\s*const\s+sfa_prefill_varlen_args\s*\*\s*args\s*,\s*int\s+"
                     r"window\s*,\s*const\s+float\s*\*\s*sinks\s*,\s*void\s*\*\s*workspace\s*,\s*size_t\s+workspace_bytes\s*,"
                     r"\s*void\s*\*\s*stream\s*\)\s*;", text)
    assert SYMBOL in _lib.EXPORTED_SYMBOLS and hasattr(lib, SYMBOL)
    assert lib.sfa_abi_version() == 4
    build = __import__("starflashattention_amd.build", fromlist=["x"])
    assert "prefill_varlen_window_kernel.hip" in build.KERNEL_SOURCES
    assert os.path.exists(os.path.join(ROOT, "starflashattention_amd", "csrc", "prefill_varlen_window_kernel.hip"))
    # the workspace is sfa_prefill_varlen_workspace_bytes': no sizing function of its own
    assert not re.search(r"\bsfa_prefill_varlen_window\w*workspace_bytes\b", text)
    assert not any("prefill_varlen_window" in s and "workspace" in s for s in _lib.EXPORTED_SYMBOLS)
    assert not hasattr(lib, "sfa_prefill_varlen_window_workspace_bytes")
    assert not hasattr(lib, "sfa_prefill_varlen_window_fwd_workspace_bytes")
    import starflashattention_amd as m
    assert callable(m.flash_attn_varlen_window_fwd)


def _call(lib, p, window, sinks, ws, nbytes):
    return lib.sfa_prefill_varlen_window_fwd(ctypes.byref(p) if p is not None else None, window, sinks, ws, nbytes, None)


# the window call's own checks, directly after the alignment step: (what, fields of args, window, sinks)
OWN = [
    ("causal = 0", dict(causal=0), 128, None),
    ("window = 0", {}, 0, None),
    ("window = -1", {}, -1, None),
    ("misaligned sinks", {}, 128, 0x8002),
]


def test_argument_validation_order(lib):
    lib.sfa_debug_get.restype = ctypes.c_int
    lib.sfa_debug_get.argtypes = [ctypes.c_char_p]
    last = lib.sfa_debug_get(b"last_prefill_kernel")
    splits = lib.sfa_debug_get(b"last_prefill_splits")
    assert _call(lib, None, 128, None, WS, BIG) == -1                                 # NULL args
    assert lib.sfa_last_error().startswith(NAME)
    assert _call(lib, None, 0, 0x8002, None, 0) == -1
    # every step of the varlen order returns its status under the new name, whatever the workspace and the sinks; and
    # before the window call's own checks
    for what, fields, want in STEPS:
        for ws, nbytes in ((WS, BIG), (None, 0), (WS + 1, 0)):
            for sinks in (None, 0x8000):
                p = _well_formed()
                _set(p, fields)
                st = _call(lib, p, 128, sinks, ws, nbytes)
                err = lib.sfa_last_error()
                assert st == want, (what, st, err)
                assert err.startswith(NAME), (what, err)
        for empty in ("batch", "total_q"):
            if empty in fields:
                continue
            p = _well_formed()
            _set(p, fields)
            setattr(p, empty, 0)
            assert _call(lib, p, 128, None, WS, BIG) == want, (what, empty)
        if want != -2:      # a stride or alignment defect (-2 like the own checks) is told apart by its message below
            for _, own_fields, window, sinks in OWN:
                p = _well_formed()
                _set(p, own_fields)
                _set(p, fields)
                assert _call(lib, p, window, sinks, WS, BIG) == want, (what, own_fields, window, sinks)
    p = _well_formed()
    p.head_dim = 256
    assert _call(lib, p, 128, None, WS, BIG) == -4
    msg = lib.sfa_last_error()
    assert b"sfa_prefill_fwd" in msg and msg.startswith(NAME)
    # the four own checks: -2 each, with batch = 0 and with total_q = 0, before any workspace defect
    texts = {"causal = 0": b"causal", "window = 0": b"window=0", "window = -1": b"window=-1", "misaligned sinks": b"sinks"}
    for what, own_fields, window, sinks in OWN:
        for empty in (None, "batch", "total_q"):
            for ws, nbytes in ((WS, BIG), (None, 0), (None, BIG), (WS + 128, BIG), (WS, 0), (WS, 255)):
                p = _well_formed()
                _set(p, own_fields)
                if empty:
                    setattr(p, empty, 0)
                st = _call(lib, p, window, sinks, ws, nbytes)
                err = lib.sfa_last_error()
                assert st == -2, (what, empty, ws, nbytes, st, err)
                assert err.startswith(NAME) and texts[what] in err, (what, err)
        # ... and after a stride or an alignment defect, whose message is the one reported
        for late, text in (("negative stride", b"strides"), ("stride not a multiple of 8", b"strides"),
                           ("misaligned k", b"16-byte"), ("misaligned lse", b"4-byte aligned")):
            p = _well_formed()
            _set(p, own_fields)
            _set(p, {w: f for w, f, _ in STEPS}[late])
            assert _call(lib, p, window, sinks, WS, BIG) == -2
            err = lib.sfa_last_error()
            assert text in err and texts[what] not in err, (what, late, err)
    # the order among the own checks: sinks, causal, window
    p = _well_formed()
    p.causal = 0
    assert _call(lib, p, 0, 0x8002, WS, BIG) == -2 and b"sinks must be" in lib.sfa_last_error()
    assert _call(lib, p, 0, None, WS, BIG) == -2 and b"causal" in lib.sfa_last_error()
    # nothing to do: SFA_OK, nothing launched (the pointers are fake), the workspace not looked at
    for field in ("batch", "total_q"):
        for ws, nbytes in ((None, 0), (WS + 1, 5), (WS, BIG)):
            for window, sinks in ((1, None), (128, 0x8000), (INT_MAX, None)):
                p = _well_formed()
                setattr(p, field, 0)
                assert _call(lib, p, window, sinks, ws, nbytes) == 0, field
    # the workspace, in its order: NULL, alignment, size; then the grid
    need = lib.sfa_prefill_varlen_workspace_bytes(3, 600)
    assert need == 256
    p = _well_formed()
    for ws, nbytes, want in ((None, 0, -1), (None, BIG, -1), (WS + 128, 0, -2), (WS + 128, BIG, -2), (WS, 0, -5),
                             (WS, need - 1, -5)):
        for window, sinks in ((128, None), (INT_MAX, None), (128, 0x8000)):
            st = _call(lib, p, window, sinks, ws, nbytes)
            assert st == want, (ws, nbytes, st, lib.sfa_last_error())
            assert lib.sfa_last_error().startswith(NAME)
    p = _well_formed()
    p.batch, p.heads_q, p.heads_kv = 2 ** 27, 32, 8
    big_need = lib.sfa_prefill_varlen_workspace_bytes(p.batch, p.total_q)
    assert _call(lib, p, 128, None, WS, big_need - 1) == -5
    assert _call(lib, p, 128, None, WS, big_need) == -2
    assert b"grid" in lib.sfa_last_error() and lib.sfa_last_error().startswith(NAME)
    assert lib.sfa_debug_get(b"last_prefill_kernel") == last
    assert lib.sfa_debug_get(b"last_prefill_splits") == splits                # no call got as far as a launch


def test_the_varlen_call_keeps_its_name(lib):
    """sfa_prefill_varlen_fwd shares the validator: its statuses and messages are what they were"""
    old = b"sfa_prefill_varlen_fwd:"
    fwd = lib.sfa_prefill_varlen_fwd
    assert fwd(None, WS, BIG, None) == -1 and lib.sfa_last_error() == b"sfa_prefill_varlen_fwd: args is NULL"
    for what, fields, want in STEPS:
        p = _well_formed()
        _set(p, fields)
        assert fwd(ctypes.byref(p), WS, BIG, None) == want, what
        assert lib.sfa_last_error().startswith(old), what
    p = _well_formed()
    p.causal = 0                                                # ... and causal = 0 is its full attention, not an error
    assert fwd(ctypes.byref(p), None, 0, None) == -1
    assert lib.sfa_last_error() == b"sfa_prefill_varlen_fwd: workspace is NULL"
    assert fwd(ctypes.byref(p), WS, 255, None) == -5
    assert lib.sfa_last_error() == b"sfa_prefill_varlen_fwd: workspace has 255 bytes, need 256"
    p.head_dim = 256
    assert fwd(ctypes.byref(p), WS, BIG, None) == -4
    assert lib.sfa_last_error() == b"sfa_prefill_varlen_fwd: head_dim 256 not in {64, 128} (sfa_prefill_fwd serves head_dim 256)"


# ---- the Python operator's argument errors that need no device ----

def test_python_argument_errors(lib):
    import starflashattention_amd as m
    f = m.flash_attn_varlen_window_fwd
    q = torch.zeros(10, 4, 64, dtype=torch.bfloat16)
    kv = torch.zeros(20, 2, 64, dtype=torch.bfloat16)
    cu = torch.tensor([0, 4, 10], dtype=torch.int32)
    cuk = torch.tensor([0, 8, 20], dtype=torch.int32)
    with pytest.raises(RuntimeError, match="float16 or bfloat16"):
        f(q.float(), kv, kv, cu, cuk, 128)
    with pytest.raises(RuntimeError, match="k dtype"):
        f(q, kv.half(), kv, cu, cuk, 128)
    with pytest.raises(RuntimeError, match=r"q must be \[tokens, heads, head_dim\]"):
        f(q[None], kv, kv, cu, cuk, 128)
    with pytest.raises(RuntimeError, match="head_dim must be contiguous"):
        f(q, kv[:, :, ::2], kv, cu, cuk, 128)
    with pytest.raises(RuntimeError, match="do not match"):
        f(q, kv, kv[:19], cu, cuk, 128)
    with pytest.raises(RuntimeError, match="cu_seqlens_q has dtype"):
        f(q, kv, kv, cu.long(), cuk, 128)
    with pytest.raises(RuntimeError, match="cu_seqlens_k is on meta"):
        f(q, kv, kv, cu, cuk.to("meta"), 128)
    with pytest.raises(RuntimeError, match="cu_seqlens_q has 3 entries, cu_seqlens_k 2"):
        f(q, kv, kv, cu, cuk[:2], 128)
    with pytest.raises(RuntimeError, match="out must match q"):
        f(q, kv, kv, cu, cuk, 128, out=torch.zeros(10, 4, 128, dtype=torch.bfloat16))
    with pytest.raises(RuntimeError, match="workspace must be a contiguous 1-d uint8"):
        f(q, kv, kv, cu, cuk, 128, workspace=torch.zeros(256, dtype=torch.float32))
    with pytest.raises(RuntimeError, match="window=0 must be >= 1"):
        f(q, kv, kv, cu, cuk, 0)
    with pytest.raises(RuntimeError, match="window=-5 must be >= 1"):
        f(q, kv, kv, cu, cuk, -5)
    with pytest.raises(RuntimeError, match="does not fit an int"):
        f(q, kv, kv, cu, cuk, 2 ** 31)
    with pytest.raises(RuntimeError, match="must live on a HIP device"):       # ... and only then the device
        f(q, kv, kv, cu, cuk, 128)
    with pytest.raises(RuntimeError, match="must live on a HIP device"):
        f(q, kv, kv, cu, cuk, INT_MAX, sinks=torch.zeros(4))
    with pytest.raises(TypeError):                                              # window is required
        f(q, kv, kv, cu, cuk)
