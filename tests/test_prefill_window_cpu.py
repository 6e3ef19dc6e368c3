"""CPU-only checks of sfa_prefill_window_fwd: the fp64 reference of tests/prefill_window_ref.py against oracle.sdpa_ref
and against closed forms, the argument validation of the C ABI (fake pointers, no launch), and the symbol in the header."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from oracle import sdpa_ref
from prefill_window_ref import prefill_window_ref, visible_counts
from sinks_ref import sigmoid
from starflashattention_amd import _lib

HEADER = os.path.join(ROOT, "include", "star_flash_attn.h")
NAME = b"sfa_prefill_window_fwd:"


def _problem(B, Hq, Hkv, Sq, Sk, D, seed=0):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((B, Hq, Sq, D)), rng.standard_normal((B, Hkv, Sk, D)),
            rng.standard_normal((B, Hkv, Sk, D)))


@pytest.mark.parametrize("Sq,Sk", [(5, 12), (9, 9), (12, 5)])
@pytest.mark.parametrize("extra", [0, 1, 2 ** 31 - 1])
def test_reference_is_sdpa_ref_without_window_and_sink(Sq, Sk, extra):
    q, k, v = _problem(2, 4, 2, Sq, Sk, 16, seed=Sq * 100 + Sk)
    window = Sk + extra if extra < 2 ** 30 else extra
    o, lse = prefill_window_ref(q, k, v, window)
    want, lse_want = sdpa_ref(q, k, v, causal=True, return_lse=True)
    assert np.array_equal(o, want)
    assert np.array_equal(lse, lse_want)            # (-inf == -inf where Sq > Sk leaves rows without a key)
    if Sq > Sk:
        assert np.all(lse[:, :, :Sq - Sk] == -np.inf) and np.all(o[:, :, :Sq - Sk] == 0)


def test_window_one_returns_the_v_rows():
    B, Hq, Hkv, Sq, Sk, D = 1, 4, 2, 6, 9, 8
    q, k, v = _problem(B, Hq, Hkv, Sq, Sk, D, seed=3)
    o, lse = prefill_window_ref(q, k, v, 1)
    for h in range(Hq):
        np.testing.assert_array_equal(o[0, h], v[0, h // 2, Sk - Sq:].astype(np.float32))
        s = np.einsum("id,id->i", q[0, h], k[0, h // 2, Sk - Sq:]) / np.sqrt(D)
        np.testing.assert_allclose(lse[0, h], s, rtol=1e-6, atol=1e-6)
    assert list(visible_counts(6, 9, 1)) == [1] * 6
    assert list(visible_counts(4, 2, 3)) == [0, 0, 1, 2]
    assert list(visible_counts(3, 8, 4)) == [4, 4, 4]


@pytest.mark.parametrize("window", [3, 100])
def test_sinks_of_minus_inf_are_no_sinks(window):
    q, k, v = _problem(1, 4, 2, 12, 7, 16, seed=5)
    o, lse = prefill_window_ref(q, k, v, window, sinks=np.full(4, -np.inf))
    o0, lse0 = prefill_window_ref(q, k, v, window)
    assert np.array_equal(o, o0) and np.array_equal(lse, lse0)


@pytest.mark.parametrize("delta", [-3.0, 0.0, 2.5])
def test_sink_share_of_a_row(delta):
    """sinks[h] = lse_nosink[row, h] + delta  =>  the sink takes sigmoid(delta) of that row's softmax"""
    B, Hq, Hkv, Sq, Sk, D = 1, 4, 2, 10, 14, 16
    q, k, v = _problem(B, Hq, Hkv, Sq, Sk, D, seed=7)
    window, row = 5, 6
    o0, lse0 = prefill_window_ref(q, k, v, window)
    sinks = lse0[0, :, row].astype(np.float64) + delta
    o, lse = prefill_window_ref(q, k, v, window, sinks=sinks)
    np.testing.assert_allclose(o[0, :, row], (1.0 - sigmoid(delta)) * o0[0, :, row], rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(lse[0, :, row], np.logaddexp(lse0[0, :, row], sinks), rtol=1e-6, atol=1e-6)
    # a row without a key stays empty under a sink
    o2, lse2 = prefill_window_ref(q[:, :, :], k[:, :, :4], v[:, :, :4], window, sinks=sinks)
    assert np.all(o2[:, :, :Sq - 4] == 0) and np.all(lse2[:, :, :Sq - 4] == -np.inf)
    assert np.all(np.isfinite(lse2[:, :, Sq - 4:]))


# ---- the C ABI ----

@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def test_symbol_exported_and_in_header(lib):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+sfa_prefill_window_fwd\s*\(\s*const\s+sfa_prefill_args\s*\*\s*args\s*,\s*int\s+window\s*,"
                     r"\s*const\s+float\s*\*\s*sinks\s*,\s*void\s*\*\s*stream\s*\)\s*;", text)
    assert "sfa_prefill_window_fwd" in _lib.EXPORTED_SYMBOLS
    assert hasattr(lib, "sfa_prefill_window_fwd")
    assert lib.sfa_abi_version() == 4
    assert lib.sfa_prefill_window_fwd(None, 1, None, None) == -1           # NULL args
    assert lib.sfa_last_error().startswith(NAME)


def _well_formed():
    p = _lib.PrefillArgs()
    p.q, p.k, p.v, p.o = 0x1000, 0x2000, 0x3000, 0x4000
    p.batch, p.heads_q, p.heads_kv, p.seqlen_q, p.seqlen_k, p.head_dim = 1, 4, 2, 16, 16, 128
    for st in (p.q_stride, p.k_stride, p.v_stride, p.o_stride):
        st[0], st[1], st[2] = 4 * 16 * 128, 16 * 128, 128
    p.dtype = _lib.DTYPE_BF16
    p.causal = 1
    return p


MALFORMED = [
    ("causal = 0", dict(causal=0), 8, None, -2),
    ("window = 0", dict(), 0, None, -2),
    ("window negative", dict(), -5, None, -2),
    ("head_dim 256", dict(head_dim=256), 8, None, -4),
    ("head_dim 96", dict(head_dim=96), 8, None, -4),
    ("misaligned sinks", dict(), 8, 0x5002, -2),
    ("bad dtype", dict(dtype=7), 8, None, -3),
    ("q missing", dict(q=None), 8, None, -1),
    ("heads not a multiple", dict(heads_q=3), 8, None, -2),
    ("misaligned k", dict(k=0x2008), 8, None, -2),
]


@pytest.mark.skipif(torch.cuda.is_available(), reason="calls sfa_prefill_window_fwd with fake device pointers")
def test_argument_validation(lib):
    lib.sfa_debug_get.restype = ctypes.c_int
    last = lib.sfa_debug_get(b"last_prefill_kernel")
    for what, fields, window, sinks, want in MALFORMED:
        p = _well_formed()
        for f, val in fields.items():
            setattr(p, f, val)
        st = lib.sfa_prefill_window_fwd(ctypes.byref(p), window, sinks, None)
        err = lib.sfa_last_error()
        assert st == want, (what, st, err)
        assert err.startswith(NAME), (what, err)
    p = _well_formed()
    p.q_stride[2] = 132
    assert lib.sfa_prefill_window_fwd(ctypes.byref(p), 8, None, None) == -2
    assert lib.sfa_last_error().startswith(NAME)
    # nothing to do: 0, and nothing is launched (the pointers are fake)
    for field in ("batch", "seqlen_q"):
        p = _well_formed()
        setattr(p, field, 0)
        assert lib.sfa_prefill_window_fwd(ctypes.byref(p), 8, 0x5000, None) == 0, field
        assert lib.sfa_prefill_window_fwd(ctypes.byref(p), 2 ** 31 - 1, None, None) == 0, field
    assert lib.sfa_debug_get(b"last_prefill_kernel") == last
    # sfa_prefill_fwd keeps its own name and still serves head_dim 256 up to its launch
    p = _well_formed()
    p.head_dim = 96
    assert lib.sfa_prefill_fwd(ctypes.byref(p), None) == -4
    assert lib.sfa_last_error().startswith(b"sfa_prefill_fwd:") and b"{64, 128, 256}" in lib.sfa_last_error()


def test_python_layer_exports_the_operator():
    import starflashattention_amd as m
    assert callable(m.flash_attn_window_fwd)
    with pytest.raises(RuntimeError, match="float16 or bfloat16"):
        m.flash_attn_window_fwd(torch.zeros(1, 1, 4, 64), torch.zeros(1, 1, 4, 64), torch.zeros(1, 1, 4, 64), 2)
