"""CPU-only checks of sfa_decode_chunk_kv8_window / sfa_decode_varlen_kv8_window (the sliding window in the multi-token
decode calls over an fp8 e4m3 KV cache): the reference of tests/chunk_kv8_window_ref.py is kv8_window_ref.
decode_kv8_window_ref applied token by token and chunk_kv8_ref.chunk_kv8_ref where the window does not bind, the window
binds in the frame's long sequence, the sweep of the GPU tests covers its factors pairwise, the window-edge problems hold
their values exactly in e4m3 and tell every one-row slip apart, and the two entry points exist and validate their
arguments before any HIP call."""
import ctypes
import itertools
import os

import numpy as np
import pytest
import torch

from conftest import ROOT
from starflashattention_amd import _lib
import chunk_kv8_ref as ckr
import chunk_kv8_window_ref as ref
import chunk_window_ref as cw
import kv8_ref
import kv8_window_ref as kwr
from chunk_kv8_window_ref import HKV, LAYER, LENS, QTILE, TOL


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


# ---- 1, 2. the reference -----------------------------------------------------------------------------------------------

def _kwargs(p):
    kw = {}
    if p.biases is not None:
        kw = dict(q_bias=p.biases[0], k_bias=p.biases[1], v_bias=p.biases[2])
    if p.tables:
        cos, sin = ref.rotary_tables(p.dtype, p.rot)
        kw.update(cos_table=cos, sin_table=sin)
    return kw


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_reference_is_decode_kv8_window_ref_token_by_token(dtype):
    """n successive decode_kv8_window_ref calls per sequence, seq_len advanced by one, each on the cache the one before
    left: the same outputs (1e-12) and the same cache bytes"""
    for tables in (False, True):
        p = ref.make_problem(dtype, 64, 2, (0, 5, 70, 130), (9, 0, 20, 3), tables=tables, seed=3, k_factors=(0.5, 2.0))
        for window in (1, 17, 33, None):
            got, k_got, v_got = ref.reference(p, window)
            kc, vc = p.k8.copy(), p.v8.copy()
            for b, (pos, n) in enumerate(zip(p.lens, p.ns)):
                assert got["o"][b].shape == (n, p.H, p.D)
                for t in range(n):
                    r = kwr.decode_kv8_window_ref(p.tok[b][t][None], kc[b:b + 1], vc[b:b + 1], [pos + t], LAYER, p.rot,
                                                  dtype, window, p.ks, p.vs, **_kwargs(p))
                    np.testing.assert_allclose(got["o"][b][t].astype(np.float32), r["o"][0], atol=1e-12, rtol=0)
            np.testing.assert_array_equal(k_got, kc)
            np.testing.assert_array_equal(v_got, vc)
            assert not np.array_equal(kc, p.k8)


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_reference_without_a_binding_window_is_chunk_kv8_ref_to_the_bit(dtype):
    p = ref.make_problem(dtype, 64, 2, (0, 5, 70, 130), (9, 0, 20, 3), seed=4)
    k0, v0 = p.k8.copy(), p.v8.copy()
    want = ckr.chunk_kv8_ref(p.tok, k0, v0, p.lens, LAYER, p.rot, dtype, p.ks, p.vs, **_kwargs(p))
    for window in (None, max(pos + n for pos, n in zip(p.lens, p.ns)), 5000):
        got, k1, v1 = ref.reference(p, window)
        for a, b in zip(got["o"] + got["q16"], want["o"] + want["q16"]):
            np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(k1, k0)
        np.testing.assert_array_equal(v1, v0)
    # one row short of it, the longest sequence's last token loses row 0: not the same any more
    got, _, _ = ref.reference(p, 132)
    assert not np.array_equal(got["o"][3][2], want["o"][3][2])
    np.testing.assert_array_equal(got["o"][3][1], want["o"][3][1])
    # 0x7F below lo_0 changes nothing of a windowed result
    q = ref.make_problem(dtype, 64, 2, p.lens, p.ns, seed=4)
    q.k8, q.v8 = ref.poisoned(p.k8, p, 17), ref.poisoned(p.v8, p, 17)
    a, b = ref.reference(p, 17)[0], ref.reference(q, 17)[0]
    for x, y in zip(a["o"], b["o"]):
        np.testing.assert_array_equal(x, y)
        assert np.isfinite(x).all()


# ---- 3. the window binds -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_window_binds_in_the_reference(dtype):
    """pos = 1000, window = 100, n = 40, G = 4, D = 128: the windowed and the full reference differ by more than ten
    tolerances (measured with numpy on this data: a gap of 0.90 against bars of 0.025 in fp16 and 0.20 in bf16)"""
    D, G, n, window = 128, 4, 40, 100
    win, full = ref.frame_reference(dtype, D, G, n, window)[0], ref.frame_reference(dtype, D, G, n, None)[0]
    b = LENS.index(1000)
    gap = np.abs(win["o"][b] - full["o"][b]).max()
    bar = 10 * TOL[dtype] * (1.0 + np.abs(full["o"][b]).max())
    print("gap %.3f, bar %.3f" % (gap, bar))
    assert gap > bar
    for b in (0, 1):                                            # pos + n <= window: the window does not bind
        np.testing.assert_array_equal(win["o"][b], full["o"][b])


# ---- 4. the sweep ------------------------------------------------------------------------------------------------------

def test_sweep_covers_its_factors_pairwise():
    F = ref.FACTORS
    assert F[:6] == kwr.FACTORS and F[6] == (1, 5, 45, 70)
    assert len(set(ref.SWEEP)) == len(ref.SWEEP)
    for c in ref.SWEEP:
        assert len(c) == len(F) and all(x in f for x, f in zip(c, F)), c
    for i, j in itertools.combinations(range(len(F)), 2):
        seen = {(c[i], c[j]) for c in ref.SWEEP}
        assert seen == set(itertools.product(F[i], F[j])), (i, j)
    assert any(QTILE < c[3] * c[6] <= 2 * QTILE for c in ref.SWEEP)      # two q-tiles
    assert any(c[3] * c[6] > 2 * QTILE for c in ref.SWEEP)               # and more


# ---- 5. the window-edge problems -----------------------------------------------------------------------------------------

def test_edge_problems_hold_the_16_bit_problems_values_exactly():
    """every cache value and every new k / v row of the edge problems is scale * (an e4m3 number) under power-of-two
    scales (edge_problem asserts it), the lengths put lo_0 on EDGE_LO0, and the spike and ramp problems give what the
    16-bit problems they are made from give"""
    assert all(float(s) == 2.0 ** round(np.log2(s)) for s in ref.EDGE_SCALES) and len(set(ref.EDGE_SCALES.tolist())) == 2
    assert ref.EDGE_N > QTILE
    for window in ref.EDGE_WINDOWS:
        assert tuple(ref.window_lo(pos, window) for pos in ref.edge_lens(window)) == ref.EDGE_LO0
    for window in (17, 100):
        for kind in ("spike", "equal", "ramp"):
            p = ref.edge_problem("bf16", window, kind)
            assert p.rot == 0 and p.biases is None and p.G == 1
            got = ref.edge_reference(window, kind)[0]
            want = cw.chunk_window_ref(cw.edge_problem("bf16", window, kind), window)
            for b in range(p.B):
                np.testing.assert_allclose(got["o"][b], want[b][0], atol=1e-5, rtol=1e-5)
    # edge_reference is reference() of the problem: the same bytes, the same outputs
    for window, kind in ((17, "spike"), (40, "ramp")):
        fast, slow = ref.edge_reference(window, kind), ref.reference(ref.edge_problem("fp16", window, kind), window)
        np.testing.assert_array_equal(fast[1], slow[1])
        np.testing.assert_array_equal(fast[2], slow[2])
        for a, b in zip(fast[0]["o"] + fast[0]["q16"], slow[0]["o"] + slow[0]["q16"]):
            np.testing.assert_allclose(a, b, atol=1e-12, rtol=0)
    # the spike carries all the weight: every token that sees row j* returns v_scale * V8[j*]
    p = ref.edge_problem("fp16", 17, "spike")
    got, _, v_ref = ref.edge_reference(17, "spike")
    for b, (pos, jstar) in enumerate(ref.spike_rows(17)):
        vstar = kv8_ref.dequantize(v_ref[b, LAYER, jstar], p.vs)
        for t in range(ref.EDGE_N):
            sees = ref.window_lo(pos + t, 17) <= jstar <= pos + t
            assert np.allclose(got["o"][b][t], vstar, atol=1e-20, rtol=1e-15) == sees, (b, t)


@pytest.mark.parametrize("window", ref.EDGE_WINDOWS)
def test_equal_keys_problem_tells_every_one_row_slip(window):
    """From the reference alone: with all keys equal, a row dropped, added or counted twice at either edge of any token's
    window moves o by more than five tolerances of either dtype (every element of a V row holds the same value, so in all
    elements).  The values are exact in fp16, bf16 and e4m3, so one problem serves both dtypes."""
    p = ref.edge_problem("bf16", window, "equal")
    got = ref.edge_reference(window, "equal")[0]
    H = p.H
    for b, pos in enumerate(p.lens):
        old = kv8_ref.dequantize(p.v8[b, LAYER, :pos], p.vs)[:, 0, 0]
        m = np.concatenate([old, p.tok[b][:, H + HKV, 0].astype(np.float64)])
        m = np.concatenate([m, [16.0 if len(m) % 2 == 0 else -16.0]])           # the row after the last token
        for t in range(ref.EDGE_N):
            lo, hi = ref.window_lo(pos + t, window), pos + t
            S, c = m[lo:hi + 1].sum(), hi - lo + 1
            o = S / c
            np.testing.assert_allclose(got["o"][b][t], o, atol=1e-9, rtol=1e-9)
            slips = [(S + m[hi + 1]) / (c + 1), (S + m[lo]) / (c + 1), (S + m[hi]) / (c + 1)]
            if c > 1:
                slips += [(S - m[lo]) / (c - 1), (S - m[hi]) / (c - 1)]
            if lo >= 1:
                slips.append((S + m[lo - 1]) / (c + 1))
            for s in slips:
                assert abs(s - o) > 5 * max(TOL.values()) * (1.0 + abs(o)), (b, t, s, o)


# ---- 6. the C ABI without a GPU ------------------------------------------------------------------------------------------

NEW_SYMBOLS = ("sfa_decode_chunk_kv8_window", "sfa_decode_varlen_kv8_window")
NULL_POINTER, BAD_SHAPE, UNSUPPORTED_HEAD_DIM, WORKSPACE_TOO_SMALL = -1, -2, -4, -5


def test_chunk_kv8_window_symbols_exported(lib):
    import starflashattention_amd as sfa
    from starflashattention_amd import ops
    with open(os.path.join(ROOT, "include", "star_flash_attn.h")) as f:
        header = f.read()
    for name in NEW_SYMBOLS:
        assert name in _lib.EXPORTED_SYMBOLS
        assert hasattr(lib, name)
        assert name + "(" in header
    assert sfa.flash_decode_chunk_kv8_window is ops.flash_decode_chunk_kv8_window
    assert sfa.flash_decode_varlen_kv8_window is ops.flash_decode_varlen_kv8_window
    assert "flash_decode_chunk_kv8_window" in ops.__doc__ and "flash_decode_varlen_kv8_window" in ops.__doc__
    # new symbols beside the same struct and the same ABI version; no sizing functions of their own
    assert "#define SFA_ABI_VERSION 4" in header and lib.sfa_abi_version() == 4
    assert "kv8_window_workspace_bytes" not in header
    # the cell is no longer listed as unserved
    assert "Not served: a sliding window over the fp8 cache" not in header
    assert "Not served: an fp8 cache in these windowed multi-token calls" not in header


def _args():
    a = _lib.DecodeArgs()
    for f in ("qkv", "o", "seq_len", "k_cache_table", "v_cache_table"):
        setattr(a, f, 0x1000)
    a.batch_size, a.num_heads, a.num_heads_kv, a.memory_max_len, a.num_layer, a.head_dim = 1, 8, 4, 64, 1, 128
    a.rotary_embedding_dim = 128
    return a


@pytest.mark.skipif(torch.cuda.is_available(), reason="calls the entry points with fake device pointers")
@pytest.mark.parametrize("fn", NEW_SYMBOLS)
def test_chunk_kv8_window_argument_validation_without_gpu(lib, fn):
    chunk = fn == "sfa_decode_chunk_kv8_window"
    P = ctypes.c_void_p

    def call(a, w=8, n=4, ks=None, vs=None, cu=0x4000):
        ap = ctypes.byref(a) if a is not None else None
        if chunk:
            return lib.sfa_decode_chunk_kv8_window(ap, P(ks), P(vs), n, 0, w, None)
        return lib.sfa_decode_varlen_kv8_window(ap, P(ks), P(vs), P(cu), n, 0, w, None)

    err = lambda: lib.sfa_last_error()
    named = lambda: err().startswith(fn.encode() + b":")
    assert call(None) == NULL_POINTER and named()
    assert call(_lib.DecodeArgs()) == NULL_POINTER and named()
    a = _args()
    for w in (0, -3):
        assert call(a, w) == BAD_SHAPE and named() and b"window" in err()
    assert call(a, n=-1) == BAD_SHAPE
    a.head_dim = 256
    assert call(a) == UNSUPPORTED_HEAD_DIM and named()
    a.head_dim = 96
    assert call(a) == UNSUPPORTED_HEAD_DIM
    a.head_dim = 128
    for ks, vs in ((0x3001, None), (None, 0x3002), (0x3004, 0x3007)):       # a scale pointer that is not 4-byte aligned
        assert call(a, ks=ks, vs=vs) == BAD_SHAPE and named() and b"k_scale / v_scale" in err()
    if not chunk:
        assert call(a, cu=None) == NULL_POINTER and named() and b"cu_tokens" in err()
        assert call(a, cu=0x4002) == BAD_SHAPE and b"cu_tokens" in err()
    assert call(a, n=0) == 0 and call(a, n=0, ks=0x3004, vs=0x3008) == 0       # nothing to do
    # the scales are checked before the workspace
    assert call(a) == NULL_POINTER and b"workspace is NULL" in err()
    assert call(a, ks=0x3001) == BAD_SHAPE
    assert call(a, 1) == NULL_POINTER and call(a, 2 ** 31 - 1) == NULL_POINTER     # any window >= 1
    # a workspace one byte too small at an explicit split count; with that byte the call gets as far as the alignment
    S, n, W = 3, 4, 8
    sizer = lib.sfa_decode_chunk_window_workspace_bytes if chunk else lib.sfa_decode_varlen_window_workspace_bytes
    need = sizer(a.batch_size, a.num_heads, a.num_heads_kv, a.head_dim, a.memory_max_len, n, W, S)
    assert need > 256
    a.num_splits, a.workspace, a.workspace_bytes = S, 0x2010, need - 1
    assert call(a, W, n) == WORKSPACE_TOO_SMALL and named()
    a.workspace_bytes = need
    assert call(a, W, n) == BAD_SHAPE and b"256-byte aligned" in err()
    a.batch_size = 0
    assert call(a) == 0
