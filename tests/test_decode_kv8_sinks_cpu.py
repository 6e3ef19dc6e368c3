"""CPU-only checks of sfa_decode_kv8_window_sinks / sfa_decode_chunk_kv8_window_sinks / sfa_decode_varlen_kv8_window_sinks
(attention sinks in the three windowed decode calls over an fp8 e4m3 KV cache): the symbols and the Python operators exist
beside an unchanged sfa_decode_args and ABI version, each entry point validates its arguments under its own name before
any HIP call, the references of tests/kv8_sinks_ref.py have the properties the GPU tests lean on -- the bars of
tests/test_decode_kv8_sinks_gpu.py are met by the references alone, at its problems -- and the three new translation units
compile for gfx950 without scratch at the occupancy and LDS size of their _kv8_window twins."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT
from starflashattention_amd import _lib
import chunk_kv8_window_ref as ckw
import kv8_sinks_ref as ksr
import kv8_window_ref as kwr
from kv8_sinks_ref import BINDS, HKV, LAYER, LENS, SCALED, TOL, scaled_problem, wrongly_scaled

CSRC = os.path.join(ROOT, "starflashattention_amd", "csrc")
NAMES = ("sfa_decode_kv8_window_sinks", "sfa_decode_chunk_kv8_window_sinks", "sfa_decode_varlen_kv8_window_sinks")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def test_kv8_sinks_symbols_exported(lib):
    for name in NAMES:
        assert name in _lib.EXPORTED_SYMBOLS
        assert hasattr(lib, name)
    import starflashattention_amd as sfa
    from starflashattention_amd import ops
    for name in ("flash_decode_kv8_window_sinks", "flash_decode_chunk_kv8_window_sinks", "flash_decode_varlen_kv8_window_sinks"):
        assert getattr(sfa, name) is getattr(ops, name)
        assert name in ops.__doc__
    with open(os.path.join(ROOT, "include", "star_flash_attn.h")) as f:
        header = f.read()
    assert all(name + "(" in header for name in NAMES)
    # new symbols beside the same struct and the same ABI version, and no sizing functions of their own
    assert lib.sfa_abi_version() == 4 and "#define SFA_ABI_VERSION 4" in header
    assert ctypes.sizeof(_lib.DecodeArgs) == 10 * 8 + 12 * 4 + 8 + 8 + 8 + 8 + 8 + 8
    assert "sinks_workspace_bytes" not in header and not any("sinks_workspace" in s for s in _lib.EXPORTED_SYMBOLS)
    # the fp8 half of the surface is no longer listed as unserved
    assert "do not serve sinks yet" not in header and "16-bit caches only" not in header


def _args():
    a = _lib.DecodeArgs()
    for f in ("qkv", "o", "seq_len", "k_cache_table", "v_cache_table"):
        setattr(a, f, 0x1000)
    a.batch_size, a.num_heads, a.num_heads_kv, a.memory_max_len, a.num_layer, a.head_dim = 1, 8, 4, 64, 1, 128
    a.rotary_embedding_dim = 128
    return a


CU, SINKS, KS, VS = 0x4000, 0x5000, 0x3004, 0x3008


def _callers(lib):
    """(name, call(a, sinks, window, count, cu, ks, vs), sizing(B, H, Hkv, D, M, count, window, S)) of the entry points"""
    P = ctypes.c_void_p
    ref = lambda a: ctypes.byref(a) if a is not None else None
    one = lambda a, sinks=SINKS, window=8, count=4, cu=CU, ks=KS, vs=VS: lib.sfa_decode_kv8_window_sinks(
        ref(a), P(ks), P(vs), P(sinks), window, None)
    chunk = lambda a, sinks=SINKS, window=8, count=4, cu=CU, ks=KS, vs=VS: lib.sfa_decode_chunk_kv8_window_sinks(
        ref(a), P(ks), P(vs), P(sinks), count, 0, window, None)
    varlen = lambda a, sinks=SINKS, window=8, count=4, cu=CU, ks=KS, vs=VS: lib.sfa_decode_varlen_kv8_window_sinks(
        ref(a), P(ks), P(vs), P(sinks), P(cu), count, 0, window, None)
    return ((NAMES[0], one, lambda B, H, Hkv, D, M, n, W, S: lib.sfa_decode_window_workspace_bytes(B, H, Hkv, D, M, W, S)),
            (NAMES[1], chunk, lib.sfa_decode_chunk_window_workspace_bytes),
            (NAMES[2], varlen, lib.sfa_decode_varlen_window_workspace_bytes))


@pytest.mark.skipif(torch.cuda.is_available(), reason="calls the entry points with fake device pointers")
@pytest.mark.parametrize("which", [0, 1, 2])
def test_kv8_sinks_argument_validation_without_gpu(lib, which):
    name, call, sizing = _callers(lib)[which]
    fn = name.encode() + b":"
    err = lambda: lib.sfa_last_error()
    assert call(None) == -1 and err().startswith(fn)
    assert call(_lib.DecodeArgs()) == -1 and err().startswith(fn)
    a = _args()
    a.v_cache_table = None
    assert call(a) == -1 and err().startswith(fn)
    a = _args()
    a.head_dim = 96
    assert call(a) == -4 and err().startswith(fn)
    a.head_dim = 256                                            # no fp8 call serves head_dim 256
    assert call(a) == -4 and err().startswith(fn) and b"256" in err()
    a.head_dim = 128
    a.dtype = 7
    assert call(a) == -3 and err().startswith(fn)
    a.dtype = 1
    a.num_heads, a.num_heads_kv = 12, 4                         # group of 3
    assert call(a) == -2 and err().startswith(fn) and b"num_heads_kv" in err()
    a.num_heads, a.num_heads_kv = 16, 1                         # every group up to 16 is served
    for w in (0, -5):
        assert call(a, window=w) == -2 and err().startswith(fn) and b"window" in err()
    for bad in (SINKS + 1, SINKS + 2, SINKS + 3):
        assert call(a, sinks=bad) == -2 and err().startswith(fn) and b"sinks" in err()
    for ks, vs in ((0x3001, None), (None, 0x3002), (0x3004, 0x3007)):       # a scale pointer that is not 4-byte aligned
        assert call(a, ks=ks, vs=vs) == -2 and err().startswith(fn) and b"k_scale / v_scale" in err()
    # the alignment of sinks is checked first; the scales before the window, as in the twins
    assert call(a, sinks=SINKS + 2, ks=0x3001, window=0) == -2 and b"sinks" in err()
    assert call(a, ks=0x3001, window=0) == -2 and b"k_scale / v_scale" in err()
    if which == 2:
        assert call(a, cu=None) == -1 and err().startswith(fn) and b"cu_tokens" in err()
        assert call(a, cu=CU + 2) == -2 and err().startswith(fn) and b"cu_tokens" in err()
    # a well-formed call -- with sinks, without (NULL), without scales (NULL = 1.0), with the largest window -- gets as far
    # as the workspace
    for kw in ({}, {"sinks": None}, {"ks": None, "vs": None}, {"window": 2 ** 31 - 1}):
        assert call(a, **kw) == -1 and err().startswith(fn + b" workspace is NULL")
    a.workspace, a.workspace_bytes, a.num_splits = 0x2000, 256, 2
    assert call(a) == -5 and err().startswith(fn)
    a.workspace_bytes = sizing(1, 16, 1, 128, 64, 4, 8, 2) - 1
    assert call(a) == -5 and err().startswith(fn)               # one byte short of the twin's sizing function
    assert call(a, sinks=None) == -5 and err().startswith(fn)   # NULL sinks: still this call's name
    if which:
        assert call(a, count=0) == 0                            # nothing to do
    a.batch_size = 0
    assert call(a) == 0


# ---- the references ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,D,G,window,anchor", [("fp16", 64, 8, 33, 0), ("bf16", 128, 1, 5000, 2), ("bf16", 64, 4, 1, 1),
                                                     ("fp16", 128, 2, 100, 3)])
def test_single_token_reference_properties(dtype, D, G, window, anchor):
    H = HKV * G
    plain = kwr.reference(dtype, D, G, window)
    _, none = ksr.single_ref(dtype, D, G, window)
    ninf = ksr.single_with(dtype, D, G, window, np.full(H, -np.inf))
    for r in (none, ninf):                      # all sinks -inf: the _kv8_window reference, exactly
        for key in ("o", "k_row", "v_row", "k8", "v8"):
            np.testing.assert_array_equal(r[key], plain[key])
    delta = ksr.deltas(H)
    sinks, got = ksr.single_ref(dtype, D, G, window, anchor=anchor)
    assert sinks.dtype == np.float32
    np.testing.assert_array_equal(got["lse"], none["lse"])
    for key in ("k_row", "v_row", "k8", "v8"):  # the caches receive exactly what the twin stores
        np.testing.assert_array_equal(got[key], plain[key])
    # o_sinks = o_window * sum / (sum + exp(sink)) = o_window * sigmoid(lse - sink), on the references' fp64 outputs
    s64 = sinks.astype(np.float64)
    want = none["o64"] * ksr.sigmoid(none["lse"] - s64[None, :])[:, :, None]
    assert np.abs(got["o64"] - want).max() <= 1e-12
    np.testing.assert_array_equal(got["o"], got["o64"].astype(np.float32))
    # the anchor row's shares are sigmoid(delta): before the sinks are rounded to float32 to 1e-12, after it to 1e-5
    exact = ksr.make_sinks(none["lse"][anchor])
    assert np.abs(ksr.sigmoid(exact - none["lse"][anchor]) - ksr.sigmoid(delta)).max() <= 1e-12
    share = ksr.sigmoid(s64 - none["lse"][anchor])
    assert np.abs(share - ksr.sigmoid(delta)).max() <= 1e-5
    assert share.min() > 0.047 and share.max() < 0.953 and len(set(np.round(share, 6))) == H


@pytest.mark.parametrize("dtype,D,G,n,window,anchor", [("bf16", 64, 8, 9, 33, 3), ("fp16", 128, 1, 40, 17, 0),
                                                       ("fp16", 64, 16, 5, 5000, 2), ("bf16", 128, 2, 3, 2, 1)])
def test_chunk_reference_properties(dtype, D, G, n, window, anchor):
    p = ckw.problem(dtype, D, G, n)
    H = p.H
    plain, k_plain, v_plain = ckw.frame_reference(dtype, D, G, n, window)
    _, (none, k_none, v_none) = ksr.chunk_ref(dtype, D, G, n, window)
    ninf, k_ninf, v_ninf = ksr.chunk_kv8_sinks_ref(p, window, np.full(H, -np.inf))
    for r, k, v in ((none, k_none, v_none), (ninf, k_ninf, v_ninf)):        # all sinks -inf: the twin's reference, exactly
        np.testing.assert_array_equal(k, k_plain)
        np.testing.assert_array_equal(v, v_plain)
        for b in range(p.B):
            np.testing.assert_array_equal(r["o"][b], plain["o"][b])
    delta = ksr.deltas(H)
    sinks, (got, k_got, v_got) = ksr.chunk_ref(dtype, D, G, n, window, anchor=anchor)
    np.testing.assert_array_equal(k_got, k_plain)
    np.testing.assert_array_equal(v_got, v_plain)
    s64 = sinks.astype(np.float64)
    for b in range(p.B):                                        # o_sinks == o_window * sigmoid(lse - sink), in fp64
        want = none["o"][b] * ksr.sigmoid(none["lse"][b] - s64[None, :])[:, :, None]
        assert np.abs(got["o"][b] - want).max() <= 1e-12
        np.testing.assert_array_equal(got["lse"][b], none["lse"][b])
    exact = ksr.make_sinks(none["lse"][anchor][0])              # token 0 of the anchor sequence
    assert np.abs(ksr.sigmoid(exact - none["lse"][anchor][0]) - ksr.sigmoid(delta)).max() <= 1e-12
    assert np.abs(ksr.sigmoid(s64 - none["lse"][anchor][0]) - ksr.sigmoid(delta)).max() <= 1e-5
    # the single-token reference is the chunk reference of one token
    if n >= 1:
        one = ckw.make_problem(dtype, D, G, LENS, (1,) * 4)
        t = kwr.tokens(dtype, D, G)
        one.tok, one.biases = [t.qkv[b][None] for b in range(4)], (t.qb, t.kb, t.vb)
        c1, _, _ = ksr.chunk_kv8_sinks_ref(one, window, sinks)
        s1 = ksr.single_with(dtype, D, G, window, sinks)
        for b in range(4):
            assert np.abs(c1["o"][b][0] - s1["o64"][b]).max() <= 1e-12
    # a ragged batch: the varlen reference gives every sequence's tokens what the chunk reference gives them
    ns = (min(3, n), 0, n, 1)
    ragged = ckw.make_problem(dtype, D, G, LENS, ns)
    ragged.tok, ragged.biases = [p.tok[b][:nb] for b, nb in enumerate(ns)], p.biases
    rv, _, _ = ksr.varlen_kv8_sinks_ref(ragged, window, sinks)
    for b, nb in enumerate(ns):
        assert rv["o"][b].shape[0] == nb
        if nb == 0:
            continue
        assert np.abs(rv["o"][b] - got["o"][b][:nb]).max() <= 1e-12
        assert np.abs(rv["lse"][b] - got["lse"][b][:nb]).max() <= 1e-12


# ---- the bars of the GPU tests, met by the references alone ----------------------------------------------------------------

@pytest.mark.parametrize("call", ["single", "chunk"])
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_sink_binds_in_the_reference(dtype, call):
    """On the anchor row the heads with delta >= 0 (a sink share of at least one half) leave the _kv8_window reference by
    more than 10 tol (1 + max |o|): a kernel that ignores `sinks` cannot pass the GPU test.  A window of 4 rows keeps |o|
    of the order of a V row, so that half of it is many tolerances.  (The varlen call's problem is the chunk call's.)"""
    D, G, n, window, anchor = (BINDS[k] for k in ("D", "G", "n", "window", "anchor"))
    H, tol = HKV * G, TOL[dtype]
    if call == "single":
        got, base = ksr.single_ref(dtype, D, G, window, anchor=anchor)[1]["o64"][anchor], ksr.single_ref(dtype, D, G, window)[1]["o64"][anchor]
    else:
        got = ksr.chunk_ref(dtype, D, G, n, window, anchor=anchor)[1][0]["o"][anchor][0]
        base = ksr.chunk_ref(dtype, D, G, n, window)[1][0]["o"][anchor][0]
    heads = [h for h in range(H) if ksr.deltas(H)[h] >= 0]
    assert len(heads) == H // 2
    for h in heads:
        gap = np.abs(got[h] - base[h]).max()
        assert gap > 10 * tol * (1.0 + np.abs(base[h]).max()), (h, gap)


@pytest.mark.parametrize("call", ["single", "chunk"])
def test_a_scaled_sink_misses_the_tolerance_in_the_reference(call):
    """k_scale / v_scale with factors (0.5, 2) per kv head, Hkv = 2, G = 8: the reference with the sink multiplied by
    k_scale, or by head_dim_inv, is more than 2 tol (1 + |o|) away from the right one in some element of the anchor row
    under either kv head -- so an output within tol of the right reference is outside tol of either wrong one."""
    s = SCALED
    dtype, D, G, window, anchor, tol = s["dtype"], s["D"], s["G"], s["window"], s["anchor"], TOL[s["dtype"]]
    if call == "single":
        sinks, right = ksr.single_ref(dtype, D, G, window, anchor=anchor, k_factors=s["k_factors"])
        ks = kwr.caches(D, s["k_factors"]).ks
        o_of = lambda sk: ksr.single_with(dtype, D, G, window, sk, k_factors=s["k_factors"])["o64"][anchor]
        right = right["o64"][anchor]
    else:
        p = scaled_problem()
        sinks = ksr.anchor_sinks(p, window, anchor)
        ks = p.ks
        o_of = lambda sk: ksr.chunk_kv8_sinks_ref(p, window, sk)[0]["o"][anchor][0]
        right = o_of(sinks)
    for what, wrong in wrongly_scaled(sinks.astype(np.float64), ks, D, G).items():
        o = o_of(wrong)
        for hk in range(HKV):
            h = slice(hk * G, (hk + 1) * G)
            assert (np.abs(o[h] - right[h]) > 2 * tol * (1.0 + np.abs(right[h]))).any(), (what, hk)


# ---- the new translation units -------------------------------------------------------------------------------------------

def _remarks(src, tmp_path, tag):
    r = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-I" + ROOT,
                        "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, src), "-o",
                        str(tmp_path / (tag + ".o"))], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    out = {}
    for blk in r.stderr.split("Function Name: ")[1:]:
        name = blk.split()[0]
        out[name] = {k: int(re.search(re.escape(k) + r": (\d+)", blk).group(1))
                     for k in ("VGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "LDS Size [bytes/block]")}
    return out


def _instantiation(mangled, kernel):
    """the template arguments after the element type of a mangled kernel name -- chunk_attn_kernel<GEO, Tr, D, PAGED>:
    (dtype, D, PAGED); decode_kv8_window*_kernel<Tr, D, NT, PAGED>: (dtype, D, NT, PAGED) -- or None"""
    if kernel not in mangled:
        return None
    m = re.search(r"(Fp16|Bf16)ELi(\d+)((?:ELb[01])+)E", mangled)
    return (m.group(1), int(m.group(2))) + tuple(int(x) for x in re.findall(r"ELb([01])", m.group(3)))


@pytest.mark.parametrize("new,twin,count,n_attn,kernel,new_kernel,marks", [
    ("decode_kv8_window_sinks_kernel.hip", "decode_kv8_window_kernel.hip", 16, 16, "decode_kv8_window_kernel",
     "decode_kv8_window_sinks_kernel", ()),
    ("decode_chunk_kv8_window_sinks_kernel.hip", "decode_chunk_kv8_window_kernel.hip", 20, 8, "chunk_attn_kernel",
     "chunk_attn_kernel", ("Kv8WindowSinkGeo", "UniformGeo")),
    ("decode_varlen_kv8_window_sinks_kernel.hip", "decode_varlen_kv8_window_kernel.hip", 21, 8, "chunk_attn_kernel",
     "chunk_attn_kernel", ("Kv8WindowSinkGeo", "RaggedGeo")),
])
def test_kv8_sinks_kernels_compile_without_scratch_at_the_twins_occupancy(tmp_path, new, twin, count, n_attn, kernel,
                                                                          new_kernel, marks):
    """Every kernel of a new translation unit compiles for gfx950 with no spill to scratch, the unit has its twin unit's
    kernel count, and each attention kernel has the occupancy and the LDS size of its _kv8_window twin's kernel of the
    same template arguments.  The VGPR counts are printed, not pinned."""
    mine = _remarks(new, tmp_path, "sinks")
    theirs = _remarks(twin, tmp_path, "twin")
    assert len(mine) == len(theirs) == count, (sorted(mine), sorted(theirs))
    assert all(v["ScratchSize [bytes/lane]"] == 0 for v in mine.values()), mine
    by_inst = {_instantiation(nm, kernel): v for nm, v in theirs.items()}
    by_inst.pop(None, None)
    assert len(by_inst) == n_attn
    seen = 0
    for nm, v in mine.items():
        inst = _instantiation(nm, new_kernel)
        if inst is None:
            continue
        assert all(m in nm for m in marks)
        seen += 1
        print(inst, "sinks VGPRs", v["VGPRs"], "twin VGPRs", by_inst[inst]["VGPRs"], "occupancy",
              v["Occupancy [waves/SIMD]"])
        assert v["Occupancy [waves/SIMD]"] == by_inst[inst]["Occupancy [waves/SIMD]"], (inst, v, by_inst[inst])
        assert v["LDS Size [bytes/block]"] == by_inst[inst]["LDS Size [bytes/block]"], (inst, v, by_inst[inst])
    assert seen == n_attn
