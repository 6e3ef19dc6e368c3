"""CPU-only checks of sfa_decode_window_sinks / sfa_decode_chunk_window_sinks / sfa_decode_varlen_window_sinks (attention
sinks in the three windowed decode calls over 16-bit caches): the symbols and the Python operators exist beside an
unchanged sfa_decode_args and ABI version, each entry point validates its arguments under its own name before any HIP
call, the references of tests/sinks_ref.py have the properties the GPU tests lean on, and the three new translation units
compile for gfx950 without scratch at the occupancy of their _window twins."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT
from starflashattention_amd import _lib
import chunk_window_ref as cw
import sinks_ref
from window_ref import decode_window_ref

CSRC = os.path.join(ROOT, "starflashattention_amd", "csrc")
NAMES = ("sfa_decode_window_sinks", "sfa_decode_chunk_window_sinks", "sfa_decode_varlen_window_sinks")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def test_sinks_symbols_exported(lib):
    for name in NAMES:
        assert name in _lib.EXPORTED_SYMBOLS
        assert hasattr(lib, name)
    import starflashattention_amd as sfa
    from starflashattention_amd import ops
    for name in ("flash_decode_window_sinks", "flash_decode_chunk_window_sinks", "flash_decode_varlen_window_sinks"):
        assert getattr(sfa, name) is getattr(ops, name)
    with open(os.path.join(ROOT, "include", "star_flash_attn.h")) as f:
        header = f.read()
    assert all(name + "(" in header for name in NAMES)
    # new symbols beside the same struct and the same ABI version, and no sizing functions of their own
    assert lib.sfa_abi_version() == 4 and "#define SFA_ABI_VERSION 4" in header
    assert ctypes.sizeof(_lib.DecodeArgs) == 10 * 8 + 12 * 4 + 8 + 8 + 8 + 8 + 8 + 8
    assert "sinks_workspace_bytes" not in header and not any("sinks_workspace" in s for s in _lib.EXPORTED_SYMBOLS)


def _args():
    a = _lib.DecodeArgs()
    for f in ("qkv", "o", "seq_len", "k_cache_table", "v_cache_table"):
        setattr(a, f, 0x1000)
    a.batch_size, a.num_heads, a.memory_max_len, a.num_layer, a.head_dim = 1, 2, 64, 1, 128
    a.rotary_embedding_dim = 128
    return a


CU, SINKS = 0x4000, 0x5000


def _callers(lib):
    """(name, call(a, sinks, window, count, cu), sizing(B, H, Hkv, D, M, count, window, S)) of the three entry points"""
    ref = lambda a: ctypes.byref(a) if a is not None else None
    one = lambda a, sinks=SINKS, window=8, count=4, cu=CU: lib.sfa_decode_window_sinks(ref(a), sinks, window, None)
    chunk = lambda a, sinks=SINKS, window=8, count=4, cu=CU: lib.sfa_decode_chunk_window_sinks(ref(a), sinks, count, 0,
                                                                                               window, None)
    varlen = lambda a, sinks=SINKS, window=8, count=4, cu=CU: lib.sfa_decode_varlen_window_sinks(ref(a), sinks, cu, count,
                                                                                                 0, window, None)
    return ((NAMES[0], one, lambda B, H, Hkv, D, M, n, W, S: lib.sfa_decode_window_workspace_bytes(B, H, Hkv, D, M, W, S)),
            (NAMES[1], chunk, lib.sfa_decode_chunk_window_workspace_bytes),
            (NAMES[2], varlen, lib.sfa_decode_varlen_window_workspace_bytes))


@pytest.mark.skipif(torch.cuda.is_available(), reason="calls the entry points with fake device pointers")
@pytest.mark.parametrize("which", [0, 1, 2])
def test_sinks_argument_validation_without_gpu(lib, which):
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
    a.head_dim, a.rotary_embedding_dim = 256, 128
    if which:                                                   # the multi-token calls do not serve head_dim 256
        assert call(a) == -4 and err().startswith(fn) and b"256" in err()
    else:                                                       # the single-token call does: it gets past validation
        assert call(a) == -1 and err().startswith(fn + b" workspace is NULL")
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
    if which == 2:
        assert call(a, cu=None) == -1 and err().startswith(fn) and b"cu_tokens" in err()
        assert call(a, cu=CU + 2) == -2 and err().startswith(fn) and b"cu_tokens" in err()
    # a well-formed call, with sinks, without (NULL), and with the largest window, gets as far as the workspace
    for kw in ({}, {"sinks": None}, {"window": 2 ** 31 - 1}):
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

def _single_token_problem(dtype, D, G, seed):
    rng = np.random.default_rng(seed)
    B, Hkv, L, M = 4, 2, 2, 160
    H = G * Hkv
    rt = lambda *s: cw.round_to(rng.standard_normal(s), dtype).astype(np.float32)
    qkv = rt(B, H + 2 * Hkv, D)
    return dict(q=qkv[:, :H], k=qkv[:, H:H + Hkv], v=qkv[:, H + Hkv:], kc=rt(B, L, M, Hkv, D), vc=rt(B, L, M, Hkv, D),
                lens=(0, 5, 130, 77), bias=dict(q_bias=rt(H, D), k_bias=rt(Hkv, D), v_bias=rt(Hkv, D)), H=H)


@pytest.mark.parametrize("dtype,D,G,window,anchor", [("fp16", 64, 8, 33, 0), ("bf16", 128, 1, 5000, 2), ("bf16", 64, 4, 1, 1),
                                                     ("fp16", 128, 2, 100, 3)])
def test_single_token_reference_properties(dtype, D, G, window, anchor):
    pr = _single_token_problem(dtype, D, G, [21, D, G])
    args = (pr["q"], pr["k"], pr["v"], pr["kc"], pr["vc"], pr["lens"], 1, D // 2, window)
    plain = decode_window_ref(*args, dtype, **pr["bias"])
    none = sinks_ref.decode_window_sinks_ref(*args, None, dtype, **pr["bias"])
    ninf = sinks_ref.decode_window_sinks_ref(*args, np.full(pr["H"], -np.inf), dtype, **pr["bias"])
    for r in (none, ninf):                      # all sinks -inf: the windowed reference, exactly
        for key in ("o", "k_row", "v_row"):
            np.testing.assert_array_equal(r[key], plain[key])
    delta = sinks_ref.deltas(pr["H"])
    sinks = sinks_ref.make_sinks(none["lse"][anchor])
    got = sinks_ref.decode_window_sinks_ref(*args, sinks, dtype, **pr["bias"])
    np.testing.assert_array_equal(got["lse"], none["lse"])
    # o_sinks = o_window * sum / (sum + exp(sink)) = o_window * sigmoid(lse - sink), on the references' fp64 outputs
    share = sinks_ref.sigmoid(sinks[None, :] - none["lse"])                     # the sink's share of each row
    want = none["o64"] * sinks_ref.sigmoid(none["lse"] - sinks[None, :])[:, :, None]
    assert np.abs(got["o64"] - want).max() <= 1e-12
    np.testing.assert_array_equal(got["o"], got["o64"].astype(np.float32))
    assert np.abs(share[anchor] - sinks_ref.sigmoid(delta)).max() <= 1e-12
    assert share[anchor].min() > 0.047 and share[anchor].max() < 0.953 and len(set(np.round(share[anchor], 6))) == pr["H"]


@pytest.mark.parametrize("dtype,D,G,n,window,anchor", [("bf16", 64, 8, 9, 33, 3), ("fp16", 128, 1, 40, 17, 0),
                                                       ("fp16", 64, 16, 5, 5000, 2), ("bf16", 128, 2, 3, 2, 1)])
def test_chunk_reference_properties(dtype, D, G, n, window, anchor):
    prob = cw.problem(dtype, D, G, n)
    H = prob.H
    plain = cw.chunk_window_ref(prob, window)
    none = sinks_ref.chunk_sinks_ref(prob, window, None)
    ninf = sinks_ref.chunk_sinks_ref(prob, window, np.full(H, -np.inf))
    for r in (none, ninf):
        for b in range(prob.B):
            for i in range(3):
                np.testing.assert_array_equal(r[b][i], plain[b][i])
    delta = sinks_ref.deltas(H)
    sinks = sinks_ref.make_sinks(none[anchor][3][0])            # token 0 of the anchor sequence
    got = sinks_ref.chunk_sinks_ref(prob, window, sinks)
    for b in range(prob.B):                                     # o_sinks == o_window * sigmoid(lse - sink), in fp64
        want = none[b][4] * sinks_ref.sigmoid(none[b][3] - sinks[None, :])[:, :, None]
        assert np.abs(got[b][4] - want).max() <= 1e-12
        np.testing.assert_array_equal(got[b][3], none[b][3])
    share = sinks_ref.sigmoid(sinks - none[anchor][3][0])
    assert np.abs(share - sinks_ref.sigmoid(delta)).max() <= 1e-12
    # a ragged batch: the varlen reference gives every sequence's tokens what the chunk reference gives them
    ns = (3, 0, n, 1)
    ragged = cw.make_problem(dtype, D, G, prob.lens, ns, qkv=prob.qkv, kc=prob.kc, vc=prob.vc)
    ragged.qb, ragged.kb, ragged.vb = prob.qb, prob.kb, prob.vb
    rv = sinks_ref.varlen_sinks_ref(ragged, window, sinks)
    for b, nb in enumerate(ns):
        assert rv[b][0].shape[0] == nb
        if nb == 0:
            continue
        assert np.abs(rv[b][4] - got[b][4][:nb]).max() <= 1e-12
        assert np.abs(rv[b][3] - got[b][3][:nb]).max() <= 1e-12
        np.testing.assert_array_equal(rv[b][1], got[b][1][:nb])


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
    (dtype, D, PAGED); decode_window*_kernel<Tr, D, NT, KLDS, PAGED>: (dtype, D, NT, KLDS, PAGED) -- or None"""
    if kernel not in mangled:
        return None
    m = re.search(r"(Fp16|Bf16)ELi(\d+)((?:ELb[01])+)E", mangled)
    return (m.group(1), int(m.group(2))) + tuple(int(x) for x in re.findall(r"ELb([01])", m.group(3)))


@pytest.mark.parametrize("new,twin,count,kernel,new_kernel,marks", [
    ("decode_window_sinks_kernel.hip", "decode_window_kernel.hip", 36, "decode_window_kernel", "decode_window_sinks_kernel",
     ()),
    ("decode_chunk_window_sinks_kernel.hip", "decode_chunk_window_kernel.hip", 20, "chunk_attn_kernel", "chunk_attn_kernel",
     ("WindowSinkGeo", "UniformGeo")),
    ("decode_varlen_window_sinks_kernel.hip", "decode_varlen_window_kernel.hip", 21, "chunk_attn_kernel", "chunk_attn_kernel",
     ("WindowSinkGeo", "RaggedGeo")),
])
def test_sinks_kernels_compile_without_scratch_at_the_twins_occupancy(tmp_path, new, twin, count, kernel, new_kernel, marks):
    """Every kernel of a new translation unit compiles for gfx950 with no spill to scratch, and each attention kernel has
    the occupancy and the LDS size of its _window twin's kernel of the same template arguments.  The VGPR counts are
    printed, not pinned."""
    mine = _remarks(new, tmp_path, "sinks")
    assert len(mine) == count, sorted(mine)
    assert all(v["ScratchSize [bytes/lane]"] == 0 for v in mine.values()), mine
    by_inst = {_instantiation(nm, kernel): v for nm, v in _remarks(twin, tmp_path, "twin").items()}
    by_inst.pop(None, None)
    n_attn = 36 if count == 36 else 8
    assert len(by_inst) == n_attn
    seen = 0
    for nm, v in mine.items():
        inst = _instantiation(nm, new_kernel)
        if inst is None:
            continue
        assert all(m in nm for m in marks)
        seen += 1
        print(inst, "sinks VGPRs", v["VGPRs"], "window VGPRs", by_inst[inst]["VGPRs"], "occupancy",
              v["Occupancy [waves/SIMD]"])
        assert v["Occupancy [waves/SIMD]"] == by_inst[inst]["Occupancy [waves/SIMD]"], (inst, v, by_inst[inst])
        assert v["LDS Size [bytes/block]"] == by_inst[inst]["LDS Size [bytes/block]"], (inst, v, by_inst[inst])
    assert seen == n_attn
