"""CPU-only checks of sfa_decode_chunk_kv8 / sfa_decode_varlen_kv8 (the multi-token decode calls over an fp8 KV cache):
the symbols and the Python operators exist beside an unchanged sfa_decode_args and ABI version, both entry points validate
their arguments before any HIP call, the reference of tests/chunk_kv8_ref.py gives what kv8_ref.decode_kv8_ref gives token
by token, and the two new translation units compile for gfx950 without scratch at the occupancy of their 16-bit twins."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT
from starflashattention_amd import _lib
import chunk_kv8_ref
import kv8_ref
from oracle import rotary_table_ref, round_to

CSRC = os.path.join(ROOT, "starflashattention_amd", "csrc")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def test_chunk_kv8_symbols_exported(lib):
    for name in ("sfa_decode_chunk_kv8", "sfa_decode_varlen_kv8"):
        assert name in _lib.EXPORTED_SYMBOLS
        assert hasattr(lib, name)
    import starflashattention_amd as sfa
    from starflashattention_amd.ops import flash_decode_chunk_kv8, flash_decode_varlen_kv8
    assert sfa.flash_decode_chunk_kv8 is flash_decode_chunk_kv8 and sfa.flash_decode_varlen_kv8 is flash_decode_varlen_kv8
    with open(os.path.join(ROOT, "include", "star_flash_attn.h")) as f:
        header = f.read()
    assert "sfa_decode_chunk_kv8(" in header and "sfa_decode_varlen_kv8(" in header
    # new symbols beside the same struct and the same ABI version, and no sizing functions of their own
    assert lib.sfa_abi_version() == 4 and "#define SFA_ABI_VERSION 4" in header
    assert ctypes.sizeof(_lib.DecodeArgs) == 10 * 8 + 12 * 4 + 8 + 8 + 8 + 8 + 8 + 8
    assert "kv8_workspace_bytes" not in header and not any("kv8_workspace" in s for s in _lib.EXPORTED_SYMBOLS)


def _args():
    a = _lib.DecodeArgs()
    for f in ("qkv", "o", "seq_len", "k_cache_table", "v_cache_table"):
        setattr(a, f, 0x1000)
    a.batch_size, a.num_heads, a.memory_max_len, a.num_layer, a.head_dim = 1, 2, 64, 1, 128
    a.rotary_embedding_dim = 128
    return a


CU = 0x4000


def _callers(lib):
    """(name, call(a, ks, vs, count, ts, cu), sizing function) of the two entry points"""
    ref = lambda a: ctypes.byref(a) if a is not None else None
    chunk = lambda a, ks=None, vs=None, count=4, ts=0, cu=CU: lib.sfa_decode_chunk_kv8(ref(a), ks, vs, count, ts, None)
    varlen = lambda a, ks=None, vs=None, count=4, ts=0, cu=CU: lib.sfa_decode_varlen_kv8(ref(a), ks, vs, cu, count, ts, None)
    return (("sfa_decode_chunk_kv8", chunk, lib.sfa_decode_chunk_workspace_bytes),
            ("sfa_decode_varlen_kv8", varlen, lib.sfa_decode_varlen_workspace_bytes))


@pytest.mark.skipif(torch.cuda.is_available(), reason="calls the entry points with fake device pointers")
@pytest.mark.parametrize("which", [0, 1])
def test_chunk_kv8_argument_validation_without_gpu(lib, which):
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
    assert call(a) == -4 and err().startswith(fn) and b"256" in err()
    a.head_dim = 128
    a.dtype = 7
    assert call(a) == -3 and err().startswith(fn)
    a.dtype = 1
    a.num_heads, a.num_heads_kv = 12, 4                         # group of 3
    assert call(a) == -2 and err().startswith(fn) and b"num_heads_kv" in err()
    a.num_heads, a.num_heads_kv = 16, 1                         # every group up to 16 is served
    assert call(a, ks=0x5002) == -2 and err().startswith(fn) and b"k_scale" in err()
    assert call(a, ks=0x5000, vs=0x6001) == -2 and err().startswith(fn) and b"v_scale" in err()
    a.k_cache_table = 0x1008                                    # the byte caches are 16-byte aligned too
    assert call(a) == -2 and err().startswith(fn) and b"16-byte aligned" in err()
    a.k_cache_table = 0x1000
    assert call(a, count=-1) == -2 and err().startswith(fn) and (b"total_tokens" if which else b"num_tokens") in err()
    assert call(a, ts=100) == -2 and err().startswith(fn) and b"token_stride" in err()
    if which:
        a.stride = 18 * 128
        assert call(a) == -2 and err().startswith(fn) and b"stride" in err()
        a.stride = 0
        assert call(a, cu=None) == -1 and err().startswith(fn) and b"cu_tokens" in err()
        assert call(a, cu=0x4002) == -2 and err().startswith(fn) and b"cu_tokens" in err()
    # a well-formed call, with and without scales, gets as far as the workspace
    assert call(a) == -1 and err().startswith(fn + b" workspace is NULL")
    assert call(a, ks=0x5000, vs=0x6000) == -1 and err().startswith(fn + b" workspace is NULL")
    a.workspace, a.workspace_bytes, a.num_splits = 0x2000, 256, 2
    assert call(a) == -5 and err().startswith(fn)               # the 16-bit call's workspace: too small
    a.workspace_bytes = sizing(1, 16, 1, 128, 64, 4, 2) - 1
    assert call(a) == -5 and err().startswith(fn)               # one byte short of that call's sizing function
    assert call(a, count=0) == 0                                # nothing to do
    a.batch_size = 0
    assert call(a) == 0


@pytest.mark.parametrize("seed,dtype,D,G,counts,rot,extras", [
    (1, "bf16", 128, 4, [5, 5], None, False),
    (2, "fp16", 64, 1, [3, 0, 7], 32, True),
    (3, "bf16", 64, 8, [1, 9], None, True),
])
def test_chunk_kv8_ref_equals_the_step_by_step_reference(seed, dtype, D, G, counts, rot, extras):
    """chunk_kv8_ref (append all rows, then attend with a limit per token) against n applications of
    kv8_ref.decode_kv8_ref, which appends and attends one token at a time: identical bytes, o to 1e-12."""
    Hkv = 2
    pr = chunk_kv8_ref.make_problem(seed, counts, Hkv, G, D, dtype, scale_factors=[0.7, 1.9])
    rng = np.random.default_rng(seed + 100)
    lens = [int(x) for x in rng.integers(0, 40, size=len(counts))]
    rd = D if rot is None else rot
    kw = {}
    if extras:
        kw = dict(q_bias=round_to(rng.standard_normal((pr["H"], D)) * 0.5, dtype),
                  k_bias=round_to(rng.standard_normal((Hkv, D)) * 0.5, dtype),
                  v_bias=round_to(rng.standard_normal((Hkv, D)) * 0.5, dtype), scale=0.05)
        kw["cos_table"], kw["sin_table"] = rotary_table_ref(chunk_kv8_ref.M, rd, dtype)
    k_a, v_a = pr["k8"].copy(), pr["v8"].copy()
    got = chunk_kv8_ref.chunk_kv8_ref(pr["tok"], k_a, v_a, lens, chunk_kv8_ref.LAYER, rd, dtype, pr["ks"], pr["vs"], **kw)
    k_b, v_b = pr["k8"].copy(), pr["v8"].copy()
    for b, n in enumerate(counts):
        for t in range(n):
            one = kv8_ref.decode_kv8_ref(pr["tok"][b][t][None], k_b[b:b + 1], v_b[b:b + 1], [lens[b] + t],
                                         chunk_kv8_ref.LAYER, rd, dtype, pr["ks"], pr["vs"], **kw)
            assert np.abs(got["o"][b][t].astype(np.float32) - one["o"][0]).max() <= 1e-12
            assert np.abs(got["o"][b][t] - one["o"][0]).max() <= 1e-6      # (decode_kv8_ref returns fp32)
    np.testing.assert_array_equal(k_a, k_b)
    np.testing.assert_array_equal(v_a, v_b)
    assert not np.array_equal(k_a, pr["k8"])


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
    """(dtype, D, PAGED) of a mangled chunk_*_kernel<GEO, Tr, D, PAGED> name, or None for another kernel."""
    if kernel not in mangled:
        return None
    m = re.search(r"(Fp16|Bf16)ELi(\d+)ELb([01])E", mangled)
    return (m.group(1), int(m.group(2)), int(m.group(3)))


@pytest.mark.parametrize("new,twin,count,geo", [
    ("decode_chunk_kv8_kernel.hip", "decode_chunk_kernel.hip", 20, "UniformGeo"),
    ("decode_varlen_kv8_kernel.hip", "decode_varlen_kernel.hip", 21, "RaggedGeo"),
])
def test_chunk_kv8_kernels_compile_without_scratch_at_the_16_bit_occupancy(tmp_path, new, twin, count, geo):
    """Every kernel of a new translation unit compiles for gfx950 with no spill to scratch, and each fp8 attention
    kernel has the occupancy of the 16-bit chunk_attn_kernel of the same <dtype, D, PAGED>.  The VGPR counts are printed,
    not pinned."""
    fp8 = _remarks(new, tmp_path, "kv8")
    # (prologue + attention) x 8 + combine x 4, and the plan kernel of the ragged call
    assert len(fp8) == count, sorted(fp8)
    assert all(v["ScratchSize [bytes/lane]"] == 0 for v in fp8.values()), fp8
    assert sum("varlen_plan_kernel" in nm for nm in fp8) == count - 20
    assert sum("chunk_prologue_kernel" in nm for nm in fp8) == 8 and sum("chunk_combine_kernel" in nm for nm in fp8) == 4
    by_inst = {_instantiation(nm, "chunk_attn_kernel"): v for nm, v in _remarks(twin, tmp_path, "twin").items()}
    by_inst.pop(None)
    assert len(by_inst) == 8
    seen = 0
    for nm, v in fp8.items():
        inst = _instantiation(nm, "chunk_attn_kernel")
        if inst is None:
            continue
        assert "Kv8Geo" in nm and geo in nm
        seen += 1
        print(inst, "fp8 VGPRs", v["VGPRs"], "16-bit VGPRs", by_inst[inst]["VGPRs"], "occupancy", v["Occupancy [waves/SIMD]"])
        assert v["Occupancy [waves/SIMD]"] == by_inst[inst]["Occupancy [waves/SIMD]"], (inst, v, by_inst[inst])
        assert v["LDS Size [bytes/block]"] == by_inst[inst]["LDS Size [bytes/block]"], (inst, v, by_inst[inst])
    assert seen == 8
