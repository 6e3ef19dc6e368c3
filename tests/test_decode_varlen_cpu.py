"""CPU-only checks of sfa_decode_varlen (a ragged, packed batch of new tokens): the symbols and the Python operator
exist, the entry point validates its arguments before any HIP call, the workspace arithmetic, the new translation unit
compiles for gfx950 without scratch, and the ragged attention kernels keep the occupancy of the chunk's."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from conftest import ROOT
from starflashattention_amd import _lib

CSRC = os.path.join(ROOT, "starflashattention_amd", "csrc")
SOURCES = ("decode_varlen_kernel.hip", "decode_chunk_body.h", "decode_chunk_kernel.hip", "decode_chunk_common.h")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def test_varlen_symbols_exported(lib):
    for name in ("sfa_decode_varlen", "sfa_decode_varlen_workspace_bytes"):
        assert name in _lib.EXPORTED_SYMBOLS
        assert hasattr(lib, name)
    import starflashattention_amd as sfa
    from starflashattention_amd.ops import flash_decode_varlen
    assert sfa.flash_decode_varlen is flash_decode_varlen
    with open(os.path.join(ROOT, "include", "star_flash_attn.h")) as f:
        header = f.read()
    assert "sfa_decode_varlen(" in header and "sfa_decode_varlen_workspace_bytes(" in header
    assert lib.sfa_abi_version() == 4                          # new symbols, the same ABI version


def _args():
    a = _lib.DecodeArgs()
    for f in ("qkv", "o", "seq_len", "k_cache_table", "v_cache_table"):
        setattr(a, f, 0x1000)
    a.batch_size, a.num_heads, a.memory_max_len, a.num_layer, a.head_dim = 1, 2, 64, 1, 128
    a.rotary_embedding_dim = 128
    return a


@pytest.mark.skipif(torch.cuda.is_available(), reason="calls sfa_decode_varlen with fake device pointers")
def test_varlen_argument_validation_without_gpu(lib):
    CU = 0x4000
    call = lambda a, cu=CU, total=4, ts=0: lib.sfa_decode_varlen(ctypes.byref(a), cu, total, ts, None)
    assert call(_lib.DecodeArgs()) == -1                        # null pointers
    assert b"sfa_decode_varlen" in lib.sfa_last_error()
    assert lib.sfa_decode_varlen(None, CU, 4, 0, None) == -1 and b"sfa_decode_varlen" in lib.sfa_last_error()
    a = _args()
    assert call(a, cu=None) == -1 and b"cu_tokens" in lib.sfa_last_error()
    assert call(a, total=-1) == -2 and b"total_tokens" in lib.sfa_last_error()
    a.stride = 6 * 128
    assert call(a) == -2 and b"stride" in lib.sfa_last_error() and b"sfa_decode_varlen" in lib.sfa_last_error()
    a.stride = 0
    a.head_dim = 96
    assert call(a) == -4
    a.head_dim = 256
    assert call(a) == -4 and b"sfa_decode_varlen" in lib.sfa_last_error()
    a.head_dim = 128
    a.num_heads, a.num_heads_kv = 12, 4                         # group of 3
    assert call(a) == -2 and b"num_heads_kv" in lib.sfa_last_error()
    a.num_heads, a.num_heads_kv = 8, 4
    assert call(a, ts=100) == -2 and b"token_stride" in lib.sfa_last_error()   # < (H + 2*Hkv)*D
    assert call(a, ts=16 * 128 + 4) == -2 and b"token_stride" in lib.sfa_last_error()   # not a multiple of 8
    a.kv_layout = _lib.KV_LAYOUTS["paged"]
    assert call(a) == -1 and b"block_table" in lib.sfa_last_error()
    a.block_table, a.page_size, a.num_pages, a.block_table_stride = 0x3000, 8, 4, 4
    assert call(a) == -2 and b"page_size" in lib.sfa_last_error()
    a.page_size, a.block_table_stride = 16, 3                   # 3 * 16 < memory_max_len 64
    assert call(a) == -2 and b"cover memory_max_len" in lib.sfa_last_error()
    a.block_table_stride = 4
    assert call(a) == -1 and b"workspace" in lib.sfa_last_error()      # workspace NULL
    a.workspace, a.workspace_bytes = 0x2000, 256
    assert call(a) == -5                                        # workspace too small
    assert call(a, total=0) == 0                                # nothing to do
    a.workspace_bytes = lib.sfa_decode_varlen_workspace_bytes(1, 8, 4, 128, 64, 4, 0) - 1
    assert call(a) == -5 and b"sfa_decode_varlen" in lib.sfa_last_error()      # one byte short


def _up(x):
    return (x + 255) // 256 * 256


def _formula(B, H, Hkv, D, T, S):
    """The layout documented in csrc/sfa_host.h next to VarlenKernelParams."""
    rows = T * (H // Hkv)
    bound = rows // 256 + B
    size = 256 + _up(bound * 8) + _up(Hkv * rows * D * 2)
    if S > 1:
        size += _up(Hkv * S * rows * D * 4) + _up(Hkv * S * rows * 8)
    return size


def test_varlen_workspace_arithmetic(lib):
    ws = lib.sfa_decode_varlen_workspace_bytes
    # linear in total_tokens (multiples of 8192 tokens keep every term a whole number of 256-byte units)
    for S in (1, 4):
        sizes = [ws(16, 32, 8, 128, 4096, k * 8192, S) for k in (1, 2, 3, 4)]
        steps = {b - a for a, b in zip(sizes, sizes[1:])}
        assert len(steps) == 1 and steps.pop() > 0, sizes
    # the size knows the token total only: no argument describes how the tokens are spread over the sequences, and
    # it matches the documented formula whatever the batch is
    for B, T in ((1, 2111), (64, 2111), (256, 4351)):
        assert ws(B, 32, 32, 128, 4096, T, 1) == _formula(B, 32, 32, 128, T, 1)
        assert ws(B, 32, 4, 64, 4096, T, 3) == _formula(B, 32, 4, 64, T, 3)
    # one split needs no partials: status + plan + rotated Q
    assert ws(64, 32, 32, 128, 4096, 2111, 1) == 256 + _up((2111 // 256 + 64) * 8) + 32 * 2111 * 128 * 2
    # num_splits = 0 is the size at the library's own choice: chunk_auto_splits' rule on bound * Hkv workgroups
    for shape in ((1, 32, 32, 128, 8192, 4), (2, 32, 4, 128, 8192, 16), (64, 32, 32, 128, 4096, 2111)):
        B, H, Hkv, D, M, T = shape
        auto = ws(B, H, Hkv, D, M, T, 0)
        wgs = (T * (H // Hkv) // 256 + B) * Hkv
        s_auto = max(1, min(-(-256 // wgs), max(M // 512, 1), 32))
        assert auto == _formula(B, H, Hkv, D, T, s_auto), shape
        assert (s_auto > 1) == (wgs < 256), shape
    assert ws(0, 32, 32, 128, 4096, 16, 0) == 256 and ws(4, 32, 32, 128, 4096, 0, 0) == 256


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


def test_varlen_kernels_compile_without_scratch_at_the_chunk_occupancy(tmp_path):
    """Every kernel of the ragged translation unit compiles for gfx950 with no spill to scratch, and each ragged
    attention kernel has the VGPR count, occupancy and LDS of the chunk_attn_kernel of the same <dtype, D, PAGED>."""
    ragged = _remarks("decode_varlen_kernel.hip", tmp_path, "varlen")
    # plan + (prologue + attention) x 8 + combine x 4
    assert len(ragged) == 21, sorted(ragged)
    assert all(v["ScratchSize [bytes/lane]"] == 0 for v in ragged.values()), ragged
    assert sum("varlen_plan_kernel" in nm for nm in ragged) == 1
    chunk = _remarks("decode_chunk_kernel.hip", tmp_path, "chunk")
    by_inst = {_instantiation(nm, "chunk_attn_kernel"): v for nm, v in chunk.items()}
    by_inst.pop(None)
    assert len(by_inst) == 8
    seen = 0
    for nm, v in ragged.items():
        inst = _instantiation(nm, "chunk_attn_kernel")
        if inst is None:
            continue
        assert "RaggedGeo" in nm
        seen += 1
        print(inst, "ragged", v, "chunk", by_inst[inst])
        assert v["Occupancy [waves/SIMD]"] == by_inst[inst]["Occupancy [waves/SIMD]"], (inst, v, by_inst[inst])
        assert v["VGPRs"] == by_inst[inst]["VGPRs"], (inst, v, by_inst[inst])
        assert v["LDS Size [bytes/block]"] == by_inst[inst]["LDS Size [bytes/block]"], (inst, v, by_inst[inst])
    assert seen == 8


def test_varlen_sources_have_no_scalar_memory_writes():
    """No kernel source of the ragged path holds a scalar-unit store, atomic or cache write-back, in any letter case
    (the word list lives in tests/scalar_memory_writes.txt so that no source file holds it)."""
    with open(os.path.join(ROOT, "tests", "scalar_memory_writes.txt")) as f:
        words = [w.strip() for w in f if w.strip() and not w.startswith("#")]
    assert len(words) >= 5
    for fn in SOURCES:
        txt = open(os.path.join(CSRC, fn)).read().lower()
        for w in words:
            assert w not in txt, (fn, w)


def test_varlen_sources_read_no_environment():
    for fn in SOURCES:
        assert "getenv" not in open(os.path.join(CSRC, fn)).read(), fn
