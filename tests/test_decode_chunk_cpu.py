"""CPU-only checks of sfa_decode_chunk (n new tokens per sequence): the symbols and the Python operator exist, the
entry point validates its arguments before any HIP call, the workspace arithmetic, and the kernel translation unit
compiles for gfx950 without scratch."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from conftest import ROOT
from starflashattention_amd import _lib

KERNEL = os.path.join(ROOT, "starflashattention_amd", "csrc", "decode_chunk_kernel.hip")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def test_chunk_symbols_exported(lib):
    for name in ("sfa_decode_chunk", "sfa_decode_chunk_workspace_bytes"):
        assert name in _lib.EXPORTED_SYMBOLS
        assert hasattr(lib, name)
    import starflashattention_amd as sfa
    from starflashattention_amd.ops import flash_decode_chunk
    assert sfa.flash_decode_chunk is flash_decode_chunk


def _args():
    a = _lib.DecodeArgs()
    for f in ("qkv", "o", "seq_len", "k_cache_table", "v_cache_table"):
        setattr(a, f, 0x1000)
    a.batch_size, a.num_heads, a.memory_max_len, a.num_layer, a.head_dim = 1, 2, 64, 1, 128
    a.rotary_embedding_dim = 128
    return a


@pytest.mark.skipif(torch.cuda.is_available(), reason="calls sfa_decode_chunk with fake device pointers")
def test_chunk_argument_validation_without_gpu(lib):
    call = lambda a, n=4, ts=0: lib.sfa_decode_chunk(ctypes.byref(a), n, ts, None)
    assert call(_lib.DecodeArgs()) == -1                        # null pointers
    assert b"sfa_decode_chunk" in lib.sfa_last_error()
    a = _args()
    assert call(a, n=-1) == -2 and b"num_tokens" in lib.sfa_last_error()
    a.head_dim = 96
    assert call(a) == -4
    a.head_dim = 256
    assert call(a) == -4 and b"chunk path" in lib.sfa_last_error()
    a.head_dim = 128
    a.num_heads, a.num_heads_kv = 12, 4                         # group of 3
    assert call(a) == -2 and b"num_heads_kv" in lib.sfa_last_error()
    a.num_heads, a.num_heads_kv = 8, 4
    assert call(a, ts=100) == -2 and b"token_stride" in lib.sfa_last_error()   # < (H + 2*Hkv)*D
    a.kv_layout = _lib.KV_LAYOUTS["paged"]
    assert call(a) == -1 and b"block_table" in lib.sfa_last_error()
    a.block_table, a.page_size, a.num_pages, a.block_table_stride = 0x3000, 8, 4, 4
    assert call(a) == -2 and b"page_size" in lib.sfa_last_error()
    a.page_size, a.block_table_stride = 16, 3                   # 3 * 16 < memory_max_len 64
    assert call(a) == -2 and b"cover memory_max_len" in lib.sfa_last_error()
    a.block_table_stride = 4
    assert call(a) == -1 and b"workspace" in lib.sfa_last_error()
    a.workspace, a.workspace_bytes = 0x2000, 256
    assert call(a) == -5                                        # workspace too small
    assert call(a, n=0) == 0                                    # nothing to do
    a.workspace_bytes = lib.sfa_decode_chunk_workspace_bytes(1, 8, 4, 128, 64, 4, 0) - 1
    assert call(a) == -5


def test_chunk_workspace_arithmetic(lib):
    ws = lib.sfa_decode_chunk_workspace_bytes
    # grows with n
    sizes = [ws(2, 32, 8, 128, 4096, n, 0) for n in (1, 4, 64, 512)]
    assert sizes == sorted(sizes) and len(set(sizes)) == 4
    # the rotated Q follows the status block: 256 + B*H*n*D*2 bytes (rounded to 256) for one split
    assert ws(4, 32, 32, 128, 4096, 2048, 1) == 256 + 4 * 32 * 2048 * 128 * 2
    # a single split with n = 1 needs no partials
    assert ws(1, 8, 8, 64, 1024, 1, 1) == 256 + 8 * 64 * 2
    # num_splits = 0 is the size at the library's own choice, which splits small problems
    for shape in ((1, 32, 32, 128, 8192, 4), (2, 32, 4, 128, 8192, 16), (64, 32, 32, 128, 4096, 8)):
        B, H, Hkv, D, M, n = shape
        auto = ws(B, H, Hkv, D, M, n, 0)
        sized = {s: ws(B, H, Hkv, D, M, n, s) for s in range(1, 33)}
        assert auto in sized.values(), shape
        s_auto = min(s for s, v in sized.items() if v == auto)
        if B * Hkv >= 256:
            assert s_auto == 1, shape
        else:
            assert s_auto > 1, shape
            rows = n * (H // Hkv)
            assert auto == 256 + B * Hkv * rows * D * 2 + B * Hkv * s_auto * rows * (D * 4 + 8), shape


def test_chunk_kernel_compiles_without_scratch(tmp_path):
    """Every kernel of the chunk translation unit compiles for gfx950 with no spill to scratch."""
    r = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", f"--offload-arch=gfx950", "-I" + ROOT,
                        "-Rpass-analysis=kernel-resource-usage", "-c", KERNEL, "-o", str(tmp_path / "k.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    assert len(names) == len(scratch) == 20, (names, scratch)       # (prologue + attention) x 8 + combine x 4
    assert all(s == 0 for s in scratch), list(zip(names, scratch))
    assert sum("chunk_attn_kernel" in nm for nm in names) == 8


def test_chunk_sources_have_no_scalar_memory_writes():
    """No kernel source of the chunk path holds a scalar-unit store, atomic or cache write-back, in any letter case.
    The word list lives in a text document (tests/scalar_memory_writes.txt) so that no source file holds it."""
    with open(os.path.join(ROOT, "tests", "scalar_memory_writes.txt")) as f:
        words = [w.strip() for w in f if w.strip() and not w.startswith("#")]
    assert len(words) >= 5
    for fn in ("decode_chunk_kernel.hip", "decode_chunk_common.h"):
        txt = open(os.path.join(ROOT, "starflashattention_amd", "csrc", fn)).read().lower()
        for w in words:
            assert w not in txt, (fn, w)
