"""CPU-only checks of sfa_decode_kv8 / sfa_kv8_quantize (decode attention over an fp8 KV cache): the symbols and the
Python operators exist beside an unchanged sfa_decode_args and ABI version, the entry points validate their arguments
before any HIP call, the reference quantiser of tests/kv8_ref.py agrees with torch's float8_e4m3fn conversion, and the
kernel translation unit compiles for gfx950 without scratch."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT
from starflashattention_amd import _lib
import kv8_ref

KERNEL = os.path.join(ROOT, "starflashattention_amd", "csrc", "decode_kv8_kernel.hip")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def test_kv8_symbols_exported(lib):
    for name in ("sfa_decode_kv8", "sfa_kv8_quantize"):
        assert name in _lib.EXPORTED_SYMBOLS
        assert hasattr(lib, name)
    import starflashattention_amd as sfa
    from starflashattention_amd.ops import flash_decode_kv8, quantize_kv8
    assert sfa.flash_decode_kv8 is flash_decode_kv8 and sfa.quantize_kv8 is quantize_kv8
    with open(os.path.join(ROOT, "include", "star_flash_attn.h")) as f:
        header = f.read()
    assert "sfa_decode_kv8(" in header and "sfa_kv8_quantize(" in header
    # new symbols beside the same struct and the same ABI version
    assert lib.sfa_abi_version() == 4
    assert ctypes.sizeof(_lib.DecodeArgs) == 10 * 8 + 12 * 4 + 8 + 8 + 8 + 8 + 8 + 8


def _args():
    a = _lib.DecodeArgs()
    for f in ("qkv", "o", "seq_len", "k_cache_table", "v_cache_table"):
        setattr(a, f, 0x1000)
    a.batch_size, a.num_heads, a.memory_max_len, a.num_layer, a.head_dim = 1, 2, 64, 1, 128
    a.rotary_embedding_dim = 128
    return a


@pytest.mark.skipif(torch.cuda.is_available(), reason="calls sfa_decode_kv8 with fake device pointers")
def test_decode_kv8_argument_validation_without_gpu(lib):
    call = lambda a, ks=None, vs=None: lib.sfa_decode_kv8(ctypes.byref(a) if a is not None else None, ks, vs, None)
    err = lambda: lib.sfa_last_error()
    assert call(None) == -1 and err().startswith(b"sfa_decode_kv8:")
    assert call(_lib.DecodeArgs()) == -1 and err().startswith(b"sfa_decode_kv8:")
    a = _args()
    a.k_cache_table = None
    assert call(a) == -1 and err().startswith(b"sfa_decode_kv8:")
    a = _args()
    a.head_dim = 96
    assert call(a) == -4 and err().startswith(b"sfa_decode_kv8:")
    a.head_dim, a.rotary_embedding_dim = 256, 128
    assert call(a) == -4 and err().startswith(b"sfa_decode_kv8:") and b"256" in err()
    a.head_dim = 128
    a.dtype = 7
    assert call(a) == -3 and err().startswith(b"sfa_decode_kv8:")
    a.dtype = 1
    a.num_heads, a.num_heads_kv = 12, 4                         # group of 3
    assert call(a) == -2 and b"num_heads_kv" in err()
    a.num_heads, a.num_heads_kv = 16, 1                         # every group up to 16 is served
    assert call(a, ks=0x5002) == -2 and err().startswith(b"sfa_decode_kv8:") and b"k_scale" in err()
    assert call(a, ks=0x5000, vs=0x6001) == -2 and b"v_scale" in err()
    a.k_cache_table = 0x1008                                    # the byte caches are 16-byte aligned too
    assert call(a) == -2 and b"16-byte aligned" in err()
    a.k_cache_table = 0x1000
    # a well-formed call, with and without scales, gets as far as the workspace
    assert call(a) == -1 and err().startswith(b"sfa_decode_kv8: workspace is NULL")
    assert call(a, ks=0x5000, vs=0x6000) == -1 and err().startswith(b"sfa_decode_kv8: workspace is NULL")
    a.workspace, a.workspace_bytes, a.num_splits = 0x2000, 256, 2
    assert call(a) == -5 and err().startswith(b"sfa_decode_kv8:")      # sfa_decode's workspace: too small for 2 splits
    a.batch_size = 0
    assert call(a) == 0                                         # nothing to do


@pytest.mark.skipif(torch.cuda.is_available(), reason="calls sfa_kv8_quantize with fake device pointers")
def test_kv8_quantize_argument_validation_without_gpu(lib):
    def call(dst=0x1000, src=0x2000, scale=None, rows=4, hkv=2, d=128, st=(256, 128, 256, 128), dtype=1):
        return lib.sfa_kv8_quantize(dst, src, scale, rows, hkv, d, *st, dtype, None)
    err = lambda: lib.sfa_last_error()
    assert call(dst=None) == -1 and err().startswith(b"sfa_kv8_quantize:")
    assert call(src=None) == -1 and err().startswith(b"sfa_kv8_quantize:")
    assert call(rows=-1) == -2 and err().startswith(b"sfa_kv8_quantize:")
    assert call(hkv=0) == -2
    assert call(d=96) == -4 and err().startswith(b"sfa_kv8_quantize:")
    assert call(dtype=7) == -3 and err().startswith(b"sfa_kv8_quantize:")
    assert call(st=(256, 128, 264, 128)) == -2 and b"multiples of 16" in err()    # a stride that is no multiple of 16
    assert call(st=(256, 120, 256, 128)) == -2 and b"multiples of 16" in err()
    assert call(dst=0x1008) == -2 and b"16-byte aligned" in err()
    assert call(scale=0x5002) == -2 and b"scale" in err()
    assert call(rows=0) == 0                                    # nothing to do: no launch


def test_e4m3_table_matches_torch():
    codes = torch.arange(256, dtype=torch.uint8)
    want = codes.view(torch.float8_e4m3fn).float().numpy().astype(np.float64)
    np.testing.assert_array_equal(kv8_ref.E4M3, want)           # NaN at 0x7F / 0xFF on both sides
    assert kv8_ref.E4M3[0x7E] == 448.0 and kv8_ref.E4M3[0x01] == 2.0 ** -9


def test_reference_quantiser_matches_torch_in_range_and_saturates():
    rng = np.random.default_rng(5)
    x = np.concatenate([
        rng.standard_normal(200000).astype(np.float32) * 100,                  # normals, up to the top binades
        rng.standard_normal(100000).astype(np.float32) * 0.01,                 # subnormals and underflow to zero
        kv8_ref.E4M3[:0x7F].astype(np.float32),                                # every code itself ...
        ((kv8_ref.E4M3[:0x7E] + kv8_ref.E4M3[1:0x7F]) / 2).astype(np.float32), # ... and every tie between two codes
        np.array([0.0, -0.0, 448.0, -448.0], np.float32)])
    x = np.concatenate([x, -x])
    x = x[np.abs(x) <= 448.0].reshape(1, -1)
    got = kv8_ref.quantize(x)
    want = torch.from_numpy(x).to(torch.float8_e4m3fn).view(torch.uint8).numpy()
    np.testing.assert_array_equal(got, want)
    # beyond +-448 the contract saturates (torch gives NaN there); NaN stays NaN
    far = np.array([[449.0, 480.0, 1e6, np.inf, -449.0, -1e6, -np.inf, np.nan]], np.float32)
    np.testing.assert_array_equal(kv8_ref.quantize(far)[0], [0x7E] * 4 + [0xFE] * 3 + [0x7F])
    # per-head scales: the division is fp32, then the same rounding
    y = rng.standard_normal((3, 2, 64)).astype(np.float32)
    s = np.array([0.013, 2.5], np.float32)
    np.testing.assert_array_equal(kv8_ref.quantize(y, s), kv8_ref.quantize((y / s[:, None]).astype(np.float32)))
    np.testing.assert_array_equal(kv8_ref.dequantize(kv8_ref.quantize(y, s), s),
                                  kv8_ref.E4M3[kv8_ref.quantize(y, s)] * s.astype(np.float64)[:, None])


def test_kv8_kernel_compiles_without_scratch(tmp_path):
    """Every kernel of the fp8 translation unit compiles for gfx950 with no spill to scratch."""
    r = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-I" + ROOT,
                        "-Rpass-analysis=kernel-resource-usage", "-c", KERNEL, "-o", str(tmp_path / "k.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    # attention: (fp16, bf16) x (64, 128) x (default, non-temporal loads) x (contiguous, paged); quantise: fp16, bf16
    assert len(names) == len(scratch) == 18, (names, scratch)
    assert all(s == 0 for s in scratch), list(zip(names, scratch))
    assert sum("decode_kv8_kernel" in nm for nm in names) == 16
    assert sum("kv8_quantize_kernel" in nm for nm in names) == 2
