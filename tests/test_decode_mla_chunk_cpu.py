"""CPU-only checks of sfa_decode_mla_chunk (n new tokens per sequence of latent-attention decode): the symbols and the
operators exist, num_tokens is validated before any HIP call, and the workspace size is the documented formula."""
import ctypes
import os

import pytest

from conftest import ROOT
from starflashattention_amd import _lib


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def _args(lib, n):
    """a good call on fake device pointers: anything that is not refused would reach HIP"""
    a = _lib.MlaDecodeArgs()
    for f in ("q", "kv_new", "o", "seq_len", "kv_cache"):
        setattr(a, f, 0x1000)
    a.batch_size, a.num_heads, a.memory_max_len, a.num_layer, a.num_splits = 2, 32, 256, 2, 3
    a.workspace, a.workspace_bytes = 0x10000, lib.sfa_decode_mla_chunk_workspace_bytes(2, 32, 256, max(n, 1), 3)
    return a


def test_mla_chunk_symbols_exported(lib):
    with open(os.path.join(ROOT, "include", "star_flash_attn.h")) as f:
        header = f.read()
    for name in ("sfa_decode_mla_chunk", "sfa_decode_mla_chunk_workspace_bytes", "sfa_decode_mla_chunk_auto_splits"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name) and name + "(" in header
    import starflashattention_amd as sfa
    from starflashattention_amd import ops
    assert sfa.flash_decode_mla_chunk is ops.flash_decode_mla_chunk
    assert sfa.decode_mla_chunk_workspace_bytes is ops.decode_mla_chunk_workspace_bytes
    assert sfa.decode_mla_chunk_auto_splits is ops.decode_mla_chunk_auto_splits


@pytest.mark.parametrize("n", [-1, 33])
def test_mla_chunk_num_tokens_out_of_range(lib, n):
    assert lib.sfa_decode_mla_chunk(ctypes.byref(_args(lib, n)), n, None) == -2        # SFA_ERR_BAD_SHAPE
    assert lib.sfa_last_error().startswith(b"sfa_decode_mla_chunk: ")


def test_mla_chunk_zero_tokens_does_nothing(lib):
    assert lib.sfa_decode_mla_chunk(ctypes.byref(_args(lib, 0)), 0, None) == 0          # SFA_OK, no launch


def test_mla_chunk_shares_the_validator(lib):
    a = _args(lib, 4)
    a.num_heads = 24
    assert lib.sfa_decode_mla_chunk(ctypes.byref(a), 4, None) == -2
    assert lib.sfa_last_error().startswith(b"sfa_decode_mla_chunk: num_heads=24")
    a = _args(lib, 4)
    a.workspace_bytes -= 1
    assert lib.sfa_decode_mla_chunk(ctypes.byref(a), 4, None) == -5                     # SFA_ERR_WORKSPACE_TOO_SMALL


@pytest.mark.parametrize("B,H,n,S", [(3, 16, 1, 3), (1, 48, 3, 5), (3, 80, 17, 3), (2, 128, 32, 2)])
def test_mla_chunk_workspace_bytes_formula(lib, B, H, n, S):
    al = lambda x: (x + 255) // 256 * 256
    ws = lib.sfa_decode_mla_chunk_workspace_bytes
    assert ws(B, H, 4096, n, S) == 256 + al(B * n * H * S * 512 * 4) + al(B * n * H * S * 8)
    assert ws(B, H, 4096, n, 1) == 256
    auto = lib.sfa_decode_mla_chunk_auto_splits(B, H, 4096, n)
    assert 1 <= auto <= 32 and ws(B, H, 4096, n, 0) == ws(B, H, 4096, n, auto)
    assert ws(B, H, 4096, 1, S) == lib.sfa_decode_mla_workspace_bytes(B, H, 4096, S)


@pytest.mark.parametrize("bad", [(0, 16, 4096, 4), (4, 0, 4096, 4), (4, 16, 0, 4), (4, 16, 4096, 0), (4, 16, 4096, -3)])
def test_mla_chunk_auto_splits_of_nothing_is_one(lib, bad):
    assert lib.sfa_decode_mla_chunk_auto_splits(*bad) == 1
