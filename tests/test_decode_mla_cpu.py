"""CPU-only checks of sfa_decode_mla (latent-attention decode): the symbols and the operator exist beside ABI version 4,
the ctypes mirror matches the header, the workspace size is the documented formula, and the entry point validates its
arguments before any HIP call."""
import ctypes
import os
import re

import pytest

from conftest import ROOT
from starflashattention_amd import _lib


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def _header():
    with open(os.path.join(ROOT, "include", "star_flash_attn.h")) as f:
        return f.read()


def test_mla_symbols_exported(lib):
    header = _header()
    for name in ("sfa_decode_mla", "sfa_decode_mla_workspace_bytes", "sfa_decode_mla_auto_splits"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name) and name + "(" in header
    import starflashattention_amd as sfa
    from starflashattention_amd import ops
    assert sfa.flash_decode_mla is ops.flash_decode_mla
    assert sfa.decode_mla_workspace_bytes is ops.decode_mla_workspace_bytes
    assert sfa.decode_mla_auto_splits is ops.decode_mla_auto_splits
    assert "#define SFA_ABI_VERSION 4" in header and lib.sfa_abi_version() == 4


def test_mla_args_mirror_the_header():
    body = re.search(r"typedef struct sfa_mla_decode_args \{(.*?)\} sfa_mla_decode_args;", _header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    ctype = {"int": ctypes.c_int, "float": ctypes.c_float, "size_t": ctypes.c_size_t}
    fields = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        kind, name = decl.rsplit(None, 1)
        fields.append((name.lstrip("*"), ctypes.c_void_p if name.startswith("*") else ctype[kind]))
    assert fields == list(_lib.MlaDecodeArgs._fields_)


@pytest.mark.parametrize("B,H,S", [(3, 16, 3), (1, 48, 5), (3, 80, 3)])     # B*H*S*8 is no multiple of 256
def test_mla_workspace_bytes_formula(lib, B, H, S):
    al = lambda x: (x + 255) // 256 * 256
    assert (B * H * S * 8) % 256
    assert lib.sfa_decode_mla_workspace_bytes(B, H, 4096, S) == 256 + al(B * H * S * 512 * 4) + al(B * H * S * 8)
    assert lib.sfa_decode_mla_workspace_bytes(B, H, 4096, 1) == 256
    auto = lib.sfa_decode_mla_auto_splits(B, H, 4096)
    assert 1 <= auto <= 32
    assert lib.sfa_decode_mla_workspace_bytes(B, H, 4096, 0) == lib.sfa_decode_mla_workspace_bytes(B, H, 4096, auto)


def _args(lib):
    a = _lib.MlaDecodeArgs()
    for f in ("q", "kv_new", "o", "seq_len", "kv_cache"):
        setattr(a, f, 0x1000)
    a.batch_size, a.num_heads, a.memory_max_len, a.num_layer, a.num_splits = 2, 32, 256, 2, 3
    a.workspace, a.workspace_bytes = 0x10000, lib.sfa_decode_mla_workspace_bytes(2, 32, 256, 3)
    return a


def _paged(a, page_size):
    a.kv_layout, a.page_size, a.block_table, a.block_table_stride, a.num_pages = 2, page_size, 0x3000, 16, 64


VALIDATION = {          # case: (what breaks a good call, status)
    "null_q": (lambda a: setattr(a, "q", None), -1),
    "dtype_7": (lambda a: setattr(a, "dtype", 7), -3),
    "heads_8": (lambda a: setattr(a, "num_heads", 8), -2),
    "heads_24": (lambda a: setattr(a, "num_heads", 24), -2),
    "heads_144": (lambda a: setattr(a, "num_heads", 144), -2),
    "layout_blhmd": (lambda a: setattr(a, "kv_layout", 1), -2),
    "page_size_24": (lambda a: _paged(a, 24), -2),
    "workspace_misaligned": (lambda a: setattr(a, "workspace", 0x10010), -2),
    "workspace_one_byte_short": (lambda a: setattr(a, "workspace_bytes", a.workspace_bytes - 1), -5),
}


@pytest.mark.parametrize("case", sorted(VALIDATION))
def test_mla_argument_validation(lib, case):
    """Fake device pointers: every case is refused before any HIP call."""
    a = _args(lib)
    spoil, status = VALIDATION[case]
    spoil(a)
    assert lib.sfa_decode_mla(ctypes.byref(a), None) == status
    assert lib.sfa_last_error().startswith(b"sfa_decode_mla: ")
