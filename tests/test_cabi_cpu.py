"""CPU-only checks of the drop-in boundary: the C-ABI library loads, exports every symbol
include/star_flash_attn.h declares, validates its arguments, and the product never routes through
the oracle.  No compute calls (there is no GPU here)."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT
from starflashattention_amd import _lib

HEADER = os.path.join(ROOT, "include", "star_flash_attn.h")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def test_header_symbols_all_exported(lib):
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(sfa_[a-z0-9_]+)\s*\(", text))
    assert declared == set(_lib.EXPORTED_SYMBOLS), declared ^ set(_lib.EXPORTED_SYMBOLS)
    for name in declared:
        assert hasattr(lib, name), f"{name} not exported by {_lib.LIB_PATH}"


def test_struct_layouts_match_header():
    # the ctypes mirrors must match the C structs field for field
    text = open(HEADER).read()
    for cname, cls in (("sfa_decode_args", _lib.DecodeArgs), ("sfa_prefill_args", _lib.PrefillArgs)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), text, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = [re.search(r"(\w+)(\[\d+\])?\s*$", d.strip()).group(1) for d in body.split(";") if d.strip()]
        assert names == [f[0] for f in cls._fields_], cname
    assert ctypes.sizeof(_lib.DecodeArgs) == 10 * 8 + 12 * 4 + 8 + 8 + 8 + 8 + 8 + 8  # + kv_layout, page_size | table | stride, pages | heads_kv
    assert ctypes.sizeof(_lib.PrefillArgs) == 5 * 8 + 6 * 4 + 12 * 8 + 4 * 4


def test_argument_validation_without_gpu(lib):
    assert lib.sfa_abi_version() == 4
    a = _lib.DecodeArgs()
    assert lib.sfa_decode(ctypes.byref(a), None) == -1          # null pointers
    assert b"non-NULL" in lib.sfa_last_error()
    for f in ("qkv", "o", "seq_len", "k_cache_table", "v_cache_table"):
        setattr(a, f, 0x1000)
    a.batch_size, a.num_heads, a.memory_max_len, a.num_layer = 1, 2, 16, 1
    a.head_dim = 96
    assert lib.sfa_decode(ctypes.byref(a), None) == -4          # unsupported head_dim
    a.head_dim = 128
    a.rotary_embedding_dim = 129
    assert lib.sfa_decode(ctypes.byref(a), None) == -2
    a.rotary_embedding_dim = 128
    a.dtype = 7
    assert lib.sfa_decode(ctypes.byref(a), None) == -3
    a.dtype = 0
    a.idx_layer = 1
    assert lib.sfa_decode(ctypes.byref(a), None) == -2          # idx_layer >= num_layer
    a.idx_layer = 0
    assert lib.sfa_decode(ctypes.byref(a), None) == -1          # workspace NULL
    assert b"workspace" in lib.sfa_last_error()
    a.workspace, a.workspace_bytes = 0x2000, 16
    assert lib.sfa_decode(ctypes.byref(a), None) == -5          # workspace too small
    # ABI v2 extensions: cache layouts, paging, grouped queries
    a.kv_layout = 3
    assert lib.sfa_decode(ctypes.byref(a), None) == -2 and b"kv_layout" in lib.sfa_last_error()
    a.kv_layout = _lib.KV_LAYOUTS["paged"]
    assert lib.sfa_decode(ctypes.byref(a), None) == -1 and b"block_table" in lib.sfa_last_error()
    a.block_table, a.page_size, a.num_pages, a.block_table_stride = 0x3000, 8, 4, 2
    assert lib.sfa_decode(ctypes.byref(a), None) == -2 and b"page_size" in lib.sfa_last_error()
    a.page_size, a.block_table_stride = 16, 0
    assert lib.sfa_decode(ctypes.byref(a), None) == -2 and b"cover memory_max_len" in lib.sfa_last_error()
    a.block_table_stride = 1
    assert lib.sfa_decode(ctypes.byref(a), None) == -5          # past the paging checks: workspace again
    a.kv_layout = _lib.KV_LAYOUTS["blhmd"]
    a.num_heads, a.num_heads_kv = 6, 4
    assert lib.sfa_decode(ctypes.byref(a), None) == -2 and b"num_heads_kv" in lib.sfa_last_error()
    a.num_heads, a.num_heads_kv = 12, 4                         # group of 3: not in {1, 2, 4, 8, 16}
    assert lib.sfa_decode(ctypes.byref(a), None) == -2
    a.num_heads, a.num_heads_kv, a.kv_layout = 8, 4, _lib.KV_LAYOUTS["paged"]
    assert lib.sfa_decode(ctypes.byref(a), None) == -5          # grouped queries over a paged cache: accepted
    assert lib.sfa_status_string(-8) == b"block_table entry out of range"
    p = _lib.PrefillArgs()
    assert lib.sfa_prefill_fwd(ctypes.byref(p), None) == -1
    assert lib.sfa_status_string(-7) == b"seq_len out of range"
    # the test / A-B knobs (the launch paths read no environment variable)
    assert lib.sfa_debug_set(b"prefill_impl", 40) == 0 and lib.sfa_debug_set(b"prefill_impl", -1) == 0
    assert lib.sfa_debug_set(b"no_such_knob", 1) == -2 and b"unknown knob" in lib.sfa_last_error()
    assert lib.sfa_debug_set(None, 1) == -1


@pytest.mark.skipif(torch.cuda.is_available(), reason="calls sfa_prefill_fwd with fake device pointers")
def test_prefill_impl_rejects_unknown_ids(lib):
    """prefill_impl ids outside the table of prefill_common.h (the retired generations' 0, 30, 84 among them) and the
    diagnostic builds this library was not compiled with (43, 44) fail before any HIP call."""
    lib.sfa_debug_get.restype = ctypes.c_int
    p = _lib.PrefillArgs()
    p.q, p.k, p.v, p.o = 0x1000, 0x2000, 0x3000, 0x4000
    p.batch, p.heads_q, p.heads_kv, p.seqlen_q, p.seqlen_k, p.head_dim = 1, 1, 1, 1, 1, 128
    for st in (p.q_stride, p.k_stride, p.v_stride, p.o_stride):
        st[0], st[1], st[2] = 128, 128, 128
    p.dtype = _lib.DTYPE_BF16
    last = lib.sfa_debug_get(b"last_prefill_kernel")
    try:
        for impl in (0, 30, 43, 44, 84, 5, 999):
            assert lib.sfa_debug_set(b"prefill_impl", impl) == 0
            for head_dim in (128, 256):             # head_dim 256 ignores the ids of the table, not unknown ones
                p.head_dim = head_dim
                assert lib.sfa_prefill_fwd(ctypes.byref(p), None) == -2, (impl, head_dim)
                err = lib.sfa_last_error()
                assert b"prefill_impl %d" % impl in err, err
                assert (b"diagnostics build" in err) == (impl in (43, 44)), err
        assert lib.sfa_debug_get(b"last_prefill_kernel") == last          # nothing was launched
        assert lib.sfa_debug_set(b"bm128_one_wg", 1) == -2 and b"diagnostics build" in lib.sfa_last_error()
        assert lib.sfa_debug_set(b"bm128_one_wg", 0) == 0
    finally:
        for knob in (b"prefill_impl", b"bm128_one_wg"):
            lib.sfa_debug_set(knob, -1)


def test_launch_paths_read_no_environment():
    """kernel selection must not depend on the environment of the process."""
    csrc = os.path.join(ROOT, "starflashattention_amd", "csrc")
    for f in sorted(os.listdir(csrc)):
        if f == "cxx_surface.hip" or not f.endswith((".hip", ".h")):     # SFA_ROCTX is read ONCE, at library load
            continue
        assert "getenv" not in open(os.path.join(csrc, f)).read(), f


def test_auto_splits_and_workspace(lib):
    # BASELINE config 4 fills the machine without splitting; the reference harness shape needs splits
    assert lib.sfa_decode_auto_splits(256, 32, 128, 8192) == 1
    s = lib.sfa_decode_auto_splits(2, 32, 128, 8192)
    assert s > 1
    assert lib.sfa_decode_workspace_bytes(256, 32, 128, 8192, 1) == 256
    assert lib.sfa_decode_workspace_bytes(2, 32, 128, 8192, 4) == 256 + 2 * 32 * 4 * 128 * 4 + 2 * 32 * 4 * 8
    assert lib.sfa_decode_workspace_bytes(2, 32, 128, 8192, 0) == lib.sfa_decode_workspace_bytes(2, 32, 128, 8192, s)
    # grouped queries: the library sizes its split count by the KV-head count (4 here, not 32)
    s_kv = lib.sfa_decode_auto_splits(2, 4, 128, 8192)
    assert s_kv > s
    assert lib.sfa_decode_workspace_bytes_gqa(2, 32, 4, 128, 8192, 0) == lib.sfa_decode_workspace_bytes(2, 32, 128, 8192, s_kv)
    assert lib.sfa_decode_workspace_bytes_gqa(2, 32, 32, 128, 8192, 0) == lib.sfa_decode_workspace_bytes(2, 32, 128, 8192, 0)


def test_product_never_imports_oracle():
    """Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may touch oracle/."""
    offenders = []
    for base in ("starflashattention_amd", "src", "include", "examples"):
        for dp, _, files in os.walk(os.path.join(ROOT, base)):
            for f in files:
                if f.endswith((".py", ".cpp", ".hip", ".h", ".cc")):
                    txt = open(os.path.join(dp, f), errors="replace").read()
                    if re.search(r"^\s*(from|import)\s+oracle\b", txt, re.M) or "oracle/" in txt:
                        offenders.append(os.path.join(dp, f))
    assert not offenders, offenders


def test_ops_fail_loudly_without_library(monkeypatch):
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", "/nonexistent/libStarFlashAttention.so")
    with pytest.raises(ImportError, match="no CPU fallback"):
        _lib.load()


def test_pybind_extension_surface_matches_reference():
    """Module name, function name and the 16 keyword names in order (reference flash_api.cpp:70-80)."""
    import glob
    import importlib
    if not glob.glob(os.path.join(ROOT, "star_flash_attn*.so")):
        import __graft_entry__
        __graft_entry__.build()
    ext = importlib.import_module("star_flash_attn")
    doc = ext.mha_fwd_cuda.__doc__
    names = ["qkv", "q_bias", "k_bias", "v_bias", "k_cache_table", "v_cache_table", "seq_len", "o",
             "batch_size", "memory_max_len", "num_heads", "head_dim", "rotary_embedding_dim",
             "max_input_length", "num_layer", "idx_layer"]
    sig = doc.split("\n")[0]
    got = re.findall(r"(\w+): ", sig)
    assert got == names, got
    assert "-> torch.Tensor" in sig
    import torch
    with pytest.raises(RuntimeError, match="HIP device"):      # CPU tensors are refused, not computed on
        z = torch.zeros(1, 3, 2, 128, dtype=torch.float16)
        ext.mha_fwd_cuda(z, z, z, z, z, z, z, z, 1, 4, 2, 128, 128, 4, 1, 0)


def test_params_header_abi():
    """src/params.h keeps the reference's field order (params.h:10-68): compile a tiny TU that checks
    the offsets the reference layout implies."""
    import subprocess, tempfile, textwrap
    src = textwrap.dedent('''
        #include <src/params.h>
        #include <cstddef>
        static_assert(offsetof(Flash_decoder_input, q_bias) == 8, "");
        static_assert(offsetof(Flash_decoder_input, v_cache_table) == 56, "");
        static_assert(offsetof(Flash_decoder_input, rotary_sin_table) == 72, "");
        static_assert(offsetof(Flash_decoder_input, memory_max_len) == 84, "");
        static_assert(offsetof(Flash_decoder_input, stride) == 108, "");
        static_assert(offsetof(Flash_decoder_params, num_splits) == 4, "");
        static_assert(offsetof(Flash_decoder_buffers, m_formula) == 16, "");
        int main() { Flash_decoder_input i; return i.qkv == nullptr ? 0 : 1; }
    ''')
    with tempfile.TemporaryDirectory() as d:
        f = os.path.join(d, "abi.cpp")
        open(f, "w").write(src)
        r = subprocess.run(["/opt/rocm/bin/hipcc", "-std=c++17", "-fsyntax-only", "-I" + ROOT, "-x", "hip",
                            "--offload-arch=gfx950", f], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
