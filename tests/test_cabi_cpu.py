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


def _up(x):
    return (x + 255) // 256 * 256


def test_decode_workspace_bytes_closed_formula(lib):
    """sfa_decode_workspace_bytes = 256 + up(B*H*S*D*4) + up(B*H*S*8) for S > 1 and 256 for S = 1, at shapes whose
    (m, l) term is not a multiple of 256 (a row of partial outputs, D * 4 bytes, always is)."""
    ws = lib.sfa_decode_workspace_bytes
    for B, H, D, S in ((3, 5, 64, 3), (1, 3, 128, 5), (7, 1, 256, 9)):
        assert (B * H * S * 8) % 256
        assert ws(B, H, D, 4096, S) == 256 + _up(B * H * S * D * 4) + _up(B * H * S * 8), (B, H, D, S)
        assert ws(B, H, D, 4096, 1) == 256
        for M in (4096, 65536):
            assert ws(B, H, D, M, 0) == ws(B, H, D, M, lib.sfa_decode_auto_splits(B, H, D, M)), (B, H, D, M)
    assert lib.sfa_decode_auto_splits(3, 5, 64, 65536) > 1         # the num_splits = 0 sizes above include partials


ENTRY_POINTS = ("sfa_decode", "sfa_decode_chunk", "sfa_decode_varlen")
_ROW = (8 + 2 * 4) * 128        # (H + 2*Hkv) * D of the well-formed call below


def _well_formed():
    """A call every entry point accepts up to its workspace check (the workspace is NULL): 4 tokens, 8 query heads in
    groups of 2, head_dim 128, fake 16-byte aligned pointers."""
    a = _lib.DecodeArgs()
    for f in ("qkv", "o", "seq_len", "k_cache_table", "v_cache_table"):
        setattr(a, f, 0x1000)
    a.batch_size, a.num_heads, a.num_heads_kv, a.memory_max_len, a.num_layer, a.head_dim = 1, 8, 4, 64, 1, 128
    a.rotary_embedding_dim = 128
    return a, {"count": 4, "token_stride": 0, "cu_tokens": 0x4000, "null_args": False}


def _set(**fields):
    def mutate(a, call, entry):
        for k, v in fields.items():
            if k in call:
                call[k] = v
            else:
                setattr(a, k, v)
    return mutate


def _paged(**fields):
    return _set(kv_layout=_lib.KV_LAYOUTS["paged"], **{**dict(block_table=0x3000, page_size=16, num_pages=4,
                                                               block_table_stride=4), **fields})


def _workspace(short=0, address=0x2000):
    """A workspace for num_splits = 3 at `address`, `short` bytes smaller than the entry point asks for."""
    def mutate(a, call, entry):
        lib = _lib.load()
        need = {"sfa_decode": lambda: lib.sfa_decode_workspace_bytes(1, 8, 128, 64, 3),
                "sfa_decode_chunk": lambda: lib.sfa_decode_chunk_workspace_bytes(1, 8, 4, 128, 64, 4, 3),
                "sfa_decode_varlen": lambda: lib.sfa_decode_varlen_workspace_bytes(1, 8, 4, 128, 64, 4, 3)}[entry]()
        a.num_splits, a.workspace, a.workspace_bytes = 3, address, need - short
    return mutate


def _malformed_status(lib, entry, mutate):
    a, call = _well_formed()
    mutate(a, call, entry)
    args = None if call["null_args"] else ctypes.byref(a)
    if entry == "sfa_decode":
        st = lib.sfa_decode(args, None)
    elif entry == "sfa_decode_chunk":
        st = lib.sfa_decode_chunk(args, call["count"], call["token_stride"], None)
    else:
        st = lib.sfa_decode_varlen(args, call["cu_tokens"], call["count"], call["token_stride"], None)
    return st, lib.sfa_last_error()


# (what is wrong, how the well-formed call is changed, the status of sfa_decode / sfa_decode_chunk / sfa_decode_varlen).
# WS: the entry point has nothing to object to and goes on to its workspace check, which fails with -1 "workspace is
# NULL"; a plain -1 is another NULL pointer.  The codes were recorded from the library as it was when sfa_decode and the
# token calls each had a validator of their own.
WS = "workspace is NULL"
MALFORMED = [
    ("nothing: the workspace check", _set(), (WS, WS, WS)),
    ("NULL args", _set(null_args=True), (-1, -1, -1)),
    ("qkv missing", _set(qkv=None), (-1, -1, -1)),
    ("o missing", _set(o=None), (-1, -1, -1)),
    ("seq_len missing", _set(seq_len=None), (-1, -1, -1)),
    ("k_cache_table missing", _set(k_cache_table=None), (-1, -1, -1)),
    ("v_cache_table missing", _set(v_cache_table=None), (-1, -1, -1)),
    ("cu_tokens missing", _set(cu_tokens=None), (WS, WS, -1)),
    ("cos table only", _set(rotary_cos_table=0x5000), (-1, -1, -1)),
    ("sin table only", _set(rotary_sin_table=0x5000), (-1, -1, -1)),
    ("negative count", _set(count=-1), (WS, -2, -2)),
    ("negative batch_size", _set(batch_size=-1), (-2, -2, -2)),
    ("batch_size 65536", _set(batch_size=65536), (WS, -2, -2)),
    ("num_heads 0", _set(num_heads=0), (-2, -2, -2)),
    ("memory_max_len 0", _set(memory_max_len=0), (-2, -2, -2)),
    ("idx_layer = num_layer", _set(idx_layer=1), (-2, -2, -2)),
    ("idx_layer negative", _set(idx_layer=-1), (-2, -2, -2)),
    ("head_dim 96", _set(head_dim=96), (-4, -4, -4)),
    ("head_dim 256", _set(head_dim=256, rotary_embedding_dim=0), (WS, -4, -4)),
    ("odd rotary_embedding_dim", _set(rotary_embedding_dim=127), (-2, -2, -2)),
    ("rotary_embedding_dim > head_dim", _set(rotary_embedding_dim=130), (-2, -2, -2)),
    ("dtype 7", _set(dtype=7), (-3, -3, -3)),
    ("group of 3", _set(num_heads=12, num_heads_kv=4), (-2, -2, -2)),
    ("heads not a multiple of kv heads", _set(num_heads=6, num_heads_kv=4), (-2, -2, -2)),
    ("negative num_heads_kv", _set(num_heads_kv=-2), (-2, -2, -2)),
    ("stride too small", _set(stride=8), (-2, -2, -2)),
    ("stride not a multiple of 8", _set(stride=4 * _ROW + 4), (-2, -2, -2)),
    ("token stride too small", _set(token_stride=100), (WS, -2, -2)),
    ("token stride not a multiple of 8", _set(token_stride=_ROW + 4), (WS, -2, -2)),
    ("num_splits 1025", _set(num_splits=1025), (-2, -2, -2)),
    ("kv_layout 3", _set(kv_layout=3), (-2, -2, -2)),
    ("paged without a table", _paged(block_table=None), (-1, -1, -1)),
    ("page_size 8", _paged(page_size=8, block_table_stride=8), (-2, -2, -2)),
    ("page_size 24", _paged(page_size=24), (-2, -2, -2)),
    ("table does not cover memory_max_len", _paged(block_table_stride=3), (-2, -2, -2)),
    ("num_pages 0", _paged(num_pages=0), (-2, -2, -2)),
    ("misaligned block_table", _paged(block_table=0x3002), (-2, -2, -2)),
    ("well-formed paged call", _paged(), (WS, WS, WS)),
    ("misaligned qkv", _set(qkv=0x1008), (-2, -2, -2)),
    ("misaligned k_bias", _set(k_bias=0x1004), (-2, -2, -2)),
    ("misaligned cu_tokens", _set(cu_tokens=0x4002), (WS, WS, -2)),
    ("head-major cache", _set(kv_layout=_lib.KV_LAYOUTS["blhmd"]), (WS, WS, WS)),
    ("workspace one byte short", _workspace(short=1), (-5, -5, -5)),
    ("workspace of 16 bytes", _set(workspace=0x2000, workspace_bytes=16, num_splits=3), (-5, -5, -5)),
    ("misaligned workspace", _workspace(address=0x2010), (-2, -2, -2)),
    ("misaligned workspace, one byte short", _workspace(short=1, address=0x2010), (-5, -5, -5)),
    ("bad idx_layer before head_dim 96", _set(idx_layer=1, head_dim=96), (-2, -2, -2)),
    ("head_dim 96 before dtype 7", _set(head_dim=96, dtype=7), (-4, -4, -4)),
    ("dtype 7 before a group of 3", _set(dtype=7, num_heads=12), (-3, -3, -3)),
    ("num_splits 1025 before paged without a table", _paged(block_table=None, num_splits=1025), (-2, -2, -2)),
    ("paged without a table before misaligned qkv", _paged(block_table=None, qkv=0x1008), (-1, -1, -1)),
    ("qkv missing before a negative count", _set(qkv=None, count=-1), (-1, -1, -1)),
]


@pytest.mark.skipif(torch.cuda.is_available(), reason="calls the decode entry points with fake device pointers")
@pytest.mark.parametrize("entry", ENTRY_POINTS)
def test_malformed_arguments_same_status_on_every_decode_entry_point(lib, entry):
    for what, mutate, expected in MALFORMED:
        st, err = _malformed_status(lib, entry, mutate)
        want = expected[ENTRY_POINTS.index(entry)]
        assert st == (-1 if want is WS else want), (what, entry, st, err)
        assert err.startswith(entry.encode() + b":"), (what, entry, err)
        assert (WS.encode() in err) == (want is WS), (what, entry, err)


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
