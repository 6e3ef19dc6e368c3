"""CPU-only checks of sfa_decode_window (sliding-window decode): the symbols and the Python operator exist beside an
unchanged sfa_decode_args and ABI version, the entry point validates its arguments before any HIP call, the workspace
size is sfa_decode's for the split count of the window, the sweep of the GPU test covers its factors pairwise, the
reference masks what it should, and the kernel translation unit compiles for gfx950 without scratch."""
import ctypes
import itertools
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT
from starflashattention_amd import _lib
import window_ref

KERNEL = os.path.join(ROOT, "starflashattention_amd", "csrc", "decode_window_kernel.hip")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def test_window_symbols_exported(lib):
    for name in ("sfa_decode_window", "sfa_decode_window_workspace_bytes"):
        assert name in _lib.EXPORTED_SYMBOLS
        assert hasattr(lib, name)
    import starflashattention_amd as sfa
    from starflashattention_amd.ops import flash_decode_window
    assert sfa.flash_decode_window is flash_decode_window
    with open(os.path.join(ROOT, "include", "star_flash_attn.h")) as f:
        header = f.read()
    assert "sfa_decode_window(" in header and "sfa_decode_window_workspace_bytes(" in header
    # new symbols beside the same struct and the same ABI version
    assert "#define SFA_ABI_VERSION 4" in header
    assert lib.sfa_abi_version() == 4
    assert ctypes.sizeof(_lib.DecodeArgs) == 10 * 8 + 12 * 4 + 8 + 8 + 8 + 8 + 8 + 8


def _args():
    a = _lib.DecodeArgs()
    for f in ("qkv", "o", "seq_len", "k_cache_table", "v_cache_table"):
        setattr(a, f, 0x1000)
    a.batch_size, a.num_heads, a.memory_max_len, a.num_layer, a.head_dim = 1, 2, 64, 1, 128
    a.rotary_embedding_dim = 128
    return a


@pytest.mark.skipif(torch.cuda.is_available(), reason="calls sfa_decode_window with fake device pointers")
def test_decode_window_argument_validation_without_gpu(lib):
    call = lambda a, w=8: lib.sfa_decode_window(ctypes.byref(a) if a is not None else None, w, None)
    err = lambda: lib.sfa_last_error()
    assert call(None) == -1 and err().startswith(b"sfa_decode_window:")
    assert call(_lib.DecodeArgs()) == -1 and err().startswith(b"sfa_decode_window:")
    a = _args()
    for w in (0, -3):
        assert call(a, w) == -2 and err().startswith(b"sfa_decode_window:") and b"window" in err()
    a.head_dim = 96
    assert call(a) == -4 and err().startswith(b"sfa_decode_window:")
    a.head_dim = 128
    a.num_heads, a.num_heads_kv = 12, 4                         # group of 3
    assert call(a) == -2 and b"num_heads_kv" in err()
    for group in (1, 2, 4, 8, 16):                              # every group up to 16 is served, as far as the workspace
        a.num_heads, a.num_heads_kv = group, 1
        assert call(a) == -1 and err().startswith(b"sfa_decode_window: workspace is NULL")
    a.head_dim, a.rotary_embedding_dim = 256, 128               # head_dim 256 too
    assert call(a) == -1 and err().startswith(b"sfa_decode_window: workspace is NULL")
    assert call(a, 1) == -1 and call(a, 2 ** 31 - 1) == -1      # any window >= 1
    a.workspace, a.workspace_bytes, a.num_splits = 0x2000, 256, 2
    assert call(a) == -5 and err().startswith(b"sfa_decode_window:")       # sfa_decode's workspace: too small for 2 splits
    a.workspace = 0x2010
    a.workspace_bytes = 1 << 30
    assert call(a) == -2 and b"256-byte aligned" in err()
    a.batch_size = 0
    assert call(a) == 0                                         # nothing to do


def test_window_workspace_is_decodes_for_the_windows_split_count(lib):
    ws = lib.sfa_decode_window_workspace_bytes
    for B, H, Hkv, D, M in ((1, 32, 8, 128, 32768), (2, 16, 1, 64, 8192), (4, 8, 2, 128, 1408), (1, 32, 32, 256, 65536),
                            (256, 32, 4, 128, 32768), (3, 64, 4, 128, 131072)):
        for W in (1, 17, 2048, 4096, 4097, 8192, 30000, M - 1, M, M + 1, 2 ** 31 - 1):
            S = lib.sfa_decode_auto_splits(B, Hkv, D, min(W, M))
            assert ws(B, H, Hkv, D, M, W, 0) == lib.sfa_decode_workspace_bytes(B, H, D, M, S), (B, H, Hkv, D, M, W)
            assert ws(B, H, Hkv, D, M, W, 0) <= lib.sfa_decode_workspace_bytes_gqa(B, H, Hkv, D, M, 0)
            for S in (1, 3, 4):
                assert ws(B, H, Hkv, D, M, W, S) == lib.sfa_decode_workspace_bytes(B, H, D, M, S)
    # a window shorter than two minimal splits is not split; the whole history would be
    assert lib.sfa_decode_auto_splits(1, 8, 128, 32768) > 1 == lib.sfa_decode_auto_splits(1, 8, 128, 4095)
    assert ws(1, 32, 8, 128, 32768, 4095, 0) == 256 < ws(1, 32, 8, 128, 32768, 32768, 0)
    assert ws(0, 32, 8, 128, 32768, 4096, 0) == 256             # never 0: the status block


def test_sweep_covers_its_factors_pairwise():
    F = window_ref.FACTORS
    for c in window_ref.SWEEP:
        assert len(c) == len(F) and all(x in f for x, f in zip(c, F)), c
    for i, j in itertools.combinations(range(len(F)), 2):
        seen = {(c[i], c[j]) for c in window_ref.SWEEP}
        assert seen == set(itertools.product(F[i], F[j])), (i, j)


def test_reference_window():
    """window = None and a window beyond pos are the full attention of oracle.decode_ref; the rows below lo do not
    matter (NaN there changes nothing); window = 1 returns the new V row."""
    from oracle import decode_ref
    rng = np.random.default_rng(9)
    B, H, Hkv, D, L, M, layer, rot = 3, 4, 2, 64, 2, 96, 1, 32
    r16 = lambda *s: torch.from_numpy(rng.standard_normal(s, dtype=np.float32)).half().float().numpy()
    q, k, v, kc, vc = r16(B, H, D), r16(B, Hkv, D), r16(B, Hkv, D), r16(B, L, M, Hkv, D), r16(B, L, M, Hkv, D)
    lens = [0, 40, 95]
    full = window_ref.decode_window_ref(q, k, v, kc, vc, lens, layer, rot, None)
    G = H // Hkv
    x = lambda t, ax: np.repeat(t, G, axis=ax)
    want = decode_ref(np.stack([q, x(k, 1), x(v, 1)], 1), x(kc, 3).copy(), x(vc, 3).copy(), lens, layer, rot)
    np.testing.assert_allclose(full["o"], want["o"], atol=1e-6, rtol=1e-6)
    np.testing.assert_array_equal(full["k_row"], want["k_row"][:, ::G])
    np.testing.assert_array_equal(full["v_row"], want["v_row"][:, ::G])
    np.testing.assert_array_equal(window_ref.decode_window_ref(q, k, v, kc, vc, lens, layer, rot, 96)["o"], full["o"])
    w = 17
    kp, vp = kc.copy(), vc.copy()
    for b, pos in enumerate(lens):
        lo = window_ref.window_lo(pos, w)
        kp[b, layer, :lo] = vp[b, layer, :lo] = np.nan
    assert [window_ref.window_lo(p, w) for p in lens] == [0, 24, 79]
    a = window_ref.decode_window_ref(q, k, v, kc, vc, lens, layer, rot, w)
    b_ = window_ref.decode_window_ref(q, k, v, kp, vp, lens, layer, rot, w)
    np.testing.assert_array_equal(a["o"], b_["o"])
    assert np.isfinite(a["o"]).all() and np.abs(a["o"][2] - full["o"][2]).max() > 0.05
    np.testing.assert_array_equal(a["o"][0], full["o"][0])       # pos 0: the window does not bind
    one = window_ref.decode_window_ref(q, k, v, kp, vp, lens, layer, rot, 1)
    np.testing.assert_allclose(one["o"], x(one["v_row"], 1), atol=1e-7, rtol=0)


def test_window_kernel_compiles_without_scratch(tmp_path):
    """Every kernel of the sliding-window translation unit compiles for gfx950 with no spill to scratch."""
    r = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-I" + ROOT,
                        "-Rpass-analysis=kernel-resource-usage", "-c", KERNEL, "-o", str(tmp_path / "k.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    # (fp16, bf16) x (64, 128, 256) x (default, non-temporal loads) x (operand-layout, row-major, paged): the group size
    # is a run-time value
    assert len(names) == len(scratch) == 36, (names, scratch)
    assert all(s == 0 for s in scratch), list(zip(names, scratch))
    assert all("decode_window_kernel" in nm for nm in names)
