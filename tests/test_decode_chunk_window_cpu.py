"""CPU-only checks of sfa_decode_chunk_window / sfa_decode_varlen_window (the sliding window in the multi-token decode
calls): the symbols and the Python operators exist beside an unchanged ABI version, the entry points validate their
arguments before any HIP call, the workspace arithmetic (never larger than the size without a window), the sweep of the
GPU tests covers its factors pairwise, the reference is window_ref.decode_window_ref applied token by token, the
conditions the GPU tests put on their inputs, a numpy model of the kernel's key range, row clamp and lower mask under
four one-row slips, and the two translation units compile for gfx950 without scratch at the occupancy of their twins."""
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
import chunk_window_ref as cw
from chunk_window_ref import HKV, KTILE, LAYER, LENS, QTILE, TOL, WAVE

CSRC = os.path.join(ROOT, "starflashattention_amd", "csrc")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


NEW_SYMBOLS = ("sfa_decode_chunk_window", "sfa_decode_chunk_window_workspace_bytes", "sfa_decode_varlen_window",
               "sfa_decode_varlen_window_workspace_bytes")


def test_chunk_window_symbols_exported(lib):
    import starflashattention_amd as sfa
    from starflashattention_amd import ops
    with open(os.path.join(ROOT, "include", "star_flash_attn.h")) as f:
        header = f.read()
    for name in NEW_SYMBOLS:
        assert name in _lib.EXPORTED_SYMBOLS
        assert hasattr(lib, name)
        assert name + "(" in header
    assert sfa.flash_decode_chunk_window is ops.flash_decode_chunk_window
    assert sfa.flash_decode_varlen_window is ops.flash_decode_varlen_window
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


@pytest.mark.skipif(torch.cuda.is_available(), reason="calls the entry points with fake device pointers")
@pytest.mark.parametrize("fn", ["sfa_decode_chunk_window", "sfa_decode_varlen_window"])
def test_chunk_window_argument_validation_without_gpu(lib, fn):
    if fn == "sfa_decode_chunk_window":
        call = lambda a, w=8, n=4: lib.sfa_decode_chunk_window(ctypes.byref(a) if a is not None else None, n, 0, w, None)
    else:
        call = lambda a, w=8, n=4: lib.sfa_decode_varlen_window(ctypes.byref(a) if a is not None else None, 0x4000, n, 0,
                                                                w, None)
    err = lambda: lib.sfa_last_error()
    assert call(None) == -1 and err().startswith(fn.encode() + b":")
    assert call(_lib.DecodeArgs()) == -1 and err().startswith(fn.encode() + b":")
    a = _args()
    for w in (0, -3):
        assert call(a, w) == -2 and err().startswith(fn.encode() + b":") and b"window" in err()
    assert call(a, n=-1) == -2
    a.head_dim = 96
    assert call(a) == -4
    a.head_dim = 256
    assert call(a) == -4 and err().startswith(fn.encode() + b":")            # SFA_ERR_UNSUPPORTED_HEAD_DIM
    a.head_dim = 128
    a.num_heads, a.num_heads_kv = 12, 4                         # group of 3
    assert call(a) == -2 and b"num_heads_kv" in err()
    a.num_heads, a.num_heads_kv = 8, 4
    assert call(a) == -1 and b"workspace is NULL" in err()
    assert call(a, 1) == -1 and call(a, 2 ** 31 - 1) == -1      # any window >= 1
    a.workspace, a.workspace_bytes, a.num_splits = 0x2000, 256, 2
    assert call(a) == -5 and err().startswith(fn.encode() + b":")
    a.workspace, a.workspace_bytes = 0x2010, 1 << 30
    assert call(a) == -2 and b"256-byte aligned" in err()
    assert call(a, n=0) == 0                                    # nothing to do
    a.batch_size = 0
    assert call(a) == 0


def _auto(wgs, M):
    """clamp_splits of c_api.hip: aim for 256 workgroups, splits of at least 512 rows, at most 32"""
    return max(1, min(-(-256 // wgs), max(M // 512, 1), 32))


def test_chunk_window_workspace_arithmetic(lib):
    cws, vws = lib.sfa_decode_chunk_window_workspace_bytes, lib.sfa_decode_varlen_window_workspace_bytes
    chunk, varlen = lib.sfa_decode_chunk_workspace_bytes, lib.sfa_decode_varlen_workspace_bytes
    shapes = ((1, 32, 8, 128, 32768), (2, 16, 1, 64, 8192), (4, 8, 2, 128, 1408), (4, 32, 32, 128, 32768),
              (64, 32, 32, 128, 32768), (3, 64, 4, 128, 131072))
    for B, H, Hkv, D, M in shapes:
        G = H // Hkv
        for n in (1, 8, 40, 512, 2048):
            sizes = []
            for W in sorted({1, 17, 512, 1024, 1025, 4096, 30000, M - 1, M, M + 1, 2 ** 31 - 1}):
                reach = min(M, W - 1 + n)                       # the most rows a sequence can read
                # an explicit split count: the size of the call without a window
                for S in (1, 3, 4):
                    assert cws(B, H, Hkv, D, M, n, W, S) == chunk(B, H, Hkv, D, M, n, S)
                    assert vws(B, H, Hkv, D, M, n, W, S) == varlen(B, H, Hkv, D, M, n, S)
                # the library's choice: the call's own rule over `reach` rows
                s_c = _auto(B * Hkv * ((n * G + 255) // 256), reach)
                s_v = _auto((n * G // 256 + B) * Hkv, reach)
                assert cws(B, H, Hkv, D, M, n, W, 0) == chunk(B, H, Hkv, D, M, n, s_c), (B, H, Hkv, D, M, n, W)
                assert vws(B, H, Hkv, D, M, n, W, 0) == varlen(B, H, Hkv, D, M, n, s_v), (B, H, Hkv, D, M, n, W)
                assert cws(B, H, Hkv, D, M, n, W, 0) == chunk(B, H, Hkv, D, reach, n, 0)
                # never larger than the size without a window
                assert cws(B, H, Hkv, D, M, n, W, 0) <= chunk(B, H, Hkv, D, M, n, 0)
                assert vws(B, H, Hkv, D, M, n, W, 0) <= varlen(B, H, Hkv, D, M, n, 0)
                sizes.append((cws(B, H, Hkv, D, M, n, W, 0), vws(B, H, Hkv, D, M, n, W, 0)))
            # the rule is monotone in the rows a sequence can read
            assert sizes == sorted(sizes), (B, H, Hkv, D, M, n, sizes)
    # the non-window sizes are monotone in memory_max_len, which is why the bound above holds for every window
    for B, H, Hkv, D, n in ((1, 32, 8, 128, 8), (4, 32, 32, 128, 512)):
        by_m = [chunk(B, H, Hkv, D, m, n, 0) for m in (1, 511, 512, 1024, 4096, 16384, 65536)]
        assert by_m == sorted(by_m)
        by_m = [varlen(B, H, Hkv, D, m, n, 0) for m in (1, 511, 512, 1024, 4096, 16384, 65536)]
        assert by_m == sorted(by_m)
    # a short window over a long cache is not split; the whole history would be
    assert cws(1, 32, 8, 128, 32768, 8, 128, 0) == chunk(1, 32, 8, 128, 32768, 8, 1) < chunk(1, 32, 8, 128, 32768, 8, 0)
    assert cws(0, 32, 8, 128, 32768, 8, 128, 0) == 256 and vws(4, 32, 8, 128, 32768, 0, 128, 0) == 256


def test_chunk_window_sweep_covers_its_factors_pairwise():
    F = cw.FACTORS
    for c in cw.SWEEP:
        assert len(c) == len(F) and all(x in f for x, f in zip(c, F)), c
    for i, j in itertools.combinations(range(len(F)), 2):
        seen = {(c[i], c[j]) for c in cw.SWEEP}
        assert seen == set(itertools.product(F[i], F[j])), (i, j)
    # two q-tiles at G = 1 (300 rows) and at G = 8 (320 rows)
    assert cw.sweep_tokens(1) > QTILE and QTILE < cw.sweep_tokens(8) * 8 <= 2 * QTILE


# ---- the reference -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_reference_is_decode_window_ref_token_by_token(dtype):
    """chunk_window_ref against its definition, n successive decode_window_ref calls with the appended rows fed forward;
    NaN below lo_0 changes nothing; a window that does not bind is the call without one."""
    for tables in (False, True):
        p = cw.make_problem(dtype, 64, 2, (0, 5, 70, 130), (9, 0, 20, 3), tables=tables, seed=3)
        for window in (1, 17, 33, None):
            a, b = cw.chunk_window_ref(p, window), cw.chunk_window_ref_literal(p, window)
            for (o1, k1, v1), (o2, k2, v2) in zip(a, b):
                np.testing.assert_allclose(o1, o2, atol=1e-6, rtol=1e-6)
                np.testing.assert_array_equal(k1, k2)
                np.testing.assert_array_equal(v1, v2)
    p = cw.make_problem(dtype, 64, 2, (0, 5, 70, 130), (9, 0, 20, 3), seed=3)
    kc, vc = p.kc.clone(), p.vc.clone()
    for b, pos in enumerate(p.lens):
        kc[b, LAYER, :cw.window_lo(pos, 17)] = float("nan")
        vc[b, LAYER, :cw.window_lo(pos, 17)] = float("nan")
    q = cw.make_problem(dtype, 64, 2, p.lens, p.ns, qkv=p.qkv, kc=kc, vc=vc, seed=3)
    q.qb, q.kb, q.vb = p.qb, p.kb, p.vb
    for (o1, _, _), (o2, _, _) in zip(cw.chunk_window_ref(p, 17), cw.chunk_window_ref(q, 17)):
        np.testing.assert_array_equal(o1, o2)
        assert np.isfinite(o1).all()
    for (o1, _, _), (o2, _, _) in zip(cw.chunk_window_ref(p, 133), cw.chunk_window_ref(p, None)):
        np.testing.assert_array_equal(o1, o2)


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_window_binds_in_the_reference(dtype):
    """pos = 1000, window = 100: the windowed and the full reference differ by more than ten tolerances"""
    D, G, n, window = 128, 4, 40, 100
    ref, full = cw.reference(dtype, D, G, n, window), cw.reference(dtype, D, G, n, None)
    b = LENS.index(1000)
    gap = np.abs(ref[b][0] - full[b][0])
    assert gap.max() > 10 * TOL[dtype] * (1.0 + np.abs(full[b][0]).max()), gap.max()
    # where the window does not bind (pos = 0, 5: pos + n <= window) the two are the same
    for b in (0, 1):
        np.testing.assert_array_equal(ref[b][0], full[b][0])


# ---- the window-edge problems --------------------------------------------------------------------------------------------

def test_edge_problems_hit_the_kernels_boundaries():
    assert cw.EDGE_N > QTILE                                    # two q-tiles
    for window in cw.EDGE_WINDOWS:
        lens = cw.edge_lens(window)
        assert tuple(cw.window_lo(pos, window) for pos in lens) == cw.EDGE_LO0
        for (pos, jstar), (tau, lo) in zip(cw.spike_rows(window), cw.SPIKES):
            assert pos >= 0 and jstar >= 0 and cw.window_lo(pos + tau, window) == jstar + 1
            assert cw.window_lo(pos + tau - 1, window) == jstar
            if lo is not None:
                assert lo % (KTILE // 2) == 0
        taus = [t for t, _ in cw.SPIKES]
        assert WAVE in taus and 2 * WAVE - 1 in taus and QTILE in taus          # first / last row of a wave, second q-tile
        los = [lo for _, lo in cw.SPIKES if lo is not None]
        assert any(lo % KTILE == 0 for lo in los) and any(lo % KTILE == KTILE // 2 for lo in los)


def _marks(prob, b):
    """the V value of every row of sequence b of an "equal" problem (all elements of a row are equal): the cache rows
    below pos, then the new rows"""
    pos = prob.lens[b]
    H = prob.H
    return np.concatenate([prob.vf[b, LAYER, :pos, 0, 0], prob.qkv[b, :, H + HKV, 0].float().numpy()]).astype(np.float64)


@pytest.mark.parametrize("window", cw.EDGE_WINDOWS)
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_equal_keys_problem_tells_every_one_row_slip(dtype, window):
    """Condition (b) of the GPU test, from the fp64 reference alone: with all keys equal, a row dropped, added or counted
    twice at either edge of any token's window moves o by more than five tolerances (every element of a V row holds the
    same value, so in all elements)."""
    prob = cw.edge_problem(dtype, window, "equal")
    ref = cw.chunk_window_ref(prob, window)
    for b, pos in enumerate(prob.lens):
        m = _marks(prob, b)
        m = np.concatenate([m, m[-1:] * 0 + (16.0 if len(m) % 2 == 0 else -16.0)])      # the row after the last token
        for t in range(cw.EDGE_N):
            lo, hi = cw.window_lo(pos + t, window), pos + t
            S, c = m[lo:hi + 1].sum(), hi - lo + 1
            o = S / c
            np.testing.assert_allclose(ref[b][0][t], o, atol=1e-5, rtol=1e-5)
            slips = [(S + m[hi + 1]) / (c + 1), (S + m[lo]) / (c + 1), (S + m[hi]) / (c + 1)]
            if c > 1:
                slips += [(S - m[lo]) / (c - 1), (S - m[hi]) / (c - 1)]
            if lo >= 1:
                slips.append((S + m[lo - 1]) / (c + 1))
            for s in slips:
                assert abs(s - o) > 5 * TOL[dtype] * (1.0 + abs(o)), (b, t, s, o)


def kernel_model(prob, window, slip=None, paged=False):
    """fp64 attention over the key slots as chunk_attn_kernel with the window flag addresses them at G = 1 and
    num_splits = 1 (decode_chunk_body.h): per wave of 32 rows, the tiles from max(the q-tile's first tile, the tile of the
    wave's smallest lower bound) to the wave's causal end; a 32-key half is masked from above where it crosses the
    wave's smallest limit and from below where it starts under the wave's largest lower bound; the row a slot reads is
    clamped to [lo_0, pos + n - 1] within the first / last tile, and (paged, page size 16, identity table) its page is
    that of min(max(first row of the 16-row slot, lo_0), pos + n - 1).
    slip: "narrow" / "wide" = the lower mask key <= lo / key < lo - 1; "long" = the window one row long; "page" = the
    first page slot resolved one row too high."""
    W = window + (1 if slip == "long" else 0)
    low = lambda lim: max(0, lim + 1 - W)
    out = []
    for b, (pos, n) in enumerate(zip(prob.lens, prob.ns)):
        H, D = prob.H, prob.D
        x = prob.qkv[b, :n].float().numpy().astype(np.float64)
        q = x[:, :H]                                                             # rot = 0, no bias: the input bits
        K = np.concatenate([prob.kf[b, LAYER, :pos].astype(np.float64), x[:, H:H + HKV]])
        V = np.concatenate([prob.vf[b, LAYER, :pos].astype(np.float64), x[:, H + HKV:]])
        Kb = pos + n
        ntot = -(-Kb // KTILE)
        lo0 = low(pos)
        tlo = lo0 // KTILE
        first0, last0 = lo0 - tlo * KTILE, Kb - 1 - (ntot - 1) * KTILE
        o = np.zeros((n, H, D))
        for wq0 in range(0, n, WAVE):                                            # a wave: the rows wq0 .. wlast
            q0 = wq0 // QTILE * QTILE
            wlast = min(wq0 + WAVE - 1, n - 1)
            ts0 = max(tlo, low(pos + q0) // KTILE)
            wlim, wlo = pos + wq0, low(pos + wlast)
            t = np.arange(wq0, wlast + 1)[:, None]
            lim, lo = pos + t, np.maximum(0, pos + t + 1 - W)
            T0, T1 = max(ts0, low(wlim) // KTILE), min(ntot, (pos + wlast) // KTILE + 1)
            key = np.arange(T0 * KTILE, T1 * KTILE)[None, :]
            tile, j, kbase = key // KTILE, key % KTILE, key // 32 * 32
            below = {"narrow": key <= lo, "wide": key < lo - 1}.get(slip, key < lo)
            seen = ~(((kbase + 31 > wlim) | (kbase < wlo)) & (key > lim)) & ~((kbase < wlo) & below)      # [rows, keys]
            r = np.minimum(np.maximum(j, np.where(tile == tlo, first0, 0)), np.where(tile == ntot - 1, last0, KTILE - 1))
            rows = tile * KTILE + r
            if paged:
                slot_row = np.minimum(np.maximum(tile * KTILE + (r >> 4 << 4), lo0 + (1 if slip == "page" else 0)), Kb - 1)
                rows = (slot_row >> 4 << 4) + (r & 15)
            rows = rows[0]
            sc = np.matmul(q[wq0:wlast + 1].transpose(1, 0, 2), K[rows].transpose(1, 2, 0)) * D ** -0.5       # [h, t, j]
            sc = np.where(seen[None], sc, -np.inf)
            w = np.exp(sc - sc.max(axis=2, keepdims=True))
            o[wq0:wlast + 1] = np.matmul(w / w.sum(axis=2, keepdims=True), V[rows].transpose(1, 0, 2)).transpose(1, 0, 2)
        out.append(o)
    return out


@pytest.mark.parametrize("window", cw.EDGE_WINDOWS)
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_chunk_window_edge_problems_tell_one_row_slips_apart(dtype, window):
    """The model without a slip is the reference on every edge problem.  With one, the tokens of the equal-keys problem
    that it puts outside the GPU test's elementwise tolerance are exactly:
      mask one key narrow -- every token whose lower bound lies in a half the wave masks from below: all but a token
          whose bound is the wave's largest and a multiple of 32;
      mask one key wide   -- every token with lo_t >= 1 whose row lo_t - 1 lies in a tile its wave computes: all but the
          wave's first token where its bound is a multiple of 64 (token 0 counts row lo_0 twice: the clamp);
      window one row long -- every token with lo_t >= 1;
      first page one off (paged) -- token 0 where lo_0 is the last row of its page."""
    low = lambda lim: max(0, lim + 1 - window)
    for kind in ("spike", "equal", "ramp"):
        prob = cw.edge_problem(dtype, window, kind)
        ref = cw.chunk_window_ref(prob, window)
        for paged in (False, True):
            for o, (r, _, _) in zip(kernel_model(prob, window, None, paged), ref):
                np.testing.assert_allclose(o, r, atol=1e-6, rtol=1e-6)
    prob = cw.edge_problem(dtype, window, "equal")
    ref = cw.chunk_window_ref(prob, window)
    tol = TOL[dtype]
    n = cw.EDGE_N
    for slip in ("narrow", "wide", "long", "page"):
        for paged in (False, True) if slip != "page" else (True,):
            got = kernel_model(prob, window, slip, paged)
            for b, pos in enumerate(prob.lens):
                out = (np.abs(got[b] - ref[b][0]) > tol * (1.0 + np.abs(ref[b][0]))).any(axis=(1, 2))
                want = []
                for t in range(n):
                    q0 = t // QTILE * QTILE
                    wq0 = q0 + (t - q0) // WAVE * WAVE
                    wlo, lo = low(pos + min(wq0 + WAVE - 1, n - 1)), low(pos + t)
                    first_tile = max(low(pos) // KTILE, low(pos + q0) // KTILE, low(pos + wq0) // KTILE)
                    want.append({"narrow": lo // 32 * 32 < wlo,
                                 "wide": lo >= 1 and (lo - 1) // KTILE >= first_tile,
                                 "long": lo >= 1,
                                 "page": t == 0 and low(pos) % 16 == 15}[slip])
                assert out.tolist() == want, (slip, paged, b, pos, np.flatnonzero(out != np.array(want))[:8])
        assert slip == "page" or any(want)


# ---- the translation units -----------------------------------------------------------------------------------------------

def _remarks(src, tmp_path):
    r = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-I" + ROOT,
                        "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, src), "-o",
                        str(tmp_path / (src + ".o"))], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    out = {}
    for blk in r.stderr.split("Function Name: ")[1:]:
        name = blk.split()[0]
        out[name] = {k: int(re.search(re.escape(k) + r": (\d+)", blk).group(1))
                     for k in ("VGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "LDS Size [bytes/block]")}
    return out


def _attention(remarks):
    """{(dtype, D, PAGED): resources} of the chunk_attn_kernel instantiations"""
    out = {}
    for nm, v in remarks.items():
        if "chunk_attn_kernel" in nm:
            m = re.search(r"(Fp16|Bf16)ELi(\d+)ELb([01])E", nm)
            out[(m.group(1), int(m.group(2)), int(m.group(3)))] = dict(v, name=nm)
    return out


@pytest.mark.parametrize("pair", [("decode_chunk_window_kernel.hip", "decode_chunk_kernel.hip", 20),
                                  ("decode_varlen_window_kernel.hip", "decode_varlen_kernel.hip", 21)],
                         ids=lambda p: p[0])
def test_window_kernels_compile_without_scratch_at_the_occupancy_of_their_twins(tmp_path, pair):
    """Both new translation units compile for gfx950 with no spill to scratch, and each window attention kernel has the
    occupancy and the LDS of the kernel without a window of the same <dtype, D, PAGED>."""
    src, twin_src, count = pair
    win, twin = _remarks(src, tmp_path), _remarks(twin_src, tmp_path)
    # (prologue + attention) x 8 + combine x 4, and the plan kernel of the ragged call
    assert len(win) == len(twin) == count, sorted(win)
    assert all(v["ScratchSize [bytes/lane]"] == 0 for v in win.values()), win
    a, b = _attention(win), _attention(twin)
    assert len(a) == len(b) == 8
    for inst, v in sorted(a.items()):
        assert "WindowGeo" in v["name"] and "WindowGeo" not in b[inst]["name"]
        print(inst, "window VGPRs", v["VGPRs"], "twin VGPRs", b[inst]["VGPRs"], "occupancy", v["Occupancy [waves/SIMD]"])
        assert v["Occupancy [waves/SIMD]"] == b[inst]["Occupancy [waves/SIMD]"], (inst, v, b[inst])
        assert v["LDS Size [bytes/block]"] == b[inst]["LDS Size [bytes/block]"], (inst, v, b[inst])
