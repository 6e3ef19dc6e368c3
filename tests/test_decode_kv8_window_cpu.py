"""CPU-only checks of sfa_decode_kv8_window (sliding-window decode over an fp8 KV cache): the symbol and the Python
operator exist beside an unchanged sfa_decode_args and ABI version, the entry point validates its arguments before any
HIP call, the kernel translation unit compiles for gfx950 without scratch (its registers and occupancy are printed beside
those of its twins in decode_kv8_kernel.hip), the reference of tests/kv8_window_ref.py is kv8_ref's where the window does
not bind, the sweep of the GPU file covers its factors pairwise, the window-edge problems keep their structure after the
quantisation to e4m3, and a numpy model of the kernel's addressing tells one-row and one-page slips apart."""
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
import decode_cases as dc
import kv8_ref
import kv8_window_ref as kw

CSRC = os.path.join(ROOT, "starflashattention_amd", "csrc")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


# ---- 1. symbols and surface -----------------------------------------------------------------------------------------

def test_kv8_window_symbol_exported(lib):
    assert "sfa_decode_kv8_window" in _lib.EXPORTED_SYMBOLS
    assert hasattr(lib, "sfa_decode_kv8_window")
    import starflashattention_amd as sfa
    from starflashattention_amd.ops import flash_decode_kv8_window
    assert sfa.flash_decode_kv8_window is flash_decode_kv8_window
    with open(os.path.join(ROOT, "include", "star_flash_attn.h")) as f:
        header = f.read()
    assert "sfa_decode_kv8_window(" in header
    # no sizing function of its own: sfa_decode_window_workspace_bytes serves it
    assert "sfa_decode_kv8_window_workspace_bytes" not in header and not hasattr(lib, "sfa_decode_kv8_window_workspace_bytes")
    # a new symbol beside the same struct and the same ABI version
    assert "#define SFA_ABI_VERSION 4" in header
    assert lib.sfa_abi_version() == 4
    assert ctypes.sizeof(_lib.DecodeArgs) == 10 * 8 + 12 * 4 + 8 + 8 + 8 + 8 + 8 + 8


# ---- 2. argument validation -----------------------------------------------------------------------------------------

def _args():
    a = _lib.DecodeArgs()
    for f in ("qkv", "o", "seq_len", "k_cache_table", "v_cache_table"):
        setattr(a, f, 0x1000)
    a.batch_size, a.num_heads, a.memory_max_len, a.num_layer, a.head_dim = 1, 2, 64, 1, 128
    a.rotary_embedding_dim = 128
    return a


@pytest.mark.skipif(torch.cuda.is_available(), reason="calls sfa_decode_kv8_window with fake device pointers")
def test_decode_kv8_window_argument_validation_without_gpu(lib):
    call = lambda a, w=8, ks=None, vs=None: lib.sfa_decode_kv8_window(ctypes.byref(a) if a is not None else None, ks, vs, w,
                                                                     None)
    err = lambda: lib.sfa_last_error()
    mine = lambda: err().startswith(b"sfa_decode_kv8_window:")
    assert call(None) == -1 and mine()
    assert call(_lib.DecodeArgs()) == -1 and mine()
    a = _args()
    for w in (0, -3):
        assert call(a, w) == -2 and mine() and b"window" in err()
    a.head_dim, a.rotary_embedding_dim = 256, 128
    assert call(a) == -4 and mine() and b"256" in err()
    a.head_dim = 96
    assert call(a) == -4 and mine()
    a.head_dim = 128
    a.dtype = 7
    assert call(a) == -3 and mine()
    a.dtype = 1
    assert call(a, ks=0x5002) == -2 and mine() and b"k_scale" in err()
    assert call(a, ks=0x5000, vs=0x6001) == -2 and mine() and b"v_scale" in err()
    a.num_heads, a.num_heads_kv = 12, 4                         # group of 3
    assert call(a) == -2 and mine() and b"num_heads_kv" in err()
    a.k_cache_table = 0x1008                                    # the byte caches are 16-byte aligned too
    a.num_heads, a.num_heads_kv = 16, 1
    assert call(a) == -2 and b"16-byte aligned" in err()
    a.k_cache_table = 0x1000
    for group in (1, 2, 4, 8, 16):                              # every group up to 16 is served, as far as the workspace
        a.num_heads, a.num_heads_kv = group, 1
        assert call(a) == -1 and err().startswith(b"sfa_decode_kv8_window: workspace is NULL")
        assert call(a, ks=0x5000, vs=0x6000) == -1 and err().startswith(b"sfa_decode_kv8_window: workspace is NULL")
    assert call(a, 1) == -1 and call(a, 2 ** 31 - 1) == -1      # any window >= 1
    a.workspace, a.workspace_bytes, a.num_splits = 0x2000, 256, 2
    assert call(a) == -5 and mine()                             # sfa_decode's workspace: too small for 2 splits
    a.workspace = 0x2010
    a.workspace_bytes = 1 << 30
    assert call(a) == -2 and b"256-byte aligned" in err()
    a.batch_size = 0
    assert call(a) == 0                                         # nothing to do


# ---- 3. the translation unit compiles without scratch ---------------------------------------------------------------

def _resource_usage(source, tmp_path):
    """{template arguments of the kernel: dict(name, vgprs, agprs, scratch, occupancy)} of every kernel of a .hip file"""
    r = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-I" + ROOT,
                        "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, source), "-o",
                        str(tmp_path / (source + ".o"))], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    field = lambda pat: [int(x) for x in re.findall(pat + r": (\d+)", r.stderr)]
    cols = (field(r" VGPRs"), field(r" AGPRs"), field(r"ScratchSize \[bytes/lane\]"), field(r"Occupancy \[waves/SIMD\]"))
    assert all(len(c) == len(names) for c in cols), (len(names), [len(c) for c in cols])
    out = {}
    for nm, v, a, s, occ in zip(names, *cols):
        key = re.search(r"kernelI(NS_4\w{4}ELi\d+ELb[01]ELb[01]E)", nm)
        out[key.group(1) if key else nm] = dict(name=nm, vgprs=v, agprs=a, scratch=s, occupancy=occ)
    return out


def test_kv8_window_kernel_compiles_without_scratch(tmp_path):
    """Every kernel of the new translation unit compiles for gfx950 with no spill to scratch: (fp16, bf16) x (64, 128) x
    (default, non-temporal loads) x (contiguous, paged), the group size a run-time value.  Registers and occupancy are
    printed beside those of the twin in decode_kv8_kernel.hip (the same template arguments without the window); an
    occupancy below the twin's is reported by this test's output and recorded in DESIGN.md 5.13, not asserted."""
    new = _resource_usage("decode_kv8_window_kernel.hip", tmp_path)
    twins = _resource_usage("decode_kv8_kernel.hip", tmp_path)
    assert len(new) == 16 and all("decode_kv8_window_kernel" in k["name"] for k in new.values()), sorted(new)
    attention = {key: k for key, k in twins.items() if "decode_kv8_kernel" in k["name"]}
    assert set(attention) == set(new)
    print("\n%-34s %14s %14s %10s %10s" % ("template arguments", "VGPRs win/twin", "AGPRs win/twin", "occ win", "occ twin"))
    for key in sorted(new):
        k, t = new[key], attention[key]
        print("%-34s %8d / %3d %8d / %3d %10d %10d%s" % (key, k["vgprs"], t["vgprs"], k["agprs"], t["agprs"], k["occupancy"],
                                                       t["occupancy"], "   LOWER" if k["occupancy"] < t["occupancy"] else ""))
    assert all(k["scratch"] == 0 for k in new.values()), {key: k["scratch"] for key, k in new.items()}


# ---- 4. the reference and the sweep ---------------------------------------------------------------------------------

def test_reference_without_a_binding_window_is_kv8_ref():
    """window = None and every window > pos: kv8_ref.decode_kv8_ref, exactly (o, the appended bytes, the caches); a window
    that binds differs, does not look below lo (the NaN byte there changes nothing), and window = 1 returns the
    dequantised new V row."""
    rng = np.random.default_rng(11)
    Bn, H, Hkv, D, L, M, layer, rot = 3, 4, 2, 64, 2, 96, 1, 32
    kc, vc = rng.standard_normal((Bn, L, M, Hkv, D)), rng.standard_normal((Bn, L, M, Hkv, D))
    ks, vs = (np.abs(kc).max(axis=(0, 1, 2, 4)) / 448).astype(np.float32), np.array([0.01, 0.02], np.float32)
    k8, v8 = kv8_ref.quantize(kc, ks), kv8_ref.quantize(vc, vs)
    from oracle import round_to
    qkv = round_to(rng.standard_normal((Bn, H + 2 * Hkv, D)), "fp16")
    bias = [round_to(rng.standard_normal((h, D)) * 0.5, "fp16") for h in (H, Hkv, Hkv)]
    lens = [0, 40, 95]
    okw = dict(k_scale=ks, v_scale=vs, q_bias=bias[0], k_bias=bias[1], v_bias=bias[2])
    a8, b8 = k8.copy(), v8.copy()
    want = kv8_ref.decode_kv8_ref(qkv, a8, b8, lens, layer, rot, "fp16", **okw)
    for window in (None, 96, 97, 5000):
        c8, d8 = k8.copy(), v8.copy()
        got = kw.decode_kv8_window_ref(qkv, c8, d8, lens, layer, rot, "fp16", window, **okw)
        for key in ("o", "k_row", "v_row"):
            np.testing.assert_array_equal(got[key], want[key])
        np.testing.assert_array_equal(c8, a8)
        np.testing.assert_array_equal(d8, b8)
    w = 17
    assert [kw.window_lo(p, w) for p in lens] == [0, 24, 79]
    kp, vp = k8.copy(), v8.copy()
    for b, pos in enumerate(lens):
        kp[b, layer, :kw.window_lo(pos, w)] = vp[b, layer, :kw.window_lo(pos, w)] = dc.NAN8
    a = kw.decode_kv8_window_ref(qkv, k8.copy(), v8.copy(), lens, layer, rot, "fp16", w, **okw)
    p = kw.decode_kv8_window_ref(qkv, kp, vp, lens, layer, rot, "fp16", w, **okw)
    np.testing.assert_array_equal(a["o"], p["o"])
    assert np.isfinite(a["o"]).all() and np.abs(a["o"][2] - want["o"][2]).max() > 0.05
    np.testing.assert_array_equal(a["o"][0], want["o"][0])          # pos 0: the window does not bind
    one = kw.decode_kv8_window_ref(qkv, kp, vp, lens, layer, rot, "fp16", 1, **okw)
    np.testing.assert_allclose(one["o"], np.repeat(kv8_ref.dequantize(one["v_row"], vs), H // Hkv, axis=1), atol=0, rtol=1e-6)


def test_sweep_covers_its_factors_pairwise():
    F = kw.FACTORS
    assert F == (("fp16", "bf16"), (64, 128), ("blmhd", "blhmd", "paged16", "paged64"), (1, 2, 4, 8, 16), (0, 1, 3),
                 (1, 2, 17, 33, 64, 100, 129, 1000, 5000))
    for c in kw.SWEEP:
        assert len(c) == len(F) and all(x in f for x, f in zip(c, F)), c
    for i, j in itertools.combinations(range(len(F)), 2):
        seen = {(c[i], c[j]) for c in kw.SWEEP}
        assert seen == set(itertools.product(F[i], F[j])), (i, j)
    assert (kw.B, kw.HKV, kw.L, kw.M, kw.LENS) == (4, 2, 2, 1408, (0, 5, 130, 1000))


# ---- 5. the window-edge problems keep their structure over the quantised cache ---------------------------------------

EDGE_SHAPES = [(2, 64), (4, 128)]
EDGES = [(dtype, G, D, w) for dtype in ("bf16", "fp16") for G, D in EDGE_SHAPES for w in dc.WINDOWS]
edge_ids = lambda e: f"{e[0]}-G{e[1]}-D{e[2]}-w{e[3]}"


@pytest.fixture(scope="module")
def edges():
    cache = {}

    def get(dtype, G, D, kind, window):
        key = (dtype, G, D, kind, window)
        if key not in cache:
            p = kw.window_edges(dtype, G, D, kind, window)
            cache[key] = (p, kw.oracle(p))
        return cache[key]
    return get


def test_window_edge_problems_are_the_window_suites():
    """the sequences of decode_cases.window_edges (a sequence per lo, pos = lo + window - 1), e4m3 bytes, power-of-two
    scales that differ between the two kv heads, no rotation"""
    assert kw.EDGE_KINDS == ["edge_in", "edge_last", "edge_out", "ramp_through", "ramp", "equal"]
    for window in dc.WINDOWS:
        for kind in kw.EDGE_KINDS:
            p = kw.window_edges("fp16", 1, 64, kind, window)
            los = [lo for lo in dc.WINDOW_LOS if lo + window <= dc.M and (kind != "edge_out" or lo > 0)]
            assert p.entry == "kv8" and p.window == window and p.lo == los and p.rot == 0
            assert p.lens == [lo + window - 1 for lo in los] and p.ns == [1] * p.B
            assert p.kc.dtype == np.uint8 and p.ks[0] != p.ks[1] and np.all(np.log2(p.ks) % 1 == 0)
            assert np.all(np.log2(p.vs) % 1 == 0)
            m = p.unread_mask()
            for b, lo in enumerate(los):
                assert m[b, dc.LAYER, :lo].all() and not m[b, dc.LAYER, lo:p.lens[b] + 1].any()
                assert m[b, dc.LAYER, p.lens[b] + 1:].all() and m[b, 1 - dc.LAYER].all()


@pytest.mark.parametrize("edge", EDGES, ids=edge_ids)
def test_window_edge_spikes_carry_the_weight_after_quantisation(edges, edge):
    """Over the quantised cache: edge_in -- row lo, edge_last -- row pos - 1 has >= 0.99 of the fp64 weight in every
    head; edge_out -- row lo - 1 holds finite bytes, has no weight, would have >= 0.99 of it if the mask let it through,
    and a kernel that saw it would be wrong by more than 10 tolerances in at least half of the elements."""
    dtype, G, D, window = edge
    for kind, row_of in (("edge_in", lambda lo, pos: lo), ("edge_last", lambda lo, pos: pos - 1)):
        p, ref = edges(dtype, G, D, kind, window)
        assert np.isfinite(ref["o"]).all()
        for b in range(p.B):
            row = row_of(p.lo[b], p.lens[b])
            assert p.hot[b] == p.spike[b] == row and p.lo[b] <= row < p.lens[b]
            assert dc.weights(p, ref, b)[:, row].min() >= 0.99, (kind, b)
    p, ref = edges(dtype, G, D, "edge_out", window)
    seen = kw.oracle(p, window=window + 1)["o"]                               # the oracle over [lo - 1, pos]
    for b in range(p.B):
        lo = p.lo[b]
        assert lo >= 1 and p.spike[b] == lo - 1 and p.hot[b] == -1
        assert np.isfinite(p.values(p.kc[b, dc.LAYER, lo - 1], p.ks)).all()
        assert np.isfinite(p.values(p.vc[b, dc.LAYER, lo - 1], p.vs)).all()
        assert dc.weights(p, ref, b)[:, lo - 1].max() == 0.0
        assert dc.weights(p, ref, b, causal=False)[:, lo - 1].min() >= 0.99
        far = np.abs(seen[b] - ref["o"][b]) > 10 * kw.elementwise_tol(p, ref["o"][b])
        assert far.mean() >= 0.5, (b, far.mean())


@pytest.mark.parametrize("edge", EDGES, ids=edge_ids)
def test_window_equal_marks_every_one_row_slip_after_quantisation(edges, edge):
    """equal, over the quantised cache: o is the mean of the dequantised V over exactly rows lo .. pos, and each one-row
    slip -- row lo dropped, row lo counted twice, row lo - 1 added, row pos - 1 dropped -- differs from it by more than 5
    times the elementwise tolerance in at least half of the elements, for every sequence."""
    dtype, G, D, window = edge
    p, ref = edges(dtype, G, D, "equal", window)
    seen = 0
    for b in range(p.B):
        lo, pos = p.lo[b], p.lens[b]
        V = np.repeat(p.values(ref["vc"][b, dc.LAYER, :pos + 1], p.vs), p.G, axis=1)     # [pos + 1, H, D]
        want = ref["o"][b]
        np.testing.assert_allclose(want, V[lo:].mean(axis=0), atol=1e-6, rtol=1e-6)
        rows = list(range(lo, pos + 1))
        wrong = {"lo dropped": rows[1:], "lo twice": [lo] + rows, "pos - 1 dropped": rows[:-2] + rows[-1:]}
        if lo >= 1:
            wrong["lo - 1 added"] = [lo - 1] + rows
        for name, rr in wrong.items():
            far = np.abs(V[rr].mean(axis=0) - want) > 5 * kw.elementwise_tol(p, want)
            assert far.mean() >= 0.5, (name, b, far.mean())
            seen += 1
    assert seen == 4 * p.B - 1                                                   # (lo = 0 has no row below it)


@pytest.mark.parametrize("edge", EDGES, ids=edge_ids)
def test_window_ramps_are_as_named_after_quantisation(edges, edge):
    """ramp_through: the largest score of [lo, pos] is at row lo in every head, the scores never rise from there on, and
    every row below lo scores at least as high as row lo (e4m3 has 3 mantissa bits: neighbouring rows of the ramp tie,
    row lo - 1 with row lo among them; the model test below shows that a kernel which saw row lo - 1 still leaves the
    tolerance).  ramp: the row max over the 32-key tiles of the window (from lo & ~31, as the kernel cuts them) strictly
    increases from tile to tile -- up to the last tile, which may tie with the one before it: the top eighth of the ramp
    is one e4m3 value -- and the rows below lo are zeros."""
    dtype, G, D, window = edge
    p, ref = edges(dtype, G, D, "ramp_through", window)
    for b in range(p.B):
        lo = p.lo[b]
        sc = dc.scores_log2(p, ref, b, causal=False)                           # [H, pos + 1], nothing masked
        assert p.ramp[b] == -1
        assert np.all(sc[:, lo:].max(axis=1) == sc[:, lo])
        assert np.all(sc[:, :lo] >= sc[:, lo:lo + 1])
        assert np.all(np.diff(sc[:, lo:], axis=1) <= 0)                        # (e4m3 steps tie)
    p, ref = edges(dtype, G, D, "ramp", window)
    for b in range(p.B):
        lo, pos = p.lo[b], p.lens[b]
        assert p.ramp[b] == 1 and not p.kc[b, dc.LAYER, :lo].any()
        masked = dc.scores_log2(p, ref, b)
        tiles = np.stack([masked[:, t:t + 32].max(axis=1) for t in range(lo & ~31, pos + 1, 32)], axis=1)
        assert tiles.shape[1] >= 2 or window <= 32 - (lo & 31)
        d = np.diff(tiles, axis=1)
        assert np.all(d[:, :-1] > 0) and np.all(d[:, -1:] >= 0), (b, tiles)


# ---- 6. a model of the kernel's addressing, and what one-line slips of it do ----------------------------------------

@pytest.mark.parametrize("window", dc.WINDOWS, ids=lambda w: f"w{w}")
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_window_edge_problems_tell_one_row_slips_apart(edges, dtype, window):
    """The model without a slip is the oracle on every window-edge problem.  With one, the sequences it puts outside the
    GPU file's elementwise tolerance are exactly: mask too narrow -- every sequence of edge_in, edge_out, equal and
    ramp_through; mask too wide -- every lo that is no multiple of 32 in edge_out, equal and ramp_through (the doubled
    row already has all the weight in edge_in); window too long -- every lo >= 1 of the same three; first page one too
    high (paged) -- every lo that is no multiple of 16 in edge_in, edge_out, equal and ramp_through.  edge_last sees none
    of them; the ascending ramp leaves the tolerance under some slips at some windows only and is asserted on the model
    without a slip alone."""
    G, D = 2, 64
    off32, off16, pos1 = (lambda lo: lo % 32 != 0), (lambda lo: lo % 16 != 0), (lambda lo: lo >= 1)
    all_, none = (lambda lo: True), (lambda lo: False)
    want = {None: dict(edge_in=none, edge_out=none, equal=none, ramp_through=none, ramp=none),
            "narrow": dict(edge_in=all_, edge_out=all_, equal=all_, ramp_through=all_),
            "wide": dict(edge_in=none, edge_out=off32, equal=off32, ramp_through=off32),
            "long": dict(edge_in=none, edge_out=pos1, equal=pos1, ramp_through=pos1),
            "page": dict(edge_in=off16, edge_out=off16, equal=off16, ramp_through=off16)}
    for kind in kw.EDGE_KINDS:
        p, ref = edges(dtype, G, D, kind, window)
        for slip, kinds in want.items():
            for paged in (False, True) if slip != "page" else (True,):
                got = kw.addressing_model(p, ref, slip, paged)
                out = (np.abs(got - ref["o"]) > kw.elementwise_tol(p, ref["o"])).any(axis=(1, 2))
                if slip is None:
                    np.testing.assert_allclose(got, ref["o"], atol=1e-6, rtol=1e-6)
                if kind == "edge_last":
                    assert not out.any(), (slip, paged)
                elif kind in kinds:
                    hit = [kinds[kind](lo) for lo in p.lo]
                    assert out.tolist() == hit, (kind, slip, paged, out.tolist())
