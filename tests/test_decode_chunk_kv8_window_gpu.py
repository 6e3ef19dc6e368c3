"""GPU checks of sfa_decode_chunk_kv8_window (the sliding window in the multi-token decode step over an fp8 e4m3 KV cache)
through the Python operator and the C ABI: parity with the reference of tests/chunk_kv8_window_ref.py over a
pairwise-covering sweep, bit-identity with sfa_decode_chunk_kv8 where the window does not bind, agreement with n
successive sfa_decode_kv8_window calls, the window's edges, the promise that no byte outside [lo_0, pos + n) is read
(0x7F, the e4m3 NaN, in all of them), the scales, rejection, the workspace and graph replay.

How o is checked is how tests/test_decode_chunk_kv8_gpu.py checks it (chunk_kv8_window_ref.check): (a) the appended bytes
against the reference quantiser -- V exact, K within one e4m3 step and > 98 % identical per call, every other byte of
both caches unchanged -- and (b) o against fp64 attention over the bytes the device stored, at the project's decode
tolerances unchanged (fp16 2e-3, bf16 1.6e-2, atol = rtol, elementwise, nothing exempt).  The common frame: B = 4
sequences at seq_len = [0, 5, 130, 1000], 2 kv heads, 2 layers, memory_max_len 1408, q / k / v bias and a partial rotary
embedding.
"""
import ctypes

import numpy as np
import pytest
import torch

import chunk_kv8_window_ref as ref
import kv8_ref
from chunk_kv8_window_ref import (EDGE_N, EDGE_WINDOWS, HKV, L, LAYER, LENS, M, SWEEP, TOL, append_mask, check,
                                  edge_problem, make_problem, page_table, poisoned, poisoned_table, problem, run, same_bits,
                                  spike_rows, window_lo)
from chunk_window_ref import TDT, bits
from oracle import round_to

pytestmark = pytest.mark.gpu

VARLEN = False                                  # tests/test_decode_varlen_kv8_window_gpu.py runs these through the packed call


@pytest.fixture(scope="module")
def sfa():
    assert torch.cuda.is_available(), "GPU tests need a GPU (run with -m gpu on the MI355X box)"
    import starflashattention_amd as m
    m._lib.load()                  # fail loudly if the HIP library is missing
    return m


def status_word(sfa):
    from starflashattention_amd import ops
    dev = torch.device("cuda:0")
    ws = ops._workspaces[(dev.index, torch.cuda.current_stream(dev).cuda_stream)]
    torch.cuda.synchronize()
    return int(ws[:4].view(torch.int32).item())


def same_appends(r, other, p, lens=None):
    m = ~append_mask(p, lens)
    return np.array_equal(r.k8[m], other.k8[m]) and np.array_equal(r.v8[m], other.v8[m])


# ---- parity ------------------------------------------------------------------------------------------------------------

def parity_case(sfa, case, varlen):
    i, (dtype, D, layout, G, num_splits, window, n) = case
    # The rotary tables: the device and the reference rotate with the same cos / sin, which criterion (a) needs at the
    # frame's long positions (chunk_kv8_window_ref.check).  Every other case runs a second time with the trigonometry
    # computed in the kernel: (b), V and the untouched bytes as before, the appended K bytes against the plain call's.
    for tables in (True, False) if i % 2 == 0 else (True,):
        p = problem(dtype, D, G, n, tables)
        r = run(sfa, p, layout, window, num_splits, varlen=varlen)
        sfa.check_decode_status()
        check(r, p, window, ref.frame_reference(dtype, D, G, n, window, tables), k_bytes=tables)
        # the prologue is shared: at every window the appended bytes are those of the call without one
        plain = run(sfa, p, "blmhd", None, 1, varlen=varlen)
        assert same_appends(r, plain, p)
        if r.spare_k is not None:
            assert bool((r.spare_k == ref.FILL).all()) and bool((r.spare_v == ref.FILL).all())


@pytest.mark.parametrize("case", list(enumerate(SWEEP)), ids=lambda c: "-".join(str(x) for x in c[1]))
def test_chunk_kv8_window_parity_sweep(sfa, case):
    parity_case(sfa, case, VARLEN)


def window_binds_case(sfa, dtype, varlen):
    D, G, n, window = 128, 4, 40, 100
    p = problem(dtype, D, G, n, True)
    win, full = ref.frame_reference(dtype, D, G, n, window, True), ref.frame_reference(dtype, D, G, n, None, True)
    b = LENS.index(1000)
    tol = TOL[dtype]
    gap = np.abs(win[0]["o"][b] - full[0]["o"][b]).max()
    assert gap > 10 * tol * (1.0 + np.abs(full[0]["o"][b]).max()), gap
    r = run(sfa, p, "blmhd", window, varlen=varlen)
    sfa.check_decode_status()
    check(r, p, window, win)
    print("device against the full-history reference: %.3f (bar %.3f)" % (np.abs(r.of[b] - full[0]["o"][b]).max(), 5 * tol))
    assert np.abs(r.of[b] - full[0]["o"][b]).max() > 5 * tol


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_chunk_kv8_window_binds(sfa, dtype):
    """pos = 1000, window = 100: the windowed and the full reference differ by many tolerances (the factor is asserted on
    the CPU as well), and the device sides with the windowed one."""
    window_binds_case(sfa, dtype, VARLEN)


def not_binding_case(sfa, layout, num_splits, varlen):
    for dtype, D, G, n in (("bf16", 128, 8, 45), ("fp16", 64, 1, 70), ("fp16", 128, 2, 5)):
        p = problem(dtype, D, G, n)
        full = run(sfa, p, layout, None, num_splits, varlen=varlen)
        for window in (max(LENS) + n, 5000):
            r = run(sfa, p, layout, window, num_splits, varlen=varlen)
            sfa.check_decode_status()
            assert same_bits(r, full), (dtype, D, G, window)


@pytest.mark.parametrize("num_splits", [1, 3])
@pytest.mark.parametrize("layout", ["blmhd", "blhmd", "paged16", "paged64"])
def test_chunk_kv8_window_bit_identical_to_chunk_kv8_where_it_does_not_bind(sfa, layout, num_splits):
    """window >= pos + n for every sequence: lo = 0 everywhere, the same tile partition, the same bits in o and in both
    caches"""
    not_binding_case(sfa, layout, num_splits, VARLEN)


@pytest.mark.parametrize("window", [1, 33, 100])
def test_chunk_kv8_window_against_successive_decode_kv8_window_calls(sfa, window):
    """n successive sfa_decode_kv8_window calls on the device, seq_len advanced by one each time: the same appended bytes
    bit for bit and the same outputs within tolerance.  The calls read the rotary tables, so that both kernels rotate with
    the same cos / sin (their own trigonometry may differ in the last bit of an angle, which can move a K byte)."""
    dtype, D, G, n, layout = "bf16", 128, 4, 40, "paged16"
    p = problem(dtype, D, G, n, True)
    r = run(sfa, p, layout, window, varlen=VARLEN)
    sfa.check_decode_status()
    dev = torch.device("cuda:0")
    dt = TDT[dtype]
    t16 = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dt).to(dev)
    kd, vd = ref.to_layout(p.k8, layout).to(dev), ref.to_layout(p.v8, layout).to(dev)
    table = torch.from_numpy(page_table(16, p.B)[0]).to(dev)
    cos, sin = ref.rotary_tables(dtype, p.rot)
    kw = dict(kv_layout="paged", block_table=table, num_heads_kv=HKV, rotary_cos_table=t16(cos), rotary_sin_table=t16(sin),
              k_scale=torch.from_numpy(p.ks).to(dev), v_scale=torch.from_numpy(p.vs).to(dev))
    tok = t16(np.stack(p.tok))
    held = [t16(x) for x in p.biases]
    o = torch.empty(p.B, n, p.H, D, dtype=dt, device=dev)
    for t in range(n):
        sl = torch.tensor([pos + t for pos in LENS], dtype=torch.int32, device=dev)
        ot = torch.empty(p.B, p.H, D, dtype=dt, device=dev)
        sfa.flash_decode_kv8_window(tok[:, t].contiguous(), *held, kd, vd, sl, ot, p.B, M, p.H, D, p.rot, M, L, LAYER, window,
                                    **kw)
        o[:, t] = ot
    torch.cuda.synchronize()
    sfa.check_decode_status()
    np.testing.assert_array_equal(ref.from_layout(kd, layout, p.B)[0], r.k8)
    np.testing.assert_array_equal(ref.from_layout(vd, layout, p.B)[0], r.v8)
    tol = TOL[dtype]
    for b in range(p.B):
        np.testing.assert_allclose(r.of[b], o[b].float().cpu().numpy(), atol=tol, rtol=tol)


# ---- the window's edges ------------------------------------------------------------------------------------------------

EDGE_LAYOUTS = {17: "paged16", 32: "blmhd", 40: "blhmd", 100: "paged64"}


def edges_case(sfa, window, num_splits, varlen):
    layout = EDGE_LAYOUTS[window]
    for dtype in ("fp16", "bf16"):
        spike = edge_problem(dtype, window, "spike")
        r = run(sfa, spike, layout, window, num_splits, varlen=varlen)
        sfa.check_decode_status()
        ref3 = ref.edge_reference(window, "spike")
        check(r, spike, window, ref3)
        np.testing.assert_array_equal(r.k8, ref3[1])            # nothing rounds: the reference's bytes
        np.testing.assert_array_equal(r.v8, ref3[2])
        for b, (pos, jstar) in enumerate(spike_rows(window)):
            # the bits of v_scale * V8[j*] in the 16-bit dtype (G = 1: head h reads kv head h)
            vstar = round_to(kv8_ref.dequantize(r.v8[b, LAYER, jstar], spike.vs), dtype).astype(np.float32)
            seen = 0
            for t in range(EDGE_N):
                if window_lo(pos + t, window) <= jstar <= pos + t:
                    assert np.array_equal(r.of[b][t], vstar), (dtype, b, t)
                    seen += 1
                else:
                    assert not np.array_equal(r.of[b][t], vstar), (dtype, b, t)
            assert seen >= min(window, 17)
        for kind in ("equal", "ramp"):
            p = edge_problem(dtype, window, kind)
            r = run(sfa, p, layout, window, num_splits, varlen=varlen)
            sfa.check_decode_status()
            check(r, p, window, ref.edge_reference(window, kind))


@pytest.mark.parametrize("num_splits", [1, 3, 4])
@pytest.mark.parametrize("window", EDGE_WINDOWS)
def test_chunk_kv8_window_edges(sfa, window, num_splits):
    """rotary_embedding_dim = 0 and no bias, one sequence per lo_0 in {0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128,
    129}, G = 1 and 300 tokens (two q-tiles), every cache value and new row exact in e4m3 under power-of-two scales:
      (a) a key that carries all the weight at row j*: every token that sees it returns the bits of v_scale * V8[j*], the
          first token with lo_t = j* + 1 does not (it is the first / last row of a wave, the first row of the second
          q-tile, or has lo_t on a 64-key / 32-key boundary);
      (b) all keys equal, V rows of alternating, marked magnitude: one row dropped, added or counted twice at either edge
          of any token's window leaves the tolerance (asserted on the CPU from the reference alone);
      (c) a ramp of scores that keeps rising below lo_t."""
    edges_case(sfa, window, num_splits, VARLEN)


# ---- what the window promises not to read ------------------------------------------------------------------------------

# lo_0 on a 64-row tile boundary, on a 32-row boundary, on a page boundary (16 rows; 64 rows is the tile), and beside each
UNREAD_LO0 = (127, 128, 129, 95, 96, 97, 79, 80, 81)
UNREAD_WINDOW, UNREAD_N = 100, 40


@pytest.fixture(scope="module")
def unread_problems():
    lens = tuple(lo + UNREAD_WINDOW - 1 for lo in UNREAD_LO0)
    return {D: make_problem(dt, D, 4, lens, (UNREAD_N,) * len(lens), seed=9, tables=True)
            for D, dt in ((64, "fp16"), (128, "bf16"))}


def unread_memory_case(sfa, p, window, layout, num_splits, varlen):
    """The same call on benign bytes with a valid table, and with 0x7F in every byte of both caches outside
    [lo_0, pos + n) of idx_layer -- the rows below lo_0, the rows from pos + n on, the other layer, the spare pages -- and
    -1 in the block_table entries [0, lo_0 / page_size) and past the last page needed: o and the appended rows bit for
    bit, the status word SFA_OK, every poisoned byte still in place."""
    sfa.check_decode_status()
    clean = run(sfa, p, layout, window, num_splits, varlen=varlen)
    assert status_word(sfa) == 0
    pk, pv = poisoned(p.k8, p, window), poisoned(p.v8, p, window)
    assert (pk == 0x7F).mean() > 0.9
    ps = ref.page_size(layout)
    table = None
    if ps:
        table = poisoned_table(p, window, ps)
        assert (table == -1).sum() > p.B * (M // ps) * 0.8
    r = run(sfa, p, layout, window, num_splits, varlen=varlen, k8=pk, v8=pv, table=table, fill=0x7F)
    assert status_word(sfa) == 0
    sfa.check_decode_status()
    for a, c in zip(r.o, clean.o):
        assert bool(torch.isfinite(a.view(TDT[p.dtype]).float()).all())
        assert torch.equal(a, c)
    assert same_appends(r, clean, p)
    m = append_mask(p)
    assert np.array_equal(r.k8[m], pk[m]) and np.array_equal(r.v8[m], pv[m])       # the poison, and the rest
    if ps:
        assert bool((r.spare_k == 0x7F).all()) and bool((r.spare_v == 0x7F).all())
    return clean


@pytest.mark.parametrize("num_splits", [1, 3])
@pytest.mark.parametrize("layout", ["blmhd", "blhmd", "paged16", "paged64"])
@pytest.mark.parametrize("D", [64, 128])
def test_chunk_kv8_window_reads_nothing_outside_it(sfa, unread_problems, D, layout, num_splits):
    """head_dim 64 (8-byte chunks, fp16) and 128 (16-byte chunks, bf16), pages of 16 and 64 rows and both contiguous
    layouts, lo_0 in {127, 128, 129, 95, 96, 97, 79, 80, 81}: a masked key has weight 0, but 0 x NaN is NaN in P.V, so the
    rows below the window must be re-addressed, not only masked."""
    p = unread_problems[D]
    assert tuple(window_lo(pos, UNREAD_WINDOW) for pos in p.lens) == UNREAD_LO0
    clean = unread_memory_case(sfa, p, UNREAD_WINDOW, layout, num_splits, VARLEN)
    if layout == "blmhd" and num_splits == 1:                   # and the clean run is the right answer
        check(clean, p, UNREAD_WINDOW, ref.reference(p, UNREAD_WINDOW))


@pytest.mark.parametrize("window", [1, 16, 17])
def test_chunk_kv8_window_reads_nothing_outside_it_in_the_frame(sfa, window):
    """the frame's sequences (lo_0 = 0 among them, and pos = 1000 with most of the table freed) at short windows"""
    p = problem("bf16", 128, 4, 40)
    for layout, num_splits in (("paged16", 3), ("paged64", 1), ("blhmd", 1)):
        unread_memory_case(sfa, p, window, layout, num_splits, VARLEN)


# ---- the scales and the variants -----------------------------------------------------------------------------------------

def scales_case(sfa, varlen):
    n, window = 45, 64
    p = make_problem("bf16", 128, 4, LENS, (n,) * 4, seed=6, k_factors=(0.5, 0.037), tables=True)
    assert len(set(p.ks.tolist()) | set(p.vs.tolist())) == 4                      # four distinct scales
    ref3 = ref.reference(p, window)
    for layout, num_splits in (("blmhd", 1), ("blhmd", 3)):
        r = run(sfa, p, layout, window, num_splits, varlen=varlen)
        sfa.check_decode_status()
        check(r, p, window, ref3)


def test_chunk_kv8_window_distinct_scales_per_head(sfa):
    scales_case(sfa, VARLEN)


def null_scales_case(sfa, num_splits, varlen):
    # (scale 1.0: the subnormal e4m3 step, 2^-9, is above what in-kernel trigonometry moves a k element by)
    p = make_problem("bf16", 128, 4, LENS, (5,) * 4, seed=7, with_scales=False)
    assert p.ks is None
    a = run(sfa, p, "blmhd", 33, num_splits, varlen=varlen)
    sfa.check_decode_status()
    check(a, p, 33, ref.reference(p, 33))
    p.ks, p.vs = np.ones(HKV, np.float32), np.ones(HKV, np.float32)
    b = run(sfa, p, "blmhd", 33, num_splits, varlen=varlen)
    p.ks = p.vs = None
    assert same_bits(a, b)                                      # bit for bit


@pytest.mark.parametrize("num_splits", [1, 3])
def test_chunk_kv8_window_null_scales_equal_ones(sfa, num_splits):
    null_scales_case(sfa, num_splits, VARLEN)


VARIANT_LENS = (0, 5, 130, 200)


def variants_case(sfa, variant, dtype, varlen):
    kw = {"softmax_scale": dict(scale=0.05), "bias": dict(bias=True, rot=0), "tables": dict(tables=True, rot=128),
          "partial_rotary": dict(rot=64), "partial_rotary_tables": dict(rot=64, tables=True), "rot0": dict(rot=0)}[variant]
    kw.setdefault("bias", False)
    # positions up to 205: where the variant computes cos / sin in the kernel, the angle is within 2.5e-5 rad of numpy's
    p = make_problem(dtype, 128, 4, VARIANT_LENS, (5,) * 4, seed=8, **kw)
    window = 33
    ref3 = ref.reference(p, window)
    for layout, num_splits in (("blmhd", 1), ("paged16", 3)):
        r = run(sfa, p, layout, window, num_splits, varlen=varlen)
        sfa.check_decode_status()
        check(r, p, window, ref3)


@pytest.mark.parametrize("variant", ["softmax_scale", "bias", "tables", "partial_rotary", "partial_rotary_tables", "rot0"])
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_chunk_kv8_window_variants(sfa, variant, dtype):
    variants_case(sfa, variant, dtype, VARLEN)


def test_chunk_kv8_window_float8_tensors(sfa):
    """torch.float8_e4m3fn caches: the bits of the uint8 call"""
    p = problem("bf16", 128, 4, 5)
    a = run(sfa, p, "paged16", 33, 2, varlen=VARLEN)
    b = run(sfa, p, "paged16", 33, 2, varlen=VARLEN, as_fp8=True)
    sfa.check_decode_status()
    assert same_bits(a, b)


# ---- rejection: the library's handled paths (status word, NaN outputs; nothing here is dereferenced) -----------------------

def rejection_case(sfa, varlen):
    """pos + n > M, a negative pos and a bad page under new rows: NaN, the sequence's cache untouched, the chunk call's
    status; the other sequences as they were"""
    dtype, D, G, n, window = "bf16", 128, 4, 40, 100
    p = problem(dtype, D, G, n)
    sfa.check_decode_status()
    good = run(sfa, p, "blmhd", window, varlen=varlen)
    assert status_word(sfa) == 0
    lens = (0, M - n + 1, 130, -1)
    r = run(sfa, p, "blmhd", window, varlen=varlen, lens=lens)
    assert status_word(sfa) == 1
    with pytest.raises(sfa.SfaError, match="seq_len") as e:
        sfa.check_decode_status()
    assert e.value.status == sfa._lib.SFA_ERR_SEQ_LEN_RANGE
    for b in (1, 3):
        assert np.isnan(r.of[b]).all()
    m = append_mask(p, (0, -1, 130, -1))
    assert np.array_equal(r.k8[m], p.k8[m]) and np.array_equal(r.v8[m], p.v8[m])
    assert torch.equal(r.o[0], good.o[0]) and torch.equal(r.o[2], good.o[2])
    assert np.array_equal(r.k8[~m], good.k8[~m]) and np.array_equal(r.v8[~m], good.v8[~m])
    # a page under new rows of sequence 2 (rows 130 .. 169) outside the pool
    ps = 16
    table = page_table(ps, p.B)[0].copy()
    table[2, 150 // ps] = -7
    goodp = run(sfa, p, "paged16", window, varlen=varlen)
    sfa.check_decode_status()
    r = run(sfa, p, "paged16", window, varlen=varlen, table=table)
    assert status_word(sfa) == 2
    with pytest.raises(sfa.SfaError, match="block_table") as e:
        sfa.check_decode_status()
    assert e.value.status == sfa._lib.SFA_ERR_BLOCK_TABLE_RANGE
    assert np.isnan(r.of[2]).all()
    m = append_mask(p, (0, 5, -1, 1000))        # nothing of sequence 2 was written, anywhere in the pools
    assert np.array_equal(r.k8[m], p.k8[m]) and np.array_equal(r.v8[m], p.v8[m])
    assert bool((r.spare_k == ref.FILL).all()) and bool((r.spare_v == ref.FILL).all())
    for b in (0, 1, 3):
        assert torch.equal(r.o[b], goodp.o[b])
    sfa.check_decode_status()                   # the flag was cleared by the raise


def bad_read_page_case(sfa, num_splits, varlen):
    """a bad entry on a read page inside the window: NaN for that sequence, the status, nothing stored through it; the same
    entry on a page wholly below lo_0: no status, finite outputs, the bits of the clean run"""
    dtype, D, G, n, window, ps = "fp16", 128, 8, 40, 100, 16
    p = problem(dtype, D, G, n)
    b, lo = LENS.index(1000), window_lo(1000, window)
    _, npages = page_table(ps, p.B)
    sfa.check_decode_status()
    clean = run(sfa, p, "paged16", window, num_splits, varlen=varlen)
    assert status_word(sfa) == 0
    inside = page_table(ps, p.B)[0].copy()
    inside[b, lo // ps + 1] = npages            # a page the window reads and no token appends to
    r = run(sfa, p, "paged16", window, num_splits, varlen=varlen, table=inside)
    assert status_word(sfa) == 2
    with pytest.raises(sfa.SfaError, match="block_table"):
        sfa.check_decode_status()
    assert np.isnan(r.of[b]).all()
    assert all(torch.equal(r.o[i], clean.o[i]) for i in range(b))
    # reads only: the same appends, and every byte of the pools but those rows as it was (the spare pages included)
    assert np.array_equal(r.k8, clean.k8) and np.array_equal(r.v8, clean.v8)
    assert bool((r.spare_k == ref.FILL).all()) and bool((r.spare_v == ref.FILL).all())
    below = page_table(ps, p.B)[0].copy()
    below[b, lo // ps - 1] = npages             # the last page wholly below lo_0: never looked at
    below[b, 0] = -1
    r = run(sfa, p, "paged16", window, num_splits, varlen=varlen, table=below)
    assert status_word(sfa) == 0
    sfa.check_decode_status()
    assert all(np.isfinite(x).all() for x in r.of)
    assert same_bits(r, clean)


def test_chunk_kv8_window_rejects_like_chunk_kv8(sfa):
    rejection_case(sfa, VARLEN)


@pytest.mark.parametrize("num_splits", [1, 3])
def test_chunk_kv8_window_bad_table_entry_inside_and_below_the_window(sfa, num_splits):
    bad_read_page_case(sfa, num_splits, VARLEN)


def test_chunk_kv8_window_bad_arguments(sfa):
    p = problem("fp16", 64, 2, 5)
    for w in (0, -3):
        with pytest.raises(sfa.SfaError, match="window") as e:
            run(sfa, p, "blmhd", w, varlen=VARLEN)
        assert e.value.status == -2
    # head_dim 256: SFA_ERR_UNSUPPORTED_HEAD_DIM (-4)
    dev = torch.device("cuda:0")
    B, H, D, n = 1, 2, 256, 2
    qkv = torch.zeros(B, n, 3, H, D, dtype=torch.float16, device=dev)
    kc = torch.zeros(B, 1, 64, H, D, dtype=torch.uint8, device=dev)
    o = torch.zeros(B, n, H, D, dtype=torch.float16, device=dev)
    sl = torch.zeros(B, dtype=torch.int32, device=dev)
    with pytest.raises(sfa.SfaError) as e:
        sfa.flash_decode_chunk_kv8_window(qkv, None, None, None, kc, kc.clone(), sl, o, B, 64, H, D, 0, 64, 1, 0, 8)
    assert e.value.status == -4


# ---- the workspace -------------------------------------------------------------------------------------------------------

def c_abi_call(sfa, p, window, varlen):
    """the tensors and the filled sfa_decode_args of one call on blmhd caches through the C ABI itself:
    (args, call(args, stream), read() -> a result like run()'s)"""
    from types import SimpleNamespace
    from starflashattention_amd import _lib, ops
    dev = torch.device("cuda:0")
    dt = TDT[p.dtype]
    t16 = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dt).to(dev)
    n, T = p.ns[0], sum(p.ns)
    kd, vd = torch.from_numpy(p.k8).to(dev), torch.from_numpy(p.v8).to(dev)
    sl = torch.tensor(list(p.lens), dtype=torch.int32, device=dev)
    held = [t16(x) for x in p.biases]
    ks, vs = torch.from_numpy(p.ks).to(dev), torch.from_numpy(p.vs).to(dev)
    cu = torch.from_numpy(np.concatenate([[0], np.cumsum(p.ns)]).astype(np.int32)).to(dev)
    lead = (T,) if varlen else (p.B, n)
    qkv = t16(np.concatenate(p.tok) if varlen else np.stack(p.tok)).view(lead + (p.H + 2 * HKV, p.D))
    o = torch.full(lead + (p.H, p.D), 7.0, dtype=dt, device=dev)
    a, *_ = ops._decode_args(qkv, *held, kd, vd, sl, o, p.B, M, p.H, p.D, p.rot, M, L, LAYER, None, None, None, "blmhd", None,
                             HKV, kv8=True, **(dict(packed=T) if varlen else dict(tokens=n)))
    a.stride = 0
    lib = _lib.load()
    P = ctypes.c_void_p
    if varlen:
        call = lambda args, stream: lib.sfa_decode_varlen_kv8_window(args, P(ks.data_ptr()), P(vs.data_ptr()),
                                                                      P(cu.data_ptr()), T, 0, window, stream)
    else:
        call = lambda args, stream: lib.sfa_decode_chunk_kv8_window(args, P(ks.data_ptr()), P(vs.data_ptr()), n, 0, window,
                                                                     stream)

    def read():
        ob = bits(o.cpu()).view(p.B, n, p.H, p.D)
        return SimpleNamespace(o=[ob[b] for b in range(p.B)], k8=kd.cpu().numpy(), v8=vd.cpu().numpy())
    keep = (qkv, kd, vd, sl, held, ks, vs, cu, o)
    return a, call, read, keep


def workspace_case(sfa, varlen):
    from exact_workspace import call_with_exact_workspace
    from starflashattention_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda:0")
    dtype, D, G, n = "bf16", 128, 4, 40
    p = problem(dtype, D, G, n)
    count = n * p.B if varlen else n
    sizer = lib.sfa_decode_varlen_window_workspace_bytes if varlen else lib.sfa_decode_chunk_window_workspace_bytes
    plain = lib.sfa_decode_varlen_workspace_bytes if varlen else lib.sfa_decode_chunk_workspace_bytes
    shape = (p.B, p.H, HKV, D, M, count)
    # (1) an explicit split count with a window so short (17 rows over 40 tokens: two key tiles) that splits are empty, in
    #     a workspace of exactly the windowed sizing function's bytes, every fp32 of it a NaN beforehand
    window, S = 17, 4
    want = run(sfa, p, "blmhd", window, S, varlen=varlen)
    sfa.check_decode_status()
    a, call, read, keep = c_abi_call(sfa, p, window, varlen)
    nbytes = sizer(*shape, window, S)
    assert nbytes == plain(*shape, S)
    call_with_exact_workspace(a, nbytes, S, call, dev, fill=0xFF)
    assert same_bits(read(), want)
    # (2) num_splits = 0 where the rule picks two splits (window 5000: the rule sees all 1408 rows), in a workspace sized
    #     for one: the largest count the workspace holds, so the bits of num_splits = 1
    window = 5000
    assert sizer(*shape, window, 0) == plain(*shape, 2) > plain(*shape, 1)
    want1, want2 = (run(sfa, p, "blmhd", window, s, varlen=varlen) for s in (1, 2))
    sfa.check_decode_status()
    a, call, read, keep = c_abi_call(sfa, p, window, varlen)
    call_with_exact_workspace(a, plain(*shape, 1), 0, call, dev, fill=0xFF)
    assert same_bits(read(), want1)
    # (3) num_splits = 0 in a workspace sized by the function without a window: never too small
    for window, want in ((5000, want2), (17, run(sfa, p, "blmhd", 17, 1, varlen=varlen))):
        assert sizer(*shape, window, 0) <= plain(*shape, 0)
        a, call, read, keep = c_abi_call(sfa, p, window, varlen)
        call_with_exact_workspace(a, plain(*shape, 0), 0, call, dev, fill=0xFF)
        assert same_bits(read(), want)


def test_chunk_kv8_window_workspaces_through_the_c_abi(sfa):
    workspace_case(sfa, VARLEN)


# ---- graph replay ------------------------------------------------------------------------------------------------------

def test_chunk_kv8_window_graph_replay(sfa):
    """One captured flash_decode_chunk_kv8_window call, replayed with two different seq_len (and tensor) contents: lo is
    computed on the device, so both replays are correct."""
    from types import SimpleNamespace
    dtype, D, G, n, window = "fp16", 128, 2, 40, 33
    dev = torch.device("cuda:0")
    probs = [make_problem(dtype, D, G, lens, (n,) * 4, seed=s, k_factors=f, tables=True)
             for s, lens, f in ((1, (3, 700, 64, 31), (1.0, 1.0)), (2, (1300, 0, 97, 500), (0.5, 2.0)))]
    cos, sin = (torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(TDT[dtype]).to(dev)
                for x in ref.rotary_tables(dtype, probs[0].rot))
    p0 = probs[0]
    dt = TDT[dtype]
    t16 = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dt)
    qkv = torch.zeros(p0.B, n, p0.H + 2 * HKV, D, dtype=dt, device=dev)
    kd = torch.zeros(p0.B, L, M, HKV, D, dtype=torch.uint8, device=dev)
    vd = torch.zeros_like(kd)
    o = torch.zeros(p0.B, n, p0.H, D, dtype=dt, device=dev)
    sl = torch.zeros(p0.B, dtype=torch.int32, device=dev)
    qb, kb, vb = (torch.zeros(x.shape, dtype=dt, device=dev) for x in p0.biases)
    ks, vs = torch.ones(HKV, device=dev), torch.ones(HKV, device=dev)
    call = lambda: sfa.flash_decode_chunk_kv8_window(qkv, qb, kb, vb, kd, vd, sl, o, p0.B, M, p0.H, D, p0.rot, M, L, LAYER,
                                                     window, num_splits=2, num_heads_kv=HKV, k_scale=ks, v_scale=vs,
                                                     rotary_cos_table=cos, rotary_sin_table=sin)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        call()                                              # warm-up: the stream's workspace exists before the capture
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            call()
        for p in probs:
            for dst, src in ((qkv, t16(np.stack(p.tok))), (kd, torch.from_numpy(p.k8)), (vd, torch.from_numpy(p.v8)),
                             (qb, t16(p.biases[0])), (kb, t16(p.biases[1])), (vb, t16(p.biases[2])),
                             (ks, torch.from_numpy(p.ks)), (vs, torch.from_numpy(p.vs))):
                dst.copy_(src.to(dev))
            o.fill_(7.0)
            sl.copy_(torch.tensor(list(p.lens), dtype=torch.int32))
            graph.replay()
            side.synchronize()
            sfa.check_decode_status(dev)
            ob = bits(o.cpu())
            o_list = [ob[b] for b in range(p.B)]
            r = SimpleNamespace(o=o_list, of=[ref.cw.as_float(x, dtype) for x in o_list], k8=kd.cpu().numpy(),
                                v8=vd.cpu().numpy())
            check(r, p, window, ref.reference(p, window))
