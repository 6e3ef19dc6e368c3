"""Reference of sfa_decode_kv8_window (sliding-window decode over an fp8 e4m3 KV cache) and the problems of
tests/test_decode_kv8_window_{cpu,gpu}.py.

The reference is kv8_ref.decode_kv8_ref with a lower bound, through the same adapter over tests/serving_model.py: the
prologue, the quantisation of the new token into the caches, then the fp64 softmax over the rows [lo, pos] of the
DEQUANTISED cache, lo = max(0, pos + 1 - window).  Rows below lo are never looked at, so they may hold the NaN byte 0x7F.
window = None, or any window > pos, gives kv8_ref.decode_kv8_ref's bits.

Because the reference sees the dequantised bytes the device sees, the quantisation error is on both sides and the
project's decode tolerances (window_ref.TOL) apply unchanged.
"""
import functools
from types import SimpleNamespace

import numpy as np

import decode_cases as dc
import kv8_ref
from oracle import rotary_table_ref, round_to
from window_ref import TOL, window_lo  # noqa: F401  (TOL: re-exported for the two test files)


def decode_kv8_window_ref(qkv, k8, v8, seq_len, idx_layer, rot_dim, dtype, window, k_scale=None, v_scale=None,
                          q_bias=None, k_bias=None, v_bias=None, cos_table=None, sin_table=None, scale=None):
    """One sfa_decode_kv8_window step for the whole batch; the arguments and the result of kv8_ref.decode_kv8_ref, plus
    `window` (None = no window).  k8 / v8 [B, L, M, Hkv, D] uint8 are MUTATED at [b, idx_layer, seq_len[b]]."""
    ref = kv8_ref.decode_kv8_model(qkv, k8, v8, seq_len, idx_layer, rot_dim, dtype, window, None, k_scale, v_scale, q_bias, k_bias,
                                   v_bias, cos_table, sin_table, scale)
    return {key: ref[key] for key in ("o", "k_row", "v_row")}


# The parity sweep of tests/test_decode_kv8_window_gpu.py: (dtype, head_dim, layout, group, num_splits, window), a
# pairwise-covering subset of the product of FACTORS (tests/test_decode_kv8_window_cpu.py checks that).  "paged16" /
# "paged64" = a paged cache of that page size.
FACTORS = (("fp16", "bf16"), (64, 128), ("blmhd", "blhmd", "paged16", "paged64"), (1, 2, 4, 8, 16), (0, 1, 3),
           (1, 2, 17, 33, 64, 100, 129, 1000, 5000))
SWEEP = [
    ('bf16', 64, 'paged64', 1, 0, 5000),
    ('fp16', 64, 'paged16', 4, 3, 33),
    ('bf16', 128, 'paged16', 8, 1, 17),
    ('fp16', 128, 'blhmd', 16, 0, 100),
    ('bf16', 128, 'blmhd', 2, 3, 129),
    ('fp16', 64, 'blmhd', 1, 1, 1000),
    ('fp16', 128, 'paged64', 8, 3, 1),
    ('bf16', 128, 'blhmd', 4, 1, 64),
    ('fp16', 64, 'blhmd', 2, 3, 17),
    ('bf16', 64, 'blmhd', 16, 1, 2),
    ('fp16', 64, 'paged16', 8, 0, 64),
    ('bf16', 64, 'paged64', 2, 1, 100),
    ('fp16', 128, 'blhmd', 1, 3, 2),
    ('fp16', 64, 'blmhd', 4, 0, 129),
    ('fp16', 128, 'paged16', 16, 3, 5000),
    ('bf16', 64, 'paged16', 1, 0, 1),
    ('bf16', 128, 'paged16', 2, 0, 1000),
    ('bf16', 128, 'blhmd', 8, 0, 33),
    ('bf16', 64, 'blmhd', 8, 1, 5000),
    ('fp16', 128, 'paged64', 16, 0, 17),
    ('fp16', 128, 'paged64', 4, 3, 1000),
    ('fp16', 64, 'blmhd', 4, 3, 100),
    ('fp16', 128, 'blmhd', 2, 1, 1),
    ('bf16', 64, 'paged16', 4, 0, 2),
    ('bf16', 64, 'blmhd', 1, 1, 33),
    ('bf16', 64, 'blhmd', 16, 1, 129),
    ('fp16', 64, 'paged64', 1, 3, 64),
    ('fp16', 64, 'blmhd', 1, 0, 17),
    ('fp16', 128, 'paged64', 2, 0, 33),
    ('bf16', 64, 'blhmd', 8, 3, 1000),
    ('bf16', 64, 'blhmd', 2, 0, 5000),
    ('bf16', 64, 'blhmd', 4, 1, 1),
    ('fp16', 128, 'paged64', 8, 1, 129),
    ('fp16', 64, 'paged16', 1, 0, 129),
    ('fp16', 128, 'blmhd', 2, 0, 64),
    ('bf16', 128, 'paged64', 2, 0, 2),
    ('bf16', 128, 'paged16', 8, 0, 100),
    ('bf16', 64, 'paged64', 8, 3, 2),
    ('fp16', 128, 'blmhd', 4, 3, 5000),
    ('fp16', 64, 'paged16', 16, 3, 64),
    ('fp16', 64, 'blmhd', 16, 3, 1000),
    ('fp16', 128, 'blhmd', 16, 1, 33),
    ('fp16', 128, 'blmhd', 1, 1, 100),
    ('bf16', 64, 'paged64', 4, 3, 17),
    ('bf16', 128, 'paged16', 16, 3, 1),
]


# ---------------------------------------------------------------------------------------------------------------------
# the problem of the window suite (tests/test_decode_window_gpu.py) over an fp8 cache: B = 4 sequences at seq_len =
# [0, 5, 130, 1000], 2 kv heads, 2 layers, memory_max_len 1408, q / k / v bias, a partial rotary embedding
# (head_dim / 2), N(0,1) caches quantised with amax / 448 per kv head.  Canonical layout [B, L, M, Hkv, D]; made once,
# never modified.
# ---------------------------------------------------------------------------------------------------------------------

B, HKV, L, M, LAYER, SPARE = 4, 2, 2, 1408, 1, 3
LENS = (0, 5, 130, 1000)


def amax_scale(x):
    """amax / 448 per kv head of x [B, L, M, Hkv, D]"""
    return (np.abs(x).max(axis=(0, 1, 2, 4)) / 448.0).astype(np.float32)


@functools.lru_cache(maxsize=None)
def caches(D, k_factors=(1.0, 1.0)):
    """k8 / v8 uint8 [B, L, M, Hkv, D] and their scales; k_factors multiply k_scale per head (v_scale: reversed)"""
    rng = np.random.default_rng([1, D])
    kc = rng.standard_normal((B, L, M, HKV, D)).astype(np.float32)
    vc = rng.standard_normal((B, L, M, HKV, D)).astype(np.float32)
    f = np.asarray(k_factors, np.float32)
    ks, vs = amax_scale(kc) * f, amax_scale(vc) * f[::-1]
    return SimpleNamespace(k8=kv8_ref.quantize(kc, ks), v8=kv8_ref.quantize(vc, vs), ks=ks, vs=vs)


@functools.lru_cache(maxsize=None)
def tokens(dtype, D, G):
    """the new tokens [B, H + 2 Hkv, D] and the biases, representable in dtype (float32)"""
    rng = np.random.default_rng([2, D, G, dtype == "bf16"])
    H = HKV * G
    r = lambda *shape: round_to(rng.standard_normal(shape), dtype).astype(np.float32)
    return SimpleNamespace(H=H, rot=D // 2, qkv=r(B, H + 2 * HKV, D), qb=r(H, D), kb=r(HKV, D), vb=r(HKV, D))


@functools.lru_cache(maxsize=None)
def rotary_tables(dtype, rot):
    return rotary_table_ref(M, rot, dtype)


@functools.lru_cache(maxsize=None)
def reference(dtype, D, G, window, tables=False, lens=LENS, scale=None, k_factors=(1.0, 1.0)):
    """decode_kv8_window_ref on the inputs the device gets; window None = sfa_decode_kv8.  Adds k8 / v8 = the caches
    after the step."""
    t, c = tokens(dtype, D, G), caches(D, k_factors)
    cos, sin = rotary_tables(dtype, t.rot) if tables else (None, None)
    k8, v8 = c.k8.copy(), c.v8.copy()
    ref = decode_kv8_window_ref(t.qkv, k8, v8, lens, LAYER, t.rot, dtype, window, c.ks, c.vs, q_bias=t.qb, k_bias=t.kb,
                                v_bias=t.vb, cos_table=cos, sin_table=sin, scale=scale)
    return dict(ref, k8=k8, v8=v8)


# ---------------------------------------------------------------------------------------------------------------------
# the structured problems: decode_cases.Problem with entry "kv8" (e4m3 caches as bytes, one power-of-two scale per kv head,
# no RoPE, no bias, M = 256) and the window of entry "window" on top of it
# ---------------------------------------------------------------------------------------------------------------------

def with_window(p, window):
    """the kv8 problem p seen through `window`: .window and .lo as entry "window" has them (unread_mask, poisoned,
    call_table, weights and scores_log2 of decode_cases follow .lo)"""
    assert p.entry == "kv8" and window >= 1
    p.window = int(window)
    p.lo = [window_lo(pos, window) for pos in p.lens]
    return p


EDGE_KINDS = ["edge_in", "edge_last", "edge_out", "ramp_through", "ramp", "equal"]


def window_edges(dtype, G, D, kind, window):
    """decode_cases.window_edges over an fp8 cache: one batch per (kind, window), a sequence per lo of decode_cases.
    WINDOW_LOS with pos = lo + window - 1.  The kinds are decode_cases' with its two ramps apart: "ramp_through" = the
    ramp that peaks at lo and goes on rising below it, "ramp" = the one that rises in every tile of the window."""
    kw = dict(G=G, D=D, window=window)
    los = dc.window_los(window, kind)
    if kind in ("edge_in", "edge_last", "edge_out"):
        seqs = [dc.seq_window_edge(500 + i, lo=lo, where=kind[5:], **kw) for i, lo in enumerate(los)]
    elif kind in ("ramp_through", "ramp"):
        seqs = [dc.seq_window_ramp(600 + i, lo=lo, through=kind == "ramp_through", **kw) for i, lo in enumerate(los)]
    elif kind == "equal":
        seqs = [dc.seq_window_equal(700 + i, lo=lo, **kw) for i, lo in enumerate(los)]
    else:
        raise ValueError(kind)
    return with_window(dc.Problem("kv8", dtype, G, D, seqs), window)


def normal_problem(dtype, G, D, window, amax_scales=False):
    """N(0,1) data at the positions of decode_cases.UNREAD_POS (sections B and C of the numerics suite) through `window`"""
    return with_window(dc.normal_problem("kv8", dtype, G, D, amax_scales=amax_scales), window)


def oracle(p, scale=None, window="own"):
    """fp64 reference of the whole call on a structured problem: dict(o [B, H, D] float32 unrounded, kc, vc = the caches
    afterwards, as bytes).  window=: another window than the problem's (None: none)."""
    kc, vc = p.kc.copy(), p.vc.copy()
    qkv = np.concatenate([p.q, p.k_new, p.v_new], axis=1)
    with np.errstate(invalid="ignore"):
        ref = decode_kv8_window_ref(qkv, kc, vc, p.lens, dc.LAYER, p.rot, p.dtype, p.window if window == "own" else window,
                                    p.ks, p.vs, scale=scale)
    return dict(o=ref["o"], kc=kc, vc=vc)


def elementwise_tol(p, want):
    """what the GPU file allows per element: atol = rtol"""
    return TOL[p.dtype] * (1.0 + np.abs(want))


# ---------------------------------------------------------------------------------------------------------------------
# a model of the kernel's addressing (decode_kv8_body.h with WINDOW), and what one-line slips of it do
# ---------------------------------------------------------------------------------------------------------------------

def addressing_model(p, ref, slip=None, paged=False):
    """fp64 attention over the key slots as the windowed kernel addresses them at num_splits = 1: tiles of 32 keys from
    lo & ~31 up to pos, a slot is real if key < pos - t and key >= lo - t, its row is min(max(row, lo), pos - 1), and
    (paged, page size 16) its page index min(max(index of the tile's 16-row half, lo's page), the last page); then the
    quantised new token (ref = oracle(p): the caches after the step).  The bytes are dequantised with the problem's
    scales.  slip: "narrow" / "wide" = the lower mask key > nlo / key >= nlo - 1, "long" = lo one row lower, "page" = the
    first page one too high where lo is not page-aligned."""
    o = np.zeros((p.B, p.H, p.D))
    for b in range(p.B):
        pos = p.lens[b]
        lo = max(0, pos - p.window) if slip == "long" else p.lo[b]
        rows = []
        for t in range(lo & ~31, pos, 32):
            nlo = lo - t
            for key in range(min(32, pos - t)):
                if not {"narrow": key > nlo, "wide": key >= nlo - 1}.get(slip, key >= nlo):
                    continue
                row = min(max(t + key, lo), pos - 1)
                if paged:
                    first = (lo >> 4) + (1 if slip == "page" and lo & 15 else 0)
                    row = 16 * min(max((t + 16 * (key >> 4)) >> 4, first), (pos - 1) >> 4) + (row & 15)
                rows.append(row)
        rows.append(pos)                                                    # the new token, as stored
        K = p.values(ref["kc"][b, dc.LAYER, rows], p.ks)
        V = p.values(ref["vc"][b, dc.LAYER, rows], p.vs)
        sc = np.einsum("kgd,tkd->kgt", p.q[b].astype(np.float64).reshape(p.Hkv, p.G, p.D), K) * p.D ** -0.5
        w = np.exp(sc - sc.max(axis=2, keepdims=True))
        o[b] = np.einsum("kgt,tkd->kgd", w / w.sum(axis=2, keepdims=True), V).reshape(p.H, p.D)
    return o
