"""Reference, problems and device harness of sfa_decode_chunk_kv8_window / sfa_decode_varlen_kv8_window (the sliding
window in the multi-token decode calls over an fp8 e4m3 KV cache) for tests/test_decode_chunk_kv8_window_{cpu,gpu}.py and
tests/test_decode_varlen_kv8_window_gpu.py.

The reference is chunk_kv8_ref.chunk_kv8_ref -- the prologue of every token and the append of its quantised rows -- with a
lower bound, through the same adapter over tests/serving_model.py: token t attends to the rows [lo_t, pos + t] of the
cache AFTER the append, lo_t = max(0, pos + t + 1 - window).  Rows below lo_0 never enter a windowed result, so they may
hold the NaN byte 0x7F.  With window None, or any window >= pos + n, the bits are chunk_kv8_ref's.

How the device is checked is how tests/test_decode_chunk_kv8_gpu.py checks it: (a) the appended bytes against the
reference quantiser (chunk_kv8_ref.check_bytes: V exact, K within one e4m3 step and > 98 % identical per call, every
other byte of both caches unchanged), (b) o against attend() over the bytes the device stored, at the project's decode
tolerances (fp16 2e-3, bf16 1.6e-2, atol = rtol, elementwise, nothing exempt).

The frame is that of tests/chunk_window_ref.py: B = 4 sequences at seq_len = [0, 5, 130, 1000], 2 kv heads, 2 layers,
idx_layer 1, memory_max_len 1408, q / k / v bias and a partial rotary embedding (head_dim / 2); the caches are those of
tests/kv8_window_ref.py (N(0,1) values, scale = factor * amax / 448 per kv head).
"""
import functools
from types import SimpleNamespace

import numpy as np

import chunk_kv8_ref as ckr
import chunk_window_ref as cw
import kv8_ref
import kv8_window_ref as kwr
from oracle import rotary_table_ref, round_to
from window_ref import TOL, window_lo  # noqa: F401

B, HKV, L, M, LAYER, SPARE = 4, 2, 2, 1408, 1, 3
LENS = (0, 5, 130, 1000)
QTILE, KTILE = 256, 64
assert (HKV, L, M, SPARE) == (cw.HKV, cw.L, cw.M, cw.SPARE)     # to_layout / from_layout below are chunk_window_ref's
FILL = 0x33                                     # what the pages no sequence owns hold


# ---- the reference -----------------------------------------------------------------------------------------------------

def attend(q16, k8, v8, pos, window, k_scale=None, v_scale=None, scale=None):
    """chunk_kv8_ref.attend with the window's lower bound: q16 [n, H, D] float64 rotated, rounded queries of the tokens at
    pos .. pos + n - 1 of one sequence; k8 / v8 [M, Hkv, D] uint8, one (sequence, layer) of the cache after the append.
    Token t attends to the rows [max(0, pos + t + 1 - window), pos + t] (window None: from row 0).  Returns o [n, H, D]
    float64."""
    return ckr.attend_bytes(q16, k8, v8, pos, window, None, k_scale, v_scale, scale)[0]


def chunk_kv8_window_ref(tokens, k8, v8, seq_len, idx_layer, rot_dim, dtype, window, k_scale=None, v_scale=None,
                         scale=None, **kw):
    """chunk_kv8_ref.chunk_kv8_ref's arguments and result, plus `window` (None = no window).  k8 / v8 are MUTATED at the
    appended rows."""
    bias_and_tables = [kw.pop(name, None) for name in ("q_bias", "k_bias", "v_bias", "cos_table", "sin_table")]
    assert not kw, sorted(kw)
    ref = ckr.chunk_kv8_model(tokens, k8, v8, seq_len, idx_layer, rot_dim, dtype, window, None, k_scale, v_scale, *bias_and_tables,
                              scale)
    return dict(o=ref["o"], q16=ref["q16"])


# ---- problems (canonical cache layout [B, L, M, Hkv, D], uint8): made once, never modified -------------------------------

@functools.lru_cache(maxsize=None)
def rotary_tables(dtype, rot):
    return rotary_table_ref(M, rot, dtype)


def make_problem(dtype, D, G, lens, ns, seed=0, k_factors=(1.0, 1.0), bias=True, rot=None, tables=False, scale=None,
                 with_scales=True):
    """len(lens) sequences at seq_len = lens with ns new N(0,1) tokens each, rounded to dtype; q / k / v bias and a partial
    rotary embedding (head_dim / 2) unless told otherwise.  Four sequences get the caches of kv8_window_ref (k_factors
    multiply k_scale per head, reversed v_scale: four distinct scales), another count caches of its own made the same way."""
    nb, H = len(lens), G * HKV
    rng = np.random.default_rng([21, D, G, dtype == "bf16", nb, max(ns), seed])
    if nb == kwr.B and with_scales:
        c = kwr.caches(D, tuple(k_factors))
        k8, v8, ks, vs = c.k8, c.v8, c.ks, c.vs
    else:
        crng = np.random.default_rng([22, D, nb])
        kc = crng.standard_normal((nb, L, M, HKV, D)).astype(np.float32)
        vc = crng.standard_normal((nb, L, M, HKV, D)).astype(np.float32)
        ks = vs = None
        if with_scales:
            f = np.asarray(k_factors, np.float32)
            ks, vs = kwr.amax_scale(kc) * f, kwr.amax_scale(vc) * f[::-1]
        k8, v8 = kv8_ref.quantize(kc, ks), kv8_ref.quantize(vc, vs)
    r = lambda *shape: round_to(rng.standard_normal(shape), dtype).astype(np.float32)
    tok = [r(n, H + 2 * HKV, D) for n in ns]
    p = SimpleNamespace(dtype=dtype, D=D, G=G, H=H, B=nb, lens=tuple(lens), ns=tuple(ns), tok=tok, k8=k8, v8=v8, ks=ks,
                        vs=vs, rot=D // 2 if rot is None else rot, tables=tables, biases=None, scale=scale)
    if bias:
        p.biases = (r(H, D), r(HKV, D), r(HKV, D))
    return p


@functools.lru_cache(maxsize=None)
def problem(dtype, D, G, n, tables=False):
    """the common frame: B = 4 at seq_len = LENS, n new tokens each"""
    return make_problem(dtype, D, G, LENS, (n,) * len(LENS), tables=tables)


def reference(p, window, lens=None):
    """chunk_kv8_window_ref on copies of the problem's caches: (ref, k8 after, v8 after)"""
    k_ref, v_ref = p.k8.copy(), p.v8.copy()
    kw = {}
    if p.biases is not None:
        kw = dict(q_bias=p.biases[0], k_bias=p.biases[1], v_bias=p.biases[2])
    if p.tables and p.rot > 0:
        cos, sin = rotary_tables(p.dtype, p.rot)
        kw.update(cos_table=cos, sin_table=sin)
    ref = chunk_kv8_window_ref(p.tok, k_ref, v_ref, p.lens if lens is None else lens, LAYER, p.rot, p.dtype, window, p.ks,
                               p.vs, scale=p.scale, **kw)
    return ref, k_ref, v_ref


@functools.lru_cache(maxsize=None)
def frame_reference(dtype, D, G, n, window, tables=False):
    return reference(problem(dtype, D, G, n, tables), window)


# The parity sweep: (dtype, head_dim, layout, group, num_splits, window, tokens per sequence), a pairwise-covering subset
# of the product of FACTORS = kv8_window_ref.FACTORS and a token count (tests/test_decode_chunk_kv8_window_cpu.py checks
# that).  "paged16" / "paged64" = a paged cache of that page size.  G * n > 256 (two q-tiles) in the first two and others.
FACTORS = kwr.FACTORS + ((1, 5, 45, 70),)
SWEEP = [
    ('bf16', 128, 'paged16', 8, 3, 100, 45),
    ('fp16', 64, 'blhmd', 16, 1, 33, 70),
    ('fp16', 128, 'blmhd', 4, 0, 1, 5),
    ('bf16', 64, 'paged64', 2, 0, 129, 1),
    ('bf16', 64, 'blmhd', 1, 1, 2, 45),
    ('fp16', 128, 'blhmd', 1, 3, 1000, 1),
    ('bf16', 128, 'paged64', 4, 1, 17, 70),
    ('fp16', 64, 'paged16', 8, 1, 5000, 5),
    ('bf16', 128, 'paged64', 16, 3, 64, 5),
    ('fp16', 64, 'blhmd', 2, 0, 17, 45),
    ('bf16', 128, 'blmhd', 2, 3, 5000, 70),
    ('fp16', 64, 'paged16', 1, 0, 64, 70),
    ('fp16', 64, 'paged16', 4, 3, 2, 1),
    ('bf16', 64, 'blhmd', 8, 1, 1, 1),
    ('fp16', 64, 'blmhd', 16, 0, 100, 1),
    ('bf16', 64, 'paged64', 8, 0, 1000, 70),
    ('fp16', 128, 'paged64', 16, 1, 129, 45),
    ('bf16', 128, 'paged16', 2, 0, 33, 5),
    ('bf16', 128, 'blhmd', 8, 0, 2, 5),
    ('fp16', 128, 'blhmd', 4, 1, 64, 45),
    ('fp16', 64, 'paged64', 1, 1, 100, 5),
    ('bf16', 64, 'blmhd', 8, 3, 129, 70),
    ('fp16', 128, 'paged16', 2, 1, 1000, 5),
    ('bf16', 64, 'paged16', 16, 3, 1, 45),
    ('bf16', 128, 'blhmd', 16, 0, 5000, 45),
    ('fp16', 64, 'paged64', 8, 3, 33, 45),
    ('bf16', 128, 'paged16', 8, 3, 17, 5),
    ('fp16', 128, 'blmhd', 8, 3, 64, 1),
    ('bf16', 128, 'blmhd', 16, 0, 17, 1),
    ('fp16', 64, 'blhmd', 4, 3, 129, 5),
    ('fp16', 64, 'paged64', 1, 0, 1, 70),
    ('fp16', 64, 'blmhd', 4, 1, 33, 1),
    ('bf16', 128, 'blmhd', 16, 1, 1000, 45),
    ('fp16', 128, 'paged64', 1, 1, 5000, 1),
    ('fp16', 128, 'blhmd', 4, 1, 100, 70),
    ('fp16', 128, 'paged64', 2, 3, 2, 70),
    ('fp16', 128, 'paged16', 1, 1, 129, 70),
    ('fp16', 64, 'blmhd', 1, 0, 33, 45),
    ('bf16', 128, 'blhmd', 16, 3, 2, 70),
    ('bf16', 64, 'paged16', 4, 3, 5000, 1),
    ('bf16', 128, 'blhmd', 2, 1, 64, 70),
    ('fp16', 64, 'paged16', 4, 1, 1000, 45),
    ('bf16', 128, 'blhmd', 1, 3, 17, 45),
    ('fp16', 128, 'blhmd', 2, 1, 1, 5),
    ('bf16', 128, 'paged64', 2, 1, 100, 5),
]


# ---- the window-edge problems ---------------------------------------------------------------------------------------------
# Those of chunk_window_ref.edge_problem (G = 1, 300 tokens, rotary_embedding_dim = 0, no bias, one sequence per lo_0 of
# EDGE_LO0) over an fp8 cache with the power-of-two scales EDGE_SCALES.  Every value / scale is an e4m3 number, so the
# bytes hold the 16-bit problem's values exactly and the device quantises the new rows without rounding: the spike at j*
# (64), the marks of the V rows (16 + 2 * (j % 7), alternating sign), zero.  The ramp's score (M - j) % 128 needs seven
# bits, e4m3 has four: it is split over two components, 16 * (s // 16) and s % 16, both read with q = 8.

EDGE_LO0, EDGE_WINDOWS, EDGE_N, spike_rows, edge_lens = cw.EDGE_LO0, cw.EDGE_WINDOWS, cw.EDGE_N, cw.spike_rows, cw.edge_lens
EDGE_SCALES = np.array([0.5, 2.0], np.float32)


@functools.lru_cache(maxsize=None)
def _edge_core(window, kind, D):
    """the bytes and the tokens of an edge problem: the same for both dtypes (every value is exact in fp16 and in bf16)"""
    p16 = cw.edge_problem("bf16", window, kind, D)
    H = HKV
    kf, vf = p16.kf.copy(), p16.vf.copy()
    tok = p16.qkv.float().numpy().copy()                        # [B, EDGE_N, H + 2 Hkv, D]
    if kind == "ramp":
        for x in (kf, tok[:, :, H:H + HKV]):
            s = x[..., 0].copy()
            x[..., 0], x[..., 1] = 16.0 * np.floor(s / 16.0), s % 16.0
        tok[:, :, :H, 1] = 8.0
    k8, v8 = kv8_ref.quantize(kf, EDGE_SCALES), kv8_ref.quantize(vf, EDGE_SCALES)
    assert np.array_equal(kv8_ref.dequantize(k8, EDGE_SCALES), kf) and np.array_equal(kv8_ref.dequantize(v8, EDGE_SCALES), vf)
    for part in (tok[:, :, H:H + HKV], tok[:, :, H + HKV:]):    # the new rows quantise without rounding
        assert np.array_equal(kv8_ref.dequantize(kv8_ref.quantize(part, EDGE_SCALES), EDGE_SCALES), part)
    assert np.array_equal(round_to(tok, "fp16"), tok) and np.array_equal(round_to(tok, "bf16"), tok)
    return p16.lens, p16.ns, list(tok), k8, v8


@functools.lru_cache(maxsize=None)
def edge_problem(dtype, window, kind, D=64):
    lens, ns, tok, k8, v8 = _edge_core(window, kind, D)
    return SimpleNamespace(dtype=dtype, D=D, G=1, H=HKV, B=len(lens), lens=lens, ns=ns, tok=tok, k8=k8, v8=v8,
                           ks=EDGE_SCALES, vs=EDGE_SCALES, rot=0, tables=False, biases=None, scale=None)


def attend_dense(q16, k8, v8, pos, window, k_scale=None, v_scale=None, scale=None):
    """attend() as one masked fp64 softmax over the rows [lo_0, pos + n) instead of a slice per token: the same sums in
    another order (tests/test_decode_chunk_kv8_window_cpu.py holds the two together), many times faster for the 14 x 300
    tokens of an edge problem"""
    n, H, D = q16.shape
    Hkv = k8.shape[1]
    if scale is None:
        scale = 1.0 / np.sqrt(float(D))
    lo0 = window_lo(pos, window)
    K, V = kv8_ref.dequantize(k8[lo0:pos + n], k_scale), kv8_ref.dequantize(v8[lo0:pos + n], v_scale)     # [rows, Hkv, D]
    j, t = lo0 + np.arange(K.shape[0]), np.arange(n)
    lo_t = np.array([window_lo(pos + int(x), window) for x in t])
    vis = (j[None, :] >= lo_t[:, None]) & (j[None, :] <= pos + t[:, None])                                # [n, rows]
    sc = np.einsum("tkgd,rkd->tkgr", q16.reshape(n, Hkv, H // Hkv, D), K) * scale
    sc = np.where(vis[:, None, None, :], sc, -np.inf)
    sc -= sc.max(axis=3, keepdims=True)
    p = np.exp(sc)
    p /= p.sum(axis=3, keepdims=True)
    return np.einsum("tkgr,rkd->tkgd", p, V).reshape(n, H, D)


@functools.lru_cache(maxsize=None)
def edge_reference(window, kind):
    """reference() of an edge problem, of either dtype (the values are exact in both), without its per-token loops: with
    no rotation and no bias q16 is the token's q and the appended bytes are the quantised k / v of the token (exactly);
    attend_dense does the rest.  (ref, k8 after, v8 after)"""
    p = edge_problem("bf16", window, kind)
    assert p.rot == 0 and p.biases is None
    k_ref, v_ref = p.k8.copy(), p.v8.copy()
    o, q = [], []
    for b, (pos, n) in enumerate(zip(p.lens, p.ns)):
        k_ref[b, LAYER, pos:pos + n] = kv8_ref.quantize(p.tok[b][:, p.H:p.H + HKV], p.ks)
        v_ref[b, LAYER, pos:pos + n] = kv8_ref.quantize(p.tok[b][:, p.H + HKV:], p.vs)
        q.append(p.tok[b][:, :p.H].astype(np.float64))
        o.append(attend_dense(q[b], k_ref[b, LAYER], v_ref[b, LAYER], pos, window, p.ks, p.vs))
    return dict(o=o, q16=q), k_ref, v_ref


# ---- layouts -----------------------------------------------------------------------------------------------------------

page_size, page_table = cw.page_size, cw.page_table


def to_layout(c, layout, fill=FILL):
    """canonical uint8 numpy [B, L, M, Hkv, D] -> the (CPU) torch tensor of `layout`; the spare pages hold `fill`"""
    import torch
    return cw.to_layout(torch.from_numpy(np.ascontiguousarray(c)), layout, fill)


def from_layout(t, layout, nb):
    """(canonical uint8 numpy [B, L, M, Hkv, D], the spare pages as a tensor or None)"""
    canon, spare = cw.from_layout(t, layout, nb)
    return canon.numpy(), spare


# ---- the device ----------------------------------------------------------------------------------------------------------

def run(sfa, p, layout, window, num_splits=0, varlen=False, k8=None, v8=None, table=None, fill=FILL, lens=None, cu=None,
        null_scales=False, as_fp8=False):
    """One call on fresh device copies: flash_decode_chunk_kv8_window (varlen: flash_decode_varlen_kv8_window, the tokens
    packed), or the call without a window for window None.  k8 / v8: canonical caches instead of the problem's own; table:
    the block_table the call gets instead of the one the pools are laid out by; lens: another seq_len; cu: the cu_tokens
    the packed call gets instead of the true ones (o is cut by the true ones); null_scales: no scale tensors.  Returns o (a
    list per sequence of [n_b, H, D] bits), of (the same as float32 numpy), k8, v8 (canonical numpy) and the spare pages."""
    import torch
    dev = torch.device("cuda:0")
    nb, H, D = p.B, p.H, p.D
    dt = cw.TDT[p.dtype]
    t16 = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dt).to(dev)
    kd = to_layout(p.k8 if k8 is None else k8, layout, fill).to(dev)
    vd = to_layout(p.v8 if v8 is None else v8, layout, fill).to(dev)
    if as_fp8:
        kd, vd = kd.view(torch.float8_e4m3fn), vd.view(torch.float8_e4m3fn)
    sl = torch.tensor(list(p.lens if lens is None else lens), dtype=torch.int32, device=dev)
    ps = page_size(layout)
    kw = dict(num_splits=num_splits, kv_layout="paged" if ps else layout, num_heads_kv=HKV, softmax_scale=p.scale)
    if ps:
        kw["block_table"] = torch.from_numpy(page_table(ps, nb)[0] if table is None else table).to(dev)
    if p.tables and p.rot > 0:
        cos, sin = rotary_tables(p.dtype, p.rot)
        kw.update(rotary_cos_table=t16(cos), rotary_sin_table=t16(sin))
    if p.ks is not None and not null_scales:
        kw.update(k_scale=torch.from_numpy(np.asarray(p.ks, np.float32)).to(dev),
                  v_scale=torch.from_numpy(np.asarray(p.vs, np.float32)).to(dev))
    biases = (None, None, None) if p.biases is None else tuple(t16(x) for x in p.biases)
    heads = (3, H, D) if p.G == 1 else (H + 2 * HKV, D)         # the reference's shape when every query head has its own kv head
    true_cu = np.concatenate([[0], np.cumsum(p.ns)]).astype(np.int32)
    if varlen:
        T = max(int(true_cu[-1]), 1)
        qkv = np.zeros((T, H + 2 * HKV, D), np.float32)
        for b, n in enumerate(p.ns):
            qkv[true_cu[b]:true_cu[b + 1]] = p.tok[b][:n]
        o = torch.full((T, H, D), 7.0, dtype=dt, device=dev)
        cu_d = torch.from_numpy(true_cu if cu is None else np.asarray(cu, np.int32)).to(dev)
        args = (t16(qkv).view((T,) + heads), *biases, kd, vd, sl, o, cu_d, nb, M, H, D, p.rot, M, L, LAYER)
        ret = (sfa.flash_decode_varlen_kv8(*args, **kw) if window is None
               else sfa.flash_decode_varlen_kv8_window(*args, window, **kw))
    else:
        n = p.ns[0]
        assert all(x == n for x in p.ns)
        o = torch.full((nb, n, H, D), 7.0, dtype=dt, device=dev)
        args = (t16(np.stack([x[:n] for x in p.tok])).view((nb, n) + heads), *biases, kd, vd, sl, o, nb, M, H, D, p.rot, M,
                L, LAYER)
        ret = (sfa.flash_decode_chunk_kv8(*args, **kw) if window is None
               else sfa.flash_decode_chunk_kv8_window(*args, window, **kw))
    assert ret.data_ptr() == o.data_ptr()
    torch.cuda.synchronize()
    ob = cw.bits(o.cpu())
    o_list = [ob[true_cu[b]:true_cu[b + 1]] for b in range(nb)] if varlen else [ob[b] for b in range(nb)]
    k_out, spare_k = from_layout(kd, layout, nb)
    v_out, spare_v = from_layout(vd, layout, nb)
    return SimpleNamespace(o=o_list, of=[cw.as_float(x, p.dtype) for x in o_list], k8=k_out, v8=v_out, spare_k=spare_k,
                           spare_v=spare_v, rest=ob[true_cu[-1]:] if varlen else None)


def same_bits(r, other):
    """o and both caches of two runs, bit for bit"""
    import torch
    return (all(torch.equal(a, b) for a, b in zip(r.o, other.o)) and np.array_equal(r.k8, other.k8) and
            np.array_equal(r.v8, other.v8))


def check(r, p, window, ref3, k_before=None, v_before=None, lens=None, k_bytes=True):
    """(a) the appended bytes against the reference quantiser and every other byte against the bytes before; (b) o of every
    sequence against attend() over the bytes the device stored, with q16 from the reference, within the project's
    tolerance, elementwise, nothing exempt.  ref3 = reference(p, window).

    (a)'s cap on K -- within one e4m3 step -- is a condition on the inputs: it holds where the device and the reference
    rotate with the same cos / sin.  With the trigonometry computed in the kernel the angle pos * 10000^(-2j/rot) differs
    from numpy's in its last fp32 bit, 1e-4 rad at pos = 1000; an element of the rotated k that nearly cancels
    (x cos - y sin ~ 0) then moves by 1e-4 * |(x, y)|, several subnormal e4m3 steps (2^-9 * k_scale ~ 2e-5) although it is
    a fraction of a 16-bit ulp of its pair.  With 45 to 300 tokens around row 1000 that happens once in some calls (at one
    token per call, tests/test_decode_kv8_window_gpu.py, it does not).  So the problems of these files that reach long
    positions read the rotary tables, and (a) holds in them by construction; k_bytes=False is for the additional runs with
    in-kernel trigonometry at those positions, whose appended bytes are held, bit for bit, against the call without a
    window instead: V exact, every other byte unchanged, and (b)."""
    ref, k_ref, v_ref = ref3
    k_true = k_ref
    lens = p.lens if lens is None else lens
    if not k_bytes:                             # K: only where the reference's bytes are the device's own
        k_ref = k_ref.copy()
        k_ref[~append_mask(p, lens)] = r.k8[~append_mask(p, lens)]
    ckr.check_bytes(lens, p.ns, r.k8, r.v8, p.k8 if k_before is None else k_before, p.v8 if v_before is None else v_before,
                    k_ref, v_ref)
    tol = TOL[p.dtype]
    for b, n in enumerate(p.ns):
        if n == 0:
            assert r.of[b].shape[0] == 0
            continue
        if np.array_equal(r.k8[b, LAYER], k_true[b, LAYER]) and np.array_equal(r.v8[b, LAYER], v_ref[b, LAYER]):
            want = ref["o"][b]                  # the device stored the reference's bytes: attend() over them is ref's o
        else:
            want = attend(ref["q16"][b], r.k8[b, LAYER], r.v8[b, LAYER], lens[b], window, p.ks, p.vs, p.scale)
        assert np.isfinite(r.of[b]).all(), b
        print("sequence %d: max |o - ref| = %.3e (tol %.1e)" % (b, np.abs(r.of[b] - want).max(), tol))
        np.testing.assert_allclose(r.of[b], want, atol=tol, rtol=tol, err_msg=f"sequence {b}")


def append_mask(p, lens=None):
    """[B, L, M] True on every row a call must leave alone"""
    m = np.ones((p.B, L, M), dtype=bool)
    for b, (pos, n) in enumerate(zip(p.lens if lens is None else lens, p.ns)):
        if 0 <= pos and pos + n <= M:
            m[b, LAYER, pos:pos + n] = False
    return m


def poisoned(c, p, window):
    """a copy of the canonical cache c with 0x7F (an e4m3 NaN) in every byte the call must not read: the other layer, the
    rows below lo_0 and the rows at or beyond pos + n (every row of a sequence without tokens)"""
    q = c.copy()
    q[:, 1 - LAYER] = 0x7F
    for b, (pos, n) in enumerate(zip(p.lens, p.ns)):
        if n == 0:
            q[b, LAYER] = 0x7F
            continue
        q[b, LAYER, :window_lo(pos, window)] = 0x7F
        q[b, LAYER, pos + n:] = 0x7F
    return q


def poisoned_table(p, window, ps):
    """-1 in the block_table entries [0, lo_0 / page_size) and past the last page a sequence needs (all of them for a
    sequence without tokens)"""
    table = page_table(ps, p.B)[0].copy()
    for b, (pos, n) in enumerate(zip(p.lens, p.ns)):
        if n == 0:
            table[b] = -1
            continue
        table[b, :window_lo(pos, window) // ps] = -1
        table[b, (pos + n - 1) // ps + 1:] = -1
    return table
