"""Reference, problems and device harness of sfa_decode_chunk_window / sfa_decode_varlen_window for
tests/test_decode_chunk_window_{cpu,gpu}.py and tests/test_decode_varlen_window_gpu.py.

chunk_window_ref is an adapter over tests/serving_model.py, which holds the arithmetic: the prologue of all tokens, the
append, then token t over the rows [lo_t, pos + t] of the cache after it.  chunk_window_ref_literal states the contract the
other way -- window_ref.decode_window_ref applied token by token, with the appended rows fed forward -- and
tests/test_decode_chunk_window_cpu.py holds the two together.  Rows below lo_0 = max(0, pos + 1 - window) are never looked
at, so they may hold NaN.

Shapes follow the constants of the kernel: a q-tile is 256 query rows (row r = t * G + g), a wave 32 rows, a key tile 64
keys, a half-tile 32.
"""
import functools
from types import SimpleNamespace

import numpy as np
import torch

import serving_model as sm
from oracle import rotary_table_ref, round_to, to_bits16  # noqa: F401  (round_to: tests reach it through this module)
from window_ref import TOL, decode_window_ref, window_lo  # noqa: F401

QTILE, WAVE, KTILE, HALF = 256, 32, 64, 32
HKV, L, M, LAYER, SPARE = 2, 2, 1408, 1, 3
LENS = (0, 5, 130, 1000)
NAN16 = 0x7FFF                                  # NaN in fp16 and in bf16
INF16 = {"fp16": 0x7C00, "bf16": 0x7F80}
TDT = {"fp16": torch.float16, "bf16": torch.bfloat16}
ULP = {"fp16": 2.0 ** -10, "bf16": 2.0 ** -7}


# ---- the reference -----------------------------------------------------------------------------------------------------

def chunk_window_model(prob, window, sinks=None, scale=None):
    """A 16-bit problem (below) through the model, for chunk_window_ref and sinks_ref.chunk_sinks_ref: per sequence b
    (o [n_b, H, D] float32 unrounded, k_rows, v_rows [n_b, Hkv, D] float32, lse [n_b, H] float64 without the sink, o in
    float64).  LAYER alone of the float caches is turned into bits."""
    f = lambda x: None if x is None else x.float().numpy()
    cos, sin = rotary_tables(prob.dtype, prob.rot) if prob.tables and prob.rot > 0 else (None, None)
    H = prob.G * getattr(prob, "Hkv", HKV)      # (a problem built by hand may have another kv-head count)
    call = sm.make_call(prob.dtype, H, prob.lens, prob.ns, [f(prob.qkv[b][:n]) for b, n in enumerate(prob.ns)], 0, prob.rot,
                        q_bias=f(prob.qb), k_bias=f(prob.kb), v_bias=f(prob.vb), cos=cos, sin=sin, window=window, sinks=sinks,
                        softmax_scale=scale)
    cache = tuple(to_bits16(c[:, LAYER:LAYER + 1], prob.dtype) for c in (prob.kf, prob.vf))
    app, res = sm.run(cache, call)
    return [(o.astype(np.float32), k16, v16, lse, o) for (o, lse), k16, v16 in zip(res, app["k16"], app["v16"])]


def chunk_window_ref(prob, window):
    """prob: a problem (below).  Returns per sequence b (o [n_b, H, D] float32 unrounded, k_rows, v_rows [n_b, Hkv, D]
    float32 = what the call stores at the cache rows pos .. pos + n_b - 1).  window None: no window."""
    return [r[:3] for r in chunk_window_model(prob, window)]


def chunk_window_ref_literal(prob, window):
    """The definition: n successive decode_window_ref calls per sequence, each on the cache the one before left."""
    H = prob.G * HKV
    f = lambda x: None if x is None else x.float().numpy()
    cos, sin = rotary_tables(prob.dtype, prob.rot) if prob.tables and prob.rot > 0 else (None, None)
    kc, vc = prob.kf.copy(), prob.vf.copy()
    out = []
    for b, (pos, n) in enumerate(zip(prob.lens, prob.ns)):
        o = np.zeros((n, H, prob.D), np.float32)
        kr = np.zeros((n, HKV, prob.D), np.float32)
        vr = np.zeros_like(kr)
        for t in range(n):
            x = prob.qkv[b, t].float().numpy()[None]
            r = decode_window_ref(x[:, :H], x[:, H:H + HKV], x[:, H + HKV:], kc[b:b + 1], vc[b:b + 1], [pos + t], LAYER,
                                  prob.rot, window, prob.dtype, q_bias=f(prob.qb), k_bias=f(prob.kb), v_bias=f(prob.vb),
                                  cos_table=cos, sin_table=sin)
            o[t], kr[t], vr[t] = r["o"][0], r["k_row"][0], r["v_row"][0]
            kc[b, LAYER, pos + t], vc[b, LAYER, pos + t] = kr[t], vr[t]
        out.append((o, kr, vr))
    return out


# ---- problems (CPU, canonical cache layout [B, L, M, Hkv, D]): made once, never modified ------------------------------

def _randn(rng, dtype, *shape):
    return torch.from_numpy(rng.standard_normal(shape, dtype=np.float32)).to(TDT[dtype])


@functools.lru_cache(maxsize=None)
def rotary_tables(dtype, rot):
    return rotary_table_ref(M, rot, dtype)


@functools.lru_cache(maxsize=None)
def caches(dtype, D, B=4):
    rng = np.random.default_rng([11, D, dtype == "bf16", B])
    kc, vc = _randn(rng, dtype, B, L, M, HKV, D), _randn(rng, dtype, B, L, M, HKV, D)
    return kc, vc


def make_problem(dtype, D, G, lens, ns, qkv=None, kc=None, vc=None, bias=True, rot=None, tables=False, seed=0):
    """B = len(lens) sequences at seq_len = lens with ns new tokens each; qkv [B, max(ns), H + 2 Hkv, D] (the tokens past
    n_b are unused), q / k / v bias and a partial rotary embedding (head_dim / 2) unless told otherwise."""
    B, H, nmax = len(lens), G * HKV, max(max(ns), 1)
    rng = np.random.default_rng([12, D, G, dtype == "bf16", B, nmax, seed])
    if qkv is None:
        qkv = _randn(rng, dtype, B, nmax, H + 2 * HKV, D)
    if kc is None:
        kc, vc = caches(dtype, D, B)
    p = SimpleNamespace(dtype=dtype, D=D, G=G, H=H, B=B, lens=tuple(lens), ns=tuple(ns), qkv=qkv, kc=kc, vc=vc,
                        kf=kc.float().numpy(), vf=vc.float().numpy(), rot=D // 2 if rot is None else rot, tables=tables,
                        qb=None, kb=None, vb=None)
    if bias:
        p.qb, p.kb, p.vb = _randn(rng, dtype, H, D), _randn(rng, dtype, HKV, D), _randn(rng, dtype, HKV, D)
    return p


@functools.lru_cache(maxsize=None)
def problem(dtype, D, G, n, tables=False):
    """the common frame: B = 4 at seq_len = LENS, n new tokens each"""
    return make_problem(dtype, D, G, LENS, (n,) * len(LENS), tables=tables)


@functools.lru_cache(maxsize=None)
def reference(dtype, D, G, n, window, tables=False):
    return chunk_window_ref(problem(dtype, D, G, n, tables), window)


def sweep_tokens(G):
    """n of a parity case: 300 tokens at G = 1 and 40 at G = 8 are two q-tiles (the second one's own lower bound lies
    above lo_0); 40 tokens otherwise"""
    return 300 if G == 1 else 40


# The parity sweep: (dtype, head_dim, layout, group, num_splits, window), a pairwise-covering subset of the product of
# FACTORS (tests/test_decode_chunk_window_cpu.py checks that).  "paged16" / "paged64" = a paged cache of that page size.
FACTORS = (("fp16", "bf16"), (64, 128), ("blmhd", "blhmd", "paged16", "paged64"), (1, 2, 4, 8, 16), (0, 1, 3),
           (1, 2, 17, 33, 64, 100, 129, 1000, 5000))
SWEEP = [
    ('bf16', 64, 'blhmd', 2, 0, 2),
    ('fp16', 128, 'paged16', 1, 1, 2),
    ('bf16', 128, 'paged64', 16, 3, 129),
    ('fp16', 64, 'blmhd', 8, 3, 1000),
    ('bf16', 128, 'blmhd', 4, 1, 5000),
    ('fp16', 64, 'paged64', 4, 0, 1),
    ('bf16', 128, 'paged16', 8, 0, 33),
    ('fp16', 64, 'blhmd', 16, 1, 100),
    ('fp16', 64, 'paged16', 2, 3, 5000),
    ('bf16', 64, 'blmhd', 1, 0, 64),
    ('bf16', 128, 'paged64', 2, 1, 1000),
    ('bf16', 128, 'blhmd', 1, 3, 17),
    ('bf16', 128, 'paged16', 4, 3, 100),
    ('fp16', 64, 'blhmd', 8, 1, 129),
    ('fp16', 64, 'blmhd', 16, 0, 17),
    ('fp16', 128, 'paged64', 8, 1, 64),
    ('fp16', 64, 'blhmd', 4, 3, 33),
    ('bf16', 128, 'blmhd', 2, 1, 1),
    ('fp16', 64, 'paged64', 1, 1, 33),
    ('fp16', 64, 'paged16', 16, 3, 1),
    ('fp16', 64, 'blhmd', 1, 0, 5000),
    ('fp16', 128, 'blhmd', 2, 3, 64),
    ('fp16', 128, 'paged64', 16, 3, 2),
    ('bf16', 128, 'paged16', 2, 0, 129),
    ('fp16', 64, 'paged16', 1, 0, 1000),
    ('bf16', 64, 'paged64', 4, 1, 17),
    ('fp16', 128, 'blmhd', 1, 0, 100),
    ('bf16', 128, 'blmhd', 4, 0, 2),
    ('fp16', 128, 'paged16', 4, 1, 64),
    ('fp16', 64, 'blmhd', 16, 1, 33),
    ('fp16', 64, 'blmhd', 1, 0, 129),
    ('bf16', 128, 'paged64', 2, 1, 100),
    ('fp16', 128, 'paged16', 2, 1, 17),
    ('bf16', 128, 'blhmd', 16, 1, 1000),
    ('bf16', 64, 'paged64', 8, 0, 5000),
    ('bf16', 128, 'blhmd', 8, 3, 1),
    ('fp16', 64, 'blmhd', 4, 0, 129),
    ('bf16', 64, 'blhmd', 8, 0, 17),
    ('bf16', 128, 'paged64', 4, 3, 1000),
    ('bf16', 128, 'blhmd', 16, 0, 5000),
    ('bf16', 128, 'blmhd', 8, 3, 2),
    ('fp16', 64, 'blmhd', 2, 3, 33),
    ('bf16', 64, 'blhmd', 8, 1, 100),
    ('bf16', 64, 'paged16', 16, 0, 64),
    ('bf16', 64, 'paged16', 1, 0, 1),
]


# ---- the window-edge problems (rotary_embedding_dim = 0 and no bias: the device's q and k are the input bits) ----------

EDGE_LO0 = (0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129)
EDGE_WINDOWS = (17, 32, 40, 100)
EDGE_N = 300                                    # G = 1: two q-tiles, ten waves


def edge_lens(window):
    """one sequence per lo_0 of EDGE_LO0: pos = lo_0 + window - 1 (lo_0 = 0: a sequence shorter than the window)"""
    return tuple(lo0 + window - 1 if lo0 else window // 2 for lo0 in EDGE_LO0)


# (token, j* + 1) of the spike problems: the first token that must not see the spike at row j* is the first and the last
# row of a wave, the first row of the second q-tile, and a row whose lower bound falls on a 64-key and on a 32-key (not
# 64-key) boundary.  None: j* = token + 10.
SPIKES = ((32, None), (63, None), (256, None), (100, 128), (100, 96))


def spike_rows(window):
    """(seq_len, j*) per sequence of the spike problem: token tau has lo_tau = j* + 1 = pos + tau + 1 - window"""
    out = []
    for tau, lo in SPIKES:
        jstar = tau + 10 if lo is None else lo - 1
        out.append((jstar - tau + window, jstar))
    return out


@functools.lru_cache(maxsize=None)
def edge_problem(dtype, window, kind, D=64):
    """G = 1, n = EDGE_N.
    kind "spike": all keys zero but row j* of each sequence (spike_rows), whose score is 64: it carries all the weight of
          every token that sees it;
    kind "equal": all keys equal (q = 0), V rows of alternating sign and a magnitude marked by the row, 16 + 2 * (j % 7):
          a row dropped, added or counted twice at either edge of a token's window moves o by more than five
          tolerances (tests/test_decode_chunk_window_cpu.py asserts that from the fp64 reference);
    kind "ramp":  the score of row j is (M - j) % 128: it rises by one with every row towards the OLD end (a sawtooth of
          period 128, longer than any edge window, exact in bf16), so the row just below lo_t would carry most of the
          weight if it were let in."""
    lens = tuple(pos for pos, _ in spike_rows(window)) if kind == "spike" else edge_lens(window)
    B, H = len(lens), HKV
    rows = np.arange(M)
    qkv = torch.zeros(B, EDGE_N, H + 2 * HKV, D)
    kc = torch.zeros(B, L, M, HKV, D)
    vc = torch.zeros(B, L, M, HKV, D)
    mark = torch.from_numpy(((16.0 + 2.0 * (rows % 7)) * np.where(rows % 2, -1.0, 1.0)).astype(np.float32))
    vrow = lambda j: mark[j][:, None, None].expand(-1, HKV, D)
    if kind == "ramp":
        # q = 8 e_0, k = k_0 e_0: score = 8 k_0 / sqrt(D) = k_0 at D = 64
        assert D == 64
        qkv[:, :, :H, 0] = 8.0
        kval = torch.from_numpy(((M - rows) % 128).astype(np.float32))
        kc[:, :, :, :, 0] = kval[None, None, :, None]
    if kind == "spike":
        qkv[:, :, :H, 0] = 8.0
    vc[:] = vrow(rows)[None, None]
    for b, pos in enumerate(lens):
        j = pos + np.arange(EDGE_N)
        qkv[b, :, H + HKV:] = vrow(j)
        if kind == "spike":
            jstar = spike_rows(window)[b][1]
            if jstar < pos:
                kc[b, :, jstar, :, 0] = 64.0
            else:
                qkv[b, jstar - pos, H:H + HKV, 0] = 64.0
        if kind == "ramp":
            qkv[b, :, H:H + HKV, 0] = kval[j][:, None]
    to = lambda x: x.to(TDT[dtype])
    assert torch.equal(to(qkv).float(), qkv) and torch.equal(to(kc).float(), kc) and torch.equal(to(vc).float(), vc)
    return make_problem(dtype, D, 1, lens, (EDGE_N,) * B, qkv=to(qkv), kc=to(kc), vc=to(vc), bias=False, rot=0)


# ---- layouts -----------------------------------------------------------------------------------------------------------

def bits(t):
    return t.contiguous().view(torch.int16)


def as_float(o_bits, dtype):
    return o_bits.view(TDT[dtype]).float().numpy()


def page_size(layout):
    return int(layout[5:]) if layout.startswith("paged") else None


def page_table(ps, B):
    """(the table that lays the pools out, the number of pages): shuffled, SPARE pages nobody owns"""
    pps = M // ps
    n = B * pps + SPARE
    return np.random.default_rng(3).permutation(n)[:B * pps].astype(np.int32).reshape(B, pps), n


def storage(t):
    """a tensor of a 16-bit or an 8-bit type as its storage integers"""
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.uint8)


def to_layout(c, layout, spare_bits=0):
    """canonical [B, L, M, Hkv, D] of a 16-bit or an 8-bit type (chunk_kv8_window_ref: uint8) -> the tensor of `layout`;
    the pages no sequence owns hold spare_bits"""
    B, D = c.shape[0], c.shape[-1]
    if layout == "blmhd":
        return c.clone()
    if layout == "blhmd":
        return c.permute(0, 1, 3, 2, 4).contiguous()
    ps = page_size(layout)
    table, n = page_table(ps, B)
    pps = M // ps
    pool = torch.full((n, L, ps, HKV, D), spare_bits, dtype=storage(c[:0]).dtype).view(c.dtype)
    pool[torch.from_numpy(table.reshape(-1)).long()] = (
        c.view(B, L, pps, ps, HKV, D).permute(0, 2, 1, 3, 4, 5).reshape(B * pps, L, ps, HKV, D))
    return pool


def from_layout(t, layout, B):
    """(canonical storage integers [B, L, M, Hkv, D], those of the spare pages or None)"""
    t = storage(t.cpu())
    D = t.shape[-1]
    if layout == "blmhd":
        return t, None
    if layout == "blhmd":
        return t.permute(0, 1, 3, 2, 4).contiguous(), None
    ps = page_size(layout)
    table, n = page_table(ps, B)
    pps = M // ps
    own = torch.from_numpy(table.reshape(-1)).long()
    rest = torch.from_numpy(np.setdiff1d(np.arange(n), table.reshape(-1))).long()
    canon = t[own].view(B, pps, L, ps, HKV, D).permute(0, 2, 1, 3, 4, 5).reshape(B, L, M, HKV, D).contiguous()
    return canon, t[rest].contiguous()


# ---- the device ----------------------------------------------------------------------------------------------------------

def run(sfa, prob, layout, window, num_splits=0, varlen=False, kc=None, vc=None, table=None, spare_bits=0, lens=None):
    """One call on fresh device copies: flash_decode_chunk_window (varlen: flash_decode_varlen_window, the tokens packed),
    or the call without a window for window None.  kc / vc: canonical caches instead of the problem's own; table: the
    block_table the call gets instead of the one the pools are laid out by; lens: another seq_len.  Returns o (a list per
    sequence of [n_b, H, D] bits), kc, vc (canonical bits) and the spare pages' bits."""
    dev = torch.device("cuda:0")
    B, H, D = prob.B, prob.H, prob.D
    dt = TDT[prob.dtype]
    kd = to_layout(prob.kc if kc is None else kc, layout, spare_bits).to(dev)
    vd = to_layout(prob.vc if vc is None else vc, layout, spare_bits).to(dev)
    sl = torch.tensor(list(prob.lens if lens is None else lens), dtype=torch.int32, device=dev)
    ps = page_size(layout)
    kw = dict(num_splits=num_splits, kv_layout="paged" if ps else layout, num_heads_kv=HKV)
    if ps:
        kw["block_table"] = torch.from_numpy(page_table(ps, B)[0] if table is None else table).to(dev)
    if prob.tables:
        cos, sin = rotary_tables(prob.dtype, prob.rot)
        td = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dt).to(dev)
        kw.update(rotary_cos_table=td(cos), rotary_sin_table=td(sin))
    z = torch.zeros(0, dtype=dt, device=dev)
    biases = [z if x is None else x.to(dev) for x in (prob.qb, prob.kb, prob.vb)]
    if varlen:
        cu = np.concatenate([[0], np.cumsum(prob.ns)]).astype(np.int32)
        T = max(int(cu[-1]), 1)
        qkv = torch.zeros(T, H + 2 * HKV, D, dtype=dt)
        for b, n in enumerate(prob.ns):
            qkv[cu[b]:cu[b + 1]] = prob.qkv[b, :n]
        o = torch.full((T, H, D), 7.0, dtype=dt, device=dev)
        if prob.G == 1:
            qkv = qkv.view(T, 3, H, D)          # the reference's shape when every query head has its own kv head
        args = (qkv.to(dev), *biases, kd, vd, sl, o, torch.from_numpy(cu).to(dev), B, M, H, D, prob.rot, M, L, LAYER)
        ret = (sfa.flash_decode_varlen(*args, **kw) if window is None
               else sfa.flash_decode_varlen_window(*args, window, **kw))
    else:
        n = prob.ns[0]
        assert all(x == n for x in prob.ns)
        o = torch.full((B, n, H, D), 7.0, dtype=dt, device=dev)
        qkv = prob.qkv[:, :n].contiguous()
        if prob.G == 1:
            qkv = qkv.view(B, n, 3, H, D)
        args = (qkv.to(dev), *biases, kd, vd, sl, o, B, M, H, D, prob.rot, M, L, LAYER)
        ret = (sfa.flash_decode_chunk(*args, **kw) if window is None
               else sfa.flash_decode_chunk_window(*args, window, **kw))
    assert ret.data_ptr() == o.data_ptr()
    torch.cuda.synchronize()
    ob = bits(o.cpu())
    o_list = [ob[cu[b]:cu[b + 1]] for b in range(B)] if varlen else [ob[b] for b in range(B)]
    k_out, spare_k = from_layout(kd, layout, B)
    v_out, spare_v = from_layout(vd, layout, B)
    return SimpleNamespace(o=o_list, kc=k_out, vc=v_out, spare_k=spare_k, spare_v=spare_v)


def append_mask(prob, lens=None):
    """[B, L, M] True on every row a call must leave alone"""
    m = torch.ones((prob.B, L, M), dtype=torch.bool)
    for b, (pos, n) in enumerate(zip(prob.lens if lens is None else lens, prob.ns)):
        if 0 <= pos and pos + n <= M:
            m[b, LAYER, pos:pos + n] = False
    return m


def check_against_reference(r, prob, ref, tol=None):
    """o of every sequence within the project's tolerance, elementwise, nothing exempt; the appended rows against the
    reference (V exact, K to one storage ulp: the device's sincosf / powf and numpy's differ in the last fp32 bit of the
    angle); every other row of the caches as it was."""
    tol = TOL[prob.dtype] if tol is None else tol
    for b, (pos, n) in enumerate(zip(prob.lens, prob.ns)):
        o_ref, k_ref, v_ref = ref[b]
        np.testing.assert_allclose(as_float(r.o[b], prob.dtype), o_ref, atol=tol, rtol=tol, err_msg=f"sequence {b}")
        krow, vrow = as_float(r.kc[b, LAYER, pos:pos + n], prob.dtype), as_float(r.vc[b, LAYER, pos:pos + n], prob.dtype)
        np.testing.assert_array_equal(vrow, v_ref)
        err = np.abs(krow - k_ref)
        assert np.all(err <= ULP[prob.dtype] * np.maximum(1.0, np.abs(krow)) * 1.01), err.max()
    m = append_mask(prob)
    assert torch.equal(r.kc[m], bits(prob.kc)[m]) and torch.equal(r.vc[m], bits(prob.vc)[m])
