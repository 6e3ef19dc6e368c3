"""Structured decode problems for tests/test_decode_numerics_{cpu,gpu}.py, their oracle, and one adapter that runs a
problem through any of the five decode entry points in any cache layout.

A canonical problem (class Problem) is layout-free and packed like sfa_decode_varlen's arguments:

  q [T, H, D], k_new / v_new [T, Hkv, D]   float32, representable in `dtype`; sequence b owns rows cu[b] .. cu[b+1]
  kc, vc [B, L, M, Hkv, D]                 the caches as STORAGE BITS: uint16 (fp16 / bf16) or uint8 (e4m3, entry "kv8")
  lens [B], ns [B]                         cached rows and new tokens per sequence (ns = 1 for "decode", "kv8" and
                                           "window", one common n for "chunk", anything for "varlen")
  window, lo [B]                           entry "window": the call's window and lo[b] = max(0, pos + 1 - window), the
                                           first row sequence b may read; else None and zeros
  ks, vs [Hkv]                             the e4m3 scales of "kv8" (powers of two, see e4m3_scales), else None

The caches are kept as bits so that a problem can hold NaN patterns in the bytes the contract never reads (poisoned)
and so that "bit-identical" and "this byte was not written" are plain array comparisons.

Every sequence is described by its whole key sequence K[0 .. pos + n): rows below pos go into the cache, the rest are
the new tokens, so one builder serves every entry point.  All structured problems use rotary_embedding_dim = 0 and
no bias: the q and k the device sees are the input bits.
"""
import ctypes

import numpy as np

import kv8_ref
import window_ref
from oracle import decode_ref, round_to
from oracle.numerics import from_bits16, to_bits16

L, M, LAYER, HKV, PS, SPARE = 2, 256, 1, 2, 16, 3
TOL = {"fp16": 2e-3, "bf16": 1.6e-2}
NAN16 = 0x7FFF                                   # NaN in fp16 and in bf16
INF16 = {"fp16": 0x7C00, "bf16": 0x7F80}
NAN8 = 0x7F                                      # e4m3 NaN

SPIKE_ROWS = [0, 1, 15, 16, 31, 32, 47, 48, 63, 64, 66, 67, 95, 96, 127, 128, 133, 134, 159, 160, 199]


class Problem:
    def __init__(self, entry, dtype, G, D, seqs, rot=0, amax_scales=False, window=None):
        """seqs: dicts with pos, q [n, H, D], K / V [pos + n, Hkv, D] (float) and the builders' notes:
        hot [n] = the key row (of the sequence) that must carry the weight of token t, or -1;
        exact [n] = True where o must equal v at the hot row bit for bit; spike = the row that is 4u; ramp = +-1."""
        self.entry, self.dtype, self.G, self.D, self.rot = entry, dtype, G, D, rot
        self.Hkv, self.H = HKV, HKV * G
        self.B = len(seqs)
        self.lens = [int(s["pos"]) for s in seqs]
        self.ns = [int(s["q"].shape[0]) for s in seqs]
        self.cu = [0] + [int(x) for x in np.cumsum(self.ns)]
        self.T = self.cu[-1]
        assert entry in ("decode", "kv8", "chunk", "varlen", "window")
        assert entry == "varlen" or len(set(self.ns)) == 1 and (entry == "chunk" or self.ns[0] == 1)
        assert (entry == "window") == (window is not None) and (window is None or window >= 1)
        self.window = None if window is None else int(window)
        self.lo = [window_ref.window_lo(pos, window) for pos in self.lens]
        assert all(p + n <= M for p, n in zip(self.lens, self.ns))
        r16 = lambda x: round_to(x, dtype).astype(np.float32) + np.float32(0.0)       # (+ 0.0: no -0.0, see to_bits)
        cat = lambda key, shape: (np.concatenate([s[key] for s in seqs]) if self.T else np.zeros(shape)).astype(np.float32)
        self.q = r16(cat("q", (0, self.H, D)))
        kn, vn = [], []
        self.ks = self.vs = None
        Kf = [np.asarray(s["K"], np.float32) for s in seqs]
        Vf = [np.asarray(s["V"], np.float32) for s in seqs]
        if entry == "kv8":
            self.ks, self.vs = e4m3_scales(Kf, 1), e4m3_scales(Vf, 0)
            if amax_scales:     # amax / 448 per kv head times [0.5, 2.0] (K) and [2.0, 0.5] (V): not powers of two, distinct
                amax = lambda xs: np.max([np.abs(x).max(axis=(0, 2)) for x in xs if x.size], axis=0)
                self.ks = (amax(Kf) / 448.0 * np.array([0.5, 2.0])).astype(np.float32)
                self.vs = (amax(Vf) / 448.0 * np.array([2.0, 0.5])).astype(np.float32)
            self.kc = np.zeros((self.B, L, M, HKV, D), np.uint8)
        else:
            self.kc = np.zeros((self.B, L, M, HKV, D), np.uint16)
        self.vc = np.zeros_like(self.kc)
        for b, (K, V) in enumerate(zip(Kf, Vf)):
            pos = self.lens[b]
            self.kc[b, LAYER, :pos] = self.to_bits(K[:pos], self.ks)
            self.vc[b, LAYER, :pos] = self.to_bits(V[:pos], self.vs)
            kn.append(K[pos:])
            vn.append(V[pos:])
        self.k_new = r16(np.concatenate(kn)) if self.T else np.zeros((0, HKV, D), np.float32)
        self.v_new = r16(np.concatenate(vn)) if self.T else np.zeros((0, HKV, D), np.float32)
        self.hot = np.concatenate([np.asarray(s.get("hot", -np.ones(n)), np.int64) for s, n in zip(seqs, self.ns)])
        self.exact = np.concatenate([np.asarray(s.get("exact", np.zeros(n)), bool) for s, n in zip(seqs, self.ns)])
        self.spike = [int(s.get("spike", -1)) for s in seqs]         # per sequence: the key row that is 4u, or -1
        self.ramp = [int(s.get("ramp", 0)) for s in seqs]            # per sequence: +1 ascending, -1 descending, 0 no ramp
        self.spare_fill = 0                       # what the pages no sequence owns hold (paged layout)

    # ---- storage bits ----
    def to_bits(self, x, scale=None):
        """Storage bits of x.  A -0.0 becomes +0.0 first: x * 1 - y * 0 of a rotation by no angle may or may not keep
        the sign of a zero, and no test here is about that."""
        x = round_to(x, self.dtype) + np.float32(0.0)
        if self.entry == "kv8":
            return kv8_ref.quantize(x, scale)
        return to_bits16(x, self.dtype)

    def values(self, bits, scale=None):
        """float64 values of cache bits [..., Hkv, D] (NaN / Inf where the bits say so)"""
        if self.entry == "kv8":
            return kv8_ref.dequantize(bits, scale)
        return from_bits16(bits, self.dtype).astype(np.float64)

    def seq_of(self, r):
        b = int(np.searchsorted(self.cu, r, side="right")) - 1
        return b, r - self.cu[b]

    def unread_mask(self):
        """[B, L, M] True on every cache row the contract does not name: the other layers, and the rows of idx_layer
        from pos + n on and (a window) below lo."""
        m = np.ones((self.B, L, M), bool)
        for b in range(self.B):
            m[b, LAYER, self.lo[b]:self.lens[b] + self.ns[b]] = False
        return m

    def poisoned(self, pattern=None):
        """A copy whose unread cache rows (and, paged, spare pages) hold `pattern` in every element: NaN by default."""
        import copy
        p = copy.copy(self)
        pat = pattern if pattern is not None else (NAN8 if self.entry == "kv8" else NAN16)
        p.kc, p.vc = self.kc.copy(), self.vc.copy()
        m = self.unread_mask()
        p.kc[m] = pat
        p.vc[m] = pat
        p.spare_fill = pat
        return p

    def pages_needed(self, b):
        return 0 if self.ns[b] == 0 else (self.lens[b] + self.ns[b] - 1) // PS + 1


def e4m3_scales(arrays, doubled):
    """One power-of-two scale per kv head, the smallest with amax / scale <= 256 (inside e4m3's +-448), and that of
    head `doubled` doubled so that the two heads differ: dividing by it and multiplying back are exact, so an e4m3-exact value stays
    one."""
    amax = np.max([np.abs(a).max(axis=(0, 2)) if a.size else np.zeros(HKV) for a in arrays], axis=0)
    e = np.ceil(np.log2(np.maximum(amax, 2.0 ** -20) / 256.0))
    e[doubled] += 1
    return (2.0 ** e).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------
# the oracle
# ---------------------------------------------------------------------------------------------------------------------

def oracle(p, scale=None, window=None):
    """fp64 reference of the whole call: dict(o [T, H, D] float32 unrounded, kc, vc = the caches afterwards, as bits).
    16-bit entries: oracle.decode_ref token by token per sequence; kv8: kv8_ref.decode_kv8_ref; window:
    window_ref.decode_window_ref, which looks at the rows [lo, pos] only (window=: another window than the problem's)."""
    kc, vc = p.kc.copy(), p.vc.copy()
    if p.entry == "window":
        layer = lambda c: from_bits16(c[:, LAYER:LAYER + 1], p.dtype)                    # [B, 1, M, Hkv, D]
        ref = window_ref.decode_window_ref(p.q, p.k_new, p.v_new, layer(kc), layer(vc), p.lens, 0, p.rot,
                                           p.window if window is None else window, p.dtype, scale=scale)
        for b, pos in enumerate(p.lens):
            kc[b, LAYER, pos] = to_bits16(ref["k_row"][b], p.dtype)
            vc[b, LAYER, pos] = to_bits16(ref["v_row"][b], p.dtype)
        return dict(o=ref["o"], kc=kc, vc=vc)
    o = np.zeros((p.T, p.H, p.D), np.float32)
    G = p.G
    if p.entry == "kv8":
        qkv = np.concatenate([p.q, p.k_new, p.v_new], axis=1)
        with np.errstate(invalid="ignore"):
            ref = kv8_ref.decode_kv8_ref(qkv, kc, vc, p.lens, LAYER, p.rot, p.dtype, p.ks, p.vs, scale=scale)
        return dict(o=ref["o"], kc=kc, vc=vc)
    for b in range(p.B):
        if p.ns[b] == 0:
            continue
        kf = np.repeat(from_bits16(kc[b, LAYER], p.dtype), G, axis=1)[None, None]        # [1, 1, M, H, D]
        vf = np.repeat(from_bits16(vc[b, LAYER], p.dtype), G, axis=1)[None, None]
        for t in range(p.ns[b]):
            r = p.cu[b] + t
            qkv_t = np.stack([p.q[r], np.repeat(p.k_new[r], G, 0), np.repeat(p.v_new[r], G, 0)])[None]
            o[r] = decode_ref(qkv_t, kf, vf, [p.lens[b] + t], 0, p.rot, dtype=p.dtype, scale=scale)["o"][0]
        new = slice(p.lens[b], p.lens[b] + p.ns[b])
        kc[b, LAYER, new] = to_bits16(kf[0, 0, new, ::G], p.dtype)
        vc[b, LAYER, new] = to_bits16(vf[0, 0, new, ::G], p.dtype)
    return dict(o=o, kc=kc, vc=vc)


def scores_log2(p, ref, r, scale=None, causal=True):
    """[H, pos + n] the scores of packed token r in log2 units over its sequence's keys (from the caches after the call,
    `ref` = oracle(p)); keys the token must not see (later tokens; a window: the rows below lo) are -inf unless
    causal=False."""
    b, t = p.seq_of(r)
    pos, n = p.lens[b], p.ns[b]
    K = np.repeat(p.values(ref["kc"][b, LAYER, :pos + n], p.ks), p.G, axis=1)               # [pos + n, H, D]
    sc = np.einsum("hd,thd->ht", p.q[r].astype(np.float64), K) * (p.D ** -0.5 if scale is None else scale) * np.log2(np.e)
    if causal:
        sc[:, pos + t + 1:] = -np.inf
        sc[:, :p.lo[b]] = -np.inf
    return sc


def weights(p, ref, r, scale=None, causal=True):
    """[H, pos + n] the fp64 softmax weights of packed token r"""
    sc = scores_log2(p, ref, r, scale, causal)
    w = np.exp2(sc - sc.max(axis=1, keepdims=True))
    return w / w.sum(axis=1, keepdims=True)


# ---------------------------------------------------------------------------------------------------------------------
# builders: one sequence each.  u is a +-1 sign vector per kv head, q = u + 0.25 N(0,1) for every query head of the
# group and every token, V = N(0,1); K is what the case is named for.
# ---------------------------------------------------------------------------------------------------------------------

def _rng(*key):
    return np.random.default_rng([0 if k is None else int(k) + 1 for k in key])


def _frame(rng, G, D, pos, n, e4m3):
    u = rng.choice([-1.0, 1.0], size=(HKV, D))
    q = np.repeat(u, G, axis=0)[None] + 0.25 * rng.standard_normal((n, HKV * G, D))
    K = 0.25 * rng.standard_normal((pos + n, HKV, D))
    V = rng.standard_normal((pos + n, HKV, D))
    if e4m3:            # multiples of 1/8 in [-2, 2]: e4m3-exact, and they stay exact under a power-of-two scale;
        # none of them 0: where o must be the bits of v, the other keys' ~1e-11 of weight would show against a zero
        V = np.clip(np.round(V * 8.0) / 8.0, -2.0, 2.0)
        V = np.where(V == 0.0, 0.125, V)
    return u, q, K, V


def seq_spike(seed, G, D, pos, n=1, row=None, new=None, cold_new=False, e4m3=False):
    """K[row] = 4u among 0.25 N(0,1) keys.  row: a cached row; new = j: the spike is new token j instead (tokens
    t >= j return v_new[j] exactly, tokens t < j must not see it); cold_new: every new key is -4u (negligible)."""
    rng = _rng(seed, G, D, pos, n, row, new)
    u, q, K, V = _frame(rng, G, D, pos, n, e4m3)
    if cold_new:
        K[pos:] = -4.0 * u
    hot = np.full(n, -1)
    exact = np.zeros(n, bool)
    if new is not None:
        K[pos + new] = 4.0 * u
        hot[new:] = pos + new
        exact[new:] = True
    else:
        K[row] = 4.0 * u
        hot[:] = row
    return dict(pos=pos, q=q, K=K, V=V, hot=hot, exact=exact, spike=row if new is None else pos + new)


def seq_ramp(seed, G, D, pos, n=1, ascending=True, e4m3=False):
    """K[r] = (4 r / last) u, last = pos + n - 1: ascending, the running max moves in every tile; descending (r -> last - r),
    it is fixed after the first."""
    rng = _rng(seed, G, D, pos, n, ascending)
    u, q, K, V = _frame(rng, G, D, pos, n, e4m3)
    last = pos + n - 1
    r = np.arange(pos + n, dtype=np.float64)
    f = 4.0 * (r if ascending else last - r) / last
    K = f[:, None, None] * u[None]
    return dict(pos=pos, q=q, K=K, V=V, ramp=1 if ascending else -1)


def seq_equal(seed, G, D, pos, n=1, e4m3=False):
    """every key = u: o = the mean of V over the rows a token sees"""
    rng = _rng(seed, G, D, pos, n)
    u, q, K, V = _frame(rng, G, D, pos, n, e4m3)
    K = np.broadcast_to(u, K.shape).copy()
    return dict(pos=pos, q=q, K=K, V=V)


def seq_below(seed, G, D, pos, n=1, hot_new=False, e4m3=False):
    """every cached key = -4u + 0.25 N(0,1) and the new keys = -4u: all scores far below zero, an ordinary softmax once
    the max is subtracted.  hot_new: new token 0 = +4u, so every token returns v_new[0] exactly."""
    rng = _rng(seed, G, D, pos, n, hot_new)
    u, q, K, V = _frame(rng, G, D, pos, n, e4m3)
    K = K - 4.0 * u
    K[pos:] = -4.0 * u
    hot = np.full(n, -1)
    exact = np.zeros(n, bool)
    if hot_new:
        K[pos] = 4.0 * u
        hot[:] = pos
        exact[:] = True
    return dict(pos=pos, q=q, K=K, V=V, hot=hot, exact=exact, spike=pos if hot_new else -1)


def seq_extreme(seed, G, D, pos, n=1, e4m3=False):
    """q and K = 6 N(0,1), the last third of the keys times 3 (tests/test_prefill_gpu.py, test_prefill_extreme_logits)"""
    rng = _rng(seed, G, D, pos, n)
    _, _, _, V = _frame(rng, G, D, pos, n, e4m3)
    q = 6.0 * rng.standard_normal((n, HKV * G, D))
    K = 6.0 * rng.standard_normal((pos + n, HKV, D))
    K[2 * (pos + n) // 3:] *= 3.0
    return dict(pos=pos, q=q, K=K, V=V)


def seq_normal(seed, G, D, pos, n=1, e4m3=False):
    """N(0,1) everywhere (sections B and C)"""
    rng = _rng(seed, G, D, pos, n)
    return dict(pos=pos, q=rng.standard_normal((n, HKV * G, D)), K=rng.standard_normal((pos + n, HKV, D)),
                V=rng.standard_normal((pos + n, HKV, D)))


# ---- the edges of a sliding window (entry "window"): one sequence per lo, pos = lo + window - 1, so that every cached row
# from lo on is inside the window and row lo - 1 is the first one outside ----

WINDOWS = (17, 32, 40, 100)
WINDOW_LOS = [0, 1, 15, 16, 17, 31, 32, 33, 48, 63, 64, 65, 96, 127, 128, 129, 156]
EDGE_KINDS = ["edge_in", "edge_last", "edge_out", "ramp_through", "equal"]
STRESS_WINDOW = 40                               # the window of sections A (the kinds it shares), B and C
UNREAD_WINDOWS = (40, 16, 1)                     # section C: 16 = a window that begins on a page boundary at pos 15, 31,
#                                                  63; 1 = no cached row is read at all, lo = pos on no tile boundary


def equal_magnitude(window):
    """|V| of the marked rows of seq_window_equal: a one-row error moves o by about A / window, which must clear 5 times
    the tolerance of bf16 (tests/test_decode_numerics_cpu.py, test_window_equal_marks_every_one_row_error)"""
    return 8.0 if window <= 40 else 32.0


def seq_window_edge(seed, G, D, lo, window, where):
    """K[row] = 4u among 0.25 N(0,1) keys.  where "in": row = lo, the first row of the window; "last": row = pos - 1, the
    last cached row; "out": row = lo - 1, the last row below the window -- finite, and nobody may see it."""
    pos = lo + window - 1
    row = {"in": lo, "last": pos - 1, "out": lo - 1}[where]
    assert 0 <= row < pos
    rng = _rng(seed, G, D, lo, window, row)
    u, q, K, V = _frame(rng, G, D, pos, 1, False)
    K[row] = 4.0 * u
    return dict(pos=pos, q=q, K=K, V=V, hot=[-1 if where == "out" else row], spike=row)


def seq_window_ramp(seed, G, D, lo, window, through):
    """through: K[r] = 4 (pos - r) / window * u for EVERY row r <= pos, so that the largest score of the window is at row
    lo and every row below lo would beat it.  Else the ascending ramp K[r] = 4 (r - lo) / (window - 1) * u over [lo, pos]
    (the running max moves in every tile of the window) above rows of zeros."""
    pos = lo + window - 1
    rng = _rng(seed, G, D, lo, window, through)
    u, q, K, V = _frame(rng, G, D, pos, 1, False)
    r = np.arange(pos + 1, dtype=np.float64)
    f = 4.0 * (pos - r) / window if through else 4.0 * np.maximum(r - lo, 0.0) / (window - 1)
    K = f[:, None, None] * u[None]
    return dict(pos=pos, q=q, K=K, V=V, ramp=-1 if through else 1)


def seq_window_equal(seed, G, D, lo, window):
    """every key of the sequence = u, below the window as well, V = N(0,1): o = the mean of V over exactly the rows
    lo .. pos.  Rows lo - 1, lo and pos - 1 of V are +-A (a sign per element, A = equal_magnitude(window)), so that each
    one-row error -- row lo dropped, row lo counted twice, row lo - 1 added, row pos - 1 dropped -- moves o by ~A / window."""
    pos = lo + window - 1
    rng = _rng(seed, G, D, lo, window)
    u, q, K, V = _frame(rng, G, D, pos, 1, False)
    K = np.broadcast_to(u, K.shape).copy()
    for row in (lo - 1, lo, pos - 1):
        if row >= 0:
            V[row] = equal_magnitude(window) * rng.choice([-1.0, 1.0], size=V[row].shape)
    return dict(pos=pos, q=q, K=K, V=V)


def window_los(window, kind):
    """the lo of each sequence of a window-edge batch: pos = lo + window - 1 stays below M; edge_out needs a row lo - 1"""
    return [lo for lo in WINDOW_LOS if lo + window - 1 <= M - 1 and (kind != "edge_out" or lo >= 1)]


def window_edges(dtype, G, D, kind, window):
    """The window-edge problems: one batch per (kind, window), a sequence per lo (ramp_through: two, the ramp that goes
    on below lo and the ascending one)."""
    kw = dict(G=G, D=D, window=window)
    los = window_los(window, kind)
    if kind in ("edge_in", "edge_last", "edge_out"):
        seqs = [seq_window_edge(500 + i, lo=lo, where=kind[5:], **kw) for i, lo in enumerate(los)]
    elif kind == "ramp_through":
        seqs = [seq_window_ramp(600 + i, lo=lo, through=t, **kw) for i, lo in enumerate(los) for t in (True, False)]
    elif kind == "equal":
        seqs = [seq_window_equal(700 + i, lo=lo, **kw) for i, lo in enumerate(los)]
    else:
        raise ValueError(kind)
    return Problem("window", dtype, G, D, seqs, window=window)


VARLEN_NS = [1, 3, 40, 0, 17]
CHUNK_SPIKES = [(pos, j) for pos in (0, 30, 100) for j in (0, 1, 31, 32, 39)]     # n = 40


def softmax_stress(entry, dtype, G, D, kind):
    """The problems of section A, one batch per kind: a sequence per case.  Entry "window": at window STRESS_WINDOW."""
    e = entry == "kv8"
    kw = dict(G=G, D=D, e4m3=e)
    n = {"decode": 1, "kv8": 1, "chunk": 5, "window": 1}.get(entry)
    window = STRESS_WINDOW if entry == "window" else None
    if entry == "varlen":
        ns = VARLEN_NS
        if kind == "spike":
            seqs = [seq_spike(1, pos=200, n=ns[0], row=66, **kw), seq_spike(2, pos=30, n=ns[1], new=1, **kw),
                    seq_spike(3, pos=100, n=ns[2], new=32, **kw), seq_normal(4, pos=50, n=ns[3], **kw),
                    seq_spike(5, pos=0, n=ns[4], new=16, **kw)]
        elif kind == "ramp":
            seqs = [seq_ramp(1, pos=200, n=ns[0], **kw), seq_ramp(2, pos=252, n=ns[1], ascending=False, **kw),
                    seq_ramp(3, pos=100, n=ns[2], **kw), seq_normal(4, pos=50, n=ns[3], **kw),
                    seq_ramp(5, pos=0, n=ns[4], ascending=False, **kw)]
        elif kind == "extreme":
            seqs = [seq_extreme(i, pos=pos, n=k, **kw) for i, (pos, k) in enumerate(zip([200, 30, 100, 50, 0], ns))]
        else:
            raise ValueError(kind)
        return Problem(entry, dtype, G, D, seqs)
    if kind == "spike":
        seqs = [seq_spike(r, pos=200, n=n, row=r, **kw) for r in SPIKE_ROWS]
        seqs += [seq_spike(300, pos=200, n=n, new=0, **kw), seq_spike(301, pos=200, n=n, row=100, cold_new=True, **kw)]
    elif kind == "chunk_spike":
        seqs = [seq_spike(400 + i, pos=pos, n=40, new=j, **kw) for i, (pos, j) in enumerate(CHUNK_SPIKES)]
    elif kind == "ramp":
        seqs = [seq_ramp(i, pos=pos, n=n, ascending=a, **kw)
                for i, (pos, a) in enumerate([(200, True), (200, False), (256 - n, True), (256 - n, False)])]
    elif kind == "equal":
        seqs = [seq_equal(i, pos=pos, n=n, **kw) for i, pos in enumerate([0, 1, 33, 200])]
    elif kind == "below":
        seqs = [seq_below(i, pos=200, n=n, hot_new=h, **kw) for i, h in enumerate([False, True])]
    elif kind == "extreme":
        seqs = [seq_extreme(i, pos=pos, n=n, **kw) for i, pos in enumerate([200, 255 if n == 1 else 256 - n, 33])]
    else:
        raise ValueError(kind)
    return Problem(entry, dtype, G, D, seqs, window=window)


def stress_kinds(entry):
    if entry == "varlen":
        return ["spike", "ramp", "extreme"]
    if entry == "window":                       # its spikes, ramps and equal keys are the window-edge problems
        return ["below", "extreme"]
    return ["spike", "ramp", "equal", "below", "extreme"] + (["chunk_spike"] if entry == "chunk" else [])


UNREAD_POS = [0, 1, 15, 16, 31, 32, 33, 63, 64, 65, 100, 129, 254]
UNREAD_CHUNK_POS = [0, 19, 51, 52, 115, 200]                   # n = 13: pos + n lands on, before and after a 64 boundary
VARLEN_POS = [200, 30, 100, 50, 0]


def normal_problem(entry, dtype, G, D, rot=0, stale=False, amax_scales=False, window=None):
    """N(0,1) data at the positions of section C (also section B's problem).  stale: the batch of the stale-workspace
    case instead: it contains pos = 0, and a sequence without tokens for varlen.  Entry "window": at `window`
    (STRESS_WINDOW if None)."""
    if entry == "window" and window is None:
        window = STRESS_WINDOW
    kw = dict(G=G, D=D)
    if entry == "varlen":
        seqs = [seq_normal(i, pos=pos, n=n, **kw) for i, (pos, n) in enumerate(zip(VARLEN_POS, VARLEN_NS))]
    elif entry == "chunk":
        seqs = [seq_normal(i, pos=pos, n=13, **kw) for i, pos in enumerate([0, 5, 200] if stale else UNREAD_CHUNK_POS)]
    else:
        seqs = [seq_normal(i, pos=pos, **kw) for i, pos in enumerate([0, 2, 129] if stale else UNREAD_POS)]
    return Problem(entry, dtype, G, D, seqs, rot=rot, amax_scales=amax_scales, window=window)


# ---------------------------------------------------------------------------------------------------------------------
# the kernel coverage of the issue: (entry, G, D, layout, dtype, knobs)
# ---------------------------------------------------------------------------------------------------------------------

def _configs():
    c = []
    # one query head per kv head (decode_kernel.hip)
    c += [("decode", 1, 64, "blmhd", "fp16", {}), ("decode", 1, 128, "blmhd", "bf16", {}),
          ("decode", 1, 128, "blhmd", "fp16", {}), ("decode", 1, 128, "paged", "bf16", {"decode_nt": 1}),
          ("decode", 1, 256, "blmhd", "fp16", {})]
    # VALU grouped (decode_gqa_kernel.hip)
    c += [("decode", 2, 128, "blmhd", "bf16", {}), ("decode", 4, 64, "paged", "fp16", {"decode_nt": 1}),
          ("decode", 8, 128, "blhmd", "fp16", {"decode_gqa_mfma": 0})]
    # matrix cores (decode_gqa_mfma_kernel.hip): blhmd = direct operand-layout loads, blmhd / paged through LDS
    i = 0
    for G, D in ((4, 128), (8, 64), (8, 256), (16, 128)):
        for layout in ("blhmd", "blmhd", "paged"):
            c.append(("decode", G, D, layout, ("bf16", "fp16")[i % 2], {"decode_nt": 1} if (G, D, layout) == (8, 64, "blmhd") else {}))
            i += 1
    # fp8 caches (decode_kv8_kernel.hip)
    c += [("kv8", 1, 128, "blmhd", "bf16", {}), ("kv8", 4, 128, "blmhd", "fp16", {}), ("kv8", 4, 128, "blhmd", "bf16", {}),
          ("kv8", 4, 128, "paged", "fp16", {"decode_nt": 1}), ("kv8", 16, 128, "blmhd", "bf16", {}),
          ("kv8", 2, 64, "blmhd", "fp16", {})]
    # the chunk body, through both of its entry points (it has no non-temporal loads: no decode_nt configuration)
    for entry in ("chunk", "varlen"):
        i = 0
        for D in (64, 128):
            for G in (1, 8):
                for layout in ("blmhd", "paged"):
                    c.append((entry, G, D, layout, ("fp16", "bf16")[(i + (D == 128)) % 2], {}))
                    i += 1
    # the sliding window (decode_window_kernel.hip): one matrix-core kernel for every group size, G = 1 and 2 on padded
    # query columns; blhmd = operand-layout loads, blmhd = row-major, paged.  Every (head_dim, layout) pair, every G
    # three times (G = 1 and 2 on each load path), non-temporal loads forced once per load path.
    shapes = [(64, "blhmd"), (64, "blmhd"), (64, "paged"), (128, "blhmd"), (128, "blmhd"), (128, "paged"),
              (256, "blhmd"), (256, "blmhd"), (256, "paged"), (128, "paged"), (64, "blmhd"), (128, "paged"),
              (256, "paged"), (128, "blmhd"), (64, "blhmd")]
    for i, (D, layout) in enumerate(shapes):
        c.append(("window", (1, 2, 4, 8, 16)[i % 5], D, layout, ("bf16", "fp16")[i % 2], {"decode_nt": 1} if i in (1, 5, 6) else {}))
    return c


CONFIGS = _configs()


def config_id(c):
    entry, G, D, layout, dtype, knobs = c
    return f"{entry}-G{G}-D{D}-{layout}-{dtype}" + "".join(f"-{k}{v}" for k, v in knobs.items())


# ---------------------------------------------------------------------------------------------------------------------
# the adapter (GPU): canonical problem -> device tensors of one layout -> entry point -> canonical results
# ---------------------------------------------------------------------------------------------------------------------

def page_table(B):
    """(the table that lays the pools out [B, M / PS], the number of pages): shuffled, SPARE pages nobody owns"""
    pps = M // PS
    num_pages = B * pps + SPARE
    return np.random.default_rng(3).permutation(num_pages)[:B * pps].astype(np.int32).reshape(B, pps), num_pages


def call_table(p, table, beyond=None, below=None):
    """the table a call gets: `beyond` (e.g. -1) in every entry past the last page a sequence needs, `below` in every
    entry of a page that lies wholly below lo (a window), that is entries [0, lo // PS)"""
    t = table.copy()
    for b in range(p.B):
        if beyond is not None:
            t[b, p.pages_needed(b):] = beyond
        if below is not None:
            t[b, :p.lo[b] // PS] = below
    return t


class Run:
    """The device side of one problem in one layout.  .call(...) makes the operator call; .result() brings o and the
    caches back in canonical form (bits)."""

    def __init__(self, p, layout, table_beyond=None, table_below=None):
        import torch
        self.torch, self.p, self.layout = torch, p, layout
        self.dev = dev = torch.device("cuda:0")
        self.tdt = {"fp16": torch.float16, "bf16": torch.bfloat16}[p.dtype]
        self.table = self.num_pages = self.block_table = None
        if layout == "paged":
            self.table, self.num_pages = page_table(p.B)
            self.block_table = torch.from_numpy(call_table(p, self.table, table_beyond, table_below)).to(dev)
        self.kc, self.vc = self._to_layout(p.kc), self._to_layout(p.vc)
        t16 = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(self.tdt).to(dev)
        H, Hkv, D = p.H, p.Hkv, p.D
        if p.G == 1:
            qkv = torch.stack([t16(p.q), t16(p.k_new), t16(p.v_new)], dim=1)                # [T, 3, H, D]
        else:
            qkv = torch.cat([t16(p.q), t16(p.k_new), t16(p.v_new)], dim=1)                  # [T, H + 2 Hkv, D]
        if p.entry == "chunk":
            qkv = qkv.view(p.B, p.ns[0], *qkv.shape[1:])
        self.qkv = qkv.contiguous()
        o_shape = (p.B, p.ns[0], H, D) if p.entry == "chunk" else (p.T, H, D)
        self.o = torch.full(o_shape, 7.0, dtype=self.tdt, device=dev)
        self.seq_len = torch.tensor(p.lens, dtype=torch.int32, device=dev)
        self.cu = torch.tensor(p.cu, dtype=torch.int32, device=dev)
        self.k_scale = self.v_scale = None
        if p.entry == "kv8":
            self.k_scale, self.v_scale = torch.from_numpy(p.ks).to(dev), torch.from_numpy(p.vs).to(dev)

    def _bits_tensor(self, a):
        torch = self.torch
        if a.dtype == np.uint8:
            return torch.from_numpy(np.ascontiguousarray(a))
        return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).view(self.tdt)

    def _to_layout(self, c):
        torch, p = self.torch, self.p
        t = self._bits_tensor(c)
        if self.layout == "blhmd":
            t = t.permute(0, 1, 3, 2, 4).contiguous()
        elif self.layout == "paged":
            pool = self._bits_tensor(np.full((self.num_pages, L, PS, p.Hkv, p.D), p.spare_fill, dtype=c.dtype))
            idx = torch.from_numpy(self.table.reshape(-1)).long()
            pool[idx] = t.view(p.B, L, M // PS, PS, p.Hkv, p.D).permute(0, 2, 1, 3, 4, 5).reshape(-1, L, PS, p.Hkv, p.D)
            t = pool
        return t.to(self.dev)

    def _from_layout(self, t):
        torch, p = self.torch, self.p
        t = t.cpu()
        t = t if t.dtype == torch.uint8 else t.view(torch.int16)
        spare = None
        if self.layout == "blhmd":
            t = t.permute(0, 1, 3, 2, 4)
        elif self.layout == "paged":
            idx = torch.from_numpy(self.table.reshape(-1)).long()
            rest = torch.from_numpy(np.setdiff1d(np.arange(self.num_pages), self.table.reshape(-1))).long()
            spare = t[rest].contiguous().numpy()
            t = t[idx].view(p.B, M // PS, L, PS, p.Hkv, p.D).permute(0, 2, 1, 3, 4, 5).reshape(p.B, L, M, p.Hkv, p.D)
        a = t.contiguous().numpy()
        view = (lambda x: x) if a.dtype == np.uint8 else (lambda x: x.view(np.uint16))
        return view(a), None if spare is None else view(spare)

    def positional(self):
        """the positional arguments every operator takes after the biases' place: caches, seq_len, o, then the sizes"""
        p = self.p
        return (self.kc, self.vc, self.seq_len, self.o), (p.B, M, p.H, p.D, p.rot, M, L, LAYER)

    def keywords(self, num_splits=0, softmax_scale=None):
        p = self.p
        kw = dict(num_splits=num_splits, kv_layout=self.layout, softmax_scale=softmax_scale)
        if p.G != 1 or p.entry == "kv8":
            kw["num_heads_kv"] = p.Hkv
        if self.layout == "paged":
            kw["block_table"] = self.block_table
        if p.entry == "kv8":
            kw.update(k_scale=self.k_scale, v_scale=self.v_scale)
        return kw

    def call(self, sfa, num_splits=0, softmax_scale=None):
        p = self.p
        (kc, vc, sl, o), sizes = self.positional()
        kw = self.keywords(num_splits, softmax_scale)
        if p.entry == "varlen":
            ret = sfa.flash_decode_varlen(self.qkv, None, None, None, kc, vc, sl, o, self.cu, *sizes, **kw)
        elif p.entry == "window":
            ret = sfa.flash_decode_window(self.qkv, None, None, None, kc, vc, sl, o, *sizes, p.window, **kw)
        else:
            fn = {"decode": sfa.flash_decode, "kv8": sfa.flash_decode_kv8, "chunk": sfa.flash_decode_chunk}[p.entry]
            ret = fn(self.qkv, None, None, None, kc, vc, sl, o, *sizes, **kw)
        assert ret.data_ptr() == o.data_ptr()
        return self

    def call_exact_workspace(self, num_splits, fill):
        """The same call through the C ABI with a workspace of exactly the size the library asks for, its body
        prefilled with `fill` (tests/exact_workspace.py)."""
        from exact_workspace import call_with_exact_workspace
        from starflashattention_amd import _lib, ops
        p = self.p
        lib = _lib.load()
        (kc, vc, sl, o), sizes = self.positional()
        kw = self.keywords()
        a, *_ = ops._decode_args(self.qkv, None, None, None, kc, vc, sl, o, *sizes, None, None, None, self.layout,
                                 kw.get("block_table"), kw.get("num_heads_kv"),
                                 tokens=p.ns[0] if p.entry == "chunk" else None,
                                 packed=p.T if p.entry == "varlen" else None, kv8=p.entry == "kv8")
        B, H, Hkv, D, S = p.B, p.H, p.Hkv, p.D, num_splits
        vp = lambda t: ctypes.c_void_p(t.data_ptr())
        if p.entry == "chunk":
            n = p.ns[0]
            a.stride = 0
            nbytes = lib.sfa_decode_chunk_workspace_bytes(B, H, Hkv, D, M, n, S)
            call = lambda args, stream: lib.sfa_decode_chunk(args, n, 0, stream)
        elif p.entry == "varlen":
            a.stride = 0
            nbytes = lib.sfa_decode_varlen_workspace_bytes(B, H, Hkv, D, M, p.T, S)
            call = lambda args, stream: lib.sfa_decode_varlen(args, vp(self.cu), p.T, 0, stream)
        else:
            a.stride = (H + 2 * Hkv) * D
            nbytes = lib.sfa_decode_workspace_bytes(B, H, D, M, S)
            call = lib.sfa_decode if p.entry == "decode" else (
                lambda args, stream: lib.sfa_decode_kv8(args, vp(self.k_scale), vp(self.v_scale), stream))
        call_with_exact_workspace(a, nbytes, S, call, self.dev, fill=fill)
        return self

    def result(self):
        """dict(o = bits [T, H, D], kc, vc = canonical bits, spare_k, spare_v = the bits of the spare pages or None)"""
        self.torch.cuda.synchronize()
        o = self.o.view(self.torch.int16).cpu().numpy().view(np.uint16).reshape(self.p.T, self.p.H, self.p.D)
        kc, sk = self._from_layout(self.kc)
        vc, sv = self._from_layout(self.vc)
        return dict(o=o, kc=kc, vc=vc, spare_k=sk, spare_v=sv)


def run(sfa, p, layout, num_splits=0, softmax_scale=None, table_beyond=None, knobs=None, table_below=None):
    """One call of p's entry point on fresh device copies; the debug knobs are set for the call and restored."""
    knobs = knobs or {}
    for k, v in knobs.items():
        sfa.debug_set(k, v)
    try:
        res = Run(p, layout, table_beyond, table_below).call(sfa, num_splits, softmax_scale).result()
    finally:
        for k in knobs:
            sfa.debug_set(k, -1)
    return res
