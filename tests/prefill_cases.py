"""Structured prefill problems for tests/test_prefill_numerics_{cpu,gpu}.py, their oracle, the kernel configurations and
one adapter that fills sfa_prefill_args itself (so that the lse pointer and every stride are the test's to choose).

A problem (class Problem) holds q [B, Hq, Sq, D] and k, v [B, Hkv, Sk, D] as float32 arrays representable in `dtype`, one
structured case per (batch, kv head) slot, and the builders' notes:

  spike [B, Hkv]   the key row that is 4u in this slot, or -1
  hot              the query rows that are aligned with u (None: every row); only these must return V[spike] exactly

The oracle is oracle.sdpa_ref (fp64) on these very arrays, for o and lse, cached per (causal, scale) in the problem.
Key tiles are 64 rows (8-wave and 4-wave kernels; the 4-wave staging moves 16 rows per wave) or 32 rows (128-row kernel,
both head_dim 256 kernels), query tiles 256 or 128 rows, rescale decisions are taken per 32 query rows: Sk = 299 is ragged
for both tile sizes, and (Sq, Sk) = (299, 299), (100, 299), (299, 100) are the three alignments of the bottom-right causal
mask (in the last one rows 0 .. 198 see no key and row 199 sees exactly key 0).
"""
import ctypes

import numpy as np

from oracle import round_to, sdpa_ref
from oracle.numerics import from_bits16, to_bits16
from test_prefill_gpu import IMPLS, LSE_TOL, TOL, select_impl, serves          # the project's kernel table and tolerances

NAN16 = 0x7FFF                                   # NaN in fp16 and in bf16
INF16 = {"fp16": 0x7C00, "bf16": 0x7F80}
LOG2E = 1.4426950408889634

SHAPES = [(299, 299), (100, 299), (299, 100)]    # (Sq, Sk): the three alignments of the causal mask
ONE_ROW_SHAPES = [(1, 299), (299, 1)]
SPIKE_ROWS = [0, 1, 15, 16, 31, 32, 47, 48, 63, 64, 65, 127, 128, 191, 192, 255, 256, 257, 287, 288, 298]
ALONE_ROWS = [0, 63, 77, 141, 191, 256, 298]     # first / last / middle rows of the 32-row blocks 0, 1, 2, 4, 5, 8, 9
EQUAL_A = 32.0                                   # |V[Sk - 1]| of the "equal" kind
# K = c_t u on key tile t of 64 rows, q = u: the row max rises by c (D / sqrt(D)) log2(e) per unit of c
STAIR64 = {64: [0, 0.609375, 1.390625, 2.0, 2.78125], 128: [0, 0.421875, 0.96875, 1.390625, 1.9375],
           256: [0, 0.296875, 0.6875, 0.984375, 1.375]}
KINDS = ["spike", "alone", "staircase64", "staircase32", "ramp", "equal", "below"]
CHAINED = [(2, 16, 16, 2304, 64), (2, 16, 16, 2304, 192), (2, 16, 4, 2304, 320)]       # B, Hq, Hkv, Sq, Sk; head_dim 128
CHAIN_RAMP = (3.5, 4.0)      # K[r] = (3.5 + 0.5 r / (Sk - 1)) u: with q = +-u the row maxima are at least (3.5 + 3.5)
#                              sqrt(128) log2(e) = 114 log2 units apart, whichever keys a row sees; the 0.25 N(0,1) on q
#                              moves q.u by at most 4 sigma = 0.25 * 4 / sqrt(128) = 9 % of it: more than 103 remain


def stair32(D):
    """c_t for ten key tiles of 32 rows: multiples of 1/32 (exact in bf16 up to 8), each the one nearest to a rise of 7
    (odd t) or 9 (even t >= 2) log2 units over the tile before.  The grid step is at most 0.72 log2 units (head_dim 256),
    so every rise lands within 0.36 of its target, inside 6.5-7.5 / 8.5-9.5."""
    unit = np.sqrt(D) * LOG2E
    c = [0.0]
    for t in range(1, 10):
        c.append(np.round((c[-1] + (7.0 if t % 2 else 9.0) / unit) * 32.0) / 32.0)
    return c


class Problem:
    def __init__(self, kind, dtype, D, G, Sq, Sk, q, k, v, spike=None, hot=None):
        self.kind, self.dtype, self.D, self.G, self.Sq, self.Sk = kind, dtype, D, G, Sq, Sk
        r16 = lambda x: round_to(np.asarray(x, np.float32), dtype).astype(np.float32)
        self.q, self.k, self.v = r16(q), r16(k), r16(v)
        self.B, self.Hq = self.q.shape[:2]
        self.Hkv = self.k.shape[1]
        assert self.Hq == self.Hkv * G and self.q.shape[2:] == (Sq, D) and self.k.shape == self.v.shape == (self.B, self.Hkv, Sk, D)
        self.spike = np.full((self.B, self.Hkv), -1) if spike is None else np.asarray(spike)
        self.hot = None if hot is None else [r for r in hot if r < Sq]
        self._ref, self._dev = {}, None

    @property
    def coff(self):
        return self.Sk - self.Sq                  # causal: key j is visible to row i iff j <= i + coff

    def oracle(self, causal, scale=None):
        """(o [B, Hq, Sq, D] float32 unrounded, lse [B, Hq, Sq]) of the fp64 reference; computed once"""
        key = (bool(causal), scale)
        if key not in self._ref:
            self._ref[key] = sdpa_ref(self.q, self.k, self.v, causal=causal, scale=scale, return_lse=True)
        return self._ref[key]

    def prescaled(self, causal, scale=None):
        """prescaled_reference of this problem; computed once"""
        key = ("prescaled", bool(causal), scale)
        if key not in self._ref:
            self._ref[key] = prescaled_reference(self, causal, scale)
        return self._ref[key]

    def sees(self, causal):
        """[B, Hkv, Sq] bool: row i of the slot sees its spike and is one of the rows aligned with u"""
        i = np.arange(self.Sq)
        s = self.spike[:, :, None]
        m = (s >= 0) & ((s <= i + self.coff) | (not causal))
        if self.hot is not None:
            m &= np.isin(i, self.hot)
        return m


def scores_log2(p, b, h, causal, scale=None):
    """[Sq, Sk] fp64 scores of query head h of batch b in log2 units, -inf where the causal mask hides the key"""
    sc = p.q[b, h].astype(np.float64) @ p.k[b, h // p.G].astype(np.float64).T
    sc *= (p.D ** -0.5 if scale is None else scale) * LOG2E
    if causal:
        sc = np.where(np.arange(p.Sk)[None, :] <= np.arange(p.Sq)[:, None] + p.coff, sc, -np.inf)
    return sc


def prescaled_reference(p, causal, scale=None):
    """What the prescaled flavours compute if everything after their one rounding were exact: Q * scale * log2(e) in
    fp32, rounded to `dtype`, then softmax in base 2 -- fp64 (o, lse)."""
    c2 = np.float32(p.D ** -0.5 if scale is None else scale) * np.float32(LOG2E)
    qs = round_to(p.q * c2, p.dtype)
    return sdpa_ref(qs, p.k, p.v, causal=causal, scale=float(np.log(2.0)), return_lse=True)


# ---------------------------------------------------------------------------------------------------------------------
# builders.  u is a +-1 sign vector per kv head, q = u + 0.25 N(0,1) for every query head of the group, V = N(0,1);
# K is what the kind is named for.
# ---------------------------------------------------------------------------------------------------------------------

def _rng(*key):
    return np.random.default_rng([int(k) + 1 for k in key])


def _grid(n):
    """(B, Hkv) with at least n slots: up to 7 kv heads, as many batches as it takes"""
    return (-(-n // 7), 7) if n >= 7 else (1, max(n, 1))


def _frame(rng, G, D, Sq, Sk):
    u = rng.choice([-1.0, 1.0], size=D)
    q = u + 0.25 * rng.standard_normal((G, Sq, D))
    return u, q, 0.25 * rng.standard_normal((Sk, D)), rng.standard_normal((Sk, D))


def _assemble(kind, dtype, D, G, Sq, Sk, slots, hot=None):
    """slots: (q [G, Sq, D], K [Sk, D], V [Sk, D], spike) per case; slot i of the (B, Hkv) grid holds case i % n"""
    B, Hkv = _grid(len(slots))
    q = np.zeros((B, Hkv * G, Sq, D), np.float32)
    k = np.zeros((B, Hkv, Sk, D), np.float32)
    v = np.zeros_like(k)
    spike = np.full((B, Hkv), -1)
    for i in range(B * Hkv):
        b, h = divmod(i, Hkv)
        q[b, h * G:(h + 1) * G], k[b, h], v[b, h], spike[b, h] = slots[i % len(slots)]
    return Problem(kind, dtype, D, G, Sq, Sk, q, k, v, spike, hot)


def softmax_stress(kind, dtype, D, G, Sq, Sk, spike_rows=SPIKE_ROWS):
    """The problems of section A: one batch per kind and shape, a case per (batch, kv head).  spike_rows: the key rows of
    the "spike" and "alone" cases (tests/prefill_window_cases.py adds rows next to the edges of its windows)."""
    slots = []
    if kind in ("spike", "alone"):
        # K[j*] = 4u among 0.25 N(0,1) keys; "alone": only the rows ALONE_ROWS are u (exactly), the others 0.25 N(0,1)
        for j in [j for j in spike_rows if j < Sk]:
            u, q, K, V = _frame(_rng(1, G, D, Sq, Sk, j), G, D, Sq, Sk)
            K[j] = 4.0 * u
            if kind == "alone":
                q -= u
                q[:, [r for r in ALONE_ROWS if r < Sq]] = u
            slots.append((q, K, V, j))
        return _assemble(kind, dtype, D, G, Sq, Sk, slots, hot=ALONE_ROWS if kind == "alone" else None)
    if kind in ("staircase64", "staircase32"):
        tile = int(kind[-2:])
        c = np.asarray(STAIR64[D] if tile == 64 else stair32(D))
        for i in range(2):
            u, q, K, V = _frame(_rng(2, G, D, Sq, Sk, tile, i), G, D, Sq, Sk)
            q = np.broadcast_to(u, q.shape)
            K = c[np.arange(Sk) // tile][:, None] * u[None]
            slots.append((q, K, V, -1))
    elif kind == "ramp":
        r = np.arange(Sk, dtype=np.float64)
        for i, asc in enumerate([True, False, True, False]):
            u, q, K, V = _frame(_rng(3, G, D, Sq, Sk, i), G, D, Sq, Sk)
            f = 4.0 * (r if asc else Sk - 1 - r) / max(Sk - 1, 1)
            slots.append((q, f[:, None] * u[None], V, -1))
    elif kind == "equal":
        for i in range(4):
            rng = _rng(4, G, D, Sq, Sk, i)
            u, q, K, V = _frame(rng, G, D, Sq, Sk)
            V[Sk - 1] = EQUAL_A * rng.choice([-1.0, 1.0], size=D)
            slots.append((q, np.broadcast_to(u, K.shape), V, -1))
    elif kind == "below":
        for i in range(4):
            u, q, K, V = _frame(_rng(5, G, D, Sq, Sk, i), G, D, Sq, Sk)
            slots.append((q, K - 4.0 * u, V, -1))
    else:
        raise ValueError(kind)
    return _assemble(kind, dtype, D, G, Sq, Sk, slots)


def normal_problem(dtype, D, G, Sq, Sk, B=2, Hkv=2):
    """N(0,1) everywhere (sections B and C)"""
    rng = _rng(6, G, D, Sq, Sk, B, Hkv)
    return Problem("normal", dtype, D, G, Sq, Sk, rng.standard_normal((B, Hkv * G, Sq, D)),
                   rng.standard_normal((B, Hkv, Sk, D)), rng.standard_normal((B, Hkv, Sk, D)))


def chained(dtype, shape):
    """Chained q-tiles of the persistent 4-wave kernels (more units than workgroup slots): K = ramp * u with the ramp of
    CHAIN_RAMP, q = s (u + 0.25 N(0,1)) with s = +1 / -1 by the parity of (256-row q-tile + query head), so that
    consecutive units of a workgroup, in either order of traversal, have row maxima of opposite sign."""
    B, Hq, Hkv, Sq, Sk = shape
    D, G = 128, Hq // Hkv
    rng = _rng(7, *shape)
    u = rng.choice([-1.0, 1.0], size=(B, Hkv, 1, D))
    sign = np.where((np.arange(Sq)[None, :] // 256 + np.arange(Hq)[:, None]) % 2 == 0, 1.0, -1.0)       # [Hq, Sq]
    q = sign[None, :, :, None] * (np.repeat(u, G, axis=1) + 0.25 * rng.standard_normal((B, Hq, Sq, D)).astype(np.float32))
    f = CHAIN_RAMP[0] + (CHAIN_RAMP[1] - CHAIN_RAMP[0]) * np.arange(Sk) / max(Sk - 1, 1)
    p = Problem("chained", dtype, D, G, Sq, Sk, q, f[None, None, :, None] * u, rng.standard_normal((B, Hkv, Sk, D)))
    p.sign = sign
    return p


# ---------------------------------------------------------------------------------------------------------------------
# the kernel coverage: (impl, head_dim, dtype, G).  fp16 and bf16 alternate over the list, so that each family (4-wave,
# 8-wave, 128-row) meets both; both head_dim 256 kernels are one-kernel families and run both types.  Every entry at
# group sizes 1 and 4.
# ---------------------------------------------------------------------------------------------------------------------

def _configs():
    impls = [(i, 128) for i in ("w4", "prescaled_w4", "rows256", "rows256x2", "rows128", "prescaled256", "prescaled128", "auto")]
    impls += [(i, 64) for i in ("rows256", "rows128", "prescaled128")]
    c = [(impl, D, ("fp16", "bf16")[n % 2]) for n, (impl, D) in enumerate(impls)]
    c += [(impl, 256, dt) for impl in ("auto", "d256_fallback") for dt in ("bf16", "fp16")]
    assert all(serves(impl, D) for impl, D, _ in c)
    return [(impl, D, dt, G) for impl, D, dt in c for G in (1, 4)]


CONFIGS = _configs()


def config_id(c):
    return "%s-D%d-%s-G%d" % c


def flavour(impl):
    return "prescaled" if impl.startswith("prescaled") else "exact"


def key_tile(impl, D):
    """rows of a key tile of the kernel a configuration runs ("auto" takes the 128-row kernel at these small grids)"""
    return 32 if D == 256 or impl.endswith("128") or impl == "auto" else 64


# Kinds the prescaled flavours run at the project tolerance: those whose prescaled_reference stays within a quarter of
# it (tests/test_prefill_numerics_cpu.py, test_prescaled_admission).  All of them do: worst case 0.15 of the tolerance,
# the staircases, where q = u exactly and every element of Q * scale * log2(e) rounds the same way.
PRESCALED_KINDS = list(KINDS)
PRESCALED_LEFT_OUT = []
# Section B by the same rule.  N(0,1) data at softmax_scale 0.03: 0.08 of the tolerance, admitted.  At 0.5 (logits of +-30)
# the fp64 result from the rounded Q is itself 0.95 to 2.3 tolerances away from the oracle (test_prescaled_admission_of_
# softmax_scale), so no kernel of the flavour can be held to the oracle there: the prescaled flavours still run 0.5, at the
# same tolerance, against prescaled_reference -- the fp64 result from the Q they round.
SCALES = (0.03, 0.5)
PRESCALED_SCALES = (0.03,)


def expected_kernel(impl, D):
    """what sfa.last_prefill_kernel() must say after a call of this configuration at the shapes of this suite: "auto" at
    head_dim 128 is the exact 128-row kernel there (fewer than 128 pair-workgroups, fewer than 256 q-tiles), which is
    what key_tile assumes"""
    if D == 256:
        return "prefill_d256_kernel" if impl == "d256_fallback" else "prefill_w4d_kernel<head_dim 256>"
    fl = flavour(impl)
    if impl.endswith("w4"):
        return f"prefill_w4_kernel<{fl}>"
    if impl.endswith("128") or impl == "auto":
        return f"prefill_kernel_bm128<{fl}>"
    return f"prefill_kernel<8 waves, 256 rows, {fl}>"


def stress_kinds(impl, D):
    """staircase64 for every kernel (on 32-row tiles it is a step every other tile), staircase32 for those whose tile is 32"""
    ks = [k for k in KINDS if k != "staircase32" or key_tile(impl, D) == 32]
    return [k for k in ks if flavour(impl) == "exact" or k in PRESCALED_KINDS]


# ---------------------------------------------------------------------------------------------------------------------
# the adapter (GPU)
# ---------------------------------------------------------------------------------------------------------------------

GUARD_Q, GUARD_K, PAD_D, LSE_TAIL = 256, 64, 8, 64
LSE_SENTINEL = 12345.0


def _tdt(dtype):
    import torch
    return {"fp16": torch.float16, "bf16": torch.bfloat16}[dtype]


def _bits_of(t):
    import torch
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def device_inputs(p):
    """contiguous device copies of q, k, v: made once per problem"""
    import torch
    if p._dev is None:
        dev = torch.device("cuda:0")
        p._dev = tuple(torch.from_numpy(x).to(_tdt(p.dtype)).to(dev) for x in (p.q, p.k, p.v))
    return p._dev


def guarded(t, guard, fill_bits, copy=True):
    """(allocation [B, H, guard + S + guard, D + 8] holding `fill_bits` everywhere, its view [:, :, guard : guard + S, :D]
    holding t, or `fill_bits` too with copy=False): a tile-sized over-read or over-write in either direction lands in the
    guard rows, one past the end of a row in the pad columns.  The row stride D + 8 keeps the 16-byte row alignment."""
    import torch
    B, H, S, D = t.shape
    base = torch.full((B, H, guard + S + guard, D + PAD_D), int(np.uint16(fill_bits).view(np.int16)), dtype=torch.int16,
                      device=t.device).view(t.dtype)
    view = base[:, :, guard:guard + S, :D]
    if copy:
        view.copy_(t)
    return base, view


def outside(base, guard, S, D):
    """uint16 bits of every element of a guarded allocation outside its view"""
    b = _bits_of(base)
    m = np.ones(b.shape, bool)
    m[:, :, guard:guard + S, :D] = False
    return b[m]


def call(sfa, q, k, v, o, lse, causal, scale=None, fast_scale=False, sizes=None):
    """sfa_prefill_fwd on torch views as they are: pointers and strides go into sfa_prefill_args unchanged (a stride of 0
    included).  lse: a float32 tensor (its data pointer is passed) or None.  sizes = (B, Hq, Hkv, Sq, Sk, D) overrides what
    the views say (empty problems).  Returns the status."""
    import torch
    from starflashattention_amd import _lib
    lib = _lib.load()
    a = _lib.PrefillArgs()
    a.q, a.k, a.v, a.o = q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr()
    a.lse = lse.data_ptr() if lse is not None else None
    B, Hq, Sq, D = q.shape
    Hkv, Sk = k.shape[1], k.shape[2]
    a.batch, a.heads_q, a.heads_kv, a.seqlen_q, a.seqlen_k, a.head_dim = sizes or (B, Hq, Hkv, Sq, Sk, D)
    for dst, t in ((a.q_stride, q), (a.k_stride, k), (a.v_stride, v), (a.o_stride, o)):
        dst[0], dst[1], dst[2] = t.stride(0), t.stride(1), t.stride(2)
    a.softmax_scale = float(scale) if scale else 0.0
    a.causal = 1 if causal else 0
    a.dtype = _lib.DTYPE_FP16 if q.dtype == torch.float16 else _lib.DTYPE_BF16
    a.fast_scale = 1 if fast_scale else 0
    with torch.cuda.device(q.device):
        return lib.sfa_prefill_fwd(ctypes.byref(a), ctypes.c_void_p(torch.cuda.current_stream(q.device).cuda_stream))


def run(sfa, p, causal, scale=None, fill_bits=None, kv=None):
    """One prefill call on problem p.  fill_bits None: contiguous tensors.  Else the guarded layout of section C with
    `fill_bits` in every element outside the views (O's own view holds it too before the call).  kv = (k, v): device views
    to pass instead of p's.  Returns dict(o = bits [B, Hq, Sq, D], lse [B, Hq, Sq], o_outside = bits outside O's view or None,
    lse_tail [LSE_TAIL])."""
    import torch
    q, k, v = device_inputs(p)
    if kv is not None:
        k, v = kv
    n = p.B * p.Hq * p.Sq
    lse = torch.full((n + LSE_TAIL,), LSE_SENTINEL, dtype=torch.float32, device=q.device)
    o_base = None
    if fill_bits is None:
        o = torch.full(q.shape, 7.0, dtype=q.dtype, device=q.device)
    else:
        _, q = guarded(q, GUARD_Q, fill_bits)
        _, k = guarded(k, GUARD_K, fill_bits)
        _, v = guarded(v, GUARD_K, fill_bits)
        o_base, o = guarded(q, GUARD_Q, fill_bits, copy=False)
    st = call(sfa, q, k, v, o, lse, causal, scale)
    assert st == 0, (st, sfa._lib.load().sfa_last_error())
    torch.cuda.synchronize()
    return dict(o=_bits_of(o), lse=lse[:n].cpu().numpy().reshape(p.B, p.Hq, p.Sq), lse_tail=lse[n:].cpu().numpy(),
                o_outside=None if o_base is None else outside(o_base, GUARD_Q, p.Sq, p.D))


def values(p, bits):
    return from_bits16(bits, p.dtype)


def v_bits(p):
    """[B, Hkv, Sk, D] storage bits of V"""
    return to_bits16(p.v, p.dtype)
