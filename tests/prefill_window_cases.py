"""Structured problems for tests/test_prefill_window_numerics_{cpu,gpu}.py: the problems, tolerances and guarded layout of
tests/prefill_cases.py under a sliding window, with sinks of material weight, the fp64 reference of
tests/prefill_window_ref.py as the oracle, and one adapter that fills sfa_prefill_args itself.

Row i (causal limit lim_i = i + Sk - Sq) sees the keys [lo_i, lim_i], lo_i = max(0, lim_i + 1 - window).  The kernel walks
64-key tiles, masks per 32-key half and never stages a key below lo_0: WINDOWS holds one key, less than a half, one more
than a tile, and more than Sk = 100 (a window >= Sk runs only with sinks: without them the call is the causal kernels').
"""
import ctypes

import numpy as np

import prefill_cases as pc
from prefill_cases import (GUARD_K, GUARD_Q, LSE_SENTINEL, LSE_TAIL, ONE_ROW_SHAPES, SCALES, SHAPES, TOL, Problem,  # noqa: F401
                           _bits_of, guarded, normal_problem, outside, softmax_stress, v_bits, values)
from prefill_window_ref import prefill_window_ref
from sinks_ref import deltas, sigmoid

LSE_TOL = pc.LSE_TOL["exact"]                    # the windowed kernel is an exact-scale kernel
WINDOWS = (1, 40, 65, 150)
GUARD_WINDOWS = (40, 150)                        # sections B and C
KINDS_W = ["spike", "alone", "staircase64", "staircase64_down", "ramp", "equal", "below"]
# (head_dim, dtype, G); with and without sinks: the eight instances of prefill_window_kernel<Tr, D, SINK>
CONFIGS_W = [(128, "bf16", 1), (128, "fp16", 4), (64, "fp16", 1), (64, "bf16", 4)]
SINKS = (False, True)
EXACT_SHARE = 2.0 ** -25                         # a sink share that 1 - share loses in fp32: the row still returns V[spike]
MAX_LAUNCHES = 40                                # per parametrized GPU case


def config_id(c):
    return "D%d-%s-G%d" % c


def instance(cfg, sinks):
    """the template instance a (configuration, sinks) pair runs: (type, head_dim, SINK)"""
    return (cfg[1], cfg[0], bool(sinks))


def windows_for(Sk, sinks, windows=WINDOWS):
    """the windows a shape runs: all of them with sinks, those shorter than Sk without"""
    return [w for w in windows if w < Sk or sinks]


def lo_lim(p, window):
    """([Sq] lo_i, [Sq] lim_i); lim_i < 0: the row has no key"""
    lim = np.arange(p.Sq) + p.coff
    return np.maximum(0, lim + 1 - int(window)), lim


def lo0_of(Sq, Sk, window):
    """the lower bound of query row 0: no row sees a key below it"""
    return max(0, Sk - Sq + 1 - int(window))


# ---------------------------------------------------------------------------------------------------------------------
# problems
# ---------------------------------------------------------------------------------------------------------------------

def spike_rows_w(Sq, Sk):
    """prefill_cases.SPIKE_ROWS and, for the rows ALONE_ROWS (the only rows of "alone" that a spike dominates): the key on
    each one's diagonal (all a window of 1 shows it), for every window below Sk the key one below the lower bound of the
    first such row that has one, and the key one above the limit of the first that has one."""
    coff = Sk - Sq
    hot = [r for r in pc.ALONE_ROWS if r < Sq]
    rows = {j for j in pc.SPIKE_ROWS if j < Sk} | {r + coff for r in hot if 0 <= r + coff < Sk}
    for w in WINDOWS:
        if w < Sk:
            rows.add(next(r + coff - w for r in hot if 0 <= r + coff - w < Sk))
    rows.add(next(r + coff + 1 for r in hot if 0 <= r + coff + 1 < Sk))
    return sorted(rows)


def stress_w(kind, dtype, D, G, Sq, Sk):
    """prefill_cases.softmax_stress for the kinds of KINDS_W, with the spike rows of spike_rows_w.  The staircases are
    built here, on four slots where softmax_stress has two (the first two of "staircase64" are its): where every row of a
    step has the same lse, the sinks of two heads -- deltas(2) = -3, +3, shares 0.047 and 0.953 -- are material in no row,
    four heads have -1 and +1 as well.  "staircase64_down" is "staircase64" with the steps reversed over the key tiles,
    K = c[::-1][tile] u: as the window slides every row's max falls, and the keys just below a lower bound on a tile edge
    are 7 to 9 log2 units above everything the row sees."""
    if kind in ("spike", "alone"):
        return softmax_stress(kind, dtype, D, G, Sq, Sk, spike_rows=spike_rows_w(Sq, Sk))
    if kind not in ("staircase64", "staircase64_down"):
        return softmax_stress(kind, dtype, D, G, Sq, Sk)
    down = kind.endswith("down")
    c = np.asarray(pc.STAIR64[D])[::-1 if down else 1]
    slots = []
    for i in range(4):
        u, q, K, V = pc._frame(pc._rng(*((8, G, D, Sq, Sk, i) if down else (2, G, D, Sq, Sk, 64, i))), G, D, Sq, Sk)
        slots.append((np.broadcast_to(u, q.shape), c[np.arange(Sk) // 64][:, None] * u[None], V, -1))
    return pc._assemble(kind, dtype, D, G, Sq, Sk, slots)


def sees_w(p, window):
    """[B, Hkv, Sq] bool: the window [lo_i, lim_i] of row i holds the slot's spike, and the row is one of the rows aligned
    with u where the problem has such rows"""
    lo, lim = lo_lim(p, window)
    s = p.spike[:, :, None]
    m = (s >= 0) & (lo <= s) & (s <= lim)
    if p.hot is not None:
        m &= np.isin(np.arange(p.Sq), p.hot)
    return m


def oracle_w(p, window, sinks=None, scale=None):
    """(o [B, Hq, Sq, D] float32 unrounded, lse [B, Hq, Sq]) of prefill_window_ref on the problem's arrays; sinks: None or
    the float32 array the device gets.  Computed once per (window, sinks, scale) and kept in the problem."""
    key = ("window", int(window), None if sinks is None else np.asarray(sinks, np.float32).tobytes(), scale)
    if key not in p._ref:
        s64 = None if sinks is None else np.asarray(sinks, np.float32).astype(np.float64)
        p._ref[key] = prefill_window_ref(p.q, p.k, p.v, window, sinks=s64, scale=scale)
    return p._ref[key]


def sinks_for(p, window):
    """[Hq] float32, sinks[h] = a_h + deltas(Hq)[h]: a_h is the no-sink reference lse of an actual row, the one of rank
    n // 2 among the n sorted finite lse of batch 0, head h -- so the sink takes sigmoid(delta_h) of that row's softmax.
    (Not np.median: for even n it averages two rows, and between two steps of a staircase lies no row at all.)"""
    _, lse = oracle_w(p, window)
    a = np.empty(p.Hq)
    for h in range(p.Hq):
        fin = np.sort(lse[0, h][np.isfinite(lse[0, h])].astype(np.float64))
        a[h] = fin[fin.size // 2]
    return (a + deltas(p.Hq)).astype(np.float32)


def sink_share(p, window, sinks):
    """[B, Hq, Sq] the sink's share of each row's softmax, sigmoid(sinks[h] - lse without the sink); nan: no key"""
    _, lse = oracle_w(p, window)
    with np.errstate(over="ignore", invalid="ignore"):
        sh = sigmoid(np.asarray(sinks, np.float64)[None, :, None] - lse.astype(np.float64))
    return np.where(np.isfinite(lse), sh, np.nan)


def exact_rows_w(p, window, sinks=None):
    """[B, Hq, Sq] bool: the rows that must return the storage bits of V[spike]: those of sees_w, and with sinks only
    where the sink's share is at most EXACT_SHARE (elsewhere the sink is material and the row is the reference's)"""
    m = np.repeat(sees_w(p, window), p.G, axis=1)
    if sinks is not None:
        with np.errstate(invalid="ignore"):
            m &= sink_share(p, window, sinks) <= EXACT_SHARE
    return m


# ---------------------------------------------------------------------------------------------------------------------
# the tables of the GPU file: what each parametrized case launches
# ---------------------------------------------------------------------------------------------------------------------

STRIDE0_SHAPES = [(299, 299), (100, 299)]
SCALE_SHAPE = (299, 299)
FILLS = ("zeros", "nan", "inf")
EMPTY = ("Sk=0", "batch=0", "Sq=0")
MARKER_CALLS = 1                                 # the one-row full-attention call in front of a block of windowed calls


def stress_runs(sinks):
    return [(s, w) for s in SHAPES for w in windows_for(s[1], sinks)]


def guard_runs(sinks):
    return [(s, w) for s in SHAPES + ONE_ROW_SHAPES for w in windows_for(s[1], sinks, GUARD_WINDOWS)]


def launches(section, sinks):
    """kernel launches of one parametrized case of the GPU file"""
    if section == "A":
        return MARKER_CALLS + len(stress_runs(sinks))
    if section == "B":
        return MARKER_CALLS + len(GUARD_WINDOWS) * (1 + len(SCALES))
    if section == "guarded":
        return MARKER_CALLS + len(guard_runs(sinks)) * len(FILLS)
    if section == "stride0":                     # (batch, head) x (expanded, contiguous) per window, and the reference run
        return MARKER_CALLS + len(STRIDE0_SHAPES) * (len(GUARD_WINDOWS) * 2 * 2 + 1)
    if section == "empty":
        return MARKER_CALLS + len(EMPTY)
    raise ValueError(section)


# ---------------------------------------------------------------------------------------------------------------------
# the adapter (GPU)
# ---------------------------------------------------------------------------------------------------------------------

def call_window(sfa, q, k, v, o, lse, window, sinks=None, scale=None, sizes=None):
    """sfa_prefill_window_fwd on torch views as they are: pointers and strides go into sfa_prefill_args unchanged (a
    stride of 0 included).  lse: a float32 tensor (its data pointer is passed) or None; sinks: a float32 device tensor
    (its data pointer is passed) or None; sizes = (B, Hq, Hkv, Sq, Sk, D) overrides what the views say.  Returns the
    status."""
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
    a.causal = 1
    a.dtype = _lib.DTYPE_FP16 if q.dtype == torch.float16 else _lib.DTYPE_BF16
    a.fast_scale = 0
    sp = None
    if sinks is not None:
        assert sinks.dtype == torch.float32 and sinks.is_contiguous() and sinks.numel() == a.heads_q
        sp = ctypes.c_void_p(sinks.data_ptr())
    with torch.cuda.device(q.device):
        return lib.sfa_prefill_window_fwd(ctypes.byref(a), int(window), sp,
                                          ctypes.c_void_p(torch.cuda.current_stream(q.device).cuda_stream))


def run_window(sfa, p, window, sinks=None, scale=None, fill_bits=None, kv=None):
    """One windowed call on problem p; sinks: None or [Hq] float32 (numpy).  fill_bits None: contiguous tensors.  Else
    the guarded layout of prefill_cases.run, and in addition the rows [0, lo_0) inside the K and V views hold the fill:
    no row sees them.  kv = (k, v): device views to pass instead of p's.  Returns prefill_cases.run's dict."""
    import torch
    q, k, v = pc.device_inputs(p)
    if kv is not None:
        k, v = kv
    n = p.B * p.Hq * p.Sq
    lse = torch.full((n + LSE_TAIL,), LSE_SENTINEL, dtype=torch.float32, device=q.device)
    ts = None if sinks is None else torch.from_numpy(np.array(sinks, np.float32)).to(q.device)
    o_base = None
    if fill_bits is None:
        o = torch.full(q.shape, 7.0, dtype=q.dtype, device=q.device)
    else:
        _, q = guarded(q, GUARD_Q, fill_bits)
        _, k = guarded(k, GUARD_K, fill_bits)
        _, v = guarded(v, GUARD_K, fill_bits)
        lo0 = lo0_of(p.Sq, p.Sk, window)
        fill = int(np.uint16(fill_bits).view(np.int16))
        k.view(torch.int16)[:, :, :lo0] = fill
        v.view(torch.int16)[:, :, :lo0] = fill
        o_base, o = guarded(q, GUARD_Q, fill_bits, copy=False)
    st = call_window(sfa, q, k, v, o, lse, window, ts, scale)
    assert st == 0, (st, sfa._lib.load().sfa_last_error())
    torch.cuda.synchronize()
    return dict(o=_bits_of(o), lse=lse[:n].cpu().numpy().reshape(p.B, p.Hq, p.Sq), lse_tail=lse[n:].cpu().numpy(),
                o_outside=None if o_base is None else outside(o_base, GUARD_Q, p.Sq, p.D))
