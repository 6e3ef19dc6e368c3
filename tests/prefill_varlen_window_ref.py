"""The reference of sfa_prefill_varlen_window_fwd (packed sequences of different lengths under a sliding window, with
attention sinks), the batches of its tests and their sinks, for tests/test_prefill_varlen_window_{cpu,gpu}.py.

prefill_varlen_window_ref loops over the valid sequences and calls tests/prefill_window_ref.py on each one's own rows --
the call's contract verbatim: sequence b gets what sfa_prefill_window_fwd gives for batch = 1, seqlen_q = n_q,
seqlen_k = n_k on its rows.  Empty sequences, rows without keys and `rows` follow tests/prefill_varlen_ref.py.
"""
import functools

import numpy as np

from oracle import round_to
from prefill_varlen_ref import cu_of, valid_sequences
from prefill_window_ref import prefill_window_ref
from sinks_ref import sigmoid

INT_MAX = 2 ** 31 - 1

# name -> (the (n_q, n_k) of each sequence, Hq, Hkv): the smallest batches that reach each edge
BATCHES = {
    # an empty sequence inside; a one-row second q-tile; a marker slot (6 items in 7 slots)
    "P": ([(300, 300), (0, 0), (1, 1), (257, 257), (64, 64)], 4, 2),
    # lo_0 = 773 at window 128 (12 whole tiles and 5 rows never read); 233 rows without a key; a sequence without keys
    "Q": ([(100, 1000), (333, 100), (5, 0), (256, 256)], 4, 2),
    # three q-tiles with different ts0 and leading idle steps; a chunk against a long prefix (lo_0 = 705 at window 1,
    # 641 = 10 * 64 + 1 at window 65); the slices = 8 block map
    "R": ([(600, 700), (64, 769), (1, 128)], 8, 1),
    # key lengths 1, 63, 1, 0 mod 64 side by side; first tile = ragged tile for (64, 65) at windows <= 1
    "S": ([(300, 321), (100, 383), (64, 65), (1, 128)], 4, 1),
}
WINDOWS = (1, 40, 64, 65, 128, 150, 300)        # one key, less than a half tile, the tile edge and one beyond, more than
#                                                 most n_k
DELTA_LO, DELTA_HI = -3.0, 3.0                  # the sinks' offsets from the anchor row's lse, spread over the heads
SHARE_LO, SHARE_HI, SHARE_ROWS = 0.05, 0.95, 0.2


def lo0(n_q, n_k, window):
    """the lower bound of a sequence's query row 0: no row of the sequence sees a key below it"""
    return max(0, n_k - n_q + 1 - int(window))


def prefill_varlen_window_ref(q, k, v, cu_q, cu_k, window, sinks=None, scale=None):
    """q [Tq, Hq, D], k / v [Tk, Hkv, D] numpy, cu_q / cu_k integer sequences [B + 1], window int >= 1, sinks None or
    [Hq].  Returns (o [Tq, Hq, D] float32, lse [Hq, Tq] float32, rows [Tq] bool: the packed query rows that belong to a
    valid sequence).  Rows of no valid sequence hold 0 in o and lse; a row with no visible key holds 0 and -inf."""
    Tq, Hq, D = q.shape
    Tk = k.shape[0]
    o = np.zeros((Tq, Hq, D), np.float32)
    lse = np.zeros((Hq, Tq), np.float32)
    rows = np.zeros(Tq, bool)
    for b, q0, q1, k0, k1 in valid_sequences(cu_q, cu_k, Tq, Tk):
        if q1 == q0:
            continue
        rows[q0:q1] = True
        if k1 == k0:
            lse[:, q0:q1] = -np.inf
            continue
        ob, lb = prefill_window_ref(q[q0:q1].transpose(1, 0, 2)[None], k[k0:k1].transpose(1, 0, 2)[None],
                                    v[k0:k1].transpose(1, 0, 2)[None], window, sinks=sinks, scale=scale)
        o[q0:q1] = ob[0].transpose(1, 0, 2)
        lse[:, q0:q1] = lb[0]
    return o, lse, rows


def batch_cu(name):
    lens = BATCHES[name][0]
    return tuple(cu_of([a for a, _ in lens])), tuple(cu_of([b for _, b in lens]))


@functools.lru_cache(maxsize=None)
def inputs(name, dtype, D, pad=0):
    """(q [Tq + pad, Hq, D], k, v [Tk + pad, Hkv, D]) N(0, 1) rounded to dtype: once per key, shared, read-only"""
    _, Hq, Hkv = BATCHES[name]
    cu_q, cu_k = batch_cu(name)
    rng = np.random.default_rng([ord(name), D, pad, 22])
    out = tuple(round_to(rng.standard_normal((n + pad, H, D)), dtype)
                for n, H in ((cu_q[-1], Hq), (cu_k[-1], Hkv), (cu_k[-1], Hkv)))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference(name, dtype, D, window, with_sinks, scale=None, pad=0):
    """(o, lse, rows, sinks) of prefill_varlen_window_ref on inputs(name, dtype, D, pad), sinks = sinks_of(...) as the
    float32 array the device gets, or None: once per key, shared, read-only"""
    q, k, v = inputs(name, dtype, D, pad)
    cu_q, cu_k = batch_cu(name)
    sinks = sinks_of(name, dtype, D, window, scale, pad) if with_sinks else None
    s64 = None if sinks is None else sinks.astype(np.float64)
    o, lse, rows = prefill_varlen_window_ref(q, k, v, cu_q, cu_k, window, sinks=s64, scale=scale)
    for a in (o, lse, rows):
        a.setflags(write=False)
    return o, lse, rows, sinks


def anchor_sinks(lse, rows):
    """[Hq] float32 sinks a_h + delta_h from a no-sink lse [Hq, Tq]: a_h is the lse of the row of median lse (rank n // 2
    of the n sorted, an actual row) among the batch's rows with a key, delta spread over [-3, 3] across the heads"""
    Hq = lse.shape[0]
    a = np.empty(Hq)
    for h in range(Hq):
        fin = np.sort(lse[h][np.isfinite(lse[h]) & rows].astype(np.float64))
        a[h] = fin[fin.size // 2]
    out = (a + np.linspace(DELTA_LO, DELTA_HI, Hq)).astype(np.float32)
    out.setflags(write=False)
    return out


def sinks_of(name, dtype, D, window, scale=None, pad=0):
    _, lse, rows, _ = reference(name, dtype, D, window, False, scale, pad)
    return anchor_sinks(lse, rows)


def sink_share(lse_nosink, sinks):
    """[Hq, Tq] the sink's share of each row's softmax, sigmoid(sinks[h] - lse without the sink); nan: no key"""
    with np.errstate(over="ignore", invalid="ignore"):
        sh = sigmoid(np.asarray(sinks, np.float64)[:, None] - lse_nosink.astype(np.float64))
    return np.where(np.isfinite(lse_nosink), sh, np.nan)
