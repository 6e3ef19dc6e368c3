"""The fp64 definition of one decode call, of any of the 18 flavours: the only place in tests/ where the prologue (bias,
rotation, rounding, quantisation) and the attention (the softmax over the window, the sink) of a decode call are written
down.  It is built from the oracle's primitives (oracle.rope_interleaved, oracle.rotary_table_ref, oracle.round_to,
kv8_ref.quantize / dequantize, window_ref.window_lo).  The reference functions of window_ref.py, sinks_ref.py, kv8_ref.py,
kv8_window_ref.py, kv8_sinks_ref.py, chunk_kv8_ref.py, chunk_kv8_window_ref.py and chunk_window_ref.py are adapters over it:
each builds a call and a cache from its own arguments, runs step(), and hands the result back in its own shape.  What those
functions returned while they had arithmetic of their own is recorded in tests/golden/decode_ref_anchors.npz, and
tests/test_serving_model_cpu.py holds the adapters against it and the model against oracle.decode_ref.  The one other
formulation is chunk_kv8_window_ref.attend_dense (one masked softmax per sequence), kept apart on purpose.

The cache is canonical, [B, L, M, Hkv, D], and kept as STORAGE BITS (uint16 for fp16 / bf16 caches, uint8 for e4m3 caches,
as in tests/decode_cases.py), so that "this byte did not change" and "the model continues from the device's bits" are plain
array operations.  Nothing here knows a layout, a page size or a kv-head count in advance.

A call is a dict:

  dtype         "fp16" / "bf16": the type of qkv, the biases, the tables, o and a 16-bit cache
  H             query heads (the kv-head count follows from the token width H + 2 Hkv)
  pos, n        [B] ints: rows already cached, new tokens (single-token: 1 each; chunk: one common n; varlen: any, 0 too)
  tokens        per sequence a float array [n_b, H + 2 Hkv, D] (q heads, k heads, v heads), representable in dtype
  q_bias, k_bias, v_bias   [H, D] / [Hkv, D] / [Hkv, D] or None
  rot, cos, sin rotary_embedding_dim; the tables [M, rot / 2] (oracle.rotary_table_ref) or None = trigonometry on the fly
  layer         idx_layer
  window        an int >= 1 or None
  sinks         [H] floats (finite or -inf) or None
  k_scale, v_scale   [Hkv] float32 or None; over an fp8 cache None means 1.0
  softmax_scale a float or None = 1 / sqrt(D)

Token t of sequence b sees the rows [max(0, pos + t + 1 - window), pos + t] of the cache AFTER the append.  An attention
sink is one more key of every softmax of query head h, with logit sinks[h] (natural-log units, multiplied neither by the
softmax scale nor by k_scale) and a zero value row: it adds exp(sinks[h]) to the denominator and nothing to the numerator.
"""
import numpy as np

import kv8_ref
import window_ref                   # (both import this module: their names are looked up when a call is made)
from oracle import from_bits16, rope_interleaved, rotary_table_ref, round_to, to_bits16  # noqa: F401

CALL_KEYS = ("dtype", "H", "pos", "n", "tokens", "q_bias", "k_bias", "v_bias", "rot", "cos", "sin", "layer", "window", "sinks",
             "k_scale", "v_scale", "softmax_scale")


def make_call(dtype, H, pos, n, tokens, layer, rot=0, **kw):
    """a call dict with every optional key present (None unless given)"""
    call = dict.fromkeys(CALL_KEYS)
    call.update(dtype=dtype, H=int(H), pos=[int(x) for x in pos], n=[int(x) for x in n], tokens=tokens, layer=int(layer), rot=int(rot))
    assert set(kw) <= set(CALL_KEYS), sorted(set(kw) - set(CALL_KEYS))
    call.update(kw)
    return call


def is_kv8(cache_bits):
    return cache_bits.dtype == np.uint8


def values(bits, dtype, scale=None):
    """float64 values of cache bits [..., Hkv, D]: e4m3 codes times scale[h], or 16-bit storage"""
    if is_kv8(bits):
        return kv8_ref.dequantize(bits, scale)
    return from_bits16(bits, dtype).astype(np.float64)


def store(x16, dtype, kv8, scale=None):
    """the storage bits of rows x16 [..., Hkv, D] (float32, already rounded to dtype): q8(x / scale[h]) or the 16 bits"""
    return kv8_ref.quantize(x16, scale) if kv8 else to_bits16(x16, dtype)


def prologue(call, b):
    """(q16 [n, H, D] float64 = the rotated queries rounded to dtype, k16, v16 [n, Hkv, D] float32 = the rows rounded to
    dtype, before any quantisation) of sequence b: bias, rotation at pos + t, rounding -- what every entry point does
    before the attention"""
    x = np.array(call["tokens"][b], dtype=np.float64)           # (a copy: the biases are added in place)
    n, pos, rot, H = call["n"][b], call["pos"][b], call["rot"], call["H"]
    Hkv = (x.shape[1] - H) // 2
    assert x.shape[0] == n and x.shape[1] == H + 2 * Hkv
    q, k, v = x[:, :H], x[:, H:H + Hkv], x[:, H + Hkv:]
    for name, part in (("q_bias", q), ("k_bias", k), ("v_bias", v)):
        if call[name] is not None:
            part += np.asarray(call[name], np.float64)
    qr, kr = np.empty_like(q), np.empty_like(k)
    for t in range(n):
        c = s = None
        if call["cos"] is not None and rot > 0:
            c, s = call["cos"][pos + t], call["sin"][pos + t]
        qr[t] = rope_interleaved(q[t], pos + t, rot, cos=c, sin=s)
        kr[t] = rope_interleaved(k[t], pos + t, rot, cos=c, sin=s)
    dt = call["dtype"]
    return round_to(qr, dt).astype(np.float64), round_to(kr, dt), round_to(v, dt)


def attend_rows(q16, kbits, vbits, pos, call, with_lse=False):
    """q16 [n, H, D] float64; kbits / vbits [M, Hkv, D] one (sequence, layer) of the cache after the append.  Returns
    o [n, H, D] float64; with_lse: (o, lse [n, H] float64 = log sum_j exp(s_j) over the token's rows, WITHOUT the sink,
    from which the sink tests build sinks of a known weight)."""
    n, H, D = q16.shape
    Hkv = kbits.shape[1]
    G = H // Hkv
    assert G * Hkv == H
    scale = 1.0 / np.sqrt(float(D)) if call["softmax_scale"] is None else call["softmax_scale"]
    ks = vs = None
    if is_kv8(kbits):
        ks = np.ones(Hkv, np.float32) if call["k_scale"] is None else np.asarray(call["k_scale"], np.float32)
        vs = np.ones(Hkv, np.float32) if call["v_scale"] is None else np.asarray(call["v_scale"], np.float32)
    sk = (np.full(H, -np.inf) if call["sinks"] is None else np.asarray(call["sinks"], np.float64))[:, None]
    lo0 = window_ref.window_lo(pos, call["window"])             # the values of the rows any token sees, once
    K0 = np.repeat(values(kbits[lo0:pos + n], call["dtype"], ks), G, axis=1)
    V0 = np.repeat(values(vbits[lo0:pos + n], call["dtype"], vs), G, axis=1)
    o = np.zeros((n, H, D), np.float64)
    lse = np.zeros((n, H), np.float64)
    for t in range(n):
        rows = slice(window_ref.window_lo(pos + t, call["window"]) - lo0, pos + t + 1 - lo0)
        sc = np.einsum("hd,thd->ht", q16[t], K0[rows]) * scale
        m0 = sc.max(axis=1, keepdims=True)
        if with_lse:
            lse[t] = (m0 + np.log(np.exp(sc - m0).sum(axis=1, keepdims=True)))[:, 0]
        sc -= np.maximum(m0, sk)
        p = np.exp(sc)
        p /= p.sum(axis=1, keepdims=True) + np.exp(sk - np.maximum(m0, sk))
        o[t] = np.einsum("ht,thd->hd", p, V0[rows])
    return (o, lse) if with_lse else o


def step(cache, call):
    """cache = (kc, vc), canonical storage bits [B, L, M, Hkv, D]; they are not modified (only their type and shape are
    looked at here).  Returns (appended, attend):

      appended   dict(k16, v16 = per sequence [n_b, Hkv, D] float32, the rows rounded to dtype; k_bits, v_bits = per
                 sequence their storage bits: what the call must write at rows pos .. pos + n_b - 1 of idx_layer; q16 =
                 per sequence [n_b, H, D] float64, the rotated queries rounded to dtype)
      attend     attend(kc_after, vc_after) -> per sequence o [n_b, H, D] float64, every token over the given bits;
                 with_lse=True: per sequence (o, lse [n_b, H]), see attend_rows

    apply(cache, call, appended) gives the model's own cache after the call."""
    kc, vc = cache
    B, L, M = kc.shape[:3]
    assert kc.shape == vc.shape and kc.dtype == vc.dtype and len(call["pos"]) == len(call["n"]) == B
    assert 0 <= call["layer"] < L
    kv8 = is_kv8(kc)
    out = dict(q16=[], k16=[], v16=[], k_bits=[], v_bits=[])
    for b in range(B):
        assert 0 <= call["pos"][b] and call["pos"][b] + call["n"][b] <= M, (b, call["pos"][b], call["n"][b], M)
        q16, k16, v16 = prologue(call, b)
        out["q16"].append(q16)
        out["k16"].append(k16)
        out["v16"].append(v16)
        out["k_bits"].append(store(k16, call["dtype"], kv8, call["k_scale"]))
        out["v_bits"].append(store(v16, call["dtype"], kv8, call["v_scale"]))

    def attend(kc_after, vc_after, with_lse=False):
        return [attend_rows(out["q16"][b], kc_after[b, call["layer"]], vc_after[b, call["layer"]], call["pos"][b], call, with_lse)
                for b in range(B)]

    return out, attend


def write(cache, call, appended):
    """the appended bits at their rows of the caches, in place"""
    for b, (pos, n) in enumerate(zip(call["pos"], call["n"])):
        cache[0][b, call["layer"], pos:pos + n] = appended["k_bits"][b]
        cache[1][b, call["layer"], pos:pos + n] = appended["v_bits"][b]


def apply(cache, call, appended):
    """copies of the caches with the appended bits at their rows"""
    after = cache[0].copy(), cache[1].copy()
    write(after, call, appended)
    return after


def run(cache, call, in_place=False):
    """The whole call, as the reference functions hand it on: (appended, per sequence (o, lse) over the cache after the
    append).  in_place: the caches themselves get the appended bits, as the fp8 references document it."""
    appended, attend = step(cache, call)
    if in_place:
        write(cache, call, appended)
    return appended, attend(*(cache if in_place else apply(cache, call, appended)), with_lse=True)


def append_mask(shape, call):
    """[B, L, M] bool, True on the rows the call appends"""
    m = np.zeros(shape[:3], bool)
    for b, (pos, n) in enumerate(zip(call["pos"], call["n"])):
        m[b, call["layer"], pos:pos + n] = True
    return m
