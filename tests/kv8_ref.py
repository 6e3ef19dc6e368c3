"""CPU reference of the fp8 (OCP e4m3) KV cache, shared by the sfa_decode_kv8 / sfa_kv8_quantize tests: the code table, the
quantiser of the header's contract, and one decode step over the dequantised cache, an adapter over tests/serving_model.py
(which quantises and dequantises with the two functions here).

e4m3: 1 sign, 4 exponent (bias 7), 3 mantissa bits, no infinities, 0x7F / 0xFF = NaN, largest finite 448 (0x7E): torch's
float8_e4m3fn."""
import numpy as np

import serving_model as sm          # (imports this module for quantize / dequantize)


def _table():
    t = np.zeros(256, dtype=np.float64)
    for code in range(256):
        e, m = (code >> 3) & 15, code & 7
        if e == 15 and m == 7:
            v = np.nan
        elif e == 0:
            v = m / 8.0 * 2.0 ** -6
        else:
            v = (1.0 + m / 8.0) * 2.0 ** (e - 7)
        t[code] = -v if code & 0x80 else v
    return t


E4M3 = _table()                     # code -> value (float64; NaN at 0x7F and 0xFF)
_POS = E4M3[:0x7F]                  # the 127 non-negative finite values, ascending: index = code
E4M3_MAX = 448.0


def dequantize(codes, scale=None):
    """uint8 codes [..., H, D] -> float64 values, times scale[h] when given."""
    x = E4M3[np.asarray(codes, dtype=np.uint8)]
    if scale is not None:
        x = x * np.asarray(scale, dtype=np.float32).astype(np.float64)[:, None]
    return x


def quantize(x, scale=None):
    """q8(x / scale[h]) for x [..., H, D]: the division in fp32, clamped to +-448, rounded to the nearest code with ties
    to the even one, NaN -> 0x7F.  Returns uint8."""
    x = np.asarray(x, dtype=np.float32)
    if scale is not None:
        with np.errstate(over="ignore", invalid="ignore"):
            x = (x / np.asarray(scale, dtype=np.float32)[:, None]).astype(np.float32)
    nan = np.isnan(x)
    neg = np.signbit(x)
    a = np.clip(np.abs(np.where(nan, np.float32(0), x)).astype(np.float64), 0.0, E4M3_MAX)
    hi = np.clip(np.searchsorted(_POS, a, side="left"), 0, 0x7E)       # first code with value >= a
    lo = np.maximum(hi - 1, 0)
    dlo, dhi = a - _POS[lo], _POS[hi] - a                               # exact: fp32 inputs, dyadic table
    code = np.where(dlo < dhi, lo, np.where(dhi < dlo, hi, np.where(lo % 2 == 0, lo, hi)))
    code = (code | np.where(neg, 0x80, 0)).astype(np.uint8)
    return np.where(nan, np.uint8(0x7F), code).astype(np.uint8)


def step_at(v):
    """The distance between neighbouring e4m3 values around |v| (the larger one at a binade boundary)."""
    a = np.maximum(np.abs(np.asarray(v, dtype=np.float64)), 2.0 ** -6)
    return 2.0 ** (np.floor(np.log2(a)) - 3)


def decode_kv8_model(qkv, k8, v8, seq_len, idx_layer, rot_dim, dtype, window, sinks, k_scale, v_scale, q_bias, k_bias, v_bias,
                     cos_table, sin_table, scale):
    """The single-token call over an fp8 cache through the model, for decode_kv8_ref, kv8_window_ref.decode_kv8_window_ref
    and kv8_sinks_ref.decode_kv8_sinks_ref.  k8 / v8 are MUTATED.  Returns dict(o, k_row, v_row, o64, lse, q16)."""
    qkv = np.asarray(qkv)
    M = k8.shape[2]
    for b, pos in enumerate(seq_len):
        if not (0 <= int(pos) < M):
            raise ValueError(f"seq_len[{b}]={int(pos)} outside [0, memory_max_len={M})")
    call = sm.make_call(dtype, qkv.shape[1] - 2 * k8.shape[3], seq_len, [1] * len(qkv), [x[None] for x in qkv], idx_layer, rot_dim,
                        q_bias=q_bias, k_bias=k_bias, v_bias=v_bias, cos=cos_table, sin=sin_table, window=window, sinks=sinks,
                        k_scale=k_scale, v_scale=v_scale, softmax_scale=scale)
    app, res = sm.run((k8, v8), call, in_place=True)
    first = lambda xs: np.stack([x[0] for x in xs])
    o = first(r[0] for r in res)
    return dict(o=o.astype(np.float32), k_row=first(app["k_bits"]), v_row=first(app["v_bits"]), o64=o,
                lse=first(r[1] for r in res), q16=first(app["q16"]))


def decode_kv8_ref(qkv, k8, v8, seq_len, idx_layer, rot_dim, dtype, k_scale=None, v_scale=None, q_bias=None,
                   k_bias=None, v_bias=None, cos_table=None, sin_table=None, scale=None):
    """One sfa_decode_kv8 step for the whole batch.

    qkv      [B, H + 2*Hkv, D] float (representable in `dtype`): q heads, k heads, v heads
    k8, v8   [B, L, M, Hkv, D] uint8, MUTATED at [b, idx_layer, seq_len[b]]
    k_scale, v_scale   [Hkv] float32 or None (= 1.0)
    returns dict(o = [B, H, D] float32 unrounded, k_row / v_row = the appended bytes [B, Hkv, D])

    k16 / v16 are what sfa_decode would store (bias, RoPE, rounded to `dtype`); the stored bytes are q8(x16 / scale);
    the attention runs in fp64 over scale * (the bytes of rows 0 .. pos), the new row included."""
    ref = decode_kv8_model(qkv, k8, v8, seq_len, idx_layer, rot_dim, dtype, None, None, k_scale, v_scale, q_bias, k_bias, v_bias,
                           cos_table, sin_table, scale)
    return {key: ref[key] for key in ("o", "k_row", "v_row")}
