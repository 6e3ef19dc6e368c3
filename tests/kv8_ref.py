"""CPU reference of the fp8 (OCP e4m3) KV cache, shared by the sfa_decode_kv8 / sfa_kv8_quantize tests: the code table,
the quantiser of the header's contract, and one decode step in fp64 over the dequantised cache.

e4m3: 1 sign, 4 exponent (bias 7), 3 mantissa bits, no infinities, 0x7F / 0xFF = NaN, largest finite 448 (0x7E): torch's
float8_e4m3fn."""
import numpy as np

from oracle import rope_interleaved, round_to


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


def decode_kv8_ref(qkv, k8, v8, seq_len, idx_layer, rot_dim, dtype, k_scale=None, v_scale=None, q_bias=None,
                   k_bias=None, v_bias=None, cos_table=None, sin_table=None, scale=None):
    """One sfa_decode_kv8 step for the whole batch.

    qkv      [B, H + 2*Hkv, D] float (representable in `dtype`): q heads, k heads, v heads
    k8, v8   [B, L, M, Hkv, D] uint8, MUTATED at [b, idx_layer, seq_len[b]]
    k_scale, v_scale   [Hkv] float32 or None (= 1.0)
    returns dict(o = [B, H, D] float32 unrounded, k_row / v_row = the appended bytes [B, Hkv, D])

    k16 / v16 are what sfa_decode would store (bias, RoPE, rounded to `dtype`); the stored bytes are q8(x16 / scale);
    the attention runs in fp64 over scale * (the bytes of rows 0 .. pos), the new row included."""
    qkv = np.asarray(qkv)
    B, HH, D = qkv.shape
    Hkv = k8.shape[3]
    H = HH - 2 * Hkv
    G = H // Hkv
    M = k8.shape[2]
    if scale is None:
        scale = 1.0 / np.sqrt(float(D))
    ks = np.ones(Hkv, np.float32) if k_scale is None else np.asarray(k_scale, dtype=np.float32)
    vs = np.ones(Hkv, np.float32) if v_scale is None else np.asarray(v_scale, dtype=np.float32)
    o = np.zeros((B, H, D), dtype=np.float64)
    k_rows = np.zeros((B, Hkv, D), dtype=np.uint8)
    v_rows = np.zeros((B, Hkv, D), dtype=np.uint8)
    for b in range(B):
        pos = int(seq_len[b])
        if not (0 <= pos < M):
            raise ValueError(f"seq_len[{b}]={pos} outside [0, memory_max_len={M})")
        q = qkv[b, :H].astype(np.float64)
        k = qkv[b, H:H + Hkv].astype(np.float64)
        v = qkv[b, H + Hkv:].astype(np.float64)
        if q_bias is not None:
            q = q + np.asarray(q_bias, dtype=np.float64)
        if k_bias is not None:
            k = k + np.asarray(k_bias, dtype=np.float64)
        if v_bias is not None:
            v = v + np.asarray(v_bias, dtype=np.float64)
        c = s = None
        if cos_table is not None and rot_dim > 0:
            c, s = cos_table[pos], sin_table[pos]
        q16 = round_to(rope_interleaved(q, pos, rot_dim, cos=c, sin=s), dtype).astype(np.float64)
        k16 = round_to(rope_interleaved(k, pos, rot_dim, cos=c, sin=s), dtype)
        v16 = round_to(v, dtype)
        k8[b, idx_layer, pos] = k_rows[b] = quantize(k16, ks)
        v8[b, idx_layer, pos] = v_rows[b] = quantize(v16, vs)
        K = dequantize(k8[b, idx_layer, :pos + 1], ks)          # [T, Hkv, D]
        V = dequantize(v8[b, idx_layer, :pos + 1], vs)
        K, V = np.repeat(K, G, axis=1), np.repeat(V, G, axis=1)
        sc = np.einsum("hd,thd->ht", q16, K) * scale
        sc -= sc.max(axis=1, keepdims=True)
        p = np.exp(sc)
        p /= p.sum(axis=1, keepdims=True)
        o[b] = np.einsum("ht,thd->hd", p, V)
    return dict(o=o.astype(np.float32), k_row=k_rows, v_row=v_rows)
