"""Plain fp64 reference of sfa_decode_mla (include/star_flash_attn.h) for tests/test_decode_mla_gpu.py.  No fused
arithmetic: RoPE in fp64 on the 16-bit inputs, rounded to the storage dtype; softmax and the value product in fp64 over
the stored, rounded rows.  The rows above pos are never looked at, so they may hold NaN."""
import numpy as np

from oracle import round_to
from oracle.decode_ref import rope_interleaved

D, DV, ROT = 576, 512, 64


def mla_decode_ref(q, kv_new, cache, seq_len, dtype, scale=None, cos_table=None, sin_table=None):
    """q [B, H, 576], kv_new [B, 576], cache [B, M, 576] = the rows of layer idx_layer in sequence order (floats
    representable in `dtype`; not modified), tables [M, 32] or None.  Returns (o [B, H, 512] float64 unrounded,
    row [B, 576] float32 = what the call stores at cache row seq_len[b])."""
    q = np.asarray(q, np.float64)
    kv_new = np.asarray(kv_new, np.float64)
    scale = 1.0 / np.sqrt(D) if not scale else float(scale)
    B, H = q.shape[:2]
    o = np.zeros((B, H, DV))
    rows = np.zeros((B, D), np.float32)
    for b in range(B):
        pos = int(seq_len[b])
        cs = (None, None) if cos_table is None else (cos_table[pos], sin_table[pos])
        row = kv_new[b].copy()
        row[DV:] = round_to(rope_interleaved(kv_new[b, DV:], pos, ROT, cos=cs[0], sin=cs[1]), dtype)
        qb = q[b].copy()
        qb[:, DV:] = round_to(rope_interleaved(q[b, :, DV:], pos, ROT, cos=cs[0], sin=cs[1]), dtype)
        C = np.concatenate([np.asarray(cache[b, :pos], np.float64), row[None]])     # rows 0..pos
        s = qb @ C.T * scale
        p = np.exp(s - s.max(axis=1, keepdims=True))
        o[b] = (p / p.sum(axis=1, keepdims=True)) @ C[:, :DV]
        rows[b] = row
    return o, rows
