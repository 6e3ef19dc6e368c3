"""fp64 reference of sfa_decode_window for tests/test_decode_window_{cpu,gpu}.py.

The new token's rotated q, and the k and v rows the call appends, come from oracle.decode_ref (bias, RoPE, rounding to
the storage dtype: everything sfa_decode does before the attention).  The attention itself is done here, over the rows
[lo, pos] of the caches the device was given plus the new row, lo = max(0, pos + 1 - window): the rows below lo are
never looked at, so they may hold NaN.  window=None is plain sfa_decode.

Grouped queries are native: q has H heads, k / v and the caches Hkv, query head h reads kv head h // (H // Hkv).
"""
import numpy as np

from oracle import decode_ref

TOL = {"fp16": 2e-3, "bf16": 1.6e-2}          # the project's decode tolerances (tests/test_decode_gpu.py)


def window_lo(pos, window):
    return 0 if window is None else max(0, pos + 1 - int(window))


def decode_window_ref(q, k, v, k_cache, v_cache, seq_len, idx_layer, rot_dim, window, dtype="fp16",
                      q_bias=None, k_bias=None, v_bias=None, cos_table=None, sin_table=None, scale=None):
    """q [B, H, D], k / v [B, Hkv, D], caches [B, L, M, Hkv, D] (float, representable in `dtype`; not modified),
    biases [H, D] / [Hkv, D] / [Hkv, D].  Returns dict(o [B, H, D] float32 unrounded, k_row, v_row [B, Hkv, D] float32 =
    what the call stores at cache row seq_len[b])."""
    q, k, v = (np.asarray(x, np.float32) for x in (q, k, v))
    B, H, D = q.shape
    Hkv = k.shape[1]
    G = H // Hkv
    assert G * Hkv == H
    if scale is None:
        scale = 1.0 / np.sqrt(float(D))
    rep = lambda x: None if x is None else np.repeat(np.asarray(x, np.float32), G, axis=0)
    o = np.zeros((B, H, D), np.float64)
    k_rows = np.zeros((B, Hkv, D), np.float32)
    v_rows = np.zeros((B, Hkv, D), np.float32)
    for b in range(B):
        pos = int(seq_len[b])
        # the prologue, on the problem expanded to one kv head per query head; decode_ref's own attention runs over a
        # cache that holds the new row only (its result is not used)
        qkv_x = np.stack([q[b], np.repeat(k[b], G, axis=0), np.repeat(v[b], G, axis=0)])[None]
        dummy_k = np.zeros((1, 1, pos + 1, H, D), np.float32)
        pro = decode_ref(qkv_x, dummy_k, np.zeros_like(dummy_k), [pos], 0, rot_dim, dtype=dtype, q_bias=q_bias,
                         k_bias=rep(k_bias), v_bias=rep(v_bias), cos_table=cos_table, sin_table=sin_table)
        k_rows[b], v_rows[b] = pro["k_row"][0, ::G], pro["v_row"][0, ::G]
        lo = window_lo(pos, window)
        K = np.concatenate([np.asarray(k_cache[b, idx_layer, lo:pos], np.float64), k_rows[b][None].astype(np.float64)])
        V = np.concatenate([np.asarray(v_cache[b, idx_layer, lo:pos], np.float64), v_rows[b][None].astype(np.float64)])
        qr = pro["q_rot"][0].astype(np.float64).reshape(Hkv, G, D)
        sc = np.einsum("kgd,tkd->kgt", qr, K) * scale
        sc -= sc.max(axis=2, keepdims=True)
        p = np.exp(sc)
        p /= p.sum(axis=2, keepdims=True)
        o[b] = np.einsum("kgt,tkd->kgd", p, V).reshape(H, D)
    return dict(o=o.astype(np.float32), k_row=k_rows, v_row=v_rows)


# The parity sweep of tests/test_decode_window_gpu.py: (dtype, head_dim, layout, group, num_splits, window), a pairwise-
# covering subset of the product of FACTORS (every value of every factor meets every value of every other factor in at
# least one case; tests/test_decode_window_cpu.py checks that).  "paged16" / "paged64" = a paged cache of that page size.
FACTORS = (("fp16", "bf16"), (64, 128, 256), ("blmhd", "blhmd", "paged16", "paged64"), (1, 2, 4, 8, 16), (0, 1, 3),
           (1, 2, 17, 33, 64, 100, 129, 1000, 5000))
SWEEP = [
    ('fp16', 64, 'blmhd', 1, 0, 1),
    ('bf16', 128, 'blhmd', 2, 1, 2),
    ('fp16', 256, 'paged16', 4, 3, 17),
    ('bf16', 64, 'paged64', 8, 3, 33),
    ('fp16', 128, 'paged64', 16, 0, 64),
    ('bf16', 256, 'blmhd', 16, 1, 100),
    ('fp16', 256, 'blhmd', 8, 0, 129),
    ('bf16', 128, 'paged16', 1, 3, 1000),
    ('fp16', 64, 'paged16', 2, 1, 5000),
    ('bf16', 128, 'blmhd', 4, 0, 5000),
    ('fp16', 64, 'blhmd', 4, 1, 1000),
    ('bf16', 256, 'paged64', 2, 3, 1),
    ('fp16', 64, 'blmhd', 16, 3, 2),
    ('fp16', 256, 'paged64', 1, 1, 33),
    ('fp16', 128, 'paged16', 8, 0, 100),
    ('bf16', 64, 'blhmd', 1, 3, 64),
    ('bf16', 128, 'blmhd', 8, 1, 17),
    ('bf16', 64, 'paged16', 16, 1, 129),
    ('bf16', 256, 'blmhd', 2, 0, 1000),
    ('fp16', 128, 'paged64', 4, 3, 129),
    ('fp16', 256, 'blhmd', 16, 3, 5000),
    ('bf16', 256, 'paged16', 4, 0, 2),
    ('bf16', 64, 'paged64', 1, 0, 17),
    ('fp16', 128, 'blhmd', 2, 0, 33),
    ('fp16', 256, 'blmhd', 8, 1, 64),
    ('bf16', 128, 'blhmd', 4, 1, 1),
    ('fp16', 64, 'paged64', 2, 3, 100),
    ('bf16', 64, 'paged16', 16, 0, 33),
    ('fp16', 128, 'blmhd', 1, 3, 129),
    ('bf16', 256, 'paged64', 8, 1, 5000),
    ('fp16', 128, 'paged16', 16, 1, 1),
    ('bf16', 256, 'blhmd', 1, 0, 100),
    ('bf16', 128, 'paged16', 2, 3, 64),
    ('fp16', 64, 'paged64', 8, 0, 2),
    ('bf16', 64, 'blmhd', 4, 3, 33),
    ('fp16', 64, 'blhmd', 2, 1, 17),
    ('bf16', 128, 'paged64', 16, 0, 1000),
    ('fp16', 256, 'paged16', 1, 1, 2),
    ('bf16', 256, 'blhmd', 8, 3, 1),
    ('fp16', 256, 'blmhd', 4, 0, 64),
    ('bf16', 64, 'paged64', 4, 1, 100),
    ('fp16', 128, 'blmhd', 8, 3, 1000),
    ('fp16', 256, 'blhmd', 16, 3, 17),
    ('bf16', 64, 'paged16', 2, 0, 129),
    ('fp16', 128, 'paged64', 1, 1, 5000),
]
