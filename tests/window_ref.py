"""Reference of sfa_decode_window for tests/test_decode_window_{cpu,gpu}.py: an adapter over tests/serving_model.py, which
holds the arithmetic (the prologue of the new token, the fp64 softmax over the rows [lo, pos] of the cache after the
append, lo = max(0, pos + 1 - window)).  The rows below lo are never looked at, so they may hold NaN.  window=None is plain
sfa_decode.

Grouped queries are native: q has H heads, k / v and the caches Hkv, query head h reads kv head h // (H // Hkv).
"""
import numpy as np

import serving_model as sm          # (imports this module for window_lo)
from oracle import to_bits16

TOL = {"fp16": 2e-3, "bf16": 1.6e-2}          # the project's decode tolerances (tests/test_decode_gpu.py), atol = rtol


def window_lo(pos, window):
    return 0 if window is None else max(0, pos + 1 - int(window))


def decode_window_model(q, k, v, k_cache, v_cache, seq_len, idx_layer, rot_dim, window, sinks, dtype, q_bias, k_bias, v_bias,
                        cos_table, sin_table, scale):
    """The 16-bit single-token call through the model, for decode_window_ref and sinks_ref.decode_window_sinks_ref: float
    caches [B, L, M, Hkv, D] representable in dtype (idx_layer alone is turned into bits).  Returns dict(o, k_row, v_row,
    lse, o64)."""
    q, k, v = (np.asarray(x, np.float32) for x in (q, k, v))
    call = sm.make_call(dtype, q.shape[1], seq_len, [1] * len(q), [np.concatenate(x)[None] for x in zip(q, k, v)], 0, rot_dim,
                        q_bias=q_bias, k_bias=k_bias, v_bias=v_bias, cos=cos_table, sin=sin_table, window=window, sinks=sinks,
                        softmax_scale=scale)
    cache = tuple(to_bits16(np.asarray(c)[:, idx_layer:idx_layer + 1], dtype) for c in (k_cache, v_cache))
    app, res = sm.run(cache, call)
    o = np.stack([r[0][0] for r in res])
    return dict(o=o.astype(np.float32), k_row=np.stack([x[0] for x in app["k16"]]), v_row=np.stack([x[0] for x in app["v16"]]),
                lse=np.stack([r[1][0] for r in res]), o64=o)


def decode_window_ref(q, k, v, k_cache, v_cache, seq_len, idx_layer, rot_dim, window, dtype="fp16",
                      q_bias=None, k_bias=None, v_bias=None, cos_table=None, sin_table=None, scale=None):
    """q [B, H, D], k / v [B, Hkv, D], caches [B, L, M, Hkv, D] (float, representable in `dtype`; not modified),
    biases [H, D] / [Hkv, D] / [Hkv, D].  Returns dict(o [B, H, D] float32 unrounded, k_row, v_row [B, Hkv, D] float32 =
    what the call stores at cache row seq_len[b])."""
    ref = decode_window_model(q, k, v, k_cache, v_cache, seq_len, idx_layer, rot_dim, window, None, dtype, q_bias, k_bias,
                              v_bias, cos_table, sin_table, scale)
    return {key: ref[key] for key in ("o", "k_row", "v_row")}


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
