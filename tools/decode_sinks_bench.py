#!/usr/bin/env python3
"""Attention-sink timings (profiles/decode_sinks_sweep.txt): each _sinks call against its _window twin on the same
buffers, in one process on one device, interleaved -- five rounds of (twin, sinks), HIP events around back-to-back calls
after a warm-up; per call the best of the five and their spread (max - min) / min.

Shapes: H = 64 query heads over Hkv = 8 kv heads, head_dim 64, bf16 (gpt-oss's attention), paged16 and blmhd caches,
B = 64 and 256.
  single token   pos 8191 with window 128 (memory_max_len 8192); pos 32767 with window 128 and with
                 window = memory_max_len = 32768 (a full-attention layer)
  chunk, varlen  the same positions and windows with 1 and with 8 tokens per sequence
  prompt         one 2048-token prompt per sequence under window 128 (B = 4, pos 0), chunk and varlen
The expectation is equal time: the sink is a few instructions per query row, once.  The yardstick is the twin's own time
in the same run and the margin its spread; every line says whether the ratio is inside it.
--small: the same lines at toy sizes (a rehearsal of the script, not a measurement)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import starflashattention_amd as sfa

dev = torch.device("cuda:0")
dt = torch.bfloat16
H, HKV, D, PS = 64, 8, 64, 16
SMALL = "--small" in sys.argv


def window_of(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3        # us per call


def interleaved(twin, sinks, iters):
    """((best, spread) of the twin, (best, spread) of the sinks call): five rounds of one timed window each, alternating"""
    for _ in range(3):
        twin()
        sinks()
    tt, ts = [], []
    for _ in range(5):
        tt.append(window_of(twin, iters))
        ts.append(window_of(sinks, iters))
    stat = lambda t: (min(t), (max(t) - min(t)) / min(t))
    return stat(tt), stat(ts)


def report(label, twin, sinks, iters):
    (tw, sw), (tsk, ssk) = interleaved(twin, sinks, iters)
    ratio = tsk / tw
    verdict = "EQUAL within the twin's spread" if abs(ratio - 1.0) <= sw else (
        f"MISS: sinks {'slower' if ratio > 1 else 'faster'} by {abs(ratio - 1) * 100:.1f} %, the twin's spread is "
        f"{sw * 100:.1f} %")
    print(f"{label}: window {tw:9.1f} us (+{100 * sw:4.1f} %) | sinks {tsk:9.1f} us (+{100 * ssk:4.1f} %) | "
          f"sinks / window {ratio:5.3f} | {verdict}", flush=True)
    sfa.check_decode_status()


def caches(B, M, layout):
    kw = dict(kv_layout="paged" if layout == "paged16" else layout, num_heads_kv=HKV)
    if layout == "paged16":
        P = M // PS
        shape = (B * P, 1, PS, HKV, D)
        kw["block_table"] = torch.randperm(B * P, device=dev, dtype=torch.int32).view(B, P)
    else:
        shape = (B, 1, M, HKV, D)
    return torch.empty(shape, device=dev, dtype=dt).normal_(), torch.empty(shape, device=dev, dtype=dt).normal_(), kw


def decode_shapes(B, M, layout, cases, iters):
    """cases: (pos, window) pairs on one pair of caches"""
    kc, vc, kw = caches(B, M, layout)
    z = torch.zeros(0, dtype=dt, device=dev)
    sk = torch.randn(H, device=dev, dtype=torch.float32)
    for pos, window in cases:
        sl = torch.full((B,), pos, dtype=torch.int32, device=dev)
        qkv = torch.randn(B, H + 2 * HKV, D, device=dev).to(dt)
        o = torch.empty(B, H, D, device=dev, dtype=dt)
        tail = (kc, vc, sl, o, B, M, H, D, D, M, 1, 0, window)
        report(f"decode B={B} pos={pos} window={window} {layout}",
               lambda: sfa.flash_decode_window(qkv, z, z, z, *tail, **kw),
               lambda: sfa.flash_decode_window_sinks(qkv, z, z, z, *tail, sk, **kw), iters(window))
        for n in (1, 8):
            p = min(pos, M - n)
            sl = torch.full((B,), p, dtype=torch.int32, device=dev)
            qkv = torch.randn(B, n, H + 2 * HKV, D, device=dev).to(dt)
            o = torch.empty(B, n, H, D, device=dev, dtype=dt)
            tail = (kc, vc, sl, o, B, M, H, D, D, M, 1, 0, window)
            report(f"chunk  B={B} pos={p} n={n} window={window} {layout}",
                   lambda: sfa.flash_decode_chunk_window(qkv, z, z, z, *tail, **kw),
                   lambda: sfa.flash_decode_chunk_window_sinks(qkv, z, z, z, *tail, sk, **kw), iters(window))
            cu = torch.arange(0, (B + 1) * n, n, dtype=torch.int32, device=dev)
            qv, ov = qkv.view(B * n, H + 2 * HKV, D), o.view(B * n, H, D)
            tail = (kc, vc, sl, ov, cu, B, M, H, D, D, M, 1, 0, window)
            report(f"varlen B={B} pos={p} n={n} window={window} {layout}",
                   lambda: sfa.flash_decode_varlen_window(qv, z, z, z, *tail, **kw),
                   lambda: sfa.flash_decode_varlen_window_sinks(qv, z, z, z, *tail, sk, **kw), iters(window))
    del kc, vc
    torch.cuda.empty_cache()


def prompt(layout):
    B, n, window = (4, 2048, 128) if not SMALL else (2, 256, 32)
    M = n
    kc, vc, kw = caches(B, M, layout)
    z = torch.zeros(0, dtype=dt, device=dev)
    sk = torch.randn(H, device=dev, dtype=torch.float32)
    sl = torch.zeros(B, dtype=torch.int32, device=dev)
    qkv = torch.randn(B, n, H + 2 * HKV, D, device=dev).to(dt)
    o = torch.empty(B, n, H, D, device=dev, dtype=dt)
    tail = (kc, vc, sl, o, B, M, H, D, D, M, 1, 0, window)
    report(f"prompt chunk  B={B} pos=0 n={n} window={window} {layout}",
           lambda: sfa.flash_decode_chunk_window(qkv, z, z, z, *tail, **kw),
           lambda: sfa.flash_decode_chunk_window_sinks(qkv, z, z, z, *tail, sk, **kw), 20)
    cu = torch.arange(0, (B + 1) * n, n, dtype=torch.int32, device=dev)
    qv, ov = qkv.view(B * n, H + 2 * HKV, D), o.view(B * n, H, D)
    tail = (kc, vc, sl, ov, cu, B, M, H, D, D, M, 1, 0, window)
    report(f"prompt varlen B={B} pos=0 n={n} window={window} {layout}",
           lambda: sfa.flash_decode_varlen_window(qv, z, z, z, *tail, **kw),
           lambda: sfa.flash_decode_varlen_window_sinks(qv, z, z, z, *tail, sk, **kw), 20)


if __name__ == "__main__":
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    print(f"H={H} Hkv={HKV} D={D} bf16; five interleaved rounds per pair, best (+spread)", flush=True)
    short, long_ = (8192, 32768) if not SMALL else (512, 1024)
    for layout in ("paged16", "blmhd"):
        for B in (64, 256) if not SMALL else (4,):
            decode_shapes(B, short, layout, [(short - 1, 128)], lambda w: 50)
            decode_shapes(B, long_, layout, [(long_ - 1, 128), (long_ - 1, long_)], lambda w: 50 if w == 128 else 8)
        prompt(layout)
