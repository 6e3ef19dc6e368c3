#!/usr/bin/env python3
"""Attention-sink timings over the fp8 KV cache (profiles/decode_kv8_sinks_sweep.txt): each _kv8_window_sinks call against
its _kv8_window twin on the same buffers, in one process on one device, interleaved -- five rounds of (twin, sinks), HIP
events around back-to-back calls after a warm-up; per call the best of the five and their spread (max - min) / min.  Beside
every fp8 pair the 16-bit pair (_window_sinks against _window) of the same shape is timed in the same process, so that the
fp8 difference can be read against the 16-bit one (DESIGN.md 5.16 recorded 2-3 us there under a 128-row window).

Shapes: H = 64 query heads over Hkv = 8 kv heads, head_dim 64, bf16 (gpt-oss's attention), paged16 and blmhd caches,
B = 64 and 256.
  single token   pos 8191 with window 128 (memory_max_len 8192); pos 32767 with window 128 and with
                 window = memory_max_len = 32768 (a full-attention layer)
  chunk, varlen  the same positions and windows with 1 and with 8 tokens per sequence
The expectation is equal time: the sink is a few instructions per query row, once.  The yardstick is the twin's own time
in the same run and the margin its spread; every line says whether the ratio is inside it.
--out PATH: where the lines are written as well (default profiles/decode_kv8_sinks_sweep.txt).
--small: the same lines at toy sizes (a rehearsal of the script, not a measurement)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

import starflashattention_amd as sfa

dev = torch.device("cuda:0")
dt = torch.bfloat16
H, HKV, D, PS = 64, 8, 64, 16
SMALL = "--small" in sys.argv
OUT = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "decode_kv8_sinks_sweep.txt")
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


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


def report(label, cache, twin, sinks, iters):
    (tw, sw), (tsk, ssk) = interleaved(twin, sinks, iters)
    ratio = tsk / tw
    verdict = "EQUAL within the twin's spread" if abs(ratio - 1.0) <= sw else (
        f"MISS: sinks {'slower' if ratio > 1 else 'faster'} by {abs(ratio - 1) * 100:.1f} % ({tsk - tw:+.1f} us), the twin's "
        f"spread is {sw * 100:.1f} %")
    say(f"{label} {cache:5s}: twin {tw:9.1f} us (+{100 * sw:4.1f} %) | sinks {tsk:9.1f} us (+{100 * ssk:4.1f} %) | "
        f"sinks / twin {ratio:5.3f} | {verdict}")
    sfa.check_decode_status()


def caches(B, M, layout):
    """(16-bit k, v), (e4m3 k, v: random finite bytes of magnitude below 2), the scales and the layout's keywords"""
    kw = dict(kv_layout="paged" if layout == "paged16" else layout, num_heads_kv=HKV)
    if layout == "paged16":
        P = M // PS
        shape = (B * P, 1, PS, HKV, D)
        kw["block_table"] = torch.randperm(B * P, device=dev, dtype=torch.int32).view(B, P)
    else:
        shape = (B, 1, M, HKV, D)
    b16 = tuple(torch.empty(shape, device=dev, dtype=dt).normal_() for _ in range(2))
    byte = lambda: (torch.randint(0, 0x40, shape, device=dev, dtype=torch.uint8)
                    | (torch.randint(0, 2, shape, device=dev, dtype=torch.uint8) << 7))
    b8 = (byte(), byte())
    scales = dict(k_scale=torch.full((HKV,), 0.75, device=dev), v_scale=torch.full((HKV,), 1.25, device=dev))
    return b16, b8, scales, kw


def decode_shapes(B, M, layout, cases, iters):
    """cases: (pos, window) pairs on one set of caches"""
    (kc, vc), (k8, v8), sc, kw = caches(B, M, layout)
    kw8 = dict(kw, **sc)
    z = torch.zeros(0, dtype=dt, device=dev)
    sk = torch.randn(H, device=dev, dtype=torch.float32)
    for pos, window in cases:
        sl = torch.full((B,), pos, dtype=torch.int32, device=dev)
        qkv = torch.randn(B, H + 2 * HKV, D, device=dev).to(dt)
        o = torch.empty(B, H, D, device=dev, dtype=dt)
        t8, t16 = (k8, v8, sl, o, B, M, H, D, D, M, 1, 0, window), (kc, vc, sl, o, B, M, H, D, D, M, 1, 0, window)
        label = f"decode B={B} pos={pos} window={window} {layout}"
        report(label, "fp8", lambda: sfa.flash_decode_kv8_window(qkv, z, z, z, *t8, **kw8),
               lambda: sfa.flash_decode_kv8_window_sinks(qkv, z, z, z, *t8, sk, **kw8), iters(window))
        report(label, "16bit", lambda: sfa.flash_decode_window(qkv, z, z, z, *t16, **kw),
               lambda: sfa.flash_decode_window_sinks(qkv, z, z, z, *t16, sk, **kw), iters(window))
        for n in (1, 8):
            p = min(pos, M - n)
            sl = torch.full((B,), p, dtype=torch.int32, device=dev)
            qkv = torch.randn(B, n, H + 2 * HKV, D, device=dev).to(dt)
            o = torch.empty(B, n, H, D, device=dev, dtype=dt)
            t8, t16 = (k8, v8, sl, o, B, M, H, D, D, M, 1, 0, window), (kc, vc, sl, o, B, M, H, D, D, M, 1, 0, window)
            label = f"chunk  B={B} pos={p} n={n} window={window} {layout}"
            report(label, "fp8", lambda: sfa.flash_decode_chunk_kv8_window(qkv, z, z, z, *t8, **kw8),
                   lambda: sfa.flash_decode_chunk_kv8_window_sinks(qkv, z, z, z, *t8, sk, **kw8), iters(window))
            report(label, "16bit", lambda: sfa.flash_decode_chunk_window(qkv, z, z, z, *t16, **kw),
                   lambda: sfa.flash_decode_chunk_window_sinks(qkv, z, z, z, *t16, sk, **kw), iters(window))
            cu = torch.arange(0, (B + 1) * n, n, dtype=torch.int32, device=dev)
            qv, ov = qkv.view(B * n, H + 2 * HKV, D), o.view(B * n, H, D)
            t8 = (k8, v8, sl, ov, cu, B, M, H, D, D, M, 1, 0, window)
            t16 = (kc, vc, sl, ov, cu, B, M, H, D, D, M, 1, 0, window)
            label = f"varlen B={B} pos={p} n={n} window={window} {layout}"
            report(label, "fp8", lambda: sfa.flash_decode_varlen_kv8_window(qv, z, z, z, *t8, **kw8),
                   lambda: sfa.flash_decode_varlen_kv8_window_sinks(qv, z, z, z, *t8, sk, **kw8), iters(window))
            report(label, "16bit", lambda: sfa.flash_decode_varlen_window(qv, z, z, z, *t16, **kw),
                   lambda: sfa.flash_decode_varlen_window_sinks(qv, z, z, z, *t16, sk, **kw), iters(window))
    del kc, vc, k8, v8
    torch.cuda.empty_cache()


if __name__ == "__main__":
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    say(f"H={H} Hkv={HKV} D={D} bf16; five interleaved rounds per pair, best (+spread); fp8 = the _kv8_window pair, "
        f"16bit = the _window pair of the same shape" + (" [--small: a rehearsal, not a measurement]" if SMALL else ""))
    short, long_ = (8192, 32768) if not SMALL else (512, 1024)
    for layout in ("paged16", "blmhd"):
        for B in (64, 256) if not SMALL else (4,):
            decode_shapes(B, short, layout, [(short - 1, 128)], lambda w: 50)
            decode_shapes(B, long_, layout, [(long_ - 1, 128), (long_ - 1, long_)], lambda w: 50 if w == 128 else 8)
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        f.write("\n".join(lines) + "\n")
