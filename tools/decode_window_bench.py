#!/usr/bin/env python3
"""sfa_decode_window timings (HIP events over back-to-back calls after a warm-up) beside sfa_decode on the same caches,
in the same process on the same device: B = 256, H = 32 query heads over 32 and 4 kv heads, D = 128, bf16,
memory_max_len 32768, over the blmhd, blhmd and paged (page_size 16, shuffled table) layouts.  Three calls per shape:
  * sfa_decode_window at pos = 32767 with a window of 4096: reads the rows 28672 .. 32766
  * sfa_decode at pos = 4095: reads the same number of bytes (the rows 0 .. 4094)
  * sfa_decode at pos = 32767: what a layer without the window costs
Per call: microseconds (the best of five runs), the five-run spread and TB/s over the cache bytes it reads.  The
expectation is parity of the first with the second within the two spreads; the line says whether it is met and by how
much it is missed.
  --small   Hkv = 4 only (a quarter of the memory)"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import starflashattention_amd as sfa

dev = torch.device("cuda:0")
dt = torch.bfloat16
PS = 16
WINDOW = 4096


def timed(fn, iters):
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3          # us


def caches(B, Hkv, D, M, layout):
    """-> (k cache, v cache, keyword arguments), N(0,1) bf16 in every row / page"""
    kw = dict(kv_layout=layout)
    if layout == "paged":
        P = M // PS
        shape = (B * P, 1, PS, Hkv, D)
        kw["block_table"] = torch.randperm(B * P, device=dev, dtype=torch.int32).view(B, P)
    elif layout == "blhmd":
        shape = (B, 1, Hkv, M, D)
    else:
        shape = (B, 1, M, Hkv, D)
    return torch.empty(shape, device=dev, dtype=dt).normal_(), torch.empty(shape, device=dev, dtype=dt).normal_(), kw


def shape(B, H, Hkv, D, M, layout, iters):
    kc, vc, kw = caches(B, Hkv, D, M, layout)
    if Hkv != H:
        kw["num_heads_kv"] = Hkv
    z = torch.zeros(0, dtype=dt, device=dev)
    qkv = torch.randn((B, 3, H, D) if Hkv == H else (B, H + 2 * Hkv, D), device=dev).to(dt)
    o = torch.empty(B, H, D, device=dev, dtype=dt)
    last = torch.full((B,), M - 1, dtype=torch.int32, device=dev)
    short = torch.full((B,), WINDOW - 1, dtype=torch.int32, device=dev)
    win = lambda: sfa.flash_decode_window(qkv, z, z, z, kc, vc, last, o, B, M, H, D, D, M, 1, 0, WINDOW, **kw)
    same = lambda: sfa.flash_decode(qkv, z, z, z, kc, vc, short, o, B, M, H, D, D, M, 1, 0, **kw)
    full = lambda: sfa.flash_decode(qkv, z, z, z, kc, vc, last, o, B, M, H, D, D, M, 1, 0, **kw)
    tw = [timed(win, iters) for _ in range(5)]
    ts = [timed(same, iters) for _ in range(5)]
    tf = [timed(full, max(2, iters // 4)) for _ in range(5)]
    sfa.check_decode_status()
    rows = lambda n: 2.0 * 2 * B * n * Hkv * D          # cache bytes of n rows per sequence
    w, s, f = min(tw), min(ts), min(tf)
    sw, ss, sf = max(tw) - w, max(ts) - s, max(tf) - f
    miss = w - s - (sw + ss)
    verdict = "PARITY within the two spreads" if abs(w - s) <= sw + ss else (
        f"window SLOWER by {w - s:.1f} us ({(w / s - 1) * 100:.1f} %), {miss:.1f} us beyond the spreads" if w > s else
        f"window FASTER by {s - w:.1f} us ({(1 - w / s) * 100:.1f} %)")
    print(f"B={B} H={H} Hkv={Hkv} D={D} M={M} bf16 {layout}{PS if layout == 'paged' else ''}: "
          f"window {WINDOW} at pos {M - 1} {w:8.1f} us {rows(WINDOW - 1) / w / 1e6:5.2f} TB/s (5 runs spread {sw:.1f}) | "
          f"sfa_decode at pos {WINDOW - 1} {s:8.1f} us {rows(WINDOW - 1) / s / 1e6:5.2f} TB/s (spread {ss:.1f}) | "
          f"sfa_decode at pos {M - 1} {f:8.1f} us {rows(M - 1) / f / 1e6:5.2f} TB/s (spread {sf:.1f}) | "
          f"full / window {f / w:4.2f}x | {verdict}", flush=True)


if __name__ == "__main__":
    for Hkv in (4,) if "--small" in sys.argv else (4, 32):
        for layout in ("blmhd", "blhmd", "paged"):
            shape(256, 32, Hkv, 128, 32768, layout, 40 if Hkv == 4 else 12)
            torch.cuda.empty_cache()
