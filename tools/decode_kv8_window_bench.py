#!/usr/bin/env python3
"""sfa_decode_kv8_window timings (HIP events over back-to-back calls after a warm-up) beside the calls it combines, in
the same process on the same device: B = 256, H = 32 query heads over 32 and 4 kv heads, D = 128, bf16, memory_max_len
32768, over the blmhd, blhmd and paged (page_size 16, shuffled table) layouts.  Four calls per shape:
  * sfa_decode_kv8_window at pos = 32767 with a window of 4096: reads the rows 28672 .. 32766 of the fp8 caches
  * sfa_decode_kv8 at pos = 4095: the same number of bytes (the rows 0 .. 4094), the kernel without the window
  * sfa_decode_kv8 at pos = 32767: what a layer without the window costs over the fp8 cache
  * sfa_decode_window at pos = 32767, window 4096, on the 16-bit cache the fp8 cache was quantised from
Per call: microseconds (the best of five runs), the five-run spread and TB/s over the cache bytes it reads.  The
expectation is parity of the first with the second within the sum of the two spreads; the line says whether it is met
and by how much it is missed.  The ratio to the 16-bit windowed call is reported, not judged.
The fp8 caches are quantize_kv8 of the 16-bit ones with one fixed scale (6 / 448: N(0,1) data); the 16-bit call is timed
first and each 16-bit cache is freed once it is quantised, so the peak is the two 16-bit caches plus one fp8 cache.
  --small   Hkv = 4 only (an eighth of the memory)"""
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


def cache16(B, Hkv, D, M, layout):
    """an N(0,1) bf16 cache of one layer in `layout`"""
    if layout == "paged":
        shape = (B * (M // PS), 1, PS, Hkv, D)
    elif layout == "blhmd":
        shape = (B, 1, Hkv, M, D)
    else:
        shape = (B, 1, M, Hkv, D)
    return torch.empty(shape, device=dev, dtype=dt).normal_()


def quantized(c, scale, layout):
    """the whole 16-bit cache -> an fp8 cache of the same layout"""
    out = torch.empty(c.shape, dtype=torch.uint8, device=dev)
    if layout == "blhmd":       # one call per sequence: [M, Hkv, D] views of the head-major slices
        for b in range(c.shape[0]):
            sfa.quantize_kv8(c[b, 0].permute(1, 0, 2), scale, out=out[b, 0].permute(1, 0, 2))
    else:                       # one layer: the rows of all sequences (all pages) are one strided run
        Hkv, D = c.shape[3], c.shape[4]
        sfa.quantize_kv8(c.view(-1, Hkv, D), scale, out=out.view(-1, Hkv, D))
    torch.cuda.synchronize()
    return out


def best(fn, iters):
    t = [timed(fn, iters) for _ in range(5)]
    return min(t), max(t) - min(t)


def shape(B, H, Hkv, D, M, layout, iters):
    kw = dict(kv_layout=layout)
    if layout == "paged":
        kw["block_table"] = torch.randperm(B * (M // PS), device=dev, dtype=torch.int32).view(B, M // PS)
    if Hkv != H:
        kw["num_heads_kv"] = Hkv
    z = torch.zeros(0, dtype=dt, device=dev)
    qkv = torch.randn((B, 3, H, D) if Hkv == H else (B, H + 2 * Hkv, D), device=dev).to(dt)
    o = torch.empty(B, H, D, device=dev, dtype=dt)
    last = torch.full((B,), M - 1, dtype=torch.int32, device=dev)
    short = torch.full((B,), WINDOW - 1, dtype=torch.int32, device=dev)
    scale = torch.full((Hkv,), 6.0 / 448.0, device=dev)
    kc, vc = cache16(B, Hkv, D, M, layout), cache16(B, Hkv, D, M, layout)
    w16, s16 = best(lambda: sfa.flash_decode_window(qkv, z, z, z, kc, vc, last, o, B, M, H, D, D, M, 1, 0, WINDOW, **kw), iters)
    k8 = quantized(kc, scale, layout)
    del kc
    v8 = quantized(vc, scale, layout)
    del vc
    torch.cuda.empty_cache()
    kw.update(k_scale=scale, v_scale=scale)
    win = lambda: sfa.flash_decode_kv8_window(qkv, z, z, z, k8, v8, last, o, B, M, H, D, D, M, 1, 0, WINDOW, **kw)
    same = lambda: sfa.flash_decode_kv8(qkv, z, z, z, k8, v8, short, o, B, M, H, D, D, M, 1, 0, **kw)
    full = lambda: sfa.flash_decode_kv8(qkv, z, z, z, k8, v8, last, o, B, M, H, D, D, M, 1, 0, **kw)
    (w, sw), (s, ss), (f, sf) = best(win, iters), best(same, iters), best(full, max(2, iters // 4))
    sfa.check_decode_status()
    rows = lambda n, eb: 2.0 * eb * B * n * Hkv * D     # cache bytes of n rows per sequence at eb bytes per element
    verdict = "PARITY within the two spreads" if abs(w - s) <= sw + ss else (
        f"window SLOWER by {w - s:.1f} us ({(w / s - 1) * 100:.1f} %), {w - s - (sw + ss):.1f} us beyond the spreads" if w > s
        else f"window FASTER by {s - w:.1f} us ({(1 - w / s) * 100:.1f} %)")
    print(f"B={B} H={H} Hkv={Hkv} D={D} M={M} bf16 {layout}{PS if layout == 'paged' else ''}: "
          f"kv8 window {WINDOW} at pos {M - 1} {w:8.1f} us {rows(WINDOW - 1, 1) / w / 1e6:5.2f} TB/s (5 runs spread {sw:.1f}) | "
          f"sfa_decode_kv8 at pos {WINDOW - 1} {s:8.1f} us {rows(WINDOW - 1, 1) / s / 1e6:5.2f} TB/s (spread {ss:.1f}) | "
          f"sfa_decode_kv8 at pos {M - 1} {f:8.1f} us {rows(M - 1, 1) / f / 1e6:5.2f} TB/s (spread {sf:.1f}) | "
          f"16-bit sfa_decode_window {w16:8.1f} us {rows(WINDOW - 1, 2) / w16 / 1e6:5.2f} TB/s (spread {s16:.1f}) | "
          f"full / window {f / w:4.2f}x | kv8 window / 16-bit window {w / w16:4.2f}x | {verdict}", flush=True)


if __name__ == "__main__":
    for Hkv in (4,) if "--small" in sys.argv else (4, 32):
        for layout in ("blmhd", "blhmd", "paged"):
            shape(256, 32, Hkv, 128, 32768, layout, 40 if Hkv == 4 else 12)
            torch.cuda.empty_cache()
