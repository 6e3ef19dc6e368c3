#!/usr/bin/env python3
"""sfa_decode_kv8 timings (HIP events over back-to-back calls after a warm-up) beside sfa_decode on a 16-bit cache of the
same shape, in the same process on the same device:
  * BASELINE config 4 (B = 256, Sk = 8192, H = 32, D = 128, bf16), one query head per kv head
  * the grouped-query shape of bench.py --full (32 query heads over 4 kv heads) and the same with 2 kv heads
    (8 and 16 query heads per kv head)
each over the blmhd, blhmd and paged (page_size 16, shuffled table) layouts.  Per shape: microseconds (the best of five
runs) and TB/s over the cache bytes actually read, the five-run spread of each call, and the ratio.  The bar is relative:
the fp8 call has to beat the 16-bit call of the same run by more than that call's own spread; bytes halve, so the ceiling
of the ratio is 0.50.
The fp8 cache is filled the way a prompt gets into it: quantize_kv8 of the 16-bit cache with scale = amax / 448 per kv
head; that call is timed too.
  --mha-only   the MHA blmhd shape alone, fp8 call only (for rocprofv3 --kernel-trace --stats)"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import starflashattention_amd as sfa

dev = torch.device("cuda:0")
dt = torch.bfloat16
PS = 16


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


def caches16(B, Hkv, D, M, layout):
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


def head_amax(c, layout):
    """amax per kv head, one batch / page slab at a time (no fp32 copy of the whole cache)"""
    axis = 2 if layout == "blhmd" else 3
    a = torch.zeros(c.shape[axis], device=dev)
    for i in range(0, c.shape[0], 4096 if layout == "paged" else 8):
        s = c[i:i + (4096 if layout == "paged" else 8)].abs()
        a = torch.maximum(a, s.movedim(axis, 0).flatten(1).amax(dim=1).float())
    return a


def quantize(c, scale, layout):
    """the whole 16-bit cache -> an fp8 cache of the same layout; returns (cache, microseconds)"""
    out = torch.empty(c.shape, dtype=torch.uint8, device=dev)
    if layout == "blhmd":       # one call per sequence: [M, Hkv, D] views of the head-major slices
        def run():
            for b in range(c.shape[0]):
                sfa.quantize_kv8(c[b, 0].permute(1, 0, 2), scale, out=out[b, 0].permute(1, 0, 2))
    else:                       # one layer: the rows of all sequences (all pages) are one strided run
        Hkv, D = c.shape[3], c.shape[4]
        run = lambda: sfa.quantize_kv8(c.view(-1, Hkv, D), scale, out=out.view(-1, Hkv, D))
    return out, timed(run, 2)


def shape(B, H, Hkv, D, Sk, layout, iters, fp8_only=False):
    M = Sk
    kc, vc, kw = caches16(B, Hkv, D, M, layout)
    if Hkv != H:
        kw["num_heads_kv"] = Hkv
    ks, vs = head_amax(kc, layout) / 448.0, head_amax(vc, layout) / 448.0
    k8, t_q = quantize(kc, ks, layout)
    v8, _ = quantize(vc, vs, layout)
    z = torch.zeros(0, dtype=dt, device=dev)
    qkv = torch.randn((B, 3, H, D) if Hkv == H else (B, H + 2 * Hkv, D), device=dev).to(dt)
    o = torch.empty(B, H, D, device=dev, dtype=dt)
    sl = torch.full((B,), Sk - 1, dtype=torch.int32, device=dev)
    f8 = lambda: sfa.flash_decode_kv8(qkv, z, z, z, k8, v8, sl, o, B, M, H, D, D, M, 1, 0, k_scale=ks, v_scale=vs, **kw)
    f16 = lambda: sfa.flash_decode(qkv, z, z, z, kc, vc, sl, o, B, M, H, D, D, M, 1, 0, **kw)
    if fp8_only:
        print(f"kv8 only: {timed(f8, iters):.1f} us", flush=True)
        return
    t16 = [timed(f16, iters) for _ in range(5)]
    t8 = [timed(f8, iters) for _ in range(5)]
    sfa.check_decode_status()
    elems = 2.0 * B * (Sk - 1) * Hkv * D             # cache elements a call reads
    a, b = min(t16), min(t8)
    s16, s8 = max(t16) - a, max(t8) - b
    verdict = "FASTER" if a - b > s16 else "not faster beyond the 16-bit call's spread"
    qbytes = 3.0 * kc.numel()                       # the quantise call: 2 bytes in, 1 out per element
    print(f"B={B} H={H} Hkv={Hkv} D={D} Sk={Sk} bf16 {layout}{PS if layout == 'paged' else ''}: "
          f"kv8 {b:8.1f} us {elems / b / 1e6:5.2f} TB/s (5 runs spread {s8:.1f}) | 16-bit {a:8.1f} us "
          f"{2 * elems / a / 1e6:5.2f} TB/s (5 runs spread {s16:.1f}) | kv8 / 16-bit {b / a:4.2f}x: {verdict} | "
          f"quantize_kv8 of one cache {t_q:8.1f} us {qbytes / t_q / 1e6:5.2f} TB/s", flush=True)


if __name__ == "__main__":
    if "--mha-only" in sys.argv:
        shape(256, 32, 32, 128, 8192, "blmhd", 20, fp8_only=True)
        sys.exit(0)
    for layout in ("blmhd", "blhmd", "paged"):
        shape(256, 32, 32, 128, 8192, layout, 20)
        torch.cuda.empty_cache()
    for Hkv in (4, 2):
        for layout in ("blmhd", "blhmd", "paged"):
            shape(256, 32, Hkv, 128, 8192, layout, 30)
            torch.cuda.empty_cache()
