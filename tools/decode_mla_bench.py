#!/usr/bin/env python3
"""sfa_decode_mla timings: HIP events over back-to-back calls after a warm-up, five repeats, best and spread.
bf16, contiguous and paged (page_size 64, shuffled table), pos in {4095, 32767}, (B, H) in {(256, 16), (64, 16),
(32, 128), (4, 128)}, the library's split choice and one split.  Per line: microseconds per call, TB/s over the cache
bytes read (B * pos * 1152), TFLOP/s (B * H * pos * 2 * (576 + 512)), which of the two bounds the least-time estimate
(8 TB/s HBM, 2.5 PFLOP/s dense bf16) and the share of it reached.
Beside them, in the same process on the same device:
  * at H = 16, flash_decode with 16 query heads over one kv head of head_dim 256 over the same number of cache bytes
    (pos * 9 / 8 rows of 1024 B): the nearest existing kernel;
  * bench.py --full's gemm_calibration workload (torch.matmul bf16 8192^3): what the matrix cores sustain here.
  --splits   the split sweep on the (4, 128) and (64, 16) lines instead (1, 2, 4, 8, 16, 32 and the library's choice)"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import starflashattention_amd as sfa

dev = torch.device("cuda:0")
dt = torch.bfloat16
PS, ROW = 64, 576
PEAK_TBS, PEAK_TFLOPS = 8.0, 2500.0


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


def five(fn, iters):
    t = [timed(fn, iters) for _ in range(5)]
    return min(t), max(t) - min(t)


def mla_call(B, H, pos, layout, splits):
    M = pos + 1
    kw = {}
    if layout == "paged":
        P = M // PS
        cache = torch.empty((B * P, 1, PS, ROW), device=dev, dtype=dt).normal_()
        kw["block_table"] = torch.randperm(B * P, device=dev, dtype=torch.int32).view(B, P)
    else:
        cache = torch.empty((B, 1, M, ROW), device=dev, dtype=dt).normal_()
    q = torch.randn(B, H, ROW, device=dev).to(dt)
    kvn = torch.randn(B, ROW, device=dev).to(dt)
    o = torch.empty(B, H, 512, device=dev, dtype=dt)
    sl = torch.full((B,), pos, dtype=torch.int32, device=dev)
    return lambda: sfa.flash_decode_mla(q, kvn, cache, sl, o, idx_layer=0, num_splits=splits, **kw)


def gqa_call(B, pos):
    """flash_decode, 16 query heads over one kv head of head_dim 256, over the bytes of an MLA call at `pos`"""
    rows = pos * 9 // 8
    M, H, D = rows + 1, 16, 256
    kc = torch.empty((B, 1, M, 1, D), device=dev, dtype=dt).normal_()
    vc = torch.empty((B, 1, M, 1, D), device=dev, dtype=dt).normal_()
    z = torch.zeros(0, dtype=dt, device=dev)
    qkv = torch.randn(B, H + 2, D, device=dev).to(dt)
    o = torch.empty(B, H, D, device=dev, dtype=dt)
    sl = torch.full((B,), rows, dtype=torch.int32, device=dev)
    return lambda: sfa.flash_decode(qkv, z, z, z, kc, vc, sl, o, B, M, H, D, D, M, 1, 0, num_heads_kv=1)


def report(tag, us, spread, B, H, pos):
    tbs = B * pos * 2.0 * ROW / us / 1e6
    tfl = B * H * pos * 2.0 * (ROW + 512) / us / 1e6
    t_hbm, t_mfma = B * pos * 2.0 * ROW / PEAK_TBS / 1e6, B * H * pos * 2.0 * (ROW + 512) / PEAK_TFLOPS / 1e6
    bound = "HBM" if t_hbm >= t_mfma else "MFMA"
    print(f"{tag}: {us:9.1f} us (5 runs spread {spread:.1f}) {tbs:5.2f} TB/s {tfl:7.1f} TFLOP/s | bound {bound}, "
          f"{max(t_hbm, t_mfma) / us:5.1%} of it", flush=True)
    return tbs


def iters_for(B, pos):
    return max(5, min(100, int(2e9 / (B * pos * 2.0 * ROW))))


def sweep():
    a = torch.randn(8192, 8192, device=dev).to(dt)
    bt = torch.randn(8192, 8192, device=dev).to(dt).t()
    us, spread = five(lambda: torch.matmul(a, bt), 20)
    print(f"gemm_calibration torch.matmul bf16 8192^3: {2.0 * 8192 ** 3 / us / 1e6:7.1f} TFLOP/s (5 runs spread {spread:.1f} us)",
          flush=True)
    del a, bt
    for pos in (4095, 32767):
        for B, H in ((256, 16), (64, 16), (32, 128), (4, 128)):
            it = iters_for(B, pos)
            for layout in ("blmhd", "paged"):
                for splits in (0, 1):
                    S = splits or sfa.decode_mla_auto_splits(B, H, pos + 1)
                    us, spread = five(mla_call(B, H, pos, layout, S), it)
                    tbs = report(f"mla B={B:3d} H={H:3d} pos={pos:5d} {layout:5s} S={S:2d}{' (auto)' if not splits else '       '}",
                                 us, spread, B, H, pos)
                    torch.cuda.empty_cache()
            if H == 16:
                us, spread = five(gqa_call(B, pos), it)
                g = B * pos * 2.0 * ROW / us / 1e6
                print(f"    flash_decode G=16 D=256 blmhd over the same bytes: {us:9.1f} us (spread {spread:.1f}) {g:5.2f} TB/s"
                      f" | mla (paged, 1 split) / it: {tbs / g:4.2f}", flush=True)
                torch.cuda.empty_cache()
    sfa.check_decode_status()


def splits():
    for pos in (4095, 32767):
        for B, H in ((4, 128), (64, 16)):
            auto = sfa.decode_mla_auto_splits(B, H, pos + 1)
            for S in (1, 2, 4, 8, 16, 32):
                us, spread = five(mla_call(B, H, pos, "blmhd", S), iters_for(B, pos))
                report(f"splits B={B:3d} H={H:3d} pos={pos:5d} S={S:2d}{' = auto' if S == auto else '       '}", us, spread,
                       B, H, pos)
                torch.cuda.empty_cache()


if __name__ == "__main__":
    splits() if "--splits" in sys.argv else sweep()
