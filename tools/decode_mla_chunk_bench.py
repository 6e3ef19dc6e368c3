#!/usr/bin/env python3
"""sfa_decode_mla_chunk timings beside the only other route to n new tokens, n successive sfa_decode_mla calls, in one
process: HIP events over back-to-back calls after a warm-up, five rounds that alternate the two, best and spread of each
(tools/decode_mla_bench.py's method).  bf16, contiguous and paged (page_size 64, shuffled table), the library's split
choice for both.
  H = 16, B in {64, 256}, pos in {4095, 32767}, n in {1, 2, 4, 8}: the call is HBM-bound, so the chunk should cost about
      what ONE single call costs; per line the ratio chunk / (n singles), chunk / (one single), and at n = 1 whether the
      two kernels agree within their spreads;
  H = 128, B in {4, 32}, n in {1, 2, 4}: the matrix cores bound it; TFLOP/s (B n H pos 2 (576 + 512)) beside
      bench.py --full's gemm_calibration workload (torch.matmul bf16 8192^3) from this process;
  --splits   the split sweep at (B, H, n) = (64, 16, 4) and (4, 128, 2) instead (1 .. 32 and the library's choice)"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import starflashattention_amd as sfa

dev = torch.device("cuda:0")
dt = torch.bfloat16
PS, ROW, NMAX = 64, 576, 8


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


def five(fns, iters):
    """five rounds, each timing every variant in turn: (best, spread) per variant"""
    t = [[timed(fn, iters) for fn in fns] for _ in range(5)]
    return [(min(c), max(c) - min(c)) for c in zip(*t)]


def calls(B, H, pos, n, layout, splits=0):
    """(the chunk call, n single calls at pos .. pos + n - 1) over one cache with room for the new rows"""
    M = pos + 1 + PS
    kw = {}
    if layout == "paged":
        P = M // PS
        cache = torch.empty((B * P, 1, PS, ROW), device=dev, dtype=dt).normal_()
        kw["block_table"] = torch.randperm(B * P, device=dev, dtype=torch.int32).view(B, P)
    else:
        cache = torch.empty((B, 1, M, ROW), device=dev, dtype=dt).normal_()
    q = torch.randn(B, n, H, ROW, device=dev).to(dt)
    kvn = torch.randn(B, n, ROW, device=dev).to(dt)
    o = torch.empty(B, n, H, 512, device=dev, dtype=dt)
    sl = [torch.full((B,), pos + t, dtype=torch.int32, device=dev) for t in range(n)]
    q1, kv1 = [q[:, t].contiguous() for t in range(n)], [kvn[:, t].contiguous() for t in range(n)]
    o1 = torch.empty(B, H, 512, device=dev, dtype=dt)

    def singles():
        for t in range(n):
            sfa.flash_decode_mla(q1[t], kv1[t], cache, sl[t], o1, idx_layer=0, **kw)
    return lambda: sfa.flash_decode_mla_chunk(q, kvn, cache, sl[0], o, idx_layer=0, num_splits=splits, **kw), singles


def iters_for(B, pos):
    return max(5, min(100, int(2e9 / (B * pos * 2.0 * ROW))))


def sweep():
    a = torch.randn(8192, 8192, device=dev).to(dt)
    bt = torch.randn(8192, 8192, device=dev).to(dt).t()
    (us, spread), = five([lambda: torch.matmul(a, bt)], 20)
    print(f"gemm_calibration torch.matmul bf16 8192^3: {2.0 * 8192 ** 3 / us / 1e6:7.1f} TFLOP/s (5 runs spread {spread:.1f} us)",
          flush=True)
    del a, bt
    for H, Bs, ns in ((16, (64, 256), (1, 2, 4, 8)), (128, (4, 32), (1, 2, 4))):
        for pos in (4095, 32767):
            for B in Bs:
                for layout in ("blmhd", "paged"):
                    for n in ns:
                        (c, cs), (s, ss) = five(calls(B, H, pos, n, layout), iters_for(B, pos))
                        S = sfa.decode_mla_chunk_auto_splits(B, H, pos + 1 + PS, n)
                        tfl = B * n * H * pos * 2.0 * (ROW + 512) / c / 1e6
                        verdict = "faster" if c + cs + ss < s else "slower" if s + cs + ss < c else "within the spreads"
                        print(f"B={B:3d} H={H:3d} pos={pos:5d} {layout:5s} n={n} S={S:2d}: chunk {c:8.1f} us (spread {cs:.1f}) "
                              f"{tfl:6.1f} TFLOP/s | {n} single calls {s:8.1f} us (spread {ss:.1f}) | chunk / singles "
                              f"{c / s:4.2f} ({verdict}), chunk / one single {c / (s / n):4.2f}", flush=True)
                        torch.cuda.empty_cache()
    sfa.check_decode_status()


def splits():
    for pos in (4095, 32767):
        for B, H, n in ((64, 16, 4), (4, 128, 2)):
            auto = sfa.decode_mla_chunk_auto_splits(B, H, pos + 1 + PS, n)
            for S in (1, 2, 4, 8, 16, 32):
                (us, spread), = five(calls(B, H, pos, n, "blmhd", S)[:1], iters_for(B, pos))
                print(f"splits B={B:3d} H={H:3d} n={n} pos={pos:5d} S={S:2d}{' = auto' if S == auto else '       '}: "
                      f"{us:8.1f} us (spread {spread:.1f})", flush=True)
                torch.cuda.empty_cache()


if __name__ == "__main__":
    splits() if "--splits" in sys.argv else sweep()
