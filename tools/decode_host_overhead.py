#!/usr/bin/env python3
"""Host wall time per decode call: what Python and the C ABI spend between the operator's `def` and the launch.

  python tools/decode_host_overhead.py [--root DIR] [--calls 3000] [--warmup 500] [--repeats 5]

Times flash_decode (the plainest of the 18 operators, what bench.py's decode lines run) and
flash_decode_varlen_kv8_window_sinks (the one with every extra argument) on the smallest shapes they accept, so the kernels
are a few microseconds and the host is the bottleneck.  The timed loop does not synchronise: it is `calls` back-to-back
operator calls between two synchronisations, wall time / calls.  One JSON line per operator: microseconds per call of
each repeat, their median, minimum and maximum.  --root: import starflashattention_amd from another checkout (an A/B of
two commits runs this script once per commit, alternating, in fresh processes)."""
import argparse
import json
import os
import statistics
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--calls", type=int, default=3000)
    ap.add_argument("--warmup", type=int, default=500)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--tag", default="")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    import starflashattention_amd as sfa

    dev = torch.device("cuda:0")
    B, H, D, L, M = 1, 1, 64, 1, 64
    f16 = dict(dtype=torch.float16, device=dev)
    seq_len = torch.zeros(B, dtype=torch.int32, device=dev)
    qkv, o = torch.zeros(B, 3, H, D, **f16), torch.zeros(B, H, D, **f16)
    kc, vc = torch.zeros(B, L, M, H, D, **f16), torch.zeros(B, L, M, H, D, **f16)
    kc8, vc8 = torch.zeros(B, L, M, H, D, dtype=torch.uint8, device=dev), torch.zeros(B, L, M, H, D, dtype=torch.uint8, device=dev)
    cu = torch.tensor([0, 1], dtype=torch.int32, device=dev)
    sinks, scale = torch.zeros(H, dtype=torch.float32, device=dev), torch.ones(H, dtype=torch.float32, device=dev)
    ops = {
        "flash_decode": lambda: sfa.flash_decode(qkv, None, None, None, kc, vc, seq_len, o, B, M, H, D, 0, M, L, 0),
        "flash_decode_varlen_kv8_window_sinks": lambda: sfa.flash_decode_varlen_kv8_window_sinks(
            qkv, None, None, None, kc8, vc8, seq_len, o, cu, B, M, H, D, 0, M, L, 0, 8, sinks, k_scale=scale, v_scale=scale),
    }
    for name, call in ops.items():
        for _ in range(args.warmup):
            call()
        torch.cuda.synchronize()
        us = []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            for _ in range(args.calls):
                call()
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            us.append((t1 - t0) / args.calls * 1e6)
        sfa.check_decode_status(dev)
        print(json.dumps({"tag": args.tag, "op": name, "calls": args.calls, "us_per_call": [round(u, 3) for u in us],
                          "median_us": round(statistics.median(us), 3), "min_us": round(min(us), 3),
                          "max_us": round(max(us), 3)}), flush=True)


if __name__ == "__main__":
    main()
