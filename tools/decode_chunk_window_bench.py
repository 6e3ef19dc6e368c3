#!/usr/bin/env python3
"""sfa_decode_chunk_window timings against the calls without a window of the same run (profiles/
decode_chunk_window_sweep.txt).  HIP events around back-to-back calls after a warm-up, best of five windows with the
spread (max - min) / min of the five, one process, one device, bf16, head_dim 128.

  (i)   chunked prefill: B = 4, H = 32, M = 32768, pos = 28672, n = 512, window = 4096, blhmd and paged16 with G = 8;
        beside it sfa_decode_chunk at the same pos (the full history) and at pos = 4096, where every row reads at least
        as many keys as the windowed rows do
  (ii)  verify: B = 64, H = 32, pos = 32767 - 8, n = 8, window = 4096; beside it one sfa_decode_window call and eight
  (iii) small window: G = 1, n = 2048, pos = 0, window 128 and 1024; beside it sfa_decode_chunk
--small: the same lines at toy sizes (a rehearsal of the script, not a measurement)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import starflashattention_amd as sfa

dev = torch.device("cuda:0")
dt = torch.bfloat16
D = 128
SMALL = "--small" in sys.argv


def timed(fn, iters):
    """(best, spread) of five timed windows of `iters` back-to-back calls, in us per call"""
    for _ in range(3):
        fn()
    ts = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / iters * 1e3)
    return min(ts), (max(ts) - min(ts)) / min(ts)


def fmt(t):
    return f"{t[0]:9.1f} us (+{100 * t[1]:4.1f} %)"


def cache(B, M, Hkv, layout, ps=16):
    kw = dict(kv_layout=layout, num_heads_kv=Hkv)
    if layout == "paged":
        P = M // ps
        kc = torch.randn(B * P, 1, ps, Hkv, D, device=dev, dtype=dt)
        kw["block_table"] = torch.randperm(B * P, device=dev, dtype=torch.int32).view(B, P)
    elif layout == "blhmd":
        kc = torch.randn(B, 1, Hkv, M, D, device=dev, dtype=dt)
    else:
        kc = torch.randn(B, 1, M, Hkv, D, device=dev, dtype=dt)
    return kc, torch.randn_like(kc), kw


def chunk_calls(B, H, Hkv, M, n, layout):
    """(chunk(pos), chunk_window(pos, window), the cache they run on)"""
    kc, vc, kw = cache(B, M, Hkv, layout)
    z = torch.zeros(0, dtype=dt, device=dev)
    qkv = (torch.randn(B, n, 3, H, D, device=dev, dtype=dt) if H == Hkv
           else torch.randn(B, n, H + 2 * Hkv, D, device=dev, dtype=dt))
    o = torch.empty(B, n, H, D, device=dev, dtype=dt)

    def plain(pos):
        sl = torch.full((B,), pos, dtype=torch.int32, device=dev)
        return lambda: sfa.flash_decode_chunk(qkv, z, z, z, kc, vc, sl, o, B, M, H, D, D, M, 1, 0, **kw)

    def windowed(pos, window):
        sl = torch.full((B,), pos, dtype=torch.int32, device=dev)
        return lambda: sfa.flash_decode_chunk_window(qkv, z, z, z, kc, vc, sl, o, B, M, H, D, D, M, 1, 0, window, **kw)

    return plain, windowed, (kc, vc, kw)


def chunked_prefill():
    B, H, M, pos, n, window = (4, 32, 32768, 28672, 512, 4096) if not SMALL else (2, 8, 2048, 1024, 64, 256)
    for layout, Hkv in (("blhmd", H), ("paged", H // 8)):
        plain, windowed, _ = chunk_calls(B, H, Hkv, M, n, layout)
        tw, tf, ts = timed(windowed(pos, window), 10), timed(plain(pos), 5), timed(plain(window), 10)
        verdict = "no slower" if tw[0] <= ts[0] * (1 + tw[1] + ts[1]) else "SLOWER"
        print(f"(i) prefill B={B} H={H} Hkv={Hkv} pos={pos} n={n} window={window} {layout}: window {fmt(tw)} | "
              f"chunk at pos (full history) {fmt(tf)} | chunk at pos={window} {fmt(ts)} | window / chunk(pos={window}) "
              f"{tw[0] / ts[0]:4.2f}: {verdict} beyond the two spreads", flush=True)


def verify():
    B, H, M, n, window = (64, 32, 32768, 8, 4096) if not SMALL else (4, 8, 2048, 8, 256)
    pos = M - 1 - n
    for layout in ("blmhd", "paged"):
        plain, windowed, (kc, vc, kw) = chunk_calls(B, H, H, M, n, layout)
        z = torch.zeros(0, dtype=dt, device=dev)
        q1 = torch.randn(B, 3, H, D, device=dev, dtype=dt)
        o1 = torch.empty(B, H, D, device=dev, dtype=dt)
        sl = torch.full((B,), pos, dtype=torch.int32, device=dev)
        one = lambda: sfa.flash_decode_window(q1, z, z, z, kc, vc, sl, o1, B, M, H, D, D, M, 1, 0, window, **kw)

        def eight():
            for _ in range(n):
                one()

        tw, t1, t8, tf = timed(windowed(pos, window), 20), timed(one, 20), timed(eight, 5), timed(plain(pos), 5)
        print(f"(ii) verify B={B} H={H} pos={pos} n={n} window={window} {layout}: chunk_window {fmt(tw)} | 1 decode_window "
              f"{fmt(t1)} | {n} decode_window {fmt(t8)} | chunk (full history) {fmt(tf)} | chunk_window / {n} decode_window "
              f"{tw[0] / t8[0]:4.2f}", flush=True)


def small_window():
    B, H, n = (4, 32, 2048) if not SMALL else (2, 4, 512)
    plain, windowed, _ = chunk_calls(B, H, H, n, n, "blhmd")
    tf = timed(plain(0), 10)
    for window in (128, 1024):
        tw = timed(windowed(0, window), 10)
        # the MFMA work of the windowed rows: 4*D FLOPs per (query, visible key)
        keys = sum(min(t + 1, window) for t in range(n))
        print(f"(iii) small window B={B} H={H} G=1 pos=0 n={n} window={window} blhmd: window {fmt(tw)} "
              f"{4.0 * D * B * H * keys / tw[0] / 1e6:6.0f} TFLOPS of visible keys | chunk (causal) {fmt(tf)} | "
              f"window / chunk {tw[0] / tf[0]:4.2f}", flush=True)


if __name__ == "__main__":
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    if "--prefill-only" in sys.argv:        # one shape, for a kernel trace (rocprofv3 --kernel-trace --stats)
        # the windowed call of (i) and the chunk call at pos = 4096 beside it, paged16 with G = 8: the kernels of the two
        # carry different geometry names, so the trace splits prologue and attention of each
        plain, windowed, _ = chunk_calls(4, 32, 4, 32768, 512, "paged")
        for fn in (windowed(28672, 4096), plain(4096)):
            for _ in range(8):
                fn()
        torch.cuda.synchronize()
        sys.exit(0)
    chunked_prefill()
    verify()
    small_window()
