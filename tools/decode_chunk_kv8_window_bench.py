#!/usr/bin/env python3
"""sfa_decode_chunk_kv8_window / sfa_decode_varlen_kv8_window timings beside the calls they are compared with, in the same
process on the same device (profiles/decode_chunk_kv8_window_sweep.txt).  HIP events around back-to-back calls after a
warm-up; the compared calls alternate, five timed windows each; the figure is the best of the five with the spread
(max - min) / min.  bf16, head_dim 128.  The fp8 cache is the 16-bit cache of the line, quantised with one scale per kv
head.

  (i)   verify (memory-bound): B = 64, H = 32, Hkv in {32, 4}, n in {1, 8}, blmhd / blhmd / paged 16, window = 4096 at
        pos = 32767:
        same bytes   against flash_decode_chunk_kv8 at pos = 4095 (the same rows per sequence, no window).  Expectation:
                     inside that call's own spread; a line outside it is a miss, recorded with its size.
        16 bit       against flash_decode_chunk_window on the 16-bit cache, the same window and pos.  Bytes halve, so 0.5x
                     is the ceiling; the bar is that the fp8 call is faster by more than the 16-bit call's own spread.
  (ii)  prompt: B = 4, H = 32, n = 2048 at pos = 0, window = 1024, against the flow the call replaces --
        flash_decode_chunk_window on a 16-bit staging layer plus quantize_kv8 of the new K and V rows of every sequence.
        The bar: not slower than the flow beyond its spread.
  (iii) varlen: 1 x 2048 tokens at pos 2048 + 63 x 1 at pos 4095, B = 64, H = 32, blhmd, M = 8192, window = 4096, beside
        flash_decode_varlen_window on the 16-bit cache and flash_decode_varlen_kv8 (no window).  Recorded only.
--small: the same lines at toy sizes (a rehearsal of the script, not a measurement)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import starflashattention_amd as sfa

dev = torch.device("cuda:0")
dt = torch.bfloat16
D = 128
PS = 16
SMALL = "--small" in sys.argv


def timed(fns, iters):
    """[(best, spread)] per function: five timed windows of `iters` back-to-back calls each, the functions alternating;
    in us per call"""
    for fn in fns:
        for _ in range(3):
            fn()
    ts = [[] for _ in fns]
    for _ in range(5):
        for i, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ts[i].append(e0.elapsed_time(e1) / iters * 1e3)
    return [(min(t), (max(t) - min(t)) / min(t)) for t in ts]


def fmt(t):
    return f"{t[0]:9.1f} us (+{100 * t[1]:4.1f} %)"


def caches(B, M, Hkv, layout):
    """-> (k16, v16, k8, v8, k_scale, v_scale, keyword arguments): N(0,1) 16-bit caches of one layer and their e4m3 copies
    (one scale for all kv heads, 6 / 448: N(0,1) values beyond six sigma saturate, which no timing notices)"""
    kw = dict(kv_layout=layout, num_heads_kv=Hkv)
    if layout == "paged":
        P = M // PS
        shape = (B * P, 1, PS, Hkv, D)
        kw["block_table"] = torch.randperm(B * P, device=dev, dtype=torch.int32).view(B, P)
    elif layout == "blhmd":
        shape = (B, 1, Hkv, M, D)
    else:
        shape = (B, 1, M, Hkv, D)
    scale = torch.full((Hkv,), 6.0 / 448.0, device=dev)
    out = []
    for _ in range(2):
        c = torch.empty(shape, device=dev, dtype=dt).normal_()
        c8 = torch.empty(shape, dtype=torch.uint8, device=dev)
        if layout == "blhmd":
            for b in range(B):
                sfa.quantize_kv8(c[b, 0].permute(1, 0, 2), scale, out=c8[b, 0].permute(1, 0, 2))
        else:
            sfa.quantize_kv8(c.view(-1, Hkv, D), scale, out=c8.view(-1, Hkv, D))
        out.append((c, c8))
    (k16, k8), (v16, v8) = out
    return k16, v16, k8, v8, scale, scale.clone(), kw


def chunk_calls(B, H, Hkv, M, n, layout):
    """call(kind, pos, window) -> a closure making one call on caches of the same shape; kind: "kv8_window", "kv8",
    "window" (16 bit); and the tensors the staging flow needs"""
    k16, v16, k8, v8, ks, vs, kw = caches(B, M, Hkv, layout)
    z = torch.zeros(0, dtype=dt, device=dev)
    qkv = torch.randn((B, n, 3, H, D) if H == Hkv else (B, n, H + 2 * Hkv, D), device=dev).to(dt)
    o = torch.empty(B, n, H, D, device=dev, dtype=dt)

    def call(kind, pos, window=None):
        sl = torch.full((B,), pos, dtype=torch.int32, device=dev)
        if kind == "kv8_window":
            return lambda: sfa.flash_decode_chunk_kv8_window(qkv, z, z, z, k8, v8, sl, o, B, M, H, D, D, M, 1, 0, window,
                                                             k_scale=ks, v_scale=vs, **kw)
        if kind == "kv8":
            return lambda: sfa.flash_decode_chunk_kv8(qkv, z, z, z, k8, v8, sl, o, B, M, H, D, D, M, 1, 0, k_scale=ks,
                                                      v_scale=vs, **kw)
        return lambda: sfa.flash_decode_chunk_window(qkv, z, z, z, k16, v16, sl, o, B, M, H, D, D, M, 1, 0, window, **kw)
    return call, (k16, v16, k8, v8, ks, vs)


def verify():
    B, H, W, pos = (64, 32, 4096, 32767) if not SMALL else (4, 8, 512, 2047)
    M = pos + 1 + 64
    for Hkv in (H, H // 8):
        for layout in ("blmhd", "blhmd", "paged"):
            for n in (1, 8):
                call, _ = chunk_calls(B, H, Hkv, M, n, layout)
                t8w, t8, t16w = timed([call("kv8_window", pos, W), call("kv8", W - 1), call("window", pos, W)], 20)
                sfa.check_decode_status()
                rows = 2.0 * B * Hkv * D * (W - 1 + n)          # cache elements a call reads
                miss = abs(t8w[0] - t8[0]) - t8[0] * t8[1]
                same = "inside its spread" if miss <= 0 else f"MISS by {100 * miss / t8[0]:.1f} % beyond its spread"
                faster = "FASTER" if t16w[0] - t8w[0] > t16w[0] * t16w[1] else "not faster beyond the 16-bit call's spread"
                print(f"(i) verify B={B} H={H} Hkv={Hkv} n={n} {layout}{PS if layout == 'paged' else ''} window={W} "
                      f"pos={pos}: chunk_kv8_window {fmt(t8w)} {rows / t8w[0] / 1e6:5.2f} TB/s | chunk_kv8 at pos={W - 1} "
                      f"{fmt(t8)} window / full {t8w[0] / t8[0]:4.2f}x: {same} | chunk_window 16-bit {fmt(t16w)} "
                      f"{2 * rows / t16w[0] / 1e6:5.2f} TB/s kv8 / 16-bit {t8w[0] / t16w[0]:4.2f}x: {faster}", flush=True)
                del call
                torch.cuda.empty_cache()


def prefill():
    B, H, M, n, W = (4, 32, 4096, 2048, 1024) if not SMALL else (2, 8, 512, 256, 128)
    pos = 0
    for layout, Hkv in (("blhmd", H), ("blmhd", H // 8)):
        call, (k16, v16, k8, v8, ks, vs) = chunk_calls(B, H, Hkv, M, n, layout)
        f8, f16 = call("kv8_window", pos, W), call("window", pos, W)
        if layout == "blhmd":
            rows = lambda c, b: c[b, 0, :, pos:pos + n].permute(1, 0, 2)
        else:
            rows = lambda c, b: c[b, 0, pos:pos + n]

        def flow():     # the staging flow: the 16-bit call (k16 / v16 as the staging layer), then the new rows -> fp8
            f16()
            for b in range(B):
                sfa.quantize_kv8(rows(k16, b), ks, out=rows(k8, b))
                sfa.quantize_kv8(rows(v16, b), vs, out=rows(v8, b))

        t8, tf, t16 = timed([f8, flow, f16], 10)
        sfa.check_decode_status()
        keys = sum(min(pos + t + 1, W) for t in range(n))
        verdict = "no slower" if t8[0] <= tf[0] * (1 + tf[1]) else "SLOWER"
        print(f"(ii) prompt B={B} H={H} Hkv={Hkv} pos={pos} n={n} window={W} {layout}: chunk_kv8_window {fmt(t8)} "
              f"{4.0 * D * B * H * keys / t8[0] / 1e6:6.0f} TFLOPS of visible keys | staging flow (chunk_window 16-bit + "
              f"{2 * B} quantize_kv8) {fmt(tf)} | chunk_window 16-bit alone {fmt(t16)} | kv8 / flow {t8[0] / tf[0]:4.2f}: "
              f"{verdict} than the flow beyond its spread | kv8 / chunk_window 16-bit {t8[0] / t16[0]:4.2f}", flush=True)
        del f8, f16, flow, call
        torch.cuda.empty_cache()


def varlen():
    B, H, M, long_n, long_pos, W = (64, 32, 8192, 2048, 2048, 4096) if not SMALL else (8, 8, 1024, 128, 128, 512)
    short_pos = M // 2 - 1
    k16, v16, k8, v8, ks, vs, kw = caches(B, M, H, "blhmd")
    T = long_n + B - 1
    z = torch.zeros(0, dtype=dt, device=dev)
    qkv = torch.randn(T, 3, H, D, device=dev).to(dt)
    o = torch.empty(T, H, D, device=dev, dtype=dt)
    sl = torch.tensor([long_pos] + [short_pos] * (B - 1), dtype=torch.int32, device=dev)
    cu = torch.tensor([0] + [long_n + i for i in range(B)], dtype=torch.int32, device=dev)
    f8w = lambda: sfa.flash_decode_varlen_kv8_window(qkv, z, z, z, k8, v8, sl, o, cu, B, M, H, D, D, M, 1, 0, W, k_scale=ks,
                                                     v_scale=vs, **kw)
    f16w = lambda: sfa.flash_decode_varlen_window(qkv, z, z, z, k16, v16, sl, o, cu, B, M, H, D, D, M, 1, 0, W, **kw)
    f8 = lambda: sfa.flash_decode_varlen_kv8(qkv, z, z, z, k8, v8, sl, o, cu, B, M, H, D, D, M, 1, 0, k_scale=ks,
                                             v_scale=vs, **kw)
    t8w, t16w, t8 = timed([f8w, f16w, f8], 10)
    sfa.check_decode_status()
    print(f"(iii) varlen B={B} H={H} blhmd M={M} window={W}: 1 x {long_n} tokens at {long_pos} + {B - 1} x 1 at "
          f"{short_pos}: varlen_kv8_window {fmt(t8w)} | varlen_window 16-bit {fmt(t16w)} | varlen_kv8 (no window) {fmt(t8)} "
          f"| kv8 window / 16-bit window {t8w[0] / t16w[0]:4.2f} | kv8 window / kv8 {t8w[0] / t8[0]:4.2f}", flush=True)


if __name__ == "__main__":
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    verify()
    prefill()
    varlen()
