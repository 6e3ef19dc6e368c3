#!/usr/bin/env python3
"""sfa_decode_chunk_kv8 / sfa_decode_varlen_kv8 timings beside the calls they are compared with, in the same process on the
same device (profiles/decode_chunk_kv8_sweep.txt).  HIP events around back-to-back calls after a warm-up; the compared
calls alternate, five timed windows each; the figure is the best of the five with the spread (max - min) / min.  bf16,
head_dim 128.  The fp8 cache is the 16-bit cache of the line, quantised with scale = amax / 448 per kv head.

  (i)   verify (memory-bound): B = 64, H = 32, Hkv in {32, 4}, pos = 4095, n in {1, 8}, blmhd / blhmd / paged 16:
        flash_decode_chunk_kv8 against flash_decode_chunk on the 16-bit cache.  Bytes halve, so 0.5x is the ceiling; the
        bar is that the fp8 call is faster by more than the 16-bit call's own spread.
  (ii)  prompt and chunked prefill (compute-bound): B = 4, H = 32, pos = 0 with n = 2048 and pos = 3584 with n = 512,
        against the flow the call replaces -- flash_decode_chunk on a 16-bit staging layer plus quantize_kv8 of the new K
        and V rows of every sequence -- and against the 16-bit chunk call alone.  The bar: not slower than the flow beyond
        its spread.
  (iii) varlen: 1 x 2048 tokens at pos 2048 + 63 x 1 at pos 4095, B = 64, H = 32, blhmd, M = 8192, against
        flash_decode_varlen on the 16-bit cache.  Recorded only.
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
    """-> (k16, v16, k8, v8, k_scale, v_scale, keyword arguments): N(0,1) 16-bit caches of one layer and their e4m3 copies"""
    kw = dict(kv_layout=layout, num_heads_kv=Hkv)
    if layout == "paged":
        P = M // PS
        shape, axis = (B * P, 1, PS, Hkv, D), 3
        kw["block_table"] = torch.randperm(B * P, device=dev, dtype=torch.int32).view(B, P)
    elif layout == "blhmd":
        shape, axis = (B, 1, Hkv, M, D), 2
    else:
        shape, axis = (B, 1, M, Hkv, D), 3
    out = []
    for _ in range(2):
        c = torch.empty(shape, device=dev, dtype=dt).normal_()
        scale = torch.zeros(Hkv, device=dev)
        step = 4096 if layout == "paged" else 8
        for i in range(0, shape[0], step):                      # amax per kv head, a slab at a time
            scale = torch.maximum(scale, c[i:i + step].abs().movedim(axis, 0).flatten(1).amax(dim=1).float())
        scale = (scale / 448.0).contiguous()
        c8 = torch.empty(shape, dtype=torch.uint8, device=dev)
        if layout == "blhmd":
            for b in range(B):
                sfa.quantize_kv8(c[b, 0].permute(1, 0, 2), scale, out=c8[b, 0].permute(1, 0, 2))
        else:
            sfa.quantize_kv8(c.view(-1, Hkv, D), scale, out=c8.view(-1, Hkv, D))
        out.append((c, c8, scale))
    (k16, k8, ks), (v16, v8, vs) = out
    return k16, v16, k8, v8, ks, vs, kw


def chunk_pair(B, H, Hkv, M, n, pos, layout):
    """(flash_decode_chunk_kv8, flash_decode_chunk) on caches of the same shape, and what the staging flow needs"""
    k16, v16, k8, v8, ks, vs, kw = caches(B, M, Hkv, layout)
    z = torch.zeros(0, dtype=dt, device=dev)
    qkv = torch.randn((B, n, 3, H, D) if H == Hkv else (B, n, H + 2 * Hkv, D), device=dev).to(dt)
    o = torch.empty(B, n, H, D, device=dev, dtype=dt)
    sl = torch.full((B,), pos, dtype=torch.int32, device=dev)
    f8 = lambda: sfa.flash_decode_chunk_kv8(qkv, z, z, z, k8, v8, sl, o, B, M, H, D, D, M, 1, 0, k_scale=ks, v_scale=vs, **kw)
    f16 = lambda: sfa.flash_decode_chunk(qkv, z, z, z, k16, v16, sl, o, B, M, H, D, D, M, 1, 0, **kw)
    return f8, f16, (k16, v16, k8, v8, ks, vs)


def verify():
    B, H, M, pos = (64, 32, 4096 + 64, 4095) if not SMALL else (4, 8, 512 + 64, 511)
    for Hkv in (H, H // 8):
        for layout in ("blmhd", "blhmd", "paged"):
            for n in (1, 8):
                f8, f16, _ = chunk_pair(B, H, Hkv, M, n, pos, layout)
                t8, t16 = timed([f8, f16], 20)
                sfa.check_decode_status()
                rows = 2.0 * B * Hkv * D * (pos + n)            # cache elements a call reads
                verdict = "FASTER" if t16[0] - t8[0] > t16[0] * t16[1] else "not faster beyond the 16-bit call's spread"
                print(f"(i) verify B={B} H={H} Hkv={Hkv} pos={pos} n={n} {layout}{PS if layout == 'paged' else ''}: "
                      f"chunk_kv8 {fmt(t8)} {rows / t8[0] / 1e6:5.2f} TB/s | chunk 16-bit {fmt(t16)} "
                      f"{2 * rows / t16[0] / 1e6:5.2f} TB/s | kv8 / 16-bit {t8[0] / t16[0]:4.2f}x: {verdict}", flush=True)
                del f8, f16
                torch.cuda.empty_cache()


def prefill():
    B, H, M = (4, 32, 4096) if not SMALL else (2, 8, 512)
    shapes = ((0, 2048), (3584, 512)) if not SMALL else ((0, 256), (384, 128))
    for layout, Hkv in (("blhmd", H), ("blmhd", H // 8)):
        for pos, n in shapes:
            f8, f16, (k16, v16, k8, v8, ks, vs) = chunk_pair(B, H, Hkv, M, n, pos, layout)
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
            keys = sum(pos + t + 1 for t in range(n))
            verdict = "no slower" if t8[0] <= tf[0] * (1 + tf[1]) else "SLOWER"
            print(f"(ii) prefill B={B} H={H} Hkv={Hkv} pos={pos} n={n} {layout}: chunk_kv8 {fmt(t8)} "
                  f"{4.0 * D * B * H * keys / t8[0] / 1e6:6.0f} TFLOPS of visible keys | staging flow (chunk 16-bit + "
                  f"{2 * B} quantize_kv8) {fmt(tf)} | chunk 16-bit alone {fmt(t16)} | kv8 / flow {t8[0] / tf[0]:4.2f}: "
                  f"{verdict} than the flow beyond its spread | kv8 / chunk 16-bit {t8[0] / t16[0]:4.2f}", flush=True)
            del f8, f16, flow
            torch.cuda.empty_cache()


def varlen():
    B, H, M, long_n, long_pos = (64, 32, 8192, 2048, 2048) if not SMALL else (8, 8, 1024, 128, 128)
    short_pos = M // 2 - 1
    k16, v16, k8, v8, ks, vs, kw = caches(B, M, H, "blhmd")
    T = long_n + B - 1
    z = torch.zeros(0, dtype=dt, device=dev)
    qkv = torch.randn(T, 3, H, D, device=dev).to(dt)
    o = torch.empty(T, H, D, device=dev, dtype=dt)
    sl = torch.tensor([long_pos] + [short_pos] * (B - 1), dtype=torch.int32, device=dev)
    cu = torch.tensor([0] + [long_n + i for i in range(B)], dtype=torch.int32, device=dev)
    f8 = lambda: sfa.flash_decode_varlen_kv8(qkv, z, z, z, k8, v8, sl, o, cu, B, M, H, D, D, M, 1, 0, k_scale=ks,
                                             v_scale=vs, **kw)
    f16 = lambda: sfa.flash_decode_varlen(qkv, z, z, z, k16, v16, sl, o, cu, B, M, H, D, D, M, 1, 0, **kw)
    t8, t16 = timed([f8, f16], 10)
    sfa.check_decode_status()
    print(f"(iii) varlen B={B} H={H} blhmd M={M}: 1 x {long_n} tokens at {long_pos} + {B - 1} x 1 at {short_pos}: "
          f"varlen_kv8 {fmt(t8)} | varlen 16-bit {fmt(t16)} | kv8 / 16-bit {t8[0] / t16[0]:4.2f}", flush=True)


if __name__ == "__main__":
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    verify()
    prefill()
    varlen()
