#!/usr/bin/env python3
"""sfa_decode_chunk timings (HIP events over back-to-back calls after a warm-up), one line per shape:
  * speculative verify (HBM-bound): B=64, H=32, D=128, pos=4095, n in {1,2,4,8,16}; GB/s against the cache bytes read;
    against one flash_decode call and n flash_decode calls on the same cache
  * prompt ingestion / chunked prefill / grouped paged (MFMA-bound): TFLOPS of the causal FLOPs; against
    flash_attn_fwd on the equivalent contiguous causal problem."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import starflashattention_amd as sfa

dev = torch.device("cuda:0")


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


def spec_verify():
    B, H, D, M, pos, dt = 64, 32, 128, 4096 + 16, 4095, torch.bfloat16
    kc = torch.randn(B, 1, M, H, D, device=dev, dtype=dt)
    vc = torch.randn_like(kc)
    sl = torch.full((B,), pos, dtype=torch.int32, device=dev)
    z = torch.zeros(0, dtype=dt, device=dev)
    q1 = torch.randn(B, 3, H, D, device=dev, dtype=dt)
    o1 = torch.empty(B, H, D, device=dev, dtype=dt)
    dec = lambda: sfa.flash_decode(q1, z, z, z, kc, vc, sl, o1, B, M, H, D, D, M, 1, 0)
    t_dec = timed(dec, 50)
    for n in (1, 2, 4, 8, 16):
        qkv = torch.randn(B, n, 3, H, D, device=dev, dtype=dt)
        o = torch.empty(B, n, H, D, device=dev, dtype=dt)
        t = timed(lambda: sfa.flash_decode_chunk(qkv, z, z, z, kc, vc, sl, o, B, M, H, D, D, M, 1, 0), 50)
        gb = 2 * B * (pos + n) * H * D * 2 / 1e9
        print(f"verify B={B} H={H} D={D} pos={pos} n={n:2d} bf16 blmhd: chunk {t:7.1f} us {gb / t * 1e6:6.0f} GB/s | "
              f"1 decode {t_dec:6.1f} us | {n} decodes {n * t_dec:7.1f} us | chunk / 1 decode {t / t_dec:4.2f}x",
              flush=True)


def prefill_like(B, H, Hkv, D, pos, n, layout, page_size=16):
    dt = torch.bfloat16
    M = pos + n
    G = H // Hkv
    z = torch.zeros(0, dtype=dt, device=dev)
    kw = dict(kv_layout=layout)
    if Hkv != H:
        kw["num_heads_kv"] = Hkv
    if layout == "paged":
        P = M // page_size
        kc = torch.randn(B * P, 1, page_size, Hkv, D, device=dev, dtype=dt)
        kw["block_table"] = torch.randperm(B * P, device=dev, dtype=torch.int32).view(B, P)
    elif layout == "blhmd":
        kc = torch.randn(B, 1, Hkv, M, D, device=dev, dtype=dt)
    else:
        kc = torch.randn(B, 1, M, Hkv, D, device=dev, dtype=dt)
    vc = torch.randn_like(kc)
    qkv = torch.randn(B, n, 3, H, D, device=dev, dtype=dt) if G == 1 else torch.randn(B, n, H + 2 * Hkv, D, device=dev, dtype=dt)
    o = torch.empty(B, n, H, D, device=dev, dtype=dt)
    sl = torch.full((B,), pos, dtype=torch.int32, device=dev)
    t = timed(lambda: sfa.flash_decode_chunk(qkv, z, z, z, kc, vc, sl, o, B, M, H, D, D, M, 1, 0, **kw), 10)
    # causal FLOPs: 4*D per (query, visible key); query t sees pos + t + 1 keys
    flops = 4.0 * D * B * H * (n * pos + n * (n + 1) / 2)
    q = torch.randn(B, H, n, D, device=dev, dtype=dt)
    k = torch.randn(B, Hkv, M, D, device=dev, dtype=dt)
    v = torch.randn_like(k)
    t_ref = timed(lambda: sfa.flash_attn_fwd(q, k, v, causal=True), 10)
    print(f"chunk B={B} H={H} Hkv={Hkv} D={D} pos={pos} n={n} bf16 {layout}{page_size if layout == 'paged' else ''}: "
          f"{t:8.1f} us {flops / t / 1e6:6.0f} TFLOPS | flash_attn_fwd causal {t_ref:8.1f} us "
          f"{flops / t_ref / 1e6:6.0f} TFLOPS | ratio {t_ref / t:4.2f}", flush=True)


if __name__ == "__main__":
    if "--prompt-only" in sys.argv:         # one prompt shape, for a kernel trace (rocprofv3 --kernel-trace --stats)
        prefill_like(4, 32, 32, 128, 0, 2048, "blhmd")
        sys.exit(0)
    spec_verify()
    for n in (512, 2048, 4096):
        for layout in ("blhmd", "blmhd"):
            prefill_like(4, 32, 32, 128, 0, n, layout)
    prefill_like(4, 32, 32, 128, 3584, 512, "blhmd")
    prefill_like(4, 32, 4, 128, 0, 2048, "paged", 16)
    prefill_like(4, 32, 4, 128, 3584, 512, "paged", 16)
