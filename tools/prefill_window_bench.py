#!/usr/bin/env python3
"""sfa_prefill_window_fwd timings (HIP events over back-to-back calls after a warm-up; five runs, interleaved with the
calls they are compared with, in one process on one device; the median and the five-run spread), bf16:
  * gpt-oss: B = 4, Hq = 64, Hkv = 8, D = 64, S = 4096 / 8192 / 32768, window 128, with sinks
  * B = 4, Hq = 32, Hkv = 8, D = 128, S = 8192, windows 1024 and 4096, with sinks
  * the gpt-oss shape at S = 8192 with window = INT_MAX and sinks: full causal attention on the windowed kernel
  * chunked: the gpt-oss heads, Sq = 512 against Sk = 4096, window 128, with sinks
Per line:
  new      flash_attn_window_fwd
  causal   flash_attn_fwd(causal=True) under the library's own choice of kernel (what a caller without the window pays)
  8w       the same under prefill_impl = 10, the 8-wave exact kernel whose tile pipeline the new kernel is built from
  chunk    flash_decode_chunk_window_sinks at pos = Sk - Sq with n = Sq over a contiguous cache: the only route to the same
           attention before this call existed (it also rotates and appends)
  r        key tiles walked by the new call's workgroups / key tiles walked by the 8-wave causal kernel's workgroups
           (from the shapes; both kernels walk 64-key tiles under 256-row q-tiles)
Expectation (recorded, not a gate): new = r x 8w within new's own spread; a line over that prints OVER with the excess.
Gates: at the gpt-oss shape with S = 8192 new is faster than causal; at S = 32768 new < 4 x new(8192) + spread.
  --small   the first two gpt-oss lines only"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import starflashattention_amd as sfa

dev = torch.device("cuda:0")
dt = torch.bfloat16
INT_MAX = 2 ** 31 - 1
BM, BN = 256, 64


def timed(fn, iters):
    for _ in range(2):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3          # us


def tile_steps(Sq, Sk, window):
    """(new, causal): key tiles the workgroups of one head walk"""
    coff = Sk - Sq
    new = causal = 0
    for q0 in range(0, Sq, BM):
        last = min(q0 + BM, Sq) - 1 + coff
        if last < 0:
            continue
        end = last // BN + 1
        causal += end
        new += end - max(0, q0 + coff + 1 - min(window, Sk)) // BN
    return new, causal


def med(xs):
    return statistics.median(xs), max(xs) - min(xs)


def line(name, B, Hq, Hkv, D, Sq, Sk, window, iters):
    q = torch.randn(B, Hq, Sq, D, device=dev).to(dt)
    k = torch.randn(B, Hkv, Sk, D, device=dev).to(dt)
    v = torch.randn(B, Hkv, Sk, D, device=dev).to(dt)
    sinks = torch.randn(Hq, device=dev)
    out = torch.empty_like(q)
    new = lambda: sfa.flash_attn_window_fwd(q, k, v, window, sinks=sinks, out=out)
    causal = lambda: sfa.flash_attn_fwd(q, k, v, causal=True, out=out)

    def eight():
        sfa.debug_set("prefill_impl", 10)
        try:
            return timed(causal, iters)
        finally:
            sfa.debug_set("prefill_impl", -1)

    # the chunk call: the keys [0, Sk - Sq) are in the cache, the Sq new tokens arrive packed [B, n, Hq + 2 Hkv, D]
    chunk = None
    try:
        z = torch.zeros(0, dtype=dt, device=dev)
        kc = torch.randn(B, 1, Hkv, Sk, D, device=dev).to(dt)
        vc = torch.randn(B, 1, Hkv, Sk, D, device=dev).to(dt)
        qkv = torch.randn(B, Sq, Hq + 2 * Hkv, D, device=dev).to(dt)
        oc = torch.empty(B, Sq, Hq, D, device=dev, dtype=dt)
        sl = torch.full((B,), Sk - Sq, dtype=torch.int32, device=dev)
        chunk = lambda: sfa.flash_decode_chunk_window_sinks(qkv, z, z, z, kc, vc, sl, oc, B, Sk, Hq, D, D, Sk, 1, 0, window,
                                                            sinks, kv_layout="blhmd", num_heads_kv=Hkv)
        chunk()
        torch.cuda.synchronize()
        sfa.check_decode_status()
    except (RuntimeError, sfa.SfaError) as e:
        chunk, why = None, str(e).splitlines()[0][:80]
    tn, tc, t8, tk = [], [], [], []
    for _ in range(5):
        tn.append(timed(new, iters))
        tc.append(timed(causal, iters))
        t8.append(eight())
        if chunk:
            tk.append(timed(chunk, max(1, iters // 2)))
    kern = sfa.last_prefill_kernel()
    (n, sn), (c, sc), (e, se) = med(tn), med(tc), med(t8)
    steps_new, steps_causal = tile_steps(Sq, Sk, window)
    r = steps_new / steps_causal
    want = r * e
    verdict = "MET" if n <= want + sn else f"OVER by {n - want:.1f} us ({(n / want - 1) * 100:.0f} %)"
    ck = f"{med(tk)[0]:9.1f} us (spread {med(tk)[1]:.1f})" if chunk else f"n/a ({why})"
    w = "INT_MAX" if window == INT_MAX else str(window)
    print(f"{name}: B={B} Hq={Hq} Hkv={Hkv} D={D} Sq={Sq} Sk={Sk} window={w} bf16 | new {n:9.1f} us (spread {sn:.1f}) | "
          f"causal [{kern}] {c:9.1f} us (spread {sc:.1f}) | 8w exact {e:9.1f} us (spread {se:.1f}) | chunk_window_sinks {ck} | "
          f"r = {steps_new}/{steps_causal} = {r:.4f}, r x 8w = {want:.1f} us: {verdict} | new / causal {n / c:.3f}", flush=True)
    return n, sn, c


if __name__ == "__main__":
    small = "--small" in sys.argv
    g = dict(B=4, Hq=64, Hkv=8, D=64)
    line("gpt-oss", **g, Sq=4096, Sk=4096, window=128, iters=20)
    n8, s8, c8 = line("gpt-oss", **g, Sq=8192, Sk=8192, window=128, iters=10)
    print(f"GATE new < causal at S=8192: {n8:.1f} < {c8:.1f} us: {'HOLDS' if n8 < c8 else 'FAILS'}", flush=True)
    if not small:
        n32, s32, _ = line("gpt-oss", **g, Sq=32768, Sk=32768, window=128, iters=2)
        print(f"GATE linear in S: new(32768) {n32:.1f} < 4 x new(8192) + spread = {4 * n8 + s32:.1f} us: "
              f"{'HOLDS' if n32 < 4 * n8 + s32 else 'FAILS'}", flush=True)
        torch.cuda.empty_cache()
        line("d128", B=4, Hq=32, Hkv=8, D=128, Sq=8192, Sk=8192, window=1024, iters=10)
        line("d128", B=4, Hq=32, Hkv=8, D=128, Sq=8192, Sk=8192, window=4096, iters=10)
        line("full+sinks", **g, Sq=8192, Sk=8192, window=INT_MAX, iters=10)
        line("chunked", **g, Sq=512, Sk=4096, window=128, iters=20)
