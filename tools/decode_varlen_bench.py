#!/usr/bin/env python3
"""sfa_decode_varlen timings (HIP events over back-to-back calls after a warm-up), the comparison beside each result:
  * uniform batches (the shapes of profiles/decode_chunk_sweep.txt): flash_decode_varlen against flash_decode_chunk in
    the same process.  The acceptance margin is the chunk call's own spread over five repeats plus the plan kernel's
    duration (PLAN_US: its longest launch in the kernel traces under profiles/, timed separately with rocprofv3
    --kernel-trace --stats; --plan-us overrides).  The cost of a call whose sequences are all idle (plan kernel plus
    launches that exit at once) is printed for information only
  * mixed batch (one 2048-token chunk + 63 decoding sequences; also paged16 with 4 kv heads): against the chunk padded
    to n = 2048 (legal only from memory_max_len 6143 on, so everything runs at 8192) and against two calls, a chunk on
    the long sequence plus flash_decode on the rest
  * empty-heavy grid: B = 256, one n = 4096 sequence and 255 with n = 1; launched workgroups next to the time."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import starflashattention_amd as sfa

dev = torch.device("cuda:0")
dt = torch.bfloat16
PLAN_US = 5.3        # varlen_plan_kernel: the upper end of its launches in profiles/decode_varlen_*_kernel_stats.txt (avg 4.6-4.8)
for _i, _a in enumerate(sys.argv):
    if _a == "--plan-us":
        PLAN_US = float(sys.argv[_i + 1])


def library_splits(B, H, Hkv, D, M, T):
    """The split count the library picks for num_splits = 0, read off its own workspace arithmetic."""
    ws = sfa._lib.load().sfa_decode_varlen_workspace_bytes
    auto = ws(B, H, Hkv, D, M, T, 0)
    return next(s for s in range(1, 33) if ws(B, H, Hkv, D, M, T, s) == auto)


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


def caches(B, Hkv, D, M, layout, page_size=16):
    """-> (k cache, v cache, keyword arguments) with every page / row random."""
    kw = dict(kv_layout=layout)
    if layout == "paged":
        P = M // page_size
        kc = torch.randn(B * P, 1, page_size, Hkv, D, device=dev, dtype=dt)
        kw["block_table"] = torch.randperm(B * P, device=dev, dtype=torch.int32).view(B, P)
    elif layout == "blhmd":
        kc = torch.randn(B, 1, Hkv, M, D, device=dev, dtype=dt)
    else:
        kc = torch.randn(B, 1, M, Hkv, D, device=dev, dtype=dt)
    return kc, torch.randn_like(kc), kw


def i32(x):
    return torch.tensor(x, dtype=torch.int32, device=dev)


def uniform(B, H, Hkv, D, pos, n, layout, iters, M=None):
    M = M or pos + n
    kc, vc, kw = caches(B, Hkv, D, M, layout)
    if Hkv != H:
        kw["num_heads_kv"] = Hkv
    z = torch.zeros(0, dtype=dt, device=dev)
    per_tok = (3, H, D) if Hkv == H else (H + 2 * Hkv, D)
    qkv = torch.randn((B, n) + per_tok, device=dev, dtype=dt)
    o = torch.empty(B, n, H, D, device=dev, dtype=dt)
    sl = torch.full((B,), pos, dtype=torch.int32, device=dev)
    cu = torch.arange(B + 1, dtype=torch.int32, device=dev) * n
    idle = torch.zeros(B + 1, dtype=torch.int32, device=dev)
    chunk = lambda: sfa.flash_decode_chunk(qkv, z, z, z, kc, vc, sl, o, B, M, H, D, D, M, 1, 0, **kw)
    qp, op = qkv.view((B * n,) + per_tok), o.view(B * n, H, D)
    varlen = lambda c=cu: sfa.flash_decode_varlen(qp, z, z, z, kc, vc, sl, op, c, B, M, H, D, D, M, 1, 0, **kw)
    t_chunk = [timed(chunk, iters) for _ in range(5)]
    t_var = [timed(varlen, iters) for _ in range(5)]
    t_idle = timed(lambda: varlen(idle), iters)
    c, v = min(t_chunk), min(t_var)
    spread = max(t_chunk) - c
    verdict = "within" if v - c <= spread + PLAN_US else "OVER"
    print(f"uniform B={B} H={H} Hkv={Hkv} D={D} pos={pos} n={n} bf16 {layout}{16 if layout == 'paged' else ''}: "
          f"varlen {v:8.1f} us (5 runs {min(t_var):.1f}..{max(t_var):.1f}) | chunk {c:8.1f} us (5 runs spread {spread:.1f}) | "
          f"idle call {t_idle:5.1f} us | varlen - chunk {v - c:+7.1f} us, margin {spread:.1f} + plan {PLAN_US:.1f}: {verdict} | "
          f"varlen / chunk {v / c:4.2f}x", flush=True)


def mixed(B, H, Hkv, D, layout, n_long=2048, pos_long=2048, pos_rest=4095, M=8192, pad=True, label="mixed"):
    """Sequence 0 brings n_long tokens at pos_long, the others one token at pos_rest."""
    G = H // Hkv
    kc, vc, kw = caches(B, Hkv, D, M, layout)
    if Hkv != H:
        kw["num_heads_kv"] = Hkv
    z = torch.zeros(0, dtype=dt, device=dev)
    per_tok = (3, H, D) if Hkv == H else (H + 2 * Hkv, D)
    T = n_long + B - 1
    qkv = torch.randn((T,) + per_tok, device=dev, dtype=dt)
    o = torch.empty(T, H, D, device=dev, dtype=dt)
    sl = i32([pos_long] + [pos_rest] * (B - 1))
    cu = i32([0] + [n_long + i for i in range(B)])
    t_var = timed(lambda: sfa.flash_decode_varlen(qkv, z, z, z, kc, vc, sl, o, cu, B, M, H, D, D, M, 1, 0, **kw), 10)
    # the attention grid, computed (not observed): plan slots (the bound documented in csrc/sfa_host.h) x Hkv x S
    S = library_splits(B, H, Hkv, D, M, T)
    wgs = (T * G // 256 + B) * Hkv * S
    tiles_max = -(-n_long * G // 256)
    head = (f"{label} B={B} H={H} Hkv={Hkv} D={D} bf16 {layout}{16 if layout == 'paged' else ''} M={M}: 1 x n={n_long} at "
            f"pos {pos_long} + {B - 1} x n=1 at pos {pos_rest}: varlen {t_var:9.1f} us, grid of {wgs} workgroups "
            f"(S={S}; B x max tiles would be {B * tiles_max * Hkv * S})")
    if not pad:
        print(head, flush=True)
        return
    # the padded chunk: every sequence n_long tokens (the only single call before sfa_decode_varlen)
    qkv_p = torch.randn((B, n_long) + per_tok, device=dev, dtype=dt)
    o_p = torch.empty(B, n_long, H, D, device=dev, dtype=dt)
    t_pad = timed(lambda: sfa.flash_decode_chunk(qkv_p, z, z, z, kc, vc, sl, o_p, B, M, H, D, D, M, 1, 0, **kw), 3)
    del qkv_p, o_p
    # two calls: a chunk on sequence 0, flash_decode on the rest (their caches / table rows are contiguous slices)
    kw1, kwr = dict(kw), dict(kw)
    if layout == "paged":
        kw1["block_table"], kwr["block_table"] = kw["block_table"][:1].contiguous(), kw["block_table"][1:].contiguous()
        k1, v1, kr, vr = kc, vc, kc, vc
    else:
        k1, v1, kr, vr = kc[:1], vc[:1], kc[1:], vc[1:]
    q1, o1 = qkv[:n_long].view((1, n_long) + per_tok), o[:n_long].view(1, n_long, H, D)
    qr, orr = qkv[n_long:], o[n_long:]
    sl1, slr = sl[:1].contiguous(), sl[1:].contiguous()

    def two():
        sfa.flash_decode_chunk(q1, z, z, z, k1, v1, sl1, o1, 1, M, H, D, D, M, 1, 0, **kw1)
        sfa.flash_decode(qr, z, z, z, kr, vr, slr, orr, B - 1, M, H, D, D, M, 1, 0, **kwr)

    t_two = timed(two, 10)
    print(f"{head} | chunk padded to n={n_long} {t_pad:10.1f} us = {t_pad / t_var:5.1f}x varlen | chunk(1 seq) + "
          f"decode({B - 1}) {t_two:9.1f} us = {t_two / t_var:4.2f}x varlen", flush=True)


if __name__ == "__main__":
    if "--mixed-only" in sys.argv:          # one mixed shape, for a kernel trace (rocprofv3 --kernel-trace --stats)
        mixed(64, 32, 32, 128, "blhmd", pad=False)
        sys.exit(0)
    if "--uniform-one" in sys.argv:         # the two one-workgroup-per-CU shapes, chunk and varlen, for a kernel trace
        uniform(4, 32, 32, 128, 3584, 512, "blhmd", 10)
        uniform(4, 32, 32, 128, 0, 512, "blhmd", 10)
        sys.exit(0)
    for n in (1, 2, 4, 8, 16):
        uniform(64, 32, 32, 128, 4095, n, "blmhd", 50, M=4096 + 16)
    for n in (512, 2048, 4096):
        for layout in ("blhmd", "blmhd"):
            uniform(4, 32, 32, 128, 0, n, layout, 10)
    uniform(4, 32, 32, 128, 3584, 512, "blhmd", 10)
    uniform(4, 32, 4, 128, 0, 2048, "paged", 10)
    uniform(4, 32, 4, 128, 3584, 512, "paged", 10)
    mixed(64, 32, 32, 128, "blhmd")
    mixed(64, 32, 4, 128, "paged")
    mixed(256, 32, 32, 128, "blhmd", n_long=4096, pos_long=0, pos_rest=4095, M=4096, pad=False, label="empty-heavy")
