#!/usr/bin/env python3
"""sfa_prefill_varlen_window_fwd timings (HIP events over back-to-back calls after a warm-up; five runs, interleaved with
the calls they are compared with, in one process on one device; the median and the five-run spread).  bf16.  Lines:
  * uniform gpt-oss: 4 sequences of 4096 rows, 64 query heads over 8 kv heads, head_dim 64, window 128, sinks.
    flash_attn_varlen_window_fwd on the packed [B * S, H, D] storage against flash_attn_window_fwd on the same storage
    viewed as [B, H, S, D] (the same walk: the bits must be equal).
    Expectation: packed <= rectangular + both spreads + the plan kernel's duration (--trace / --summary).
  * ragged prompts: one sequence of 8192 rows plus 31 of 256, the same heads, window 128, sinks.  Against (a) a loop of 32
    flash_attn_window_fwd calls on the packed storage and (b) flash_attn_varlen_fwd(causal=True) on the same batch (no
    window, no sinks: every key tile up to the diagonal).
    Expectation (a): faster by more than the summed spreads.  (b): the ratio is stated beside the ratio of key tiles
    walked; recorded.
  * chunked mix: 8 sequences with n_q = 512 against n_k = 1024, 2048, ..., 8192, 32 query heads over 8 kv heads, head_dim
    128, windows 128 and 1024, no sinks, against flash_attn_varlen_fwd(causal=True).  Recorded.
  * ragged prompts with window = INT_MAX and sinks (the windowed kernel under the causal mask) against
    flash_attn_varlen_fwd(causal=True).  Recorded.
Key tiles walked: 64-key tiles staged, summed over the (sequence, 256-row q-tile) work items of one head.
  --trace         the launches only: the uniform line's packed call twelve times, for
                  `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/prefill_varlen_window_bench.py --trace`
  --summary DIR   the plan kernel and the attention kernel from that run's kernel trace (median of the last ten)
  --plan-us X     the plan kernel's duration from such a run: the uniform line then states its expectation HELD / MISSED"""
import csv
import glob
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

INT_MAX = 2 ** 31 - 1
TRACE_ITERS = 12
GPT_OSS = (64, 8, 64)       # Hq, Hkv, D


def timed(fn, iters):
    import torch
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


def med(xs):
    return statistics.median(xs), max(xs) - min(xs)


def interleaved(calls, iters):
    times = {key: [] for key in calls}
    for _ in range(5):
        for key, fn in calls.items():
            times[key].append(timed(fn, iters))
    return {key: med(t) for key, t in times.items()}


def cu_of(lengths):
    import torch
    cu = [0]
    for n in lengths:
        cu.append(cu[-1] + n)
    return cu, torch.tensor(cu, dtype=torch.int32, device="cuda:0")


def packed(lens_q, lens_k, heads, seed):
    import torch
    Hq, Hkv, D = heads
    dev, dt = torch.device("cuda:0"), torch.bfloat16
    torch.manual_seed(seed)
    q = torch.randn(sum(lens_q), Hq, D, device=dev).to(dt)
    k = torch.randn(sum(lens_k), Hkv, D, device=dev).to(dt)
    v = torch.randn(sum(lens_k), Hkv, D, device=dev).to(dt)
    sinks = torch.linspace(-1.0, 2.0, Hq, device=dev, dtype=torch.float32)     # around the lse of a 128-key window of N(0,1) scores
    return q, k, v, torch.empty_like(q), sinks


def key_tiles(lens_q, lens_k, window):
    """64-key tiles the work items of one head stage: [ts0, wg_end) per (sequence, 256-row q-tile); window None: causal"""
    total = 0
    for nq, nk in zip(lens_q, lens_k):
        coff = nk - nq
        for q0 in range(0, nq, 256):
            lim = min(q0 + 256, nq) - 1 + coff
            end = lim // 64 + 1 if lim >= 0 else 0
            lo = 0 if window is None or q0 + coff < window else q0 + coff + 1 - window
            total += max(0, end - lo // 64)
    return total


def rect(t, B, S):
    """packed [B * S, H, D] storage viewed as [B, H, S, D]"""
    return t.view(B, S, t.shape[1], t.shape[2]).transpose(1, 2)


def show(m, key):
    t, s = m[key]
    return f"{key} {t:8.1f} us (spread {s:.1f})"


def uniform(sfa, plan_us):
    import torch
    B, S, W, iters = 4, 4096, 128, 20
    q, k, v, out, sinks = packed([S] * B, [S] * B, GPT_OSS, 1)
    _, cu = cu_of([S] * B)
    out_r = torch.empty_like(out)
    calls = {"packed": lambda: sfa.flash_attn_varlen_window_fwd(q, k, v, cu, cu, W, sinks=sinks, out=out),
             "rectangular": lambda: sfa.flash_attn_window_fwd(rect(q, B, S), rect(k, B, S), rect(v, B, S), W, sinks=sinks,
                                                              out=rect(out_r, B, S))}
    calls["packed"]()
    calls["rectangular"]()
    torch.cuda.synchronize()
    same = torch.equal(out.view(torch.int16), out_r.view(torch.int16))
    err = (out.float() - out_r.float()).abs().max().item()
    assert err <= 1.6e-2, err
    m = interleaved(calls, iters)
    (a, sa), (u, su) = m["packed"], m["rectangular"]
    if plan_us is None:
        verdict = f"EXPECTATION packed <= rectangular + spreads {sa + su:.1f} us + plan kernel: packed - rectangular = {a - u:.1f} us " \
                  f"(plan kernel duration: --trace / --summary)"
    else:
        verdict = f"EXPECTATION packed <= rectangular + spreads {sa + su:.1f} us + plan kernel {plan_us:.1f} us: " \
                  f"{'HELD' if a <= u + sa + su + plan_us else 'MISSED'} (packed - rectangular = {a - u:.1f} us)"
    print(f"uniform gpt-oss: B={B} S={S} Hq={GPT_OSS[0]} Hkv={GPT_OSS[1]} D={GPT_OSS[2]} window={W} sinks bf16 | {show(m, 'packed')} | "
          f"{show(m, 'rectangular')} (bits {'equal' if same else 'differ, max |diff| %.2e' % err}) | packed / rectangular {a / u:.3f} | "
          f"{verdict}", flush=True)


def ragged(sfa, window):
    import torch
    lens = [8192] + [256] * 31
    q, k, v, out, sinks = packed(lens, lens, GPT_OSS, 2)
    cu_list, cu = cu_of(lens)
    out_l, out_c = torch.empty_like(out), torch.empty_like(out)

    def loop():
        for b, n in enumerate(lens):
            c0 = cu_list[b]
            sfa.flash_attn_window_fwd(*(t[c0:c0 + n].transpose(0, 1)[None] for t in (q, k, v)), window, sinks=sinks,
                                      out=out_l[c0:c0 + n].transpose(0, 1)[None])
    calls = {"packed": lambda: sfa.flash_attn_varlen_window_fwd(q, k, v, cu, cu, window, sinks=sinks, out=out),
             "causal varlen": lambda: sfa.flash_attn_varlen_fwd(q, k, v, cu, cu, causal=True, out=out_c)}
    if window != INT_MAX:
        calls["loop of 32"] = loop
    calls["packed"]()
    loop()
    torch.cuda.synchronize()
    same = torch.equal(out.view(torch.int16), out_l.view(torch.int16))
    m = interleaved(calls, 5)
    w = None if window == INT_MAX else window
    tiles_w, tiles_c = key_tiles(lens, lens, w), key_tiles(lens, lens, None)
    (a, sa), (c, sc) = m["packed"], m["causal varlen"]
    head = f"ragged prompts: 1 x 8192 + 31 x 256 rows, Hq={GPT_OSS[0]} Hkv={GPT_OSS[1]} D={GPT_OSS[2]} window=" \
           f"{'INT_MAX' if w is None else w} sinks bf16 | {show(m, 'packed')} | {show(m, 'causal varlen')}"
    tail = f"packed / causal varlen {a / c:.3f} (key tiles walked {tiles_w} / {tiles_c} = {tiles_w / tiles_c:.3f}): recorded"
    if w is None:
        print(f"{head} | {tail}", flush=True)
        return
    l, sl = m["loop of 32"]
    print(f"{head} | loop of 32 calls {l:8.1f} us (spread {sl:.1f}) (bits {'equal' if same else 'differ'}) | loop / packed {l / a:.2f} | "
          f"EXPECTATION faster than the loop by more than the spreads {sa + sl:.1f} us: {'HELD' if a < l - sa - sl else 'MISSED'} | {tail}",
          flush=True)


def chunked(sfa):
    heads = (32, 8, 128)
    lens_q, lens_k = [512] * 8, [1024 * i for i in range(1, 9)]
    q, k, v, out, _ = packed(lens_q, lens_k, heads, 3)
    _, cq = cu_of(lens_q)
    _, ck = cu_of(lens_k)
    calls = {"causal varlen": lambda: sfa.flash_attn_varlen_fwd(q, k, v, cq, ck, causal=True, out=out)}
    for W in (128, 1024):
        calls[f"window {W}"] = lambda W=W: sfa.flash_attn_varlen_window_fwd(q, k, v, cq, ck, W, out=out)
    m = interleaved(calls, 20)
    tiles_c = key_tiles(lens_q, lens_k, None)
    parts = [show(m, "causal varlen")]
    for W in (128, 1024):
        t = key_tiles(lens_q, lens_k, W)
        parts.append(f"{show(m, f'window {W}')} = {m[f'window {W}'][0] / m['causal varlen'][0]:.3f} of causal (key tiles walked {t} / "
                     f"{tiles_c} = {t / tiles_c:.3f})")
    print(f"chunked mix: 8 x n_q = 512 against n_k = 1024 .. 8192, Hq={heads[0]} Hkv={heads[1]} D={heads[2]} bf16, no sinks | "
          + " | ".join(parts) + " | recorded", flush=True)


def trace(sfa):
    import torch
    B, S = 4, 4096
    q, k, v, out, sinks = packed([S] * B, [S] * B, GPT_OSS, 1)
    _, cu = cu_of([S] * B)
    for _ in range(TRACE_ITERS):
        sfa.flash_attn_varlen_window_fwd(q, k, v, cu, cu, 128, sinks=sinks, out=out)
    torch.cuda.synchronize()
    print(f"uniform gpt-oss: {TRACE_ITERS} packed calls", flush=True)


def summary(root):
    rows = []
    for f in glob.glob(os.path.join(root, "**", "*kernel_trace.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            rows.append((int(row["Start_Timestamp"]), int(row["End_Timestamp"]), row["Kernel_Name"]))
    rows.sort()
    plan = [(e - s) / 1e3 for s, e, n in rows if "prefill_varlen_plan_kernel" in n]
    attn = [(e - s) / 1e3 for s, e, n in rows if "prefill_varlen_window_kernel" in n]
    gap = [(s2 - e1) / 1e3 for (s1, e1, n1), (s2, e2, n2) in zip(rows, rows[1:])
           if "prefill_varlen_plan_kernel" in n1 and "prefill_varlen_window_kernel" in n2]
    assert len(plan) == len(attn) == TRACE_ITERS, (len(plan), len(attn))
    print(f"uniform gpt-oss, kernel trace: prefill_varlen_plan_kernel {statistics.median(plan[2:]):6.1f} us | "
          f"prefill_varlen_window_kernel {statistics.median(attn[2:]):8.1f} us | plan end -> attention start "
          f"{statistics.median(gap[2:]):6.1f} us")
    return statistics.median(plan[2:])


if __name__ == "__main__":
    if "--summary" in sys.argv:
        summary(sys.argv[sys.argv.index("--summary") + 1])
        sys.exit(0)
    import starflashattention_amd as sfa
    if "--trace" in sys.argv:
        trace(sfa)
        sys.exit(0)
    plan_us = float(sys.argv[sys.argv.index("--plan-us") + 1]) if "--plan-us" in sys.argv else None
    uniform(sfa, plan_us)
    ragged(sfa, 128)
    chunked(sfa)
    ragged(sfa, INT_MAX)
