#!/usr/bin/env python3
"""sfa_prefill_varlen_fwd timings (HIP events over back-to-back calls after a warm-up; five runs, interleaved with the
calls they are compared with, in one process on one device; the median and the five-run spread).  bf16, head_dim 128, 32
query heads over 8 kv heads.  Lines:
  * uniform: B = 8 sequences of 2048 rows, full and causal.  flash_attn_varlen_fwd on the packed [B * S, H, D] storage
    against flash_attn_fwd on the same storage viewed as [B, H, S, D], under the library's own choice of kernel and under
    prefill_impl 10 (the exact 8-wave 256-row kernel: the same tile pipeline on a rectangular grid).
    Expectation, full attention: varlen <= impl 10 + both spreads + the plan kernel's duration (--trace / --summary).
    The causal lines and the library's-choice lines are recorded.
  * ragged prompts: one sequence of 8192 rows plus 31 of 256, causal.  Against the padded flash_attn_fwd at
    [32, H, 8192, D] and against a loop of 32 flash_attn_fwd calls on the packed storage.
    Expectation: faster than both by more than the summed spreads; the ratios are stated next to the ratio of visible
    query-key pairs.
  * chunked mix: 8 sequences with n_q = 512 against n_k = 1024, 2048, ..., 8192, causal.  Recorded only.
TFLOPS from 4 Hq D x (visible query-key pairs summed over the sequences).
  --trace         the launches only: the uniform full line's packed call twelve times, for
                  `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/prefill_varlen_bench.py --trace`
  --summary DIR   the plan kernel and the attention kernel from that run's kernel trace (median of the last ten)
  --plan-us X     the plan kernel's duration from such a run: the uniform full line then states its expectation HELD / MISSED"""
import csv
import glob
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HQ, HKV, D = 32, 8, 128
TRACE_ITERS = 12
LIB = "library's choice"


def visible_pairs(Sq, Sk, causal):
    if not causal:
        return Sq * Sk
    return sum(max(0, min(Sk, i + Sk - Sq + 1)) for i in range(Sq))


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


def cu_of(lengths):
    import torch
    cu = [0]
    for n in lengths:
        cu.append(cu[-1] + n)
    return cu, torch.tensor(cu, dtype=torch.int32, device="cuda:0")


def packed(lens_q, lens_k, seed):
    import torch
    dev, dt = torch.device("cuda:0"), torch.bfloat16
    torch.manual_seed(seed)
    q = torch.randn(sum(lens_q), HQ, D, device=dev).to(dt)
    k = torch.randn(sum(lens_k), HKV, D, device=dev).to(dt)
    v = torch.randn(sum(lens_k), HKV, D, device=dev).to(dt)
    return q, k, v, torch.empty_like(q)


def interleaved(calls, iters):
    times = {key: [] for key in calls}
    for _ in range(5):
        for key, fn in calls.items():
            times[key].append(timed(fn, iters))
    return {key: med(t) for key, t in times.items()}


def rect(t, B, S):
    """packed [B * S, H, D] storage viewed as [B, H, S, D]"""
    return t.view(B, S, t.shape[1], t.shape[2]).transpose(1, 2)


def show(m, flops, key):
    t, s = m[key]
    return f"{key} {t:8.1f} us (spread {s:.1f}) {flops / t * 1e-6:6.1f} TFLOPS"


def uniform(sfa, causal, plan_us):
    import torch
    B, S, iters = 8, 2048, 20
    q, k, v, out = packed([S] * B, [S] * B, 1)
    _, cu = cu_of([S] * B)
    out_r = torch.empty_like(out)

    def impl10():
        sfa.debug_set("prefill_impl", 10)
        r = sfa.flash_attn_fwd(rect(q, B, S), rect(k, B, S), rect(v, B, S), causal=causal, out=rect(out_r, B, S))
        sfa.debug_set("prefill_impl", -1)
        return r
    calls = {"varlen": lambda: sfa.flash_attn_varlen_fwd(q, k, v, cu, cu, causal=causal, out=out),
             "impl 10": impl10,
             LIB: lambda: sfa.flash_attn_fwd(rect(q, B, S), rect(k, B, S), rect(v, B, S), causal=causal, out=rect(out_r, B, S))}
    # the same result first: the packed call and the 8-wave exact kernel walk the same tiles in the same order
    calls["varlen"]()
    calls["impl 10"]()
    torch.cuda.synchronize()
    same = torch.equal(out.view(torch.int16), out_r.view(torch.int16))
    err = (out.float() - out_r.float()).abs().max().item()
    assert err <= 1.6e-2, err
    calls[LIB]()
    torch.cuda.synchronize()
    kern = sfa.last_prefill_kernel()
    m = interleaved(calls, iters)
    flops = 4.0 * HQ * D * B * visible_pairs(S, S, causal)
    (a, sa), (u, su) = m["varlen"], m["impl 10"]
    tag = "causal" if causal else "full"
    verdict = ""
    if not causal:
        if plan_us is None:
            verdict = f" | EXPECTATION varlen <= impl 10 + spreads {sa + su:.1f} us + plan kernel: varlen - impl 10 = {a - u:.1f} us " \
                      f"(plan kernel duration: --trace / --summary)"
        else:
            verdict = f" | EXPECTATION varlen <= impl 10 + spreads {sa + su:.1f} us + plan kernel {plan_us:.1f} us: " \
                      f"{'HELD' if a <= u + sa + su + plan_us else 'MISSED'} (varlen - impl 10 = {a - u:.1f} us)"
    print(f"uniform {tag}: B={B} S={S} Hq={HQ} Hkv={HKV} D={D} bf16 | {show(m, flops, 'varlen')} | {show(m, flops, 'impl 10')} "
          f"(bits {'equal' if same else 'differ, max |diff| %.2e' % err}) | {show(m, flops, LIB)} "
          f"[{kern}] | varlen / impl 10 {a / u:.3f}, varlen / library's choice {a / m[LIB][0]:.3f}{verdict}", flush=True)


def ragged(sfa):
    import torch
    lens = [8192] + [256] * 31
    B, Smax, iters = len(lens), max(lens), 3
    q, k, v, out = packed(lens, lens, 2)
    cu_list, cu = cu_of(lens)
    dev, dt = q.device, q.dtype
    qp = torch.zeros(B, HQ, Smax, D, device=dev, dtype=dt)
    kp = torch.zeros(B, HKV, Smax, D, device=dev, dtype=dt)
    vp = torch.zeros(B, HKV, Smax, D, device=dev, dtype=dt)
    for b, n in enumerate(lens):        # padded at the end: with n_q = n_k the causal mask of the real rows is unchanged
        c0 = cu_list[b]
        qp[b, :, :n], kp[b, :, :n], vp[b, :, :n] = (t[c0:c0 + n].transpose(0, 1) for t in (q, k, v))
    op = torch.empty_like(qp)
    out_l = torch.empty_like(out)

    def loop():
        for b, n in enumerate(lens):
            c0 = cu_list[b]
            sfa.flash_attn_fwd(*(t[c0:c0 + n].transpose(0, 1)[None] for t in (q, k, v)), causal=True,
                               out=out_l[c0:c0 + n].transpose(0, 1)[None])
    calls = {"varlen": lambda: sfa.flash_attn_varlen_fwd(q, k, v, cu, cu, causal=True, out=out),
             "padded": lambda: sfa.flash_attn_fwd(qp, kp, vp, causal=True, out=op),
             "loop of 32": loop}
    calls["varlen"]()
    loop()
    torch.cuda.synchronize()
    err = (out.float() - out_l.float()).abs().max().item()
    assert err <= 1.6e-2, err
    m = interleaved(calls, iters)
    pairs = sum(visible_pairs(n, n, True) for n in lens)
    pairs_padded = B * visible_pairs(Smax, Smax, True)
    flops = 4.0 * HQ * D * pairs
    (a, sa), (p, sp), (l, sl) = m["varlen"], m["padded"], m["loop of 32"]
    print(f"ragged prompts: 1 x 8192 + 31 x 256 rows, causal, Hq={HQ} Hkv={HKV} D={D} bf16 | {show(m, flops, 'varlen')} | "
          f"padded [32, H, 8192, D] {p:8.1f} us (spread {sp:.1f}) | loop of 32 calls {l:8.1f} us (spread {sl:.1f}) | "
          f"padded / varlen {p / a:.2f} (visible pairs padded / packed {pairs_padded / pairs:.2f}), loop / varlen {l / a:.2f} | "
          f"EXPECTATION faster than padded by more than the spreads {sa + sp:.1f} us: {'HELD' if a < p - sa - sp else 'MISSED'}; "
          f"faster than the loop by more than the spreads {sa + sl:.1f} us: {'HELD' if a < l - sa - sl else 'MISSED'}", flush=True)


def chunked(sfa):
    import torch
    lens_q, lens_k = [512] * 8, [1024 * i for i in range(1, 9)]
    q, k, v, out = packed(lens_q, lens_k, 3)
    _, cq = cu_of(lens_q)
    _, ck = cu_of(lens_k)
    m = interleaved({"varlen": lambda: sfa.flash_attn_varlen_fwd(q, k, v, cq, ck, causal=True, out=out)}, 20)
    flops = 4.0 * HQ * D * sum(visible_pairs(a, b, True) for a, b in zip(lens_q, lens_k))
    print(f"chunked mix: 8 x n_q = 512 against n_k = 1024 .. 8192, causal, Hq={HQ} Hkv={HKV} D={D} bf16 | {show(m, flops, 'varlen')} "
          f"| recorded only", flush=True)


def trace(sfa):
    import torch
    B, S = 8, 2048
    q, k, v, out = packed([S] * B, [S] * B, 1)
    _, cu = cu_of([S] * B)
    for _ in range(TRACE_ITERS):
        sfa.flash_attn_varlen_fwd(q, k, v, cu, cu, causal=False, out=out)
    torch.cuda.synchronize()
    print(f"uniform full: {TRACE_ITERS} packed calls", flush=True)


def summary(root):
    rows = []
    for f in glob.glob(os.path.join(root, "**", "*kernel_trace.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            rows.append((int(row["Start_Timestamp"]), int(row["End_Timestamp"]), row["Kernel_Name"]))
    rows.sort()
    plan = [(e - s) / 1e3 for s, e, n in rows if "prefill_varlen_plan_kernel" in n]
    attn = [(e - s) / 1e3 for s, e, n in rows if "prefill_varlen_kernel" in n]
    gap = [(s2 - e1) / 1e3 for (s1, e1, n1), (s2, e2, n2) in zip(rows, rows[1:])
           if "prefill_varlen_plan_kernel" in n1 and "prefill_varlen_kernel" in n2]
    assert len(plan) == len(attn) == TRACE_ITERS, (len(plan), len(attn))
    print(f"uniform full, kernel trace: prefill_varlen_plan_kernel {statistics.median(plan[2:]):6.1f} us | prefill_varlen_kernel "
          f"{statistics.median(attn[2:]):8.1f} us | plan end -> attention start {statistics.median(gap[2:]):6.1f} us")
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
    uniform(sfa, False, plan_us)
    uniform(sfa, True, plan_us)
    ragged(sfa)
    chunked(sfa)
