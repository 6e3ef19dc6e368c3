#!/usr/bin/env python3
"""sfa_prefill_varlen_split_fwd timings (HIP events over back-to-back calls after a warm-up; five runs, interleaved with the
calls they are compared with, in one process on one device; the median and the five-run spread).  bf16, head_dim 128.
Every line is compared with flash_attn_varlen_fwd -- the unsplit packed call -- on the same tensors.  Lines:
  1. chunked mix, few heads: 8 sequences with n_q = 512 against n_k = 1024, 2048, ..., 8192, causal, 8 query heads over 2:
     128 workgroups unsplit.  Explicit 2, 4, 8 and the library's choice, max_seqlen_k = 8192.
     Expectation: the best explicit count and the library's choice are faster than the unsplit call by more than the two
     spreads.
  2. the same with 32 heads over 8: 512 workgroups.  Expectation: the library's choice resolves to 1 and its time equals
     the unsplit call's within that call's spread.
  3. one short block against a long prefix: 1 x n_q = 256 against 32768 keys and 3 x n_q = 256 against 1024, one batch, 8
     heads over 2, max_seqlen_k = 32768.  Explicit 4, 8, 16 and the library's choice.  Recorded: the uneven case a uniform
     chunk length serves worst.
  4. loop comparison: the shape of line 1 against a loop of 8 flash_attn_split_fwd calls (library's choice each).  Recorded.
TFLOPS from 4 Hq D x (visible query-key pairs summed over the sequences).
  --trace         the launches only: line 1's call with 4 splits twelve times, for
                  `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/prefill_varlen_split_bench.py --trace`
  --summary DIR   the plan, items, attention and combine kernels from that run's kernel trace (median of the last ten)"""
import csv
import glob
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.prefill_varlen_bench import cu_of, interleaved, visible_pairs     # noqa: E402

D = 128
TRACE_ITERS = 12
UNSPLIT, AUTO = "unsplit", "auto"


def packed(lens_q, lens_k, Hq, Hkv, seed):
    import torch
    dev, dt = torch.device("cuda:0"), torch.bfloat16
    torch.manual_seed(seed)
    q = torch.randn(sum(lens_q), Hq, D, device=dev).to(dt)
    k = torch.randn(sum(lens_k), Hkv, D, device=dev).to(dt)
    v = torch.randn(sum(lens_k), Hkv, D, device=dev).to(dt)
    return q, k, v


def line(sfa, title, lens_q, lens_k, Hq, Hkv, counts, seed, iters, loop=False):
    """times of the unsplit call, the explicit counts and the library's choice; returns (medians, resolved auto count)"""
    import torch
    q, k, v = packed(lens_q, lens_k, Hq, Hkv, seed)
    cuq_list, cq = cu_of(lens_q)
    cuk_list, ck = cu_of(lens_k)
    max_k = max(lens_k)
    out_u, out_s = torch.empty_like(q), torch.empty_like(q)
    calls = {UNSPLIT: lambda: sfa.flash_attn_varlen_fwd(q, k, v, cq, ck, causal=True, out=out_u)}
    for S in counts:
        calls[f"S={S}"] = (lambda S=S: sfa.flash_attn_varlen_split_fwd(q, k, v, cq, ck, max_k, causal=True, num_splits=S, out=out_s))
    calls[AUTO] = lambda: sfa.flash_attn_varlen_split_fwd(q, k, v, cq, ck, max_k, causal=True, num_splits=0, out=out_s)
    if loop:
        def loop_of_calls():
            for b, (nq, nk) in enumerate(zip(lens_q, lens_k)):
                q0, k0 = cuq_list[b], cuk_list[b]
                sfa.flash_attn_split_fwd(q[q0:q0 + nq].transpose(0, 1)[None], k[k0:k0 + nk].transpose(0, 1)[None],
                                         v[k0:k0 + nk].transpose(0, 1)[None], causal=True, num_splits=0,
                                         out=out_s[q0:q0 + nq].transpose(0, 1)[None])
        calls[f"loop of {len(lens_q)}"] = loop_of_calls
    # the same result first
    calls[UNSPLIT]()
    for key, fn in calls.items():
        if key == UNSPLIT:
            continue
        out_s.zero_()
        fn()
        torch.cuda.synchronize()
        err = (out_s.float() - out_u.float()).abs().max().item()
        assert err <= 1.6e-2, (key, err)
    calls[AUTO]()
    torch.cuda.synchronize()
    auto = sfa.debug_get("last_prefill_splits")
    m = interleaved(calls, iters)
    flops = 4.0 * Hq * D * sum(visible_pairs(a, b, True) for a, b in zip(lens_q, lens_k))
    cols = " | ".join(f"{key}{' -> %d' % auto if key == AUTO else ''} {t:8.1f} us (spread {s:.1f}) {flops / t * 1e-6:6.1f} TFLOPS"
                      for key, (t, s) in m.items())
    print(f"{title}: Hq={Hq} Hkv={Hkv} D={D} bf16 causal max_seqlen_k={max_k} | {cols}", end="", flush=True)
    return m, auto


def chunked_few_heads(sfa):
    lens_q, lens_k = [512] * 8, [1024 * i for i in range(1, 9)]
    m, auto = line(sfa, "1. chunked mix, few heads: 8 x n_q = 512 against n_k = 1024 .. 8192", lens_q, lens_k, 8, 2, (2, 4, 8), 3, 20)
    u, su = m[UNSPLIT]
    best = min((k for k in m if k.startswith("S=")), key=lambda k: m[k][0])
    (b, sb), (a, sa) = m[best], m[AUTO]
    print(f" | EXPECTATION best explicit ({best}) faster than unsplit by more than the spreads {su + sb:.1f} us: "
          f"{'HELD' if b < u - su - sb else 'MISSED'} (unsplit / split {u / b:.2f}); the library's choice ({auto}) by more than "
          f"{su + sa:.1f} us: {'HELD' if a < u - su - sa else 'MISSED'} (unsplit / auto {u / a:.2f})", flush=True)


def chunked_many_heads(sfa):
    lens_q, lens_k = [512] * 8, [1024 * i for i in range(1, 9)]
    m, auto = line(sfa, "2. chunked mix, 32 heads: 8 x n_q = 512 against n_k = 1024 .. 8192", lens_q, lens_k, 32, 8, (2,), 3, 20)
    (u, su), (a, sa) = m[UNSPLIT], m[AUTO]
    print(f" | EXPECTATION the library's choice resolves to 1: {'HELD' if auto == 1 else 'MISSED'} ({auto}); its time within the "
          f"unsplit call's spread {su:.1f} us: {'HELD' if abs(a - u) <= su else 'MISSED'} (auto - unsplit = {a - u:.1f} us)", flush=True)


def long_prefix(sfa):
    lens_q, lens_k = [256] * 4, [32768, 1024, 1024, 1024]
    m, auto = line(sfa, "3. one short block against a long prefix: 1 x n_q = 256 against 32768, 3 x 256 against 1024", lens_q, lens_k,
                   8, 2, (4, 8, 16), 4, 10)
    u = m[UNSPLIT][0]
    print(" | recorded: " + ", ".join(f"unsplit / {key} {u / t:.2f}" for key, (t, _) in m.items() if key != UNSPLIT), flush=True)


def loop_comparison(sfa):
    lens_q, lens_k = [512] * 8, [1024 * i for i in range(1, 9)]
    m, auto = line(sfa, "4. loop comparison: the shape of line 1", lens_q, lens_k, 8, 2, (4,), 3, 10, loop=True)
    l = m["loop of 8"][0]
    print(f" | recorded: loop / S=4 {l / m['S=4'][0]:.2f}, loop / auto {l / m[AUTO][0]:.2f}, loop / unsplit {l / m[UNSPLIT][0]:.2f}",
          flush=True)


def trace(sfa):
    import torch
    lens_q, lens_k = [512] * 8, [1024 * i for i in range(1, 9)]
    q, k, v = packed(lens_q, lens_k, 8, 2, 3)
    _, cq = cu_of(lens_q)
    _, ck = cu_of(lens_k)
    out = torch.empty_like(q)
    for _ in range(TRACE_ITERS):
        sfa.flash_attn_varlen_split_fwd(q, k, v, cq, ck, 8192, causal=True, num_splits=4, out=out)
    torch.cuda.synchronize()
    print(f"line 1, 4 splits: {TRACE_ITERS} calls", flush=True)


def summary(root):
    rows = []
    for f in glob.glob(os.path.join(root, "**", "*kernel_trace.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            rows.append((int(row["Start_Timestamp"]), int(row["End_Timestamp"]), row["Kernel_Name"]))
    rows.sort()
    names = ("prefill_varlen_plan_kernel", "prefill_varlen_split_items_kernel", "prefill_varlen_split_kernel",
             "prefill_varlen_split_combine_kernel")
    cols = []
    for name in names:
        d = [(e - s) / 1e3 for s, e, n in rows if name + "<" in n or name + "(" in n or n.endswith(name) or name + " " in n]
        assert len(d) == TRACE_ITERS, (name, len(d))
        cols.append(f"{name} {statistics.median(d[2:]):7.1f} us")
    first = [s for s, e, n in rows if names[0] in n]
    last = [e for s, e, n in rows if names[3] in n]
    span = [(e - s) / 1e3 for s, e in zip(first, last)]
    print("line 1, 4 splits, kernel trace: " + " | ".join(cols) + f" | plan start -> combine end {statistics.median(span[2:]):7.1f} us")


if __name__ == "__main__":
    if "--summary" in sys.argv:
        summary(sys.argv[sys.argv.index("--summary") + 1])
        sys.exit(0)
    import starflashattention_amd as sfa
    if "--trace" in sys.argv:
        trace(sfa)
        sys.exit(0)
    chunked_few_heads(sfa)
    chunked_many_heads(sfa)
    long_prefix(sfa)
    loop_comparison(sfa)
