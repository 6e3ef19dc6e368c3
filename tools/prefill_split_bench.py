#!/usr/bin/env python3
"""sfa_prefill_split_fwd timings (HIP events over back-to-back calls after a warm-up; five runs, interleaved with the
calls they are compared with, in one process on one device; the median and the five-run spread), bf16.  Lines, head_dim
128 unless noted:
  * B = 1, H = 8 / 16 / 32, S = 4096, causal and full (the lines of profiles/r03_prefill_crossover.txt)
  * chunked prefill: Sq = 512 against Sk = 8192 / 32768, B = 1, Hq = 32, Hkv = 8, causal; Sq = 256 against Sk = 32768
  * B = 1, H = 4, S = 16384, causal
  * B = 4, H = 16, S = 1024, D = 64, full
  * a large grid, B = 4, H = 32, S = 4096 causal, where the auto rule must resolve to 1
Per line:
  unsplit  flash_attn_fwd under the library's own choice of kernel
  S=n      flash_attn_split_fwd with num_splits = n (-> the resolved count), n = 2, 4, 8, 16
  auto     flash_attn_split_fwd with num_splits = 0 (-> the count the library picked)
  TFLOPS of the unsplit and the auto call from 4 B Hq D x (visible query-key pairs)
Gates (margins are the two calls' own spreads):
  never loses  on every line auto <= unsplit + spread(auto) + spread(unsplit)
  win          on Sq = 512, Sk = 32768: auto < unsplit - spread(auto) - spread(unsplit); the ratio is stated and compared with
               the expectation unsplit / min(S', 4) + combine
  --trace      the launches only: every line's split call (auto's count, or 4 where auto resolves to 1) twelve times, for
               `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/prefill_split_bench.py --trace`
  --summary DIR   the attention kernel and the combine of each line from that run's kernel trace (median of the last ten)
  --probe      the minimum chunk: B = 1, Hq = 8, Sq = 256 (8 workgroups, every split fits the chip at once) against
               Sk = 1024 / 2048 / 4096 / 8192, full; an explicit count n walks chunks of Sk / 64 / n tiles
  --small      the first chunked line and the large grid only"""
import csv
import glob
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# (name, B, Hq, Hkv, D, Sq, Sk, causal, iters)
LINES = [(f"square H={H}", 1, H, H, 128, 4096, 4096, c, 20) for H in (8, 16, 32) for c in (True, False)] + [
    ("chunked 8k", 1, 32, 8, 128, 512, 8192, True, 20),
    ("chunked 32k", 1, 32, 8, 128, 512, 32768, True, 10),
    ("chunked 32k one q-tile", 1, 32, 8, 128, 256, 32768, True, 10),
    ("long H=4", 1, 4, 4, 128, 16384, 16384, True, 5),
    ("d64 short", 4, 16, 16, 64, 1024, 1024, False, 40),
    ("large grid", 4, 32, 32, 128, 4096, 4096, True, 5),
]
WIN_LINE = "chunked 32k"
TRACE_ITERS = 12


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


def tensors(B, Hq, Hkv, D, Sq, Sk):
    import torch
    dev, dt = torch.device("cuda:0"), torch.bfloat16
    torch.manual_seed(Sq + Sk + Hq)
    q = torch.randn(B, Hq, Sq, D, device=dev).to(dt)
    k = torch.randn(B, Hkv, Sk, D, device=dev).to(dt)
    v = torch.randn(B, Hkv, Sk, D, device=dev).to(dt)
    return q, k, v, torch.empty_like(q)


def line(sfa, name, B, Hq, Hkv, D, Sq, Sk, causal, iters):
    import torch
    q, k, v, out = tensors(B, Hq, Hkv, D, Sq, Sk)
    calls = {"unsplit": lambda: sfa.flash_attn_fwd(q, k, v, causal=causal, out=out)}
    for S in (2, 4, 8, 16, 0):
        calls["auto" if S == 0 else f"S={S}"] = (lambda S=S: sfa.flash_attn_split_fwd(q, k, v, causal=causal, num_splits=S, out=out))
    # the same result first: faster and different is not faster
    want = sfa.flash_attn_fwd(q, k, v, causal=causal).float()
    resolved = {}
    for key, fn in calls.items():
        if key == "unsplit":
            continue
        got = fn().float()
        torch.cuda.synchronize()
        resolved[key] = sfa.debug_get("last_prefill_splits")
        err = (got - want).abs().max().item()
        assert err <= 1.6e-2, (name, key, err)
    calls["unsplit"]()
    torch.cuda.synchronize()
    kern = sfa.last_prefill_kernel()
    times = {key: [] for key in calls}
    for _ in range(5):
        for key, fn in calls.items():
            times[key].append(timed(fn, iters))
    m = {key: med(t) for key, t in times.items()}
    flops = 4.0 * B * Hq * D * visible_pairs(Sq, Sk, causal)
    tf = lambda us: flops / us * 1e-6
    (u, su), (a, sa) = m["unsplit"], m["auto"]
    loses = a > u + su + sa
    cols = " | ".join(f"{key} -> {resolved[key]} {m[key][0]:8.1f} us (spread {m[key][1]:.1f})" for key in calls if key != "unsplit")
    print(f"{name}: B={B} Hq={Hq} Hkv={Hkv} D={D} Sq={Sq} Sk={Sk} {'causal' if causal else 'full'} bf16 | unsplit [{kern}] "
          f"{u:8.1f} us (spread {su:.1f}) {tf(u):6.1f} TFLOPS | {cols} | auto {tf(a):6.1f} TFLOPS, auto / unsplit {a / u:.3f}"
          f"{' (auto resolves to 1: the unsplit launch)' if resolved['auto'] == 1 else ''} | never-loses "
          f"{'FAILS' if loses else 'HOLDS'}", flush=True)
    return dict(name=name, m=m, resolved=resolved, loses=loses)


def trace(sfa):
    """the launches of the kernel trace: per line TRACE_ITERS split calls, in the order of LINES"""
    import torch
    for name, B, Hq, Hkv, D, Sq, Sk, causal, _ in LINES:
        q, k, v, out = tensors(B, Hq, Hkv, D, Sq, Sk)
        S = sfa.prefill_auto_splits(B, Hq, Sq, Sk, D, causal)
        S = S if S > 1 else 4
        for _ in range(TRACE_ITERS):
            sfa.flash_attn_split_fwd(q, k, v, causal=causal, num_splits=S, out=out)
        torch.cuda.synchronize()
        print(f"{name}: {TRACE_ITERS} calls with num_splits = {S} -> {sfa.debug_get('last_prefill_splits')}", flush=True)
        del q, k, v, out
        torch.cuda.empty_cache()


def summary(root):
    rows = []
    for f in glob.glob(os.path.join(root, "**", "*kernel_trace.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            rows.append((int(row["Start_Timestamp"]), int(row["End_Timestamp"]), row["Kernel_Name"]))
    rows.sort()
    attn = [(e - s) / 1e3 for s, e, n in rows if "prefill_split_kernel" in n]
    comb = [(e - s) / 1e3 for s, e, n in rows if "prefill_split_combine_kernel" in n]
    assert len(attn) == len(comb) == TRACE_ITERS * len(LINES), (len(attn), len(comb))
    for i, (name, B, Hq, Hkv, D, Sq, Sk, causal, _) in enumerate(LINES):
        a = statistics.median(attn[i * TRACE_ITERS + 2:(i + 1) * TRACE_ITERS])
        c = statistics.median(comb[i * TRACE_ITERS + 2:(i + 1) * TRACE_ITERS])
        print(f"{name}: Sq={Sq} Sk={Sk} Hq={Hq} {'causal' if causal else 'full'} | prefill_split_kernel {a:8.1f} us | "
              f"prefill_split_combine_kernel {c:7.1f} us | sum {a + c:8.1f} us")


if __name__ == "__main__":
    if "--summary" in sys.argv:
        summary(sys.argv[sys.argv.index("--summary") + 1])
        sys.exit(0)
    import starflashattention_amd as sfa
    if "--trace" in sys.argv:
        trace(sfa)
        sys.exit(0)
    if "--probe" in sys.argv:
        for Sk in (1024, 2048, 4096, 8192):
            r = line(sfa, f"probe {Sk // 64} tiles", 1, 8, 8, 128, 256, Sk, False, 40)
            u = r["m"]["unsplit"][0]
            print("    chunk length in tiles -> split / unsplit: " + ", ".join(
                f"{Sk // 64 // n} -> {r['m'][f'S={n}'][0] / u:.2f}" for n in (2, 4, 8, 16) if Sk // 64 // n >= 1), flush=True)
        sys.exit(0)
    lines = [l for l in LINES if l[0] in ("chunked 8k", "large grid")] if "--small" in sys.argv else LINES
    results = [line(sfa, *l) for l in lines]
    losers = [r["name"] for r in results if r["loses"]]
    print(f"GATE never loses (auto <= unsplit + both spreads on every line): {'HOLDS' if not losers else 'FAILS on ' + ', '.join(losers)}")
    for r in results:
        if r["name"] == WIN_LINE:
            (u, su), (a, sa) = r["m"]["unsplit"], r["m"]["auto"]
            S = r["resolved"]["auto"]
            print(f"GATE win on {WIN_LINE}: auto -> {S} {a:.1f} us < unsplit {u:.1f} us - spreads {su + sa:.1f} us: "
                  f"{'HOLDS' if a < u - su - sa else 'FAILS'}; unsplit / auto = {u / a:.2f}, expectation unsplit / min(S', 4) = "
                  f"{u / min(S, 4):.1f} us plus the combine (its time: --summary)")
