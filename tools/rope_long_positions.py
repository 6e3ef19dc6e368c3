"""The table of profiles/decode_rope_long_positions.txt: which deviations of inv_freq, in fp32 ulps from
-2 to +2, are consistent with the cos / sin the device stored for the probe tokens of tests/test_long_context_gpu.py, per
position and pair, and whether the entries stored the same bits.  Needs a GPU.

    python tools/rope_long_positions.py [output file]          (default: standard output only)
"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "tests"))
sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
import numpy as np
import torch
import long_context_cases as lc
import test_long_context_gpu as t
import starflashattention_amd as sfa
sfa._lib.load()
out = open(sys.argv[1], "w") if len(sys.argv) > 1 else None


def P(*a):
    print(*a)
    if out:
        print(*a, file=out)


devs = np.arange(-lc.ENVELOPE_ULPS, lc.ENVELOPE_ULPS + 1)
fmt = lambda ok: "".join("x" if v else "." for v in ok)
P("Far-position RoPE probe on the MI355X: head_dim 64, one kv head, memory_max_len 131072, trigonometry in the kernel.")
P("Per pair j: the deviations d in -2..+2 (fp32 ulps of oracle inv_freq[j]) for which cos/sin of fl32(p * f_d) in fp64 are both")
P("within one storage ulp of the stored row; 'x' = consistent, '.' = not, columns d = -2 -1 0 +1 +2.  'xxxxx' = the pair cannot tell.")
for dtype in ("fp16", "bf16"):
    for rot in (64, 32):
        per_entry = {}
        for name, shape, windowed, G in t.PROBE_ENTRIES:
            rows = t.run_probe(sfa, name, shape, windowed, G, dtype, rot, False)
            per_entry[name] = {p: rows[p][0].astype(np.float64) for p in lc.PROBE_POSITIONS}
        first = per_entry[t.PROBE_ENTRIES[0][0]]
        same = all(np.array_equal(per_entry[n][p], first[p]) for n in per_entry for p in lc.PROBE_POSITIONS)
        P(f"\n== {dtype}, rot {rot}: the {len(per_entry)} entries ({', '.join(per_entry)}) bit-identical at every probe position: {same}")
        inter = np.ones((len(devs), rot // 2), bool)
        for p in lc.PROBE_POSITIONS:
            ok = lc.consistent_deviations(first[p], p, rot, dtype)
            inter &= ok
            tell = [j for j in range(rot // 2) if not ok[:, j].all()]
            P(f"position {p:6d}: pairs outside the envelope: {np.flatnonzero(~ok.any(axis=0)).tolist()}; pairs that can tell ({len(tell)}): " +
              " ".join(f"{j}:{fmt(ok[:, j])}" for j in tell))
            if not same:
                for n in per_entry:
                    okn = lc.consistent_deviations(per_entry[n][p], p, rot, dtype)
                    P(f"    {n}: " + " ".join(f"{j}:{fmt(okn[:, j])}" for j in range(rot // 2) if not okn[:, j].all()))
        P("all positions together, per pair: " + " ".join(f"{j}:{fmt(inter[:, j])}" for j in range(rot // 2)))
        P("pairs with no deviation consistent at every position: ", np.flatnonzero(~inter.any(axis=0)).tolist())
        P("pairs the probe pins to the oracle's inv_freq (d = 0 only): ", np.flatnonzero(inter[2] & (inter.sum(axis=0) == 1)).tolist())
        P("pairs that exclude d = 0: ", np.flatnonzero(~inter[2]).tolist())
if out:
    out.close()
