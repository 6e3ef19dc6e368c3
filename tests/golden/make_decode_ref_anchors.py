#!/usr/bin/env python3
"""Record tests/golden/decode_ref_anchors.npz: what the reference functions of the tests/*_ref.py files returned at the last
commit at which each of them held fp64 arithmetic of its own.  Since then they are adapters over tests/serving_model.py,
and section 1 of tests/test_serving_model_cpu.py holds the adapters against this file; without it those anchors would
compare the model with itself.

The cases are decode_ref_anchor_cases.py beside this script, of THIS tree; the functions they call are imported from
--tests-dir, the tests/ directory of a checkout of that earlier commit (the parent of the commit that added this script),
for example

    git worktree add /tmp/before <commit>
    python tests/golden/make_decode_ref_anchors.py --tests-dir /tmp/before/tests

The script refuses a tree whose references are adapters already.  Inputs are not stored (the seeded builders regenerate
them); the file records the commit it was made from under the key "commit"."""
import argparse
import importlib.util
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF_MODULES = ("window_ref", "sinks_ref", "kv8_ref", "kv8_window_ref", "kv8_sinks_ref", "chunk_kv8_ref", "chunk_kv8_window_ref",
               "chunk_window_ref")


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--tests-dir", required=True, help="tests/ of a checkout of the commit to record")
    ap.add_argument("--out", default=os.path.join(HERE, "decode_ref_anchors.npz"))
    args = ap.parse_args()
    tests_dir = os.path.abspath(args.tests_dir)
    for name in REF_MODULES:
        with open(os.path.join(tests_dir, name + ".py")) as f:
            if "serving_model" in f.read():
                sys.exit(f"{tests_dir}/{name}.py is an adapter over serving_model already: nothing independent to record")
    commit = subprocess.check_output(["git", "-C", tests_dir, "rev-parse", "HEAD"], text=True).strip()
    sys.path[:0] = [tests_dir, os.path.dirname(tests_dir)]
    spec = importlib.util.spec_from_file_location("decode_ref_anchor_cases", os.path.join(HERE, "decode_ref_anchor_cases.py"))
    cases = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cases)
    assert all(sys.modules[name].__file__.startswith(tests_dir) for name in REF_MODULES)
    out = {"commit": np.array(commit)}
    for name, fn in cases.CASES.items():
        for field, value in fn().items():
            out[name + "/" + field] = np.asarray(value)
        print(name, flush=True)
    np.savez_compressed(args.out, **out)
    print("%s: %d arrays of %d cases, %d bytes, from %s" % (args.out, len(out) - 1, len(cases.CASES), os.path.getsize(args.out),
                                                            commit))


if __name__ == "__main__":
    main()
