"""bench.py's own multi-rank path: `python bench.py --gpus 2` with no launcher starts two
fresh ranks itself (torch.distributed.run children), barriers, takes the max over ranks and prints ONE JSON
line from rank 0.  On the one-GPU test box both ranks share the device (SFA_BENCH_BACKEND=gloo: the
rendezvous and the timing path are the product's, only RCCL is swapped for gloo)."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def run_bench(*extra, env=None):
    e = dict(os.environ, **(env or {}))
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        e.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1",
                        "--no-decode", "--no-cpu-baseline", *extra],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600, env=e, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout            # exactly one JSON line, from rank 0
    return json.loads(lines[0])


def test_bench_two_ranks_self_launch():
    rec = run_bench("--gpus", "2", "--full", env={"SFA_BENCH_BACKEND": "gloo"})
    assert rec["n_gpus"] == 2 and rec["steps"] == 3 and rec["warmup"] == 1
    assert rec["config"]["global_batch"] == 32 and rec["scaling"] == "weak"
    assert rec["unit"] == "TFLOPS" and rec["dtype"] == "bf16" and rec["vs_baseline"] is None
    # two ranks time-share one GPU here: the aggregate is about one GPU's rate, not two
    assert 100.0 < rec["value"] < 2 * 2500.0
    assert abs(rec["tflops_per_gpu"] * 2 - rec["value"]) < 0.02 * rec["value"]
    # BASELINE.json configs[4]'s shard is timed on every rank as well, and every rank's time is in the line
    c5 = rec["config5"]
    assert c5["tflops_total"] > 100.0 and abs(c5["tflops_per_gpu"] * 2 - c5["tflops_total"]) < 0.02 * c5["tflops_total"]
    assert abs(c5["frac_mfma_peak"] - c5["tflops_per_gpu"] / 2500.0) < 1e-3
    assert len(rec["per_rank_ms"]["headline"]) == 2 and len(rec["per_rank_ms"]["config5"]) == 2
    assert all(x > 0 for x in rec["per_rank_ms"]["headline"] + rec["per_rank_ms"]["config5"])
    assert "prefill_w4_kernel" in rec["roofline"]["kernel"] and "prefill_w4_kernel" in c5["kernel"]


def test_bench_single_rank_line(tmp_path):
    """A plain run: the headline only (no supplementary keys without --full), and --dump-outputs writes the last timed
    step's output as float32 .npy files within 64 MB."""
    rec = run_bench("--dump-outputs", str(tmp_path))
    assert rec["n_gpus"] == 1 and rec["config"]["global_batch"] == 16
    assert rec["higher_is_better"] is True and rec["dtype"] == "bf16" and rec["ms_per_step"] > 0
    assert not {"fast_scale_variant", "config5_shard", "decode_roofline", "gemm_calibration", "cpu_baseline"} & set(rec)
    import numpy as np
    heads, sample = np.load(tmp_path / "out_heads.npy"), np.load(tmp_path / "out_sample.npy")
    assert heads.dtype == np.float32 and heads.shape == (8, 4096, 128) and sample.dtype == np.float32
    assert heads.nbytes + sample.nbytes <= 64 << 20
    assert np.isfinite(heads).all() and np.isfinite(sample).all() and heads.std() > 0
    rf = rec["roofline"]
    assert rf["bound"] == "mfma" and rf["peak"] == 2500.0 and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-3
    assert 100.0 < rec["value"] < 2500.0
    assert rf["kernel"] == "prefill_w4_kernel<exact>"           # read back from the dispatcher, not a literal
    assert len(rec["per_rank_ms"]["headline"]) == 1


def test_bench_measures_traffic_live():
    """--measure-traffic: roofline.traffic comes from rocprofv3 --pmc child runs of this very invocation, not from profiles/.
    Q + K + V + O of the headline shape are 2.147e9 B; the kernel re-reads part of K / V (2.9-3.1e9 measured)."""
    import shutil
    if not shutil.which("rocprofv3"):
        pytest.skip("rocprofv3 not on PATH")
    rec = run_bench("--measure-traffic")
    rf = rec["roofline"]
    assert "measured in this run" in rf["traffic_source"], rf["traffic_source"]
    assert 2.147e9 <= rf["traffic"] < 4.5e9
