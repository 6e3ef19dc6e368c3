"""Serving traces: six decode calls of mixed entry points on ONE device cache, 32 seeded traces over a 16-bit cache and 32
over an fp8 cache, against tests/serving_model.py.

A trace draws its geometry once (tests/serving_cases.py: batch, kv heads, group, head_dim, layers and the layer, layout,
page size, memory_max_len, a shuffled block table with spare pages and sometimes a wider stride, rotary dim, tables, bias,
fp8 scales) and then makes six calls, each drawn from the nine entry points of its cache type, with seq_len advancing by
what was appended.  The first three calls go through ops.py on the current stream with no synchronisation between them --
the cached workspace grows and is reused across entry points -- and are checked after the third; the others one at a time.

After each call, nothing exempt:
  * every byte of both device caches outside the appended rows is what it was before the call (other layers, other
    sequences, rows from pos + n on, spare pages, the pages of a wide table no row can reach);
  * the appended rows against the model: 16-bit caches by the rule of chunk_window_ref.check_against_reference (V exact, K
    within one storage ulp), fp8 caches by chunk_kv8_ref.check_bytes (V bytes exact, K within one e4m3 step, more than 98 %
    of the K bytes of the whole trace identical);
  * o finite and within TOL (atol = rtol, elementwise) of the model's attend() over the bits the device stored;
  * then the model continues from the device's bits: a one-ulp difference in K, already checked, cannot turn into an output
    difference two calls later, and no row is adopted before it has been compared.
check_decode_status() is clean at the end.

A failure carries the call's description, a repr-able dict; run_call(that dict) reproduces the call alone.
"""
import numpy as np
import pytest
import torch

import serving_cases as sc
import serving_model as sm
from serving_device import Device, FILL, TDT, TOL  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sfa():
    assert torch.cuda.is_available(), "GPU tests need a GPU (run with -m gpu on the MI355X box)"
    import starflashattention_amd as m
    m._lib.load()
    return m


def run_call(desc, sfa=None):
    """Reproduce one call of a trace alone: the trace is rebuilt from desc["seed"] / desc["kv8"], the model advances the
    cache through the steps before desc["step"] on the CPU, and the call runs on a fresh device cache and is checked."""
    if sfa is None:
        import starflashattention_amd as sfa
    trace = sc.make_trace(desc["seed"], desc["kv8"])
    call = trace["calls"][desc["step"]]
    assert all(call[k] == v or (k == "sinks" and repr(call[k]) == repr(v)) for k, v in desc.items()), (call, desc)
    data = sc.trace_data(trace)
    cache = (data["kc"], data["vc"])
    for c in trace["calls"][:desc["step"]]:
        mc = sc.model_call(trace["geo"], c, data)
        cache = sm.apply(cache, mc, sm.step(cache, mc)[0])
    d = Device(trace, data, *cache)
    a = d.prepare(call)
    before = d.snapshot()
    d.launch(sfa, call, a)
    torch.cuda.synchronize()
    d.check(call, a, before, (d.kc, d.vc))
    sfa.check_decode_status()
    return d, a


def run_trace(sfa, seed, kv8):
    trace = sc.make_trace(seed, kv8)
    sfa.check_decode_status()
    sfa.release_workspaces()            # every trace starts from no workspace: its first calls make it and grow it
    d = Device(trace, sc.trace_data(trace))
    calls = trace["calls"]
    # the first calls: launched back to back, snapshots between them on the same stream, nothing read back before the last
    prepared = [d.prepare(c) for c in calls[:sc.UNSYNCED]]
    snaps = []
    for c, a in zip(calls[:sc.UNSYNCED], prepared):
        snaps.append(d.snapshot())
        d.launch(sfa, c, a)
    snaps.append(d.snapshot())
    torch.cuda.synchronize()
    for i, (c, a) in enumerate(zip(calls[:sc.UNSYNCED], prepared)):
        d.check(c, a, snaps[i], snaps[i + 1])
    for c in calls[sc.UNSYNCED:]:
        a = d.prepare(c)
        before = d.snapshot()
        d.launch(sfa, c, a)
        torch.cuda.synchronize()
        d.check(c, a, before, (d.kc, d.vc))
    sfa.check_decode_status()
    return d


@pytest.mark.parametrize("seed", sc.TRACE_SEEDS)
def test_serving_trace_16bit(sfa, seed):
    run_trace(sfa, seed, False)


@pytest.mark.parametrize("seed", sc.TRACE_SEEDS)
def test_serving_trace_kv8(sfa, seed):
    d = run_trace(sfa, seed, True)
    if d.k_total:
        print("K bytes identical to the reference quantiser over the trace: %.4f of %d" % (d.k_same / d.k_total, d.k_total))
        assert d.k_same / d.k_total > 0.98, (d.k_same, d.k_total)


def test_run_call_reproduces_a_call_alone(sfa):
    """the description a failure prints is enough: a middle step of an fp8 trace, run alone from the model's cache"""
    desc = sc.make_trace(5, True)["calls"][4]
    run_call(eval(repr(desc), {"inf": float("inf")}), sfa)
