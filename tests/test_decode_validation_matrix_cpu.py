"""The host side of the 18 decode entry points, pinned without a GPU: every case of tests/decode_validation_cases.py -- a
well-formed call of each entry point with fake device pointers, single mutations of it, pairs of mutations (which pin the
order of the checks), "nothing to do", and the split count and workspace layout read off the `need %zu` of the workspace
errors -- returns the status and leaves the sfa_last_error() text recorded in tests/golden/decode_validation_matrix.json.
That file was recorded (tests/golden/make_golden.py decode_validation_matrix) from a library built at the commit before
the decode host path became one pipeline; it is not regenerated from the code under test.  No case reaches a HIP call."""
import ctypes
import json
import os

import pytest
import torch

from conftest import ROOT
from starflashattention_amd import _lib
import decode_validation_cases as dvc

with open(os.path.join(ROOT, "tests", "golden", "decode_validation_matrix.json")) as f:
    GOLDEN = dvc.ungroup(json.load(f))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    _lib.load()
    return ctypes.CDLL(_lib.LIB_PATH)       # a handle of its own: the cases pass explicit ctypes values, no argtypes


def test_the_matrix_covers_the_18_entry_points():
    names = [e.name for e in dvc.ENTRIES]
    assert len(names) == len(set(names)) == 18 and sorted(names) == sorted(GOLDEN)
    assert all(n in _lib.EXPORTED_SYMBOLS for n in names)


@pytest.mark.skipif(torch.cuda.is_available(), reason="calls the entry points with fake device pointers")
@pytest.mark.parametrize("e", dvc.ENTRIES, ids=lambda e: e.name)
def test_status_and_error_text_are_the_recorded_ones(lib, e):
    want = GOLDEN[e.name]
    cases = dvc.cases(lib, e)
    assert sorted(cases) == sorted(want)                    # no case left out, none added without a record
    wrong = []
    for name, spec in cases.items():
        got = list(dvc.call(lib, e, spec))
        if got != want[name]:
            wrong.append((name, got, want[name]))
    assert not wrong, "%d of %d cases differ, the first: %r" % (len(wrong), len(cases), wrong[:3])


@pytest.mark.parametrize("e", dvc.ENTRIES, ids=lambda e: e.name)
def test_the_record_follows_the_documented_order(e):
    """The recorded behaviour itself, spot-checked against the order of checks and the trim rule of DESIGN.md 5.19 (so a
    bad recording cannot pass)"""
    g = GOLDEN[e.name]
    fn = e.name + ": "
    untouched = "sfa_debug_set: knob is NULL"               # what an OK call leaves in sfa_last_error()
    assert all(text.startswith(fn) for status, text in g.values() if status != 0)
    assert all(text == untouched for status, text in g.values() if status == 0)
    assert g["base"][0] == -1 and g["base"][1].startswith(fn + "workspace is NULL (need ")
    assert g["batch_0"] == [0, untouched]
    assert g["args_null"] == [-1, fn + "args is NULL"]
    need = lambda k: int(g[k][1].rsplit("need ", 1)[1].split()[0].rstrip(")"))
    for tag in [k[:-len("null")] for k in g if k.startswith("ws_") and k.endswith("_null")]:
        auto, two = need(tag + "null"), need(tag + "null_splits_2")
        if tag != "ws_w2048_" or not e.single:              # (one token under window 2048: one split)
            assert auto > two                               # the automatic split count is above 2 ... or 1:
        assert need(tag + "tiny_splits_2") == need(tag + "short_splits_2") == two
        assert g[tag + "misaligned_splits_2"] == [-2, fn + "workspace must be 256-byte aligned"]
        # trimmed to one split where the call trims, the automatic count where it does not
        assert (need(tag + "tiny") < two) if e.trims else (need(tag + "tiny") == auto)
    if e.sinks:
        assert g["sinks_misaligned+args_null" if "sinks_misaligned+args_null" in g else "args_null+sinks_misaligned"] == \
            [-1, fn + "args is NULL"]                       # the sink alignment is only checked when args is non-NULL
        assert "sinks" in g["qkv_null+sinks_misaligned"][1]
    if e.kv8:
        scales = fn + "k_scale / v_scale must be 4-byte aligned"
        first = e.varlen                                    # the varlen fp8 calls check the scales before anything else
        assert (g["args_null+k_scale_misaligned"][1] == scales) == first
        assert (g["qkv_null+k_scale_misaligned"][1] == scales) == first
        assert g["k_scale_misaligned+window_0"][1] == scales if e.window else True
        assert ("256" in g["head_dim_256+v_scale_misaligned"][1]) == (not first)
    if e.window:
        assert g["window_0+batch_0"][0] == -2 and "window=0" in g["window_0+batch_0"][1]
    if e.varlen:
        assert g["qkv_null+cu_null"] == [-1, fn + "cu_tokens is NULL"]
        assert g["args_null+cu_null"] == [-1, fn + "args is NULL"]
        assert "qkv" in g["qkv_null+cu_misaligned"][1]
        assert "attention workgroups" in g["varlen_grid"][1]
