"""Long-context decode: all 18 entry points at memory_max_len 32768 and 131072 against tests/serving_model.py (DESIGN.md
5.27).  The cases, their inputs and the rules are in tests/long_context_cases.py; tests/test_long_context_cpu.py holds the
conditions on the inputs on the reference alone.

Sections A and B (test_long_context): one call per case on a cache whose background is built once per (M, Hkv, D, L,
storage type) and copied on the device for every case, checked by Device._check as it stands -- every byte outside the
appended rows unchanged, appended V exact, appended K within the existing rule, o within the project's TOL of the model over
the bits the device stored, a clean status.  Nothing is loosened for length.

Section C (in-kernel trigonometry at far positions): the appended K rows of probe tokens hold the device's cos / sin; they
must lie in the 2-ulp envelope of inv_freq, be bit-identical across the copies of the recipe, and agree with
sfa_compute_rotary_table; fp8 rows lie between the codes of the envelope's extremes.
"""
import numpy as np
import pytest
import torch

import long_context_cases as lc
import serving_cases as sc
import serving_model as sm
from chunk_window_ref import ULP
from oracle import from_bits16
from serving_device import Device, FILL, TDT, TOL

pytestmark = pytest.mark.gpu

_BACKGROUND = {}        # (bg_key, layout, page size, "kc" / "vc") -> the background cache on the device, in that layout


@pytest.fixture(scope="module")
def sfa():
    assert torch.cuda.is_available(), "GPU tests need a GPU (run with -m gpu on the MI355X box)"
    import starflashattention_amd as m
    m._lib.load()
    yield m
    _BACKGROUND.clear()


class LongDevice(Device):
    """Device over a materialised long-context case: the tokens are the case's own, and the device caches are a copy of the
    background's device tensor with the planted rows written in, so that every case starts from the same bits whatever ran
    before it."""

    def __init__(self, case, m):
        self.case, self.m = case, m
        self.tokens = m["tokens"]
        super().__init__(m["trace"], m["data"])

    def to_device(self, bits, rng):
        g, c = self.g, self.case
        name = "kc" if bits is self.data["kc"] else "vc"
        key = (lc.bg_key(c), g["layout"], g["ps"], name)
        if key not in _BACKGROUND:
            for k in [k for k in _BACKGROUND if k[0] != key[0]]:        # one background at a time stays on the device
                del _BACKGROUND[k]
            _BACKGROUND[key] = super().to_device(lc.background(key[0])[name], rng)
        t = _BACKGROUND[key].clone()
        if c["section"] == "C" and name == "kc":
            t[..., :c["rot"]] = 0
        layer, ps = g["layer"], g["ps"]
        for b in range(g["B"]):
            rows = self.m["visible"][b] + ([self.m["below"][b]] if self.m["below"][b] is not None else [])
            if not rows or self.case["n"][b] == 0:
                continue
            r = torch.tensor(rows, dtype=torch.int64)
            src = self._tensor(bits[b, layer, rows]).to(self.dev)                # [rows, Hkv, D]
            if g["layout"] == "blmhd":
                t[b, layer, r.to(self.dev)] = src
            elif g["layout"] == "blhmd":
                t[b, layer, :, r.to(self.dev)] = src.permute(1, 0, 2)
            else:
                pages = torch.from_numpy(self.table[b, np.asarray(rows) // ps].astype(np.int64)).to(self.dev)
                t[pages, layer, (r % ps).to(self.dev)] = src
        return t

    def check_invariant(self, call, a, before, after):
        """Device._check for a rotation-invariant problem (section C), where the model's angle is not the contract: the same
        unchanged bytes, exact V rows and o (finite, nothing written past the last token, within TOL of the model over the
        bits the device stored); the appended K rows against the far-position envelope instead of the model's own angle.
        Steps (1) and (3) must track serving_device.Device._check."""
        g = self.g
        dtype, layer, kv8, H, Hkv = g["dtype"], g["layer"], g["kv8"], g["H"], g["Hkv"]
        m = self.appended(call)
        for name, x, y in (("k", before[0], after[0]), ("v", before[1], after[1])):
            changed = (self.raw(x) != self.raw(y)) & ~m
            assert not bool(changed.any()), f"{name} cache: {int(changed.sum())} elements outside the appended rows changed"
        cb = (self.canonical(before[0]), self.canonical(before[1]))
        ca = (self.canonical(after[0]), self.canonical(after[1]))
        mc = sc.model_call(g, call, self.data, a["tokens"])
        app, attend = sm.step(cb, mc)
        for b, (pos, n) in enumerate(zip(call["pos"], call["n"])):
            for t in range(n):
                kd, vd = ca[0][b, layer, pos + t], ca[1][b, layer, pos + t]
                np.testing.assert_array_equal(vd, app["v_bits"][b][t], err_msg=f"sequence {b}: appended V rows")
                k = np.asarray(a["tokens"][b][t, H:H + Hkv], np.float64)
                if kv8:
                    lc.check_k_bytes_envelope(kd, k, pos + t, g["rot"], dtype, self.data["k_scale"])
                else:
                    lc.check_k_row_envelope(from_bits16(kd, dtype).astype(np.float64), k, pos + t, g["rot"], dtype, ULP[dtype])
        o = a["o"].float().cpu().numpy()
        cu = np.concatenate([[0], np.cumsum(call["n"])])
        o_list = list(o) if call["shape"] == "_chunk" else [o[cu[b]:cu[b + 1]] for b in range(g["B"])]
        if call["shape"] != "_chunk":
            assert np.all(o[sum(call["n"]):] == FILL), "rows of o past the last token were written"
        want = attend(*ca)
        for b, n in enumerate(call["n"]):
            if n:
                assert np.isfinite(o_list[b]).all(), f"sequence {b}: o is not finite"
                print("sequence %d: max |o - ref| = %.3e (tol %.1e)" % (b, np.abs(o_list[b] - want[b]).max(), TOL[dtype]))
                np.testing.assert_allclose(o_list[b], want[b], atol=TOL[dtype], rtol=TOL[dtype], err_msg=f"sequence {b}")

    def launch(self, sfa, call, a):
        """Device.launch with long_context_cases.check_preconditions, which admits head_dim 256 where the header does.  The
        rest is Device.launch's body and must track serving_device.py."""
        g = self.g
        lc.check_preconditions(g, call, self.table, self.data["k_scale"], self.data["v_scale"])
        pos_args = [a["qkv"], *self.biases, self.kc, self.vc, a["seq_len"], a["o"]]
        if call["shape"] == "_varlen":
            pos_args.append(a["cu"])
        pos_args += [g["B"], g["M"], g["H"], g["D"], g["rot"], g["M"], g["L"], g["layer"]]
        if call["window"] is not None:
            pos_args.append(call["window"])
        if call["flavour"] == "_window_sinks":
            pos_args.append(a["sinks"])
        ret = getattr(sfa, call["entry"])(*pos_args, num_splits=call["num_splits"], softmax_scale=call["softmax_scale"],
                                          **self.kw)
        assert ret.data_ptr() == a["o"].data_ptr()

    def prepare(self, call):
        """Device.prepare with the case's tokens in place of the seeded ones (the only difference: it must track
        serving_device.py)"""
        g = self.g
        H, Hkv, D, B = g["H"], g["Hkv"], g["D"], g["B"]
        tok = self.tokens
        heads = (3, H, D) if g["G"] == 1 else (H + 2 * Hkv, D)
        total = sum(call["n"])
        if call["shape"] == "_chunk":
            x, lead = np.stack(tok), (B, call["n"][0])
        else:
            x = np.concatenate(list(tok) + [np.zeros((0 if total else 1, H + 2 * Hkv, D), np.float32)])
            lead = (x.shape[0],)
        qkv = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(self.dt).view(lead + heads).to(self.dev)
        o = torch.full(lead + (H, D), FILL, dtype=self.dt, device=self.dev)
        args = dict(qkv=qkv, o=o, tokens=tok, seq_len=torch.tensor(call["pos"], dtype=torch.int32, device=self.dev))
        if call["shape"] == "_varlen":
            args["cu"] = torch.tensor(np.concatenate([[0], np.cumsum(call["n"])]), dtype=torch.int32, device=self.dev)
        if call["sinks"] is not None:
            args["sinks"] = torch.tensor(call["sinks"], dtype=torch.float32, device=self.dev)
        return args


def test_the_device_copy_of_a_case_is_its_canonical_cache(sfa):
    """LongDevice's cached background plus planted rows is bit for bit what the model starts from, in every layout"""
    seen = set()
    for c in lc.CASES:
        if c["M"] == 32768 and c["Hkv"] == 1 and (c["layout"], c["ps"]) not in seen:
            seen.add((c["layout"], c["ps"]))
            m = lc.materialise(c)
            d = LongDevice(c, m)
            np.testing.assert_array_equal(d.canonical(d.kc), m["data"]["kc"])
            np.testing.assert_array_equal(d.canonical(d.vc), m["data"]["vc"])
    assert len(seen) == 4


@pytest.mark.parametrize("case", lc.CASES, ids=lc.case_id)
def test_long_context(sfa, case):
    m = lc.materialise(case)
    call = m["call"]
    if case["num_splits"] == 0:         # the library's own choice, from its exported host functions: above 1 unless the window is 1
        S = lc.auto_splits(sfa._lib.load(), case)
        print("auto splits:", S)
        assert (S == 1) == (case["window"] == 1), S
    sfa.check_decode_status()
    d = LongDevice(case, m)
    a = d.prepare(call)
    before = d.snapshot()
    d.launch(sfa, call, a)
    torch.cuda.synchronize()
    d.check(call, a, before, (d.kc, d.vc))
    sfa.check_decode_status()


@pytest.mark.parametrize("case", lc.INVARIANT_CASES, ids=lc.case_id)
def test_q_and_k_are_rotated_at_the_same_position(sfa, case):
    """section C, rotation-invariant problems with the trigonometry in the kernel: o needs no tolerance for the angle"""
    m = lc.materialise(case)
    call = m["call"]
    sfa.check_decode_status()
    d = LongDevice(case, m)
    a = d.prepare(call)
    before = d.snapshot()
    d.launch(sfa, call, a)
    torch.cuda.synchronize()
    try:
        d.check_invariant(call, a, before, (d.kc, d.vc))
    except AssertionError as e:
        raise AssertionError(f"case {case!r}\n{e}") from None
    sfa.check_decode_status()


# ---- section C: the angle probe -----------------------------------------------------------------------------------------

PROBE_HKV, PROBE_D = 1, 64
# (name, entry shape, windowed, G): G = 1 decode_kernel, G = 2 decode_gqa_kernel, G = 8 the matrix-core body (decode_dispatch.hip)
PROBE_ENTRIES = (("decode_g1", "", False, 1), ("decode_g2", "", False, 2), ("decode_g8", "", False, 8),
                 ("window", "", True, 2), ("chunk_n1", "_chunk", False, 2), ("chunk_n4", "_chunk", False, 2),
                 ("varlen", "_varlen", False, 2))


def run_probe(sfa, name, shape, windowed, G, dtype, rot, kv8):
    """One call with probe tokens on a zeroed blmhd cache, one sequence per probe position.  Returns {position: the appended K
    row [Hkv, D]} (float values of a 16-bit cache, bytes of an fp8 one).  chunk_n4: sequence b starts 3 rows before its
    probe position where there are that many, so token t lands on p - 3 + t; every token's row is a probe of its own row."""
    Hkv, D, M, dev = PROBE_HKV, PROBE_D, lc.PROBE_M, torch.device("cuda:0")
    H, n = Hkv * G, 4 if name == "chunk_n4" else 1
    P = lc.PROBE_POSITIONS
    Bp = len(P)
    pos = [max(p - (n - 1), 0) for p in P]
    tok = lc.probe_tokens(n, H, Hkv, D, rot, dtype)
    x = np.broadcast_to(tok[None], (Bp,) + tok.shape)
    lead = (Bp, n) if shape == "_chunk" else (Bp * n,)
    heads = (3, H, D) if G == 1 else (H + 2 * Hkv, D)
    qkv = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(TDT[dtype]).view(lead + heads).to(dev)
    o = torch.full(lead + (H, D), FILL, dtype=TDT[dtype], device=dev)
    cdt = torch.uint8 if kv8 else TDT[dtype]
    kc, vc = (torch.zeros((Bp, 1, M, Hkv, D), dtype=cdt, device=dev) for _ in range(2))
    seq_len = torch.tensor(pos, dtype=torch.int32, device=dev)
    entry = sc.entry_name(shape, "_window" if windowed else "", kv8)
    geo = dict(B=Bp, M=M, ps=16, stride=M // 16, num_pages=Bp * M // 16, kv8=kv8, G=G, H=H, Hkv=Hkv, D=D, rot=rot, L=1, layer=0)
    call = dict(entry=entry, shape=shape, flavour="_window" if windowed else "", pos=pos, n=[n] * Bp,
                window=4096 if windowed else None, sinks=None, softmax_scale=None, num_splits=0)
    k_scale = np.asarray(lc.K_SCALE[:Hkv], np.float32) if kv8 else None
    sc.check_preconditions(geo, call, np.arange(Bp * M // 16, dtype=np.int32).reshape(Bp, -1), k_scale, k_scale)
    args = [qkv, None, None, None, kc, vc, seq_len, o]
    if shape == "_varlen":
        args.append(torch.arange(Bp + 1, dtype=torch.int32, device=dev) * n)
    args += [Bp, M, H, D, rot, M, 1, 0]
    if windowed:
        args.append(call["window"])
    kw = dict(num_heads_kv=Hkv)
    if kv8:
        kw.update(k_scale=torch.from_numpy(k_scale).to(dev), v_scale=torch.from_numpy(k_scale).to(dev))
    getattr(sfa, entry)(*args, **kw)
    torch.cuda.synchronize()
    sfa.check_decode_status()
    rows = {}
    for b in range(Bp):
        for t in range(n):
            r = kc[b, 0, pos[b] + t].cpu()
            rows[pos[b] + t] = r.numpy() if kv8 else from_bits16(r.view(torch.int16).numpy().view(np.uint16), dtype)
    return rows


@pytest.mark.parametrize("rot", (PROBE_D, PROBE_D // 2))
@pytest.mark.parametrize("dtype", ("fp16", "bf16"))
def test_the_angle_probe_16bit(sfa, dtype, rot):
    """every copy of the recipe, at positions 0 .. 131071: inside the envelope, bit-identical to each other and to
    sfa_compute_rotary_table at max_seq_len 131072"""
    table = sfa.compute_rotary_table(lc.PROBE_M, rot, dtype=TDT[dtype])
    cos, sin = (t.float().cpu().numpy() for t in table)
    first = None
    for name, shape, windowed, G in PROBE_ENTRIES:
        rows = run_probe(sfa, name, shape, windowed, G, dtype, rot, False)
        for p, row in rows.items():
            lc.check_probe_row(row[0].astype(np.float64), p, rot, dtype)
        at = {p: rows[p] for p in lc.PROBE_POSITIONS}
        if first is None:
            first = at
            for p in lc.PROBE_POSITIONS:
                np.testing.assert_array_equal(at[p][0, 0:rot:2], cos[p], err_msg=f"cos table row {p}")
                np.testing.assert_array_equal(at[p][0, 1:rot:2], sin[p], err_msg=f"sin table row {p}")
        for p in lc.PROBE_POSITIONS:
            np.testing.assert_array_equal(at[p], first[p], err_msg=f"{name} against {PROBE_ENTRIES[0][0]} at position {p}")


@pytest.mark.parametrize("rot", (PROBE_D, PROBE_D // 2))
@pytest.mark.parametrize("dtype", ("fp16", "bf16"))
def test_the_angle_probe_kv8(sfa, dtype, rot):
    for name, shape, windowed, G in PROBE_ENTRIES:
        rows = run_probe(sfa, name, shape, windowed, G, dtype, rot, True)
        for p, row in rows.items():
            lc.check_probe_bytes(row, p, rot, dtype, np.asarray(lc.K_SCALE[:PROBE_HKV], np.float32))
