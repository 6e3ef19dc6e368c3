"""The device side of a serving trace, for tests/test_serving_trace_gpu.py and tests/test_long_context_gpu.py: class Device
runs any of the 18 decode entry points in any layout on caches it keeps on the GPU, and checks a call against
tests/serving_model.py -- unchanged bytes, appended rows, o (the rules are in tests/test_serving_trace_gpu.py's header).
"""
import numpy as np
import torch

import kv8_ref
import serving_cases as sc
import serving_model as sm
from chunk_window_ref import ULP
from oracle import from_bits16
from window_ref import TOL          # the project's decode tolerances, atol = rtol

TDT ={"fp16": torch.float16, "bf16": torch.bfloat16}
FILL = 7.0                                      # what o holds before a call


class Device:
    """The device side of one trace: both caches in the trace's layout, and the constant arguments of its calls."""

    def __init__(self, trace, data, kc=None, vc=None):
        self.g = g = trace["geo"]
        self.trace, self.data = trace, data
        self.dev = torch.device("cuda:0")
        self.dt = TDT[g["dtype"]]
        self.need = g["M"] // g["ps"]
        self.table = trace["table"]
        self.own = torch.from_numpy(self.table[:, :self.need].reshape(-1).astype(np.int64))
        rng = np.random.default_rng([12, int(g["kv8"]), g["seed"]])
        self.kc = self.to_device(data["kc"] if kc is None else kc, rng)
        self.vc = self.to_device(data["vc"] if vc is None else vc, rng)
        t16 = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(self.dt).to(self.dev)
        f32 = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(self.dev)
        self.biases = tuple(t16(data[k]) for k in ("q_bias", "k_bias", "v_bias"))
        self.kw = dict(kv_layout=g["layout"], num_heads_kv=g["Hkv"])
        if g["layout"] == "paged":
            self.kw["block_table"] = torch.from_numpy(self.table).to(self.dev)
        if g["tables"]:
            self.kw.update(rotary_cos_table=t16(data["cos"]), rotary_sin_table=t16(data["sin"]))
        if g["kv8"]:
            self.kw.update(k_scale=f32(data["k_scale"]), v_scale=f32(data["v_scale"]))
        self.k_same = self.k_total = 0          # K bytes identical to the reference quantiser's, over the whole trace

    # ---- layouts: canonical bits [B, L, M, Hkv, D] (numpy) <-> the device tensor ----
    def _tensor(self, bits):
        if bits.dtype == np.uint8:
            return torch.from_numpy(np.ascontiguousarray(bits))
        return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).view(self.dt)

    def to_device(self, bits, rng):
        g = self.g
        t = self._tensor(bits)
        if g["layout"] == "blhmd":
            t = t.permute(0, 1, 3, 2, 4).contiguous()
        elif g["layout"] == "paged":    # the pages no row of a sequence can reach hold random bits (NaN patterns among them)
            shape = (g["num_pages"], g["L"], g["ps"], g["Hkv"], g["D"])
            pool = self._tensor(rng.integers(0, 256 if g["kv8"] else 65536, shape).astype(bits.dtype))
            pool[self.own] = (t.view(g["B"], g["L"], self.need, g["ps"], g["Hkv"], g["D"]).permute(0, 2, 1, 3, 4, 5)
                              .reshape(-1, g["L"], g["ps"], g["Hkv"], g["D"]))
            t = pool
        return t.to(self.dev)

    def raw(self, t):
        """the tensor's bits as an integer tensor"""
        return t if t.dtype == torch.uint8 else t.view(torch.int16)

    def canonical(self, t):
        g = self.g
        t = self.raw(t).cpu()
        if g["layout"] == "blhmd":
            t = t.permute(0, 1, 3, 2, 4)
        elif g["layout"] == "paged":
            t = (t[self.own].view(g["B"], self.need, g["L"], g["ps"], g["Hkv"], g["D"]).permute(0, 2, 1, 3, 4, 5)
                 .reshape(g["B"], g["L"], g["M"], g["Hkv"], g["D"]))
        a = t.contiguous().numpy()
        return a if a.dtype == np.uint8 else a.view(np.uint16)

    def appended(self, call):
        """bool tensor, broadcastable against a device cache: True on the rows the call appends"""
        g = self.g
        if g["layout"] == "paged":
            m = np.zeros((g["num_pages"], g["L"], g["ps"], 1, 1), bool)
            for b, (pos, n) in enumerate(zip(call["pos"], call["n"])):
                r = np.arange(pos, pos + n)
                m[self.table[b, r // g["ps"]], g["layer"], r % g["ps"]] = True
        else:
            m = sm.append_mask((g["B"], g["L"], g["M"]), dict(call, layer=g["layer"]))
            m = m[:, :, :, None, None] if g["layout"] == "blmhd" else m[:, :, None, :, None]
        return torch.from_numpy(m).to(self.dev)

    # ---- one call ----
    def prepare(self, call):
        """the device arguments of a call (made before a group of calls is launched, so that nothing but the calls and the
        snapshots sits between them on the stream)"""
        g = self.g
        H, Hkv, D, B = g["H"], g["Hkv"], g["D"], g["B"]
        tok = sc.call_tokens(g, call)
        heads = (3, H, D) if g["G"] == 1 else (H + 2 * Hkv, D)
        total = sum(call["n"])
        if call["shape"] == "_chunk":
            x, lead = np.stack(tok), (B, call["n"][0])
        else:
            x = np.concatenate(tok + [np.zeros((0 if total else 1, H + 2 * Hkv, D), np.float32)])
            lead = (x.shape[0],)                # (a packed call with no token at all still gets one row of storage)
        qkv = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(self.dt).view(lead + heads).to(self.dev)
        o = torch.full(lead + (H, D), FILL, dtype=self.dt, device=self.dev)
        args = dict(qkv=qkv, o=o, tokens=tok, seq_len=torch.tensor(call["pos"], dtype=torch.int32, device=self.dev))
        if call["shape"] == "_varlen":
            args["cu"] = torch.tensor(np.concatenate([[0], np.cumsum(call["n"])]), dtype=torch.int32, device=self.dev)
        if call["sinks"] is not None:
            args["sinks"] = torch.tensor(call["sinks"], dtype=torch.float32, device=self.dev)
        return args

    def launch(self, sfa, call, a):
        g = self.g
        sc.check_preconditions(g, call, self.table, self.data["k_scale"], self.data["v_scale"])
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

    def check(self, call, a, before, after):
        """before / after: (k, v) device tensors around the call.  Returns the canonical caches after the call, from the
        device's bits: what the model continues from."""
        try:
            return self._check(call, a, before, after)
        except AssertionError as e:
            raise AssertionError(f"seed {self.g['seed']} step {call['step']}: run_call({call!r})\ngeometry {self.g!r}\n{e}") from None

    def _check(self, call, a, before, after):
        g = self.g
        dtype, layer, kv8 = g["dtype"], g["layer"], g["kv8"]
        # (1) every byte outside the appended rows
        m = self.appended(call)
        for name, x, y in (("k", before[0], after[0]), ("v", before[1], after[1])):
            changed = (self.raw(x) != self.raw(y)) & ~m
            assert not bool(changed.any()), f"{name} cache: {int(changed.sum())} elements outside the appended rows changed"
        # (2) the appended rows against the model
        cb = (self.canonical(before[0]), self.canonical(before[1]))
        ca = (self.canonical(after[0]), self.canonical(after[1]))
        mc = sc.model_call(g, call, self.data, a["tokens"])
        app, attend = sm.step(cb, mc)
        for b, (pos, n) in enumerate(zip(call["pos"], call["n"])):
            if n == 0:
                continue
            kd, vd = ca[0][b, layer, pos:pos + n], ca[1][b, layer, pos:pos + n]
            np.testing.assert_array_equal(vd, app["v_bits"][b], err_msg=f"sequence {b}: appended V rows")
            if kv8:
                got, want = kv8_ref.E4M3[kd], kv8_ref.E4M3[app["k_bits"][b]]
                steps = np.abs(got - want) / kv8_ref.step_at(np.maximum(np.abs(got), np.abs(want)))
                print("sequence %d: K bytes differ by at most %.2f e4m3 steps" % (b, steps.max()))
                assert np.all(steps <= 1.0), f"sequence {b}: an appended K byte is {steps.max()} e4m3 steps off"
                self.k_same += int(np.sum(kd == app["k_bits"][b]))
                self.k_total += kd.size
            else:
                got = from_bits16(kd, dtype)
                err = np.abs(got - app["k16"][b])
                print("sequence %d: max |k - ref| = %.3e" % (b, err.max()))
                assert np.all(err <= ULP[dtype] * np.maximum(1.0, np.abs(got)) * 1.01), f"sequence {b}: appended K rows, {err.max()}"
        # (3) o against the model over the bits the device stored
        o = a["o"].float().cpu().numpy()
        total = sum(call["n"])
        if call["shape"] == "_chunk":
            o_list = list(o)
        else:
            cu = np.concatenate([[0], np.cumsum(call["n"])])
            o_list = [o[cu[b]:cu[b + 1]] for b in range(g["B"])]
            assert np.all(o[total:] == FILL), "rows of o past the last token were written"
        want = attend(*ca)
        tol = TOL[dtype]
        for b, n in enumerate(call["n"]):
            if n == 0:
                continue
            assert np.isfinite(o_list[b]).all(), f"sequence {b}: o is not finite"
            print("sequence %d: max |o - ref| = %.3e (tol %.1e)" % (b, np.abs(o_list[b] - want[b]).max(), tol))
            np.testing.assert_allclose(o_list[b], want[b], atol=tol, rtol=tol, err_msg=f"sequence {b}")
        return ca

    def snapshot(self):
        return self.kc.clone(), self.vc.clone()
