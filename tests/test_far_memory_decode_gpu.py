"""Far-address tests of the 18 decode entry points (tests/decode_validation_cases.py::ENTRIES: three shapes x six
flavours) in the three cache layouts: the K and V caches are views whose rows lie beyond 2^31 elements from the cache
pointer (tests/far_memory.py: the tables, the arena and why running them is safe; tests/test_far_memory_cpu.py: the proof,
without a GPU), and the call must give what the same call gives on small caches that hold the same rows.

  SFA_KV_BLMHD, SFA_KV_BLHMD   caches [B, L, M, Hkv, D] with L so large that (b * L + idx_layer) * M * Hkv * D exceeds
                               2^31 + 2^20 for b = B - 1, idx_layer = L - 1; the compact twin has L = 1
  SFA_KV_PAGED                 a pool of more than 2^31 elements, page_size 16; the block tables name its highest pages and
                               hold -1 behind the last page a sequence touches; the compact twin is a pool of 67 pages

K and V come out of one arena, V right behind K, so K is V's guard.  Only the rows a case uses are written: the histories
and, behind them, the rows the call appends plus 16 more, filled with a sentinel.

Every case asserts: o bit-identical to the compact call's; the appended K and V rows, read back from the far cache, equal
to the compact cache's (and, 16-bit, to the input bits: no bias, no rotation); the 16 rows behind them still the sentinel;
a clean status word; and the compact call within the family's tolerance of its reference -- sinks_ref.
decode_window_sinks_ref token by token for the 16-bit entry points (window None and sinks None give the plain calls'
oracle.decode_ref attention), kv8_sinks_ref.attend_sinks over the bytes the device stored for the fp8 ones, as
tests/test_decode_kv8_sinks_gpu.py checks them.  The operators are the package's (starflashattention_amd.ops): no second
binding.

At the end: the plain flavour of each shape with qkv far -- args->stride = 2^30 and qkv_token_stride = 2^30.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import far_memory as fm
from decode_validation_cases import ENTRIES
from kv8_ref import quantize
from kv8_sinks_ref import attend_sinks
from oracle import round_to
from sinks_ref import decode_window_sinks_ref
from window_ref import TOL

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
TDT = {"fp16": torch.float16, "bf16": torch.bfloat16}
B, H, HKV, M, PS = fm.DEC_B, fm.DEC_HQ, fm.DEC_HKV, fm.DEC_M, fm.DEC_PS
WINDOW, TAIL = fm.DEC_WINDOW, fm.DEC_TAIL
K_SCALE = np.array([2.0 ** -6, 2.0 ** -5], np.float32)     # N(0, 1) rows: |x| / scale stays inside e4m3's +-448
V_SCALE = np.array([2.0 ** -5, 2.0 ** -6], np.float32)
SINKS = np.linspace(2.0, 6.0, H).astype(np.float32)        # material against a log-sum-exp of about 5


@pytest.fixture(scope="module")
def sfa():
    assert torch.cuda.is_available(), "GPU tests need a GPU (run with -m gpu on the MI355X box)"
    import starflashattention_amd as m
    m._lib.load()
    return m


@pytest.fixture(scope="module")
def arena(sfa):
    need = max([fm.decode_arena_bytes(cm) for cm in fm.decode_cache_maps().values()] +
               [fm.qkv_placement(n).arena_bytes() for n in fm.QKV_CASES])
    a = fm.Arena(need + 2 ** 20, DEV)
    yield a
    a.free()
    sfa.release_workspaces()
    torch.cuda.empty_cache()


# ---- the problem --------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def problem(lens, ns, D, dtype, kv8):
    """q [T, H, D], k_new / v_new [T, Hkv, D] float32 representable in dtype, and per sequence the history K / V
    [pos, Hkv, D]: float32 representable in dtype, or e4m3 codes"""
    rng = np.random.default_rng(sum(lens) * 31 + sum(ns) * 7 + D + kv8)
    r16 = lambda *s: round_to(rng.standard_normal(s), dtype).astype(np.float32)
    T = sum(ns)
    q, kn, vn = r16(T, H, D), r16(T, HKV, D), r16(T, HKV, D)
    hist = [(r16(pos, HKV, D), r16(pos, HKV, D)) for pos in lens]
    if kv8:
        hist = [(quantize(k, K_SCALE), quantize(v, V_SCALE)) for k, v in hist]
    return q, kn, vn, hist


def reference(e, lens, ns, D, dtype, stored):
    """o [T, H, D] of the family's reference.  stored: per sequence the (K, V) rows [pos + n, Hkv, D] of the cache after the
    call -- floats, or for the fp8 entry points the bytes the device stored"""
    q, kn, vn, _ = problem(lens, ns, D, dtype, e.kv8)
    window, sinks = (WINDOW if e.window else None), (SINKS if e.sinks else None)
    out = np.zeros((sum(ns), H, D), np.float64)
    r = 0
    for b, (pos, n) in enumerate(zip(lens, ns)):
        K, V = stored[b]
        if e.kv8:
            o, _ = attend_sinks(q[r:r + n].astype(np.float64), K, V, pos, window, sinks, K_SCALE, V_SCALE)
            out[r:r + n] = o
        else:
            for t in range(n):
                ref = decode_window_sinks_ref(q[r + t][None], kn[r + t][None], vn[r + t][None], K[None, None], V[None, None],
                                              [pos + t], 0, 0, window, sinks, dtype)
                out[r + t] = ref["o64"][0]
        r += n
    return out


# ---- caches in a layout, compact or far ---------------------------------------------------------------------------------

class Cache:
    def __init__(self, cm, dt, arena=None, base=None):
        self.cm, self.dt = cm, dt
        if arena is None:
            self.t = torch.empty(cm.shape, dtype=dt, device=DEV)
            bits = self.t.view(torch.int16 if cm.itemsize == 2 else torch.uint8)
            bits.fill_(fm.SENTINEL if cm.itemsize == 2 else fm.SENTINEL & 0xFF)
        else:
            assert cm.safe_in(arena.nbytes, base) and (base * cm.itemsize) % 16 == 0
            strides = [1]
            for n in reversed(cm.shape[1:]):
                strides.insert(0, strides[0] * n)
            self.t = torch.as_strided(arena.typed(dt), cm.shape, strides, storage_offset=base)
            assert self.t.is_contiguous()
        self.table = None if cm.layout != "paged" else torch.from_numpy(cm.table).to(DEV)

    def _index(self, b, r0, r1):
        cm = self.cm
        rows = torch.arange(r0, r1, device=DEV)
        pages = self.table[b].long()[rows // PS]
        assert int(pages.min()) >= 0
        return pages, rows % PS

    def write(self, b, r0, data):
        """rows r0 .. of sequence b <- data [n, Hkv, D]"""
        cm, n = self.cm, data.shape[0]
        if cm.layout == "blmhd":
            self.t[b, cm.layer, r0:r0 + n] = data
        elif cm.layout == "blhmd":
            self.t[b, cm.layer, :, r0:r0 + n] = data.permute(1, 0, 2)
        else:
            pages, slots = self._index(b, r0, r0 + n)
            self.t[pages, cm.layer, slots] = data

    def read(self, b, r0, r1):
        cm = self.cm
        if cm.layout == "blmhd":
            return self.t[b, cm.layer, r0:r1].clone()
        if cm.layout == "blhmd":
            return self.t[b, cm.layer, :, r0:r1].permute(1, 0, 2).contiguous()
        pages, slots = self._index(b, r0, r1)
        return self.t[pages, cm.layer, slots]


def bits(t):
    return t.view(torch.int16) if t.element_size() == 2 else t.view(torch.uint8)


def sentinel(n, D, dt):
    if dt == torch.uint8:
        return torch.full((n, HKV, D), fm.SENTINEL & 0xFF, dtype=torch.uint8, device=DEV)
    return torch.full((n, HKV, D), fm.SENTINEL, dtype=torch.int16, device=DEV).view(dt)


def to_dev(x, dt):
    if dt == torch.uint8:
        return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dt).to(DEV)


def fill(caches, lens, ns, hist, dt, D):
    for b, (pos, n) in enumerate(zip(lens, ns)):
        for c, rows in zip(caches, hist[b]):
            c.write(b, 0, to_dev(rows, dt))
            c.write(b, pos, sentinel(n + TAIL, D, dt))


def call(sfa, e, qkv, o, kc, vc, lens, ns, D, num_splits):
    """the operator of entry point e on the caches kc, vc (Cache) -> o"""
    cm = kc.cm
    args = [qkv, None, None, None, kc.t, vc.t, torch.tensor(lens, dtype=torch.int32, device=DEV), o]
    if e.varlen:
        args.append(torch.tensor(fm.cu_of(ns), dtype=torch.int32, device=DEV))
    args += [len(lens), M, H, D, 0, M, cm.L, cm.layer]
    if e.window:
        args.append(WINDOW)
    if e.sinks:
        args.append(torch.from_numpy(SINKS).to(DEV))
    kw = dict(num_splits=num_splits, kv_layout=cm.layout, num_heads_kv=HKV)
    if cm.layout == "paged":
        kw["block_table"] = kc.table
    if e.kv8:
        kw.update(k_scale=torch.from_numpy(K_SCALE).to(DEV), v_scale=torch.from_numpy(V_SCALE).to(DEV))
    getattr(sfa, e.name.replace("sfa_decode", "flash_decode"))(*args, **kw)
    sfa.check_decode_status(DEV)            # synchronises; raises unless the status word is clean
    return o


def operands(e, lens, ns, D, dtype):
    q, kn, vn, hist = problem(lens, ns, D, dtype, e.kv8)
    qkv = torch.cat([to_dev(x, TDT[dtype]) for x in (q, kn, vn)], dim=1)                # [T, H + 2 Hkv, D]
    o_shape = (sum(ns), H, D)
    if e.shape == "_chunk":
        qkv, o_shape = qkv.view(len(lens), ns[0], H + 2 * HKV, D), (len(lens), ns[0], H, D)
    return qkv.contiguous(), o_shape, kn, vn, hist


def check_caches(e, far, small, lens, ns, kn, vn, dtype, D):
    """appended rows equal (and the input's bits, 16-bit), the TAIL rows behind them the sentinel; returns the rows the
    compact caches hold per sequence, for the reference"""
    dt = torch.uint8 if e.kv8 else TDT[dtype]
    stored, r = [], 0
    for b, (pos, n) in enumerate(zip(lens, ns)):
        per = []
        for fc, sc, new in ((far[0], small[0], kn), (far[1], small[1], vn)):
            got, want = fc.read(b, 0, pos + n + TAIL), sc.read(b, 0, pos + n + TAIL)
            assert torch.equal(bits(got[:pos]), bits(want[:pos])), "the call changed a history row"
            assert torch.equal(bits(got[pos:pos + n]), bits(want[pos:pos + n])), "appended rows differ from the compact cache's"
            assert torch.equal(bits(got[pos + n:]), bits(sentinel(TAIL, D, dt))), "a row behind the appended ones was written"
            assert torch.equal(bits(want[pos + n:]), bits(sentinel(TAIL, D, dt)))
            if not e.kv8:
                assert torch.equal(bits(got[pos:pos + n]), bits(to_dev(new[r:r + n], dt))), "appended rows are not the input's"
                per.append(want[:pos + n].float().cpu().numpy())
            else:
                per.append(want[:pos + n].cpu().numpy())
        stored.append(per)
        r += n
    return stored


def run_pair(sfa, arena, e, layout, D, dtype, num_splits, lens=fm.DEC_LENS, ns=None):
    ns = ns or ((1,) * len(lens) if e.single else fm.DEC_VARLEN_NS if e.varlen else (fm.DEC_N,) * len(lens))
    dt = torch.uint8 if e.kv8 else TDT[dtype]
    isz = 1 if e.kv8 else 2
    qkv, o_shape, kn, vn, hist = operands(e, lens, ns, D, dtype)
    cm_far, cm_small = fm.CacheMap(layout, D, isz, True), fm.CacheMap(layout, D, isz, False)
    far = [Cache(cm_far, dt, arena, fm.GUARD), Cache(cm_far, dt, arena, fm.GUARD + cm_far.elems)]
    small = [Cache(cm_small, dt), Cache(cm_small, dt)]
    outs = []
    for caches in (far, small):
        fill(caches, lens, ns, hist, dt, D)
        o = torch.full(o_shape, 7.0, dtype=TDT[dtype], device=DEV)
        outs.append(call(sfa, e, qkv, o, caches[0], caches[1], lens, ns, D, num_splits))
    assert torch.equal(bits(outs[0]), bits(outs[1])), "o differs from the compact call's"
    stored = check_caches(e, far, small, lens, ns, kn, vn, dtype, D)
    want = reference(e, lens, ns, D, dtype, stored)
    got = outs[1].float().cpu().numpy().reshape(want.shape)
    np.testing.assert_allclose(got, want, atol=TOL[dtype], rtol=TOL[dtype])


def cases():
    out = []
    for i, e in enumerate(ENTRIES):
        for j, layout in enumerate(fm.DEC_LAYOUTS):
            for S in (1, 2):
                dtype = ("fp16", "bf16")[(i + j + S) % 2]
                out.append(pytest.param(e, layout, 128, dtype, S, id="%s-%s-%s-splits%d" % (e.name, layout, dtype, S)))
    # head_dim 64 over the fp8 cache
    e = next(x for x in ENTRIES if x.name == "sfa_decode_chunk_kv8_window")
    out += [pytest.param(e, layout, 64, "bf16", 2, id="%s-%s-D64-bf16-splits2" % (e.name, layout)) for layout in fm.DEC_LAYOUTS]
    return out


def test_the_table_is_the_eighteen_entry_points():
    assert len(ENTRIES) == 18 and len({e.name for e in ENTRIES}) == 18


@pytest.mark.parametrize("e,layout,D,dtype,num_splits", cases())
def test_far_cache(sfa, arena, e, layout, D, dtype, num_splits):
    run_pair(sfa, arena, e, layout, D, dtype, num_splits)


# ---- qkv with a far stride -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(fm.QKV_CASES))
def test_far_qkv_stride(sfa, arena, name):
    """The plain flavour of each shape with its qkv rows 2^30 elements apart, against the same call on packed rows.  The
    operators take packed qkv only, so the call is made as decode_cases.Run.call_exact_workspace makes it: the package's
    own argument marshalling (ops._decode_args), then the pointer and the strides of the far view."""
    from starflashattention_amd import _lib, ops
    c = fm.QKV_CASES[name]
    e = next(x for x in ENTRIES if x.name == "sfa_decode" + c["call"])
    D, dtype, layout = 128, "bf16", "blmhd"
    lens, ns, nb = c["lens"], c["ns"], c["B"]
    p = fm.qkv_placement(name, D)
    qkv, o_shape, kn, vn, hist = operands(e, lens, ns, D, dtype)
    far_qkv = arena.view(p, TDT[dtype])
    far_qkv.copy_(qkv.view(far_qkv.shape))
    lib = _lib.load()
    outs, caches = [], []
    for view in (far_qkv, None):
        cm = fm.CacheMap(layout, D, 2, False, B=nb, lens=lens, n=max(ns))
        kc, vc = Cache(cm, TDT[dtype]), Cache(cm, TDT[dtype])
        fill((kc, vc), lens, ns, hist, TDT[dtype], D)
        o = torch.full(o_shape, 7.0, dtype=TDT[dtype], device=DEV)
        sl = torch.tensor(lens, dtype=torch.int32, device=DEV)
        cu = torch.tensor(fm.cu_of(ns), dtype=torch.int32, device=DEV)
        a, *_ = ops._decode_args(qkv, None, None, None, kc.t, vc.t, sl, o, nb, M, H, D, 0, M, cm.L, cm.layer, None, None, None,
                                 layout, None, HKV, tokens=ns[0] if e.shape == "_chunk" else None,
                                 packed=sum(ns) if e.varlen else None)
        stride, tok = (H + 2 * HKV) * D if e.single else 0, 0
        if view is not None:
            a.qkv = view.data_ptr()
            if name.endswith("batch"):
                stride = fm.QKV_STRIDE
            else:
                tok = fm.QKV_STRIDE
        T = sum(ns)
        if e.single:
            S = lib.sfa_decode_auto_splits(nb, HKV, D, M)
            ws = ops._workspace(DEV, lib.sfa_decode_workspace_bytes(nb, H, D, M, S))
            extra = []
        elif e.varlen:
            S = 0
            ws = ops._workspace(DEV, lib.sfa_decode_varlen_workspace_bytes(nb, H, HKV, D, M, T, 0))
            extra = [ctypes.c_void_p(cu.data_ptr()), T, tok]
        else:
            S = 0
            ws = ops._workspace(DEV, lib.sfa_decode_chunk_workspace_bytes(nb, H, HKV, D, M, ns[0], 0))
            extra = [ns[0], tok]
        with torch.cuda.device(DEV):
            ops._call_decode(DEV, a, stride, S, ws, getattr(lib, e.name), extra)
        sfa.check_decode_status(DEV)
        outs.append(o)
        caches.append((kc, vc))
    assert torch.equal(bits(outs[0]), bits(outs[1])), "o differs from the packed call's"
    stored = check_caches(e, caches[0], caches[1], lens, ns, kn, vn, dtype, D)
    want = reference(e, lens, ns, D, dtype, stored)
    np.testing.assert_allclose(outs[1].float().cpu().numpy().reshape(want.shape), want, atol=TOL[dtype], rtol=TOL[dtype])
