"""GPU parity of sfa_decode_chunk (flash_decode_chunk: n new tokens per sequence in one call).

Oracle: oracle.decode_ref called n times on one cache, with qkv[:, t] and seq_len + t -- the semantics the chunk
promises.  Tolerances are those of tests/test_decode_gpu.py: o at 2e-3 (fp16) / 1.6e-2 (bf16) against fp64, the
appended K rows within one storage ulp and >= 98 % exact, appended V rows and every untouched cache byte bit-exact.
"""

import numpy as np
import pytest
import torch

from oracle import decode_ref, rope_interleaved, rotary_table_ref, round_to

pytestmark = pytest.mark.gpu

TOL = {"fp16": 2e-3, "bf16": 1.6e-2}
ULP = {"fp16": 2.0 ** -10, "bf16": 2.0 ** -7}
TDT = {"fp16": torch.float16, "bf16": torch.bfloat16}
DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def sfa():
    assert torch.cuda.is_available(), "GPU tests need a GPU (run with -m gpu on the MI355X box)"
    import starflashattention_amd as m
    m._lib.load()
    return m


def rnd(shape, dtype, rng, scale=1.0):
    return round_to(rng.standard_normal(shape).astype(np.float32) * scale, dtype).astype(np.float32)


def to_dev(x, dtype):
    return torch.from_numpy(np.ascontiguousarray(x)).to(TDT[dtype]).to(DEV)


class Problem:
    """A chunk problem with caches kept in the oracle's BLMHD form (expanded to H heads for the oracle)."""

    def __init__(self, B, H, Hkv, D, L, M, n, lens, dtype, layer=1, rot=None, seed=0, bias=False, lut=False):
        rng = np.random.default_rng(seed)
        self.B, self.H, self.Hkv, self.D, self.L, self.M, self.n = B, H, Hkv, D, L, M, n
        self.G = H // Hkv
        self.lens, self.dtype, self.layer = list(lens), dtype, layer
        self.rot = D if rot is None else rot
        self.q = rnd((B, n, H, D), dtype, rng)
        self.k = rnd((B, n, Hkv, D), dtype, rng)
        self.v = rnd((B, n, Hkv, D), dtype, rng)
        self.kc = rnd((B, L, M, Hkv, D), dtype, rng)
        self.vc = rnd((B, L, M, Hkv, D), dtype, rng)
        self.biases = None
        if bias:
            self.biases = (rnd((H, D), dtype, rng, 0.5), rnd((Hkv, D), dtype, rng, 0.5), rnd((Hkv, D), dtype, rng, 0.5))
        self.tables = rotary_table_ref(M, self.rot, dtype) if lut else None

    def qkv(self):
        if self.G == 1:
            return np.stack([self.q, self.k, self.v], axis=2)                  # [B, n, 3, H, D]
        return np.concatenate([self.q, self.k, self.v], axis=2)                # [B, n, H + 2 Hkv, D]

    def oracle(self):
        """o [B, n, H, D] float32 and the caches after the chunk (Hkv heads), by n decode_ref steps."""
        G = self.G
        kc = np.repeat(self.kc, G, axis=3)
        vc = np.repeat(self.vc, G, axis=3)
        kw = {}
        if self.biases is not None:
            kw = dict(q_bias=self.biases[0], k_bias=np.repeat(self.biases[1], G, 0), v_bias=np.repeat(self.biases[2], G, 0))
        if self.tables is not None:
            kw.update(cos_table=self.tables[0], sin_table=self.tables[1])
        o = np.zeros((self.B, self.n, self.H, self.D), np.float32)
        for t in range(self.n):
            qkv_t = np.stack([self.q[:, t], np.repeat(self.k[:, t], G, 1), np.repeat(self.v[:, t], G, 1)], axis=1)
            r = decode_ref(qkv_t, kc, vc, [s + t for s in self.lens], self.layer, self.rot, dtype=self.dtype, **kw)
            o[:, t] = r["o"]
        return o, kc[:, :, :, ::G], vc[:, :, :, ::G]

    def run(self, sfa, layout="blmhd", page_size=16, num_splits=0, lens=None):
        """-> (o [B,n,H,D], kc, vc in BLMHD form) from the device."""
        dt = self.dtype
        B, L, M, Hkv, D = self.B, self.L, self.M, self.Hkv, self.D
        kw = dict(num_splits=num_splits, kv_layout=layout)
        if self.Hkv != self.H:
            kw["num_heads_kv"] = Hkv
        if self.tables is not None:
            kw.update(rotary_cos_table=to_dev(self.tables[0], dt), rotary_sin_table=to_dev(self.tables[1], dt))
        if layout == "paged":
            P = M // page_size
            perm = np.random.default_rng(7).permutation(B * P).astype(np.int32)
            table = perm.reshape(B, P)
            pool_k = np.zeros((B * P, L, page_size, Hkv, D), np.float32)
            pool_v = np.zeros_like(pool_k)
            for b in range(B):
                for i in range(P):
                    pool_k[table[b, i]] = self.kc[b, :, i * page_size:(i + 1) * page_size]
                    pool_v[table[b, i]] = self.vc[b, :, i * page_size:(i + 1) * page_size]
            kc_d, vc_d = to_dev(pool_k, dt), to_dev(pool_v, dt)
            kw["block_table"] = torch.from_numpy(table).to(DEV)
        elif layout == "blhmd":
            kc_d, vc_d = to_dev(self.kc.transpose(0, 1, 3, 2, 4), dt), to_dev(self.vc.transpose(0, 1, 3, 2, 4), dt)
        else:
            kc_d, vc_d = to_dev(self.kc, dt), to_dev(self.vc, dt)
        if self.biases is None:
            bq = bk = bv = torch.zeros(0, dtype=TDT[dt], device=DEV)
        else:
            bq, bk, bv = (to_dev(x, dt) for x in self.biases)
        o = torch.full((B, self.n, self.H, D), 7.0, dtype=TDT[dt], device=DEV)
        lens = self.lens if lens is None else lens
        ret = sfa.flash_decode_chunk(to_dev(self.qkv(), dt), bq, bk, bv, kc_d, vc_d,
                                     torch.tensor(lens, dtype=torch.int32, device=DEV), o,
                                     B, M, self.H, D, self.rot, M, L, self.layer, **kw)
        assert ret.data_ptr() == o.data_ptr()
        torch.cuda.synchronize()
        kc_o, vc_o = kc_d.float().cpu().numpy(), vc_d.float().cpu().numpy()
        if layout == "paged":
            kb = np.zeros_like(self.kc)
            vb = np.zeros_like(self.vc)
            for b in range(B):
                for i in range(M // page_size):
                    kb[b, :, i * page_size:(i + 1) * page_size] = kc_o[table[b, i]]
                    vb[b, :, i * page_size:(i + 1) * page_size] = vc_o[table[b, i]]
            kc_o, vc_o = kb, vb
        elif layout == "blhmd":
            kc_o, vc_o = kc_o.transpose(0, 1, 3, 2, 4), vc_o.transpose(0, 1, 3, 2, 4)
        return o.float().cpu().numpy(), kc_o, vc_o


def check(p, got, want, rows=None):
    o, kc, vc = got
    o_ref, kc_ref, vc_ref = want
    tol = TOL[p.dtype]
    bs = range(p.B) if rows is None else rows
    for b in bs:
        np.testing.assert_allclose(o[b], o_ref[b], atol=tol, rtol=tol, err_msg=f"o[{b}]")
    new = np.zeros(kc.shape[:3], bool)
    for b in bs:
        new[b, p.layer, p.lens[b]:p.lens[b] + p.n] = True
    np.testing.assert_array_equal(vc[new], vc_ref[new])                        # V rows: data movement, exact
    kd, kr = kc[new], kc_ref[new]
    assert np.all(np.abs(kd - kr) <= ULP[p.dtype] * np.maximum(1.0, np.abs(kr)) * 1.01), np.abs(kd - kr).max()
    assert np.mean(kd == kr) > 0.98
    untouched = ~new
    if rows is not None:
        untouched[[b for b in range(p.B) if b not in rows]] = False
    np.testing.assert_array_equal(kc[untouched], p.kc[untouched])
    np.testing.assert_array_equal(vc[untouched], p.vc[untouched])


# pairwise-covering subset of dtype x D x layout x n x num_splits (n = 300 only at D = 128)
_LAYOUTS = [("blmhd", 16), ("blhmd", 16), ("paged", 16), ("paged", 64)]
_SWEEP = [
    ("fp16", 64, 0, 1, 0), ("bf16", 128, 1, 1, 1), ("fp16", 128, 2, 1, 3), ("bf16", 64, 3, 1, 0),
    ("bf16", 64, 0, 3, 3), ("fp16", 128, 1, 3, 0), ("bf16", 128, 2, 3, 1), ("fp16", 64, 3, 3, 1),
    ("bf16", 128, 0, 16, 1), ("fp16", 64, 1, 16, 3), ("bf16", 64, 2, 16, 0), ("fp16", 128, 3, 16, 3),
    ("fp16", 64, 0, 67, 3), ("bf16", 64, 1, 67, 1), ("fp16", 128, 2, 67, 0), ("bf16", 128, 3, 67, 0),
    ("fp16", 128, 0, 300, 0), ("bf16", 128, 1, 300, 3), ("bf16", 128, 2, 300, 1), ("fp16", 128, 3, 300, 1),
]


@pytest.mark.parametrize("dtype,D,li,n,splits", _SWEEP)
def test_chunk_parity_sweep(sfa, dtype, D, li, n, splits):
    layout, ps = _LAYOUTS[li]
    lens = [0, 5, 130, 1000]
    M = 1024 + 384                          # room for pos + n at n = 300; a multiple of both page sizes
    p = Problem(4, 2, 2, D, 2, M, n, lens, dtype, seed=n + D)
    check(p, p.run(sfa, layout, ps, splits), p.oracle())


@pytest.mark.parametrize("variant", ["bias", "lut", "partial_rot", "rot0"])
def test_chunk_bias_and_rotary_variants(sfa, variant):
    kw = dict(bias=variant == "bias", lut=variant in ("lut", "partial_rot"))
    rot = {"partial_rot": 64, "rot0": 0}.get(variant)
    p = Problem(3, 4, 4, 128, 1, 512, 20, [0, 33, 400], "fp16", layer=0, rot=rot, seed=3, **kw)
    check(p, p.run(sfa, "blmhd", num_splits=2), p.oracle())
    p2 = Problem(3, 4, 4, 128, 1, 512, 20, [0, 33, 400], "bf16", layer=0, rot=rot, seed=4, **kw)
    check(p2, p2.run(sfa, "paged", 16), p2.oracle())


@pytest.mark.parametrize("G", [2, 8, 16])
def test_chunk_grouped_queries(sfa, G):
    Hkv = 2
    p = Problem(2, G * Hkv, Hkv, 128, 1, 768, 13, [7, 300], "bf16", layer=0, seed=G, bias=True)
    want = p.oracle()
    check(p, p.run(sfa, "blhmd"), want)
    check(p, p.run(sfa, "paged", 32, num_splits=3), want)


def test_chunk_equals_successive_decode_calls(sfa):
    """One chunk of n = 8 against 8 flash_decode calls on a copy of the cache."""
    n, B, H, D, L, M, layer = 8, 3, 4, 128, 2, 256, 1
    for dtype in ("fp16", "bf16"):
        p = Problem(B, H, H, D, L, M, n, [0, 17, 200], dtype, layer=layer, seed=11)
        o_c, kc_c, vc_c = p.run(sfa, "blmhd")
        kc_d, vc_d = to_dev(p.kc, dtype), to_dev(p.vc, dtype)
        z = torch.zeros(0, dtype=TDT[dtype], device=DEV)
        for t in range(n):
            qkv_t = to_dev(np.stack([p.q[:, t], p.k[:, t], p.v[:, t]], axis=1), dtype)
            o_t = torch.empty(B, H, D, dtype=TDT[dtype], device=DEV)
            sfa.flash_decode(qkv_t, z, z, z, kc_d, vc_d, torch.tensor([s + t for s in p.lens], dtype=torch.int32,
                                                                       device=DEV), o_t, B, M, H, D, D, M, L, layer)
            np.testing.assert_allclose(o_c[:, t], o_t.float().cpu().numpy(), atol=TOL[dtype], rtol=TOL[dtype])
        torch.cuda.synchronize()
        kc_s, vc_s = kc_d.float().cpu().numpy(), vc_d.float().cpu().numpy()
        np.testing.assert_array_equal(vc_c, vc_s)
        assert np.all(np.abs(kc_c - kc_s) <= ULP[dtype] * np.maximum(1.0, np.abs(kc_s)) * 1.01)
        # n = 1 gives what sfa_decode gives
        p1 = Problem(B, H, H, D, L, M, 1, [0, 17, 200], dtype, layer=layer, seed=12)
        o1, kc1, vc1 = p1.run(sfa, "blmhd")
        kc_d, vc_d = to_dev(p1.kc, dtype), to_dev(p1.vc, dtype)
        o_t = torch.empty(B, H, D, dtype=TDT[dtype], device=DEV)
        sfa.flash_decode(to_dev(np.stack([p1.q[:, 0], p1.k[:, 0], p1.v[:, 0]], axis=1), dtype), z, z, z, kc_d, vc_d,
                         torch.tensor(p1.lens, dtype=torch.int32, device=DEV), o_t, B, M, H, D, D, M, L, layer)
        np.testing.assert_allclose(o1[:, 0], o_t.float().cpu().numpy(), atol=TOL[dtype], rtol=TOL[dtype])
        np.testing.assert_array_equal(vc1, vc_d.float().cpu().numpy())
        kd = kc_d.float().cpu().numpy()
        assert np.all(np.abs(kc1 - kd) <= ULP[dtype] * np.maximum(1.0, np.abs(kd)) * 1.01)


@pytest.mark.parametrize("layout", ["blmhd", "paged"])
def test_chunk_prompt_then_decode(sfa, layout):
    """Ingest a padded prompt batch from seq_len = 0, set seq_len to the real lengths, run 4 decode steps; every
    output against the oracle run token by token over the real tokens only."""
    dtype, B, H, D, L, M, layer, ps = "bf16", 3, 4, 64, 1, 256, 0, 16
    real = [5, 40, 37]
    n = max(real)
    p = Problem(B, H, H, D, L, M, n, [0] * B, dtype, layer=layer, seed=21)
    rng = np.random.default_rng(22)
    steps = [rnd((B, 3, H, D), dtype, rng) for _ in range(4)]
    # oracle: each sequence's real prompt tokens, then the decode steps
    kc_r, vc_r = p.kc.copy(), p.vc.copy()
    want_prompt = np.zeros((B, n, H, D), np.float32)
    for b in range(B):
        for t in range(real[b]):
            qkv_t = np.stack([p.q[b:b + 1, t], p.k[b:b + 1, t], p.v[b:b + 1, t]], axis=1)
            want_prompt[b, t] = decode_ref(qkv_t, kc_r[b:b + 1], vc_r[b:b + 1], [t], layer, D, dtype=dtype)["o"][0]
    want_steps = []
    for i, s in enumerate(steps):
        want_steps.append(decode_ref(s, kc_r, vc_r, [r + i for r in real], layer, D, dtype=dtype)["o"])
    # device
    kw = dict(kv_layout=layout)
    if layout == "paged":
        table = np.random.default_rng(5).permutation(B * (M // ps)).astype(np.int32).reshape(B, M // ps)
        pool_k = np.zeros((B * (M // ps), L, ps, H, D), np.float32)
        pool_v = np.zeros_like(pool_k)
        for b in range(B):
            for i in range(M // ps):
                pool_k[table[b, i]] = p.kc[b, :, i * ps:(i + 1) * ps]
                pool_v[table[b, i]] = p.vc[b, :, i * ps:(i + 1) * ps]
        kc_d, vc_d = to_dev(pool_k, dtype), to_dev(pool_v, dtype)
        kw["block_table"] = torch.from_numpy(table).to(DEV)
    else:
        kc_d, vc_d = to_dev(p.kc, dtype), to_dev(p.vc, dtype)
    z = torch.zeros(0, dtype=TDT[dtype], device=DEV)
    o = torch.empty(B, n, H, D, dtype=TDT[dtype], device=DEV)
    sfa.flash_decode_chunk(to_dev(p.qkv(), dtype), z, z, z, kc_d, vc_d, torch.zeros(B, dtype=torch.int32, device=DEV),
                           o, B, M, H, D, D, M, L, layer, **kw)
    sfa.check_decode_status(DEV)
    o = o.float().cpu().numpy()
    for b in range(B):
        np.testing.assert_allclose(o[b, :real[b]], want_prompt[b, :real[b]], atol=TOL[dtype], rtol=TOL[dtype])
    for i, s in enumerate(steps):
        o_t = torch.empty(B, H, D, dtype=TDT[dtype], device=DEV)
        sfa.flash_decode(to_dev(s, dtype), z, z, z, kc_d, vc_d,
                         torch.tensor([r + i for r in real], dtype=torch.int32, device=DEV), o_t, B, M, H, D, D, M, L,
                         layer, **kw)
        np.testing.assert_allclose(o_t.float().cpu().numpy(), want_steps[i], atol=TOL[dtype], rtol=TOL[dtype])
    sfa.check_decode_status(DEV)


def test_chunk_rejection(sfa):
    from starflashattention_amd import SfaError
    from starflashattention_amd._lib import SFA_ERR_BLOCK_TABLE_RANGE, SFA_ERR_SEQ_LEN_RANGE
    dtype, B, H, D, L, M, n = "fp16", 4, 2, 128, 1, 256, 20
    for splits in (1, 3):
        # pos + n > M (sequence 1), pos < 0 (sequence 2): NaN, caches untouched; the others correct
        p = Problem(B, H, H, D, L, M, n, [3, M - n + 1, -1, 100], dtype, layer=0, seed=31)
        good = [0, 3]
        q = Problem(B, H, H, D, L, M, n, [3, 0, 0, 100], dtype, layer=0, seed=31)
        want = q.oracle()
        got = p.run(sfa, "blmhd", num_splits=splits)
        with pytest.raises(SfaError) as e:
            sfa.check_decode_status(DEV)
        assert e.value.status == SFA_ERR_SEQ_LEN_RANGE
        assert np.all(np.isnan(got[0][1])) and np.all(np.isnan(got[0][2]))
        for b in (1, 2):
            np.testing.assert_array_equal(got[1][b], p.kc[b])
            np.testing.assert_array_equal(got[2][b], p.vc[b])
        check(q, got, want, rows=good)
    # paged: an append page outside the pool rejects the whole sequence with nothing written
    ps = 16
    p = Problem(2, H, H, D, L, M, n, [10, 50], dtype, layer=0, seed=32)
    P = M // ps
    table = np.arange(2 * P, dtype=np.int32).reshape(2, P)
    table[1, (50 + n - 1) // ps] = 10 ** 6                   # the last append page of sequence 1
    pool_k = np.concatenate([p.kc[b, :].reshape(L, P, ps, H, D).transpose(1, 0, 2, 3, 4) for b in range(2)])
    pool_v = np.concatenate([p.vc[b, :].reshape(L, P, ps, H, D).transpose(1, 0, 2, 3, 4) for b in range(2)])
    kc_d, vc_d = to_dev(pool_k, dtype), to_dev(pool_v, dtype)
    z = torch.zeros(0, dtype=TDT[dtype], device=DEV)
    o = torch.empty(2, n, H, D, dtype=TDT[dtype], device=DEV)
    sfa.flash_decode_chunk(to_dev(p.qkv(), dtype), z, z, z, kc_d, vc_d,
                           torch.tensor(p.lens, dtype=torch.int32, device=DEV), o, 2, M, H, D, D, M, L, 0,
                           kv_layout="paged", block_table=torch.from_numpy(table).to(DEV))
    with pytest.raises(SfaError) as e:
        sfa.check_decode_status(DEV)
    assert e.value.status == SFA_ERR_BLOCK_TABLE_RANGE
    o = o.float().cpu().numpy()
    assert np.all(np.isnan(o[1]))
    np.testing.assert_array_equal(vc_d[P:].float().cpu().numpy(), pool_v[P:])      # sequence 1: nothing written
    np.testing.assert_array_equal(kc_d[P:].float().cpu().numpy(), pool_k[P:])
    want = p.oracle()                                       # (the oracle has no pages: sequence 0 is valid there)
    np.testing.assert_allclose(o[0], want[0][0], atol=TOL[dtype], rtol=TOL[dtype])


def test_chunk_exact_workspace_through_the_c_abi(sfa):
    """sfa_decode_chunk itself, with a workspace of exactly sfa_decode_chunk_workspace_bytes(..., 3) bytes and a canary
    behind it: bit-identical to the operator (which uses its roomy cached workspace) and nothing written past the end."""
    from exact_workspace import call_with_exact_workspace, decode_problem
    from starflashattention_amd import _lib, ops
    B, n, H, Hkv, D, L, M, S = 2, 3, 4, 2, 64, 1, 128, 3
    qkv, kc0, vc0, o0 = decode_problem((B, n), B, H, Hkv, D, L, M, 72, DEV)
    sl = torch.tensor([0, 100], dtype=torch.int32, device=DEV)
    z = torch.zeros(0, dtype=torch.float16, device=DEV)
    kc1, vc1, o1 = kc0.clone(), vc0.clone(), o0.clone()
    sfa.flash_decode_chunk(qkv, z, z, z, kc1, vc1, sl, o1, B, M, H, D, D, M, L, 0, num_splits=S, num_heads_kv=Hkv)
    sfa.check_decode_status(DEV)
    kc2, vc2, o2 = kc0.clone(), vc0.clone(), o0.clone()
    a, *_ = ops._decode_args(qkv, z, z, z, kc2, vc2, sl, o2, B, M, H, D, D, M, L, 0, None, None, None, "blmhd", None, Hkv,
                             tokens=n)
    lib = _lib.load()
    a.stride = 0
    call_with_exact_workspace(a, lib.sfa_decode_chunk_workspace_bytes(B, H, Hkv, D, M, n, S), S,
                              lambda args, stream: lib.sfa_decode_chunk(args, n, 0, stream), DEV)
    assert torch.equal(o2, o1) and torch.equal(kc2, kc1) and torch.equal(vc2, vc1)
    assert bool(torch.isfinite(o2.float()).all()) and not torch.equal(o2, o0) and not torch.equal(kc2, kc0)


def test_chunk_at_scale_against_prefill(sfa):
    """B=4, H=32, D=128, bf16, blhmd, pos=2048, n=2048 against flash_attn_fwd(q_rot, K[:pos+n], V[:pos+n], causal)
    -- its bottom-right alignment is exactly j <= pos + t -- and 64 sampled rows against fp64."""
    B, H, D, L, M, pos, n, dtype = 4, 32, 128, 1, 4096, 2048, 2048, "bf16"
    g = torch.Generator(device="cpu").manual_seed(41)
    qkv = torch.randn(B, n, 3, H, D, generator=g).bfloat16()
    kc = torch.randn(B, L, H, M, D, generator=g).bfloat16()
    vc = torch.randn(B, L, H, M, D, generator=g).bfloat16()
    kc_d, vc_d = kc.to(DEV), vc.to(DEV)
    o = torch.empty(B, n, H, D, dtype=torch.bfloat16, device=DEV)
    z = torch.zeros(0, dtype=torch.bfloat16, device=DEV)
    sfa.flash_decode_chunk(qkv.to(DEV), z, z, z, kc_d, vc_d, torch.full((B,), pos, dtype=torch.int32, device=DEV), o,
                           B, M, H, D, D, M, L, 0, kv_layout="blhmd")
    sfa.check_decode_status(DEV)
    # oracle RoPE of the inputs (positions pos + t), rounded to bf16
    qn = qkv[:, :, 0].float().numpy()                       # [B, n, H, D]
    q_rot = np.stack([rope_interleaved(qn[:, t], pos + t, D) for t in range(n)], axis=1)
    q_rot = torch.from_numpy(round_to(q_rot, dtype).astype(np.float32)).bfloat16()
    q_d = q_rot.permute(0, 2, 1, 3).contiguous().to(DEV)   # [B, H, n, D]
    k_all, v_all = kc_d[:, 0, :, :pos + n], vc_d[:, 0, :, :pos + n]
    ref = sfa.flash_attn_fwd(q_d, k_all, v_all, causal=True).permute(0, 2, 1, 3).float().cpu().numpy()
    got = o.float().cpu().numpy()
    np.testing.assert_allclose(got, ref, atol=1.6e-2, rtol=1.6e-2)
    # 64 sampled rows against fp64
    rng = np.random.default_rng(0)
    K = k_all.float().cpu().numpy().astype(np.float64)
    V = v_all.float().cpu().numpy().astype(np.float64)
    qr = q_rot.float().numpy().astype(np.float64)
    for _ in range(64):
        b, t, h = rng.integers(B), rng.integers(n), rng.integers(H)
        s = K[b, h, :pos + t + 1] @ qr[b, t, h] / np.sqrt(D)
        w = np.exp(s - s.max())
        want = (w / w.sum()) @ V[b, h, :pos + t + 1]
        np.testing.assert_allclose(got[b, t, h], want, atol=1.6e-2, rtol=1.6e-2)


def test_chunk_cache_beyond_2g_elements(sfa):
    """Caches of more than 2^31 elements per tensor (B=72, M=8192, H=32, D=128) with the chunk in the last sequence."""
    B, H, D, L, M, n, dtype = 72, 32, 128, 1, 8192, 40, "fp16"
    assert B * L * M * H * D > 2 ** 31
    kc_d = torch.zeros(B, L, M, H, D, dtype=torch.float16, device=DEV)
    vc_d = torch.zeros_like(kc_d)
    lens = [0] * B
    lens[-1] = M - n - 3
    rng = np.random.default_rng(51)
    hist = 300                                            # the last sequence's history just below pos
    pos = lens[-1]
    kh = rnd((hist, H, D), dtype, rng)
    vh = rnd((hist, H, D), dtype, rng)
    kc_d[-1, 0, pos - hist:pos] = to_dev(kh, dtype)
    vc_d[-1, 0, pos - hist:pos] = to_dev(vh, dtype)
    qkv = np.zeros((B, n, 3, H, D), np.float32)
    qkv[-1] = rnd((n, 3, H, D), dtype, rng)
    o = torch.empty(B, n, H, D, dtype=torch.float16, device=DEV)
    z = torch.zeros(0, dtype=torch.float16, device=DEV)
    sfa.flash_decode_chunk(to_dev(qkv, dtype), z, z, z, kc_d, vc_d, torch.tensor(lens, dtype=torch.int32, device=DEV),
                           o, B, M, H, D, D, M, L, 0)
    sfa.check_decode_status(DEV)
    # oracle on the last sequence alone (zero history below pos - hist)
    kc1 = np.zeros((1, 1, M, H, D), np.float32)
    vc1 = np.zeros_like(kc1)
    kc1[0, 0, pos - hist:pos], vc1[0, 0, pos - hist:pos] = kh, vh
    want = np.zeros((n, H, D), np.float32)
    for t in range(n):
        want[t] = decode_ref(qkv[-1:, t], kc1, vc1, [pos + t], 0, D, dtype=dtype)["o"][0]
    np.testing.assert_allclose(o[-1].float().cpu().numpy(), want, atol=2e-3, rtol=2e-3)
    np.testing.assert_array_equal(vc_d[-1, 0, pos:pos + n].float().cpu().numpy(), vc1[0, 0, pos:pos + n])
    assert torch.count_nonzero(kc_d[-1, 0, pos + n:]) == 0


@pytest.mark.parametrize("splits", [1, 3])
def test_chunk_bad_read_only_page(sfa, splits):
    """A history page (read only) of one sequence outside the pool: not dereferenced, SFA_ERR_BLOCK_TABLE_RANGE, that
    sequence's outputs NaN; the other sequence correct."""
    from starflashattention_amd import SfaError
    from starflashattention_amd._lib import SFA_ERR_BLOCK_TABLE_RANGE
    dtype, H, D, L, M, n, ps = "bf16", 2, 128, 1, 256, 8, 16
    p = Problem(2, H, H, D, L, M, n, [100, 70], dtype, layer=0, seed=33)
    P = M // ps
    table = np.arange(2 * P, dtype=np.int32).reshape(2, P)
    table[0, 2] = -5                                        # rows 32..47 of sequence 0: history only
    pool_k = np.concatenate([p.kc[b].reshape(L, P, ps, H, D).transpose(1, 0, 2, 3, 4) for b in range(2)])
    pool_v = np.concatenate([p.vc[b].reshape(L, P, ps, H, D).transpose(1, 0, 2, 3, 4) for b in range(2)])
    kc_d, vc_d = to_dev(pool_k, dtype), to_dev(pool_v, dtype)
    z = torch.zeros(0, dtype=TDT[dtype], device=DEV)
    o = torch.empty(2, n, H, D, dtype=TDT[dtype], device=DEV)
    sfa.flash_decode_chunk(to_dev(p.qkv(), dtype), z, z, z, kc_d, vc_d,
                           torch.tensor(p.lens, dtype=torch.int32, device=DEV), o, 2, M, H, D, D, M, L, 0,
                           num_splits=splits, kv_layout="paged", block_table=torch.from_numpy(table).to(DEV))
    with pytest.raises(SfaError) as e:
        sfa.check_decode_status(DEV)
    assert e.value.status == SFA_ERR_BLOCK_TABLE_RANGE
    o = o.float().cpu().numpy()
    assert np.all(np.isnan(o[0]))
    want = p.oracle()
    np.testing.assert_allclose(o[1], want[0][1], atol=TOL[dtype], rtol=TOL[dtype])
    # sequence 1's appended rows are in its own pages P.. of the pool
    vd = vc_d.float().cpu().numpy()[P:].transpose(1, 0, 2, 3, 4).reshape(L, M, H, D)
    np.testing.assert_array_equal(vd[0, 70:70 + n], want[2][1, 0, 70:70 + n])
