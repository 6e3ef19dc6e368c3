"""GPU parity of sfa_decode_varlen (flash_decode_varlen: a ragged, packed batch of new tokens in one call).

Oracle: oracle.decode_ref called token by token per sequence, with seq_len + t -- the semantics the call promises.
Tolerances are those of tests/test_decode_chunk_gpu.py: o at 2e-3 (fp16) / 1.6e-2 (bf16) against fp64, the appended K
rows within one storage ulp and >= 98 % exact, appended V rows and every untouched cache byte bit-exact.
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import decode_ref, rope_interleaved, rotary_table_ref, round_to

pytestmark = pytest.mark.gpu

TOL = {"fp16": 2e-3, "bf16": 1.6e-2}
ULP = {"fp16": 2.0 ** -10, "bf16": 2.0 ** -7}
TDT = {"fp16": torch.float16, "bf16": torch.bfloat16}
DEV = torch.device("cuda:0")
BAD_PAGE = 10 ** 6


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


def i32(x):
    return torch.tensor(list(x), dtype=torch.int32, device=DEV)


class Ragged:
    """A ragged problem: sequence b brings ns[b] tokens at position lens[b]; caches kept in the oracle's BLMHD form."""

    def __init__(self, H, Hkv, D, L, M, ns, lens, dtype, layer=1, rot=None, seed=0, bias=False, lut=False, pad=0):
        rng = np.random.default_rng(seed)
        self.B, self.H, self.Hkv, self.D, self.L, self.M = len(ns), H, Hkv, D, L, M
        self.G = H // Hkv
        self.ns, self.lens, self.dtype, self.layer = list(ns), list(lens), dtype, layer
        self.cu = [0] + list(np.cumsum(ns))
        self.T = int(self.cu[-1]) + pad             # pad: rows of qkv / o past cu[B]
        self.rot = D if rot is None else rot
        T, B = self.T, self.B
        self.q = rnd((T, H, D), dtype, rng)
        self.k = rnd((T, Hkv, D), dtype, rng)
        self.v = rnd((T, Hkv, D), dtype, rng)
        self.kc = rnd((B, L, M, Hkv, D), dtype, rng)
        self.vc = rnd((B, L, M, Hkv, D), dtype, rng)
        self.biases = None
        if bias:
            self.biases = (rnd((H, D), dtype, rng, 0.5), rnd((Hkv, D), dtype, rng, 0.5), rnd((Hkv, D), dtype, rng, 0.5))
        self.tables = rotary_table_ref(M, self.rot, dtype) if lut else None

    def qkv(self):
        if self.G == 1:
            return np.stack([self.q, self.k, self.v], axis=1)                  # [T, 3, H, D]
        return np.concatenate([self.q, self.k, self.v], axis=1)                # [T, H + 2 Hkv, D]

    def oracle(self, seqs=None):
        """o [T, H, D] float32 (NaN where no listed sequence owns the row) and the caches afterwards (Hkv heads):
        decode_ref token by token for every listed sequence."""
        G = self.G
        kc = np.repeat(self.kc, G, axis=3)
        vc = np.repeat(self.vc, G, axis=3)
        kw = {}
        if self.biases is not None:
            kw = dict(q_bias=self.biases[0], k_bias=np.repeat(self.biases[1], G, 0), v_bias=np.repeat(self.biases[2], G, 0))
        if self.tables is not None:
            kw.update(cos_table=self.tables[0], sin_table=self.tables[1])
        o = np.full((self.T, self.H, self.D), np.nan, np.float32)
        for b in (range(self.B) if seqs is None else seqs):
            for t in range(self.ns[b]):
                r = self.cu[b] + t
                qkv_t = np.stack([self.q[r], np.repeat(self.k[r], G, 0), np.repeat(self.v[r], G, 0)])[None]
                o[r] = decode_ref(qkv_t, kc[b:b + 1], vc[b:b + 1], [self.lens[b] + t], self.layer, self.rot,
                                  dtype=self.dtype, **kw)["o"][0]
        return o, kc[:, :, :, ::G], vc[:, :, :, ::G]

    def page_table(self, page_size, strict):
        """A random page assignment; strict: every entry past a sequence's last needed page (all of them for a
        sequence without tokens) points outside the pool."""
        P = self.M // page_size
        full = np.random.default_rng(7).permutation(self.B * P).astype(np.int32).reshape(self.B, P)
        used = full.copy()
        if strict:
            for b in range(self.B):
                need = 0 if self.ns[b] == 0 else (self.lens[b] + self.ns[b] - 1) // page_size + 1
                used[b, need:] = BAD_PAGE
        return full, used

    def run(self, sfa, layout="blmhd", page_size=16, num_splits=0, strict_table=False, table_edit=None, cu=None):
        """-> (o [T, H, D], kc, vc in BLMHD form) from the device.  o starts as 7.0 everywhere."""
        dt = self.dtype
        B, L, M, Hkv, D = self.B, self.L, self.M, self.Hkv, self.D
        kw = dict(num_splits=num_splits, kv_layout=layout)
        if self.Hkv != self.H:
            kw["num_heads_kv"] = Hkv
        if self.tables is not None:
            kw.update(rotary_cos_table=to_dev(self.tables[0], dt), rotary_sin_table=to_dev(self.tables[1], dt))
        if layout == "paged":
            P = M // page_size
            full, used = self.page_table(page_size, strict_table)
            if table_edit is not None:
                table_edit(used)
            pool_k = np.zeros((B * P, L, page_size, Hkv, D), np.float32)
            pool_v = np.zeros_like(pool_k)
            for b in range(B):
                for i in range(P):
                    pool_k[full[b, i]] = self.kc[b, :, i * page_size:(i + 1) * page_size]
                    pool_v[full[b, i]] = self.vc[b, :, i * page_size:(i + 1) * page_size]
            kc_d, vc_d = to_dev(pool_k, dt), to_dev(pool_v, dt)
            kw["block_table"] = torch.from_numpy(used).to(DEV)
        elif layout == "blhmd":
            kc_d, vc_d = to_dev(self.kc.transpose(0, 1, 3, 2, 4), dt), to_dev(self.vc.transpose(0, 1, 3, 2, 4), dt)
        else:
            kc_d, vc_d = to_dev(self.kc, dt), to_dev(self.vc, dt)
        if self.biases is None:
            bq = bk = bv = torch.zeros(0, dtype=TDT[dt], device=DEV)
        else:
            bq, bk, bv = (to_dev(x, dt) for x in self.biases)
        o = torch.full((self.T, self.H, D), 7.0, dtype=TDT[dt], device=DEV)
        ret = sfa.flash_decode_varlen(to_dev(self.qkv(), dt), bq, bk, bv, kc_d, vc_d, i32(self.lens), o,
                                      i32(self.cu if cu is None else cu), B, M, self.H, D, self.rot, M, L, self.layer,
                                      **kw)
        assert ret.data_ptr() == o.data_ptr()
        torch.cuda.synchronize()
        kc_o, vc_o = kc_d.float().cpu().numpy(), vc_d.float().cpu().numpy()
        if layout == "paged":
            kb = np.zeros_like(self.kc)
            vb = np.zeros_like(self.vc)
            for b in range(B):
                for i in range(M // page_size):
                    kb[b, :, i * page_size:(i + 1) * page_size] = kc_o[full[b, i]]
                    vb[b, :, i * page_size:(i + 1) * page_size] = vc_o[full[b, i]]
            kc_o, vc_o = kb, vb
        elif layout == "blhmd":
            kc_o, vc_o = kc_o.transpose(0, 1, 3, 2, 4), vc_o.transpose(0, 1, 3, 2, 4)
        return o.float().cpu().numpy(), kc_o, vc_o


def check(p, got, want, seqs=None):
    """The listed sequences (default: all) are correct; every cache row that is not one of their appended rows --
    the rows at or past pos + n_b, other layers and every other sequence included -- is bit-identical to its initial
    value; every row of o that belongs to no sequence still holds its initial 7.0."""
    o, kc, vc = got
    o_ref, kc_ref, vc_ref = want
    tol = TOL[p.dtype]
    seqs = list(range(p.B)) if seqs is None else list(seqs)
    new = np.zeros(kc.shape[:3], bool)
    for b in seqs:
        r0, r1 = p.cu[b], p.cu[b] + p.ns[b]
        np.testing.assert_allclose(o[r0:r1], o_ref[r0:r1], atol=tol, rtol=tol, err_msg=f"o of sequence {b}")
        new[b, p.layer, p.lens[b]:p.lens[b] + p.ns[b]] = True
    if new.any():
        np.testing.assert_array_equal(vc[new], vc_ref[new])                    # V rows: data movement, exact
        kd, kr = kc[new], kc_ref[new]
        assert np.all(np.abs(kd - kr) <= ULP[p.dtype] * np.maximum(1.0, np.abs(kr)) * 1.01), np.abs(kd - kr).max()
        assert np.mean(kd == kr) > 0.98
    np.testing.assert_array_equal(kc[~new], p.kc[~new])
    np.testing.assert_array_equal(vc[~new], p.vc[~new])
    assert np.all(o[p.cu[-1]:] == 7.0)


# The mixed batch of the sweep: an idle sequence, plain decode (one at pos 0), a verify-sized step, chunks with a ragged
# and a multi-tile row count, and sequence 6 decoding in the last page of the cache (rows 1399 of 1408).  The same batch
# with sequence 6 at 1407, so that pos + n_b == memory_max_len exactly, is test_varlen_sequence_ending_at_memory_max_len.
_NS = [0, 1, 1, 5, 67, 300, 1, 16]
_LENS = [9, 0, 1000, 130, 5, 700, 1399, 64]
_M = 1408
_LAYOUTS = [("blmhd", 16), ("blhmd", 16), ("paged", 16), ("paged", 64)]
# pairwise-covering subset of dtype x D x layout x num_splits
_SWEEP = [
    ("fp16", 64, 0, 0), ("bf16", 128, 0, 1), ("fp16", 128, 0, 3), ("bf16", 64, 1, 3), ("fp16", 128, 1, 0),
    ("fp16", 64, 1, 1), ("fp16", 128, 2, 3), ("bf16", 128, 2, 1), ("bf16", 64, 2, 0), ("bf16", 64, 3, 0),
    ("fp16", 64, 3, 1), ("bf16", 128, 3, 0), ("fp16", 128, 3, 3),
]


@pytest.mark.parametrize("dtype,D,li,splits", _SWEEP)
def test_varlen_mixed_batch_sweep(sfa, dtype, D, li, splits):
    """Cases 1 and 2 of the feature: the mixed batch is correct in every layout, sequence 6 (the last page) succeeds,
    the idle sequence's cache and every row at or past pos + n_b of every sequence are byte-identical afterwards, and
    with a paged cache every table entry past a sequence's last needed page points outside the pool -- which padding
    to a common n could not serve."""
    layout, ps = _LAYOUTS[li]
    p = Ragged(2, 2, D, 2, _M, _NS, _LENS, dtype, layer=1, seed=D + li, pad=3)
    got = p.run(sfa, layout, ps, splits, strict_table=True)
    sfa.check_decode_status(DEV)                                               # clean status
    check(p, got, p.oracle())
    np.testing.assert_array_equal(got[1][0], p.kc[0])                          # the n = 0 sequence
    np.testing.assert_array_equal(got[2][0], p.vc[0])
    for b in range(p.B):                                                       # (check() covers these rows too)
        end = p.lens[b] + p.ns[b]
        np.testing.assert_array_equal(got[1][b, :, end:], p.kc[b, :, end:])
        np.testing.assert_array_equal(got[2][b, :, end:], p.vc[b, :, end:])


@pytest.mark.parametrize("dtype,D,li,splits", [("bf16", 64, 0, 3), ("fp16", 128, 1, 1), ("fp16", 64, 2, 0),
                                               ("bf16", 128, 3, 3)])
def test_varlen_sequence_ending_at_memory_max_len(sfa, dtype, D, li, splits):
    """The sweep's batch with sequence 6 at pos = M - 1: pos + n_b == memory_max_len exactly must succeed, in every
    layout, with a clean status, and sequence 5 moved up so that its 300 tokens end exactly at M as well."""
    layout, ps = _LAYOUTS[li]
    lens = list(_LENS)
    lens[6] = _M - _NS[6]
    lens[5] = _M - _NS[5]
    p = Ragged(2, 2, D, 2, _M, _NS, lens, dtype, layer=1, seed=D + li + 100, pad=3)
    got = p.run(sfa, layout, ps, splits, strict_table=True)
    sfa.check_decode_status(DEV)
    check(p, got, p.oracle())


def _chunk_call(sfa, p, n, layout, splits, ps=16):
    """flash_decode_chunk on the uniform problem p (all ns == n) -> (o [T, H, D], kc, vc) as Ragged.run gives."""
    dt, B, H, D, L, M = p.dtype, p.B, p.H, p.D, p.L, p.M
    z = torch.zeros(0, dtype=TDT[dt], device=DEV)
    kw = dict(num_splits=splits, kv_layout=layout)
    if layout == "paged":
        P = M // ps
        full, _ = p.page_table(ps, False)
        pool_k = np.zeros((B * P, L, ps, p.Hkv, D), np.float32)
        pool_v = np.zeros_like(pool_k)
        for b in range(B):
            for i in range(P):
                pool_k[full[b, i]] = p.kc[b, :, i * ps:(i + 1) * ps]
                pool_v[full[b, i]] = p.vc[b, :, i * ps:(i + 1) * ps]
        kc_d, vc_d = to_dev(pool_k, dt), to_dev(pool_v, dt)
        kw["block_table"] = torch.from_numpy(full).to(DEV)
    else:
        kc_d, vc_d = to_dev(p.kc, dt), to_dev(p.vc, dt)
    o = torch.empty(B, n, H, D, dtype=TDT[dt], device=DEV)
    sfa.flash_decode_chunk(to_dev(p.qkv().reshape((B, n) + p.qkv().shape[1:]), dt), z, z, z, kc_d, vc_d, i32(p.lens),
                           o, B, M, H, D, p.rot, M, L, p.layer, **kw)
    torch.cuda.synchronize()
    kc_o, vc_o = kc_d.float().cpu().numpy(), vc_d.float().cpu().numpy()
    if layout == "paged":
        kb, vb = np.zeros_like(p.kc), np.zeros_like(p.vc)
        for b in range(B):
            for i in range(M // ps):
                kb[b, :, i * ps:(i + 1) * ps] = kc_o[full[b, i]]
                vb[b, :, i * ps:(i + 1) * ps] = vc_o[full[b, i]]
        kc_o, vc_o = kb, vb
    return o.float().cpu().numpy().reshape(B * n, H, D), kc_o, vc_o


@pytest.mark.parametrize("dtype,layout,splits", [("fp16", "blmhd", 1), ("bf16", "paged", 3), ("bf16", "blmhd", 0)])
def test_varlen_uniform_lengths_reproduce_the_chunk(sfa, dtype, layout, splits):
    """All n_b = 8 with the same num_splits: the same kernels on the same rows and the same key splits, so o and both
    caches are bit-identical to flash_decode_chunk's (asserted as such), and correct against the oracle."""
    n = 8
    p = Ragged(4, 4, 128, 2, 512, [n] * 3, [0, 17, 400], dtype, layer=1, seed=11)
    # num_splits = 0 leaves the count to each entry point's own rule; the two agree here (B * Hkv * tiles = 12 and
    # bound * Hkv = 12 workgroups)
    got = p.run(sfa, layout, 16, splits)
    ref = _chunk_call(sfa, p, n, layout, splits)
    sfa.check_decode_status(DEV)
    for g, r, what in zip(got, ref, ("o", "k_cache", "v_cache")):
        np.testing.assert_array_equal(g, r, err_msg=what)
    check(p, got, p.oracle())


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_varlen_all_single_tokens_match_flash_decode(sfa, dtype):
    B, H, D, L, M, layer = 3, 4, 128, 2, 256, 1
    p = Ragged(H, H, D, L, M, [1] * B, [0, 17, 200], dtype, layer=layer, seed=12)
    got = p.run(sfa, "blmhd")
    sfa.check_decode_status(DEV)
    check(p, got, p.oracle())
    kc_d, vc_d = to_dev(p.kc, dtype), to_dev(p.vc, dtype)
    z = torch.zeros(0, dtype=TDT[dtype], device=DEV)
    o_t = torch.empty(B, H, D, dtype=TDT[dtype], device=DEV)
    sfa.flash_decode(to_dev(p.qkv(), dtype), z, z, z, kc_d, vc_d, i32(p.lens), o_t, B, M, H, D, D, M, L, layer)
    np.testing.assert_allclose(got[0], o_t.float().cpu().numpy(), atol=TOL[dtype], rtol=TOL[dtype])
    np.testing.assert_array_equal(got[2], vc_d.float().cpu().numpy())
    kd = kc_d.float().cpu().numpy()
    assert np.all(np.abs(got[1] - kd) <= ULP[dtype] * np.maximum(1.0, np.abs(kd)) * 1.01)
    assert np.mean(got[1] == kd) > 0.98


@pytest.mark.parametrize("variant", ["bias", "lut", "partial_rot", "rot0"])
def test_varlen_bias_and_rotary_variants(sfa, variant):
    kw = dict(bias=variant == "bias", lut=variant in ("lut", "partial_rot"))
    rot = {"partial_rot": 64, "rot0": 0}.get(variant)
    p = Ragged(4, 4, 128, 1, 512, [3, 40, 1], [0, 33, 400], "fp16", layer=0, rot=rot, seed=3, **kw)
    check(p, p.run(sfa, "blmhd", num_splits=2), p.oracle())
    p2 = Ragged(4, 4, 128, 1, 512, [3, 40, 1], [0, 33, 400], "bf16", layer=0, rot=rot, seed=4, **kw)
    check(p2, p2.run(sfa, "paged", 16, strict_table=True), p2.oracle())
    sfa.check_decode_status(DEV)


@pytest.mark.parametrize("G", [2, 8, 16])
def test_varlen_grouped_queries(sfa, G):
    Hkv = 2
    p = Ragged(G * Hkv, Hkv, 128, 1, 768, [3, 40, 1], [7, 300, 767], "bf16", layer=0, seed=G, bias=True)
    want = p.oracle()
    check(p, p.run(sfa, "blhmd"), want)
    check(p, p.run(sfa, "paged", 32, num_splits=3, strict_table=True), want)
    sfa.check_decode_status(DEV)


@pytest.mark.parametrize("splits", [1, 3])
def test_varlen_rejection(sfa, splits):
    """One paged batch: pos + n_b > M (sequence 1), pos < 0 (2), an append page outside the pool (4), a cu_tokens range
    that exceeds total_tokens (5), and two good sequences (0, 3)."""
    from starflashattention_amd import SfaError, ops
    from starflashattention_amd._lib import SFA_ERR_BLOCK_TABLE_RANGE
    dtype, H, D, L, M, ps = "fp16", 2, 128, 1, 256, 16
    ns = [5, 20, 4, 33, 20, 9]
    lens = [3, M - 20 + 1, -1, 100, 50, 10]
    p = Ragged(H, H, D, L, M, ns, lens, dtype, layer=0, seed=31)
    try:
        sfa.check_decode_status(DEV)                        # start from a clean status word
    except SfaError:
        pass
    cu = list(p.cu)
    cu[-1] = p.T + 7                                        # sequence 5 claims rows past the end of qkv / o

    def edit(table):
        table[4, (50 + 20 - 1) // ps] = BAD_PAGE             # the last append page of sequence 4

    got = p.run(sfa, "paged", ps, splits, table_edit=edit, cu=cu)
    ws = ops._workspaces[(DEV.index, torch.cuda.current_stream(DEV).cuda_stream)]
    assert int(ws[:4].view(torch.int32).item()) == 3        # both sticky bits: seq_len / cu_tokens range, block table
    with pytest.raises(SfaError) as e:
        sfa.check_decode_status(DEV)
    assert e.value.status == SFA_ERR_BLOCK_TABLE_RANGE      # (the poll reports the block-table bit first)
    o = got[0]
    for b in (1, 2, 4):                                     # rejected: NaN rows
        assert np.all(np.isnan(o[p.cu[b]:p.cu[b + 1]])), b
    assert np.all(o[p.cu[5]:] == 7.0)                       # skipped: nothing written
    check(p, got, p.oracle(seqs=[0, 3]), seqs=[0, 3])       # the good ones correct, every other cache byte untouched


@pytest.mark.parametrize("splits", [1, 3])
def test_varlen_bad_read_only_page(sfa, splits):
    """A history page (read only) of one sequence outside the pool: not dereferenced, SFA_ERR_BLOCK_TABLE_RANGE, that
    sequence's outputs NaN; the other sequences correct."""
    from starflashattention_amd import SfaError
    from starflashattention_amd._lib import SFA_ERR_BLOCK_TABLE_RANGE
    dtype, H, D, L, M, ps = "bf16", 2, 128, 1, 256, 16
    p = Ragged(H, H, D, L, M, [8, 3, 1], [100, 70, 200], dtype, layer=0, seed=33)

    def edit(table):
        table[0, 2] = -5                                    # rows 32..47 of sequence 0: history only

    got = p.run(sfa, "paged", ps, splits, strict_table=True, table_edit=edit)
    with pytest.raises(SfaError) as e:
        sfa.check_decode_status(DEV)
    assert e.value.status == SFA_ERR_BLOCK_TABLE_RANGE
    assert np.all(np.isnan(got[0][:8]))
    want = p.oracle()
    for b in (1, 2):
        r0, r1 = p.cu[b], p.cu[b + 1]
        np.testing.assert_allclose(got[0][r0:r1], want[0][r0:r1], atol=TOL[dtype], rtol=TOL[dtype])
        rows = slice(p.lens[b], p.lens[b] + p.ns[b])
        np.testing.assert_array_equal(got[2][b, 0, rows], want[2][b, 0, rows])


def test_varlen_token_stride_through_the_c_abi(sfa):
    """qkv rows as a strided view of a wider buffer (qkv_token_stride), through sfa_decode_varlen itself; the bytes
    between the rows are unchanged afterwards."""
    from starflashattention_amd import _lib, ops
    dtype, H, D, L, M = "fp16", 4, 64, 1, 256
    p = Ragged(H, H, D, L, M, [2, 0, 21, 1], [5, 9, 100, 255], dtype, layer=0, seed=44, pad=2)
    row, wide = 3 * H * D, 3 * H * D + 40                   # 40 extra elements (a multiple of 8) after every token
    buf = torch.full((p.T, wide), -3.0, dtype=TDT[dtype], device=DEV)
    buf[:, :row] = to_dev(p.qkv().reshape(p.T, row), dtype)
    before = buf.clone()
    kc_d, vc_d = to_dev(p.kc, dtype), to_dev(p.vc, dtype)
    o = torch.full((p.T, H, D), 7.0, dtype=TDT[dtype], device=DEV)
    z = torch.zeros(0, dtype=TDT[dtype], device=DEV)
    dense = torch.empty(p.T, 3, H, D, dtype=TDT[dtype], device=DEV)            # only to let _decode_args check shapes
    sl = i32(p.lens)
    a, *_ = ops._decode_args(dense, z, z, z, kc_d, vc_d, sl, o, p.B, M, H, D, D, M, L, 0, None, None, None,
                             "blmhd", None, None, packed=p.T)
    lib = _lib.load()
    ws = torch.empty(lib.sfa_decode_varlen_workspace_bytes(p.B, H, H, D, M, p.T, 2), dtype=torch.uint8, device=DEV)
    stream = ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    _lib.check(lib.sfa_decode_reset_status(ctypes.c_void_p(ws.data_ptr()), stream))
    cu = i32(p.cu)
    a.qkv, a.stride, a.num_splits = buf.data_ptr(), 0, 2
    a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
    _lib.check(lib.sfa_decode_varlen(ctypes.byref(a), ctypes.c_void_p(cu.data_ptr()), p.T, wide, stream))
    assert lib.sfa_decode_poll_status(ctypes.c_void_p(ws.data_ptr()), stream) == 0
    assert torch.equal(buf, before)
    check(p, (o.float().cpu().numpy(), kc_d.float().cpu().numpy(), vc_d.float().cpu().numpy()), p.oracle())


def test_varlen_exact_workspace_through_the_c_abi(sfa):
    """sfa_decode_varlen itself, with a workspace of exactly sfa_decode_varlen_workspace_bytes(..., 3) bytes (status,
    a plan of 3 entries, rotated Q, partials) and a canary behind it: bit-identical to the operator (which uses its
    roomy cached workspace) and nothing written past the end."""
    from exact_workspace import call_with_exact_workspace, decode_problem
    from starflashattention_amd import _lib, ops
    H, Hkv, D, L, M, S = 4, 2, 64, 1, 128, 3
    ns, B, T = [0, 5, 1], 3, 8                             # two padding rows behind the six tokens
    assert T * (H // Hkv) // 256 + B == 3
    qkv, kc0, vc0, o0 = decode_problem((T,), B, H, Hkv, D, L, M, 73, DEV)
    sl, cu = i32([9, 100, 127]), i32([0] + list(np.cumsum(ns)))
    z = torch.zeros(0, dtype=torch.float16, device=DEV)
    kc1, vc1, o1 = kc0.clone(), vc0.clone(), o0.clone()
    sfa.flash_decode_varlen(qkv, z, z, z, kc1, vc1, sl, o1, cu, B, M, H, D, D, M, L, 0, num_splits=S, num_heads_kv=Hkv)
    sfa.check_decode_status(DEV)
    kc2, vc2, o2 = kc0.clone(), vc0.clone(), o0.clone()
    a, *_ = ops._decode_args(qkv, z, z, z, kc2, vc2, sl, o2, B, M, H, D, D, M, L, 0, None, None, None, "blmhd", None, Hkv,
                             packed=T)
    lib = _lib.load()
    a.stride = 0
    call_with_exact_workspace(a, lib.sfa_decode_varlen_workspace_bytes(B, H, Hkv, D, M, T, S), S,
                              lambda args, stream: lib.sfa_decode_varlen(args, ctypes.c_void_p(cu.data_ptr()), T, 0, stream),
                              DEV)
    assert torch.equal(o2, o1) and torch.equal(kc2, kc1) and torch.equal(vc2, vc1)
    assert bool(torch.isfinite(o2[:6].float()).all()) and bool((o2[6:] == 7.0).all()) and not torch.equal(kc2, kc0)


def test_varlen_at_scale(sfa):
    """B=64, H=32, D=128, bf16, blhmd, M=4096: one sequence with n=2048 at pos=2048, 63 with n=1 at pos=4095.  The long
    sequence against flash_attn_fwd(q_rot, K[:pos+n], V[:pos+n], causal) -- its bottom-right alignment is exactly
    j <= pos + t -- and 64 sampled rows of the whole batch against fp64."""
    B, H, D, L, M, dtype = 64, 32, 128, 1, 4096, "bf16"
    long_b, pos, n = 20, 2048, 2048
    ns = [1] * B
    ns[long_b] = n
    lens = [M - 1] * B
    lens[long_b] = pos
    cu = [0] + list(np.cumsum(ns))
    T = cu[-1]
    g = torch.Generator(device="cpu").manual_seed(41)
    qkv = torch.randn(T, 3, H, D, generator=g).bfloat16()
    gd = torch.Generator(device=DEV).manual_seed(42)
    kc_d = torch.randn(B, L, H, M, D, generator=gd, device=DEV, dtype=torch.bfloat16)
    vc_d = torch.randn(B, L, H, M, D, generator=gd, device=DEV, dtype=torch.bfloat16)
    o = torch.empty(T, H, D, dtype=torch.bfloat16, device=DEV)
    z = torch.zeros(0, dtype=torch.bfloat16, device=DEV)
    sfa.flash_decode_varlen(qkv.to(DEV), z, z, z, kc_d, vc_d, i32(lens), o, i32(cu), B, M, H, D, D, M, L, 0,
                            kv_layout="blhmd")
    sfa.check_decode_status(DEV)
    got = o.float().cpu().numpy()
    # oracle RoPE of every token's q at its own position, rounded to bf16
    qn = qkv[:, 0].float().numpy()                          # [T, H, D]
    where = [(b, lens[b] + t) for b in range(B) for t in range(ns[b])]         # (sequence, position) of packed row r
    q_rot = np.stack([rope_interleaved(qn[r:r + 1], where[r][1], D)[0] for r in range(T)])
    q_rot = round_to(q_rot, dtype).astype(np.float32)
    r0 = cu[long_b]
    q_d = torch.from_numpy(q_rot[r0:r0 + n]).bfloat16().permute(1, 0, 2).contiguous()[None].to(DEV)   # [1, H, n, D]
    k_all, v_all = kc_d[long_b:long_b + 1, 0, :, :pos + n], vc_d[long_b:long_b + 1, 0, :, :pos + n]
    ref = sfa.flash_attn_fwd(q_d, k_all, v_all, causal=True)[0].permute(1, 0, 2).float().cpu().numpy()
    np.testing.assert_allclose(got[r0:r0 + n], ref, atol=1.6e-2, rtol=1.6e-2)
    # 64 sampled rows against fp64: half from the long sequence, half from the single-token ones
    rng = np.random.default_rng(0)
    single = [r for r in range(T) if not r0 <= r < r0 + n]
    rows = list(r0 + rng.integers(n, size=32)) + list(rng.choice(single, size=32, replace=False))
    assert len(rows) == 64
    for r in rows:
        b, at = where[r]
        h = int(rng.integers(H))
        K = kc_d[b, 0, h, :at + 1].float().cpu().numpy().astype(np.float64)
        V = vc_d[b, 0, h, :at + 1].float().cpu().numpy().astype(np.float64)
        s = K @ q_rot[r, h].astype(np.float64) / np.sqrt(D)
        w = np.exp(s - s.max())
        np.testing.assert_allclose(got[r, h], (w / w.sum()) @ V, atol=1.6e-2, rtol=1.6e-2)


def test_varlen_graph_replay(sfa):
    """One captured flash_decode_varlen call, replayed once each with two different cu_tokens / seq_len contents under
    the same total_tokens bound: the lengths are read on the device, so both replays are correct."""
    dtype, H, D, L, M, T = "fp16", 4, 128, 1, 512, 44
    cases = [Ragged(H, H, D, L, M, [3, 0, 40, 1], [10, 5, 300, 511], dtype, layer=0, seed=61),
             Ragged(H, H, D, L, M, [1, 20, 0, 10], [0, 77, 9, 200], dtype, layer=0, seed=62, pad=13)]
    assert all(c.T == T for c in cases)
    B = 4
    dt = TDT[dtype]
    qkv = torch.zeros(T, 3, H, D, dtype=dt, device=DEV)
    kc_d = torch.zeros(B, L, M, H, D, dtype=dt, device=DEV)
    vc_d = torch.zeros_like(kc_d)
    o = torch.zeros(T, H, D, dtype=dt, device=DEV)
    cu = torch.zeros(B + 1, dtype=torch.int32, device=DEV)     # all sequences idle during warm-up and capture
    sl = torch.zeros(B, dtype=torch.int32, device=DEV)
    z = torch.zeros(0, dtype=dt, device=DEV)
    call = lambda: sfa.flash_decode_varlen(qkv, z, z, z, kc_d, vc_d, sl, o, cu, B, M, H, D, D, M, L, 0, num_splits=2)
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        call()                                              # warm-up: the stream's workspace exists before the capture
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            call()
        for c in cases:
            qkv.copy_(to_dev(c.qkv(), dtype))
            kc_d.copy_(to_dev(c.kc, dtype))
            vc_d.copy_(to_dev(c.vc, dtype))
            o.fill_(7.0)
            cu.copy_(i32(c.cu))
            sl.copy_(i32(c.lens))
            graph.replay()
            side.synchronize()
            sfa.check_decode_status(DEV)
            check(c, (o.float().cpu().numpy(), kc_d.float().cpu().numpy(), vc_d.float().cpu().numpy()), c.oracle())
