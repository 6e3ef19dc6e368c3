"""Far addresses: operands whose element offsets do not fit 32 bits, and the arithmetic that makes running them safe.

A kernel that forms an offset beyond 2^31 elements (2^32 bytes for 16-bit data) in a 32-bit register reads or writes
somewhere else.  The tests of tests/test_far_memory_*_gpu.py hand the kernels such offsets and compare with the same call
on compact copies, bit for bit.  As in test_invalid_sequences_are_skipped, not even a wrong implementation may leave memory
the test owns, so every operand that is made far lives in one arena, and for every offset x the call can form the four
addresses a truncating implementation would form instead --

    x cut to signed 32 bits and to unsigned 32 bits, as an element count;  the same two cuts of x as a byte count

-- are computed here (int64 numpy) and shown to lie inside the arena.  The layout of an arena:

    [ guard: GUARD elements | the operand: its base, ..., the far term at >= FAR elements ... ]

The guard in front absorbs the negative results of the signed cuts (at least -2^31 elements); everything else lands between
the base and the true address.  The arena is torch.empty, never zeros: a case writes the rows it uses and nothing else.

This module is pure numpy (the CPU twin tests/test_far_memory_cpu.py imports it); only Arena touches torch, on use.
"""
import numpy as np

FAR = 2 ** 31 + 2 ** 20         # elements: the least true offset of the term a case makes far
GUARD = 2 ** 31                 # elements in front of an operand's base
NEAR = 2 ** 24                  # elements: every term a case does not make far stays below this ...
CAP = 13 * 2 ** 30 + 2 ** 29    # bytes: "about 13 GiB" live at once
BAND = 64                       # rows of sentinel on either side of what a call writes
SENTINEL = 0x5A5A               # the 16-bit pattern of the bands (a finite value in fp16 and bf16)


def up(x, m=8):
    return -(-int(x) // m) * m


# ---- the K / V row-pitch limit of the 8-wave prefill kernels (csrc/prefill_common.h) ------------------------------------

def pitch_limit(tile_rows, head_dim):
    """the largest K / V row pitch (elements, a multiple of 8) at which the last 16-byte chunk of a tile's last row,
    (tile_rows - 1) * 2 * pitch + 16 * (head_dim / 8 - 1) bytes from the tile's base, stays below 2^32"""
    return (2 ** 32 - 1 - 16 * (head_dim // 8 - 1)) // (2 * (tile_rows - 1)) // 8 * 8


def wraps_at(pitch, tile_rows, head_dim):
    """whether any (row, chunk) of a tile gets a 32-bit byte offset that differs from the true one"""
    rows = np.arange(tile_rows, dtype=np.int64)[:, None]
    true = rows * 2 * pitch + 16 * np.arange(head_dim // 8, dtype=np.int64)[None, :]
    return bool(np.any(true % 2 ** 32 != true))


def w4_serves(D, Sq, Sk, q_pitch, k_pitch, v_pitch):
    """prefill_w4_serves / prefill_w4d_serves (csrc): one head's Q / K / V rows fit the 32-bit buffer descriptors"""
    if D not in (128, 256):
        return False
    tail = 2 * D if D == 128 else 512
    ext = lambda S, p: (S - 1) * 2 * p + tail
    return all(ext(S, p) < 2 ** 31 and 2 * p < 2 ** 24 for S, p in ((Sq, q_pitch), (Sk, k_pitch), (Sk, v_pitch)))


# ---- truncations -------------------------------------------------------------------------------------------------------

def _s32(y):
    return (y + 2 ** 31) % 2 ** 32 - 2 ** 31


def _u32(y):
    return y % 2 ** 32


def truncations(x, itemsize):
    """[4, n] byte offsets from the operand's base that stand where the element offsets x belong when x is cut to signed /
    unsigned 32 bits as an element count, and when x * itemsize is cut to signed / unsigned 32 bits"""
    x = np.asarray(x, dtype=np.int64).ravel()
    assert np.all(x >= 0) and np.all(x < 2 ** 40)
    return np.stack([_s32(x) * itemsize, _u32(x) * itemsize, _s32(x * itemsize), _u32(x * itemsize)])


class Placement:
    """One operand as a strided view: `shape` rows of `D` contiguous elements at `strides` (elements), plus what the
    tables claim about it.  terms: name -> (largest value the term takes, kind) with kind "far" (the one term of the
    case, >= FAR), "near" (< NEAR) or "bounded" (neither: a term that shares the far term's stride and is limited
    elsewhere -- `bound` names where)."""

    def __init__(self, operand, term, shape, strides, D, terms, itemsize=2, bound=""):
        self.operand, self.term, self.shape, self.strides, self.D = operand, term, tuple(shape), tuple(strides), D
        self.terms, self.itemsize, self.bound = terms, itemsize, bound

    def row_offsets(self):
        """element offset of every row of the view from its base"""
        x = np.zeros((), np.int64)
        for n, s in zip(self.shape, self.strides):
            x = x[..., None] + np.arange(n, dtype=np.int64) * int(s)
        return x

    def offsets(self):
        """every offset the call can form for this operand: each term alone, and every row's sum of terms"""
        alone = [np.arange(n, dtype=np.int64) * int(s) for n, s in zip(self.shape, self.strides)]
        return np.unique(np.concatenate([a.ravel() for a in alone + [self.row_offsets()]]))

    def extent(self):
        """elements from the base to the end of the last row"""
        return int(self.row_offsets().max()) + self.D

    def arena_bytes(self):
        """the arena this placement needs: the guard, then everything a true or a truncated address can reach"""
        reach = max(self.extent() * self.itemsize, int(truncations(self.offsets(), self.itemsize).max()) + self.D * self.itemsize)
        return up(GUARD * self.itemsize + reach, 4096)

    def safe_in(self, arena_bytes, base=GUARD):
        """every true and every truncated row address lies inside an arena of arena_bytes with the base `base` elements in"""
        base = base * self.itemsize
        t = truncations(self.offsets(), self.itemsize) + base
        x = self.offsets() * self.itemsize + base
        end = arena_bytes - self.D * self.itemsize
        return bool(t.min() >= 0 and t.max() <= end and x.min() >= 0 and x.max() <= end)

    def written(self):
        """[(first element, one past the last)] of the maximal runs of memory the view covers, in base-relative elements"""
        starts = np.sort(self.row_offsets().ravel())
        cut = np.flatnonzero(np.diff(starts) != self.D) + 1
        lo = starts[np.concatenate([[0], cut])]
        hi = starts[np.concatenate([cut - 1, [len(starts) - 1]])] + self.D
        assert np.all(lo[1:] >= hi[:-1])        # rows never overlap
        return list(zip(lo.tolist(), hi.tolist()))

    def bands(self):
        """base-relative element indices of BAND rows on either side of every run of written(), clipped to the gaps"""
        runs = self.written()
        n = BAND * self.D
        out = []
        for i, (lo, hi) in enumerate(runs):
            prev_hi = runs[i - 1][1] if i else lo - n
            next_lo = runs[i + 1][0] if i + 1 < len(runs) else hi + n
            out.append(np.arange(max(lo - n, prev_hi), lo, dtype=np.int64))
            out.append(np.arange(hi, min(hi + n, next_lo), dtype=np.int64))
        return np.unique(np.concatenate(out))


# ---- the prefill tables -------------------------------------------------------------------------------------------------
# B = 2, Hq = 4 over Hkv = 2; the two shapes put the ragged tile, the second q-tile and the rows without a key on either
# side; packed: four sequences of prefill_varlen_split_ref.LENS, a ragged one, one without query rows and one with more
# rows than keys among them.
B, HQ, HKV = 2, 4, 2
SHAPES = ((100, 299), (299, 100))
PACKED_LENS = ((300, 300), (0, 5), (257, 520), (300, 100))
KEY_TILE = 64
RECT_TERMS = {"q": ("batch", "head", "row"), "o": ("batch", "head", "row"), "k": ("batch", "head", "tile"),
              "v": ("batch", "head", "tile")}
PACKED_TERMS = ("token", "head")


def rect_placement(operand, term, Sq, Sk, D):
    """[B, H, S] rows of operand "q" / "k" / "v" / "o" with `term` made far:
    batch  the batch stride: batch 1 is far;                 head  the head stride: the last head is far;
    row    (q, o) the seq stride: the last rows are far;     tile  (k, v) the seq stride, so that the base of the last
    64-key tile is far while the pitch stays inside the admitted range (pitch_limit(64, D))."""
    H, S = (HQ, Sq) if operand in "qo" else (HKV, Sk)
    tiles = -(-S // KEY_TILE)
    if term == "batch":
        strides = (up(FAR), S * D, D)
    elif term == "head":
        strides = (S * D, up(-(-FAR // (H - 1))), D)
    elif term == "row":
        strides = (H * D, D, up(-(-FAR // (S - 1))))
    else:
        strides = (H * D, D, up(-(-FAR // ((tiles - 1) * KEY_TILE))))
    sb, sh, ss = strides
    if term == "tile":
        terms = {"batch": ((B - 1) * sb, "near"), "head": ((H - 1) * sh, "near"),
                 "tile": ((tiles - 1) * KEY_TILE * ss, "far"), "row in tile": ((KEY_TILE - 1) * ss, "bounded")}
        bound = "pitch_limit: (T - 1) * 2 * pitch + 16 * (D / 8 - 1) < 2^32 bytes"
    else:
        terms = {"batch": ((B - 1) * sb, "far" if term == "batch" else "near"),
                 "head": ((H - 1) * sh, "far" if term == "head" else "near"),
                 "row": ((S - 1) * ss, "far" if term == "row" else "near")}
        bound = ""
    return Placement(operand, term, (B, H, S), strides, D, terms, bound=bound)


def cu_of(lens):
    return [int(x) for x in np.concatenate([[0], np.cumsum(lens)])]


def packed_placement(operand, term, D, lens=PACKED_LENS):
    """[T, H] rows of a packed operand with `term` made far:
    token  the token stride, so that cu[b] * stride is far for the last sequence (for k and v inside pitch_limit(64, D));
    head   the head stride: the last head is far."""
    side = 0 if operand in "qo" else 1
    H = HQ if operand in "qo" else HKV
    cu = cu_of([n[side] for n in lens])
    T, start, n_last = cu[-1], cu[-2], cu[-1] - cu[-2]
    if term == "token":
        strides = (up(-(-FAR // start)), D)
        terms = {"base": (start * strides[0], "far"), "head": ((H - 1) * D, "near"),
                 "row in sequence": ((n_last - 1) * strides[0], "bounded")}
        bound = "the token stride's other multiplier: 64-bit wherever the base is; its 32-bit part is the row in a tile " \
                "(k, v: pitch_limit)"
    else:
        strides = (D, up(-(-FAR // (H - 1))))
        terms = {"token": ((T - 1) * D, "near"), "head": ((H - 1) * strides[1], "far")}
        bound = ""
    return Placement(operand, term, (T, H), strides, D, terms, bound=bound)


def limit_placement(operand, tile_rows, D, Sk, packed=False):
    """k or v at the largest admitted pitch of a kernel with tile_rows-key tiles: [B, HKV, Sk] (packed: [Sk, HKV]) rows,
    batches and heads interleaved inside a row's gap"""
    pitch = pitch_limit(tile_rows, D)
    if packed:
        return Placement(operand, "limit", (Sk, HKV), (pitch, D), D,
                         {"head": ((HKV - 1) * D, "near"), "row in tile": ((tile_rows - 1) * pitch, "bounded")},
                         bound="pitch_limit")
    return Placement(operand, "limit", (B, HKV, Sk), (HKV * D, D, pitch), D,
                     {"batch": ((B - 1) * HKV * D, "near"), "head": ((HKV - 1) * D, "near"),
                      "row in tile": ((tile_rows - 1) * pitch, "bounded")}, bound="pitch_limit")


# keys of the cases at the pitch limit: one full tile and a ragged one, so that the rows T/2 .. T-1 of a full tile -- those
# that wrap one notch above the limit -- are read.  70 for the 64-key tiles; the 32-key tiles of the 128-row kernel reach
# the same with 38 (70 rows at its pitch of 69 M elements would take the arena past the cap).
LIMIT_SK = {64: 70, 32: 38}
LIMIT_SQ = 100
# packed: the sequence with the full tile starts 30 rows in, so its base is a 64-bit term of its own
LIMIT_PACKED_LENS = ((50, 30), (100, 70))


RECT_DIMS = (64, 128, 256)
PACKED_DIMS = (64, 128)


def prefill_placements():
    """every placement the prefill GPU module runs: id -> Placement"""
    out = {}
    for Sq, Sk in SHAPES:
        for D in RECT_DIMS:
            for op, ts in RECT_TERMS.items():
                for t in ts:
                    out["rect-%dx%d-D%d-%s-%s" % (Sq, Sk, D, op, t)] = rect_placement(op, t, Sq, Sk, D)
    for D in PACKED_DIMS:
        for op in "qkvo":
            for t in PACKED_TERMS:
                out["packed-D%d-%s-%s" % (D, op, t)] = packed_placement(op, t, D)
    for D in PACKED_DIMS:
        for op in "kv":
            out["limit64-D%d-%s" % (D, op)] = limit_placement(op, 64, D, LIMIT_SK[64])
            out["limit32-D%d-%s" % (D, op)] = limit_placement(op, 32, D, LIMIT_SK[32])
            out["limit64-packed-D%d-%s" % (D, op)] = limit_placement(op, 64, D, cu_of([n for _, n in LIMIT_PACKED_LENS])[-1],
                                                                    packed=True)
    return out


# ---- the arena ---------------------------------------------------------------------------------------------------------

class Arena:
    """One torch.empty uint8 arena on the device, shared by the cases of a module.  view(p, dtype): the strided view of
    placement p, its base GUARD elements in."""

    def __init__(self, nbytes, device):
        import torch
        assert nbytes <= CAP, nbytes
        self.nbytes = int(nbytes)
        self.mem = torch.empty(self.nbytes, dtype=torch.uint8, device=device)

    def typed(self, dtype):
        return self.mem.view(dtype)

    def view(self, p, dtype, base=GUARD):
        import torch
        assert p.safe_in(self.nbytes, base) and self.mem.element_size() == 1 and torch.empty(0, dtype=dtype).element_size() == p.itemsize
        return torch.as_strided(self.typed(dtype), p.shape + (p.D,), p.strides + (1,), storage_offset=base)

    def paint(self, p, dtype, base=GUARD):
        """write the sentinel into the bands around what a call may write through view(p); returns the band indices"""
        import torch
        idx = torch.from_numpy(p.bands() + base).to(self.mem.device)
        assert int(idx.min()) >= 0 and int(idx.max()) < self.nbytes // p.itemsize
        self.typed(torch.int16).index_fill_(0, idx, SENTINEL)
        return idx

    def intact(self, idx):
        import torch
        return bool((self.typed(torch.int16)[idx] == SENTINEL).all())

    def free(self):
        import torch
        del self.mem
        torch.cuda.empty_cache()


# ---- the decode tables -------------------------------------------------------------------------------------------------
# B = 2, Hq = 8 over Hkv = 2, M = 512, histories of 200 and 37 rows, 3 new tokens (packed: 3 and 1), window 40; behind the
# appended rows TAIL rows of sentinel.  A far cache holds the sequences' rows at element offsets beyond FAR from the cache
# pointer: the contiguous layouts through the layer term (b * L + idx_layer) * M * Hkv * D with idx_layer = L - 1, the paged
# layout through page * page_stride with the block tables naming the highest pages of a pool of more than 2^31 elements.
DEC_B, DEC_HQ, DEC_HKV, DEC_M, DEC_PS = 2, 8, 2, 512, 16
DEC_LENS, DEC_N, DEC_VARLEN_NS, DEC_WINDOW, DEC_TAIL = (200, 37), 3, (3, 1), 40, 16
DEC_LAYOUTS = ("blmhd", "blhmd", "paged")
DEC_PAGED_L = 2


class CacheMap:
    """Where the rows of a K or V cache lie.  shape: the tensor the operator takes; offset(b, row, h): elements from the
    cache pointer; terms as in Placement."""

    def __init__(self, layout, D, itemsize, far, B=DEC_B, lens=DEC_LENS, n=DEC_N):
        self.layout, self.D, self.itemsize, self.far, self.B = layout, D, itemsize, far, B
        Hkv, M, PS = DEC_HKV, DEC_M, DEC_PS
        pps = M // PS
        if layout == "paged":
            self.L, self.layer = DEC_PAGED_L, DEC_PAGED_L - 1
            self.page_stride = self.L * PS * Hkv * D
            first = -(-FAR // self.page_stride) if far else 3
            self.num_pages = first + B * pps
            # sequence b owns the highest pages, downwards; entries past the last page it touches (the sentinel rows
            # included) hold -1
            self.table = np.full((B, pps), -1, np.int32)
            for b in range(B):
                need = -(-(lens[b] + n + DEC_TAIL) // PS)
                self.table[b, :need] = self.num_pages - 1 - (b * pps + np.arange(need))
            self.shape = (self.num_pages, self.L, PS, Hkv, D)
        else:
            per_layer = M * Hkv * D
            # the smallest L at which sequence B - 1's last layer lies beyond FAR
            self.L = -(-(-(-FAR // per_layer) + 1) // B) if far else 1
            self.layer = self.L - 1
            self.shape = (B, self.L, M, Hkv, D) if layout == "blmhd" else (B, self.L, Hkv, M, D)
        self.elems = int(np.prod(self.shape, dtype=np.int64))

    def row_offsets(self):
        """[B, M, Hkv] element offsets of the rows from the cache pointer; -1 where a page is not mapped"""
        Hkv, M, PS, D = DEC_HKV, DEC_M, DEC_PS, self.D
        b = np.arange(self.B, dtype=np.int64)[:, None, None]
        r = np.arange(M, dtype=np.int64)[None, :, None]
        h = np.arange(Hkv, dtype=np.int64)[None, None, :]
        if self.layout == "blmhd":
            return ((b * self.L + self.layer) * M + r) * Hkv * D + h * D
        if self.layout == "blhmd":
            return (((b * self.L + self.layer) * Hkv + h) * M + r) * D
        pg = self.table.astype(np.int64)[:, np.arange(M) // PS][:, :, None]
        x = pg * self.page_stride + ((self.layer * PS + r % PS) * Hkv + h) * D
        return np.where(pg < 0, -1, x)

    def terms(self):
        Hkv, M, PS, D = DEC_HKV, DEC_M, DEC_PS, self.D
        kind = "far" if self.far else "near"
        if self.layout == "paged":
            return {"page": (int(self.table[self.table >= 0].min()) * self.page_stride, kind),
                    "layer": (self.layer * PS * Hkv * D, "near"), "row in page": ((PS - 1) * Hkv * D, "near"),
                    "head": ((Hkv - 1) * D, "near")}
        row, head = (Hkv * D, D) if self.layout == "blmhd" else (D, M * D)
        return {"layer": (((self.B - 1) * self.L + self.layer) * M * Hkv * D, kind), "row": ((M - 1) * row, "near"),
                "head": ((Hkv - 1) * head, "near")}

    def offsets(self):
        """every offset a call can form: the rows', and the far term alone for every sequence"""
        x = self.row_offsets().ravel()
        if self.layout == "paged":
            alone = self.table[self.table >= 0].astype(np.int64) * self.page_stride
        else:
            alone = (np.arange(self.B, dtype=np.int64) * self.L + self.layer) * DEC_M * DEC_HKV * self.D
        return np.unique(np.concatenate([x[x >= 0], alone]))

    def safe_in(self, arena_bytes, base):
        lo = base * self.itemsize
        t = truncations(self.offsets(), self.itemsize) + lo
        x = self.offsets() * self.itemsize + lo
        end = arena_bytes - self.D * self.itemsize
        return bool(min(t.min(), x.min()) >= 0 and max(t.max(), x.max()) <= end and self.elems * self.itemsize + lo <= arena_bytes)


def decode_arena_bytes(cm):
    """K behind the guard, V behind K: K is V's guard"""
    return up((GUARD + 2 * cm.elems) * cm.itemsize, 4096)


def decode_cache_maps():
    """every far cache of the decode GPU module: id -> CacheMap"""
    return {"%s-D%d-%dbit" % (lay, D, 8 * isz): CacheMap(lay, D, isz, True)
            for lay in DEC_LAYOUTS for D, isz in ((128, 2), (128, 1), (64, 1))}


# qkv with a far stride: (shape of the rows, strides in elements); args->stride is an int and 2^30 its largest power of two
QKV_STRIDE = 2 ** 30
QKV_CASES = {
    "single-batch": dict(call="", B=3, lens=(200, 37, 5), ns=(1, 1, 1), rows=(3,), strides=(QKV_STRIDE,)),
    "chunk-batch": dict(call="_chunk", B=3, lens=(200, 37, 5), ns=(3, 3, 3), rows=(3, 3), strides=(QKV_STRIDE, None)),
    # (a chunk's batch stride is then n * token stride, which no int holds: args->stride = 0, one sequence)
    "chunk-token": dict(call="_chunk", B=1, lens=(200,), ns=(3,), rows=(1, 3), strides=(3 * QKV_STRIDE, QKV_STRIDE)),
    "varlen-token": dict(call="_varlen", B=2, lens=(200, 37), ns=(2, 1), rows=(3,), strides=(QKV_STRIDE,)),
}


def qkv_placement(name, D=128):
    c = QKV_CASES[name]
    row = (DEC_HQ + 2 * DEC_HKV) * D
    strides = tuple(row if s is None else s for s in c["strides"])
    top = sum((n - 1) * s for n, s in zip(c["rows"], strides))
    return Placement("qkv", name, c["rows"], strides, row, {"stride": (top, "far")})
