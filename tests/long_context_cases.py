"""Long-context decode cases: all 18 decode entry points at memory_max_len 32768 and 131072, numpy only,
for tests/test_long_context_cpu.py (structure, preconditions, conditions on the inputs) and tests/test_long_context_gpu.py.

A case is a repr-able dict of Python scalars and lists.  materialise(case) turns it into what the Device class of
tests/serving_device.py takes -- trace = dict(geo, table, calls = [call]), data = the arrays -- plus the tokens of the
call and the rows that were planted.

Sections A and B: softmax over 10^5 keys with inputs under which it can fail.
  * The background cache is drawn once per (M, Hkv, D, L, storage type): K = 0.15 N(0,1), so that background scores stay
    within +-1 (checked), V = N(0,1).  Every row is its own draw.
  * q = u + 0.25 N(0,1) per token and head, u a +-1 sign vector per (sequence, kv head).  A planted row holds
    K = alpha * (mean of the rotated, rounded queries of its kv head's group over the tokens), alpha chosen so that the
    smallest planted score of the sequence is PLANT_SCORE = 16: exp(16) against a background of 131072 * exp(+-1).  All
    planted rows of a sequence therefore weigh about the same, and each has V = +-PLANT_V in a dim of its own, so that
    its weight can be read off o.
  * Planted rows: see planted_rows().  The row just below the window is planted too and must not count.
  * A: rotary_embedding_dim 0.  B: rot in {D/2, D} through the cos/sin tables, with biases.
Section C (in-kernel trigonometry at far positions): see envelope(), probe_*() and invariant_case() below.
"""
import functools

import numpy as np

import kv8_ref
import serving_cases as sc
import serving_model as sm
from oracle import rotary_table_ref, round_to, to_bits16
from oracle.decode_ref import _inv_freq
from window_ref import window_lo

TOL = {"fp16": 2e-3, "bf16": 1.6e-2}            # the project's decode tolerances, atol = rtol; nothing is loosened for length
B = 3
M_VALUES = (32768, 131072)
LAYOUTS = (("blmhd", 16), ("blhmd", 16), ("paged", 16), ("paged", 128))     # (kv_layout, page size)
SPLITS = (0, 1, 7, 32)
PLANT_SCORE, PLANT_V, BG_K = 16.0, 32.0, 0.15
K_SCALE, V_SCALE = (0.017, 0.023), (0.09, 0.075)   # per kv head: PLANT_V / V_SCALE <= 427 and a planted |k| <= 7 stays below 448
TILE = 32                                       # keys per tile of the matrix-core decode body (decode_mfma_common.h, kTile)

# (M, Hkv, D, L, layer).  One 16-bit cache is B * L * M * Hkv * D * 2 bytes <= 201 MB.  L = 2 only at 32768.
GEOS = ((131072, 2, 64, 1, 0), (131072, 1, 128, 1, 0), (32768, 2, 128, 2, 1), (32768, 1, 64, 2, 1))
GEO_D256 = (32768, 1, 256, 1, 0)                # head_dim 256: the single-token 16-bit entries only
# Groups.  sfa_decode picks by decode_dispatch.hip: G = 1 decode_kernel; matrix cores for G = 16, for G = 8, and for G = 4 at
# head_dim 128; decode_gqa_kernel otherwise (G = 2, and G = 4 at head_dim 64).  No debug key reports the kernel that ran.
# The fp64 model repeats K and V per query head, T * H * D * 8 bytes each: at 131072 rows H * D stays <= 1024.
GROUPS_BY_GEO = {GEOS[0]: (1, 2, 4, 8), GEOS[1]: (1, 2, 4, 8), GEOS[2]: (1, 2, 4, 8, 16), GEOS[3]: (1, 2, 4, 8, 16), GEO_D256: (1, 4)}


def varlen_by_role(n_far, i):
    """tokens of the (far, middle, short) sequence of a varlen call: [n_far, 0, 3] or [n_far, 2, 0]"""
    return (n_far, 0, 3 if n_far > 4 else 2) if (i // 2) % 2 else (n_far, 3 if n_far > 4 else 2, 0)


def reads_far_table(c):
    """a token of the case is rotated through the cos / sin tables at a row past 65535"""
    return c["tables"] and any(n and pos + n - 1 >= 65536 for pos, n in zip(c["pos"], c["n"]))


def far_positions(M):
    """the far rows: the last rows always; at 131072 the rows around 2^16 and 98304 + 17"""
    return ("last",) if M < 131072 else ("last", 65535, 65536, 65537, 98304 + 17)


def windows(M):
    return (1, 4096, M, 2 * M) + ((65536 + 17,) if M == 131072 else ())


def mid_position(M, k):
    """on no tile or page boundary; 40000 + odd where the cache has that many rows"""
    return (40001 if M > 65536 else 20001) + 16 * (k % 50) + 2 * (k % 3)         # pos % 16 in (1, 3, 5)


def _cases():
    """A covering design, not a product: every entry with every layout (72 cases), everything else
    cycled so that the coverage table of tests/test_long_context_cpu.py holds."""
    out = []
    i = 0
    for kv8 in (False, True):
        for si, shape in enumerate(sc.SHAPES):
            for fi, flavour in enumerate(sc.FLAVOURS):
                for li, (layout, ps) in enumerate(LAYOUTS):
                    geo = GEOS[(i + i // 4) % 4]         # (every geometry meets every layout)
                    M, Hkv, D, L, layer = geo
                    groups = GROUPS_BY_GEO[geo]
                    G = groups[(i // 4 + li + i // 12) % len(groups)]
                    fars = far_positions(M)
                    far = fars[(i // 4) % len(fars)]
                    window = None
                    if flavour:
                        ws = windows(M)
                        window = ws[(i // 3 + li + 4 * (i // 12)) % len(ws)]
                    small_window = window is not None and window <= 4096
                    section = "AB"[(i // 4 + li) % 2]
                    # n <= 4 over the full key range (the model's time); up to 40 under a small window, without rotation:
                    # a planted key is one vector for all tokens, and 40 rotated queries share too little of one
                    many = small_window and section == "A"
                    order = [(0, 1, 2), (2, 0, 1), (1, 2, 0), (2, 1, 0), (0, 2, 1), (1, 0, 2)][i % 6]
                    # roles: 0 = far, 1 = middle, 2 = short; the role of batch slot b is order[b].  n goes by role: the far
                    # sequence always has tokens, and the empty sequence of a varlen call is the middle or the short one
                    if shape == "_chunk":
                        by_role = [(2, 4, 3)[i % 3]] * B if not many else [(40, 7)[i % 2]] * B
                    elif shape == "_varlen":
                        by_role = varlen_by_role(40 if many else 4, i)
                    else:
                        by_role = [1] * B
                    n = [by_role[role] for role in order]
                    pos = []
                    for b in range(B):
                        role = order[b]
                        if role == 0:
                            pos.append(M - n[b] if far == "last" else far)
                        elif role == 1:
                            pos.append(mid_position(M, i))
                        else:
                            pos.append((0, 3)[i % 2])
                    rot = 0 if section == "A" else (D // 2, D)[(i // 2) % 2]
                    out.append(dict(id=len(out), section=section, kv8=kv8, dtype=("fp16", "bf16")[(i + si) % 2],
                                    M=M, Hkv=Hkv, G=G, D=D, L=L, layer=layer, layout=layout, ps=ps, rot=rot,
                                    tables=rot > 0, bias=rot > 0, entry=sc.entry_name(shape, flavour, kv8), shape=shape,
                                    flavour=flavour, pos=pos, n=n, far=far, order=list(order), window=window,
                                    num_splits=SPLITS[(fi + li) % 4]))
                    i += 1
    # head_dim 256, single-token 16-bit entries
    for j, flavour in enumerate(sc.FLAVOURS):
        M, Hkv, D, L, layer = GEO_D256
        out.append(dict(id=len(out), section="A", kv8=False, dtype=("fp16", "bf16")[j % 2], M=M, Hkv=Hkv, G=(1, 4, 1)[j], D=D, L=L,
                        layer=layer, layout=LAYOUTS[j][0], ps=LAYOUTS[j][1], rot=0, tables=False, bias=False,
                        entry=sc.entry_name("", flavour, False), shape="", flavour=flavour,
                        pos=[mid_position(M, j), M - 1, 3], n=[1] * B, far="last", order=[1, 0, 2],
                        window=None if not flavour else (4096, 2 * M)[j % 2], num_splits=(0, 7, 32)[j]))
    # sfa_decode's three kernels at both lengths: the grouped scalar kernel at 32768 and the matrix-core body at 131072
    # ... and each of them through the cos / sin tables at a row past 65535
    for j, (geo, G, far, dtype) in enumerate(((GEOS[3], 2, "last", "bf16"), (GEOS[1], 8, 65536, "fp16"),
                                              (GEOS[0], 1, 65537, "bf16"), (GEOS[0], 2, "last", "fp16"))):
        M, Hkv, D, L, layer = geo
        out.append(dict(id=len(out), section="B", kv8=False, dtype=dtype, M=M, Hkv=Hkv, G=G, D=D, L=L, layer=layer,
                        layout=LAYOUTS[(2 + j) % 4][0], ps=LAYOUTS[(2 + j) % 4][1], rot=(D // 2, D)[j // 2], tables=True, bias=True,
                        entry="flash_decode",
                        shape="", flavour="", pos=[0, M - 1 if far == "last" else far, mid_position(M, j)], n=[1] * B, far=far,
                        order=[2, 0, 1], window=None, num_splits=(0, 32, 7, 1)[j]))
    # every entry point reads its cos / sin tables at a row past 65535 (the prologues are several: decode_kernel, the grouped
    # kernels, the windowed and fp8 single-token kernels, the chunk body): a case of its own where the design above has none
    have = {c["entry"] for c in out if reads_far_table(c)}
    for j, entry in enumerate(e for e in sc.ENTRIES if e not in have):
        kv8 = "_kv8" in entry
        shape = "_chunk" if "_chunk" in entry else "_varlen" if "_varlen" in entry else ""
        flavour = "_window_sinks" if "_sinks" in entry else "_window" if "_window" in entry else ""
        M, Hkv, D, L, layer = GEOS[j % 2]
        order = [(1, 0, 2), (2, 1, 0)][j % 2]
        by_role = {"": [1] * B, "_chunk": [3] * B, "_varlen": varlen_by_role(4, j)}[shape]
        far = (65536, 65537, 98304 + 17)[j % 3]
        out.append(dict(id=len(out), section="B", kv8=kv8, dtype=("bf16", "fp16")[j % 2], M=M, Hkv=Hkv, G=(2, 1, 4)[j % 3], D=D, L=L,
                        layer=layer, layout=LAYOUTS[j % 4][0], ps=LAYOUTS[j % 4][1], rot=(D, D // 2)[j % 2], tables=True, bias=True,
                        entry=entry, shape=shape, flavour=flavour, pos=[(far, mid_position(M, j), 3)[r] for r in order],
                        n=[by_role[r] for r in order], far=far, order=list(order),
                        window=(None if not flavour else (M, 65536 + 17)[j % 2]), num_splits=SPLITS[j % 4]))
    return sorted(out, key=lambda c: (bg_key(c), c["id"]))     # neighbours share a background cache


def bg_key(c):
    """what a background cache is built once for"""
    return (c["M"], c["Hkv"], c["D"], c["L"], "e4m3" if c["kv8"] else c["dtype"])


CASES = _cases()


def _invariant_cases():
    """Section C, rotation-invariant problems: rot = D / 2 with the trigonometry in the kernel; the cached K rows are zero in
    the rotated dims, and token t of a sequence has q and k nonzero there only on its own pair, own_pair(t): distinct across the tokens.  Then q_t . k_s
    vanishes on the rotated dims for s != t, and q_t . k_t is the unrotated product whatever angle both were rotated by: the
    model's o does not depend on the inv_freq the device used, and the ordinary TOL applies.  The own-token score carries
    OWN_SCORE more than a planted cached row, so a kernel that rotates q_t and k_t at different positions loses it.
    The three shapes, both cache types, windowed and not, at the far positions; M = 131072."""
    out = []
    fars = far_positions(131072)
    i = 0
    for kv8 in (False, True):
        for shape in sc.SHAPES:
            for flavour in ("", "_window"):
                M, Hkv, D, L, layer = GEOS[i % 2]
                far = fars[i % len(fars)]
                order = [(0, 1, 2), (2, 0, 1), (1, 2, 0)][i % 3]
                by_role = {"": [1] * B, "_chunk": [4] * B, "_varlen": varlen_by_role(4, i // 2)}[shape]
                n = [by_role[role] for role in order]
                pos = [(M - n[b] if far == "last" else far) if order[b] == 0 else mid_position(M, i) if order[b] == 1 else 3
                       for b in range(B)]
                layout, ps = LAYOUTS[i % 4]
                out.append(dict(id=1000 + i, section="C", kv8=kv8, dtype=("fp16", "bf16")[(i // 2) % 2], M=M, Hkv=Hkv,
                                G=(1, 2, 4, 8)[(i // 2) % 4], D=D, L=L, layer=layer, layout=layout, ps=ps, rot=D // 2,
                                tables=False, bias=False, entry=sc.entry_name(shape, flavour, kv8), shape=shape, flavour=flavour,
                                pos=pos, n=n, far=far, order=list(order), window=4096 if flavour else None, num_splits=(0, 7)[i % 2]))
                i += 1
    return out


OWN_SCORE, OWN_Q = 3.0, 4.0


def own_pair(t, rot):
    """The rotated pair token t of a rotation-invariant problem lives on.  t >= 1: the pair that turns by about 0.6 rad over t
    rows, so that a query rotated at pos instead of pos + t loses a sixth of its own-token score, while the envelope's width
    at that frequency (2 ulps of inv_freq at row 131071: 0.03 rad * f) changes q . k only in the second order.  Token 0 has no
    such mismatch to show and takes the slowest pair."""
    if t == 0:
        return rot // 2 - 1
    return int(np.argmin(np.abs(_inv_freq(rot).astype(np.float64) - 0.6 / t)))


INVARIANT_CASES = _invariant_cases()


def case_id(c):
    return "%03d-%s-%s%d-%s-M%d-Hkv%d-G%d-D%d-%s-S%d-w%s-far%s-n%s" % (
        c["id"], c["entry"], c["layout"], c["ps"], c["dtype"], c["M"], c["Hkv"], c["G"], c["D"],
        c["section"] + (str(c["rot"]) if c["rot"] else ""), c["num_splits"], c["window"], c["far"], "_".join(map(str, c["n"])))


@functools.lru_cache(maxsize=2)
def background(key):
    """kc, vc = canonical storage bits [B, L, M, Hkv, D] (read-only), drawn through a 256-entry table of representable
    values per cache (quantiles of N(0, BG_K^2) for K and N(0,1) for V) so that 10^8 elements take a second"""
    M, Hkv, D, L, storage = key
    rng = np.random.default_rng([21, M, Hkv, D, L, ("fp16", "bf16", "e4m3").index(storage)])
    z = np.sort(np.random.default_rng(22).standard_normal(256))
    shape = (B, L, M, Hkv, D)
    out = {}
    for name, amp in (("kc", BG_K), ("vc", 1.0)):
        idx = rng.integers(0, 256, shape, dtype=np.uint8)
        if storage == "e4m3":
            scale = np.asarray((K_SCALE if name == "kc" else V_SCALE)[:Hkv], np.float32)
            lut = np.stack([kv8_ref.quantize(np.broadcast_to((amp * z)[:, None, None], (256, Hkv, 1)), scale)[:, h, 0]
                            for h in range(Hkv)])                                        # [Hkv, 256]
            bits = np.empty(shape, np.uint8)
            for h in range(Hkv):
                bits[..., h, :] = lut[h][idx[..., h, :]]
        else:
            bits = to_bits16(round_to(amp * z, storage), storage)[idx]
        bits.setflags(write=False)
        out[name] = bits
    return out


def block_table(c):
    """a permuted table whose stride is wider than M / page_size, with spare pages"""
    need = c["M"] // c["ps"]
    stride = need + 3
    num_pages = B * stride + sc.SPARE
    rng = np.random.default_rng([23, c["M"], c["ps"]])       # (one table per geometry: the device copy of a background is reused)
    return rng.permutation(num_pages)[:B * stride].astype(np.int32).reshape(B, stride), stride, num_pages


def planted_rows(pos, n, window):
    """(visible, below) of one sequence: the cached rows to plant that at least one token sees, ascending, and the row just
    below token 0's window (None when there is none).  Visible: the first visible row of token 0 and of the last token,
    the last cached row, rows 65535 and 65536, and rows beside multiples of pos / 32 and pos / 7 (where the key range is
    cut for 32 and 7 splits), +-1 and +- one tile of 32 rows (pos / 32) or of 64 rows (pos / 7)."""
    lo0 = window_lo(pos, window)
    want = {lo0, window_lo(pos + n - 1, window), pos - 1, 65535, 65536}
    for base, mults, tile in ((pos // 32, (1, 17, 31), TILE), (pos // 7, (3, 6), 2 * TILE)):
        for m in mults:
            want |= {m * base + d for d in (-tile, -1, 1, tile)}
    visible = sorted(r for r in want if lo0 <= r <= pos - 1)
    return visible, (lo0 - 1 if lo0 >= 1 else None)


def auto_splits(lib, c):
    """The split count the library picks for the case when num_splits = 0, from its exported host functions alone:
    sfa_decode_auto_splits for sfa_decode / sfa_decode_kv8; for the others the count S whose workspace size is the one the
    sizing function returns for 0 (the partials grow with S; the smallest such S when a rounding makes several agree)."""
    H, windowed = c["Hkv"] * c["G"], c["window"] is not None
    if not c["shape"] and not windowed:
        return lib.sfa_decode_auto_splits(B, c["Hkv"], c["D"], c["M"])
    size = getattr(lib, "sfa_decode" + c["shape"] + ("_window" if windowed else "") + "_workspace_bytes")
    dims = [B, H, c["Hkv"], c["D"], c["M"]] + ([c["n"][0] if c["shape"] == "_chunk" else sum(c["n"])] if c["shape"] else [])
    dims += [c["window"]] if windowed else []
    same = [S for S in range(1, 33) if size(*dims, S) == size(*dims, 0)]
    assert same, (c["id"], dims)
    return same[0]


COLD_SCORE = 100.0


def cold_alone(c, b):
    """The first token of a sequence at position 0 of a 16-bit cache without sinks sees its own row alone, so o = v whatever the
    score: its key is turned round, and the score is at most -COLD_SCORE (later tokens of a chunk see that cold row and their own
    hot one).  With the key range split, every other partial of that sequence
    is empty; a combine that gives an empty partial a maximum of 0 instead of -inf scales the only real one by exp(-100) and
    loses it in fp32 (exp2 of -144 underflows).  Not over an fp8 cache: |k| <= 448 * k_scale = 7.6 bounds the score at about
    -79 (head_dim 128), which fp32 still carries, so the break would not show."""
    return c["pos"][b] == 0 and c["n"][b] >= 1 and not c["kv8"] and c["flavour"] != "_window_sinks" and c["section"] != "C"


def check_preconditions(geo, call, table, k_scale=None, v_scale=None):
    """serving_cases.check_preconditions, which knows the head dims every entry point serves; head_dim 256 is the header's
    for the single-token calls over a 16-bit cache only, and is checked here"""
    if geo["D"] == 256:
        assert call["shape"] == "" and not geo["kv8"], call["entry"]
        geo = dict(geo, D=128)
    sc.check_preconditions(geo, call, table, k_scale, v_scale)


def _geo(c, stride, num_pages):
    return dict(seed=c["id"], kv8=c["kv8"], dtype=c["dtype"], B=B, Hkv=c["Hkv"], G=c["G"], H=c["Hkv"] * c["G"], D=c["D"], L=c["L"],
                layer=c["layer"], layout=c["layout"], ps=c["ps"], M=c["M"], stride=stride, num_pages=num_pages, rot=c["rot"],
                tables=c["tables"], bias=c["bias"])


def _plant_v(i, Hkv, D, rng):
    """the V row of the i-th planted row of a sequence: +-PLANT_V in a dim of its own per kv head, small elsewhere"""
    v = 0.25 * rng.standard_normal((Hkv, D))
    for h in range(Hkv):
        v[h, (i + 5 * h) % D] = PLANT_V * (-1) ** i
    return v


def materialise(c):
    """The arrays of a case.  Returns dict(trace, data, tokens, visible, below, call): data["kc"] / ["vc"] are the
    background with the planted rows written in (a copy); call is trace["calls"][0] with the sinks filled in."""
    g_table, stride, num_pages = block_table(c)
    geo = _geo(c, stride, num_pages)
    H, Hkv, G, D, M, dtype, kv8, layer = geo["H"], c["Hkv"], c["G"], c["D"], c["M"], c["dtype"], c["kv8"], c["layer"]
    rng = np.random.default_rng([24, c["id"]])
    bg = background(bg_key(c))
    data = dict(q_bias=None, k_bias=None, v_bias=None, cos=None, sin=None, k_scale=None, v_scale=None)
    if kv8:
        data["k_scale"], data["v_scale"] = np.asarray(K_SCALE[:Hkv], np.float32), np.asarray(V_SCALE[:Hkv], np.float32)
    if c["bias"]:
        r = lambda h: round_to(0.1 * rng.standard_normal((h, D)), dtype)
        data["q_bias"], data["k_bias"], data["v_bias"] = r(H), r(Hkv), r(Hkv)
    if c["tables"]:
        data["cos"], data["sin"] = rotary_table_ref(M, c["rot"], dtype)
    qb, kb, vb = (0.0 if data[k] is None else np.asarray(data[k], np.float64) for k in ("q_bias", "k_bias", "v_bias"))
    kc, vc = bg["kc"].copy(), bg["vc"].copy()
    if c["section"] == "C":
        kc[..., :c["rot"]] = 0           # (+0 in every storage type)
    tokens, vis_all, below_all = [], [], []
    smax = -np.inf
    for b, (pos, n) in enumerate(zip(c["pos"], c["n"])):
        visible, below = planted_rows(pos, n, c["window"])
        vis_all.append(visible)
        below_all.append(below)
        if n == 0:                      # no token: nothing is read or written; the rows stay background
            tokens.append(np.zeros((0, H + 2 * Hkv, D), np.float32))
            continue
        u = rng.choice([-1.0, 1.0], size=(Hkv, D))
        q = np.repeat(u, G, axis=0)[None] + 0.25 * rng.standard_normal((n, H, D))
        if c["section"] == "C":         # the rotated dims: token t's own pairs only, (1, 0.5) each
            own = np.zeros((n, c["rot"]))
            assert len({own_pair(t, c["rot"]) for t in range(n)}) == n
            for t in range(n):
                own[t, 2 * own_pair(t, c["rot"])], own[t, 2 * own_pair(t, c["rot"]) + 1] = 1.0, 0.5
            q[:, :, :c["rot"]] = OWN_Q * own[:, None, :]
        q = round_to(q, dtype).astype(np.float64)
        tok = np.zeros((n, H + 2 * Hkv, D), np.float64)
        tok[:, :H] = q
        # the rotated, rounded queries: serving_model.prologue (k and v of the tokens do not enter them)
        call0 = sm.make_call(dtype, H, c["pos"], c["n"], [tok if bb == b else None for bb in range(B)], layer, c["rot"],
                             q_bias=data["q_bias"], cos=data["cos"], sin=data["sin"])
        q16 = sm.prologue(call0, b)[0]                                          # [n, H, D]
        kdir = q16.reshape(n, Hkv, G, D).mean(axis=(0, 2))                      # the component the group and the tokens share
        if c["section"] == "C":
            kdir[:, :c["rot"]] = 0.0
        s = np.einsum("nkgd,kd->nkg", q16.reshape(n, Hkv, G, D), kdir) / np.sqrt(D)
        assert s.min() > 0.1 * np.sqrt(D), (c["id"], b, s.min())
        alpha = PLANT_SCORE / s.min()
        if not (cold_alone(c, b) and n == 1):
            smax = max(smax, alpha * s.max())
        krow = round_to(alpha * kdir, dtype)
        assert np.abs(krow).max() <= 7.0, (c["id"], b, np.abs(krow).max())
        rows = visible + ([below] if below is not None else [])
        for i, r in enumerate(rows):
            kc[b, layer, r] = sm.store(krow, dtype, kv8, data["k_scale"])
            vc[b, layer, r] = sm.store(round_to(_plant_v(i, Hkv, D, rng), dtype), dtype, kv8, data["v_scale"])
        # the new tokens are planted rows too: k_new = alpha * (the group's mean query, bias included) before rotation
        tok[:, H:H + Hkv] = alpha * (q + qb).reshape(n, Hkv, G, D).mean(axis=2) - kb
        if cold_alone(c, b):
            tok[0, H:H + Hkv] *= -COLD_SCORE / PLANT_SCORE
        if c["section"] == "C":         # q_t . k_t over the token's own pairs = OWN_SCORE * sqrt(D), under any common rotation
            tok[:, H:H + Hkv, :c["rot"]] = own[:, None, :] * OWN_SCORE * np.sqrt(D) / (1.25 * OWN_Q)
        for t in range(n):
            tok[t, H + Hkv:] = _plant_v(len(rows) + t, Hkv, D, rng) - vb
        tokens.append(round_to(tok, dtype))
    sinks = None
    if c["flavour"] == "_window_sinks":     # from a few units below to a few above the largest score; one head at -inf
        sinks = [float(np.float32(smax + x)) for x in (np.linspace(-3.0, 3.0, H) if H > 1 else [1.0])]
        if H > 1:
            sinks[(c["id"] * 7) % H] = float("-inf")
    call = dict(seed=c["id"], kv8=kv8, step=0, entry=c["entry"], shape=c["shape"], flavour=c["flavour"], pos=list(c["pos"]),
                n=list(c["n"]), window=c["window"], sinks=sinks, num_splits=c["num_splits"], softmax_scale=None)
    data["kc"], data["vc"] = kc, vc
    return dict(trace=dict(geo=geo, table=g_table, calls=[call]), data=data, tokens=tokens, visible=vis_all,
                below=below_all, call=call)


def weights(mc, cache_after, b, extra_row=None, q16=None):
    """The model's attention of sequence b written out with its weights: (o [n, H, D], p [n, H, T_all] with zero outside a
    token's rows, V [T_all, H, D], e).  The expressions are serving_model.attend_rows'.  extra_row: a row below token 0's
    window; e [H] is then the weight it would get in token 0's softmax, relative to the present denominator."""
    kbits, vbits = cache_after[0][b, mc["layer"]], cache_after[1][b, mc["layer"]]
    pos, n, H = mc["pos"][b], mc["n"][b], mc["H"]
    Hkv, D = kbits.shape[1], kbits.shape[2]
    G = H // Hkv
    q16 = sm.prologue(mc, b)[0] if q16 is None else q16
    scale = 1.0 / np.sqrt(float(D)) if mc["softmax_scale"] is None else mc["softmax_scale"]
    ks = vs = None
    if sm.is_kv8(kbits):
        ks, vs = np.asarray(mc["k_scale"], np.float32), np.asarray(mc["v_scale"], np.float32)
    sk = (np.full(H, -np.inf) if mc["sinks"] is None else np.asarray(mc["sinks"], np.float64))[:, None]
    lo_all = window_lo(pos, mc["window"])
    T = pos + n - lo_all
    K = sm.values(kbits[lo_all:pos + n], mc["dtype"], ks)                       # [T, Hkv, D]
    V = sm.values(vbits[lo_all:pos + n], mc["dtype"], vs)
    o = np.zeros((n, H, D))
    p_all = np.zeros((n, H, T))
    e = None
    for t in range(n):
        lo = window_lo(pos + t, mc["window"]) - lo_all
        hi = pos + t + 1 - lo_all
        s = np.einsum("kgd,tkd->kgt", q16[t].reshape(Hkv, G, D), K[lo:hi]).reshape(H, hi - lo) * scale
        m0 = s.max(axis=1, keepdims=True)
        mx = np.maximum(m0, sk)
        p = np.exp(s - mx)
        den = p.sum(axis=1, keepdims=True) + np.exp(sk - mx)
        p /= den
        p_all[t, :, lo:hi] = p
        o[t] = np.einsum("kgt,tkd->kgd", p.reshape(Hkv, G, hi - lo), V[lo:hi]).reshape(H, D)
        if t == 0 and extra_row is not None:
            kx = sm.values(kbits[extra_row:extra_row + 1], mc["dtype"], ks)[0]  # [Hkv, D]
            sx = np.einsum("kgd,kd->kg", q16[0].reshape(Hkv, G, D), kx).reshape(H) * scale
            e = np.exp(sx - mx[:, 0]) / den[:, 0]
    return o, p_all, V, e, lo_all, K


def mutation_margins(m):
    """For every sequence of a materialised case: the smallest, over the planted visible rows (cached and new), of
    max_elements |o_without_row - o| / (TOL + TOL |o|), and the same for admitting the row below the window.  Dropping row
    r renormalises the other weights: o' = (o - p_r V_r) / (1 - p_r).  Both must be >= 10.  Also returns the largest
    |background score|."""
    c, data = m["call"], m["data"]
    geo = m["trace"]["geo"]
    mc = sc.model_call(geo, c, data, m["tokens"])
    cache = (data["kc"], data["vc"])
    after = sm.apply(cache, mc, sm.step(cache, mc)[0])
    tol = TOL[geo["dtype"]]
    G = geo["G"]
    out = []
    for b, (pos, n) in enumerate(zip(c["pos"], c["n"])):
        if n == 0:
            continue
        o, p, V, e, lo_all, K = weights(mc, after, b, m["below"][b])
        rows = [r - lo_all for r in m["visible"][b]] + [pos + t - lo_all for t in range(n)]
        drop = np.inf
        for r in rows:
            pr = p[:, :, r][:, :, None]                                         # [n, H, 1]
            with np.errstate(invalid="ignore", divide="ignore"):            # (a token that sees this row alone: p = 1)
                o2 = (o - pr * np.repeat(V[r], G, axis=0)[None]) / (1.0 - pr)
            ratio = np.nan_to_num(np.abs(o2 - o) / (tol + tol * np.abs(o)), nan=np.inf)
            drop = min(drop, ratio.max())
        admit = np.inf
        if m["below"][b] is not None:
            vx = np.repeat(sm.values(after[1][b, mc["layer"], m["below"][b]:m["below"][b] + 1], geo["dtype"],
                                     data["v_scale"])[0], G, axis=0)            # [H, D]
            o2 = (o[0] + e[:, None] * vx) / (1.0 + e[:, None])
            admit = (np.abs(o2 - o[0]) / (tol + tol * np.abs(o[0]))).max()
        # background scores of token 0: every row but the planted ones
        q16 = sm.prologue(mc, b)[0][0].reshape(geo["Hkv"], G, geo["D"])
        s = np.einsum("kgd,tkd->kgt", q16, K[:pos - lo_all]) / np.sqrt(geo["D"])
        s[:, :, [r - lo_all for r in m["visible"][b]]] = 0.0
        out.append(dict(b=b, drop=float(drop), admit=float(admit), background=float(np.abs(s).max()) if s.size else 0.0))
    return out


# ---- section C: in-kernel trigonometry at far positions ---------------------------------------------------------------
#
# The contract: the kernel's angle for pair j at position p is fl32(p * f) for some fp32 f within ENVELOPE_ULPS = 2 ulps of
# oracle.decode_ref._inv_freq(rot)[j]: one ulp for powf's result and one for the reciprocal.  f is an fp32 number, so the
# envelope is five angles per (p, j); sincosf's own error (a few fp32 ulps of a value <= 1) is far inside the storage ulp
# the stored cos / sin are compared with.

ENVELOPE_ULPS = 2
PROBE_POSITIONS = (0, 1, 8191, 32767, 65536, 131071)
PROBE_M = 131072
STORAGE_ULP = {"fp16": (10, -14), "bf16": (7, -126)}    # mantissa bits, smallest normal exponent


def envelope(pos, rot):
    """[2 * ENVELOPE_ULPS + 1, rot / 2] float64: the angles fl32(pos * f), f = inv_freq moved by -2 .. +2 fp32 ulps"""
    f = _inv_freq(rot)
    out = []
    for d in range(-ENVELOPE_ULPS, ENVELOPE_ULPS + 1):
        fd = f.copy()
        for _ in range(abs(d)):
            fd = np.nextafter(fd, np.float32(np.inf if d > 0 else -np.inf), dtype=np.float32)
        out.append((np.float32(pos) * fd).astype(np.float32).astype(np.float64))
    return np.stack(out)


def ulps_between(a, b):
    """fp32 ulps from b to a (both positive float32)"""
    return np.asarray(a, np.float32).view(np.int32).astype(np.int64) - np.asarray(b, np.float32).view(np.int32).astype(np.int64)


def storage_ulp(x, dtype):
    """the spacing of dtype's numbers at |x|"""
    mant, emin = STORAGE_ULP[dtype]
    a = np.maximum(np.abs(np.asarray(x, np.float64)), 2.0 ** emin)
    return 2.0 ** (np.floor(np.log2(a)) - mant)


def probe_tokens(n, H, Hkv, D, rot, dtype):
    """[n, H + 2 Hkv, D]: k has (1, 0) in every pair, so that its rotated row is (cos, sin); q and v are small"""
    rng = np.random.default_rng([25, n, H, Hkv, D])
    tok = 0.25 * rng.standard_normal((n, H + 2 * Hkv, D))
    tok[:, H:H + Hkv] = 0.0
    tok[:, H:H + Hkv, 0::2] = 1.0
    return round_to(tok, dtype)


def consistent_deviations(krow, pos, rot, dtype):
    """krow [D] float: the stored rotated (1, 0) pairs.  Returns ok [2 U + 1, rot / 2] bool: deviation d is consistent with
    pair j when the fp64 cos and sin of the envelope angle are both within one storage ulp of what was stored."""
    ang = envelope(pos, rot)
    c, s = krow[0:rot:2][None], krow[1:rot:2][None]
    return (np.abs(np.cos(ang) - c) <= storage_ulp(c, dtype)) & (np.abs(np.sin(ang) - s) <= storage_ulp(s, dtype))


def check_probe_row(krow, pos, rot, dtype):
    """the 16-bit probe rule: every rotated pair has an envelope angle; the pairs past rot are (1, 0) untouched"""
    ok = consistent_deviations(krow, pos, rot, dtype)
    bad = np.flatnonzero(~ok.any(axis=0))
    assert bad.size == 0, f"position {pos} rot {rot}: pairs {bad.tolist()} hold cos / sin of no angle in the envelope"
    assert np.all(krow[rot::2] == 1.0) and np.all(krow[rot + 1::2] == 0.0), f"position {pos}: a pair past rot was rotated"
    return ok


def check_probe_bytes(kbytes, pos, rot, dtype, k_scale):
    """the fp8 probe rule, kbytes [Hkv, D] uint8: each byte lies between the codes of the envelope's extremes, widened by one
    e4m3 step"""
    ang = envelope(pos, rot)                                                    # [5, rot / 2]
    Hkv, D = kbytes.shape
    want = np.zeros((ang.shape[0], Hkv, D))
    want[:, :, 0::2] = 1.0
    want[:, :, 0:rot:2] = np.cos(ang)[:, None, :]
    want[:, :, 1:rot:2] = np.sin(ang)[:, None, :]
    codes = kv8_ref.E4M3[kv8_ref.quantize(round_to(want, dtype), k_scale)]      # values of the codes (before the scale)
    got = kv8_ref.E4M3[kbytes]
    lo, hi = codes.min(axis=0), codes.max(axis=0)
    step = kv8_ref.step_at(np.maximum(np.abs(lo), np.abs(hi)))
    bad = (got < lo - step) | (got > hi + step)
    assert not bad.any(), f"position {pos} rot {rot}: {int(bad.sum())} K bytes outside the envelope's codes"


def case_items(c):
    """what a case covers, as the strings of tests/test_long_context_cpu.py's coverage table"""
    M, D, G = c["M"], c["D"], c["G"]
    cache = "kv8" if c["kv8"] else "16bit"
    items = {"%s:%s%d" % (c["entry"], c["layout"], c["ps"] if c["layout"] == "paged" else 0),
             "splits:%d:%s:%s" % (c["num_splits"], c["shape"] or "_single", cache),
             "order:%d%d%d" % tuple(c["order"]), "M:%d:D:%d:%s" % (M, D, cache), "M:%d:%s%d" % (M, c["layout"], c["ps"]), "G:%d:M:%d" % (G, M),
             "section:%s:rot:%s:%s" % (c["section"], {0: "0", D // 2: "D/2", D: "D"}[c["rot"]], cache)}
    for b in range(B):
        if c["order"][b] == 0 and c["n"][b]:
            far = c["far"] if c["far"] != "last" else "M-1" if c["n"][b] == 1 else "M-n"
            items.add("far:%s:%s" % (far, c["dtype"]))
        if c["order"][b] == 2:
            items.add("short:%d" % c["pos"][b])
    if c["window"] is not None:
        w = {1: "1", 4096: "4096", 65536 + 17: "65536+17", M: "M", 2 * M: "2M"}[c["window"]]
        items.add("window:%s:M:%d" % (w, M))
    if c["entry"] == "flash_decode":    # decode_dispatch.hip's rule
        mfma = G == 16 or (G >= 4 and (D == 128 or G == 8))
        kernel = "decode_kernel" if G == 1 else "matrix-core" if mfma else "decode_gqa_kernel"
        items.add("flash_decode:%s:M:%d" % (kernel, M))
        if c["tables"] and max(c["pos"]) >= 65536:
            items.add("flash_decode:%s:table_row>=65536" % kernel)
    if reads_far_table(c):
        items.add("table_row>=65536:%s" % c["entry"])
    if any(cold_alone(c, b) for b in range(B)):
        items.add("cold_alone:S:%d:%s" % (c["num_splits"], c["entry"]))
    if max(c["n"]) == 40:
        items.add("n:40:%s" % (c["shape"]))
    if c["shape"] == "_varlen" and 0 in c["n"]:
        items.add("varlen:empty_sequence")
    return items


def rotated_envelope(k, pos, rot, dtype):
    """[2 U + 1, ..., D]: the row k (already rounded to dtype, bias included) rotated in fp64 by each angle of the envelope and
    rounded to dtype"""
    from oracle import rope_interleaved
    ang = envelope(pos, rot)
    return np.stack([round_to(rope_interleaved(k, pos, rot, cos=np.cos(a), sin=np.sin(a)), dtype) for a in ang]).astype(np.float64)


def check_k_row_envelope(got, k, pos, rot, dtype, ulp):
    """16-bit: every rotated pair of the stored row is, in both elements, within the suite's K rule (ulp * max(1, |k|) * 1.01) of
    the row rotated by ONE angle of the envelope; the dims past rot are the rule's as they stand"""
    want = rotated_envelope(k, pos, rot, dtype)
    ok = np.abs(got[None] - want) <= ulp * np.maximum(1.0, np.abs(got))[None] * 1.01
    pair_ok = (ok[..., 0:rot:2] & ok[..., 1:rot:2]).any(axis=0)
    assert pair_ok.all(), f"position {pos}: {int((~pair_ok).sum())} rotated pairs of an appended K row match no angle of the envelope"
    assert ok[0][..., rot:].all(), f"position {pos}: appended K row, the dims past rot"


def check_k_bytes_envelope(kbytes, k, pos, rot, dtype, k_scale):
    """fp8: every byte lies between the codes of the envelope's extremes, widened by one e4m3 step"""
    codes = kv8_ref.E4M3[kv8_ref.quantize(rotated_envelope(k, pos, rot, dtype), k_scale)]
    got = kv8_ref.E4M3[kbytes]
    lo, hi = codes.min(axis=0), codes.max(axis=0)
    step = kv8_ref.step_at(np.maximum(np.abs(lo), np.abs(hi)))
    bad = (got < lo - step) | (got > hi + step)
    assert not bad.any(), f"position {pos}: {int(bad.sum())} appended K bytes outside the envelope's codes"
