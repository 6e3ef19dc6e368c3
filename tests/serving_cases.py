"""The seeded generators of tests/test_serving_trace_gpu.py (serving traces over one KV cache) and
tests/test_fuzz_prefill_forwards_gpu.py (the five newer prefill forwards), numpy only, so that
tests/test_serving_model_cpu.py can hold them to their coverage table and to the header's preconditions without a GPU.

A trace is a dict(geo = the geometry drawn once, table = the block table [B, stride] int32, calls = six call
descriptions).  Everything in geo and in a call description is a Python scalar or a list of them: a description is
repr-able and names its trace (seed, kv8) and its step, which is all run_call() of the GPU file needs to rebuild it.
The arrays -- the initial cache, biases, tables, scales, the tokens of a call -- come from trace_data() and
call_tokens(), seeded by the same numbers.
"""
import numpy as np

import kv8_ref
from oracle import rotary_table_ref, round_to, to_bits16
from oracle.decode_ref import _inv_freq
import serving_model as sm

TRACE_SEEDS = tuple(range(32))                  # per cache type; dtype alternates with the seed
STEPS, UNSYNCED = 6, 3                          # calls per trace; how many of them go out before the first read-back
GROUPS = (1, 2, 4, 8, 16)                       # num_heads / num_heads_kv the windowed and fp8 entry points serve
HEAD_DIMS = (64, 128)                           # the head dims EVERY decode entry point serves (256: single-token only)
PAGE_SIZES = (16, 32, 64, 128)
M_MAX, H_MAX, N_MAX, SPARE = 512, 32, 40, 3
SHAPES = ("", "_chunk", "_varlen")
FLAVOURS = ("", "_window", "_window_sinks")
# fp8 caches, trigonometry in the kernel: the angle pos * inv_freq differs from numpy's in its last fp32 bit, which moves a
# nearly cancelling element of the rotated k by about 6e-8 * pos * |(x, y)|; around row 1000 that is several subnormal e4m3
# steps (2^-9 * k_scale ~ 1e-5) and "K within one e4m3 step" no longer holds for the reference itself
# (tests/chunk_kv8_window_ref.py, check()).  The rule is a condition on the inputs, so an fp8 trace that draws in-kernel
# trigonometry draws memory_max_len up to 256, the length at which tests/chunk_kv8_ref.py's suite holds the same rule with
# in-kernel trigonometry; the drawn rotary setting itself is never changed.
KV8_TRIG_M_MAX = 256


def entry_name(shape, flavour, kv8):
    return "flash_decode" + shape + ("_kv8" if kv8 else "") + flavour


ENTRIES = tuple(entry_name(s, f, kv8) for kv8 in (False, True) for s in SHAPES for f in FLAVOURS)


def make_trace(seed, kv8):
    rng = np.random.default_rng([7, int(kv8), seed])
    pick = lambda xs: xs[int(rng.integers(len(xs)))]
    B, Hkv, D = int(rng.integers(1, 7)), int(rng.integers(1, 5)), pick(HEAD_DIMS)
    G = pick([g for g in GROUPS if Hkv * g <= H_MAX])
    L = int(rng.integers(1, 4))
    layer = int(rng.integers(L))
    layout, ps = pick(("blmhd", "blhmd", "paged")), pick(PAGE_SIZES)
    rot = pick((0, D // 2, D))
    tables = bool(rot > 0 and rng.integers(2))
    m_max = KV8_TRIG_M_MAX if kv8 and rot > 0 and not tables else M_MAX
    M = ps * int(rng.integers(max(1, 64 // ps), m_max // ps + 1))
    need = -(-M // ps)
    stride = need + (int(rng.integers(1, 4)) if rng.integers(2) else 0)
    num_pages = B * stride + SPARE
    table = rng.permutation(num_pages)[:B * stride].astype(np.int32).reshape(B, stride)
    geo = dict(seed=int(seed), kv8=bool(kv8), dtype=("fp16", "bf16")[seed % 2], B=B, Hkv=Hkv, G=G, H=Hkv * G, D=D, L=L,
               layer=layer, layout=layout, ps=ps, M=M, stride=stride, num_pages=num_pages, rot=rot, tables=tables,
               bias=bool(rng.integers(2)))
    pos = [0 if rng.random() < 0.25 else int(rng.integers(0, M + 1)) for _ in range(B)]
    calls = []
    for step in range(STEPS):
        room = [M - p for p in pos]
        shape = pick(SHAPES) if min(room) > 0 else "_varlen"
        flavour = pick(FLAVOURS)
        if shape == "":
            n = [1] * B
        elif shape == "_chunk":
            top = min(N_MAX, min(room))
            n = [top if rng.random() < 0.2 else int(rng.integers(1, top + 1))] * B
        else:
            n = []
            for r in room:
                top, u = min(N_MAX, r), rng.random()
                n.append(0 if u < 0.15 else top if u < 0.35 else int(rng.integers(0, top + 1)))
        window = sinks = None
        if flavour:
            window = 1 if rng.random() < 0.15 else int(rng.integers(1, 2 * M + 1))
        if flavour == "_window_sinks":
            sinks = [float("-inf") if rng.random() < 0.1 else float(np.float32(2.0 * rng.standard_normal()))
                     for _ in range(Hkv * G)]
        calls.append(dict(seed=int(seed), kv8=bool(kv8), step=step, entry=entry_name(shape, flavour, kv8), shape=shape,
                          flavour=flavour, pos=list(pos), n=n, window=window, sinks=sinks,
                          num_splits=pick((0, 1, 2, 3)), softmax_scale=pick((None, None, 0.05, 0.2))))
        pos = [p + k for p, k in zip(pos, n)]
    return dict(geo=geo, table=table, calls=calls)


def check_preconditions(geo, call, table, k_scale=None, v_scale=None):
    """What include/star_flash_attn.h asks of the caller of any of the 18 decode entry points, for a call of a trace: a
    call that passes is neither rejected by the library nor able to raise a sticky status."""
    B, M, ps = geo["B"], geo["M"], geo["ps"]
    assert call["entry"] == entry_name(call["shape"], call["flavour"], geo["kv8"]) and call["entry"] in ENTRIES
    assert len(call["pos"]) == len(call["n"]) == B
    for pos, n in zip(call["pos"], call["n"]):
        assert 0 <= pos and 0 <= n and pos + n <= M, (pos, n, M)
    if call["shape"] == "":
        assert all(n == 1 for n in call["n"])
    if call["shape"] == "_chunk":
        assert call["n"][0] >= 1 and all(n == call["n"][0] for n in call["n"])
    assert geo["G"] in GROUPS and geo["H"] == geo["Hkv"] * geo["G"]
    assert geo["D"] in HEAD_DIMS
    assert geo["rot"] % 2 == 0 and 0 <= geo["rot"] <= geo["D"] and 0 <= geo["layer"] < geo["L"]
    assert ps >= 16 and ps & (ps - 1) == 0 and M % ps == 0 and geo["stride"] >= -(-M // ps)
    t = np.asarray(table)
    assert t.shape == (B, geo["stride"]) and t.min() >= 0 and t.max() < geo["num_pages"]
    assert np.unique(t).size == t.size                          # every sequence owns valid, distinct pages
    assert (call["window"] is None) == (call["flavour"] == "") and (call["window"] is None or call["window"] >= 1)
    assert (call["sinks"] is None) == (call["flavour"] != "_window_sinks")
    if call["sinks"] is not None:
        s = np.asarray(call["sinks"], np.float64)
        assert s.shape == (geo["H"],) and np.all(np.isfinite(s) | (s == -np.inf))
    for sc in (k_scale, v_scale):
        if sc is not None:
            sc = np.asarray(sc)
            assert sc.shape == (geo["Hkv"],) and np.all(np.isfinite(sc)) and np.all(sc > 0)
    assert call["softmax_scale"] is None or call["softmax_scale"] > 0
    assert call["num_splits"] >= 0


def trace_data(trace):
    """The arrays of a trace: kc, vc = the initial canonical cache as storage bits (N(0,1) everywhere, the rows past
    seq_len and the other layers included), biases (or None), cos / sin tables (or None), k_scale / v_scale (fp8)."""
    g = trace["geo"]
    rng = np.random.default_rng([8, int(g["kv8"]), g["seed"]])
    shape = (g["B"], g["L"], g["M"], g["Hkv"], g["D"])
    kf, vf = rng.standard_normal(shape, dtype=np.float32), rng.standard_normal(shape, dtype=np.float32)
    d = dict(q_bias=None, k_bias=None, v_bias=None, cos=None, sin=None, k_scale=None, v_scale=None)
    if g["kv8"]:        # amax / 448 per kv head times a factor in [0.5, 2]
        amax = lambda x: np.abs(x).max(axis=(0, 1, 2, 4)) / 448.0
        d["k_scale"] = (amax(kf) * rng.uniform(0.5, 2.0, g["Hkv"])).astype(np.float32)
        d["v_scale"] = (amax(vf) * rng.uniform(0.5, 2.0, g["Hkv"])).astype(np.float32)
        d["kc"], d["vc"] = kv8_ref.quantize(kf, d["k_scale"]), kv8_ref.quantize(vf, d["v_scale"])
    else:
        d["kc"], d["vc"] = to_bits16(round_to(kf, g["dtype"]), g["dtype"]), to_bits16(round_to(vf, g["dtype"]), g["dtype"])
    if g["bias"]:
        r = lambda h: round_to(0.5 * rng.standard_normal((h, g["D"])), g["dtype"])
        d["q_bias"], d["k_bias"], d["v_bias"] = r(g["H"]), r(g["Hkv"]), r(g["Hkv"])
    if g["tables"]:
        d["cos"], d["sin"] = rotary_table_ref(g["M"], g["rot"], g["dtype"])
    return d


def call_tokens(geo, call):
    """per sequence [n_b, H + 2 Hkv, D] float32 N(0,1) rounded to dtype"""
    rng = np.random.default_rng([9, int(geo["kv8"]), geo["seed"], call["step"]])
    return [round_to(rng.standard_normal((n, geo["H"] + 2 * geo["Hkv"], geo["D"])), geo["dtype"]) for n in call["n"]]


def model_call(geo, call, data, tokens=None):
    """the serving_model call of a call description"""
    return sm.make_call(geo["dtype"], geo["H"], call["pos"], call["n"], call_tokens(geo, call) if tokens is None else tokens,
                        geo["layer"], geo["rot"], q_bias=data["q_bias"], k_bias=data["k_bias"], v_bias=data["v_bias"],
                        cos=data["cos"], sin=data["sin"], window=call["window"], sinks=call["sinks"],
                        k_scale=data["k_scale"], v_scale=data["v_scale"], softmax_scale=call["softmax_scale"])


def rope_float32(x, pos, rot, cos=None, sin=None):
    """oracle.rope_interleaved in float32 arithmetic, as a kernel has it: the angle, its cosine and sine and the two
    products and their sum are all rounded to fp32"""
    x = np.asarray(x, np.float32)
    out = x.copy()
    if rot <= 0:
        return out
    if cos is None:
        ang = (np.float32(pos) * _inv_freq(rot)).astype(np.float32)
        cos, sin = np.cos(ang), np.sin(ang)
    cos, sin = np.asarray(cos, np.float32), np.asarray(sin, np.float32)
    xe, xo = x[..., 0:rot:2], x[..., 1:rot:2]
    out[..., 0:rot:2] = xe * cos - xo * sin
    out[..., 1:rot:2] = xo * cos + xe * sin
    return out


def kv8_k_bytes_float32(trace, data):
    """(identical, total, worst) over all K bytes an fp8 trace appends: the reference quantiser applied to the rotated k
    computed in float32 arithmetic against the model's bytes (fp64 rotation); worst = the largest difference in e4m3
    steps.  The 0.98 share of DESIGN.md 5.8 is a condition on the inputs: this is where it is checked."""
    g = trace["geo"]
    same = total = 0
    worst = 0.0
    H, Hkv = g["H"], g["Hkv"]
    for call in trace["calls"]:
        mc = model_call(g, call, data)
        for b, (pos, n) in enumerate(zip(call["pos"], call["n"])):
            if n == 0:
                continue
            want = sm.store(sm.prologue(mc, b)[1], g["dtype"], True, data["k_scale"])
            k = np.asarray(mc["tokens"][b], np.float32)[:, H:H + Hkv]
            if data["k_bias"] is not None:
                k = k + np.asarray(data["k_bias"], np.float32)
            kr = np.stack([rope_float32(k[t], pos + t, g["rot"], *((data["cos"][pos + t], data["sin"][pos + t])
                                                                   if data["cos"] is not None else ()))
                           for t in range(n)])
            got = kv8_ref.quantize(round_to(kr, g["dtype"]), data["k_scale"])
            same += int(np.sum(got == want))
            total += want.size
            a, w = kv8_ref.E4M3[got], kv8_ref.E4M3[want]
            worst = max(worst, float(np.max(np.abs(a - w) / kv8_ref.step_at(np.maximum(np.abs(a), np.abs(w))))))
    return same, total, worst


# ---- the five newer prefill forwards -----------------------------------------------------------------------------------

PREFILL_KINDS = ("window", "split", "varlen", "varlen_window", "varlen_split")
PREFILL_SEEDS = tuple(range(24))
PREFILL_GROUPS = (1, 2, 3, 4, 6, 8)
PREFILL_SPLITS = (0, 1, 2, 3, 5, 9)


def _sinks(rng, Hq):
    if rng.random() < 0.3:
        return None
    return [float("-inf") if rng.random() < 0.1 else float(np.float32(2.0 * rng.standard_normal())) for _ in range(Hq)]


def prefill_case(kind, seed):
    """The parameters of one fuzz case (Python scalars and lists only).  Rectangular kinds: B, Sq, Sk.  Packed kinds: cu_q,
    cu_k (as the call gets them), total_q, total_k (the totals the call gets; the allocations have alloc_k >= total_k key
    rows), invalid = None / "backwards" / "past_total_k", max_seqlen_k and low_hint for varlen_split."""
    rng = np.random.default_rng([10, PREFILL_KINDS.index(kind), seed])
    pick = lambda xs: xs[int(rng.integers(len(xs)))]
    Hkv, G = int(rng.integers(1, 6)), pick(PREFILL_GROUPS)
    c = dict(kind=kind, seed=int(seed), dtype=("bf16", "fp16")[seed % 2], D=pick((64, 128)), Hkv=Hkv, G=G, Hq=Hkv * G,
             softmax_scale=pick((None, 0.05, 0.2)), packed=bool(rng.integers(2)), causal=True, window=None, sinks=None,
             num_splits=None)
    if kind in ("window", "split"):
        Sk = int(rng.integers(1, 701))
        Sq = int(rng.integers(Sk + 1, 701)) if Sk < 700 and rng.random() < 1 / 3 else int(rng.integers(1, Sk + 1))
        c.update(B=int(rng.integers(1, 4)), Sq=Sq, Sk=Sk)
        longest = Sk
    else:
        B = int(rng.integers(1, 7))
        lens = []
        for _ in range(B):
            u = rng.random()
            n_k = 0 if u < 0.1 else int(rng.integers(1, 401))
            u = rng.random()
            n_q = 0 if u < 0.15 else int(rng.integers(n_k + 1, 401)) if u < 0.4 and n_k < 400 else int(rng.integers(1, max(n_k, 1) + 1))
            lens.append((n_q, n_k))
        if not any(a for a, _ in lens):                         # (a call needs storage: at least one query row and one key row)
            lens[0] = (1, lens[0][1])
        if not any(b for _, b in lens):
            lens[0] = (lens[0][0], 1)
        cu_q = [0] + [int(x) for x in np.cumsum([a for a, _ in lens])]
        cu_k = [0] + [int(x) for x in np.cumsum([b for _, b in lens])]
        total_k = alloc_k = cu_k[-1]
        invalid = None
        if rng.random() < 0.25:
            backwards = [j for j in range(2, B + 1) if cu_k[j - 1] >= 1]     # sequence j - 1 can be made to run backwards
            if rng.integers(2) and backwards:
                j = pick(backwards)
                cu_k[j] = cu_k[j - 1] - int(rng.integers(1, cu_k[j - 1] + 1))
                invalid = "backwards"
            elif lens[-1][1] >= 1:
                total_k = alloc_k - int(rng.integers(1, lens[-1][1] + 1))    # the last sequence ends past total_k
                invalid = "past_total_k"
        n_k_valid = [cu_k[b + 1] - cu_k[b] for b in range(B)
                     if 0 <= cu_k[b] <= cu_k[b + 1] <= total_k]
        longest = max(n_k_valid + [1])
        c.update(B=B, lens=lens, cu_q=cu_q, cu_k=cu_k, total_q=cu_q[-1], total_k=total_k, alloc_k=alloc_k, invalid=invalid)
    if kind in ("split", "varlen", "varlen_split"):
        c["causal"] = bool(rng.integers(2))
    if kind in ("window", "varlen_window"):
        c.update(window=int(rng.integers(1, 2 * longest + 1)), sinks=_sinks(rng, c["Hq"]))
    if kind in ("split", "varlen_split"):
        c["num_splits"] = pick(PREFILL_SPLITS)
    if kind == "varlen_split":
        low = bool(rng.integers(2)) and longest > 1
        c.update(low_hint=low, max_seqlen_k=int(rng.integers(1, longest)) if low else longest)
    return c


def prefill_inputs(c):
    """(q, k, v) float32 N(0,1) rounded to dtype: [B, Hq, Sq, D] / [B, Hkv, Sk, D], or packed [total_q, Hq, D] /
    [alloc_k, Hkv, D]"""
    rng = np.random.default_rng([11, PREFILL_KINDS.index(c["kind"]), c["seed"]])
    r = lambda *shape: round_to(rng.standard_normal(shape), c["dtype"])
    if "Sq" in c:
        return r(c["B"], c["Hq"], c["Sq"], c["D"]), r(c["B"], c["Hkv"], c["Sk"], c["D"]), r(c["B"], c["Hkv"], c["Sk"], c["D"])
    return r(c["total_q"], c["Hq"], c["D"]), r(c["alloc_k"], c["Hkv"], c["D"]), r(c["alloc_k"], c["Hkv"], c["D"])
