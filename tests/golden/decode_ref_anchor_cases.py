"""The cases of decode_ref_anchors.npz: what every reference function of the tests/*_ref.py files returned while it still
held arithmetic of its own (make_decode_ref_anchors.py records them from a checkout of that commit), for section 1 of
tests/test_serving_model_cpu.py, which evaluates the same cases on the adapters over tests/serving_model.py.  The module
is loaded by path, with tests/ of the tree under test on sys.path.

CASES maps a name to a function without arguments that returns {field: array}.  Inputs are not stored: the seeded problem
builders regenerate them.  Lists per sequence are stored concatenated along the token axis; a cache a function mutates is
stored as the sha256 of its bytes after the call.  Over the cases: both dtypes, head_dim 64 / 128 (256 in the 16-bit
single-token ones), group 1 and larger, window None / binding / not binding / 1, sinks with one -inf, rotary tables on and
off, biases on and off, ragged counts with an empty sequence, k / v scale factors other than 1 and a softmax_scale other
than 1 / sqrt(head_dim)."""
import hashlib

import numpy as np

import chunk_kv8_ref as ckr
import chunk_kv8_window_ref as ckw
import chunk_window_ref as cw
import kv8_ref
import kv8_sinks_ref as k8s
import kv8_window_ref as kwr
import sinks_ref
from oracle import round_to
from window_ref import decode_window_ref

CASES = {}


def case(name):
    def add(fn):
        CASES[name] = fn
        return fn
    return add


def sha(c):
    return np.array(hashlib.sha256(np.ascontiguousarray(c).tobytes()).hexdigest())


def cat(per_sequence):
    return np.concatenate(per_sequence)


def some_sinks(H, lo=-2.0, hi=3.0, dtype=np.float64):
    """a sink per head, one of them -inf"""
    s = np.linspace(lo, hi, H).astype(dtype)
    s[1 % H] = -np.inf
    return s


# ---- the 16-bit single-token references: the first token of a chunk_window_ref problem ---------------------------------------

def single16(fn, dtype, D, G, *window_and_sinks, bias=True, tables=False, scale=None, fields=("o", "k_row", "v_row")):
    prob = cw.make_problem(dtype, D, G, cw.LENS, (1,) * 4, bias=bias, tables=tables, seed=4)
    f = lambda x: None if x is None else x.float().numpy()
    x, H = f(prob.qkv[:, 0]), prob.H
    cos, sin = cw.rotary_tables(dtype, prob.rot) if tables else (None, None)
    ref = fn(x[:, :H], x[:, H:H + cw.HKV], x[:, H + cw.HKV:], prob.kf, prob.vf, prob.lens, cw.LAYER, prob.rot,
             *window_and_sinks, dtype, q_bias=f(prob.qb), k_bias=f(prob.kb), v_bias=f(prob.vb), cos_table=cos, sin_table=sin,
             scale=scale)
    return {k: ref[k] for k in fields}


for _name, _args, _kw in (("fp16-D64-G1-w100", ("fp16", 64, 1, 100), {}),
                          ("bf16-D64-G4-w1", ("bf16", 64, 4, 1), {}),
                          ("fp16-D64-G8-w5000", ("fp16", 64, 8, 5000), dict(bias=False)),
                          ("bf16-D256-G1-wNone-tables-scale", ("bf16", 256, 1, None), dict(tables=True, scale=0.05))):
    case("decode_window_ref/" + _name)(lambda a=_args, k=_kw: single16(decode_window_ref, *a, **k))

_SINK_FIELDS = ("o", "k_row", "v_row", "lse", "o64")
for _name, _args, _kw in (("fp16-D256-G1-w17-tables", ("fp16", 256, 1, 17), dict(tables=True, bias=False)),
                          ("bf16-D64-G4-wNone-scale", ("bf16", 64, 4, None), dict(scale=0.2)),
                          ("fp16-D64-G2-w5000-nosinks", ("fp16", 64, 2, 5000), dict(sinks=False))):
    def _sinks16(a=_args, k=_kw):
        k = dict(k)
        sinks = some_sinks(cw.HKV * a[2]) if k.pop("sinks", True) else None
        return single16(sinks_ref.decode_window_sinks_ref, *a, sinks, fields=_SINK_FIELDS, **k)
    case("decode_window_sinks_ref/" + _name)(_sinks16)


# ---- the 16-bit multi-token references -----------------------------------------------------------------------------------------

def chunk16(fn, dtype, D, G, ns, window, *sinks, bias=True, tables=False, seed=3, **kw):
    prob = cw.make_problem(dtype, D, G, cw.LENS, ns, bias=bias, tables=tables, seed=seed)
    ref = fn(prob, window, *sinks, **kw)
    return {f: cat([r[i] for r in ref]) for i, f in enumerate(("o", "k_rows", "v_rows", "lse", "o64")[:len(ref[0])])}


for _name, _args, _kw in (("bf16-D64-G2-w3", ("bf16", 64, 2, (2,) * 4, 3), {}),
                          ("fp16-D128-G1-w130-tables-ragged", ("fp16", 128, 1, (3, 0, 1, 4), 130), dict(tables=True)),
                          ("fp16-D64-G8-w5000", ("fp16", 64, 8, (1,) * 4, 5000), dict(bias=False)),
                          ("bf16-D64-G4-wNone", ("bf16", 64, 4, (2, 3, 0, 4), None), {}),
                          ("fp16-D64-G1-w1", ("fp16", 64, 1, (3,) * 4, 1), {})):
    case("chunk_window_ref/" + _name)(lambda a=_args, k=_kw: chunk16(cw.chunk_window_ref, *a, **k))

for _name, _args, _kw in (("bf16-D64-G2-w3", ("bf16", 64, 2, (3,) * 4, 3), {}),
                          ("fp16-D128-G1-w130-tables", ("fp16", 128, 1, (2,) * 4, 130), dict(tables=True)),
                          ("fp16-D64-G2-w5000", ("fp16", 64, 2, (2,) * 4, 5000), {})):
    case("chunk_window_ref_literal/" + _name)(lambda a=_args, k=_kw: chunk16(cw.chunk_window_ref_literal, *a, **k))

for _name, _args, _kw in (("fp16-D64-G2-w4", ("fp16", 64, 2, (2, 0, 1, 2), 4), {}),
                          ("bf16-D128-G1-w200-tables", ("bf16", 128, 1, (2, 0, 1, 2), 200), dict(tables=True)),
                          ("bf16-D64-G1-wNone-scale", ("bf16", 64, 1, (2, 2, 2, 2), None), dict(scale=0.3, bias=False))):
    case("chunk_sinks_ref/" + _name)(lambda a=_args, k=_kw: chunk16(sinks_ref.chunk_sinks_ref, *a, some_sinks(cw.HKV * a[2]), **k))


# ---- the fp8 single-token references, at the frame of kv8_window_ref ------------------------------------------------------------

def single8(fn, dtype, D, G, *window_and_sinks, tables=False, bias=True, scale=None, k_factors=(1.0, 1.0), fields=("o", "k_row", "v_row")):
    t, c = kwr.tokens(dtype, D, G), kwr.caches(D, k_factors)
    cos, sin = kwr.rotary_tables(dtype, t.rot) if tables else (None, None)
    qb, kb, vb = (t.qb, t.kb, t.vb) if bias else (None, None, None)
    k8, v8 = c.k8.copy(), c.v8.copy()
    ref = fn(t.qkv, k8, v8, kwr.LENS, kwr.LAYER, t.rot, dtype, *window_and_sinks, c.ks, c.vs, q_bias=qb, k_bias=kb, v_bias=vb,
             cos_table=cos, sin_table=sin, scale=scale)
    return dict({k: ref[k] for k in fields}, k8=sha(k8), v8=sha(v8))


for _name, _args, _kw in (("fp16-D64-G1", ("fp16", 64, 1), {}),
                          ("bf16-D128-G4-tables-factors-scale", ("bf16", 128, 4), dict(tables=True, k_factors=(0.5, 2.0), scale=0.07)),
                          ("fp16-D128-G2-nobias", ("fp16", 128, 2), dict(bias=False))):
    case("decode_kv8_ref/" + _name)(lambda a=_args, k=_kw: single8(kv8_ref.decode_kv8_ref, *a, **k))


@case("decode_kv8_ref/fp16-D64-G2-noscales-rot0")
def _():
    """no scale tensors (None = 1.0), no rotation, the last row of the cache"""
    pr = ckr.make_problem(7, [1, 1, 1], 2, 2, 64, "fp16", with_scales=False)
    k8, v8 = pr["k8"].copy(), pr["v8"].copy()
    ref = kv8_ref.decode_kv8_ref(np.concatenate(pr["tok"]), k8, v8, [0, 100, ckr.M - 1], ckr.LAYER, 0, "fp16")
    return dict(ref, k8=sha(k8), v8=sha(v8))


for _name, _args, _kw in (("fp16-D64-G2-w17", ("fp16", 64, 2, 17), {}),
                          ("bf16-D128-G4-wNone-tables-factors", ("bf16", 128, 4, None), dict(tables=True, k_factors=(2.0, 0.5))),
                          ("bf16-D64-G1-w1-scale", ("bf16", 64, 1, 1), dict(scale=0.3)),
                          ("fp16-D128-G1-w5000-nobias", ("fp16", 128, 1, 5000), dict(bias=False))):
    case("decode_kv8_window_ref/" + _name)(lambda a=_args, k=_kw: single8(kwr.decode_kv8_window_ref, *a, **k))

_SINK8_FIELDS = ("o", "k_row", "v_row", "o64", "lse", "q16")
for _name, _args, _kw in (("bf16-D64-G2-w4-factors", ("bf16", 64, 2, 4), dict(k_factors=(0.5, 2.0))),
                          ("fp16-D128-G1-wNone-tables-scale", ("fp16", 128, 1, None), dict(tables=True, scale=0.1)),
                          ("fp16-D64-G2-w1000-nosinks", ("fp16", 64, 2, 1000), dict(sinks=False))):
    def _sinks8(a=_args, k=_kw):
        k = dict(k)
        sinks = some_sinks(kwr.HKV * a[2], 3.0, -2.0, np.float32) if k.pop("sinks", True) else None
        return single8(k8s.decode_kv8_sinks_ref, *a, sinks, fields=_SINK8_FIELDS, **k)
    case("decode_kv8_sinks_ref/" + _name)(_sinks8)


# ---- the fp8 multi-token references ----------------------------------------------------------------------------------------------

def chunk8(pr, lens, **kw):
    """chunk_kv8_ref at its own frame (L, M, LAYER = 2, 256, 1), through chunk_kv8_ref.reference"""
    ref, k_ref, v_ref = ckr.reference(pr, lens, **kw)
    return dict(o=cat(ref["o"]), q16=cat(ref["q16"]), k8=sha(k_ref), v8=sha(v_ref))


@case("chunk_kv8_ref/fp16-D64-G4-ragged-factors")
def _():
    return chunk8(ckr.make_problem(5, [1, 0, 2], 2, 4, 64, "fp16", scale_factors=(0.5, 2.0)), [0, 100, 253], rot=64)


@case("chunk_kv8_ref/bf16-D128-G1-bias-tables-scale")
def _():
    pr = ckr.make_problem(5, [2, 0, 2], 2, 1, 128, "bf16", scale_factors=(2.0, 0.5))
    rng = np.random.default_rng(6)
    biases = tuple(round_to(rng.standard_normal((h, 128)), "bf16") for h in (pr["H"], 2, 2))
    return chunk8(pr, [0, 100, 248], rot=64, biases=biases, tables=ckw.rotary_tables("bf16", 64), softmax_scale=0.06)


@case("chunk_kv8_ref/fp16-D64-G2-noscales")
def _():
    return chunk8(ckr.make_problem(8, [4, 1], 2, 2, 64, "fp16", with_scales=False), [17, 0])


def chunk8w(dtype, D, G, ns, window, sinks=False, **kw):
    """chunk_kv8_window_ref (sinks: kv8_sinks_ref.chunk_kv8_sinks_ref) through its reference(), then the three attend
    functions over the caches after the append"""
    p = ckw.make_problem(dtype, D, G, ckw.LENS, ns, **kw)
    s = some_sinks(p.H, 3.0, -2.0, np.float32) if sinks else None
    ref, k_ref, v_ref = k8s.chunk_kv8_sinks_ref(p, window, s) if sinks else ckw.reference(p, window)
    out = dict(o=cat(ref["o"]), q16=cat(ref["q16"]), k8=sha(k_ref), v8=sha(v_ref))
    b = p.ns.index(min(n for n in p.ns if n))       # the shortest sequence that has tokens
    rows = ref["q16"][b], k_ref[b, ckw.LAYER], v_ref[b, ckw.LAYER], p.lens[b]
    if sinks:
        out["lse"] = cat(ref["lse"])
        out["attend_sinks_o"], out["attend_sinks_lse"] = k8s.attend_sinks(*rows, window, s, p.ks, p.vs, p.scale)
    else:
        out["attend_window"] = ckw.attend(*rows, window, p.ks, p.vs, p.scale)
        out["attend_full"] = ckr.attend(*rows, p.ks, p.vs, p.scale)
    return out


for _name, _args, _kw in (("fp16-D64-G2-w3-ragged", ("fp16", 64, 2, (2, 0, 3, 1), 3), dict(seed=1, k_factors=(0.5, 2.0))),
                          ("bf16-D128-G2-w140", ("bf16", 128, 2, (1, 0, 2, 1), 140), dict(seed=1, k_factors=(0.5, 2.0))),
                          ("bf16-D64-G1-wNone-tables-scale-nobias", ("bf16", 64, 1, (2,) * 4, None),
                           dict(tables=True, scale=0.2, bias=False)),
                          ("fp16-D64-G1-w1-noscales", ("fp16", 64, 1, (2, 1, 0, 3), 1), dict(with_scales=False))):
    case("chunk_kv8_window_ref/" + _name)(lambda a=_args, k=_kw: chunk8w(*a, **k))

for _name, _args, _kw in (("bf16-D64-G2-w4", ("bf16", 64, 2, (2, 1, 0, 2), 4), dict(seed=2, k_factors=(2.0, 0.5), tables=True)),
                          ("fp16-D128-G1-w1000", ("fp16", 128, 1, (2, 1, 0, 1), 1000), dict(seed=2, k_factors=(2.0, 0.5), tables=True))):
    case("chunk_kv8_sinks_ref/" + _name)(lambda a=_args, k=_kw: chunk8w(*a, sinks=True, **k))
