"""CPU reference of the multi-token decode step over an fp8 (e4m3) KV cache (sfa_decode_chunk_kv8, sfa_decode_varlen_kv8)
and the helpers the two GPU test files share.  The arithmetic is that of tests/serving_model.py; the functions here are
adapters over it.

The contract is "what n successive sfa_decode_kv8 calls give".  chunk_kv8_ref states it the way the header does -- append
the quantised rows of all new tokens, then let token t attend to the rows [0, pos + t] of the cache AFTER the append --
and tests/test_decode_chunk_kv8_cpu.py holds it against kv8_ref.decode_kv8_ref applied token by token.

attend() is the second half alone: fp64 attention of given rotated queries over a GIVEN byte cache.  The GPU tests use it
over the bytes the device stored, because on-device sincosf can move a K byte across an e4m3 rounding boundary
 and one e4m3 step on a heavy key is outside the 16-bit tolerance: the bytes are checked against the
reference quantiser, the output against the cache after the call."""
import numpy as np

import kv8_ref
import serving_model as sm
from oracle import round_to
from window_ref import TOL  # noqa: F401  (the project's decode tolerances, atol = rtol)

L, M, LAYER = 2, 256, 1


def attend_bytes(q16, k8, v8, pos, window, sinks, k_scale, v_scale, scale):
    """The model's attention over a given byte cache, for attend(), chunk_kv8_window_ref.attend and
    kv8_sinks_ref.attend_sinks: q16 [n, H, D] float64 rotated, rounded queries of the tokens at pos .. pos + n - 1 of one
    sequence; k8 / v8 [M, Hkv, D] uint8, one (sequence, layer) of the cache after the append.  Returns (o [n, H, D], lse
    [n, H] without the sink), float64."""
    call = sm.make_call(None, q16.shape[1], [pos], [len(q16)], None, 0, window=window, sinks=sinks, k_scale=k_scale,
                        v_scale=v_scale, softmax_scale=scale)
    return sm.attend_rows(q16, k8, v8, int(pos), call, with_lse=True)


def attend(q16, k8, v8, pos, k_scale=None, v_scale=None, scale=None):
    """attend_bytes without a window or sinks: token t attends to the rows [0, pos + t].  Returns o [n, H, D] float64."""
    return attend_bytes(q16, k8, v8, pos, None, None, k_scale, v_scale, scale)[0]


def chunk_kv8_model(tokens, k8, v8, seq_len, idx_layer, rot_dim, dtype, window, sinks, k_scale, v_scale, q_bias, k_bias, v_bias,
                    cos_table, sin_table, scale):
    """The multi-token call over an fp8 cache through the model, for chunk_kv8_ref and chunk_kv8_window_ref.
    chunk_kv8_window_ref (window, sinks: None here).  k8 / v8 are MUTATED.  Returns dict(o, q16, lse = per sequence float64)."""
    tokens = [np.asarray(t) for t in tokens]
    Mx = k8.shape[2]
    pos = [int(p) if len(t) else 0 for p, t in zip(seq_len, tokens)]        # (a sequence without tokens may say anything)
    for b, (p, t) in enumerate(zip(pos, tokens)):
        if not (0 <= p and p + len(t) <= Mx):
            raise ValueError(f"sequence {b}: rows [{p}, {p + len(t)}) outside [0, memory_max_len={Mx})")
    call = sm.make_call(dtype, tokens[0].shape[1] - 2 * k8.shape[3], pos, [len(t) for t in tokens], tokens, idx_layer, rot_dim,
                        q_bias=q_bias, k_bias=k_bias, v_bias=v_bias, cos=cos_table, sin=sin_table, window=window, sinks=sinks,
                        k_scale=k_scale, v_scale=v_scale, softmax_scale=scale)
    app, res = sm.run((k8, v8), call, in_place=True)
    return dict(o=[r[0] for r in res], q16=app["q16"], lse=[r[1] for r in res])


def chunk_kv8_ref(tokens, k8, v8, seq_len, idx_layer, rot_dim, dtype, k_scale=None, v_scale=None, q_bias=None,
                  k_bias=None, v_bias=None, cos_table=None, sin_table=None, scale=None):
    """tokens: one [n_b, H + 2*Hkv, D] float array per sequence (n_b may be 0; values representable in `dtype`).
    k8, v8 [B, L, M, Hkv, D] uint8, MUTATED at [b, idx_layer, seq_len[b] .. seq_len[b] + n_b).
    Returns dict(o = per sequence [n_b, H, D] float64, q16 = per sequence [n_b, H, D] float64)."""
    ref = chunk_kv8_model(tokens, k8, v8, seq_len, idx_layer, rot_dim, dtype, None, None, k_scale, v_scale, q_bias, k_bias, v_bias,
                          cos_table, sin_table, scale)
    return dict(o=ref["o"], q16=ref["q16"])


# ---- what the GPU tests share ------------------------------------------------------------------------------------------

def amax_scale(x):
    """amax / 448 per kv head of x [B, L, M, Hkv, D]"""
    return (np.abs(x).max(axis=(0, 1, 2, 4)) / 448.0).astype(np.float32)


def make_problem(seed, counts, Hkv, G, D, dtype, scale_factors=None, with_scales=True):
    """N(0,1) caches quantised with scale = factor * amax / 448 per kv head, and counts[b] N(0,1) tokens per sequence
    rounded to dtype."""
    rng = np.random.default_rng(seed)
    B, H = len(counts), Hkv * G
    kc = rng.standard_normal((B, L, M, Hkv, D)).astype(np.float32)
    vc = rng.standard_normal((B, L, M, Hkv, D)).astype(np.float32)
    ks = vs = None
    if with_scales:
        f = np.ones(Hkv, np.float32) if scale_factors is None else np.asarray(scale_factors, np.float32)
        ks, vs = amax_scale(kc) * f, amax_scale(vc) * f[::-1]
    tok = [round_to(rng.standard_normal((n, H + 2 * Hkv, D)), dtype) for n in counts]
    return dict(tok=tok, k8=kv8_ref.quantize(kc, ks), v8=kv8_ref.quantize(vc, vs), ks=ks, vs=vs, B=B, H=H, Hkv=Hkv,
                D=D, dtype=dtype, counts=list(counts))


def page_table(B, ps, seed=3):
    """a shuffled block table over a pool with a few pages to spare"""
    import torch
    pps = M // ps
    num_pages = B * pps + 3
    g = torch.Generator().manual_seed(seed)
    return torch.randperm(num_pages, generator=g)[:B * pps].to(torch.int32).view(B, pps), num_pages


def to_layout(c, layout, table=None, num_pages=0, ps=16, fill=0x33):
    """canonical uint8 [B, L, M, Hkv, D] (numpy) -> the device tensor of `layout`"""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(c))
    if layout == "blhmd":
        t = t.permute(0, 1, 3, 2, 4).contiguous()
    elif layout == "paged":
        B, _, _, Hkv, D = c.shape
        pool = torch.full((num_pages, L, ps, Hkv, D), fill, dtype=torch.uint8)
        pool[table.long().view(-1)] = t.view(B, L, M // ps, ps, Hkv, D).permute(0, 2, 1, 3, 4, 5).reshape(-1, L, ps, Hkv, D)
        t = pool
    return t.cuda()


def from_layout(t, layout, B, table=None, ps=16):
    t = t.cpu()
    if layout == "blhmd":
        t = t.permute(0, 1, 3, 2, 4)
    elif layout == "paged":
        Hkv, D = t.shape[3], t.shape[4]
        t = t[table.long().view(-1)].view(B, M // ps, L, ps, Hkv, D).permute(0, 2, 1, 3, 4, 5).reshape(B, L, M, Hkv, D)
    return t.contiguous().numpy()


def split_layout(layout):
    """"paged16" / "paged64" -> ("paged", page size)"""
    return ("paged", int(layout[5:])) if layout.startswith("paged") and len(layout) > 5 else (layout, 16)


def run(sfa, pr, lens, k8, v8, layout="blmhd", *, varlen=False, num_splits=0, rot=None, biases=None, tables=None,
        table=None, num_pages=0, ps=16, call_table=None, softmax_scale=None, cu=None, as_fp8=False, fill=0x33):
    """One flash_decode_chunk_kv8 (every sequence has pr["counts"][0] tokens) or flash_decode_varlen_kv8 call on canonical
    numpy caches.  Returns (o per sequence fp32 [n_b, H, D], k8 after, v8 after, raw device caches).  Paged: `table` lays
    the pools out and reads them back; the call gets call_table when given (a damaged copy).  cu: the cu_tokens the
    varlen call gets instead of the true ones (the rows of o are cut by the true ones)."""
    import torch
    dev = torch.device("cuda:0")
    dt = {"fp16": torch.float16, "bf16": torch.bfloat16}[pr["dtype"]]
    B, H, Hkv, D, counts = pr["B"], pr["H"], pr["Hkv"], pr["D"], pr["counts"]
    t16 = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dt).to(dev)
    kd, vd = to_layout(k8, layout, table, num_pages, ps, fill), to_layout(v8, layout, table, num_pages, ps, fill)
    if as_fp8:
        kd, vd = kd.view(torch.float8_e4m3fn), vd.view(torch.float8_e4m3fn)
    kw = dict(num_splits=num_splits, kv_layout=layout, num_heads_kv=Hkv, softmax_scale=softmax_scale)
    if layout == "paged":
        kw["block_table"] = (table if call_table is None else call_table).to(dev)
    if tables is not None:
        kw.update(rotary_cos_table=t16(tables[0]), rotary_sin_table=t16(tables[1]))
    if pr["ks"] is not None:
        kw.update(k_scale=torch.from_numpy(pr["ks"]).to(dev), v_scale=torch.from_numpy(pr["vs"]).to(dev))
    bq, bk, bv = (None, None, None) if biases is None else (t16(x) for x in biases)
    seq = torch.tensor(list(lens), dtype=torch.int32, device=dev)
    heads = (3, H, D) if Hkv == H else (H + 2 * Hkv, D)
    rd = D if rot is None else rot
    if varlen:
        T = sum(counts)
        true_cu = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
        qkv = t16(np.concatenate([np.asarray(x).reshape(-1, H + 2 * Hkv, D) for x in pr["tok"]])).view((T,) + heads)
        o = torch.full((T, H, D), 7.0, dtype=dt, device=dev)
        cu_d = torch.from_numpy(true_cu if cu is None else np.asarray(cu, np.int32)).to(dev)
        ret = sfa.flash_decode_varlen_kv8(qkv, bq, bk, bv, kd, vd, seq, o, cu_d, B, M, H, D, rd, M, L, LAYER, **kw)
        torch.cuda.synchronize()
        of = o.float().cpu().numpy()
        o_list = [of[true_cu[b]:true_cu[b + 1]] for b in range(B)]
    else:
        n = counts[0]
        assert all(c == n for c in counts)
        qkv = t16(np.stack(pr["tok"])).view((B, n) + heads)
        o = torch.full((B, n, H, D), 7.0, dtype=dt, device=dev)
        ret = sfa.flash_decode_chunk_kv8(qkv, bq, bk, bv, kd, vd, seq, o, B, M, H, D, rd, M, L, LAYER, **kw)
        torch.cuda.synchronize()
        o_list = list(o.float().cpu().numpy())
    assert ret.data_ptr() == o.data_ptr()
    kd, vd = kd.view(torch.uint8), vd.view(torch.uint8)
    return o_list, from_layout(kd, layout, B, table, ps), from_layout(vd, layout, B, table, ps), (kd, vd)


def check_bytes(lens, counts, k_out, v_out, k_before, v_before, k_ref, v_ref):
    """(a) The appended rows against the reference quantiser with DESIGN.md 5.8's criterion -- V exact; K within one e4m3
    step, more than 98 % of the call's K bytes identical -- and every other byte of both caches against the bytes before."""
    mask = np.ones(k_before.shape[:3], bool)
    same = total = 0
    for b, (pos, n) in enumerate(zip(lens, counts)):
        if n == 0:
            continue
        rows = slice(pos, pos + n)
        mask[b, LAYER, rows] = False
        np.testing.assert_array_equal(v_out[b, LAYER, rows], v_ref[b, LAYER, rows])             # exact
        got, want = kv8_ref.E4M3[k_out[b, LAYER, rows]], kv8_ref.E4M3[k_ref[b, LAYER, rows]]
        assert np.all(np.abs(got - want) <= kv8_ref.step_at(np.maximum(np.abs(got), np.abs(want)))), b
        same += int(np.sum(k_out[b, LAYER, rows] == k_ref[b, LAYER, rows]))
        total += k_out[b, LAYER, rows].size
    if total:
        print("K bytes identical to the reference quantiser: %.4f" % (same / total))
        assert same / total > 0.98
    np.testing.assert_array_equal(k_out[mask], k_before[mask])
    np.testing.assert_array_equal(v_out[mask], v_before[mask])


def check_o(pr, lens, o_list, k_out, v_out, ref, softmax_scale=None):
    """(b) o against attend() over the bytes the device stored, with q16 from the reference, at the decode tolerances."""
    tol = TOL[pr["dtype"]]
    for b, n in enumerate(pr["counts"]):
        if n == 0:
            continue
        want = attend(ref["q16"][b], k_out[b, LAYER], v_out[b, LAYER], lens[b], pr["ks"], pr["vs"], softmax_scale)
        assert np.isfinite(o_list[b]).all(), b
        err = np.abs(o_list[b] - want)
        print("sequence %d: max |o - ref| = %.3e (tol %.1e)" % (b, err.max(), tol))
        np.testing.assert_allclose(o_list[b], want, atol=tol, rtol=tol)


def reference(pr, lens, rot=None, biases=None, tables=None, softmax_scale=None):
    """The reference run on copies of the problem's caches: (ref, k8 after, v8 after)"""
    k_ref, v_ref = pr["k8"].copy(), pr["v8"].copy()
    okw = {}
    if biases is not None:
        okw = dict(q_bias=biases[0], k_bias=biases[1], v_bias=biases[2])
    if tables is not None:
        okw.update(cos_table=tables[0], sin_table=tables[1])
    ref = chunk_kv8_ref(pr["tok"], k_ref, v_ref, lens, LAYER, pr["D"] if rot is None else rot, pr["dtype"], pr["ks"],
                        pr["vs"], scale=softmax_scale, **okw)
    return ref, k_ref, v_ref


def check(sfa, pr, lens, layout="blmhd", ps=16, **kw):
    """(a) and (b) for one call, the other layer and, paged, the pages no sequence owns included"""
    import torch
    table = num_pages = None
    if layout == "paged":
        table, num_pages = page_table(pr["B"], ps)
    rkw = {k: kw[k] for k in ("rot", "biases", "tables", "softmax_scale") if k in kw}
    ref, k_ref, v_ref = reference(pr, lens, **rkw)
    o, k_out, v_out, raw = run(sfa, pr, lens, pr["k8"], pr["v8"], layout, table=table, num_pages=num_pages, ps=ps, **kw)
    sfa.check_decode_status()
    check_bytes(lens, pr["counts"], k_out, v_out, pr["k8"], pr["v8"], k_ref, v_ref)
    check_o(pr, lens, o, k_out, v_out, ref, kw.get("softmax_scale"))
    if layout == "paged":           # the spare pages of the pool
        spare = torch.from_numpy(np.setdiff1d(np.arange(num_pages), table.numpy().ravel())).to(raw[0].device)
        fill = kw.get("fill", 0x33)
        assert bool((raw[0][spare] == fill).all()) and bool((raw[1][spare] == fill).all())
    return o, k_out, v_out, ref


def poison(pr, lens):
    """0x7F (an e4m3 NaN) in every row at and beyond pos + n of LAYER and in every other layer"""
    for c in (pr["k8"], pr["v8"]):
        for l in range(L):
            if l != LAYER:
                c[:, l] = 0x7F
        for b, (pos, n) in enumerate(zip(lens, pr["counts"])):
            c[b, LAYER, pos + n:] = 0x7F


def poisoned_table(table, lens, counts, ps):
    """-1 in every block_table entry past the last page a sequence needs"""
    bad = table.clone()
    for b, (pos, n) in enumerate(zip(lens, counts)):
        bad[b, (pos + n - 1) // ps + 1:] = -1
    return bad
