"""The cases of tests/test_decode_validation_matrix_cpu.py: every decode entry point of the C ABI (three call shapes x six
flavours) called with fake device pointers, one well-formed call plus single and paired mutations of it, none of which gets
as far as a HIP call.  tests/golden/make_golden.py runs the same cases against a library built at the commit whose behaviour
is to be kept and records (status, sfa_last_error()) of each; the test replays them against the library under test.

The binding is this module's own (explicit ctypes values, no argtypes), so it does not lean on starflashattention_amd/_lib.py.
"""
import ctypes
import itertools

SHAPES = ("", "_chunk", "_varlen")                     # one token, n tokens per sequence, packed ragged tokens
FLAVOURS = ("", "_window", "_window_sinks", "_kv8", "_kv8_window", "_kv8_window_sinks")


class Entry:
    def __init__(self, shape, flavour):
        self.name = "sfa_decode" + shape + flavour
        self.shape = shape
        self.single, self.varlen = shape == "", shape == "_varlen"
        self.window, self.kv8, self.sinks = "_window" in flavour, "_kv8" in flavour, "_sinks" in flavour
        # the workspace-sizing export that serves the entry point
        self.sizing = "sfa_decode" + shape + ("_window" if self.window else "") + "_workspace_bytes"
        # the call trims an automatic split count to the workspace it was given ("Decode host pipeline")
        self.trims = self.single or self.window


ENTRIES = [Entry(s, f) for s in SHAPES for f in FLAVOURS]

ARG_FIELDS = [                                          # struct sfa_decode_args (include/star_flash_attn.h)
    ("qkv", ctypes.c_void_p), ("q_bias", ctypes.c_void_p), ("k_bias", ctypes.c_void_p), ("v_bias", ctypes.c_void_p),
    ("o", ctypes.c_void_p), ("seq_len", ctypes.c_void_p), ("k_cache_table", ctypes.c_void_p),
    ("v_cache_table", ctypes.c_void_p), ("rotary_cos_table", ctypes.c_void_p), ("rotary_sin_table", ctypes.c_void_p),
    ("batch_size", ctypes.c_int), ("memory_max_len", ctypes.c_int), ("num_heads", ctypes.c_int), ("head_dim", ctypes.c_int),
    ("head_dim_inv", ctypes.c_float), ("rotary_embedding_dim", ctypes.c_int), ("max_input_length", ctypes.c_int),
    ("stride", ctypes.c_int), ("num_layer", ctypes.c_int), ("idx_layer", ctypes.c_int), ("num_splits", ctypes.c_int),
    ("dtype", ctypes.c_int), ("workspace", ctypes.c_void_p), ("workspace_bytes", ctypes.c_size_t),
    ("kv_layout", ctypes.c_int), ("page_size", ctypes.c_int), ("block_table", ctypes.c_void_p),
    ("block_table_stride", ctypes.c_int), ("num_pages", ctypes.c_int), ("num_heads_kv", ctypes.c_int),
]


class Args(ctypes.Structure):
    _fields_ = ARG_FIELDS


ROW = (4 + 2 * 1) * 128                                 # (H + 2 * Hkv) * D of the base call


def base(e, window=None):
    """A well-formed call of entry point e but for its workspace (NULL): one kv head, batch 1, a shape whose automatic
    split count is above 1 -- memory_max_len 8192 for one token (4 splits), 4096 with 4 tokens for chunk and varlen
    (4 splits under window 2048).  A single-token call under window 2048 is not split (a split is at least 2048 rows), so
    the workspace cases give it window 6144 (3 splits) as well."""
    return {
        "args": True,
        "a": dict(qkv=0x1000, o=0x2000, seq_len=0x3000, k_cache_table=0x4000, v_cache_table=0x5000, batch_size=1,
                  num_heads=4, num_heads_kv=1, memory_max_len=8192 if e.single else 4096, num_layer=2, idx_layer=1,
                  head_dim=128, rotary_embedding_dim=64, dtype=1),
        "ks": 0x6000, "vs": 0x6100, "sinks": 0x6200, "cu": 0x6300, "count": 4, "tok": 0,
        "window": 2048 if window is None else window,
    }


def _a(**kw):
    return lambda s: s["a"].update(kw)


def _x(**kw):
    return lambda s: s.update(kw)


ALL = lambda e: True
MULTI = lambda e: not e.single
PAGED = dict(kv_layout=2, block_table=0x7000, page_size=16, num_pages=4096, block_table_stride=512)

# name -> (the entry points it applies to, what it does to the call)
MUTATIONS = {
    "args_null": (ALL, _x(args=False)),
    "qkv_null": (ALL, _a(qkv=None)),
    "o_null": (ALL, _a(o=None)),
    "seq_len_null": (ALL, _a(seq_len=None)),
    "k_cache_null": (ALL, _a(k_cache_table=None)),
    "v_cache_null": (ALL, _a(v_cache_table=None)),
    "cos_only": (ALL, _a(rotary_cos_table=0x8000)),
    "sin_only": (ALL, _a(rotary_sin_table=0x8000)),
    "count_neg": (MULTI, _x(count=-1)),
    "batch_neg": (ALL, _a(batch_size=-1)),
    "batch_65536": (ALL, _a(batch_size=65536)),
    "idx_layer_high": (ALL, _a(idx_layer=2)),
    "idx_layer_neg": (ALL, _a(idx_layer=-1)),
    "head_dim_96": (ALL, _a(head_dim=96, rotary_embedding_dim=0)),
    "head_dim_256": (ALL, _a(head_dim=256)),
    "rotary_odd": (ALL, _a(rotary_embedding_dim=3)),
    "rotary_large": (ALL, _a(rotary_embedding_dim=130)),
    "dtype_7": (ALL, _a(dtype=7)),
    "group_3": (ALL, _a(num_heads=3)),
    "heads_kv_neg": (ALL, _a(num_heads_kv=-1)),
    "tok_stride_small": (MULTI, _x(tok=ROW - 8)),
    "tok_stride_odd": (MULTI, _x(tok=ROW + 4)),
    "stride_small": (lambda e: not e.varlen, _a(stride=8)),
    "stride_odd": (lambda e: not e.varlen, _a(stride=4 * ROW + 4)),
    "stride_nonzero": (lambda e: e.varlen, _a(stride=4 * ROW)),
    "splits_1025": (ALL, _a(num_splits=1025)),
    "kv_layout_3": (ALL, _a(kv_layout=3)),
    "blhmd": (ALL, _a(kv_layout=1)),                    # (well-formed: as far as the workspace)
    "paged": (ALL, _a(**PAGED)),                        # (well-formed)
    "paged_no_table": (ALL, _a(**dict(PAGED, block_table=None))),
    "page_size_8": (ALL, _a(**dict(PAGED, page_size=8))),
    "page_size_24": (ALL, _a(**dict(PAGED, page_size=24))),
    "table_short": (ALL, _a(**dict(PAGED, block_table_stride=255))),
    "no_pages": (ALL, _a(**dict(PAGED, num_pages=0))),
    "table_misaligned": (ALL, _a(**dict(PAGED, block_table=0x7002))),
    "qkv_misaligned": (ALL, _a(qkv=0x1008)),
    "o_misaligned": (ALL, _a(o=0x2004)),
    "bias_misaligned": (ALL, _a(k_bias=0x9001)),
    "window_0": (lambda e: e.window, _x(window=0)),
    "window_neg": (lambda e: e.window, _x(window=-5)),
    "window_max": (lambda e: e.window, _x(window=2 ** 31 - 1)),     # (well-formed)
    "k_scale_misaligned": (lambda e: e.kv8, _x(ks=0x6001)),
    "v_scale_misaligned": (lambda e: e.kv8, _x(vs=0x6102)),
    "scales_null": (lambda e: e.kv8, _x(ks=None, vs=None)),         # (well-formed: NULL = 1.0)
    "sinks_misaligned": (lambda e: e.sinks, _x(sinks=0x6203)),
    "sinks_null": (lambda e: e.sinks, _x(sinks=None)),              # (well-formed: the twin's call)
    "cu_null": (lambda e: e.varlen, _x(cu=None)),
    "cu_misaligned": (lambda e: e.varlen, _x(cu=0x6302)),
    "batch_0": (ALL, _a(batch_size=0)),                 # nothing to do
    "count_0": (MULTI, _x(count=0)),                    # nothing to do
    # more than 2^31 - 1 attention workgroups: 65537 plan slots x 64 kv heads x 1024 splits
    "varlen_grid": (lambda e: e.varlen, lambda s: (s.update(count=1 << 24), s["a"].update(num_heads=64, num_heads_kv=64,
                                                                                           num_splits=1024))),
}

# The order of the checks is pinned by pairs of mutations.  The checks that the flavours and shapes add are where the
# entry points differ in order: every pair of these is called, and each of them with four of the shared checks (the first
# two, one in the middle and the last), and those four with each other
SPECIFIC = ("sinks_misaligned", "k_scale_misaligned", "cu_null", "cu_misaligned", "head_dim_256", "window_0", "batch_0",
            "count_0", "varlen_grid")
SHARED = ("args_null", "qkv_null", "count_neg", "qkv_misaligned")
# ... and pairs with a mutation that is not among those
PAIRS = [("sinks_misaligned", "v_scale_misaligned"), ("v_scale_misaligned", "window_neg"), ("cu_null", "seq_len_null"),
         ("window_0", "batch_0"), ("head_dim_256", "v_scale_misaligned"), ("scales_null", "args_null"),
         ("sinks_null", "window_0"), ("cu_null", "stride_nonzero"), ("window_max", "count_0")]


def call(lib, e, s):
    """Make the call s of entry point e: (status, sfa_last_error()).  The error text is first set to a known one (that of
    sfa_debug_set(NULL)), so a call that succeeds shows that it left the text alone."""
    P = ctypes.c_void_p
    a = Args()
    for k, v in s["a"].items():
        setattr(a, k, v)
    argv = [ctypes.byref(a) if s["args"] else None]
    if e.kv8:
        argv += [P(s["ks"]), P(s["vs"])]
    if e.sinks:
        argv += [P(s["sinks"])]
    if e.varlen:
        argv += [P(s["cu"])]
    if not e.single:
        argv += [ctypes.c_int(s["count"]), ctypes.c_int64(s["tok"])]
    if e.window:
        argv += [ctypes.c_int(s["window"])]
    argv += [None]                                      # the stream
    fn = getattr(lib, e.name)
    fn.restype = ctypes.c_int
    lib.sfa_last_error.restype = ctypes.c_char_p
    lib.sfa_debug_set.restype = ctypes.c_int
    lib.sfa_debug_set(None, ctypes.c_int(0))
    status = fn(*argv)
    return status, lib.sfa_last_error().decode()


def _size(lib, e, s, num_splits):
    fn = getattr(lib, e.sizing)
    fn.restype = ctypes.c_size_t
    a = s["a"]
    v = [a["batch_size"], a["num_heads"]] + ([a["num_heads_kv"]] if e.sizing != "sfa_decode_workspace_bytes" else [])
    v += [a["head_dim"], a["memory_max_len"]] + ([] if e.single else [s["count"]]) + ([s["window"]] if e.window else [])
    return fn(*[ctypes.c_int(x) for x in v + [num_splits]])


def workspace_cases(lib, e):
    """The split count and the workspace layout, read off the `need %zu` of the workspace errors"""
    out = {}
    for w in ([2048, 6144] if e.single and e.window else [2048]):
        def spec(**kw):
            s = base(e, w)
            s["a"].update(kw)
            return s
        tag = "ws_w%d_" % w if e.window else "ws_"
        out[tag + "null"] = spec()                                              # no trim: the automatic count
        out[tag + "null_splits_2"] = spec(num_splits=2)
        # too small for one split (a single-token call needs 256 bytes for that): trimmed to one split where the call trims
        tiny = 255 if e.single else 256
        out[tag + "tiny"] = spec(workspace=0x10000, workspace_bytes=tiny)
        out[tag + "tiny_splits_2"] = spec(workspace=0x10000, workspace_bytes=tiny, num_splits=2)
        two = _size(lib, e, spec(), 2)
        out[tag + "short_splits_2"] = spec(workspace=0x10000, workspace_bytes=two - 1, num_splits=2)
        out[tag + "misaligned_splits_2"] = spec(workspace=0x10010, workspace_bytes=two, num_splits=2)
        out[tag + "misaligned_large"] = spec(workspace=0x10080, workspace_bytes=1 << 40)
        if not e.trims:     # (a call that trims would run with one split less)
            out[tag + "short_auto"] = spec(workspace=0x10000, workspace_bytes=_size(lib, e, spec(), 0) - 1)
    return out


def cases(lib, e):
    """name -> call spec, for entry point e"""
    applies = lambda m: MUTATIONS[m][0](e)
    out = {"base": base(e)}
    names = [(m,) for m in MUTATIONS if applies(m)]
    pairs = list(itertools.combinations(SHARED, 2)) + list(itertools.product(SHARED, SPECIFIC))
    pairs += list(itertools.combinations(SPECIFIC, 2)) + PAIRS
    names += [p for p in pairs if applies(p[0]) and applies(p[1])]
    for ms in names:
        s = base(e)
        for m in ms:
            MUTATIONS[m][1](s)
        out["+".join(ms)] = s
    out.update(workspace_cases(lib, e))
    return out


def run_all(lib):
    """{entry point: {case: [status, error text]}} of the library `lib` (a ctypes.CDLL)"""
    return {e.name: {k: list(call(lib, e, s)) for k, s in cases(lib, e).items()} for e in ENTRIES}


def group(results):
    """The record as it is kept: rows [status, error text with the entry point's name as {fn}, the entry points (blank
    between names) that end so in the same cases, those cases]"""
    rows = {}
    for name, by_case in results.items():
        ends = {}
        for case, (status, text) in by_case.items():
            text = "{fn}" + text[len(name):] if text.startswith(name + ":") else text
            ends.setdefault((status, text), []).append(case)
        for end, cs in ends.items():
            rows.setdefault(end + (tuple(cs),), []).append(name)
    return [[status, text, " ".join(names), list(cs)] for (status, text, cs), names in rows.items()]


def ungroup(rows):
    """group()'s inverse; a case listed twice is an error"""
    out = {}
    for status, text, names, cs in rows:
        for name in names.split():
            for case in cs:
                assert case not in out.setdefault(name, {}), (name, case)
                out[name][case] = [status, text.replace("{fn}", name)]
    return out
