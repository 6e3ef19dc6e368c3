"""CPU-only checks of the K / V row-pitch limit of the prefill calls (include/star_flash_attn.h, sfa_prefill_args; the
limits are written once, in csrc/prefill_common.h).

The 8-wave kernels keep a key tile's base in 64 bits and form a row's byte offset inside the tile in 32:
row * 2 * pitch + 16 * chunk, row < T (the tile's keys), chunk < head_dim / 8.  The limit is the largest multiple of 8 at
which the last chunk of the last row stays below 2^32; one notch (8 elements: strides are multiples of 8) above it that
offset wraps, and rows T/2 .. T-1 of every tile would be read from the wrong place.  So every call rejects limit + 8 and
accepts the limit.

Fake pointers, as in the other tests/test_prefill_*_cpu.py: every case returns before a launch.  "Accepts" therefore
means: the call gets past the pitch check and ends at a later check, one that the same call with limit + 8 does not
reach --
  * the packed calls and sfa_prefill_split_fwd: the NULL workspace (SFA_ERR_NULL_POINTER);
  * sfa_prefill_window_fwd: a grid beyond 2^31 - 1 workgroups (the last check before its launch);
  * sfa_prefill_fwd, whose check sits in the dispatcher because the limit depends on the kernel picked: prefill_impl 2,
    a diagnostic build of the 256-row kernel (64-key tiles) that the release library does not hold, so the call ends at
    "needs the diagnostics build".  The 128-row kernel has no such stand-in: its rejection is checked here, its acceptance
    at the limit by tests/test_far_memory_prefill_gpu.py, which runs it there.
"""
import ctypes
import os

import pytest

from far_memory import pitch_limit, wraps_at
from starflashattention_amd import _lib
from test_prefill_split_cpu import _well_formed as rect_args
from test_prefill_varlen_cpu import _well_formed as packed_args

WS, BIG = 0x100000, 1 << 30
DIMS = (64, 128)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = _lib.load()
    lib.sfa_debug_get.restype = ctypes.c_int
    lib.sfa_debug_get.argtypes = [ctypes.c_char_p]
    return lib


def test_the_limit_is_where_the_row_offset_wraps():
    """63 (31) * row bytes + the last chunk's offset is below 2^32 at the limit and not at limit + 8"""
    assert pitch_limit(64, 128) == pitch_limit(64, 64) == 34087040
    assert (pitch_limit(32, 128), pitch_limit(32, 64)) == (69273656, 69273664)
    for T in (64, 32):
        for D in DIMS:
            lim = pitch_limit(T, D)
            assert lim % 8 == 0
            assert (T - 1) * 2 * lim + 16 * (D // 8 - 1) < 2 ** 32 <= (T - 1) * 2 * (lim + 8) + 16 * (D // 8 - 1)
            assert not wraps_at(lim, T, D) and wraps_at(lim + 8, T, D)
            # what wraps first is the second half of the tile: at limit + 8 no row of the first half does
            assert (T // 2 - 1) * 2 * (lim + 8) + 16 * (D // 8 - 1) < 2 ** 32


def message(name, which, what, pitch, T, D):
    return b"%s: %s %s stride %d exceeds %d elements, the row pitch the %d-key tiles address at head_dim %d" % (
        name, which, what, pitch, pitch_limit(T, D), T, D)


def set_pitch(p, which, pitch, packed):
    st = p.k_stride if which == b"k" else p.v_stride
    st[0 if packed else 2] = pitch


# (name, the call on args p with a NULL workspace, packed, (status, text) the call ends with AT the limit)
def _rect(name, *extra):
    return lambda lib, p: getattr(lib, name)(ctypes.byref(p), *extra, None)


CALLS = [
    ("sfa_prefill_window_fwd", _rect("sfa_prefill_window_fwd", 40, None), False, (-2, b"grid too large")),
    ("sfa_prefill_split_fwd", _rect("sfa_prefill_split_fwd", 2, None, 0), False, (-1, b"workspace is NULL")),
    ("sfa_prefill_varlen_fwd", _rect("sfa_prefill_varlen_fwd", None, 0), True, (-1, b"workspace is NULL")),
    ("sfa_prefill_varlen_window_fwd", _rect("sfa_prefill_varlen_window_fwd", 40, None, None, 0), True,
     (-1, b"workspace is NULL")),
    ("sfa_prefill_varlen_split_fwd", _rect("sfa_prefill_varlen_split_fwd", 520, 3, None, 0), True,
     (-1, b"workspace is NULL")),
]


def _args(name, packed, D):
    p = packed_args() if packed else rect_args()
    p.head_dim = D
    if name == "sfa_prefill_window_fwd":        # 2^24 (batch, head) pairs of 129 q-tiles: one workgroup too many
        p.batch, p.heads_q, p.heads_kv, p.seqlen_q = 2 ** 22, 4, 2, 128 * 256 + 1
    return p


@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("which", [b"k", b"v"])
@pytest.mark.parametrize("call", CALLS, ids=[c[0] for c in CALLS])
def test_stream_calls_reject_above_the_limit_and_accept_it(lib, call, which, D):
    name, fn, packed, (st_ok, text_ok) = call
    lim = pitch_limit(64, D)
    last = lib.sfa_debug_get(b"last_prefill_kernel")
    # at the limit: past the pitch check, as far as the later check
    p = _args(name, packed, D)
    set_pitch(p, b"k", lim, packed)
    set_pitch(p, b"v", lim, packed)
    assert fn(lib, p) == st_ok, lib.sfa_last_error()
    assert lib.sfa_last_error().startswith(name.encode() + b":") and text_ok in lib.sfa_last_error()
    # nothing to do: SFA_OK at the limit, the rejection above it (the pitch belongs to the stride checks, which come first)
    for empty in ("batch", "total_q" if packed else "seqlen_q"):
        p = _args(name, packed, D)
        set_pitch(p, which, lim, packed)
        setattr(p, empty, 0)
        assert fn(lib, p) == 0
        set_pitch(p, which, lim + 8, packed)
        assert fn(lib, p) == -2
    # one notch above: SFA_ERR_BAD_SHAPE under the call's name, with the pitch and the limit
    p = _args(name, packed, D)
    set_pitch(p, which, lim + 8, packed)
    assert fn(lib, p) == -2
    assert lib.sfa_last_error() == message(name.encode(), which, b"token" if packed else b"seq", lim + 8, 64, D)
    # ... and after the other stride checks, before the alignment check
    p.k = 0x2008
    assert fn(lib, p) == -2 and lib.sfa_last_error().startswith(name.encode() + b": " + which)
    p.q_stride[1] = 12
    assert fn(lib, p) == -2 and b"multiples of 8" in lib.sfa_last_error()
    assert lib.sfa_debug_get(b"last_prefill_kernel") == last          # no call got as far as a launch


@pytest.fixture
def impl(lib):
    lib.sfa_debug_set.argtypes = [ctypes.c_char_p, ctypes.c_int]
    yield lambda v: lib.sfa_debug_set(b"prefill_impl", v)
    lib.sfa_debug_set(b"prefill_impl", -1)


@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("which", [b"k", b"v"])
def test_prefill_fwd_checks_the_limit_of_the_kernel_it_picks(lib, impl, which, D):
    name = b"sfa_prefill_fwd"
    fwd = lambda p: lib.sfa_prefill_fwd(ctypes.byref(p), None)
    last = lib.sfa_debug_get(b"last_prefill_kernel")
    lim64, lim32 = pitch_limit(64, D), pitch_limit(32, D)
    # the 256-row kernel's 64-key tiles, through its diagnostic build that this library does not hold
    impl(2)
    p = rect_args()
    p.head_dim = D
    set_pitch(p, b"k", lim64, False)
    set_pitch(p, b"v", lim64, False)
    assert fwd(p) == -2 and b"needs the diagnostics build" in lib.sfa_last_error()     # accepted: the next check
    set_pitch(p, which, lim64 + 8, False)
    assert fwd(p) == -2 and lib.sfa_last_error() == message(name, which, b"seq", lim64 + 8, 64, D)
    # forced, by id: the 256-row kernel at its limit + 8, the 128-row kernel (32-key tiles) at its own
    # (rejections only: a forced kernel that accepts would launch)
    for ids, T, lim in (((1, 3, 10), 64, lim64), ((20, 21, 22), 32, lim32)):
        set_pitch(p, which, lim + 8, False)
        for i in ids:
            impl(i)
            assert fwd(p) == -2 and lib.sfa_last_error() == message(name, which, b"seq", lim + 8, T, D), i
    # the library's own choice for this small grid is the 128-row kernel: its limit holds
    impl(-1)
    assert fwd(p) == -2 and lib.sfa_last_error() == message(name, which, b"seq", lim32 + 8, 32, D)
    assert lib.sfa_debug_get(b"last_prefill_kernel") == last          # no call got as far as picking a kernel
    # the 4-wave kernel forced: its own refusal (descriptors, or the head_dim), not this one
    impl(42)
    assert fwd(p) in (-2, -4) and not lib.sfa_last_error().startswith(name + b": " + which + b" seq stride")


def test_head_dim_256_takes_any_pitch(lib, impl):
    """prefill_d256_kernel.hip indexes in 64 bits: under the stand-in id that ends a head_dim 64 / 128 call at the pitch
    check, a head_dim 256 call gets past it, at a pitch far beyond every limit"""
    impl(2)
    for pitch in (pitch_limit(64, 128) + 8, pitch_limit(32, 64) + 8, 2 ** 33):
        p = rect_args()
        p.head_dim = 256
        set_pitch(p, b"k", pitch, False)
        set_pitch(p, b"v", pitch, False)
        assert lib.sfa_prefill_fwd(ctypes.byref(p), None) == -2
        assert b"needs the diagnostics build" in lib.sfa_last_error(), lib.sfa_last_error()
        p.head_dim = 128
        assert lib.sfa_prefill_fwd(ctypes.byref(p), None) == -2 and b"seq stride" in lib.sfa_last_error()
