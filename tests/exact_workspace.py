"""Shared by the GPU tests that call a decode entry point of the C ABI with a workspace of exactly the size its
*_workspace_bytes function returns: the regions the entry point carves out of it must lie inside it."""
import ctypes

import torch

from starflashattention_amd import _lib

CANARY = 0xA5


def decode_problem(lead, B, H, Hkv, D, L, M, seed, device):
    """fp16 tensors of one grouped-query decode call over blmhd caches: qkv [*lead, H + 2*Hkv, D], the two caches, o."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    rand = lambda *shape: torch.randn(*shape, generator=g).half().to(device)
    return (rand(*lead, H + 2 * Hkv, D), rand(B, L, M, Hkv, D), rand(B, L, M, Hkv, D),
            torch.full((*lead, H, D), 7.0, dtype=torch.float16, device=device))


def call_with_exact_workspace(a, nbytes, num_splits, call, device, fill=CANARY):
    """Give the filled sfa_decode_args `a` a workspace of exactly nbytes, followed in the same allocation by 256 canary
    bytes, make call(args, stream) -> status, and check the status, the polled status and the canary.  fill: what the
    workspace itself holds before the call (0xFF: every fp32 of it a NaN, so a partial that is read without having been
    written shows in the output); the guard bytes behind it are always CANARY."""
    lib = _lib.load()
    buf = torch.full((nbytes + 256,), CANARY, dtype=torch.uint8, device=device)
    if fill != CANARY:
        buf[:nbytes] = fill
    assert buf.data_ptr() % 256 == 0
    stream = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
    _lib.check(lib.sfa_decode_reset_status(ctypes.c_void_p(buf.data_ptr()), stream))
    a.num_splits, a.workspace, a.workspace_bytes = num_splits, buf.data_ptr(), nbytes
    _lib.check(call(ctypes.byref(a), stream))
    assert lib.sfa_decode_poll_status(ctypes.c_void_p(buf.data_ptr()), stream) == 0
    torch.cuda.synchronize(device)
    assert bool((buf[nbytes:] == CANARY).all()), "the call wrote past the workspace it asked for"
    assert not bool((buf[256:nbytes] == fill).all()), "the partials were not written"
