"""Host-side operators over the C ABI: torch tensors in, HIP kernels underneath.

torch is plumbing here (device memory, current stream); every byte of compute happens in
libStarFlashAttention.so.  The public operators:

  flash_decode(...)   same arguments, meaning and side effects as the reference's
                      star_flash_attn.mha_fwd_cuda (src/flash_api.cpp:42-68): mutates `o` and the
                      two caches in place and returns `o`.
  flash_attn_fwd(...) prefill forward (new entry point; the reference is decode-only).
  flash_decode_chunk(...)  n new tokens per sequence in one call: prompt ingestion, chunked prefill,
                      speculative verification (new entry point).
  flash_decode_varlen(...) the same with a token count of its own per sequence, packed: one call for a mixed
                      prefill / verify / decode step (new entry point).
  flash_decode_kv8(...)  flash_decode over an fp8 (e4m3) KV cache with a scale per kv head; quantize_kv8(...) moves
                      16-bit cache rows into such a cache (new entry points).
  flash_decode_window(...)  flash_decode with a sliding window: the token attends to the last `window` positions only
                      (new entry point).
  flash_decode_chunk_window(...) / flash_decode_varlen_window(...)  flash_decode_chunk / flash_decode_varlen with that
                      window: what n successive flash_decode_window calls give (new entry points).
  flash_decode_chunk_kv8(...) / flash_decode_varlen_kv8(...)  flash_decode_chunk / flash_decode_varlen over an fp8 KV
                      cache: what n successive flash_decode_kv8 calls give (new entry points).
  flash_decode_chunk_kv8_window(...)  flash_decode_chunk_kv8 with the sliding window: what n successive
                      flash_decode_kv8_window calls give (new entry point).
  flash_decode_varlen_kv8_window(...)  flash_decode_varlen_kv8 with the sliding window (new entry point).
  flash_decode_window_sinks(...) / flash_decode_chunk_window_sinks(...) / flash_decode_varlen_window_sinks(...)  the
                      three windowed calls over 16-bit caches with a learned sink logit per query head in every softmax
                      (new entry points).
  flash_decode_kv8_window_sinks(...) / flash_decode_chunk_kv8_window_sinks(...) /
  flash_decode_varlen_kv8_window_sinks(...)  the same sink in the three windowed calls over an fp8 KV cache (new entry
                      points).
  flash_attn_window_fwd(...) / flash_attn_split_fwd(...) / flash_attn_varlen_fwd(...)  flash_attn_fwd under a sliding
                      window with attention sinks, with a split key range for small grids, and over packed sequences of
                      different lengths delimited by cu_seqlens_q / cu_seqlens_k (new entry points).
"""
import ctypes
import math

import torch

from . import _lib

_DTYPES = {torch.float16: _lib.DTYPE_FP16, torch.bfloat16: _lib.DTYPE_BF16}

_KV8_DTYPES = (torch.uint8, torch.float8_e4m3fn)     # an e4m3 cache, as bytes or as torch's own type

_workspaces = {}          # (device index, stream) -> torch.uint8 tensor
_STATUS_BYTES = 256   # the status block at the front of that tensor (the decode calls' sticky error word)
_sync_checks = False


def set_sync_checks(enabled: bool):
    """When on, flash_decode synchronises after every call and raises if a seq_len[b] was out of
    range (the kernel rejects such rows on the device either way)."""
    global _sync_checks
    _sync_checks = bool(enabled)


def _stream_ptr(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _require(cond, msg):
    if not cond:
        raise RuntimeError("star_flash_attn: " + msg)


def _check_gpu_tensor(t, name, dtype=None, shape=None, device=None):
    _require(isinstance(t, torch.Tensor), f"{name} must be a tensor")
    _require(t.is_cuda, f"{name} must live on a HIP device (got {t.device})")
    if device is not None:
        _require(t.device == device, f"{name} is on {t.device}, expected {device}")
    if dtype is not None:
        _require(t.dtype == dtype, f"{name} has dtype {t.dtype}, expected {dtype}")
    if shape is not None:
        _require(tuple(t.shape) == tuple(shape), f"{name} has shape {tuple(t.shape)}, expected {tuple(shape)}")
    _require(t.is_contiguous(), f"{name} must be contiguous")


def _workspace(device, nbytes):
    lib = _lib.load()
    key = (device.index, torch.cuda.current_stream(device).cuda_stream)
    ws = _workspaces.get(key)
    if ws is None or ws.numel() < nbytes:
        grown = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=device)
        if ws is None:
            _lib.check(lib.sfa_decode_reset_status(ctypes.c_void_p(grown.data_ptr()), _stream_ptr(device)))
        else:
            grown[:256].copy_(ws[:256])      # the sticky status block survives growth (stream-ordered, no sync)
        _workspaces[key] = ws = grown
    return ws


def release_workspaces():
    """Drop the cached decode scratch of every (device, stream).  Pending sticky flags are lost:
    call check_decode_status() first if they matter."""
    _workspaces.clear()


def _decode_args(qkv, q_bias, k_bias, v_bias, k_cache_table, v_cache_table, seq_len, o, batch_size, memory_max_len,
                 num_heads, head_dim, rotary_embedding_dim, max_input_length, num_layer, idx_layer, rotary_cos_table,
                 rotary_sin_table, softmax_scale, kv_layout, block_table, num_heads_kv, tokens=None, packed=None,
                 kv8=False):
    """Check the tensors of one decode call and fill its sfa_decode_args, all but the workspace, num_splits and stride.
    tokens None: flash_decode (qkv [B, 3, H, D] or [B, H + 2*Hkv, D], o [B, H, D]); tokens = n: flash_decode_chunk
    (qkv [B, n, 3, H, D] or [B, n, H + 2*Hkv, D], o [B, n, H, D]); packed = T: flash_decode_varlen (qkv [T, 3, H, D] or
    [T, H + 2*Hkv, D], o [T, H, D]: the tokens of all sequences, one after another).  kv8: the caches hold e4m3 bytes
    (torch.uint8 or torch.float8_e4m3fn).  Returns (args, B, H, Hkv, D, M)."""
    _require(isinstance(qkv, torch.Tensor) and qkv.dtype in _DTYPES,
             f"qkv must be a float16 or bfloat16 tensor (got {getattr(qkv, 'dtype', type(qkv))})")
    dt, dev = qkv.dtype, qkv.device
    B, H, D, M, L = int(batch_size), int(num_heads), int(head_dim), int(memory_max_len), int(num_layer)
    Hkv = H if num_heads_kv is None else int(num_heads_kv)
    _require(Hkv > 0 and H % Hkv == 0, f"num_heads={H} must be a multiple of num_heads_kv={Hkv}")
    lead = (packed,) if packed is not None else (B,) if tokens is None else (B, tokens)
    _check_gpu_tensor(qkv, "qkv", dt, lead + ((3, H, D) if Hkv == H else (H + 2 * Hkv, D)))
    _check_gpu_tensor(o, "o", dt, lead + (H, D), dev)
    _check_gpu_tensor(seq_len, "seq_len", torch.int32, (B,), dev)
    _require(kv_layout in _lib.KV_LAYOUTS, f"kv_layout must be one of {sorted(_lib.KV_LAYOUTS)} (got {kv_layout!r})")
    if kv_layout == "paged":
        _require(isinstance(block_table, torch.Tensor) and block_table.dim() == 2,
                 "kv_layout='paged' needs block_table, an int32 [batch, pages_per_seq] tensor")
        _require(isinstance(k_cache_table, torch.Tensor) and k_cache_table.dim() == 5,
                 "k_cache_table must be a [num_pages, num_layer, page_size, num_heads, head_dim] pool")
        num_pages, page_size = int(k_cache_table.shape[0]), int(k_cache_table.shape[2])
        cache_shape = (num_pages, L, page_size, Hkv, D)
        _check_gpu_tensor(block_table, "block_table", torch.int32, (B, int(block_table.shape[1])), dev)
    else:
        _require(block_table is None, "block_table is only meaningful with kv_layout='paged'")
        cache_shape = (B, L, M, Hkv, D) if kv_layout == "blmhd" else (B, L, Hkv, M, D)
    for name, t in (("k_cache_table", k_cache_table), ("v_cache_table", v_cache_table)):
        if kv8:
            _require(isinstance(t, torch.Tensor) and t.dtype in _KV8_DTYPES,
                     f"{name} must be a uint8 or float8_e4m3fn tensor (got {getattr(t, 'dtype', type(t))})")
        _check_gpu_tensor(t, name, t.dtype if kv8 else dt, cache_shape, dev)
    biases = []
    for name, t in (("q_bias", q_bias), ("k_bias", k_bias), ("v_bias", v_bias)):
        if t is None or t.numel() == 0:
            biases.append(None)
        else:
            _check_gpu_tensor(t, name, dt, (H if name == "q_bias" else Hkv, D), dev)
            biases.append(t)
    for name, t in (("rotary_cos_table", rotary_cos_table), ("rotary_sin_table", rotary_sin_table)):
        if t is not None:
            _check_gpu_tensor(t, name, dt, (M, int(rotary_embedding_dim) // 2), dev)
    a = _lib.DecodeArgs()
    a.qkv = qkv.data_ptr()
    a.q_bias, a.k_bias, a.v_bias = (b.data_ptr() if b is not None else None for b in biases)
    a.o = o.data_ptr()
    a.seq_len = seq_len.data_ptr()
    a.k_cache_table = k_cache_table.data_ptr()
    a.v_cache_table = v_cache_table.data_ptr()
    a.rotary_cos_table = rotary_cos_table.data_ptr() if rotary_cos_table is not None else None
    a.rotary_sin_table = rotary_sin_table.data_ptr() if rotary_sin_table is not None else None
    a.batch_size, a.memory_max_len, a.num_heads, a.head_dim = B, M, H, D
    a.head_dim_inv = float(softmax_scale) if softmax_scale else 1.0 / math.sqrt(D)
    a.rotary_embedding_dim = int(rotary_embedding_dim)
    a.max_input_length = int(max_input_length)
    a.num_heads_kv = Hkv
    a.num_layer, a.idx_layer = L, int(idx_layer)
    a.dtype = _DTYPES[dt]
    a.kv_layout = _lib.KV_LAYOUTS[kv_layout]
    if kv_layout == "paged":
        a.page_size, a.num_pages = page_size, num_pages
        a.block_table = block_table.data_ptr()
        a.block_table_stride = int(block_table.shape[1])
    return a, B, H, Hkv, D, M


def _call_decode(dev, a, stride, num_splits, ws, fn, extra):
    """What the decode operators end in: the batch stride, the split count and the workspace go into `a`,
    fn(args, *extra, stream) makes the C-ABI call and, with sync checks on, the status is polled."""
    a.stride = stride
    a.num_splits = num_splits
    a.workspace = ws.data_ptr()
    a.workspace_bytes = ws.numel()
    _lib.check(fn(ctypes.byref(a), *extra, _stream_ptr(dev)))
    if _sync_checks:
        check_decode_status(dev)


def _kv8_scale(t, name, Hkv, dev):
    if t is None:
        return None
    _check_gpu_tensor(t, name, torch.float32, (Hkv,), dev)
    return ctypes.c_void_p(t.data_ptr())


def _window_int(window):
    W = int(window)
    _require(-2 ** 31 <= W < 2 ** 31, f"window={window} does not fit an int")
    return W


def _sinks_ptr(sinks, H, dev):
    """sinks: None (NULL: the call is its _window twin) or a float32 [num_heads] device tensor, one logit per query head"""
    if sinks is None:
        return None
    _check_gpu_tensor(sinks, "sinks", torch.float32, (H,), dev)
    return ctypes.c_void_p(sinks.data_ptr())


def _decode_op(shape, flavour, qkv, q_bias, k_bias, v_bias, k_cache_table, v_cache_table, seq_len, o, batch_size,
               memory_max_len, num_heads, head_dim, rotary_embedding_dim, max_input_length, num_layer, idx_layer,
               num_splits, rotary_cos_table, rotary_sin_table, softmax_scale, kv_layout, block_table, num_heads_kv,
               cu_tokens=None, window=None, sinks=None, k_scale=None, v_scale=None, sized_by_query_heads=False):
    """The body of the 18 flash_decode* operators: the C call sfa_decode<shape><flavour>, shape "" / "_chunk" / "_varlen",
    flavour "" / "_window" / "_window_sinks" / "_kv8" / "_kv8_window" / "_kv8_window_sinks".  The C calls take, between
    args and the stream, [k_scale, v_scale], [sinks], [cu_tokens], [count, token stride], [window] (as _lib.load() declares
    them); the operators check their arguments in the order window, scales, sinks, cu_tokens.  Returns `o`."""
    lib = _lib.load()
    windowed, kv8 = "_window" in flavour, "_kv8" in flavour
    tokens = packed = None
    if shape == "_chunk":
        _require(isinstance(qkv, torch.Tensor) and qkv.dim() in (4, 5),
                 f"qkv must be [B, n, 3, H, D] or [B, n, H + 2*Hkv, D] (got {tuple(getattr(qkv, 'shape', ()))})")
        tokens = count = int(qkv.shape[1])
    elif shape:
        _require(isinstance(qkv, torch.Tensor) and qkv.dim() in (3, 4),
                 f"qkv must be [T, 3, H, D] or [T, H + 2*Hkv, D] (got {tuple(getattr(qkv, 'shape', ()))})")
        packed = count = int(qkv.shape[0])
    a, B, H, Hkv, D, M = _decode_args(qkv, q_bias, k_bias, v_bias, k_cache_table, v_cache_table, seq_len, o, batch_size,
                                      memory_max_len, num_heads, head_dim, rotary_embedding_dim, max_input_length,
                                      num_layer, idx_layer, rotary_cos_table, rotary_sin_table, softmax_scale,
                                      kv_layout, block_table, num_heads_kv, tokens, packed, kv8)
    dev = qkv.device
    extra = []
    if windowed:
        W = _window_int(window)
    if kv8:
        extra += [_kv8_scale(k_scale, "k_scale", Hkv, dev), _kv8_scale(v_scale, "v_scale", Hkv, dev)]
    if "_sinks" in flavour:
        extra.append(_sinks_ptr(sinks, H, dev))
    if packed is not None:
        _check_gpu_tensor(cu_tokens, "cu_tokens", torch.int32, (B + 1,), dev)
        extra.append(ctypes.c_void_p(cu_tokens.data_ptr()))
    dims = [B, H, Hkv, D, M]        # ... and what the sizing function of the shape and window takes behind them
    if shape:
        extra += [count, 0]         # (token stride 0: packed rows)
        dims.append(count)
    if windowed:
        extra.append(W)
        dims.append(W)
    fn = getattr(lib, "sfa_decode" + shape + flavour)
    with torch.cuda.device(dev):
        S = int(num_splits) if num_splits and num_splits > 0 else 0
        if shape or windowed:
            size = getattr(lib, "sfa_decode" + shape + ("_window" if windowed else "") + "_workspace_bytes")
            ws = _workspace(dev, size(*dims, S))
        else:
            # the library sizes the split count by the KV heads (one workgroup serves a whole group); flash_decode and
            # flash_decode_kv8 resolve an unset count themselves and pass it on
            S = S or lib.sfa_decode_auto_splits(B, Hkv, D, M)
            ws = _workspace(dev, lib.sfa_decode_workspace_bytes(B, H, D, M, S))
            if sized_by_query_heads:
                # (tests) the older contract of the C ABI: a caller that leaves the split count to the library sizes its
                # workspace with sfa_decode_workspace_bytes(..., 0), which knows the query-head count only
                S = 0
                ws = torch.empty(lib.sfa_decode_workspace_bytes(B, H, D, M, 0), dtype=torch.uint8, device=dev)
                _lib.check(lib.sfa_decode_reset_status(ctypes.c_void_p(ws.data_ptr()), _stream_ptr(dev)))
        # (stride 0 of a chunk: n * (H + 2*Hkv) * D, computed by the library in 64 bit)
        _call_decode(dev, a, 0 if shape else (H + 2 * Hkv) * D, S, ws, fn, extra)
    return o


def flash_decode(qkv, q_bias, k_bias, v_bias, k_cache_table, v_cache_table, seq_len, o,
                 batch_size, memory_max_len, num_heads, head_dim, rotary_embedding_dim,
                 max_input_length, num_layer, idx_layer, *, num_splits=0, _sized_by_query_heads=False,
                 rotary_cos_table=None, rotary_sin_table=None, softmax_scale=None, kv_layout="blmhd",
                 block_table=None, num_heads_kv=None):
    """One decode step (see include/star_flash_attn.h, sfa_decode).  Returns `o` (same tensor).
    kv_layout: "blmhd" = the reference's [B, L, M, H, D] caches; "blhmd" = head-major [B, L, H, M, D];
    "paged" = page pools [num_pages, L, page_size, H, D] addressed through block_table (int32
    [B, pages_per_seq]); memory_max_len is then the capacity of one sequence.
    num_heads_kv (grouped queries, an extension): qkv is then [B, num_heads + 2*num_heads_kv, D] (q heads,
    k heads, v heads), k_bias / v_bias and the caches carry num_heads_kv heads."""
    return _decode_op("", "", qkv, q_bias, k_bias, v_bias, k_cache_table, v_cache_table, seq_len, o, batch_size,
                      memory_max_len, num_heads, head_dim, rotary_embedding_dim, max_input_length, num_layer, idx_layer,
                      num_splits, rotary_cos_table, rotary_sin_table, softmax_scale, kv_layout, block_table, num_heads_kv,
                      sized_by_query_heads=_sized_by_query_heads)


def flash_decode_window(qkv, q_bias, k_bias, v_bias, k_cache_table, v_cache_table, seq_len, o,
                        batch_size, memory_max_len, num_heads, head_dim, rotary_embedding_dim,
                        max_input_length, num_layer, idx_layer, window, *, num_splits=0,
                        rotary_cos_table=None, rotary_sin_table=None, softmax_scale=None, kv_layout="blmhd",
                        block_table=None, num_heads_kv=None):
    """flash_decode with a sliding window (include/star_flash_attn.h, sfa_decode_window): the new token at position
    pos = seq_len[b] attends to itself and the window - 1 cache rows before it, lo = max(0, pos + 1 - window) .. pos
    (flash-attn's window_size = (window - 1, 0)).  window >= 1; every other argument as in flash_decode.  Cache rows
    below lo, and block_table entries of pages wholly below lo, are never read.  Returns `o`."""
    return _decode_op("", "_window", qkv, q_bias, k_bias, v_bias, k_cache_table, v_cache_table, seq_len, o, batch_size,
                      memory_max_len, num_heads, head_dim, rotary_embedding_dim, max_input_length, num_layer, idx_layer,
                      num_splits, rotary_cos_table, rotary_sin_table, softmax_scale, kv_layout, block_table, num_heads_kv,
                      window=window)


def flash_decode_kv8(qkv, q_bias, k_bias, v_bias, k_cache_table, v_cache_table, seq_len, o,
                     batch_size, memory_max_len, num_heads, head_dim, rotary_embedding_dim,
                     max_input_length, num_layer, idx_layer, *, num_splits=0,
                     rotary_cos_table=None, rotary_sin_table=None, softmax_scale=None, kv_layout="blmhd",
                     block_table=None, num_heads_kv=None, k_scale=None, v_scale=None):
    """flash_decode over an fp8 KV cache (include/star_flash_attn.h, sfa_decode_kv8).  The caches are torch.uint8 or
    torch.float8_e4m3fn tensors in flash_decode's layouts; qkv, the biases, the rotary tables and o stay fp16 / bf16;
    head_dim 64 or 128.  k_scale / v_scale: float32 device tensors [num_heads_kv], one scale per kv head, None = 1.0.
    The new token is stored as q8(x / scale) and attends through that stored value.  Returns `o`."""
    return _decode_op("", "_kv8", qkv, q_bias, k_bias, v_bias, k_cache_table, v_cache_table, seq_len, o, batch_size,
                      memory_max_len, num_heads, head_dim, rotary_embedding_dim, max_input_length, num_layer, idx_layer,
                      num_splits, rotary_cos_table, rotary_sin_table, softmax_scale, kv_layout, block_table, num_heads_kv,
                      k_scale=k_scale, v_scale=v_scale)


def flash_decode_kv8_window(qkv, q_bias, k_bias, v_bias, k_cache_table, v_cache_table, seq_len, o,
                            batch_size, memory_max_len, num_heads, head_dim, rotary_embedding_dim,
                            max_input_length, num_layer, idx_layer, window, *, num_splits=0,
                            rotary_cos_table=None, rotary_sin_table=None, softmax_scale=None, kv_layout="blmhd",
                            block_table=None, num_heads_kv=None, k_scale=None, v_scale=None):
    """flash_decode_kv8 with a sliding window (include/star_flash_attn.h, sfa_decode_kv8_window): the new token at
    position pos = seq_len[b] is stored as q8(x / scale) and attends, through that stored value, to itself and the
    window - 1 rows of the fp8 cache before it, lo = max(0, pos + 1 - window) .. pos.  window >= 1; the caches, the scales
    and every other argument as in flash_decode_kv8.  Cache rows below lo, and block_table entries of pages wholly below
    lo, are never read.  Returns `o`."""
    return _decode_op("", "_kv8_window", qkv, q_bias, k_bias, v_bias, k_cache_table, v_cache_table, seq_len, o, batch_size,
                      memory_max_len, num_heads, head_dim, rotary_embedding_dim, max_input_length, num_layer, idx_layer,
                      num_splits, rotary_cos_table, rotary_sin_table, softmax_scale, kv_layout, block_table, num_heads_kv,
                      window=window, k_scale=k_scale, v_scale=v_scale)


def quantize_kv8(src, scale=None, out=None):
    """16-bit cache rows -> e4m3 bytes (include/star_flash_attn.h, sfa_kv8_quantize): out[r, h, d] = q8(src[r, h, d] /
    scale[h]).  src is a [rows, Hkv, D] fp16 / bf16 view with any row and head strides that are multiples of 16
    elements and a contiguous last axis (a (sequence, layer) slice of either contiguous cache layout, or a page); out
    is such a view of a torch.uint8 / torch.float8_e4m3fn cache (None: a new contiguous uint8 tensor); scale a float32
    [Hkv] device tensor or None = 1.0.  Returns `out`."""
    lib = _lib.load()
    _require(isinstance(src, torch.Tensor) and src.is_cuda and src.dtype in _DTYPES and src.dim() == 3,
             "src must be a [rows, Hkv, D] float16 or bfloat16 tensor on a HIP device")
    rows, Hkv, D = (int(x) for x in src.shape)
    dev = src.device
    if out is None:
        out = torch.empty((rows, Hkv, D), dtype=torch.uint8, device=dev)
    _require(isinstance(out, torch.Tensor) and out.dtype in _KV8_DTYPES and out.device == dev and
             tuple(out.shape) == (rows, Hkv, D), f"out must be a uint8 or float8_e4m3fn tensor of shape {(rows, Hkv, D)} on {dev}")
    _require(src.stride(2) == 1 and out.stride(2) == 1, "the last axis of src and out must be contiguous")
    sc = _kv8_scale(scale, "scale", Hkv, dev)
    if rows == 0:
        return out
    with torch.cuda.device(dev):
        _lib.check(lib.sfa_kv8_quantize(ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(src.data_ptr()), sc, rows, Hkv, D,
                                        src.stride(0), src.stride(1), out.stride(0), out.stride(1), _DTYPES[src.dtype],
                                        _stream_ptr(dev)))
    return out


def flash_decode_chunk(qkv, q_bias, k_bias, v_bias, k_cache_table, v_cache_table, seq_len, o,
                       batch_size, memory_max_len, num_heads, head_dim, rotary_embedding_dim,
                       max_input_length, num_layer, idx_layer, *, num_splits=0,
                       rotary_cos_table=None, rotary_sin_table=None, softmax_scale=None, kv_layout="blmhd",
                       block_table=None, num_heads_kv=None):
    """n new tokens per sequence in one call (include/star_flash_attn.h, sfa_decode_chunk): the same arguments as
    flash_decode and the result of n successive flash_decode calls.  qkv is [B, n, 3, H, D] (grouped queries:
    [B, n, H + 2*num_heads_kv, D]), o is [B, n, H, D]; n = qkv.shape[1].  Token t of sequence b is rotated at and
    appended to position seq_len[b] + t and attends to the cache rows [0, seq_len[b] + t].  seq_len is not
    incremented.  Ragged prompts: flash_decode_varlen, or pad to a common n (the rows past a sequence's real length are overwritten by the
    decode steps that follow, before anything reads them).  Returns `o`."""
    return _decode_op("_chunk", "", qkv, q_bias, k_bias, v_bias, k_cache_table, v_cache_table, seq_len, o, batch_size,
                      memory_max_len, num_heads, head_dim, rotary_embedding_dim, max_input_length, num_layer, idx_layer,
                      num_splits, rotary_cos_table, rotary_sin_table, softmax_scale, kv_layout, block_table, num_heads_kv)


def flash_decode_varlen(qkv, q_bias, k_bias, v_bias, k_cache_table, v_cache_table, seq_len, o, cu_tokens,
                        batch_size, memory_max_len, num_heads, head_dim, rotary_embedding_dim,
                        max_input_length, num_layer, idx_layer, *, num_splits=0,
                        rotary_cos_table=None, rotary_sin_table=None, softmax_scale=None, kv_layout="blmhd",
                        block_table=None, num_heads_kv=None):
    """A ragged batch of new tokens in one call (include/star_flash_attn.h, sfa_decode_varlen): flash_decode_chunk
    with a token count of its own per sequence.  cu_tokens is an int32 device tensor [B + 1], starting at 0 and
    non-decreasing; sequence b owns the packed rows [cu_tokens[b], cu_tokens[b+1]) of qkv ([T, 3, H, D]; grouped
    queries: [T, H + 2*num_heads_kv, D]) and o ([T, H, D]), T = qkv.shape[0] >= cu_tokens[B].  Row cu_tokens[b] + t is
    rotated at and appended to position seq_len[b] + t and attends to the cache rows [0, seq_len[b] + t]; a sequence
    with no tokens takes no part, and no cache row past a sequence's own tokens is written.  cu_tokens is only read
    on the device (no synchronisation; graph replays may change it).  seq_len is not incremented.  Returns `o`."""
    return _decode_op("_varlen", "", qkv, q_bias, k_bias, v_bias, k_cache_table, v_cache_table, seq_len, o, batch_size,
                      memory_max_len, num_heads, head_dim, rotary_embedding_dim, max_input_length, num_layer, idx_layer,
                      num_splits, rotary_cos_table, rotary_sin_table, softmax_scale, kv_layout, block_table, num_heads_kv,
                      cu_tokens=cu_tokens)


def flash_decode_chunk_kv8(qkv, q_bias, k_bias, v_bias, k_cache_table, v_cache_table, seq_len, o,
                           batch_size, memory_max_len, num_heads, head_dim, rotary_embedding_dim,
                           max_input_length, num_layer, idx_layer, *, num_splits=0,
                           rotary_cos_table=None, rotary_sin_table=None, softmax_scale=None, kv_layout="blmhd",
                           block_table=None, num_heads_kv=None, k_scale=None, v_scale=None):
    """flash_decode_chunk over an fp8 KV cache (include/star_flash_attn.h, sfa_decode_chunk_kv8): the result of n
    successive flash_decode_kv8 calls.  The caches are torch.uint8 or torch.float8_e4m3fn tensors, k_scale / v_scale
    float32 device tensors [num_heads_kv] or None = 1.0, as in flash_decode_kv8; every other argument as in
    flash_decode_chunk.  Token t is stored at row seq_len[b] + t as q8(x / scale) and attends to the rows
    [0, seq_len[b] + t] of the cache after the append, the new rows through their stored values.  Returns `o`."""
    return _decode_op("_chunk", "_kv8", qkv, q_bias, k_bias, v_bias, k_cache_table, v_cache_table, seq_len, o, batch_size,
                      memory_max_len, num_heads, head_dim, rotary_embedding_dim, max_input_length, num_layer, idx_layer,
                      num_splits, rotary_cos_table, rotary_sin_table, softmax_scale, kv_layout, block_table, num_heads_kv,
                      k_scale=k_scale, v_scale=v_scale)


def flash_decode_varlen_kv8(qkv, q_bias, k_bias, v_bias, k_cache_table, v_cache_table, seq_len, o, cu_tokens,
                            batch_size, memory_max_len, num_heads, head_dim, rotary_embedding_dim,
                            max_input_length, num_layer, idx_layer, *, num_splits=0,
                            rotary_cos_table=None, rotary_sin_table=None, softmax_scale=None, kv_layout="blmhd",
                            block_table=None, num_heads_kv=None, k_scale=None, v_scale=None):
    """flash_decode_varlen over an fp8 KV cache (include/star_flash_attn.h, sfa_decode_varlen_kv8): every packed token
    gets what flash_decode_chunk_kv8 gives it at pos = seq_len[b].  The caches and the scales as in flash_decode_kv8,
    every other argument as in flash_decode_varlen.  Returns `o`."""
    return _decode_op("_varlen", "_kv8", qkv, q_bias, k_bias, v_bias, k_cache_table, v_cache_table, seq_len, o, batch_size,
                      memory_max_len, num_heads, head_dim, rotary_embedding_dim, max_input_length, num_layer, idx_layer,
                      num_splits, rotary_cos_table, rotary_sin_table, softmax_scale, kv_layout, block_table, num_heads_kv,
                      cu_tokens=cu_tokens, k_scale=k_scale, v_scale=v_scale)


def flash_decode_chunk_window(qkv, q_bias, k_bias, v_bias, k_cache_table, v_cache_table, seq_len, o,
                              batch_size, memory_max_len, num_heads, head_dim, rotary_embedding_dim,
                              max_input_length, num_layer, idx_layer, window, *, num_splits=0,
                              rotary_cos_table=None, rotary_sin_table=None, softmax_scale=None, kv_layout="blmhd",
                              block_table=None, num_heads_kv=None):
    """flash_decode_chunk with a sliding window (include/star_flash_attn.h, sfa_decode_chunk_window): the result of n
    successive flash_decode_window calls.  Token t of sequence b, at position seq_len[b] + t, attends to the rows
    [max(0, seq_len[b] + t + 1 - window), seq_len[b] + t].  window >= 1; every other argument as in flash_decode_chunk.
    Cache rows below lo_0 = max(0, seq_len[b] + 1 - window), and block_table entries of pages wholly below lo_0, are
    never read.  Returns `o`."""
    return _decode_op("_chunk", "_window", qkv, q_bias, k_bias, v_bias, k_cache_table, v_cache_table, seq_len, o, batch_size,
                      memory_max_len, num_heads, head_dim, rotary_embedding_dim, max_input_length, num_layer, idx_layer,
                      num_splits, rotary_cos_table, rotary_sin_table, softmax_scale, kv_layout, block_table, num_heads_kv,
                      window=window)


def flash_decode_varlen_window(qkv, q_bias, k_bias, v_bias, k_cache_table, v_cache_table, seq_len, o, cu_tokens,
                               batch_size, memory_max_len, num_heads, head_dim, rotary_embedding_dim,
                               max_input_length, num_layer, idx_layer, window, *, num_splits=0,
                               rotary_cos_table=None, rotary_sin_table=None, softmax_scale=None, kv_layout="blmhd",
                               block_table=None, num_heads_kv=None):
    """flash_decode_varlen with a sliding window (include/star_flash_attn.h, sfa_decode_varlen_window): every packed
    token gets what flash_decode_chunk_window gives it at pos = seq_len[b].  window >= 1; every other argument as in
    flash_decode_varlen.  Returns `o`."""
    return _decode_op("_varlen", "_window", qkv, q_bias, k_bias, v_bias, k_cache_table, v_cache_table, seq_len, o, batch_size,
                      memory_max_len, num_heads, head_dim, rotary_embedding_dim, max_input_length, num_layer, idx_layer,
                      num_splits, rotary_cos_table, rotary_sin_table, softmax_scale, kv_layout, block_table, num_heads_kv,
                      cu_tokens=cu_tokens, window=window)


def flash_decode_chunk_kv8_window(qkv, q_bias, k_bias, v_bias, k_cache_table, v_cache_table, seq_len, o,
                                  batch_size, memory_max_len, num_heads, head_dim, rotary_embedding_dim,
                                  max_input_length, num_layer, idx_layer, window, *, num_splits=0,
                                  rotary_cos_table=None, rotary_sin_table=None, softmax_scale=None, kv_layout="blmhd",
                                  block_table=None, num_heads_kv=None, k_scale=None, v_scale=None):
    """flash_decode_chunk_kv8 with a sliding window (include/star_flash_attn.h, sfa_decode_chunk_kv8_window): the result
    of n successive flash_decode_kv8_window calls.  Token t is stored at row seq_len[b] + t as q8(x / scale) and attends
    to the rows [max(0, seq_len[b] + t + 1 - window), seq_len[b] + t] of the cache after the append, the new rows through
    their stored values.  window >= 1; the caches and the scales as in flash_decode_kv8, every other argument as in
    flash_decode_chunk.  Cache rows below lo_0 = max(0, seq_len[b] + 1 - window), and block_table entries of pages wholly
    below lo_0, are never read.  Returns `o`."""
    return _decode_op("_chunk", "_kv8_window", qkv, q_bias, k_bias, v_bias, k_cache_table, v_cache_table, seq_len, o, batch_size,
                      memory_max_len, num_heads, head_dim, rotary_embedding_dim, max_input_length, num_layer, idx_layer,
                      num_splits, rotary_cos_table, rotary_sin_table, softmax_scale, kv_layout, block_table, num_heads_kv,
                      window=window, k_scale=k_scale, v_scale=v_scale)


def flash_decode_varlen_kv8_window(qkv, q_bias, k_bias, v_bias, k_cache_table, v_cache_table, seq_len, o, cu_tokens,
                                   batch_size, memory_max_len, num_heads, head_dim, rotary_embedding_dim,
                                   max_input_length, num_layer, idx_layer, window, *, num_splits=0,
                                   rotary_cos_table=None, rotary_sin_table=None, softmax_scale=None, kv_layout="blmhd",
                                   block_table=None, num_heads_kv=None, k_scale=None, v_scale=None):
    """flash_decode_varlen_kv8 with a sliding window (include/star_flash_attn.h, sfa_decode_varlen_kv8_window): every
    packed token gets what flash_decode_chunk_kv8_window gives it at pos = seq_len[b].  window >= 1; the caches and the
    scales as in flash_decode_kv8, every other argument as in flash_decode_varlen.  Returns `o`."""
    return _decode_op("_varlen", "_kv8_window", qkv, q_bias, k_bias, v_bias, k_cache_table, v_cache_table, seq_len, o, batch_size,
                      memory_max_len, num_heads, head_dim, rotary_embedding_dim, max_input_length, num_layer, idx_layer,
                      num_splits, rotary_cos_table, rotary_sin_table, softmax_scale, kv_layout, block_table, num_heads_kv,
                      cu_tokens=cu_tokens, window=window, k_scale=k_scale, v_scale=v_scale)


def flash_decode_window_sinks(qkv, q_bias, k_bias, v_bias, k_cache_table, v_cache_table, seq_len, o,
                              batch_size, memory_max_len, num_heads, head_dim, rotary_embedding_dim,
                              max_input_length, num_layer, idx_layer, window, sinks, *, num_splits=0,
                              rotary_cos_table=None, rotary_sin_table=None, softmax_scale=None, kv_layout="blmhd",
                              block_table=None, num_heads_kv=None):
    """flash_decode_window with attention sinks (include/star_flash_attn.h, sfa_decode_window_sinks): sinks[h], a float32
    device tensor [num_heads], is one more logit in query head h's softmax with a zero value row; it is not multiplied by
    the softmax scale.  sinks=None is flash_decode_window; window >= memory_max_len is full attention with sinks.  Every
    other argument as in flash_decode_window.  Returns `o`."""
    return _decode_op("", "_window_sinks", qkv, q_bias, k_bias, v_bias, k_cache_table, v_cache_table, seq_len, o, batch_size,
                      memory_max_len, num_heads, head_dim, rotary_embedding_dim, max_input_length, num_layer, idx_layer,
                      num_splits, rotary_cos_table, rotary_sin_table, softmax_scale, kv_layout, block_table, num_heads_kv,
                      window=window, sinks=sinks)


def flash_decode_chunk_window_sinks(qkv, q_bias, k_bias, v_bias, k_cache_table, v_cache_table, seq_len, o,
                                    batch_size, memory_max_len, num_heads, head_dim, rotary_embedding_dim,
                                    max_input_length, num_layer, idx_layer, window, sinks, *, num_splits=0,
                                    rotary_cos_table=None, rotary_sin_table=None, softmax_scale=None, kv_layout="blmhd",
                                    block_table=None, num_heads_kv=None):
    """flash_decode_chunk_window with attention sinks (include/star_flash_attn.h, sfa_decode_chunk_window_sinks): the
    result of n successive flash_decode_window_sinks calls.  sinks: float32 device tensor [num_heads] or None
    (= flash_decode_chunk_window); every other argument as in flash_decode_chunk_window.  Returns `o`."""
    return _decode_op("_chunk", "_window_sinks", qkv, q_bias, k_bias, v_bias, k_cache_table, v_cache_table, seq_len, o, batch_size,
                      memory_max_len, num_heads, head_dim, rotary_embedding_dim, max_input_length, num_layer, idx_layer,
                      num_splits, rotary_cos_table, rotary_sin_table, softmax_scale, kv_layout, block_table, num_heads_kv,
                      window=window, sinks=sinks)


def flash_decode_varlen_window_sinks(qkv, q_bias, k_bias, v_bias, k_cache_table, v_cache_table, seq_len, o, cu_tokens,
                                     batch_size, memory_max_len, num_heads, head_dim, rotary_embedding_dim,
                                     max_input_length, num_layer, idx_layer, window, sinks, *, num_splits=0,
                                     rotary_cos_table=None, rotary_sin_table=None, softmax_scale=None,
                                     kv_layout="blmhd", block_table=None, num_heads_kv=None):
    """flash_decode_varlen_window with attention sinks (include/star_flash_attn.h, sfa_decode_varlen_window_sinks): every
    packed token gets what flash_decode_chunk_window_sinks gives it at pos = seq_len[b].  sinks: float32 device tensor
    [num_heads] or None (= flash_decode_varlen_window); every other argument as in flash_decode_varlen_window.
    Returns `o`."""
    return _decode_op("_varlen", "_window_sinks", qkv, q_bias, k_bias, v_bias, k_cache_table, v_cache_table, seq_len, o, batch_size,
                      memory_max_len, num_heads, head_dim, rotary_embedding_dim, max_input_length, num_layer, idx_layer,
                      num_splits, rotary_cos_table, rotary_sin_table, softmax_scale, kv_layout, block_table, num_heads_kv,
                      cu_tokens=cu_tokens, window=window, sinks=sinks)


def flash_decode_kv8_window_sinks(qkv, q_bias, k_bias, v_bias, k_cache_table, v_cache_table, seq_len, o,
                                  batch_size, memory_max_len, num_heads, head_dim, rotary_embedding_dim,
                                  max_input_length, num_layer, idx_layer, window, sinks, *, num_splits=0,
                                  rotary_cos_table=None, rotary_sin_table=None, softmax_scale=None, kv_layout="blmhd",
                                  block_table=None, num_heads_kv=None, k_scale=None, v_scale=None):
    """flash_decode_kv8_window with attention sinks (include/star_flash_attn.h, sfa_decode_kv8_window_sinks): sinks[h], a
    float32 device tensor [num_heads], is one more logit in query head h's softmax with a zero value row; it is multiplied
    neither by the softmax scale nor by k_scale.  sinks=None is flash_decode_kv8_window; window >= memory_max_len is full
    attention with sinks.  Every other argument as in flash_decode_kv8_window.  Returns `o`."""
    return _decode_op("", "_kv8_window_sinks", qkv, q_bias, k_bias, v_bias, k_cache_table, v_cache_table, seq_len, o, batch_size,
                      memory_max_len, num_heads, head_dim, rotary_embedding_dim, max_input_length, num_layer, idx_layer,
                      num_splits, rotary_cos_table, rotary_sin_table, softmax_scale, kv_layout, block_table, num_heads_kv,
                      window=window, sinks=sinks, k_scale=k_scale, v_scale=v_scale)


def flash_decode_chunk_kv8_window_sinks(qkv, q_bias, k_bias, v_bias, k_cache_table, v_cache_table, seq_len, o,
                                        batch_size, memory_max_len, num_heads, head_dim, rotary_embedding_dim,
                                        max_input_length, num_layer, idx_layer, window, sinks, *, num_splits=0,
                                        rotary_cos_table=None, rotary_sin_table=None, softmax_scale=None,
                                        kv_layout="blmhd", block_table=None, num_heads_kv=None, k_scale=None,
                                        v_scale=None):
    """flash_decode_chunk_kv8_window with attention sinks (include/star_flash_attn.h, sfa_decode_chunk_kv8_window_sinks):
    the result of n successive flash_decode_kv8_window_sinks calls.  sinks: float32 device tensor [num_heads] or None
    (= flash_decode_chunk_kv8_window); every other argument as in flash_decode_chunk_kv8_window.  Returns `o`."""
    return _decode_op("_chunk", "_kv8_window_sinks", qkv, q_bias, k_bias, v_bias, k_cache_table, v_cache_table, seq_len, o, batch_size,
                      memory_max_len, num_heads, head_dim, rotary_embedding_dim, max_input_length, num_layer, idx_layer,
                      num_splits, rotary_cos_table, rotary_sin_table, softmax_scale, kv_layout, block_table, num_heads_kv,
                      window=window, sinks=sinks, k_scale=k_scale, v_scale=v_scale)


def flash_decode_varlen_kv8_window_sinks(qkv, q_bias, k_bias, v_bias, k_cache_table, v_cache_table, seq_len, o,
                                         cu_tokens, batch_size, memory_max_len, num_heads, head_dim,
                                         rotary_embedding_dim, max_input_length, num_layer, idx_layer, window, sinks, *,
                                         num_splits=0, rotary_cos_table=None, rotary_sin_table=None, softmax_scale=None,
                                         kv_layout="blmhd", block_table=None, num_heads_kv=None, k_scale=None,
                                         v_scale=None):
    """flash_decode_varlen_kv8_window with attention sinks (include/star_flash_attn.h,
    sfa_decode_varlen_kv8_window_sinks): every packed token gets what flash_decode_chunk_kv8_window_sinks gives it at
    pos = seq_len[b].  sinks: float32 device tensor [num_heads] or None (= flash_decode_varlen_kv8_window); every other
    argument as in flash_decode_varlen_kv8_window.  Returns `o`."""
    return _decode_op("_varlen", "_kv8_window_sinks", qkv, q_bias, k_bias, v_bias, k_cache_table, v_cache_table, seq_len, o, batch_size,
                      memory_max_len, num_heads, head_dim, rotary_embedding_dim, max_input_length, num_layer, idx_layer,
                      num_splits, rotary_cos_table, rotary_sin_table, softmax_scale, kv_layout, block_table, num_heads_kv,
                      cu_tokens=cu_tokens, window=window, sinks=sinks, k_scale=k_scale, v_scale=v_scale)


def check_decode_status(device=None):
    """Synchronise the current stream and raise if any decode call on it saw a bad seq_len."""
    lib = _lib.load()
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else device
    key = (device.index, torch.cuda.current_stream(device).cuda_stream)
    ws = _workspaces.get(key)
    if ws is None:
        return
    with torch.cuda.device(device):
        st = lib.sfa_decode_poll_status(ctypes.c_void_p(ws.data_ptr()), _stream_ptr(device))
        if st != _lib.SFA_OK:
            lib.sfa_decode_reset_status(ctypes.c_void_p(ws.data_ptr()), _stream_ptr(device))
        _lib.check(st)


def _prefill_args(q, k, v, out, return_lse, softmax_scale):
    """The checks and the sfa_prefill_args of flash_attn_fwd and flash_attn_window_fwd: (args, out, lse, device)"""
    _require(isinstance(q, torch.Tensor) and q.dtype in _DTYPES,
             f"q must be float16 or bfloat16 (got {getattr(q, 'dtype', type(q))})")
    dt, dev = q.dtype, q.device
    for name, t in (("q", q), ("k", k), ("v", v)):
        _require(t.is_cuda and t.device == dev, f"{name} must be on {dev}")
        _require(t.dtype == dt, f"{name} dtype {t.dtype} != {dt}")
        _require(t.dim() == 4, f"{name} must be [batch, heads, seq, head_dim]")
        _require(t.stride(3) == 1, f"{name}: head_dim must be contiguous")
    B, Hq, Sq, D = q.shape
    _require(k.shape == v.shape and k.shape[0] == B and k.shape[3] == D,
             f"k/v shapes {tuple(k.shape)}/{tuple(v.shape)} do not match q {tuple(q.shape)}")
    Hkv, Sk = k.shape[1], k.shape[2]
    if out is None:
        out = torch.empty((B, Hq, Sq, D), dtype=dt, device=dev)
    else:
        _require(out.shape == q.shape and out.dtype == dt and out.device == dev and out.stride(3) == 1,
                 "out must match q in shape/dtype/device with contiguous head_dim")
    lse = torch.empty((B, Hq, Sq), dtype=torch.float32, device=dev) if return_lse else None
    a = _lib.PrefillArgs()
    a.q, a.k, a.v, a.o = q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr()
    a.lse = lse.data_ptr() if lse is not None else None
    a.batch, a.heads_q, a.heads_kv, a.seqlen_q, a.seqlen_k, a.head_dim = B, Hq, Hkv, Sq, Sk, D
    for dst, t in ((a.q_stride, q), (a.k_stride, k), (a.v_stride, v), (a.o_stride, out)):
        dst[0], dst[1], dst[2] = t.stride(0), t.stride(1), t.stride(2)
    a.softmax_scale = float(softmax_scale) if softmax_scale else 0.0
    a.dtype = _DTYPES[dt]
    return a, out, lse, dev


def flash_attn_fwd(q, k, v, causal=False, softmax_scale=None, out=None, return_lse=False, fast_scale=False):
    """O = softmax(mask(Q K^T * scale)) V.   q [B,Hq,Sq,D], k/v [B,Hkv,Sk,D] (batch/head/seq strides that are
    multiples of 8, D contiguous; at D 64 / 128 the seq stride of k and v is bounded, about 34 M elements -- the
    limits are in include/star_flash_attn.h), fp16 or bf16, D in {64,128,256}.  causal is bottom-right aligned.
    fast_scale=True (ignored with return_lse) allows the prescaled-Q kernels: ~5 % faster, the scale is
    folded into Q in 16 bit, so the score error grows with the logits (include/star_flash_attn.h)."""
    lib = _lib.load()
    a, out, lse, dev = _prefill_args(q, k, v, out, return_lse, softmax_scale)
    a.causal = 1 if causal else 0
    a.fast_scale = 1 if fast_scale else 0
    with torch.cuda.device(dev):
        _lib.check(lib.sfa_prefill_fwd(ctypes.byref(a), _stream_ptr(dev)))
    return (out, lse) if return_lse else out


def flash_attn_window_fwd(q, k, v, window, sinks=None, softmax_scale=None, out=None, return_lse=False):
    """flash_attn_fwd(causal=True) under a sliding window, with an optional attention sink per query head
    (sfa_prefill_window_fwd): row i with causal limit lim = i + (Sk - Sq) sees the keys max(0, lim + 1 - window) .. lim --
    flash-attn's window_size = (window - 1, 0) -- and its softmax counts one more element with logit sinks[h] (natural-log
    units, not scaled) and a zero value row.  window: an int >= 1 (>= Sk: the causal mask); sinks: None or a float32 [Hq]
    tensor on q's device; D in {64, 128}.  With return_lse the second result is log(exp(sinks[h]) + sum_j exp(s_j))."""
    lib = _lib.load()
    a, out, lse, dev = _prefill_args(q, k, v, out, return_lse, softmax_scale)
    W = _window_int(window)
    _require(W >= 1, f"window={window} must be >= 1")
    a.causal = 1
    a.fast_scale = 0
    with torch.cuda.device(dev):
        _lib.check(lib.sfa_prefill_window_fwd(ctypes.byref(a), W, _sinks_ptr(sinks, q.shape[1], dev), _stream_ptr(dev)))
    return (out, lse) if return_lse else out


def prefill_auto_splits(batch, heads_q, seqlen_q, seqlen_k, head_dim, causal=False):
    """sfa_prefill_auto_splits: the split count flash_attn_split_fwd(num_splits=0) picks for these shapes."""
    return _lib.load().sfa_prefill_auto_splits(batch, heads_q, seqlen_q, seqlen_k, head_dim, 1 if causal else 0)


def prefill_split_workspace_bytes(batch, heads_q, seqlen_q, seqlen_k, head_dim, causal=False, num_splits=0):
    """sfa_prefill_split_workspace_bytes: bytes of workspace flash_attn_split_fwd needs for num_splits (0: auto)."""
    return _lib.load().sfa_prefill_split_workspace_bytes(batch, heads_q, seqlen_q, seqlen_k, head_dim,
                                                         1 if causal else 0, int(num_splits))


def flash_attn_split_fwd(q, k, v, causal=False, num_splits=0, softmax_scale=None, out=None, return_lse=False,
                         fast_scale=False, workspace=None):
    """flash_attn_fwd with each q-tile's key range cut into num_splits chunks, one workgroup each, and a combine over
    the fp32 partials (sfa_prefill_split_fwd): for grids with fewer 256-row q-tiles than compute units -- a short query
    block against a long context.  Same o and lse as flash_attn_fwd; D in {64, 128}.  num_splits <= 0: the library's
    choice (prefill_auto_splits); a count that resolves to 1 is flash_attn_fwd's launch, bit for bit (fast_scale is
    honoured only there).  workspace: None takes the cached per-(device, stream) scratch; a uint8 tensor on q's device
    (prefill_split_workspace_bytes, 256-byte aligned) is passed as it is."""
    lib = _lib.load()
    a, out, lse, dev = _prefill_args(q, k, v, out, return_lse, softmax_scale)
    a.causal = 1 if causal else 0
    a.fast_scale = 1 if fast_scale else 0
    _require(isinstance(num_splits, int) and not isinstance(num_splits, bool), f"num_splits={num_splits!r} must be an int")
    B, Hq, Sq, D = q.shape
    if workspace is None:
        need = lib.sfa_prefill_split_workspace_bytes(B, Hq, Sq, k.shape[2], D, a.causal, num_splits)
        # behind the 256-byte status block of the decode calls, whose sticky word this call must not overwrite
        ws = _workspace(dev, _STATUS_BYTES + need)[_STATUS_BYTES:] if need else None
    else:
        _require(isinstance(workspace, torch.Tensor) and workspace.dtype == torch.uint8 and workspace.dim() == 1 and
                 workspace.is_contiguous(), "workspace must be a contiguous 1-d uint8 tensor")
        _require(workspace.is_cuda and workspace.device == dev, f"workspace must be on {dev}")
        ws = workspace
    with torch.cuda.device(dev):
        _lib.check(lib.sfa_prefill_split_fwd(ctypes.byref(a), num_splits,
                                             ctypes.c_void_p(ws.data_ptr()) if ws is not None else None,
                                             ws.numel() if ws is not None else 0, _stream_ptr(dev)))
    return (out, lse) if return_lse else out


def prefill_varlen_workspace_bytes(batch, total_q):
    """sfa_prefill_varlen_workspace_bytes: bytes of workspace flash_attn_varlen_fwd needs (the plan: 8 bytes per slot,
    total_q // 256 + batch slots, rounded up to 256)."""
    return _lib.load().sfa_prefill_varlen_workspace_bytes(int(batch), int(total_q))


def _prefill_varlen_args(q, k, v, cu_seqlens_q, cu_seqlens_k, causal, softmax_scale, out, return_lse, workspace,
                         window=None):
    """The checks and the sfa_prefill_varlen_args of flash_attn_varlen_fwd and flash_attn_varlen_window_fwd (window: the
    latter's, checked before anything needs a device): (lib, args, out, lse, workspace, device, window as an int)"""
    _require(isinstance(q, torch.Tensor) and q.dtype in _DTYPES,
             f"q must be float16 or bfloat16 (got {getattr(q, 'dtype', type(q))})")
    dt, dev = q.dtype, q.device
    for name, t in (("q", q), ("k", k), ("v", v)):
        _require(isinstance(t, torch.Tensor) and t.device == dev, f"{name} must be a tensor on {dev}")
        _require(t.dtype == dt, f"{name} dtype {t.dtype} != {dt}")
        _require(t.dim() == 3, f"{name} must be [tokens, heads, head_dim]")
        _require(t.stride(2) == 1, f"{name}: head_dim must be contiguous")
    Tq, Hq, D = (int(x) for x in q.shape)
    _require(k.shape == v.shape and k.shape[2] == D,
             f"k/v shapes {tuple(k.shape)}/{tuple(v.shape)} do not match q {tuple(q.shape)}")
    Tk, Hkv = int(k.shape[0]), int(k.shape[1])
    for name, t in (("cu_seqlens_q", cu_seqlens_q), ("cu_seqlens_k", cu_seqlens_k)):
        _require(isinstance(t, torch.Tensor), f"{name} must be a tensor")
        _require(t.dtype == torch.int32, f"{name} has dtype {t.dtype}, expected torch.int32")
        _require(t.device == dev, f"{name} is on {t.device}, expected {dev}")
        _require(t.dim() == 1 and t.numel() >= 1 and t.is_contiguous(), f"{name} must be a contiguous [batch + 1] tensor")
    _require(cu_seqlens_q.numel() == cu_seqlens_k.numel(),
             f"cu_seqlens_q has {cu_seqlens_q.numel()} entries, cu_seqlens_k {cu_seqlens_k.numel()}")
    B = cu_seqlens_q.numel() - 1
    if out is None:
        out = torch.empty((Tq, Hq, D), dtype=dt, device=dev)
    else:
        _require(isinstance(out, torch.Tensor) and out.shape == q.shape and out.dtype == dt and out.device == dev and
                 out.stride(2) == 1, "out must match q in shape/dtype/device with contiguous head_dim")
    if workspace is not None:
        _require(isinstance(workspace, torch.Tensor) and workspace.dtype == torch.uint8 and workspace.dim() == 1 and
                 workspace.is_contiguous(), "workspace must be a contiguous 1-d uint8 tensor")
        _require(workspace.device == dev, f"workspace must be on {dev}")
    W = None
    if window is not None:
        W = _window_int(window)
        _require(W >= 1, f"window={window} must be >= 1")
    _require(q.is_cuda, f"q must live on a HIP device (got {dev})")
    lib = _lib.load()
    lse = torch.empty((Hq, Tq), dtype=torch.float32, device=dev) if return_lse else None
    a = _lib.PrefillVarlenArgs()
    a.q, a.k, a.v, a.o = q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr()
    a.lse = lse.data_ptr() if lse is not None else None
    a.cu_seqlens_q, a.cu_seqlens_k = cu_seqlens_q.data_ptr(), cu_seqlens_k.data_ptr()
    a.batch, a.heads_q, a.heads_kv, a.total_q, a.total_k, a.head_dim = B, Hq, Hkv, Tq, Tk, D
    for dst, t in ((a.q_stride, q), (a.k_stride, k), (a.v_stride, v), (a.o_stride, out)):
        dst[0], dst[1] = t.stride(0), t.stride(1)
    a.softmax_scale = float(softmax_scale) if softmax_scale else 0.0
    a.causal = 1 if causal else 0
    a.dtype = _DTYPES[dt]
    if workspace is None:
        need = lib.sfa_prefill_varlen_workspace_bytes(B, Tq)
        # behind the 256-byte status block of the decode calls, whose sticky word this call must not overwrite
        ws = _workspace(dev, _STATUS_BYTES + need)[_STATUS_BYTES:] if need else None
    else:
        ws = workspace
    return lib, a, out, lse, ws, dev, W


def flash_attn_varlen_fwd(q, k, v, cu_seqlens_q, cu_seqlens_k, causal=False, softmax_scale=None, out=None,
                          return_lse=False, workspace=None):
    """flash_attn_fwd over packed sequences of different lengths (sfa_prefill_varlen_fwd).  q [Tq, Hq, D], k / v
    [Tk, Hkv, D] with token and head strides that are multiples of 8 (k and v: a token stride of at most 34087040
    elements) and D contiguous, fp16 or bf16, D in {64, 128}; cu_seqlens_q /
    cu_seqlens_k int32 [B + 1] tensors on q's device: sequence b owns the query rows [cu_q[b], cu_q[b+1]) and the key rows
    [cu_k[b], cu_k[b+1]) and gets what flash_attn_fwd gives for those rows alone (causal: bottom-right aligned per
    sequence).  The cu tensors are read on the device only (no synchronisation; a graph replay may change them); a
    sequence whose entries are not a range of the tensors is skipped, and rows of no sequence keep their contents.
    workspace: None takes the cached per-(device, stream) scratch; a uint8 tensor on q's device
    (prefill_varlen_workspace_bytes, 256-byte aligned) is passed as it is.  Returns out [Tq, Hq, D], with return_lse
    (out, lse [Hq, Tq])."""
    lib, a, out, lse, ws, dev, _ = _prefill_varlen_args(q, k, v, cu_seqlens_q, cu_seqlens_k, causal, softmax_scale, out,
                                                        return_lse, workspace)
    with torch.cuda.device(dev):
        _lib.check(lib.sfa_prefill_varlen_fwd(ctypes.byref(a), ctypes.c_void_p(ws.data_ptr()) if ws is not None else None,
                                              ws.numel() if ws is not None else 0, _stream_ptr(dev)))
    return (out, lse) if return_lse else out


def flash_attn_varlen_window_fwd(q, k, v, cu_seqlens_q, cu_seqlens_k, window, sinks=None, softmax_scale=None, out=None,
                                 return_lse=False, workspace=None):
    """flash_attn_varlen_fwd(causal=True) under a sliding window, with an optional attention sink per query head
    (sfa_prefill_varlen_window_fwd): sequence b gets what flash_attn_window_fwd gives for its rows alone -- row i with
    causal limit lim = i + (n_k - n_q) sees the keys max(0, lim + 1 - window) .. lim of its own sequence, and its softmax
    counts one more element with logit sinks[h] (natural-log units, not scaled) and a zero value row.  window: an int
    >= 1 (>= a sequence's n_k: the causal mask for it); sinks: None or a float32 [Hq] tensor on q's device; every other
    argument, the workspace included, as in flash_attn_varlen_fwd.  With return_lse the second result is
    log(exp(sinks[h]) + sum_j exp(s_j)), [Hq, Tq]."""
    lib, a, out, lse, ws, dev, W = _prefill_varlen_args(q, k, v, cu_seqlens_q, cu_seqlens_k, True, softmax_scale, out,
                                                        return_lse, workspace, window)
    with torch.cuda.device(dev):
        _lib.check(lib.sfa_prefill_varlen_window_fwd(ctypes.byref(a), W, _sinks_ptr(sinks, q.shape[1], dev),
                                                     ctypes.c_void_p(ws.data_ptr()) if ws is not None else None,
                                                     ws.numel() if ws is not None else 0, _stream_ptr(dev)))
    return (out, lse) if return_lse else out


def prefill_varlen_auto_splits(batch, heads_q, total_q, max_seqlen_k, head_dim, causal=False):
    """sfa_prefill_varlen_auto_splits: the split count flash_attn_varlen_split_fwd(num_splits=0) picks for these shapes."""
    return _lib.load().sfa_prefill_varlen_auto_splits(int(batch), int(heads_q), int(total_q), int(max_seqlen_k),
                                                      int(head_dim), 1 if causal else 0)


def prefill_varlen_split_workspace_bytes(batch, heads_q, total_q, max_seqlen_k, head_dim, num_splits=0):
    """sfa_prefill_varlen_split_workspace_bytes: bytes of workspace flash_attn_varlen_split_fwd needs for num_splits
    (0: auto): the plan, the item list and the fp32 partials."""
    return _lib.load().sfa_prefill_varlen_split_workspace_bytes(int(batch), int(heads_q), int(total_q), int(max_seqlen_k),
                                                                int(head_dim), int(num_splits))


def flash_attn_varlen_split_fwd(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_k, causal=False, num_splits=0,
                                softmax_scale=None, out=None, return_lse=False, workspace=None):
    """flash_attn_varlen_fwd with each q-tile's key range cut into num_splits chunks, one workgroup each, and a combine
    over the fp32 partials (sfa_prefill_varlen_split_fwd): for packed batches with fewer 256-row q-tiles than compute
    units -- a few query blocks against long prefixes.  Same o and lse as flash_attn_varlen_fwd.  max_seqlen_k: an int
    >= 1, the host's bound of the longest key range; a partition hint only (a longer sequence is still computed in full).
    num_splits <= 0: the library's choice (prefill_varlen_auto_splits); a count that resolves to 1 is
    flash_attn_varlen_fwd's launch, bit for bit.  workspace: None takes the cached per-(device, stream) scratch; a uint8
    tensor on q's device (prefill_varlen_split_workspace_bytes, 256-byte aligned) is passed as it is."""
    _require(isinstance(max_seqlen_k, int) and not isinstance(max_seqlen_k, bool),
             f"max_seqlen_k={max_seqlen_k!r} must be an int")
    _require(max_seqlen_k >= 1, f"max_seqlen_k={max_seqlen_k} must be >= 1")
    _require(isinstance(num_splits, int) and not isinstance(num_splits, bool), f"num_splits={num_splits!r} must be an int")
    lib, a, out, lse, ws, dev, _ = _prefill_varlen_args(q, k, v, cu_seqlens_q, cu_seqlens_k, causal, softmax_scale, out,
                                                        return_lse, workspace)
    if workspace is None:
        need = lib.sfa_prefill_varlen_split_workspace_bytes(a.batch, a.heads_q, a.total_q, max_seqlen_k, a.head_dim,
                                                            num_splits)
        # behind the 256-byte status block of the decode calls, whose sticky word this call must not overwrite
        ws = _workspace(dev, _STATUS_BYTES + need)[_STATUS_BYTES:] if need else None
    with torch.cuda.device(dev):
        _lib.check(lib.sfa_prefill_varlen_split_fwd(ctypes.byref(a), max_seqlen_k, num_splits,
                                                    ctypes.c_void_p(ws.data_ptr()) if ws is not None else None,
                                                    ws.numel() if ws is not None else 0, _stream_ptr(dev)))
    return (out, lse) if return_lse else out


def compute_rotary_table(max_seq_len, rot_dim, dtype=torch.float16, device="cuda"):
    lib = _lib.load()
    device = torch.device(device)
    cos = torch.empty((max_seq_len, rot_dim // 2), dtype=dtype, device=device)
    sin = torch.empty_like(cos)
    with torch.cuda.device(device):
        _lib.check(lib.sfa_compute_rotary_table(cos.data_ptr(), sin.data_ptr(), max_seq_len, rot_dim,
                                                _DTYPES[dtype], _stream_ptr(device)))
    return cos, sin


def fill_16bit(t, value):
    """t[...] = value for a contiguous fp16/bf16 tensor (init_half_array's job)."""
    lib = _lib.load()
    _require(t.is_cuda and t.is_contiguous() and t.dtype in _DTYPES, "fill_16bit: contiguous 16-bit HIP tensor")
    bits = torch.tensor([value], dtype=t.dtype).view(torch.int16).item() & 0xFFFF
    with torch.cuda.device(t.device):
        _lib.check(lib.sfa_fill_16bit(t.data_ptr(), bits, t.numel(), _stream_ptr(t.device)))
    return t
