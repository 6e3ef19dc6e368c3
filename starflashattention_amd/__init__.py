"""star_flash_attn for MI355X (gfx950): fused decode attention + prefill forward.

Thin host layer over libStarFlashAttention.so (HIP kernels behind the C ABI in
include/star_flash_attn.h).  No CPU fallback: importing the operators without the built
library raises.
"""
from .ops import (  # noqa: F401
    flash_decode, flash_decode_chunk, flash_decode_varlen, flash_decode_kv8, quantize_kv8, flash_decode_window,
    flash_decode_chunk_window, flash_decode_varlen_window, flash_decode_kv8_window, flash_decode_chunk_kv8,
    flash_decode_varlen_kv8, flash_decode_chunk_kv8_window, flash_decode_varlen_kv8_window, flash_decode_window_sinks,
    flash_decode_chunk_window_sinks, flash_decode_varlen_window_sinks, flash_decode_kv8_window_sinks,
    flash_decode_chunk_kv8_window_sinks, flash_decode_varlen_kv8_window_sinks, flash_attn_fwd,
    flash_attn_window_fwd, flash_attn_split_fwd, prefill_auto_splits, prefill_split_workspace_bytes,
    flash_attn_varlen_fwd, prefill_varlen_workspace_bytes, flash_attn_varlen_window_fwd,
    flash_attn_varlen_split_fwd, prefill_varlen_auto_splits, prefill_varlen_split_workspace_bytes,
    compute_rotary_table, fill_16bit, check_decode_status, set_sync_checks, release_workspaces,
)
from ._lib import SfaError, LIB_PATH, debug_set, debug_get, last_prefill_kernel  # noqa: F401

__version__ = "0.1.0"
