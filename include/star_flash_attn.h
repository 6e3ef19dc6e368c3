/*
 * star_flash_attn.h -- C ABI of libStarFlashAttention.so (MI355X / gfx950 build).
 *
 * This is the drop-in boundary for the reference's one hot path (fused decode
 * attention) plus the prefill forward the north-star adds.  Plain pointers and
 * sizes only: no torch / ATen types, no C++ in the signatures.  Every pointer
 * is a DEVICE pointer unless it says "host".  `stream` is a hipStream_t passed
 * as void* (NULL = the null stream).  All entry points are asynchronous on
 * `stream`, allocate nothing, never synchronise the device and are safe to
 * capture in a hipGraph.  They return SFA_OK or a negative sfa_status;
 * sfa_last_error() gives the message for the calling thread.
 *
 * Reference interfaces replaced (paths relative to the reference repo):
 *   sfa_decode                  <- run_flash_decoder<T>      src/flash_attn.h:7-8,  src/flash_attn.cu:937-1018
 *                                  (+ the two kernels it launches, cu:554-935)
 *   sfa_decode_args             <- Flash_decoder_input       src/params.h:10-51
 *                                  Flash_decoder_params      src/params.h:53-58
 *                                  Flash_decoder_buffers     src/params.h:60-68 (now `workspace`)
 *   sfa_compute_rotary_table    <- compute_rotary_table<T>   src/flash_attn.h:9-10, cu:512-538
 *   sfa_fill_16bit              <- init_half_array           src/flash_attn.h:11,   cu:493-510
 *   sfa_prefill_fwd             <- (no reference function; BASELINE.json configs 2,3,5)
 *   sfa_decode_chunk            <- (no reference function: prompt ingestion before the first decode step)
 *   sfa_decode_kv8              <- (no reference function: sfa_decode over an fp8 (e4m3) KV cache)
 *   sfa_kv8_quantize            <- (no reference function: 16-bit cache rows -> fp8 cache rows)
 *   sfa_decode_window           <- (no reference function: sfa_decode over the last `window` positions)
 *   sfa_decode_chunk_window     <- (no reference function: sfa_decode_chunk / sfa_decode_varlen with that window)
 *   sfa_decode_kv8_window       <- (no reference function: sfa_decode_kv8 over the last `window` positions)
 *   sfa_decode_chunk_kv8        <- (no reference function: sfa_decode_chunk / sfa_decode_varlen over an fp8 KV cache)
 *   sfa_decode_chunk_kv8_window <- (no reference function: those two calls with the sliding window)
 *   sfa_decode_window_sinks     <- (no reference function: the three windowed calls with an attention sink per head)
 *   sfa_decode_kv8_window_sinks <- (no reference function: the three windowed fp8 calls with that sink)
 *   sfa_prefill_window_fwd      <- (no reference function: sfa_prefill_fwd with a sliding window and attention sinks)
 *   sfa_prefill_split_fwd       <- (no reference function: sfa_prefill_fwd with each q-tile's key range split)
 *   sfa_prefill_varlen_fwd      <- (no reference function: sfa_prefill_fwd over packed sequences of different lengths)
 *   sfa_prefill_varlen_window_fwd <- (no reference function: sfa_prefill_varlen_fwd with a sliding window and sinks)
 *   sfa_prefill_varlen_split_fwd  <- (no reference function: sfa_prefill_varlen_fwd with each q-tile's key range split)
 * The Python-facing mha_fwd_cuda (src/flash_api.cpp:42-68) and the C++ template
 * surface (src/flash_attn.h) in this repo are thin layers over these symbols.
 */
#ifndef STAR_FLASH_ATTN_C_API_H_
#define STAR_FLASH_ATTN_C_API_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bumped whenever a struct below changes layout or an entry point changes meaning:
 *   2  kv_layout, fast_scale
 *   3  page_size / block_table / block_table_stride / num_pages / num_heads_kv appended to sfa_decode_args;
 *      a block_table entry outside the pool on the APPEND page now rejects the sequence; sfa_debug_set
 *   4  sfa_debug_get, sfa_decode_workspace_bytes_gqa added (nothing changed); sfa_decode_chunk and
 *      sfa_decode_chunk_workspace_bytes added later under the same version, with no layout or meaning change:
 *      callers detect them by symbol
 *      sfa_decode_kv8 and sfa_kv8_quantize (fp8 KV cache) added under the same version, beside an unchanged
 *      sfa_decode_args: callers detect these entry points by symbol
 *      sfa_decode_window and sfa_decode_window_workspace_bytes (sliding-window decode) added under the same version,
 *      beside an unchanged sfa_decode_args: callers detect them by symbol
 *      sfa_decode_chunk_window, sfa_decode_varlen_window and their _workspace_bytes functions (the sliding window in the
 *      multi-token calls) added under the same version, in the same way
 *      sfa_decode_kv8_window (the sliding window over an fp8 KV cache) added under the same version, in the same way
 *      sfa_decode_chunk_kv8 and sfa_decode_varlen_kv8 (the multi-token calls over an fp8 KV cache) added under the same
 *      version, in the same way; they have no sizing functions of their own
 *      sfa_decode_chunk_kv8_window and sfa_decode_varlen_kv8_window (the sliding window in the multi-token calls over an
 *      fp8 KV cache) added under the same version, in the same way; no sizing functions of their own either
 *      sfa_decode_window_sinks, sfa_decode_chunk_window_sinks and sfa_decode_varlen_window_sinks (attention sinks in the
 *      three windowed calls over 16-bit caches) added under the same version, in the same way; no sizing functions of
 *      their own either
 *      sfa_decode_kv8_window_sinks, sfa_decode_chunk_kv8_window_sinks and sfa_decode_varlen_kv8_window_sinks (attention
 *      sinks in the three windowed calls over an fp8 KV cache) added under the same version, in the same way; no sizing
 *      functions of their own either
 *      sfa_prefill_window_fwd (the prefill forward with a sliding window and attention sinks) added under the same
 *      version, beside an unchanged sfa_prefill_args: callers detect it by symbol; sfa_prefill_split_fwd (the prefill
 *      forward with a split key range), its sizing function and its auto rule likewise
 *      sfa_prefill_varlen_fwd (the prefill forward over packed sequences of different lengths) and its sizing function
 *      added under the same version with a struct of their own, sfa_prefill_varlen_args: callers detect them by symbol
 *      sfa_prefill_varlen_window_fwd (the packed prefill forward with a sliding window and attention sinks) added under
 *      the same version beside an unchanged sfa_prefill_varlen_args: callers detect it by symbol
 *      sfa_prefill_varlen_split_fwd (the packed prefill forward with a split key range), its sizing function and its auto
 *      rule added under the same version, in the same way */
#define SFA_ABI_VERSION 4

typedef enum sfa_status {
    SFA_OK = 0,
    SFA_ERR_NULL_POINTER = -1,   /* a required pointer is NULL                       */
    SFA_ERR_BAD_SHAPE = -2,      /* sizes/strides out of the supported range         */
    SFA_ERR_BAD_DTYPE = -3,
    SFA_ERR_UNSUPPORTED_HEAD_DIM = -4,
    SFA_ERR_WORKSPACE_TOO_SMALL = -5,
    SFA_ERR_LAUNCH = -6,         /* HIP reported a launch/runtime failure            */
    SFA_ERR_SEQ_LEN_RANGE = -7,  /* reported by sfa_decode_poll_status: some
                                    seq_len[b] was outside [0, memory_max_len)       */
    SFA_ERR_BLOCK_TABLE_RANGE = -8 /* reported by sfa_decode_poll_status: a block_table
                                    entry was outside [0, num_pages): nothing was stored through
                                    it and the outputs that depended on it are NaN            */
} sfa_status;

typedef enum sfa_dtype {
    SFA_DTYPE_FP16 = 0,          /* IEEE half  (the reference's only dtype)          */
    SFA_DTYPE_BF16 = 1
} sfa_dtype;

/* How the KV caches are laid out.  SFA_KV_BLMHD is the reference's documented layout
 * (src/params.h:22-25, examples/python/testFlashDecoder.py:115-116) and what mha_fwd_cuda /
 * run_flash_decoder use.  SFA_KV_BLHMD keeps every (batch, layer, head) contiguous -- the
 * head-major layout the reference's kernel indexes internally (src/flash_attn.cu:617-619) --
 * so one (b,h) streams a dense 2*M*D-byte region instead of 2*D-byte segments H*D*2 bytes apart. */
typedef enum sfa_kv_layout {
    SFA_KV_BLMHD = 0,            /* [batch, num_layer, memory_max_len, num_heads, head_dim] */
    SFA_KV_BLHMD = 1,            /* [batch, num_layer, num_heads, memory_max_len, head_dim] */
    SFA_KV_PAGED = 2             /* page pools [num_pages, num_layer, page_size, num_heads, head_dim]
                                    addressed through block_table (the reference only NAMES its
                                    cache pointers k_cache_table / v_cache_table, src/params.h:22-25):
                                    token t of sequence b lives in page block_table[b][t / page_size],
                                    row t % page_size.  memory_max_len = the capacity of one sequence
                                    (<= block_table_stride * page_size).                            */
} sfa_kv_layout;

/* ---- library ------------------------------------------------------------------ */
int sfa_abi_version(void);
const char *sfa_status_string(int status);
const char *sfa_last_error(void);            /* thread-local, never NULL            */

/* ---- decode: one new token per sequence, fused RoPE + KV append + split-KV ----- */
/*
 * Field order, names and meaning of the first block mirror Flash_decoder_input
 * (src/params.h:10-51) so a binding can fill it 1:1; the trailing fields replace
 * Flash_decoder_params / Flash_decoder_buffers.
 *
 * Semantics, for every (b, h):
 *   pos   = seq_len[b]                      tokens already cached, 0 <= pos < memory_max_len
 *   q,k,v = qkv[b, {0,1,2}, h, :] (+ bias)  16-bit, `stride` elements between batches
 *   q,k   = rope(q,k; pos)                  interleaved pairs (x[2j], x[2j+1]),
 *                                           angle pos * 10000^(-2j/rot_dim) for 2j < rot_dim,
 *                                           fp32 math, result rounded to the 16-bit dtype
 *   k_cache[b, idx_layer, pos, h, :] = k;  v_cache[b, idx_layer, pos, h, :] = v
 *   o[b, h, :] = softmax(q . K[0..pos]^T * head_dim_inv) . V[0..pos]     (fp32 accumulate)
 * Caches are [batch, num_layer, memory_max_len, num_heads, head_dim], contiguous
 * (kv_layout = SFA_KV_BLMHD), or head-major with kv_layout = SFA_KV_BLHMD.
 * seq_len is NOT incremented (caller's job, as in the reference).
 * Cache rows beyond pos (beyond pos + n - 1 for the calls that append n tokens), the other layers, and
 * block_table entries past the last page a sequence needs are never read and may hold anything.
 * A sequence whose seq_len is out of range -- or, with paged caches, whose
 * block_table entry for the page the new token goes to lies outside [0, num_pages) --
 * is left untouched in the caches, gets NaN in o[b] and raises the sticky status word
 * (see sfa_decode_poll_status).  A bad entry on a page that is only READ is not
 * dereferenced either (page 0 is read in its place), raises the same status and turns the
 * outputs of that sequence's affected heads into NaN.
 */
typedef struct sfa_decode_args {
    void *qkv;                      /* [batch, 3, num_heads, head_dim]                */
    const void *q_bias;             /* [num_heads, head_dim] or NULL                  */
    const void *k_bias;             /* [num_heads, head_dim] or NULL                  */
    const void *v_bias;             /* [num_heads, head_dim] or NULL                  */
    void *o;                        /* [batch, num_heads, head_dim]                   */
    const void *seq_len;            /* int32 [batch]                                  */
    void *k_cache_table;            /* see above; written at one row per sequence     */
    void *v_cache_table;
    const void *rotary_cos_table;   /* [memory_max_len, rot_dim/2] 16-bit, or NULL:   */
    const void *rotary_sin_table;   /*   NULL => cos/sin computed in-kernel in fp32   */
    int batch_size;
    int memory_max_len;
    int num_heads;
    int head_dim;                   /* 64, 128 or 256                                 */
    float head_dim_inv;             /* softmax scale; <= 0 => 1/sqrt(head_dim)        */
    int rotary_embedding_dim;       /* even, 0..head_dim                              */
    int max_input_length;           /* carried for interface parity; unused           */
    int stride;                     /* elements between qkv batches; 0 => 3*H*D       */
    int num_layer;
    int idx_layer;
    /* -- replaces Flash_decoder_params (kBlockN / kNThreads are internal now) -- */
    int num_splits;                 /* KV splits per (b,h); <= 0 => chosen by the library */
    int dtype;                      /* sfa_dtype                                      */
    /* -- replaces Flash_decoder_buffers -- */
    void *workspace;                /* >= sfa_decode_workspace_bytes(...), 256-B aligned */
    size_t workspace_bytes;
    int kv_layout;                  /* sfa_kv_layout; 0 = the reference's layout (ABI v2) */
    /* -- SFA_KV_PAGED only -- */
    int page_size;                  /* tokens per page: a power of two >= 16             */
    const void *block_table;        /* int32 [batch, block_table_stride] page numbers    */
    int block_table_stride;         /* entries per sequence, >= ceil(memory_max_len / page_size) */
    int num_pages;                  /* pages in each pool (bounds the table entries)     */
    /* -- grouped queries (no counterpart in the reference; 0 = num_heads) -- */
    int num_heads_kv;               /* kv heads; num_heads / num_heads_kv in {1, 2, 4, 8, 16}.  With
                                       num_heads_kv != num_heads: qkv is [batch, num_heads +
                                       2*num_heads_kv, head_dim] (q heads, k heads, v heads; default
                                       stride (num_heads + 2*num_heads_kv)*head_dim), k_bias / v_bias
                                       and the caches carry num_heads_kv heads, o and q_bias num_heads */
} sfa_decode_args;

/* Bytes of scratch sfa_decode needs for this shape (num_splits <= 0: the library's choice
 * for this shape, which is what sfa_decode will then use). Never 0: the first 256 bytes hold
 * the status word.  Grouped queries (num_heads_kv != num_heads): the library sizes its split
 * count by the KV-head count (one workgroup serves a whole group), so ask
 * sfa_decode_auto_splits(batch_size, num_heads_kv, ...) and pass that count here with num_heads. */
size_t sfa_decode_workspace_bytes(int batch_size, int num_heads, int head_dim,
                                  int memory_max_len, int num_splits);
/* The same for grouped queries: with num_splits <= 0 it sizes for the split count sfa_decode picks from the KV-head
 * count.  (A workspace sized with sfa_decode_workspace_bytes(..., 0) still works: sfa_decode then takes the largest
 * split count that fits it.) */
size_t sfa_decode_workspace_bytes_gqa(int batch_size, int num_heads, int num_heads_kv, int head_dim,
                                      int memory_max_len, int num_splits);
/* The split count the library picks for num_splits <= 0; num_heads = the KV-head count. */
int sfa_decode_auto_splits(int batch_size, int num_heads, int head_dim, int memory_max_len);
/* Zero the sticky status word (async). Call once after allocating a workspace. */
int sfa_decode_reset_status(void *workspace, void *stream);
/* Synchronises `stream`, reads the status word: SFA_OK, SFA_ERR_SEQ_LEN_RANGE or
 * SFA_ERR_BLOCK_TABLE_RANGE. */
int sfa_decode_poll_status(const void *workspace, void *stream);
int sfa_decode(const sfa_decode_args *args, void *stream);

/* ---- decode chunk: n new tokens per sequence in one call ------------------------- */
/*
 * Exactly n successive sfa_decode calls, for every b, h and t in [0, n):
 *   pos   = seq_len[b]                     NOT incremented (caller's job, as in sfa_decode)
 *   q,k,v = qkv[b, t, ...] (+ bias)        same head split as sfa_decode, grouped queries included
 *   q,k   = rope(q, k; pos + t)            sfa_decode's recipe (LUT row pos + t when tables are given)
 *   cache[b, idx_layer, pos + t] = k, v    every kv_layout
 *   o[b, t, h, :] = softmax(q . K[0 .. pos+t]^T * scale) . V[0 .. pos+t]      (fp32 accumulate)
 * so token t sees the history and the new tokens 0..t (causal within the chunk).
 * qkv is [batch, n, 3, num_heads, head_dim] (grouped: [batch, n, H + 2*Hkv, head_dim]); args->stride = elements
 * between batches (0 => n * qkv_token_stride), qkv_token_stride = elements between tokens (0 => (H + 2*Hkv) *
 * head_dim); args->o is [batch, n, num_heads, head_dim], contiguous.  Every other field of sfa_decode_args keeps its
 * sfa_decode meaning; head_dim 64 or 128 (256 returns SFA_ERR_UNSUPPORTED_HEAD_DIM).  num_tokens = 0 does nothing.
 * Ragged prompts: use sfa_decode_varlen (below), or pad every sequence to a common n.  The rows written past a sequence's real length land at
 * positions >= its next seq_len, so the following decode steps overwrite them before anything reads them, and
 * causality keeps the real tokens' outputs independent of the padding.  With a paged cache the table must map the
 * padded rows [pos, pos + n) to valid pages too.
 * Rejection, with the status word of sfa_decode (sfa_decode_poll_status): pos < 0 or pos + n > memory_max_len, or
 * (paged) a page covering [pos, pos + n) outside [0, num_pages), leaves sequence b's cache untouched, makes o[b] NaN
 * and raises SFA_ERR_SEQ_LEN_RANGE / SFA_ERR_BLOCK_TABLE_RANGE.  A bad entry on a page that is only read is not
 * dereferenced; it raises SFA_ERR_BLOCK_TABLE_RANGE and turns the outputs that may depend on it into NaN.
 * Workspace: the 256-byte status block, the rotated Q, then (split key range) fp32 partials;
 * sfa_decode_chunk_workspace_bytes sizes it (num_splits <= 0: the library's choice for this shape).
 */
int    sfa_decode_chunk(const sfa_decode_args *args, int num_tokens, int64_t qkv_token_stride, void *stream);
size_t sfa_decode_chunk_workspace_bytes(int batch_size, int num_heads, int num_heads_kv, int head_dim,
                                        int memory_max_len, int num_tokens, int num_splits);

/* ---- decode varlen: a ragged, packed batch of new tokens in one call -------------- */
/*
 * sfa_decode_chunk with a token count of its own for every sequence: a mix of prompt chunks, speculative verification
 * and plain decode in one call, with no padding.
 *   cu_tokens      device int32 [batch_size + 1], cu_tokens[0] = 0, non-decreasing: sequence b owns the packed rows
 *                  [cu_tokens[b], cu_tokens[b+1]) of qkv and o; n_b is their count.  Read on the device only: the call
 *                  allocates nothing, never synchronises, and a captured graph may be replayed with other contents.
 *   total_tokens   host value: the rows of qkv and o, >= cu_tokens[batch_size].  It sizes the grid and the workspace.
 *   qkv            [total_tokens, 3, num_heads, head_dim] (grouped: [total_tokens, H + 2*Hkv, head_dim]),
 *                  qkv_token_stride elements between tokens (0 => dense); args->stride must be 0
 *   o              [total_tokens, num_heads, head_dim], contiguous
 * Packed row cu_tokens[b] + t, t < n_b, is token t of sfa_decode_chunk at pos = seq_len[b]: rotated at pos + t,
 * appended to cache row pos + t (every kv_layout), attends to [0, pos + t]; bias, rotary tables, partial rotary,
 * grouped queries, fp16 / bf16 and head_dim 64 / 128 as there (256 returns SFA_ERR_UNSUPPORTED_HEAD_DIM).  seq_len is
 * not incremented.  total_tokens = 0 does nothing.
 * Per sequence:
 *   n_b == 0       the sequence takes no part: nothing of it is read or written, seq_len[b] is not looked at.
 *   otherwise      it needs 0 <= pos and pos + n_b <= memory_max_len, and (paged) valid pages for its own rows
 *                  [pos, pos + n_b) only.  No cache row at or past pos + n_b is written.
 *   rejected       (pos out of range, or an append page outside the pool): cache untouched, its n_b rows of o NaN,
 *                  SFA_ERR_SEQ_LEN_RANGE / SFA_ERR_BLOCK_TABLE_RANGE in the sticky status word, as sfa_decode_chunk.
 *                  A bad page that is only read behaves as in sfa_decode_chunk.
 *   bad cu_tokens  cu_tokens[b+1] < cu_tokens[b], cu_tokens[b] < 0 or cu_tokens[b+1] > total_tokens: the sequence is
 *                  skipped with nothing written (o included) and SFA_ERR_SEQ_LEN_RANGE is raised.
 * Workspace: the status block, the plan (one entry per attention workgroup slot, total_tokens * G / 256 + batch_size
 * of them), the rotated Q packed over tokens, then (split key range) fp32 partials.  sfa_decode_varlen_workspace_bytes
 * depends on total_tokens, not on how the tokens are spread over the sequences (num_splits <= 0: the library's choice).
 * The same workspace (status word) may serve sfa_decode and sfa_decode_chunk calls on the same stream.
 */
int    sfa_decode_varlen(const sfa_decode_args *args, const void *cu_tokens, int total_tokens,
                         int64_t qkv_token_stride, void *stream);
size_t sfa_decode_varlen_workspace_bytes(int batch_size, int num_heads, int num_heads_kv, int head_dim,
                                         int memory_max_len, int total_tokens, int num_splits);

/* ---- decode over an fp8 KV cache ---------------------------------------------------- */
/*
 * sfa_decode with caches of one byte per element.  Every field of args keeps its sfa_decode meaning, except:
 *   k_cache_table / v_cache_table   OCP e4m3 bytes (1-4-3, bias 7, max 448, no infinities, 0x7F / 0xFF = NaN: torch's
 *                  float8_e4m3fn), in the same three layouts; the row, head and page strides keep their values in
 *                  elements, which now are bytes.  16-byte aligned.
 *   dtype          still the dtype of qkv, the biases, the rotary tables and o: fp16 or bf16
 *   head_dim       64 or 128 (256 returns SFA_ERR_UNSUPPORTED_HEAD_DIM)
 *   k_scale, v_scale   device fp32 [num_heads_kv], 4-byte aligned, one scale per kv head; NULL = 1.0.  The scales must
 *                  be finite and > 0: they are device data, so this is the caller's contract and is not checked.
 * num_heads / num_heads_kv in {1, 2, 4, 8, 16}; paging, bias, partial rotary, the rotary tables and num_splits as in
 * sfa_decode.
 * Semantics, for every (b, h), hk = the kv head of h:
 *   k16, v16 = exactly what sfa_decode would have stored (bias, RoPE in fp32, rounded to the 16-bit dtype)
 *   k8 = q8(k16 / k_scale[hk]),  v8 = q8(v16 / v_scale[hk])     written at row pos; no other byte of a cache changes
 *   q8(x) = e4m3_rne(clamp(x, -448, 448)): IEEE fp32 division, saturating, ties to even, NaN stays NaN (0x7F)
 *   o = softmax(q16 . (k_scale[hk] * K8[0..pos])^T * head_dim_inv) . (v_scale[hk] * V8[0..pos])     (fp32 accumulate)
 * The new token takes part through its QUANTISED value: the output of a step is a function of the cache contents
 * after the step.
 * Rejection (pos out of range, a bad append page, a bad read page) behaves exactly as in sfa_decode: the same status
 * bits, NaN in o[b], nothing stored, a bad read page never dereferenced.
 * Workspace: the size and layout of sfa_decode_workspace_bytes_gqa; the same workspace and status word serve sfa_decode
 * and sfa_decode_kv8 calls (and the chunk / varlen calls) on the same stream.
 */
int sfa_decode_kv8(const sfa_decode_args *args, const float *k_scale, const float *v_scale, void *stream);

/*
 * 16-bit cache rows -> rows of an fp8 cache.  A prompt gets into an fp8 cache directly through sfa_decode_chunk_kv8 /
 * sfa_decode_varlen_kv8 (below).  The alternative this function serves: the prompt runs through sfa_decode_chunk /
 * sfa_decode_varlen on a 16-bit staging cache (one layer of it is enough) -- its tokens then attend through their 16-bit
 * values -- and its rows are quantised into the fp8 cache afterwards:
 *   dst[r*dst_row_stride + h*dst_head_stride + d] = q8(src[r*src_row_stride + h*src_head_stride + d] / scale[h])
 * for r < rows, h < num_heads_kv, d < head_dim (64 or 128); rows = 0 does nothing.  src holds `dtype` (fp16 / bf16)
 * elements, dst bytes.  Strides are in elements and multiples of 16, dst and src 16-byte aligned; scale is device fp32
 * [num_heads_kv] (finite, > 0, not checked) or NULL = 1.0.  One call covers a (sequence, layer) slice of either
 * contiguous layout, or one page.
 */
int sfa_kv8_quantize(void *dst, const void *src, const float *scale, int64_t rows, int num_heads_kv, int head_dim,
                     int64_t src_row_stride, int64_t src_head_stride,
                     int64_t dst_row_stride, int64_t dst_head_stride, int dtype, void *stream);

/* ---- decode with a sliding window --------------------------------------------------- */
/*
 * sfa_decode for a sliding-window attention layer.  Every field of args keeps its sfa_decode meaning: bias, RoPE at
 * pos = seq_len[b], the rotary tables, partial rotary, the append at row pos, fp16 / bf16, head_dim 64 / 128 / 256, the
 * three kv_layouts, num_heads / num_heads_kv in {1, 2, 4, 8, 16}, the rejection rules and the status word.  The only
 * difference is the key range.  With lo = max(0, pos + 1 - window):
 *   o[b, h, :] = softmax(q . K[lo..pos]^T * head_dim_inv) . V[lo..pos]
 * The token sees itself and the window - 1 rows before it (flash-attn's window_size = (window - 1, 0)).
 *   window >= 1     window < 1 returns SFA_ERR_BAD_SHAPE.  window = 1 attends to the new token only; window > pos for
 *                   every sequence is plain sfa_decode.
 * Cache rows are absolute positions (a ring-buffer cache is not supported).  What the window promises:
 *   - cache rows below lo are never read and may hold anything (as do the rows beyond pos and the other layers);
 *   - in a paged cache, a block_table entry whose page lies wholly below lo (entries [0, lo / page_size)) is never
 *     read and may hold any value, -1 included: a server may free those pages;
 *   - only a bad entry on a page that intersects [lo, pos] raises SFA_ERR_BLOCK_TABLE_RANGE (on the append page it
 *     rejects the sequence, on a read page it makes the affected outputs NaN, as in sfa_decode);
 *   - lo is computed on the device from seq_len: the call allocates nothing, never synchronises and may be captured
 *     in a graph and replayed with other seq_len contents.
 * Workspace: the layout of sfa_decode (the status block, then the fp32 partials).  With num_splits <= 0 the split
 * count is sfa_decode_auto_splits(batch_size, num_heads_kv, head_dim, min(window, memory_max_len)) -- sfa_decode's rule
 * over the rows a sequence can read, so a short window is not split -- and sfa_decode_window_workspace_bytes sizes for
 * that count.  A workspace sized by sfa_decode_workspace_bytes_gqa is never too small; one that holds fewer splits than
 * the library would pick gets the largest count it holds, as in sfa_decode.  The same workspace and status word serve
 * every decode entry point on a stream.
 */
int    sfa_decode_window(const sfa_decode_args *args, int window, void *stream);
size_t sfa_decode_window_workspace_bytes(int batch_size, int num_heads, int num_heads_kv, int head_dim,
                                         int memory_max_len, int window, int num_splits);

/* ---- multi-token decode with a sliding window -------------------------------------- */
/*
 * sfa_decode_chunk / sfa_decode_varlen for a sliding-window attention layer: the call gives exactly what n successive
 * sfa_decode_window calls would.  Everything of sfa_decode_chunk / sfa_decode_varlen holds unchanged: bias, RoPE at
 * pos + t, the append of all n rows, every kv_layout, grouped queries, fp16 / bf16, head_dim 64 / 128 (256 returns
 * SFA_ERR_UNSUPPORTED_HEAD_DIM), the cu_tokens rules, the rejection rules and the status word.  The only difference is
 * the key range: token t of a sequence at pos = seq_len[b] attends to the rows [lo_t, pos + t], with
 *   lo_t = max(0, pos + t + 1 - window).
 *   window >= 1     window < 1 returns SFA_ERR_BAD_SHAPE.  window = 1 leaves each token its own row only; when
 *                   window >= pos + n for every sequence the call is the plain chunk / varlen call, bit for bit.
 * What the window promises, with lo_0 = max(0, pos + 1 - window), the lower bound of the sequence's first token, and n
 * the sequence's token count:
 *   - cache rows below lo_0 are never read and may hold anything (as do the rows from pos + n on and the other layers);
 *   - in a paged cache the block_table entries [0, lo_0 / page_size) are never read and may hold any value, -1
 *     included: a server may free the pages wholly below the window before a multi-token step as well;
 *   - only a bad entry on a page that intersects [lo_0, pos + n) raises SFA_ERR_BLOCK_TABLE_RANGE, under the chunk
 *     call's two rules: on a page that covers new rows it rejects the sequence, on a page that is only read it makes
 *     the affected outputs NaN;
 *   - lo is computed on the device from seq_len (and cu_tokens): the call allocates nothing, never synchronises and may
 *     be captured in a graph and replayed with other contents.
 * Workspace: layout and status word are those of the chunk / varlen call.  With num_splits <= 0 the split count is that
 * call's own rule with min(memory_max_len, window - 1 + count) in place of memory_max_len, count = num_tokens /
 * total_tokens: the most rows a sequence can read, so a short window is not split into slivers.  The _workspace_bytes
 * functions size for that count.  The rule never grows with that argument, so a workspace sized by
 * sfa_decode_chunk_workspace_bytes / sfa_decode_varlen_workspace_bytes is never too small; one that holds fewer splits
 * than the library would pick gets the largest count it holds.  The split key range is the tiles that hold
 * [lo_0, pos + n), not [0, pos + n): a short window over a long history is shared by all splits.
 * Not served: head_dim 256, ring-buffer caches, soft-capping.  (An fp8 cache: sfa_decode_chunk_kv8_window /
 * sfa_decode_varlen_kv8_window, below.  Attention sinks: sfa_decode_window_sinks / sfa_decode_chunk_window_sinks /
 * sfa_decode_varlen_window_sinks, below, for these two calls and for sfa_decode_window.)
 */
int    sfa_decode_chunk_window(const sfa_decode_args *args, int num_tokens, int64_t qkv_token_stride, int window,
                               void *stream);
size_t sfa_decode_chunk_window_workspace_bytes(int batch_size, int num_heads, int num_heads_kv, int head_dim,
                                               int memory_max_len, int num_tokens, int window, int num_splits);
int    sfa_decode_varlen_window(const sfa_decode_args *args, const void *cu_tokens, int total_tokens,
                                int64_t qkv_token_stride, int window, void *stream);
size_t sfa_decode_varlen_window_workspace_bytes(int batch_size, int num_heads, int num_heads_kv, int head_dim,
                                                int memory_max_len, int total_tokens, int window, int num_splits);

/* ---- sliding-window decode with attention sinks ------------------------------------ */
/*
 * sfa_decode_window / sfa_decode_chunk_window / sfa_decode_varlen_window for a layer whose softmax carries a learned
 * per-head sink logit (gpt-oss: 64 query heads over 8 kv heads, head_dim 64, a 128-row window on every second layer).
 * Everything of the _window call each one extends holds unchanged: bias, RoPE, the append, the three kv_layouts,
 * num_heads / num_heads_kv in {1, 2, 4, 8, 16}, fp16 / bf16, head_dim 64 / 128 / 256 for the single-token call and
 * 64 / 128 for the other two (256 returns SFA_ERR_UNSUPPORTED_HEAD_DIM), the never-read promises below lo / lo_0, the
 * cu_tokens rules, the rejection rules and the status bits; the call allocates nothing, never synchronises and may be
 * captured in a graph.  A layer with full attention passes window >= memory_max_len (INT_MAX works); window < 1 returns
 * SFA_ERR_BAD_SHAPE.
 *   sinks           device fp32 [num_heads], one logit per QUERY head, 4-byte aligned (checked: otherwise
 *                   SFA_ERR_BAD_SHAPE).  Every value is finite or -inf (the caller's contract, not checked).  Read on
 *                   the device only: a replayed graph sees new contents.
 *                   NULL: the call validates under its own name and then launches exactly what the _window call
 *                   launches; output and caches are bit-identical to it.
 * Semantics, for query head h over its key range [lo, pos] (chunk / varlen: [lo_t, pos + t]), s_j = q . K_j * head_dim_inv:
 *   o[h] = sum_j exp(s_j) V_j / (exp(sinks[h]) + sum_j exp(s_j))
 * -- one more key with logit sinks[h] and a zero value row.  The sink is NOT multiplied by head_dim_inv.  The output is
 * a function of the sink and the cache after the call; the caches receive exactly what the _window call stores.
 * Numerics: the sink joins the online softmax once per query row, whatever the split count.  A sink far above the scores
 * gives a small finite output, with no overflow; a sink whose weight underflows in fp32 (-inf is one) gives the _window
 * call's output bit for bit at the same explicit num_splits.
 * Workspace: there are no sizing functions of their own.  Layout, split rule and status word are those of the _window
 * call each one extends, and sfa_decode_window_workspace_bytes / sfa_decode_chunk_window_workspace_bytes /
 * sfa_decode_varlen_window_workspace_bytes size it; with num_splits <= 0 a workspace that holds fewer splits than the
 * library would pick gets the largest count it holds.
 * Not served: head_dim 256 in the multi-token calls, ring-buffer caches, soft-capping.  (Sinks over an fp8 cache:
 * sfa_decode_kv8_window_sinks / sfa_decode_chunk_kv8_window_sinks / sfa_decode_varlen_kv8_window_sinks, below.)
 */
int sfa_decode_window_sinks(const sfa_decode_args *args, const float *sinks, int window, void *stream);
int sfa_decode_chunk_window_sinks(const sfa_decode_args *args, const float *sinks, int num_tokens,
                                  int64_t qkv_token_stride, int window, void *stream);
int sfa_decode_varlen_window_sinks(const sfa_decode_args *args, const float *sinks, const void *cu_tokens,
                                   int total_tokens, int64_t qkv_token_stride, int window, void *stream);

/* ---- decode with a sliding window over an fp8 KV cache ------------------------------ */
/*
 * sfa_decode_kv8 for a sliding-window attention layer: the conjunction of the contracts of sfa_decode_kv8 and
 * sfa_decode_window.
 * Everything of sfa_decode_kv8 holds unchanged: the caches are e4m3 bytes in the three layouts (strides in elements =
 * bytes, 16-byte aligned); dtype is the dtype of qkv, the biases, the rotary tables and o; head_dim 64 or 128 (256 returns
 * SFA_ERR_UNSUPPORTED_HEAD_DIM); k_scale / v_scale are device fp32 [num_heads_kv], 4-byte aligned, finite and > 0
 * (not checked), NULL = 1.0; the new token is stored at row pos as k8 = q8(k16 / k_scale[hk]), v8 = q8(v16 / v_scale[hk])
 * and attends through that quantised value; the rejection rules and the status word.
 * The only difference is the key range.  With lo = max(0, pos + 1 - window):
 *   o = softmax(q16 . (k_scale[hk] * K8[lo..pos])^T * head_dim_inv) . (v_scale[hk] * V8[lo..pos])     (fp32 accumulate)
 *   window >= 1     window < 1 returns SFA_ERR_BAD_SHAPE.  window = 1 attends to the (quantised) new token only; window >
 *                   pos for every sequence is sfa_decode_kv8, bit for bit, at the same explicit num_splits.
 * What the window promises is what sfa_decode_window promises:
 *   - cache rows below lo are never read and may hold anything, the NaN byte 0x7F included (as do the rows beyond pos
 *     and the other layers);
 *   - in a paged cache the block_table entries [0, lo / page_size) are never read and may hold any value, -1 included: a
 *     server may free those pages;
 *   - only a bad entry on a page that intersects [lo, pos] raises SFA_ERR_BLOCK_TABLE_RANGE (on the append page it
 *     rejects the sequence, on a read page it makes the affected outputs NaN);
 *   - lo is computed on the device from seq_len: the call allocates nothing, never synchronises and may be captured in
 *     a graph and replayed with other seq_len contents.
 * Workspace: there is no sizing function of its own.  Layout and split rule are sfa_decode_window's (num_splits <= 0:
 * sfa_decode_auto_splits(batch_size, num_heads_kv, head_dim, min(window, memory_max_len))), and
 * sfa_decode_window_workspace_bytes sizes it.  A workspace sized by sfa_decode_workspace_bytes_gqa is never too small;
 * with num_splits <= 0 one that holds fewer splits than the library would pick gets the largest count it holds.  The
 * same workspace and status word serve every decode entry point on a stream.
 * Not served: head_dim 256, per-token or per-block scales, ring-buffer caches, soft-capping.  (More than one token per
 * sequence: sfa_decode_chunk_kv8_window / sfa_decode_varlen_kv8_window, below.  Attention sinks:
 * sfa_decode_kv8_window_sinks, below.)
 */
int sfa_decode_kv8_window(const sfa_decode_args *args, const float *k_scale, const float *v_scale, int window,
                          void *stream);

/* ---- multi-token decode over an fp8 KV cache ---------------------------------------- */
/*
 * sfa_decode_chunk / sfa_decode_varlen over the e4m3 caches of sfa_decode_kv8: the call gives exactly what n successive
 * sfa_decode_kv8 calls would.  It is the conjunction of two contracts.
 * Everything of sfa_decode_chunk / sfa_decode_varlen holds unchanged: the qkv / o shapes and strides, bias, RoPE at
 * pos + t, the rotary tables, partial rotary, every kv_layout, num_heads / num_heads_kv in {1, 2, 4, 8, 16}, fp16 / bf16,
 * head_dim 64 / 128 (256 returns SFA_ERR_UNSUPPORTED_HEAD_DIM), the cu_tokens rules and n_b == 0, the rejection rules
 * and the status word; seq_len is not incremented; the call allocates nothing, never synchronises and may be captured
 * in a graph and replayed with other seq_len / cu_tokens contents.
 * Everything of sfa_decode_kv8 holds unchanged: the caches are e4m3 bytes in the three layouts (strides in elements =
 * bytes, 16-byte aligned); dtype is the dtype of qkv, the biases, the rotary tables and o; k_scale / v_scale are device
 * fp32 [num_heads_kv], 4-byte aligned (checked), finite and > 0 (not checked), NULL = 1.0.
 * Semantics, for token t of a sequence at pos = seq_len[b] and every kv head hk:
 *   k16, v16 = exactly what sfa_decode_chunk would have stored at row pos + t
 *   k8 = q8(k16 / k_scale[hk]),  v8 = q8(v16 / v_scale[hk])     written at row pos + t; no other byte of a cache changes
 *   o = softmax(q16 . (k_scale[hk] * K8[0..pos+t])^T * head_dim_inv) . (v_scale[hk] * V8[0..pos+t])    (fp32 accumulate)
 * over the cache AFTER the append: token t sees the new rows 0..t, its own included, through their quantised values,
 * so the output is a function of the cache bytes after the call.  (Through a 16-bit staging cache and sfa_kv8_quantize
 * the new tokens attend through their 16-bit values instead: n draft tokens verified that way do not get what n
 * sfa_decode_kv8 steps give them.)
 * Rows at and beyond pos + n, the other layers and spare pages are never read and may hold anything, the NaN byte 0x7F
 * included.
 * Workspace: there are no sizing functions of their own.  Layout, split rule and status word are those of
 * sfa_decode_chunk / sfa_decode_varlen, and sfa_decode_chunk_workspace_bytes / sfa_decode_varlen_workspace_bytes size
 * it.  (The split rule was tuned on 16-bit rows and has not been re-tuned for one-byte rows.)  The same workspace and
 * status word serve every decode entry point on a stream.
 * Not served: head_dim 256, per-token or per-block scales, fp8 matrix instructions on a quantised Q.  (A sliding
 * window: sfa_decode_chunk_kv8_window / sfa_decode_varlen_kv8_window, below.)
 */
int sfa_decode_chunk_kv8(const sfa_decode_args *args, const float *k_scale, const float *v_scale, int num_tokens,
                         int64_t qkv_token_stride, void *stream);
int sfa_decode_varlen_kv8(const sfa_decode_args *args, const float *k_scale, const float *v_scale,
                          const void *cu_tokens, int total_tokens, int64_t qkv_token_stride, void *stream);

/* ---- multi-token decode with a sliding window over an fp8 KV cache ----------------- */
/*
 * sfa_decode_chunk_kv8 / sfa_decode_varlen_kv8 for a sliding-window attention layer: the call gives exactly what n
 * successive sfa_decode_kv8_window calls would.  It is the conjunction of the contracts of sfa_decode_chunk_kv8 /
 * sfa_decode_varlen_kv8 and of sfa_decode_chunk_window / sfa_decode_varlen_window.
 * Everything of sfa_decode_chunk_kv8 / sfa_decode_varlen_kv8 holds unchanged: the qkv / o shapes and strides, bias, RoPE
 * at pos + t, the rotary tables, partial rotary, the three kv_layouts of e4m3 bytes (strides in elements = bytes, 16-byte
 * aligned), num_heads / num_heads_kv in {1, 2, 4, 8, 16}, fp16 / bf16, head_dim 64 / 128 (256 returns
 * SFA_ERR_UNSUPPORTED_HEAD_DIM); k_scale / v_scale are device fp32 [num_heads_kv], 4-byte aligned (checked: otherwise
 * SFA_ERR_BAD_SHAPE), finite and > 0 (not checked), NULL = 1.0; row pos + t receives k8 = q8(k16 / k_scale[hk]),
 * v8 = q8(v16 / v_scale[hk]) and no other byte of a cache changes; the cu_tokens rules and n_b == 0, the rejection rules
 * and the status word; seq_len is not incremented; the call allocates nothing, never synchronises and may be captured in
 * a graph and replayed with other seq_len / cu_tokens contents.
 * The only difference is the key range.  Token t of a sequence at pos = seq_len[b] attends to the rows [lo_t, pos + t] of
 * the cache AFTER the append, with lo_t = max(0, pos + t + 1 - window):
 *   o = softmax(q16 . (k_scale[hk] * K8[lo_t..pos+t])^T * head_dim_inv) . (v_scale[hk] * V8[lo_t..pos+t])  (fp32 accumulate)
 * The new rows, its own included, enter through their stored bytes.
 *   window >= 1     window < 1 returns SFA_ERR_BAD_SHAPE.  window = 1 leaves each token its own quantised row only; when
 *                   window >= pos + n for every sequence the call is sfa_decode_chunk_kv8 / sfa_decode_varlen_kv8, bit
 *                   for bit, at the same explicit num_splits.
 * What the window promises is what sfa_decode_chunk_window promises, with lo_0 = max(0, pos + 1 - window) and n the
 * sequence's token count; the cache being bytes, "anything" includes the NaN byte 0x7F:
 *   - cache rows below lo_0, rows from pos + n on and the other layers are never read and may hold anything;
 *   - in a paged cache the block_table entries [0, lo_0 / page_size) are never read and may hold any value, -1 included;
 *   - only a bad entry on a page that intersects [lo_0, pos + n) raises SFA_ERR_BLOCK_TABLE_RANGE: on a page that covers
 *     new rows it rejects the sequence, on a page that is only read it makes the affected outputs NaN.
 * Workspace: there are no sizing functions of their own.  Layout, split rule and status word are those of
 * sfa_decode_chunk_window / sfa_decode_varlen_window: with num_splits <= 0 the chunk / varlen rule over
 * min(memory_max_len, window - 1 + count) rows, a workspace that holds fewer splits than that gets the largest count it
 * holds, and the split key range is the tiles that hold [lo_0, pos + n).  sfa_decode_chunk_window_workspace_bytes /
 * sfa_decode_varlen_window_workspace_bytes size it; a workspace sized by sfa_decode_chunk_workspace_bytes /
 * sfa_decode_varlen_workspace_bytes is never too small.  The same workspace and status word serve every decode entry
 * point on a stream.
 * Not served: head_dim 256, per-token or per-block scales, ring-buffer caches, soft-capping, fp8 matrix instructions on a
 * quantised Q.  (Attention sinks: sfa_decode_chunk_kv8_window_sinks / sfa_decode_varlen_kv8_window_sinks, below.)
 */
int sfa_decode_chunk_kv8_window(const sfa_decode_args *args, const float *k_scale, const float *v_scale, int num_tokens,
                                int64_t qkv_token_stride, int window, void *stream);
int sfa_decode_varlen_kv8_window(const sfa_decode_args *args, const float *k_scale, const float *v_scale,
                                 const void *cu_tokens, int total_tokens, int64_t qkv_token_stride, int window,
                                 void *stream);

/* ---- sliding-window decode with attention sinks over an fp8 KV cache ---------------- */
/*
 * sfa_decode_kv8_window / sfa_decode_chunk_kv8_window / sfa_decode_varlen_kv8_window for a layer whose softmax carries a
 * learned per-head sink logit: each call is its _kv8_window twin plus the sink rule of sfa_decode_window_sinks.
 * Everything of the _kv8_window call each one extends holds unchanged: the caches are e4m3 bytes in the three layouts;
 * fp16 / bf16; head_dim 64 / 128 (256 returns SFA_ERR_UNSUPPORTED_HEAD_DIM); num_heads / num_heads_kv in {1, 2, 4, 8, 16};
 * bias, RoPE, the rotary tables, partial rotary; k_scale / v_scale device fp32 [num_heads_kv], NULL = 1.0, 4-byte aligned
 * (checked, in the twin's place among its checks); the quantised append -- row pos (+ t) receives k8 = q8(k16 /
 * k_scale[hk]), v8 = q8(v16 / v_scale[hk]), no other byte of a cache changes, and the new tokens attend through their
 * stored bytes; rows below lo / lo_0 and the block_table entries of pages wholly below the window are never read; the
 * cu_tokens rules, the rejection rules and the status bits; the call allocates nothing, never synchronises and may be
 * captured in a graph.  A layer with full attention passes window >= memory_max_len (INT_MAX works); window < 1 returns
 * SFA_ERR_BAD_SHAPE.
 *   sinks           device fp32 [num_heads], one logit per QUERY head, 4-byte aligned (checked first: otherwise
 *                   SFA_ERR_BAD_SHAPE).  Every value is finite or -inf (the caller's contract, not checked).  Read on
 *                   the device only: a replayed graph sees new contents.
 *                   NULL: the call validates under its own name and then launches exactly what the _kv8_window call
 *                   launches; output and caches are bit-identical to it.
 * Semantics, for query head h of kv head hk over its key range [lo, pos] (chunk / varlen: [lo_t, pos + t]) of the cache
 * after the append, s_j = q16 . (k_scale[hk] * K8_j) * head_dim_inv:
 *   o[h] = v_scale[hk] * sum_j exp(s_j) V8_j / (exp(sinks[h]) + sum_j exp(s_j))
 * -- one more key with logit sinks[h] and a zero value row.  The sink is multiplied NEITHER by head_dim_inv NOR by
 * k_scale: it is a logit, not a key.  The caches receive exactly what the _kv8_window call stores.
 * Numerics: the sink joins the online softmax once per query row, whatever the split count.  A sink far above the scores
 * gives a small finite output, with no overflow; a sink whose weight underflows in fp32 (-inf and -1e30 are two) gives
 * the _kv8_window call's output bit for bit at the same explicit num_splits.
 * Workspace: there are no sizing functions of their own.  Layout, split rule and status word are those of the
 * _kv8_window call each one extends, and sfa_decode_window_workspace_bytes / sfa_decode_chunk_window_workspace_bytes /
 * sfa_decode_varlen_window_workspace_bytes size it; with num_splits <= 0 a workspace that holds fewer splits than the
 * library would pick gets the largest count it holds.
 * Not served: sinks on the calls without a window argument (window >= memory_max_len serves them), head_dim 256,
 * per-token or per-block scales, ring-buffer caches, soft-capping, fp8 matrix instructions on a quantised Q.
 */
int sfa_decode_kv8_window_sinks(const sfa_decode_args *args, const float *k_scale, const float *v_scale,
                                const float *sinks, int window, void *stream);
int sfa_decode_chunk_kv8_window_sinks(const sfa_decode_args *args, const float *k_scale, const float *v_scale,
                                      const float *sinks, int num_tokens, int64_t qkv_token_stride, int window,
                                      void *stream);
int sfa_decode_varlen_kv8_window_sinks(const sfa_decode_args *args, const float *k_scale, const float *v_scale,
                                       const float *sinks, const void *cu_tokens, int total_tokens,
                                       int64_t qkv_token_stride, int window, void *stream);

/* ---- prefill: O = softmax(mask(Q K^T * scale)) V ------------------------------- */
/*
 * q [batch, heads_q, seqlen_q, head_dim], k/v [batch, heads_kv, seqlen_k, head_dim],
 * o like q; batch/head/seq strides in elements, >= 0 and multiples of 8, head_dim
 * contiguous, 16-byte aligned rows.  Batch and head strides and the seq strides of q
 * and o are unbounded (64-bit).  The seq stride of k and of v is bounded at head_dim 64
 * and 128, where the kernels address a key row inside its tile in 32 bits: at most
 * floor((2^32 - 1 - 16 * (head_dim / 8 - 1)) / (2 * (T - 1)) / 8) * 8 elements for a tile
 * of T keys -- 34087040 for the 64-key tiles of sfa_prefill_window_fwd and
 * sfa_prefill_split_fwd and of this call's 256-row kernel, 69273656 (head_dim 64:
 * 69273664) for the 32-key tiles of its 128-row kernel (whichever the call picks) -- and what the 4-wave kernel's
 * descriptors cover, from which the call falls back to the former.  The packed calls
 * below bound the token stride of k and v by the same 34087040.  A stride above the
 * limit returns SFA_ERR_BAD_SHAPE ("... k seq stride N exceeds LIMIT elements ...");
 * head_dim 256 is served at any stride.  heads_q % heads_kv == 0 (GQA: query head h reads kv head
 * h / (heads_q/heads_kv)).  causal != 0: key j visible to query i iff
 * j <= i + (seqlen_k - seqlen_q).  lse (optional, fp32 [batch, heads_q, seqlen_q],
 * contiguous) receives log(sum(exp(scaled scores))) per row.  A row with no visible
 * key gets zeros (lse = -inf).
 */
typedef struct sfa_prefill_args {
    const void *q;
    const void *k;
    const void *v;
    void *o;
    float *lse;                     /* may be NULL                                    */
    int batch;
    int heads_q;
    int heads_kv;
    int seqlen_q;
    int seqlen_k;
    int head_dim;                   /* 64, 128 or 256                                 */
    int64_t q_stride[3];            /* {batch, head, seq} strides in elements         */
    int64_t k_stride[3];
    int64_t v_stride[3];
    int64_t o_stride[3];
    float softmax_scale;            /* <= 0 => 1/sqrt(head_dim)                       */
    int causal;
    int dtype;                      /* sfa_dtype                                      */
    int fast_scale;                 /* 0 (default): scores are the fp32 Q.K^T times the scale in fp32.
                                       nonzero, and only when lse == NULL: allow the prescaled-Q kernels
                                       (Q * scale * log2(e) rounded to the 16-bit dtype once, ~5 % faster):
                                       every score then carries a relative error of up to 2^-9 (bf16) /
                                       2^-12 (fp16) of the |q_i k_i| it sums -- invisible for unit-variance
                                       data, several per cent of a softmax weight once logits reach
                                       hundreds (ABI v2)                                                */
} sfa_prefill_args;

int sfa_prefill_fwd(const sfa_prefill_args *args, void *stream);

/* ---- prefill with a sliding window and attention sinks ------------------------------ */
/*
 * sfa_prefill_fwd for a layer whose causal mask is a sliding window and whose softmax may carry a learned per-head sink
 * logit (gpt-oss: 64 query heads over 8 kv heads, head_dim 64, a 128-row window on every second layer).
 * Every field of `args` keeps its sfa_prefill_fwd meaning: strides in elements, multiples of 8; 16-byte alignment; GQA by
 * heads_q % heads_kv == 0; fp16 / bf16; softmax_scale <= 0 means 1/sqrt(head_dim); lse is optional.  Except:
 *   head_dim        64 or 128; 256 returns SFA_ERR_UNSUPPORTED_HEAD_DIM, as in the multi-token decode calls.
 *   causal          must be non-zero, otherwise SFA_ERR_BAD_SHAPE: a two-sided window is not served.
 *   fast_scale      ignored: scores are always the fp32 Q.K^T times the scale in fp32.
 *   window          >= 1 (window < 1 returns SFA_ERR_BAD_SHAPE).  With lim_i = i + (seqlen_k - seqlen_q) and
 *                   lo_i = max(0, lim_i + 1 - window), query row i sees the keys [lo_i, lim_i]: the decode calls' window,
 *                   and flash-attn's window_size = (window - 1, 0).  window = 1 leaves each row its own key;
 *                   window >= seqlen_k (INT_MAX works) is the causal mask.
 *   sinks           device fp32 [heads_q], one logit per QUERY head, in natural-log units; it is NOT multiplied by
 *                   softmax_scale.  4-byte aligned (checked: otherwise SFA_ERR_BAD_SHAPE).  Every value is finite or
 *                   -inf (the caller's contract, not checked).  Read on the device only: a replayed graph sees new
 *                   contents.  NULL: no sink.
 * Semantics, for row i of query head h over j in [lo_i, lim_i], s_j = q_i . k_j * softmax_scale:
 *   o   = sum_j exp(s_j) V_j / (exp(sinks[h]) + sum_j exp(s_j))
 *   lse = log(exp(sinks[h]) + sum_j exp(s_j))
 * -- one more key with logit sinks[h] and a zero value row.  lse is the normaliser of the o that is returned, so
 * o * exp(lse) is the un-normalised sum.  A row with no visible key (lim_i < 0) gets zeros and lse = -inf, sink or not,
 * as in sfa_prefill_fwd: the sink joins only a softmax that has a key.  So seqlen_k == 0 writes zeros and -inf exactly as
 * sfa_prefill_fwd does.
 * What the window promises: with lo_0 = max(0, seqlen_k - seqlen_q + 1 - window), the bound of the first query row, the K
 * and V rows below lo_0 are never read; they may hold anything, NaN included.  A workgroup (256 query rows of one head)
 * reads only the 64-key tiles between its first row's lo and its last row's lim.
 * Numerics: the sink joins the online softmax once per query row.  A sink far above the scores gives a small finite
 * output, with no overflow; a sink whose weight underflows in fp32 (-inf and -1e30 are two) gives the output of the same
 * kernel with no sink, bit for bit.
 * Forwarding: with sinks == NULL and window >= seqlen_k the call validates under its own name and then launches exactly
 * what sfa_prefill_fwd(causal = 1, fast_scale = 0) launches; the output is bit-identical to it, and
 * sfa_debug_get("last_prefill_kernel") reports that kernel.  Every other case -- window >= seqlen_k with sinks included --
 * runs the windowed kernel (csrc/prefill_window_kernel.hip), after which last_prefill_kernel keeps its previous value.
 * Like every entry point it is asynchronous on `stream`, allocates nothing, never synchronises and may be captured in a
 * graph.
 * Not served: head_dim 256, two-sided windows, soft-capping, a paged or fp8 K/V, split key ranges.  (Packed sequences of
 * different lengths: sfa_prefill_varlen_window_fwd, below.)
 */
int sfa_prefill_window_fwd(const sfa_prefill_args *args, int window, const float *sinks, void *stream);

/* ---- prefill with a split key range (small grids) ------------------------------------ */
/*
 * sfa_prefill_fwd for problems with fewer 256-row q-tiles than the chip has compute units -- a short query block against
 * a long context (chunked prefill, prefix-cache hits), one sequence with few heads: the key range of every q-tile is cut
 * into chunks, one workgroup walks each chunk, and a second kernel merges the fp32 partial results.  Added under ABI
 * version 4, beside an unchanged sfa_prefill_args: callers detect the three functions by symbol.
 * Semantics are exactly sfa_prefill_fwd's: the same o and lse, the same strides (elements, multiples of 8) and 16-byte
 * alignment, GQA by heads_q % heads_kv == 0, fp16 / bf16, causal of either value (bottom-right aligned), softmax_scale
 * <= 0 means 1/sqrt(head_dim), a row with no visible key gets zeros and lse = -inf (seqlen_k == 0: every row),
 * batch == 0 or seqlen_q == 0 returns SFA_OK and launches nothing.  Only the work partition differs.  Except:
 *   head_dim        64 or 128; 256 returns SFA_ERR_UNSUPPORTED_HEAD_DIM, as in sfa_prefill_window_fwd.
 *   fast_scale      honoured only where the call forwards (below); the split kernels always use the exact scale.
 *   num_splits      >= 1: explicit.  <= 0: sfa_prefill_auto_splits(batch, heads_q, seqlen_q, seqlen_k, head_dim, causal),
 *                   and a workspace that holds fewer splits than that gets the largest count it holds (a NULL or empty
 *                   one: 1), as in the decode calls.
 *   workspace       device scratch of sfa_prefill_split_workspace_bytes(...) bytes, 256-byte aligned.  It has no status
 *                   block and no contents that survive a call; it may hold anything on entry, NaN included.  Checked
 *                   only when the resolved count (below) is above 1: NULL returns SFA_ERR_NULL_POINTER, a misaligned
 *                   one SFA_ERR_BAD_SHAPE, too few bytes for an explicit num_splits SFA_ERR_WORKSPACE_TOO_SMALL.
 * The checks of `args` come first, with the texts and the order of sfa_prefill_fwd's under this call's name.
 * Partition.  nkt_max = ceil(seqlen_k / 64) is the number of 64-key tiles of the longest q-tile.  A request for S splits
 * resolves to C = ceil(nkt_max / S) tiles per split and S' = ceil(nkt_max / C) <= S splits (5 tiles, S = 4: C = 2, S' = 3).
 * Split s of q-tile qt (256 query rows) owns the tiles [s C, min((s + 1) C, nkt(qt))), where nkt(qt) is the number of
 * tiles the q-tile's last row sees: nkt_max without a mask; under the causal mask lim / 64 + 1 with
 * lim = min(256 (qt + 1), seqlen_q) - 1 + seqlen_k - seqlen_q, and 0 when lim < 0.  A split with s C >= nkt(qt) is empty:
 * its workgroup reads no K or V and writes nothing.  Chunks have one length, so under the causal mask a short q-tile
 * yields fewer partials, not thinner ones, and the partial traffic -- 4 (head_dim + 2) bytes per row and split, written
 * and read once -- stays proportional to the work.
 * Forwarding: a resolved count of 1 launches exactly what sfa_prefill_fwd launches for the same args (fast_scale
 * honoured); the output is bit-identical to it, sfa_debug_get("last_prefill_kernel") reports that kernel, and the
 * workspace may be NULL.  Every resolved count above 1 runs csrc/prefill_split_kernel.hip's two kernels, after which
 * last_prefill_kernel keeps its previous value.  sfa_debug_get("last_prefill_splits") reports the resolved count.
 * Like every entry point it is asynchronous on `stream`, allocates nothing, never synchronises and may be captured in a
 * graph: two launches on the one stream, no parallel branches.
 * Not served: head_dim 256; a window or sinks together with the split (short windows need no split; full attention with
 * sinks is a follow-up); a combine fused into the last-arriving split; a paged or fp8 K/V.  (Packed sequences of
 * different lengths: sfa_prefill_varlen_split_fwd, below.)
 */
int sfa_prefill_split_fwd(const sfa_prefill_args *args, int num_splits, void *workspace, size_t workspace_bytes,
                          void *stream);
/* Bytes of workspace for `num_splits` (as given to the call: >= 1 explicit, <= 0 the library's choice): a multiple of
 * 256, the same for a request and the count it resolves to, non-decreasing in num_splits, 0 where the count resolves to 1.
 * It does not depend on `causal` (the mask only leaves some partials unused).  Bad dimensions: 0. */
size_t sfa_prefill_split_workspace_bytes(int batch, int heads_q, int seqlen_q, int seqlen_k, int head_dim, int causal,
                                         int num_splits);
/* The split count the library picks from the shapes alone (>= 1, at most ceil(seqlen_k / 64)): 1 whenever
 * batch * heads_q * ceil(seqlen_q / 256) reaches the 256 compute units or the key range is too short to give every
 * split its minimum chunk; otherwise the smallest count that brings the workgroups to the compute-unit count, capped
 * (csrc/c_api.hip has the rule and its measurements). */
int sfa_prefill_auto_splits(int batch, int heads_q, int seqlen_q, int seqlen_k, int head_dim, int causal);

/* ---- prefill over packed sequences of different lengths ------------------------------- */
/*
 * sfa_prefill_fwd for a batch whose sequences do not share one seqlen_q and one seqlen_k -- prompts of different lengths,
 * chunked-prefill blocks against prefixes of different lengths -- in flash-attn's packed layout: the rows of all
 * sequences one after another, delimited by cu_seqlens_q / cu_seqlens_k.  Added under ABI version 4 with a struct of its
 * own, beside an unchanged sfa_prefill_args: callers detect the two functions by symbol.
 *   q               [total_q, heads_q, head_dim]; k, v [total_k, heads_kv, head_dim]; o like q.  {token, head} strides in
 *                   elements, >= 0 and multiples of 8, head_dim contiguous, 16-byte aligned.  The token stride of k and of v
 *                   is at most 34087040 elements (sfa_prefill_args above: the 64-key tiles' 32-bit row offset); a larger
 *                   one returns SFA_ERR_BAD_SHAPE ("... k token stride N exceeds 34087040 elements ...") with the strides.
 *   lse             optional, fp32 [heads_q, total_q], contiguous, 4-byte aligned: the row of packed query row r of head h
 *                   is h * total_q + r.
 *   cu_seqlens_q, cu_seqlens_k   device int32 [batch + 1], 4-byte aligned.  Sequence b owns the packed query rows
 *                   [cu_q[b], cu_q[b+1]) and the packed key rows [cu_k[b], cu_k[b+1]).  Read on the device only: the call
 *                   never synchronises, and a captured graph may be replayed with other contents as long as batch,
 *                   total_q and total_k stay the same.
 *   total_q, total_k   host values: the rows the tensors hold, >= cu[batch].  They size the grid and the workspace.
 *   head_dim        64 or 128; 256 returns SFA_ERR_UNSUPPORTED_HEAD_DIM: sfa_prefill_fwd is the call that serves it.
 *   softmax_scale   <= 0 means 1/sqrt(head_dim).  There is no fast_scale: scores are always the fp32 Q.K^T times the scale
 *                   in fp32.
 *   workspace       device scratch of sfa_prefill_varlen_workspace_bytes(batch, total_q) bytes, 256-byte aligned.  It
 *                   holds the plan only -- one 8-byte entry per work-item slot, total_q / 256 + batch of them -- and has
 *                   no status block.  Its contents on entry never matter: every slot is written on every call.
 * Semantics.  With n_q and n_k the row counts of sequence b, its o and lse rows are what sfa_prefill_fwd gives for
 * batch = 1, seqlen_q = n_q, seqlen_k = n_k on those rows: exact scale, fp32 scores, GQA by heads_q % heads_kv == 0,
 * fp16 / bf16, causal of either value, bottom-right aligned per sequence (key j visible to row i iff j <= i + (n_k - n_q)),
 * a row with no visible key gets zeros and lse = -inf -- every row of a sequence with n_k == 0.  A sequence with
 * n_q == 0 takes no part.
 * A sequence is valid iff 0 <= cu[b] <= cu[b+1] <= total holds in both arrays; every kernel re-derives this for the
 * sequence it serves.  An invalid sequence is skipped: none of its rows is read or written.  There is no status word:
 * a caller that needs to know checks its cu arrays itself.
 * What the call promises about memory: packed rows that belong to no valid sequence -- the rows between cu_q[batch] and
 * total_q included -- are neither read nor written, in o and lse as in q, k and v.  The workgroups of sequence b read no
 * K or V row outside [cu_k[b], cu_k[b+1]) and no q row outside [cu_q[b], cu_q[b+1]) (ragged last tiles clamp to the
 * sequence's own last row), and write no o row outside it.  So a valid sequence's result is a function of its own rows
 * only, bit-identical whether it is computed alone or inside any batch.
 * Argument checks, in this order: args NULL; q / k / v / o / cu_seqlens_q / cu_seqlens_k NULL (SFA_ERR_NULL_POINTER);
 * batch < 0, a head count <= 0, total_q < 0 or total_k < 0; heads_q % heads_kv != 0 (SFA_ERR_BAD_SHAPE); head_dim
 * (SFA_ERR_UNSUPPORTED_HEAD_DIM); dtype (SFA_ERR_BAD_DTYPE); strides; alignment (SFA_ERR_BAD_SHAPE).  Then batch == 0 or
 * total_q == 0 returns SFA_OK: nothing is launched and the workspace is not looked at.  Then the workspace: NULL
 * (SFA_ERR_NULL_POINTER), not 256-byte aligned (SFA_ERR_BAD_SHAPE), too small (SFA_ERR_WORKSPACE_TOO_SMALL).  Last, a
 * grid of (total_q / 256 + batch) * heads_q workgroups that does not fit 2^31 - 1 (SFA_ERR_BAD_SHAPE).
 * Runs csrc/prefill_varlen_kernel.hip's two kernels; sfa_debug_get("last_prefill_kernel") and "last_prefill_splits" keep
 * their values.  Like every entry point it is asynchronous on `stream`, allocates nothing, never synchronises and may be
 * captured in a graph: two launches on the one stream, no parallel branches.
 * Not served: head_dim 256; a paged or fp8 K/V; a status word for bad cu_seqlens; backward.  (A sliding window and sinks:
 * sfa_prefill_varlen_window_fwd; a key-range split for batches of few q-tiles: sfa_prefill_varlen_split_fwd, both below.)
 */
typedef struct sfa_prefill_varlen_args {
    const void *q;
    const void *k;
    const void *v;
    void *o;
    float *lse;                     /* may be NULL                                    */
    const void *cu_seqlens_q;       /* device int32 [batch + 1]                       */
    const void *cu_seqlens_k;       /* device int32 [batch + 1]                       */
    int batch;
    int heads_q;
    int heads_kv;
    int total_q;
    int total_k;
    int head_dim;                   /* 64 or 128                                      */
    int64_t q_stride[2];            /* {token, head} strides in elements              */
    int64_t k_stride[2];
    int64_t v_stride[2];
    int64_t o_stride[2];
    float softmax_scale;            /* <= 0 => 1/sqrt(head_dim)                       */
    int causal;
    int dtype;                      /* sfa_dtype                                      */
} sfa_prefill_varlen_args;

int sfa_prefill_varlen_fwd(const sfa_prefill_varlen_args *args, void *workspace, size_t workspace_bytes, void *stream);
/* Bytes of workspace: 8 * (total_q / 256 + batch) rounded up to a multiple of 256; non-decreasing in both arguments.
 * batch <= 0 or total_q <= 0: 0. */
size_t sfa_prefill_varlen_workspace_bytes(int batch, int total_q);

/* ---- packed prefill with a sliding window and attention sinks -------------------------- */
/*
 * sfa_prefill_varlen_fwd for a layer whose causal mask is a sliding window and whose softmax may carry a learned per-head
 * sink logit: sfa_prefill_window_fwd's mask and sink on sfa_prefill_varlen_fwd's packed, ragged batches.  Added under ABI
 * version 4 beside an unchanged sfa_prefill_varlen_args: callers detect it by symbol.
 * Every field of `args` keeps its sfa_prefill_varlen_fwd meaning -- layouts, strides, alignment, cu_seqlens read on the
 * device only, total_q / total_k, head_dim 64 or 128, fp16 / bf16, GQA, exact scale -- and the workspace is that call's:
 * sfa_prefill_varlen_workspace_bytes(batch, total_q) bytes, 256-byte aligned, the plan alone.  Except:
 *   causal          must be non-zero, otherwise SFA_ERR_BAD_SHAPE: a two-sided window is not served.
 *   window          >= 1 (window < 1 returns SFA_ERR_BAD_SHAPE).  In sequence b with n_q query rows and n_k key rows, with
 *                   lim_i = i + (n_k - n_q) and lo_i = max(0, lim_i + 1 - window), query row i sees the keys [lo_i, lim_i]
 *                   of its own sequence.  A window of n_k or more is the causal mask for that sequence (INT_MAX works).
 *   sinks           device fp32 [heads_q], one logit per QUERY head, in natural-log units; it is NOT multiplied by
 *                   softmax_scale.  4-byte aligned (checked: otherwise SFA_ERR_BAD_SHAPE).  Every value is finite or
 *                   -inf (the caller's contract, not checked).  Read on the device only: a replayed graph sees new
 *                   contents.  NULL: no sink.
 * Semantics.  The o and lse rows of sequence b are what sfa_prefill_window_fwd gives for batch = 1, seqlen_q = n_q,
 * seqlen_k = n_k on those rows -- bit for bit wherever that call runs its windowed kernel (sinks given, or window < n_k):
 *   o   = sum_j exp(s_j) V_j / (exp(sinks[h]) + sum_j exp(s_j))
 *   lse = log(exp(sinks[h]) + sum_j exp(s_j))
 * over j in [lo_i, lim_i], s_j = q_i . k_j * softmax_scale.  A row without a visible key gets zeros and lse = -inf, sink
 * or not: every row of a sequence with n_k == 0, and the rows with lim_i < 0 when n_q > n_k.  A sequence with n_q == 0
 * takes no part; an invalid sequence is skipped with nothing of it read or written; there is no status word.
 * What the call promises about memory: everything sfa_prefill_varlen_fwd promises, and with
 * lo_0(b) = max(0, n_k - n_q + 1 - window), the bound of the sequence's first query row, no K or V row of sequence b
 * below cu_k[b] + lo_0(b) is read; those rows may hold anything, NaN included.
 * Argument checks: sfa_prefill_varlen_fwd's, in its order with its texts under this call's name.  Directly after the
 * alignment step and before the batch == 0 or total_q == 0 return: sinks not 4-byte aligned, causal == 0, window < 1
 * (SFA_ERR_BAD_SHAPE each).  The workspace checks and the grid check follow unchanged.
 * Forwarding: with sinks == NULL and window >= total_k the call validates under its own name and then launches exactly
 * what sfa_prefill_varlen_fwd(causal = 1) launches; the output is bit-identical to it.  Every other case -- window >=
 * total_k with sinks included -- runs the plan kernel and csrc/prefill_varlen_window_kernel.hip's kernel.
 * sfa_debug_get("last_prefill_kernel") and "last_prefill_splits" keep their values.  Like every entry point it is
 * asynchronous on `stream`, allocates nothing, never synchronises and may be captured in a graph: two launches on the one
 * stream, no parallel branches.
 * Not served: head_dim 256; two-sided windows; soft-capping; a paged or fp8 K/V; a key-range split together with the window
 * (sfa_prefill_varlen_split_fwd, below, splits the causal and the full mask only); a status word for bad cu_seqlens;
 * backward.
 */
int sfa_prefill_varlen_window_fwd(const sfa_prefill_varlen_args *args, int window, const float *sinks, void *workspace,
                                  size_t workspace_bytes, void *stream);

/* ---- packed prefill with a split key range (few q-tiles, long prefixes) ---------------- */
/*
 * sfa_prefill_varlen_fwd for packed batches with fewer q-tiles than the chip has compute units -- chunked prefill under
 * continuous batching: a handful of sequences, each a query block of a few hundred rows against a prefix of thousands of
 * keys: sfa_prefill_split_fwd's partition on sfa_prefill_varlen_fwd's packed, ragged batches.  Added under ABI version 4
 * beside an unchanged sfa_prefill_varlen_args: callers detect the three functions by symbol.
 * Semantics are exactly sfa_prefill_varlen_fwd's: the same o and lse, the same layouts, strides and alignment, cu_seqlens
 * read on the device only, total_q / total_k, head_dim 64 or 128 (256: SFA_ERR_UNSUPPORTED_HEAD_DIM), fp16 / bf16, GQA,
 * exact scale, causal of either value, bottom-right aligned per sequence, zeros and lse = -inf for a row without a visible
 * key (every row of a sequence with n_k == 0), a sequence with n_q == 0 takes no part, an invalid sequence is skipped
 * with nothing of it read or written, no status word.  Only the work partition differs.  Except:
 *   max_seqlen_k    a host value, because the lengths live on the device: a partition hint only.  >= 1 (< 1 returns
 *                   SFA_ERR_BAD_SHAPE).  Results are correct for any value >= 1, whatever the real lengths are.
 *   num_splits      >= 1: explicit.  <= 0: sfa_prefill_varlen_auto_splits(batch, heads_q, total_q, max_seqlen_k, head_dim,
 *                   causal), and a workspace that holds fewer splits than that gets the largest count it holds (an empty
 *                   one: 1), as in sfa_prefill_split_fwd.
 *   workspace       device scratch of sfa_prefill_varlen_split_workspace_bytes(...) bytes, 256-byte aligned, no status
 *                   block.  Its contents on entry never matter (NaN, 0x00 and 0xFF give identical results): what is read
 *                   was written by the same call.
 * Partition.  nkt_max = ceil(max_seqlen_k / 64).  A request for S splits resolves exactly as in sfa_prefill_split_fwd:
 * C = ceil(nkt_max / min(S, nkt_max)) tiles per split and S' = ceil(nkt_max / C) splits.  For q-tile qt (256 query rows) of
 * sequence b, nkt(b, qt) is the number of 64-key tiles its last row sees: ceil(n_k / 64) without a mask; under the causal
 * mask lim / 64 + 1 with lim = min(256 (qt + 1), n_q) - 1 + n_k - n_q, and 0 when lim < 0.  Split s < S' - 1 owns the tiles
 * [s C, min((s + 1) C, nkt)); the last split S' - 1 owns [(S' - 1) C, nkt), so a sequence longer than max_seqlen_k is still
 * computed in full, only unevenly.  A split with s C >= nkt is empty: no workgroup runs for it, nothing of K or V is read
 * for it, and no partial is written or read.
 * Workspace layout.  With bound = total_q / 256 + batch q-tile slots, three regions, each rounded up to 256 bytes:
 *   the q-tile plan of sfa_prefill_varlen_fwd       8 * bound bytes
 *   the item list, (q-tile slot, split) entries     8 * bound * S' bytes
 *   the fp32 partials                               bound * heads_q * S' * 256 rows of head_dim + 2 floats
 * sfa_prefill_varlen_split_workspace_bytes returns exactly this sum; for S' == 1 the plan alone.
 * What the call promises about memory: everything sfa_prefill_varlen_fwd promises.  A valid sequence's result is a
 * function of its own rows and of (C, S') only, bit-identical whether it is computed alone or inside any batch; and where
 * sfa_prefill_split_fwd on the sequence's own [1, heads, n, head_dim] view resolves to the same C and covers the same
 * tiles per split, the packed call returns that call's bits for the sequence's rows (the same walk, the same ordered
 * merge).
 * Argument checks: sfa_prefill_varlen_fwd's, in its order with its texts under this call's name.  Directly after the
 * alignment step and before the batch == 0 or total_q == 0 return: max_seqlen_k < 1 (SFA_ERR_BAD_SHAPE).  The workspace
 * checks use the resolved count: NULL (SFA_ERR_NULL_POINTER), not 256-byte aligned (SFA_ERR_BAD_SHAPE), too few bytes for
 * an explicit num_splits (SFA_ERR_WORKSPACE_TOO_SMALL).  Last, the attention grid of bound * S' * heads_q workgroups or the
 * combine grid of bound * heads_q * head_dim / 4 that does not fit 2^31 - 1 (SFA_ERR_BAD_SHAPE).
 * Forwarding: a resolved count of 1 validates under this call's name and then launches exactly what
 * sfa_prefill_varlen_fwd launches; the output is bit-identical to it, and only the plan part of the workspace is needed.
 * Every other count runs the plan kernel and csrc/prefill_varlen_split_kernel.hip's three kernels.
 * sfa_debug_get("last_prefill_splits") reports the resolved count (1: forwarded); "last_prefill_kernel" keeps its value.
 * Like every entry point it is asynchronous on `stream`, allocates nothing, never synchronises and may be captured in a
 * graph and replayed with other cu_seqlens contents under the same batch, totals, max_seqlen_k and num_splits: up to four
 * launches on the one stream, no parallel branches.
 * Not served: head_dim 256; a window or sinks together with the split; a chunk length per sequence (one C serves the
 * batch, so one long prefix among short ones is walked by its last split alone); a paged or fp8 K/V; backward.
 */
int sfa_prefill_varlen_split_fwd(const sfa_prefill_varlen_args *args, int max_seqlen_k, int num_splits, void *workspace,
                                 size_t workspace_bytes, void *stream);
/* Bytes of workspace for `num_splits` (as given to the call: >= 1 explicit, <= 0 the library's choice), with
 * bound = total_q / 256 + batch and S' the resolved count:
 *   S' == 1:  up256(8 bound)                                  (= sfa_prefill_varlen_workspace_bytes(batch, total_q))
 *   S' >= 2:  up256(8 bound) + up256(8 bound S') + 4 (head_dim + 2) * 256 bound heads_q S'
 * A multiple of 256, the same for a request and the count it resolves to, non-decreasing in num_splits.  Bad dimensions
 * (a count <= 0, max_seqlen_k < 1, head_dim not 64 / 128): 0. */
size_t sfa_prefill_varlen_split_workspace_bytes(int batch, int heads_q, int total_q, int max_seqlen_k, int head_dim,
                                                int num_splits);
/* The split count the library picks from what the host knows: sfa_prefill_auto_splits' rule and constants (measured on
 * rectangular problems) for heads_q * ceil(total_q / 256) workgroups and ceil(max_seqlen_k / 64) key tiles, that is
 * sfa_prefill_auto_splits(1, heads_q, total_q, max_seqlen_k, head_dim, causal).  1 from 256 workgroups on. */
int sfa_prefill_varlen_auto_splits(int batch, int heads_q, int total_q, int max_seqlen_k, int head_dim, int causal);

/* ---- test / A-B hooks: NOT part of the drop-in surface ------------------------------ */
/* The launch paths read no environment variable; the test-suite and tools/ select kernel
 * variants through this call.  knob: "prefill_impl" (-1 auto; the kernel ids of csrc/prefill_common.h, see
 * csrc/prefill_dispatch.hip), "prefill_pairs" (1/2), "decode_nt" (0/1), "decode_gqa_mfma" (0/1),
 * "bm128_one_wg" (0/1).  value -1 = the library's own choice.  Process-wide.  The diagnostic values -- prefill_impl
 * 2, 4, 43, 44 and bm128_one_wg 1 -- need the diagnostics build of the library (build_lib(variants=True)); elsewhere
 * sfa_debug_set refuses bm128_one_wg 1 and sfa_prefill_fwd refuses those ids, as it refuses any id not in the table. */
int sfa_debug_set(const char *knob, int value);
/* Read back: the knobs above, and "last_prefill_kernel" = which kernel the last sfa_prefill_fwd of this process
 * launched (the dispatcher's choice included): 1 / 3 the 8-wave 256-row kernel (exact / prescaled), 20 + f the 128-row
 * geometry, 40 + f the 4-wave persistent kernel (f: 1 prescaled, 2 exact), 60 / 61 the head_dim 256 kernels, -1 none
 * yet; "last_prefill_splits" = the resolved split count of this process's last sfa_prefill_split_fwd or
 * sfa_prefill_varlen_split_fwd, 1 if it
 * forwarded, -1 if there was none yet.  Unknown knob: INT_MIN.  (bench.py names its roofline kernel from this.) */
int sfa_debug_get(const char *knob);

/* ---- small helpers the reference's C++ harness uses ----------------------------- */
/* cos/sin LUT, [max_seq_len, rot_dim/2] each, entry (pos, j) = cos/sin(pos * 10000^(-2j/rot_dim)). */
int sfa_compute_rotary_table(void *cos_table, void *sin_table, int max_seq_len,
                             int rot_dim, int dtype, void *stream);
/* array[i] = bits for i < n (16-bit elements). */
int sfa_fill_16bit(void *array, uint16_t bits, size_t n, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* STAR_FLASH_ATTN_C_API_H_ */
