// Host-side glue between the C ABI (include/star_flash_attn.h) and the kernel launchers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

#include <atomic>

#include "../../include/star_flash_attn.h"

namespace sfa {

// thread-local error text for sfa_last_error()
void set_error(const char *fmt, ...);
int fail(int status, const char *fmt, ...);

constexpr size_t kStatusBytes = 256;

// The workspace of sfa_decode, sfa_decode_chunk and sfa_decode_varlen: byte offsets of its regions, in this order, each
// rounded up to 256 bytes (a region an entry point does not have is empty), and the size the caller must provide.
//   [0, 256)   status block (sticky error word)
//   plan       int2 (b, q_tile) per attention workgroup slot, b = -1 = empty.  varlen only: bound = rows / 256 + B entries
//              (every sequence with tokens has ceil(n_b * G / 256) <= n_b * G / 256 + 1 q-tiles)
//   q_rot      rotated Q, 16 bit.  chunk: [B, Hkv, R, D], row r = t*G + g of kv head hk is query head hk*G + g of token
//              t; varlen: [Hkv, rows, D], row cu_tokens[b] * G + t * G + g, rows = total_tokens * G
//   part_o     (S > 1) fp32 partial outputs.  decode: [B, H, S, D]; chunk: [B, Hkv, S, R, D]; varlen: [Hkv, S, rows, D]
//   part_ml    (S > 1) float2 (m, l), the same index without D
// The sizes depend on the token total, never on how the tokens are spread over sequences.
struct DecodeWorkspace {
    size_t plan, q_rot, part_o, part_ml, total;
};
// q_rows rows of rotated Q (0: sfa_decode), part_rows * S rows of partials
DecodeWorkspace decode_workspace(size_t plan_entries, size_t q_rows, size_t part_rows, int S, int D);

struct DecodeKernelParams {
    const uint16_t *qkv;
    const uint16_t *q_bias, *k_bias, *v_bias;
    uint16_t *o;
    const int32_t *seq_len;
    uint16_t *k_cache, *v_cache;
    const uint16_t *cos_tab, *sin_tab;
    float *part_o;          // [B,H,S,D]   un-normalised partial outputs
    float2 *part_ml;        // [B,H,S]     (running max in log2 units, running sum)
    int32_t *status;        // sticky error word
    int B, M, H, L, layer, rot_dim, num_splits;
    int Hkv;                // kv heads (== H unless grouped queries)
    long long qkv_stride;   // elements between batches of qkv
    long long kv_row_stride, kv_head_stride;    // elements between cache rows / heads of one (b, layer)
    const int32_t *block_table;  // paged caches: [B, table_stride] page numbers, else nullptr
    int page_shift, table_stride, num_pages;    // page_size = 1 << page_shift
    long long page_stride;       // elements between pages of a pool
    float scale_log2;       // softmax scale * log2(e)
};

// sfa_decode_chunk (decode_chunk_kernel.hip, decode_chunk_body.h): n new tokens per sequence.
struct ChunkKernelParams {
    DecodeKernelParams d;   // every field keeps its sfa_decode meaning; d.part_o / d.part_ml are the chunk partials
    uint16_t *q_rot;        // workspace: rotated, rounded Q
    long long tok_stride;   // elements between tokens of qkv
    int n;                  // new tokens per sequence
    int G;                  // query heads per kv head
    int R;                  // query rows per (batch, kv head) = n * G
};

// sfa_decode_varlen (decode_varlen_kernel.hip): n_b = cu_tokens[b+1] - cu_tokens[b] new tokens for sequence b, packed.
struct VarlenKernelParams {
    ChunkKernelParams c;    // c.n, c.R and c.d.qkv_stride are unused (0): they are per sequence here
    const int32_t *cu_tokens;   // [B + 1]
    int2 *plan;             // workspace: [bound]
    long long rows;         // total * G: packed query rows per kv head
    int total;              // host bound of cu_tokens[B]: rows of qkv / o
    int bound;              // plan entries = grid.x of the attention kernel
};

// sfa_decode_chunk_window / sfa_decode_varlen_window (decode_chunk_window_kernel.hip, decode_varlen_window_kernel.hip):
// the two calls above with a sliding window.  The window rides behind the unchanged parameters, so the kernels without
// one keep their argument layout.
struct ChunkWindowKernelParams {
    ChunkKernelParams base;
    int window;             // >= 1: token t at pos + t attends to the rows max(0, pos + t + 1 - window) .. pos + t
};
struct VarlenWindowKernelParams {
    VarlenKernelParams base;
    int window;
};

// sfa_decode_kv8 (decode_kv8_kernel.hip, decode_kv8_body.h): caches of one byte per element (e4m3) with a scale per kv head.
struct Kv8KernelParams {
    DecodeKernelParams d;   // every field keeps its sfa_decode meaning; d.k_cache / d.v_cache point to bytes, the cache
                            // strides are in elements = bytes
    const float *k_scale, *v_scale;     // [Hkv] each, nullptr = 1.0
};

// sfa_decode_chunk_kv8 / sfa_decode_varlen_kv8 (decode_chunk_kv8_kernel.hip, decode_varlen_kv8_kernel.hip): the chunk and
// varlen calls over e4m3 caches.  As in Kv8KernelParams the cache pointers of `base` point to bytes and the cache strides
// are in elements = bytes; the scales ride behind the unchanged parameters, as the window does above.
struct ChunkKv8KernelParams {
    ChunkKernelParams base;
    const float *k_scale, *v_scale;     // [Hkv] each, nullptr = 1.0
};
struct VarlenKv8KernelParams {
    VarlenKernelParams base;
    const float *k_scale, *v_scale;
};

// sfa_decode_chunk_kv8_window / sfa_decode_varlen_kv8_window (decode_chunk_kv8_window_kernel.hip,
// decode_varlen_kv8_window_kernel.hip): the chunk and varlen calls over e4m3 caches with a sliding window -- the window
// and the scales of the structs above, with their meanings, behind the same unchanged parameters.
struct ChunkKv8WindowKernelParams {
    ChunkKernelParams base;
    int window;
    const float *k_scale, *v_scale;
};
struct VarlenKv8WindowKernelParams {
    VarlenKernelParams base;
    int window;
    const float *k_scale, *v_scale;
};

// sfa_decode_window (decode_window_kernel.hip, the body of decode_mfma16.h with its window): sfa_decode over the last
// `window` positions.
struct WindowKernelParams {
    DecodeKernelParams d;   // every field keeps its sfa_decode meaning
    int window;             // >= 1: the token at pos attends to the rows max(0, pos + 1 - window) .. pos
};

// sfa_decode_window_sinks / sfa_decode_chunk_window_sinks / sfa_decode_varlen_window_sinks (decode_window_sinks_kernel.hip,
// decode_chunk_window_sinks_kernel.hip, decode_varlen_window_sinks_kernel.hip): the three windowed calls over 16-bit caches
// with an attention sink.  The sink pointer rides behind the unchanged parameters, as the window does.
struct WindowSinksKernelParams {
    WindowKernelParams base;
    const float *sinks;     // [H] fp32, one logit per query head (natural-log units, not scaled); never nullptr here
};
struct ChunkWindowSinksKernelParams {
    ChunkKernelParams base;
    int window;
    const float *sinks;
};
struct VarlenWindowSinksKernelParams {
    VarlenKernelParams base;
    int window;
    const float *sinks;
};

// sfa_decode_kv8_window (decode_kv8_window_kernel.hip, the body of decode_kv8_body.h with its window): sfa_decode_kv8
// over the last `window` positions.  The window rides behind the unchanged parameters, so decode_kv8_kernel keeps its
// argument layout.
struct Kv8WindowKernelParams {
    Kv8KernelParams base;
    int window;             // >= 1: the token at pos attends to the rows max(0, pos + 1 - window) .. pos
};

// sfa_decode_kv8_window_sinks / sfa_decode_chunk_kv8_window_sinks / sfa_decode_varlen_kv8_window_sinks
// (decode_kv8_window_sinks_kernel.hip, decode_chunk_kv8_window_sinks_kernel.hip, decode_varlen_kv8_window_sinks_kernel.hip):
// the three windowed calls over e4m3 caches with an attention sink.  The sink pointer rides behind the unchanged
// parameters of the call without one.
struct Kv8WindowSinksKernelParams {
    Kv8WindowKernelParams base;
    const float *sinks;     // [H] fp32, one logit per query head (natural-log units, scaled by nothing); never nullptr here
};
struct ChunkKv8WindowSinksKernelParams {
    ChunkKernelParams base;
    int window;
    const float *k_scale, *v_scale;
    const float *sinks;
};
struct VarlenKv8WindowSinksKernelParams {
    VarlenKernelParams base;
    int window;
    const float *k_scale, *v_scale;
    const float *sinks;
};

struct PrefillKernelParams {
    const uint16_t *q, *k, *v;
    uint16_t *o;
    float *lse;
    int B, Hq, Hkv, Sq, Sk;
    long long qs[3], ks[3], vs[3], os[3];   // {batch, head, seq} strides (elements)
    float scale_log2;
    int nq_tiles;           // workgroup slots per (batch, head) -- set by each kernel's launcher
    int pairs_per_wg;       // prefill_kernel.hip: balanced q-tile pairs one workgroup walks (1 or 2)
    int bh_per_xcd;         // ceil(B*Hq / 8)
    int fast_scale;         // caller allows the prescaled-Q flavour (only used when lse == nullptr)
};

// sfa_prefill_window_fwd (prefill_window_kernel.hip): the prefill forward with a sliding window and an optional attention
// sink.  Window and sink ride behind the unchanged parameters, so the prefill kernels keep their argument layout.
struct PrefillWindowKernelParams {
    PrefillKernelParams base;   // every field keeps its meaning; nq_tiles = q-tiles (256 rows) per (batch, head)
    int window;             // >= 1: row i with causal limit lim sees the keys max(0, lim + 1 - window) .. lim
    const float *sinks;     // [Hq] fp32, one logit per query head (natural-log units, not scaled), or nullptr
};

// sfa_prefill_split_fwd (prefill_split_kernel.hip): the prefill forward with each q-tile's key range cut into num_splits
// chunks of tiles_per_split 64-key tiles, one workgroup per (q-tile, chunk), and a combine over the fp32 partials.  The
// split rides behind the unchanged parameters, as the window does above.  Partials of row r (< 256) of q-tile qt of
// (batch, head) bh, split s: index ((bh * nq_tiles + qt) * num_splits + s) * 256 + r of part_ml, times head_dim of part_o.
struct PrefillSplitKernelParams {
    PrefillKernelParams base;   // every field keeps its meaning; nq_tiles = q-tiles (256 rows) per (batch, head)
    float *part_o;          // workspace: un-normalised fp32 partial outputs
    float2 *part_ml;        // workspace: (reference max in log2 units, row sum) of each partial
    int num_splits;         // resolved count, >= 2
    int tiles_per_split;    // ceil(ceil(Sk / 64) / requested splits)
};

// sfa_prefill_varlen_fwd (prefill_varlen_kernel.hip): the prefill forward over packed sequences of different lengths.
// Sequence b owns the q / o rows [cu_q[b], cu_q[b+1]) and the k / v rows [cu_k[b], cu_k[b+1]); the cu arrays are read on
// the device only.  The workspace is the plan alone: int2 (b, q_tile) per workgroup slot, b = -1 = empty.
struct PrefillVarlenKernelParams {
    const uint16_t *q, *k, *v;
    uint16_t *o;
    float *lse;             // [Hq, total_q] or nullptr
    const int32_t *cu_q, *cu_k;     // [B + 1] each
    int2 *plan;             // workspace: [bound]
    int B, Hq, Hkv;
    int total_q, total_k;   // host bounds of cu_q[B] / cu_k[B]: rows of q, o / k, v
    int bound;              // plan entries = total_q / 256 + B; the attention grid is bound * Hq workgroups
    int slices;             // 8 (Hq % 8 == 0: blockIdx & 7 selects Hq / 8 query heads) or 1
    long long qs[2], ks[2], vs[2], os[2];   // {token, head} strides (elements)
    float scale_log2;
};

// sfa_prefill_varlen_window_fwd (prefill_varlen_window_kernel.hip): the packed prefill forward with a sliding window and
// an optional attention sink, per sequence.  Window and sink ride behind the unchanged parameters, as above.
struct PrefillVarlenWindowKernelParams {
    PrefillVarlenKernelParams base;     // every field keeps its meaning
    int window;             // >= 1: row i of a sequence with causal limit lim sees its keys max(0, lim + 1 - window) .. lim
    const float *sinks;     // [Hq] fp32, one logit per query head (natural-log units, not scaled), or nullptr
};

// sfa_prefill_varlen_split_fwd (prefill_varlen_split_kernel.hip): the packed prefill forward with each q-tile's key range
// cut into num_splits chunks of tiles_per_split 64-key tiles, the last chunk open-ended.  The split rides behind the
// unchanged parameters, as above.  Partials of row r (< 256) of plan slot i, query head h, split s: index
// ((i * Hq + h) * num_splits + s) * 256 + r of part_ml, times head_dim of part_o.
struct PrefillVarlenSplitKernelParams {
    PrefillVarlenKernelParams base;     // every field keeps its meaning
    int2 *items;            // workspace: [bound * num_splits] (plan slot, split) per attention workgroup slot, (-1, 0) = empty
    float *part_o;          // workspace: un-normalised fp32 partial outputs
    float2 *part_ml;        // workspace: (reference max in log2 units, row sum) of each partial
    int num_splits;         // resolved count, >= 2
    int tiles_per_split;    // ceil(ceil(max_seqlen_k / 64) / num_splits)
};

int launch_decode(const DecodeKernelParams &p, int dtype, int head_dim, hipStream_t stream);     // decode_dispatch.hip
// non-temporal cache loads? (both caches of elem_bytes per element against the Infinity Cache, or the decode_nt knob)
bool decode_nt(const DecodeKernelParams &p, int head_dim, int elem_bytes);                       // decode_dispatch.hip
// the attention kernels launch_decode chooses from (validated dtype / head_dim; nt: non-temporal cache loads) and the
// split combine
int launch_decode_mha(const DecodeKernelParams &p, int dtype, int head_dim, bool nt, hipStream_t stream);
int launch_decode_gqa(const DecodeKernelParams &p, int dtype, int head_dim, bool nt, hipStream_t stream);
int launch_decode_gqa_mfma(const DecodeKernelParams &p, int dtype, int head_dim, bool nt, hipStream_t stream);
int launch_decode_combine(const DecodeKernelParams &p, int dtype, int head_dim, hipStream_t stream);
int launch_decode_chunk(const ChunkKernelParams &p, int dtype, int head_dim, hipStream_t stream);
int launch_decode_varlen(const VarlenKernelParams &p, int dtype, int head_dim, hipStream_t stream);
int launch_decode_chunk_window(const ChunkWindowKernelParams &p, int dtype, int head_dim, hipStream_t stream);
int launch_decode_varlen_window(const VarlenWindowKernelParams &p, int dtype, int head_dim, hipStream_t stream);
int launch_decode_chunk_kv8(const ChunkKv8KernelParams &p, int dtype, int head_dim, hipStream_t stream);
int launch_decode_varlen_kv8(const VarlenKv8KernelParams &p, int dtype, int head_dim, hipStream_t stream);
int launch_decode_chunk_kv8_window(const ChunkKv8WindowKernelParams &p, int dtype, int head_dim, hipStream_t stream);
int launch_decode_varlen_kv8_window(const VarlenKv8WindowKernelParams &p, int dtype, int head_dim, hipStream_t stream);
// decode_kv8_kernel.hip: the attention kernel over e4m3 caches plus the split combine; the 16-bit -> e4m3 row copy
int launch_decode_kv8(const Kv8KernelParams &p, int dtype, int head_dim, hipStream_t stream);
int launch_kv8_quantize(void *dst, const void *src, const float *scale, long long rows, int Hkv, int head_dim,
                        long long src_row, long long src_head, long long dst_row, long long dst_head, int dtype,
                        hipStream_t stream);
// decode_window_kernel.hip: the sliding-window attention kernel (every group size; one body with launch_decode_gqa_mfma's
// kernel, decode_mfma16.h) plus the split combine
int launch_decode_window(const WindowKernelParams &p, int dtype, int head_dim, hipStream_t stream);
// decode_window_sinks_kernel.hip, decode_chunk_window_sinks_kernel.hip, decode_varlen_window_sinks_kernel.hip: the
// windowed kernels with the sink flag of their bodies set
int launch_decode_window_sinks(const WindowSinksKernelParams &p, int dtype, int head_dim, hipStream_t stream);
int launch_decode_chunk_window_sinks(const ChunkWindowSinksKernelParams &p, int dtype, int head_dim, hipStream_t stream);
int launch_decode_varlen_window_sinks(const VarlenWindowSinksKernelParams &p, int dtype, int head_dim, hipStream_t stream);
// decode_kv8_window_kernel.hip: the sliding-window attention kernel over e4m3 caches (one body with launch_decode_kv8's
// kernel, decode_kv8_body.h) plus the split combine
int launch_decode_kv8_window(const Kv8WindowKernelParams &p, int dtype, int head_dim, hipStream_t stream);
// decode_kv8_window_sinks_kernel.hip, decode_chunk_kv8_window_sinks_kernel.hip, decode_varlen_kv8_window_sinks_kernel.hip:
// the windowed kernels over e4m3 caches with the sink flag of their bodies set
int launch_decode_kv8_window_sinks(const Kv8WindowSinksKernelParams &p, int dtype, int head_dim, hipStream_t stream);
int launch_decode_chunk_kv8_window_sinks(const ChunkKv8WindowSinksKernelParams &p, int dtype, int head_dim,
                                         hipStream_t stream);
int launch_decode_varlen_kv8_window_sinks(const VarlenKv8WindowSinksKernelParams &p, int dtype, int head_dim,
                                          hipStream_t stream);
int launch_prefill(const PrefillKernelParams &p, int dtype, int head_dim, bool causal, hipStream_t stream);
int launch_prefill_no_keys(const PrefillKernelParams &p, int head_dim, hipStream_t stream);
// prefill_window_kernel.hip: called by sfa_prefill_window_fwd only (validated dtype, head_dim 64 / 128, Sk > 0)
int launch_prefill_window(const PrefillWindowKernelParams &p, int dtype, int head_dim, hipStream_t stream);
// prefill_split_kernel.hip: called by sfa_prefill_split_fwd only (validated dtype, head_dim 64 / 128, Sk > 0, two or more
// splits): the attention kernel over the split key ranges, then the combine, on the same stream
int launch_prefill_split(const PrefillSplitKernelParams &p, int dtype, int head_dim, bool causal, hipStream_t stream);
int launch_prefill_split_combine(const PrefillSplitKernelParams &p, int dtype, int head_dim, bool causal,
                                 hipStream_t stream);
// prefill_varlen_kernel.hip: called by sfa_prefill_varlen_fwd, and by sfa_prefill_varlen_window_fwd and
// sfa_prefill_varlen_split_fwd where they forward
// (validated dtype, head_dim 64 / 128, B > 0, total_q > 0): the plan kernel, then the attention kernel over the plan, on
// the same stream
int launch_prefill_varlen(const PrefillVarlenKernelParams &p, int dtype, int head_dim, bool causal, hipStream_t stream);
// prefill_varlen_kernel.hip: the plan kernel alone (every slot of p.plan written), for the packed kernels of other units
int launch_prefill_varlen_plan(const PrefillVarlenKernelParams &p, hipStream_t stream);
// prefill_varlen_window_kernel.hip: called by sfa_prefill_varlen_window_fwd only (validated as above, window >= 1): the
// plan kernel, then the windowed attention kernel over the plan, on the same stream
int launch_prefill_varlen_window(const PrefillVarlenWindowKernelParams &p, int dtype, int head_dim, hipStream_t stream);
// prefill_varlen_split_kernel.hip: called by sfa_prefill_varlen_split_fwd only (validated as above, two or more splits):
// the item list from the plan (launch_prefill_varlen_plan comes first), the attention kernel over the items, then the
// combine, on the same stream
int launch_prefill_varlen_split_items(const PrefillVarlenSplitKernelParams &p, bool causal, hipStream_t stream);
int launch_prefill_varlen_split(const PrefillVarlenSplitKernelParams &p, int dtype, int head_dim, bool causal,
                                hipStream_t stream);
int launch_prefill_varlen_split_combine(const PrefillVarlenSplitKernelParams &p, int dtype, int head_dim, bool causal,
                                        hipStream_t stream);
int launch_rotary_table(void *cos_t, void *sin_t, int max_seq_len, int rot_dim, int dtype, hipStream_t stream);
int launch_fill16(void *arr, uint16_t bits, size_t n, hipStream_t stream);

int check_launch(const char *what);

// Test / A-B knobs, set through sfa_debug_set() (include/star_flash_attn.h) and nothing else: the launch
// paths read no environment variable.  -1 = the library's own choice.
struct DebugKnobs {
    std::atomic<int> prefill_impl{-1};      // prefill_dispatch.hip: which prefill kernel (PrefillImpl, prefill_common.h)
    std::atomic<int> prefill_pairs{-1};     // prefill_kernel.hip: balanced q-tile pairs per workgroup (1 or 2)
    std::atomic<int> decode_nt{-1};         // decode_dispatch.hip: 0 / 1 force default / non-temporal cache loads
    std::atomic<int> decode_gqa_mfma{-1};   // decode_dispatch.hip: 0 forces the VALU grouped-query kernel
    std::atomic<int> bm128_one_wg{-1};      // prefill_kernel_bm128.hip: 1 = one workgroup per CU (A/B library only)
    std::atomic<int> last_prefill_kernel{-1};   // written by launch_prefill: what ran last (sfa_debug_get)
    std::atomic<int> last_prefill_splits{-1};   // written by sfa_prefill_split_fwd / sfa_prefill_varlen_split_fwd: the resolved split count (1: forwarded)
};
extern DebugKnobs g_knobs;

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) is a per-DEVICE setting: one of these per kernel
// instantiation (a function-local static) remembers which devices of the process already have it.
struct DynLdsAttr {
    std::atomic<unsigned long long> done{0};
    // SFA_OK, or SFA_ERR_LAUNCH with the HIP error text
    int ensure(const void *func, int bytes, const char *what) {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess) return fail(SFA_ERR_LAUNCH, "%s: hipGetDevice failed", what);
        const unsigned long long bit = 1ull << (dev & 63);
        if (done.load(std::memory_order_relaxed) & bit) return SFA_OK;
        const hipError_t e = hipFuncSetAttribute(func, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
        if (e != hipSuccess)
            return fail(SFA_ERR_LAUNCH, "%s: cannot raise dynamic LDS to %d bytes on device %d: %s", what, bytes, dev,
                        hipGetErrorString(e));
        done.fetch_or(bit, std::memory_order_relaxed);
        return SFA_OK;
    }
};

}  // namespace sfa
