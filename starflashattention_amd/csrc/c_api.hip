// extern "C" entry points of libStarFlashAttention.so (declared in include/star_flash_attn.h).
// Validation, workspace layout and parameter marshalling only; decode_dispatch.hip and prefill_dispatch.hip pick the
// kernels, which live in the decode_*_kernel.hip, prefill_*_kernel.hip and aux_kernels.hip files.  Nothing here
// allocates, copies or synchronises (except sfa_decode_poll_status, which exists to do exactly that).
#include <climits>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "prefill_common.h"
#include "sfa_host.h"

namespace sfa {

static thread_local char g_err[512] = "";

DebugKnobs g_knobs;

void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

int fail(int status, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return status;
}

int check_launch(const char *what) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(SFA_ERR_LAUNCH, "%s: %s", what, hipGetErrorString(e));
    return SFA_OK;
}

static size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

DecodeWorkspace decode_workspace(size_t plan_entries, size_t q_rows, size_t part_rows, int S, int D) {
    DecodeWorkspace w;
    w.plan = kStatusBytes;
    w.q_rot = w.plan + align_up(plan_entries * sizeof(int2), 256);
    w.part_o = w.q_rot + align_up(q_rows * D * sizeof(uint16_t), 256);
    w.part_ml = w.part_o + align_up(part_rows * S * D * sizeof(float), 256);
    w.total = S > 1 ? w.part_ml + align_up(part_rows * S * sizeof(float2), 256) : w.part_o;
    return w;
}

// Split count when the caller does not choose one (num_splits <= 0; the reference hard-codes 4 with a TODO,
// flash_api.cpp:38, flash_attn.cu:1024): split the key range only while the unsplit grid of `wgs` workgroups leaves CUs
// idle -- aim for `target` workgroups, keep every split at least `min_rows` cache rows of memory_max_len long and at
// most 32 splits.  The count is chosen on the host from memory_max_len; the device splits the actual keys, so a split
// past a sequence's keys only writes an empty partial.
static int clamp_splits(long long wgs, long long target, int M, int min_rows) {
    long long s = (target + wgs - 1) / wgs;
    const long long cap = M / min_rows > 1 ? M / min_rows : 1;
    if (s > cap) s = cap;
    if (s > 32) s = 32;
    if (s < 1) s = 1;
    return (int)s;
}

// sfa_decode: one 4-wave workgroup per (b, h, split).  Measured on MI355X (tools/decode_small.py, fp16 D=128): splitting
// pays only while B*H alone leaves most CUs without a workgroup -- B=1 H=32 M=8192: 72.8 us unsplit, 29.1 us at 4-8
// splits, 35.7 at 32; B=2: 74.2 -> 46.8 at 2 splits, 52.0 at 16; from B*H >= 256 on one split is best (the combine kernel
// and the partials cost ~3 us).  Aim for ~128 workgroups, and keep every split at least 2048 cache rows long.
static int auto_splits(int B, int H, int M) { return clamp_splits((long long)B * H, 128, M, 2048); }

// sfa_decode_chunk: the attention kernel runs one 8-wave workgroup per (batch, kv head, 256-row q-tile, split), one per
// CU (its LDS): ~256 workgroups, splits of at least 512 cache rows (8 tiles).
static int chunk_auto_splits(int B, int Hkv, int rows, int M) {
    return clamp_splits((long long)B * Hkv * ((rows + 255) / 256), 256, M, 512);
}

// sfa_decode_varlen: the attention grid is bound * Hkv * S workgroups with bound = total_tokens * G / 256 + batch_size
// plan slots (sfa_host.h); chunk_auto_splits' rule with the workgroup count taken from that bound.
static int varlen_plan_bound(int B, long long rows) { return (int)(rows / 256 + B); }
static int varlen_auto_splits(int B, int Hkv, long long rows, int M) {
    return clamp_splits((long long)varlen_plan_bound(B, rows) * Hkv, 256, M, 512);
}

// The kernel parameters of an (already validated) sfa_decode_args, shared by the three decode entry points; the
// callers place part_o / part_ml in the workspace.
static DecodeKernelParams decode_params(const sfa_decode_args *a, int hkv, int page_shift, int S, long long stride) {
    const long long hd = (long long)hkv * a->head_dim;          // elements per cache row
    DecodeKernelParams p;
    memset(&p, 0, sizeof(p));
    p.qkv = (const uint16_t *)a->qkv;
    p.q_bias = (const uint16_t *)a->q_bias;
    p.k_bias = (const uint16_t *)a->k_bias;
    p.v_bias = (const uint16_t *)a->v_bias;
    p.o = (uint16_t *)a->o;
    p.seq_len = (const int32_t *)a->seq_len;
    p.k_cache = (uint16_t *)a->k_cache_table;
    p.v_cache = (uint16_t *)a->v_cache_table;
    p.cos_tab = (const uint16_t *)a->rotary_cos_table;
    p.sin_tab = (const uint16_t *)a->rotary_sin_table;
    p.status = (int32_t *)a->workspace;
    p.B = a->batch_size;
    p.M = a->memory_max_len;
    p.H = a->num_heads;
    p.Hkv = hkv;
    p.L = a->num_layer;
    p.layer = a->idx_layer;
    p.rot_dim = a->rotary_embedding_dim;
    p.num_splits = S;
    p.qkv_stride = stride;
    if (a->kv_layout == SFA_KV_PAGED) {
        p.kv_row_stride = hd;                   // rows of a page are [page_size, H, D]
        p.kv_head_stride = a->head_dim;
        p.block_table = (const int32_t *)a->block_table;
        p.page_shift = page_shift;
        p.table_stride = a->block_table_stride;
        p.num_pages = a->num_pages;
        p.page_stride = (long long)a->num_layer * a->page_size * hd;
    } else if (a->kv_layout == SFA_KV_BLHMD) {
        p.kv_row_stride = a->head_dim;
        p.kv_head_stride = (long long)a->memory_max_len * a->head_dim;
    } else {
        p.kv_row_stride = hd;
        p.kv_head_stride = a->head_dim;
    }
    const float scale = a->head_dim_inv > 0.f ? a->head_dim_inv : 1.0f / std::sqrt((float)a->head_dim);
    p.scale_log2 = scale * 1.4426950408889634f;
    return p;
}

// A decode entry point, described by data: one of three call shapes in one of six flavours ("Decode host
// pipeline").  decode_call() below is everything the 18 of them do up to the launch.
enum Shape { kSingle, kChunk, kVarlen };    // one token per sequence / `count` tokens per sequence / `count` packed tokens
struct EntryPoint {
    const char *fn;             // names the entry point in the error text
    Shape shape;
    bool window, kv8, sinks;    // a sliding window / e4m3 caches with scales / an attention sink per query head
};
// What differs by shape in the argument checks
struct ShapeRules {
    const char *count_name;     // the token count: num_tokens per sequence, or, packed, total_tokens over all sequences
    bool d256;                  // head_dim 256 passes the shared checks (the single-token fp8 calls refuse it themselves)
    bool token_limits;          // the limits of the chunk kernels: batch_size, 32-bit lane offsets, count * group
    bool packed;                // the tokens of all sequences are packed: no batch stride
};
constexpr ShapeRules kShapeRules[3] = {{"num_tokens", true, false, false},
                                       {"num_tokens", false, true, false},
                                       {"total_tokens", false, true, true}};

// What the entry points check alike, before any HIP call, and what they derive on the way.  sfa_decode is the case of
// one token per sequence (count = 1) with no token stride.
struct DecodeCall {
    int hkv, group, page_shift;
    long long tok, stride;      // elements between tokens / batches of qkv
};
static int validate_decode_call(const EntryPoint &ep, const sfa_decode_args *a, int count, int64_t qkv_token_stride,
                                DecodeCall *out) {
    const char *fn = ep.fn;
    const ShapeRules &e = kShapeRules[ep.shape];
    if (!a) return fail(SFA_ERR_NULL_POINTER, "%s: args is NULL", fn);
    if (!a->qkv || !a->o || !a->seq_len || !a->k_cache_table || !a->v_cache_table)
        return fail(SFA_ERR_NULL_POINTER, "%s: qkv/o/seq_len/k_cache_table/v_cache_table must be non-NULL", fn);
    if ((a->rotary_cos_table == nullptr) != (a->rotary_sin_table == nullptr))
        return fail(SFA_ERR_NULL_POINTER, "%s: give both rotary tables or neither", fn);
    if (count < 0) return fail(SFA_ERR_BAD_SHAPE, "%s: %s=%d < 0", fn, e.count_name, count);
    if (a->batch_size < 0 || (e.token_limits && a->batch_size > 65535) || a->num_heads <= 0 || a->memory_max_len <= 0 ||
        a->num_layer <= 0)
        return fail(SFA_ERR_BAD_SHAPE, "%s: batch_size=%d%s num_heads=%d memory_max_len=%d num_layer=%d", fn,
                    a->batch_size, e.token_limits ? " (<= 65535)" : "", a->num_heads, a->memory_max_len, a->num_layer);
    if (a->idx_layer < 0 || a->idx_layer >= a->num_layer)
        return fail(SFA_ERR_BAD_SHAPE, "%s: idx_layer=%d outside [0, num_layer=%d)", fn, a->idx_layer,
                    a->num_layer);
    if (a->head_dim == 256 && !e.d256)
        return fail(SFA_ERR_UNSUPPORTED_HEAD_DIM,
                    "%s: head_dim 256 is not supported by the chunk path yet (64 or 128; sfa_decode "
                    "serves 256 one token at a time)", fn);
    if (a->head_dim != 64 && a->head_dim != 128 && a->head_dim != 256)
        return fail(SFA_ERR_UNSUPPORTED_HEAD_DIM, "%s: head_dim %d not in {64, 128%s}", fn, a->head_dim,
                    e.d256 ? ", 256" : "");
    if (a->rotary_embedding_dim < 0 || a->rotary_embedding_dim > a->head_dim || (a->rotary_embedding_dim & 1))
        return fail(SFA_ERR_BAD_SHAPE, "%s: rotary_embedding_dim=%d must be even and in [0, head_dim]", fn,
                    a->rotary_embedding_dim);
    if (a->dtype != SFA_DTYPE_FP16 && a->dtype != SFA_DTYPE_BF16)
        return fail(SFA_ERR_BAD_DTYPE, "%s: dtype %d is not fp16(0)/bf16(1)", fn, a->dtype);
    const int hkv = a->num_heads_kv > 0 ? a->num_heads_kv : a->num_heads;
    const int group = hkv > 0 ? a->num_heads / hkv : 0;
    if (a->num_heads_kv < 0 || group * hkv != a->num_heads ||
        (group != 1 && group != 2 && group != 4 && group != 8 && group != 16))
        return fail(SFA_ERR_BAD_SHAPE, "%s: num_heads=%d / num_heads_kv=%d must be 1, 2, 4, 8 or 16", fn,
                    a->num_heads, a->num_heads_kv);
    const long long row = (long long)(a->num_heads + 2 * hkv) * a->head_dim;    // packed q,k,v of one token
    const long long tok = qkv_token_stride > 0 ? qkv_token_stride : row;
    if (tok < row || (tok % 8) != 0)
        return fail(SFA_ERR_BAD_SHAPE,
                    "%s: qkv_token_stride %lld must be >= (H + 2*Hkv)*D and a multiple of 8", fn, tok);
    if (e.packed && a->stride != 0)
        return fail(SFA_ERR_BAD_SHAPE, "%s: args->stride=%d must be 0 (the tokens of all sequences are packed)", fn,
                    a->stride);
    const long long stride = a->stride > 0 ? a->stride : (long long)count * tok;
    if ((count > 0 && stride < (count - 1) * tok + row) || (stride % 8) != 0)
        return fail(SFA_ERR_BAD_SHAPE,
                    "%s: qkv stride %lld must be >= (num_tokens-1)*token_stride + (H + 2*Hkv)*D and a "
                    "multiple of 8", fn, stride);
    // (packed: the plan kernel sums up to 256 sequences' q-tiles of garbage cu_tokens in an int)
    if (e.token_limits && (long long)count * group > (e.packed ? INT_MAX / 2 : INT_MAX))
        return fail(SFA_ERR_BAD_SHAPE, "%s: %s * group = %lld query rows per kv head is too many", fn, e.count_name,
                    (long long)count * group);
    if (a->num_splits > 1024)
        return fail(SFA_ERR_BAD_SHAPE, "%s: num_splits=%d > 1024", fn, a->num_splits);
    if (a->kv_layout != SFA_KV_BLMHD && a->kv_layout != SFA_KV_BLHMD && a->kv_layout != SFA_KV_PAGED)
        return fail(SFA_ERR_BAD_SHAPE,
                    "%s: kv_layout %d is not SFA_KV_BLMHD(0)/SFA_KV_BLHMD(1)/SFA_KV_PAGED(2)", fn, a->kv_layout);
    // the attention kernel addresses the 64 rows of a tile with 32-bit lane offsets
    if (e.token_limits && a->kv_layout != SFA_KV_BLHMD && 128ll * hkv * a->head_dim >= (1ll << 31))
        return fail(SFA_ERR_BAD_SHAPE, "%s: num_heads_kv * head_dim = %lld too large", fn,
                    (long long)hkv * a->head_dim);
    int page_shift = 0;
    if (a->kv_layout == SFA_KV_PAGED) {
        if (!a->block_table) return fail(SFA_ERR_NULL_POINTER, "%s: kv_layout PAGED needs block_table", fn);
        if (a->page_size < 16 || (a->page_size & (a->page_size - 1)))
            return fail(SFA_ERR_BAD_SHAPE, "%s: page_size=%d must be a power of two >= 16", fn, a->page_size);
        while ((1 << page_shift) < a->page_size) ++page_shift;
        if (a->num_pages <= 0 || (long long)a->block_table_stride * a->page_size < (long long)a->memory_max_len)
            return fail(SFA_ERR_BAD_SHAPE,
                        "%s: num_pages=%d, block_table_stride=%d * page_size=%d must cover memory_max_len=%d", fn,
                        a->num_pages, a->block_table_stride, a->page_size, a->memory_max_len);
        if ((uintptr_t)a->block_table & 3)
            return fail(SFA_ERR_BAD_SHAPE, "%s: block_table must be 4-byte aligned", fn);
    }
    const uintptr_t align_or = (uintptr_t)a->qkv | (uintptr_t)a->o | (uintptr_t)a->k_cache_table |
                               (uintptr_t)a->v_cache_table | (uintptr_t)a->q_bias | (uintptr_t)a->k_bias |
                               (uintptr_t)a->v_bias;
    if (align_or & 15) return fail(SFA_ERR_BAD_SHAPE, "%s: tensors must be 16-byte aligned", fn);
    out->hkv = hkv, out->group = group, out->page_shift = page_shift;
    out->tok = tok, out->stride = stride;
    return SFA_OK;
}

// The workspace an entry point was given holds `need` bytes at a 256-byte boundary
static int check_workspace(const EntryPoint &e, const sfa_decode_args *a, size_t need) {
    if (!a->workspace) return fail(SFA_ERR_NULL_POINTER, "%s: workspace is NULL (need %zu bytes)", e.fn, need);
    if (a->workspace_bytes < need)
        return fail(SFA_ERR_WORKSPACE_TOO_SMALL, "%s: workspace has %zu bytes, need %zu", e.fn, a->workspace_bytes, need);
    if ((uintptr_t)a->workspace & 255) return fail(SFA_ERR_BAD_SHAPE, "%s: workspace must be 256-byte aligned", e.fn);
    return SFA_OK;
}

// The rows a sequence can read under a sliding window, which the split count is chosen from instead of memory_max_len:
// min(memory_max_len, window - 1 + count), count = the call's num_tokens / total_tokens, 1 for a single token (the first
// token reads window rows, the last one ends count - 1 rows later).  A short window is not split into slivers, and the
// rule never grows with that argument, so a workspace sized for the call without a window is never too small.
static int window_rows(int M, int window, int count) {
    const long long r = (long long)(window > 1 ? window : 1) - 1 + count;
    return (int)(r < M ? (r > 1 ? r : 1) : M);
}

// (query rows per (batch, kv head) = num_tokens * group; bhr of them in all)
static DecodeWorkspace chunk_workspace(int B, int hkv, long long rows, int S, int D) {
    const size_t bhr = (size_t)B * hkv * rows;
    return decode_workspace(0, bhr, bhr, S, D);
}

// (rows = total_tokens * group packed query rows per kv head)
static DecodeWorkspace varlen_workspace(int B, int hkv, long long rows, int S, int D) {
    const size_t hr = (size_t)hkv * rows;
    return decode_workspace((size_t)varlen_plan_bound(B, rows), hr, hr, S, D);
}

// The arguments an entry point takes beside sfa_decode_args and the stream; one it does not take is 0 / nullptr
// (count: 1 for a single token)
struct DecodeExtras {
    const float *k_scale, *v_scale, *sinks;
    const void *cu_tokens;
    int count;
    int64_t tok_stride;
    int window;
};

constexpr int kRun = 1;     // decode_call: launch (no status is positive)

// Every decode entry point up to the launch: the argument checks, "nothing to do", the split count, the workspace and
// the kernel parameters of the call's shape with their workspace pointers -- out->c.d for a single token, out->c for a
// chunk, *out for varlen (what a shape does not have stays 0).  Returns kRun, SFA_OK (nothing to do) or an error.
// The order of the checks is part of the C ABI's behaviour (an input may break several rules; DESIGN.md, "Decode host
// pipeline", has the table).
static int decode_call(const EntryPoint &e, const sfa_decode_args *a, const DecodeExtras &x, VarlenKernelParams *out) {
    const bool single = e.shape == kSingle, varlen = e.shape == kVarlen;
    const bool bad_scales = e.kv8 && (((uintptr_t)x.k_scale | (uintptr_t)x.v_scale) & 3);
    const int count = x.count;
    DecodeCall dc;
    if (e.sinks && a && ((uintptr_t)x.sinks & 3)) return fail(SFA_ERR_BAD_SHAPE, "%s: sinks must be 4-byte aligned", e.fn);
    // (the varlen fp8 calls check the scales first, the other fp8 calls after the shared checks)
    if (varlen && bad_scales) return fail(SFA_ERR_BAD_SHAPE, "%s: k_scale / v_scale must be 4-byte aligned", e.fn);
    if (varlen && a && !x.cu_tokens) return fail(SFA_ERR_NULL_POINTER, "%s: cu_tokens is NULL", e.fn);
    if (const int rc = validate_decode_call(e, a, count, x.tok_stride, &dc)) return rc;
    if (varlen && ((uintptr_t)x.cu_tokens & 3)) return fail(SFA_ERR_BAD_SHAPE, "%s: cu_tokens must be 4-byte aligned", e.fn);
    if (single && e.kv8 && a->head_dim == 256)
        return fail(SFA_ERR_UNSUPPORTED_HEAD_DIM,
                    "%s: head_dim 256 is not supported over an fp8 cache yet (64 or 128; %s serves 256 on a 16-bit cache)",
                    e.fn, e.window ? "sfa_decode_window" : "sfa_decode");
    if (bad_scales) return fail(SFA_ERR_BAD_SHAPE, "%s: k_scale / v_scale must be 4-byte aligned", e.fn);
    if (e.window && x.window < 1) return fail(SFA_ERR_BAD_SHAPE, "%s: window=%d must be >= 1", e.fn, x.window);
    if (a->batch_size == 0 || count == 0) return SFA_OK;

    const int B = a->batch_size, hkv = dc.hkv, D = a->head_dim;
    const long long rows = (long long)count * dc.group;        // query rows per kv head (varlen: of all sequences)
    const int bound = varlen ? varlen_plan_bound(B, rows) : 0;
    const int M = e.window ? window_rows(a->memory_max_len, x.window, count) : a->memory_max_len;
    // (single token: grouped queries launch one workgroup per kv head, so the split count follows the kv-head count)
    const auto workspace = [&](int S) {
        return single ? decode_workspace(0, 0, (size_t)B * a->num_heads, S, D)
                      : varlen ? varlen_workspace(B, hkv, rows, S, D) : chunk_workspace(B, hkv, rows, S, D);
    };
    int S = a->num_splits > 0 ? a->num_splits
                              : single ? auto_splits(B, hkv, M)
                                       : varlen ? varlen_auto_splits(B, hkv, rows, M) : chunk_auto_splits(B, hkv, (int)rows, M);
    // A caller that left the choice to the library may have sized its workspace for fewer splits than the library picks
    // (sfa_decode_workspace_bytes(..., 0) knows the query-head count only; the windowed sizing functions may be given
    // another window): take the largest split count the workspace holds rather than fail.  The single-token calls and
    // every windowed call do; the chunk and varlen calls without a window do not.
    if ((single || e.window) && a->num_splits <= 0 && a->workspace)
        while (S > 1 && a->workspace_bytes < workspace(S).total) --S;
    // the varlen attention kernel's 1-D grid: one workgroup per (plan slot, kv head, split)
    if (varlen && (long long)bound * hkv * S > INT_MAX)
        return fail(SFA_ERR_BAD_SHAPE,
                    "%s: total_tokens=%d, batch_size=%d, num_heads_kv=%d and num_splits=%d need more than "
                    "2^31 - 1 attention workgroups", e.fn, count, B, hkv, S);
    const DecodeWorkspace w = workspace(S);
    if (const int rc = check_workspace(e, a, w.total)) return rc;

    VarlenKernelParams &p = *out;
    memset(&p, 0, sizeof(p));
    p.c.d = decode_params(a, hkv, dc.page_shift, S, varlen ? 0 : dc.stride);
    char *ws = (char *)a->workspace;
    p.c.d.part_o = (float *)(ws + w.part_o);
    p.c.d.part_ml = (float2 *)(ws + w.part_ml);
    if (single) return kRun;
    p.c.q_rot = (uint16_t *)(ws + w.q_rot);
    p.c.tok_stride = dc.tok;
    p.c.G = dc.group;
    if (varlen) {
        p.cu_tokens = (const int32_t *)x.cu_tokens;
        p.plan = (int2 *)(ws + w.plan);
        p.rows = rows;
        p.total = count;
        p.bound = bound;
    } else {
        p.c.n = count;
        p.c.R = (int)rows;
    }
    return kRun;
}

// The parameter struct P of a chunk or varlen flavour: `base`, the shape's parameters, and behind it the members the
// flavour adds.  A _sinks call without sinks launches its twin, so both structs are filled here, from one source.
template <class P, bool WINDOW, bool KV8, bool SINKS, class Base>
static P flavour_params(const Base &base, const DecodeExtras &x) {
    P p;
    memset(&p, 0, sizeof(p));
    p.base = base;
    if constexpr (WINDOW) p.window = x.window;
    if constexpr (KV8) p.k_scale = x.k_scale, p.v_scale = x.v_scale;
    if constexpr (SINKS) p.sinks = x.sinks;
    return p;
}

// The single-token flavours nest instead: kv8 = {d, scales}, window = {d or kv8, window}, sinks = {window, sinks}
static Kv8KernelParams kv8_params(const DecodeKernelParams &d, const DecodeExtras &x) {
    Kv8KernelParams p;
    memset(&p, 0, sizeof(p));
    p.d = d, p.k_scale = x.k_scale, p.v_scale = x.v_scale;
    return p;
}
static WindowKernelParams window_params(const DecodeKernelParams &d, const DecodeExtras &x) {
    WindowKernelParams p;
    memset(&p, 0, sizeof(p));
    p.d = d, p.window = x.window;
    return p;
}
static Kv8WindowKernelParams kv8_window_params(const DecodeKernelParams &d, const DecodeExtras &x) {
    Kv8WindowKernelParams p;
    memset(&p, 0, sizeof(p));
    p.base = kv8_params(d, x), p.window = x.window;
    return p;
}

}  // namespace sfa

using namespace sfa;

extern "C" {

int sfa_abi_version(void) { return SFA_ABI_VERSION; }

const char *sfa_status_string(int status) {
    switch (status) {
        case SFA_OK: return "ok";
        case SFA_ERR_NULL_POINTER: return "null pointer";
        case SFA_ERR_BAD_SHAPE: return "bad shape";
        case SFA_ERR_BAD_DTYPE: return "bad dtype";
        case SFA_ERR_UNSUPPORTED_HEAD_DIM: return "unsupported head_dim";
        case SFA_ERR_WORKSPACE_TOO_SMALL: return "workspace too small";
        case SFA_ERR_LAUNCH: return "HIP launch failure";
        case SFA_ERR_SEQ_LEN_RANGE: return "seq_len out of range";
        case SFA_ERR_BLOCK_TABLE_RANGE: return "block_table entry out of range";
        default: return "unknown status";
    }
}

const char *sfa_last_error(void) { return g_err; }

int sfa_debug_set(const char *knob, int value) {
    if (!knob) return fail(SFA_ERR_NULL_POINTER, "sfa_debug_set: knob is NULL");
    std::atomic<int> *k = nullptr;
    if (!strcmp(knob, "prefill_impl")) k = &g_knobs.prefill_impl;
    else if (!strcmp(knob, "prefill_pairs")) k = &g_knobs.prefill_pairs;
    else if (!strcmp(knob, "decode_nt")) k = &g_knobs.decode_nt;
    else if (!strcmp(knob, "decode_gqa_mfma")) k = &g_knobs.decode_gqa_mfma;
    else if (!strcmp(knob, "bm128_one_wg")) k = &g_knobs.bm128_one_wg;
    else return fail(SFA_ERR_BAD_SHAPE, "sfa_debug_set: unknown knob '%s'", knob);
#ifndef SFA_WITH_VARIANTS
    if (k == &g_knobs.bm128_one_wg && value > 0)
        return fail(SFA_ERR_BAD_SHAPE, "sfa_debug_set: bm128_one_wg %d needs the diagnostics build of the library", value);
#endif
    k->store(value, std::memory_order_relaxed);
    return SFA_OK;
}

int sfa_debug_get(const char *knob) {
    if (!knob) return INT_MIN;
    if (!strcmp(knob, "prefill_impl")) return g_knobs.prefill_impl.load(std::memory_order_relaxed);
    if (!strcmp(knob, "prefill_pairs")) return g_knobs.prefill_pairs.load(std::memory_order_relaxed);
    if (!strcmp(knob, "decode_nt")) return g_knobs.decode_nt.load(std::memory_order_relaxed);
    if (!strcmp(knob, "decode_gqa_mfma")) return g_knobs.decode_gqa_mfma.load(std::memory_order_relaxed);
    if (!strcmp(knob, "bm128_one_wg")) return g_knobs.bm128_one_wg.load(std::memory_order_relaxed);
    if (!strcmp(knob, "last_prefill_kernel")) return g_knobs.last_prefill_kernel.load(std::memory_order_relaxed);
    if (!strcmp(knob, "last_prefill_splits")) return g_knobs.last_prefill_splits.load(std::memory_order_relaxed);
    return INT_MIN;
}

int sfa_decode_auto_splits(int batch_size, int num_heads, int /*head_dim*/, int memory_max_len) {
    if (batch_size <= 0 || num_heads <= 0 || memory_max_len <= 0) return 1;
    return auto_splits(batch_size, num_heads, memory_max_len);
}

size_t sfa_decode_workspace_bytes(int batch_size, int num_heads, int head_dim, int memory_max_len,
                                  int num_splits) {
    if (batch_size <= 0 || num_heads <= 0 || head_dim <= 0) return kStatusBytes;
    const int S = num_splits > 0 ? num_splits : auto_splits(batch_size, num_heads, memory_max_len);
    return decode_workspace(0, 0, (size_t)batch_size * num_heads, S, head_dim).total;
}

size_t sfa_decode_workspace_bytes_gqa(int batch_size, int num_heads, int num_heads_kv, int head_dim, int memory_max_len,
                                      int num_splits) {
    const int hkv = num_heads_kv > 0 ? num_heads_kv : num_heads;
    const int S = num_splits > 0 ? num_splits : auto_splits(batch_size, hkv, memory_max_len);
    return sfa_decode_workspace_bytes(batch_size, num_heads, head_dim, memory_max_len, S);
}

int sfa_decode_reset_status(void *workspace, void *stream) {
    if (!workspace) return fail(SFA_ERR_NULL_POINTER, "sfa_decode_reset_status: workspace is NULL");
    const hipError_t e = hipMemsetAsync(workspace, 0, kStatusBytes, (hipStream_t)stream);
    if (e != hipSuccess) return fail(SFA_ERR_LAUNCH, "hipMemsetAsync: %s", hipGetErrorString(e));
    return SFA_OK;
}

int sfa_decode_poll_status(const void *workspace, void *stream) {
    if (!workspace) return fail(SFA_ERR_NULL_POINTER, "sfa_decode_poll_status: workspace is NULL");
    int32_t word = 0;
    hipError_t e = hipMemcpyAsync(&word, workspace, sizeof(word), hipMemcpyDeviceToHost, (hipStream_t)stream);
    if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
    if (e != hipSuccess) return fail(SFA_ERR_LAUNCH, "sfa_decode_poll_status: %s", hipGetErrorString(e));
    if (word & 2)
        return fail(SFA_ERR_BLOCK_TABLE_RANGE,
                    "sfa_decode: a block_table entry was outside [0, num_pages); nothing was stored through it and those "
                    "outputs are NaN");
    if (word != 0)
        return fail(SFA_ERR_SEQ_LEN_RANGE,
                    "sfa_decode: some seq_len[b] was outside [0, memory_max_len); those outputs are NaN "
                    "and their cache rows were not written");
    return SFA_OK;
}

// The workspace sizes of the windowed calls: the split count, when the library picks it, is the twin's rule over
// window_rows() instead of memory_max_len.
size_t sfa_decode_window_workspace_bytes(int batch_size, int num_heads, int num_heads_kv, int head_dim,
                                         int memory_max_len, int window, int num_splits) {
    if (batch_size <= 0 || num_heads <= 0 || head_dim <= 0 || memory_max_len <= 0) return kStatusBytes;
    const int hkv = num_heads_kv > 0 ? num_heads_kv : num_heads;
    const int S = num_splits > 0 ? num_splits : auto_splits(batch_size, hkv, window_rows(memory_max_len, window, 1));
    return sfa_decode_workspace_bytes(batch_size, num_heads, head_dim, memory_max_len, S);
}

size_t sfa_decode_chunk_workspace_bytes(int batch_size, int num_heads, int num_heads_kv, int head_dim,
                                        int memory_max_len, int num_tokens, int num_splits) {
    if (batch_size <= 0 || num_heads <= 0 || head_dim <= 0 || num_tokens <= 0) return kStatusBytes;
    const int hkv = num_heads_kv > 0 ? num_heads_kv : num_heads;
    const long long rows = (long long)num_tokens * (num_heads / hkv);
    const int S = num_splits > 0 ? num_splits
                                 : chunk_auto_splits(batch_size, hkv, (int)(rows < INT_MAX ? rows : INT_MAX), memory_max_len);
    return chunk_workspace(batch_size, hkv, rows, S, head_dim).total;
}

size_t sfa_decode_chunk_window_workspace_bytes(int batch_size, int num_heads, int num_heads_kv, int head_dim,
                                               int memory_max_len, int num_tokens, int window, int num_splits) {
    return sfa_decode_chunk_workspace_bytes(batch_size, num_heads, num_heads_kv, head_dim,
                                            window_rows(memory_max_len, window, num_tokens), num_tokens, num_splits);
}

size_t sfa_decode_varlen_workspace_bytes(int batch_size, int num_heads, int num_heads_kv, int head_dim,
                                         int memory_max_len, int total_tokens, int num_splits) {
    if (batch_size <= 0 || num_heads <= 0 || head_dim <= 0 || total_tokens <= 0) return kStatusBytes;
    const int hkv = num_heads_kv > 0 ? num_heads_kv : num_heads;
    const long long rows = (long long)total_tokens * (num_heads / hkv);
    const int S = num_splits > 0 ? num_splits : varlen_auto_splits(batch_size, hkv, rows, memory_max_len);
    return varlen_workspace(batch_size, hkv, rows, S, head_dim).total;
}

size_t sfa_decode_varlen_window_workspace_bytes(int batch_size, int num_heads, int num_heads_kv, int head_dim,
                                                int memory_max_len, int total_tokens, int window, int num_splits) {
    return sfa_decode_varlen_workspace_bytes(batch_size, num_heads, num_heads_kv, head_dim,
                                             window_rows(memory_max_len, window, total_tokens), total_tokens, num_splits);
}

// The 18 decode entry points: describe the call, run decode_call(), fill the flavour's parameter struct and call its
// launcher.  The fp8 calls keep the workspace, the split rule (tuned on 16-bit rows and not re-tuned for one-byte rows)
// and the status word of their 16-bit twins.  A _sinks call with sinks == NULL is its twin, launch and all.


int sfa_decode(const sfa_decode_args *a, void *stream) {
    const DecodeExtras x = {nullptr, nullptr, nullptr, nullptr, 1, 0, 0};
    VarlenKernelParams v;
    if (const int rc = decode_call({"sfa_decode", kSingle, false, false, false}, a, x, &v); rc != kRun) return rc;
    return launch_decode(v.c.d, a->dtype, a->head_dim, (hipStream_t)stream);
}

int sfa_decode_kv8(const sfa_decode_args *a, const float *k_scale, const float *v_scale, void *stream) {
    const DecodeExtras x = {k_scale, v_scale, nullptr, nullptr, 1, 0, 0};
    VarlenKernelParams v;
    if (const int rc = decode_call({"sfa_decode_kv8", kSingle, false, true, false}, a, x, &v); rc != kRun) return rc;
    return launch_decode_kv8(kv8_params(v.c.d, x), a->dtype, a->head_dim, (hipStream_t)stream);
}

int sfa_decode_window(const sfa_decode_args *a, int window, void *stream) {
    const DecodeExtras x = {nullptr, nullptr, nullptr, nullptr, 1, 0, window};
    VarlenKernelParams v;
    if (const int rc = decode_call({"sfa_decode_window", kSingle, true, false, false}, a, x, &v); rc != kRun) return rc;
    return launch_decode_window(window_params(v.c.d, x), a->dtype, a->head_dim, (hipStream_t)stream);
}

int sfa_decode_window_sinks(const sfa_decode_args *a, const float *sinks, int window, void *stream) {
    const DecodeExtras x = {nullptr, nullptr, sinks, nullptr, 1, 0, window};
    VarlenKernelParams v;
    if (const int rc = decode_call({"sfa_decode_window_sinks", kSingle, true, false, true}, a, x, &v); rc != kRun) return rc;
    WindowSinksKernelParams p;
    memset(&p, 0, sizeof(p));
    p.base = window_params(v.c.d, x), p.sinks = sinks;
    return sinks ? launch_decode_window_sinks(p, a->dtype, a->head_dim, (hipStream_t)stream)
                 : launch_decode_window(p.base, a->dtype, a->head_dim, (hipStream_t)stream);
}

int sfa_decode_kv8_window(const sfa_decode_args *a, const float *k_scale, const float *v_scale, int window,
                          void *stream) {
    const DecodeExtras x = {k_scale, v_scale, nullptr, nullptr, 1, 0, window};
    VarlenKernelParams v;
    if (const int rc = decode_call({"sfa_decode_kv8_window", kSingle, true, true, false}, a, x, &v); rc != kRun) return rc;
    return launch_decode_kv8_window(kv8_window_params(v.c.d, x), a->dtype, a->head_dim, (hipStream_t)stream);
}

int sfa_decode_kv8_window_sinks(const sfa_decode_args *a, const float *k_scale, const float *v_scale, const float *sinks,
                                int window, void *stream) {
    const DecodeExtras x = {k_scale, v_scale, sinks, nullptr, 1, 0, window};
    VarlenKernelParams v;
    if (const int rc = decode_call({"sfa_decode_kv8_window_sinks", kSingle, true, true, true}, a, x, &v); rc != kRun)
        return rc;
    Kv8WindowSinksKernelParams p;
    memset(&p, 0, sizeof(p));
    p.base = kv8_window_params(v.c.d, x), p.sinks = sinks;
    return sinks ? launch_decode_kv8_window_sinks(p, a->dtype, a->head_dim, (hipStream_t)stream)
                 : launch_decode_kv8_window(p.base, a->dtype, a->head_dim, (hipStream_t)stream);
}

int sfa_decode_chunk(const sfa_decode_args *a, int num_tokens, int64_t qkv_token_stride, void *stream) {
    const DecodeExtras x = {nullptr, nullptr, nullptr, nullptr, num_tokens, qkv_token_stride, 0};
    VarlenKernelParams v;
    if (const int rc = decode_call({"sfa_decode_chunk", kChunk, false, false, false}, a, x, &v); rc != kRun) return rc;
    return launch_decode_chunk(v.c, a->dtype, a->head_dim, (hipStream_t)stream);
}

int sfa_decode_chunk_kv8(const sfa_decode_args *a, const float *k_scale, const float *v_scale, int num_tokens,
                         int64_t qkv_token_stride, void *stream) {
    const DecodeExtras x = {k_scale, v_scale, nullptr, nullptr, num_tokens, qkv_token_stride, 0};
    VarlenKernelParams v;
    if (const int rc = decode_call({"sfa_decode_chunk_kv8", kChunk, false, true, false}, a, x, &v); rc != kRun) return rc;
    return launch_decode_chunk_kv8(flavour_params<ChunkKv8KernelParams, false, true, false>(v.c, x), a->dtype,
                                   a->head_dim, (hipStream_t)stream);
}

int sfa_decode_chunk_window(const sfa_decode_args *a, int num_tokens, int64_t qkv_token_stride, int window,
                            void *stream) {
    const DecodeExtras x = {nullptr, nullptr, nullptr, nullptr, num_tokens, qkv_token_stride, window};
    VarlenKernelParams v;
    if (const int rc = decode_call({"sfa_decode_chunk_window", kChunk, true, false, false}, a, x, &v); rc != kRun) return rc;
    return launch_decode_chunk_window(flavour_params<ChunkWindowKernelParams, true, false, false>(v.c, x), a->dtype,
                                      a->head_dim, (hipStream_t)stream);
}

int sfa_decode_chunk_window_sinks(const sfa_decode_args *a, const float *sinks, int num_tokens, int64_t qkv_token_stride,
                                  int window, void *stream) {
    const DecodeExtras x = {nullptr, nullptr, sinks, nullptr, num_tokens, qkv_token_stride, window};
    VarlenKernelParams v;
    if (const int rc = decode_call({"sfa_decode_chunk_window_sinks", kChunk, true, false, true}, a, x, &v); rc != kRun)
        return rc;
    if (!sinks)
        return launch_decode_chunk_window(flavour_params<ChunkWindowKernelParams, true, false, false>(v.c, x), a->dtype,
                                          a->head_dim, (hipStream_t)stream);
    return launch_decode_chunk_window_sinks(flavour_params<ChunkWindowSinksKernelParams, true, false, true>(v.c, x),
                                            a->dtype, a->head_dim, (hipStream_t)stream);
}

int sfa_decode_chunk_kv8_window(const sfa_decode_args *a, const float *k_scale, const float *v_scale, int num_tokens,
                                int64_t qkv_token_stride, int window, void *stream) {
    const DecodeExtras x = {k_scale, v_scale, nullptr, nullptr, num_tokens, qkv_token_stride, window};
    VarlenKernelParams v;
    if (const int rc = decode_call({"sfa_decode_chunk_kv8_window", kChunk, true, true, false}, a, x, &v); rc != kRun)
        return rc;
    return launch_decode_chunk_kv8_window(flavour_params<ChunkKv8WindowKernelParams, true, true, false>(v.c, x), a->dtype,
                                          a->head_dim, (hipStream_t)stream);
}

int sfa_decode_chunk_kv8_window_sinks(const sfa_decode_args *a, const float *k_scale, const float *v_scale,
                                      const float *sinks, int num_tokens, int64_t qkv_token_stride, int window,
                                      void *stream) {
    const DecodeExtras x = {k_scale, v_scale, sinks, nullptr, num_tokens, qkv_token_stride, window};
    VarlenKernelParams v;
    if (const int rc = decode_call({"sfa_decode_chunk_kv8_window_sinks", kChunk, true, true, true}, a, x, &v); rc != kRun)
        return rc;
    if (!sinks)
        return launch_decode_chunk_kv8_window(flavour_params<ChunkKv8WindowKernelParams, true, true, false>(v.c, x),
                                              a->dtype, a->head_dim, (hipStream_t)stream);
    return launch_decode_chunk_kv8_window_sinks(flavour_params<ChunkKv8WindowSinksKernelParams, true, true, true>(v.c, x),
                                                a->dtype, a->head_dim, (hipStream_t)stream);
}

int sfa_decode_varlen(const sfa_decode_args *a, const void *cu_tokens, int total_tokens, int64_t qkv_token_stride,
                      void *stream) {
    const DecodeExtras x = {nullptr, nullptr, nullptr, cu_tokens, total_tokens, qkv_token_stride, 0};
    VarlenKernelParams v;
    if (const int rc = decode_call({"sfa_decode_varlen", kVarlen, false, false, false}, a, x, &v); rc != kRun) return rc;
    return launch_decode_varlen(v, a->dtype, a->head_dim, (hipStream_t)stream);
}

int sfa_decode_varlen_kv8(const sfa_decode_args *a, const float *k_scale, const float *v_scale, const void *cu_tokens,
                          int total_tokens, int64_t qkv_token_stride, void *stream) {
    const DecodeExtras x = {k_scale, v_scale, nullptr, cu_tokens, total_tokens, qkv_token_stride, 0};
    VarlenKernelParams v;
    if (const int rc = decode_call({"sfa_decode_varlen_kv8", kVarlen, false, true, false}, a, x, &v); rc != kRun) return rc;
    return launch_decode_varlen_kv8(flavour_params<VarlenKv8KernelParams, false, true, false>(v, x), a->dtype,
                                    a->head_dim, (hipStream_t)stream);
}

int sfa_decode_varlen_window(const sfa_decode_args *a, const void *cu_tokens, int total_tokens, int64_t qkv_token_stride,
                             int window, void *stream) {
    const DecodeExtras x = {nullptr, nullptr, nullptr, cu_tokens, total_tokens, qkv_token_stride, window};
    VarlenKernelParams v;
    if (const int rc = decode_call({"sfa_decode_varlen_window", kVarlen, true, false, false}, a, x, &v); rc != kRun)
        return rc;
    return launch_decode_varlen_window(flavour_params<VarlenWindowKernelParams, true, false, false>(v, x), a->dtype,
                                       a->head_dim, (hipStream_t)stream);
}

int sfa_decode_varlen_window_sinks(const sfa_decode_args *a, const float *sinks, const void *cu_tokens, int total_tokens,
                                   int64_t qkv_token_stride, int window, void *stream) {
    const DecodeExtras x = {nullptr, nullptr, sinks, cu_tokens, total_tokens, qkv_token_stride, window};
    VarlenKernelParams v;
    if (const int rc = decode_call({"sfa_decode_varlen_window_sinks", kVarlen, true, false, true}, a, x, &v); rc != kRun)
        return rc;
    if (!sinks)
        return launch_decode_varlen_window(flavour_params<VarlenWindowKernelParams, true, false, false>(v, x), a->dtype,
                                           a->head_dim, (hipStream_t)stream);
    return launch_decode_varlen_window_sinks(flavour_params<VarlenWindowSinksKernelParams, true, false, true>(v, x),
                                             a->dtype, a->head_dim, (hipStream_t)stream);
}

int sfa_decode_varlen_kv8_window(const sfa_decode_args *a, const float *k_scale, const float *v_scale,
                                 const void *cu_tokens, int total_tokens, int64_t qkv_token_stride, int window,
                                 void *stream) {
    const DecodeExtras x = {k_scale, v_scale, nullptr, cu_tokens, total_tokens, qkv_token_stride, window};
    VarlenKernelParams v;
    if (const int rc = decode_call({"sfa_decode_varlen_kv8_window", kVarlen, true, true, false}, a, x, &v); rc != kRun)
        return rc;
    return launch_decode_varlen_kv8_window(flavour_params<VarlenKv8WindowKernelParams, true, true, false>(v, x), a->dtype,
                                           a->head_dim, (hipStream_t)stream);
}

int sfa_decode_varlen_kv8_window_sinks(const sfa_decode_args *a, const float *k_scale, const float *v_scale,
                                       const float *sinks, const void *cu_tokens, int total_tokens,
                                       int64_t qkv_token_stride, int window, void *stream) {
    const DecodeExtras x = {k_scale, v_scale, sinks, cu_tokens, total_tokens, qkv_token_stride, window};
    VarlenKernelParams v;
    if (const int rc = decode_call({"sfa_decode_varlen_kv8_window_sinks", kVarlen, true, true, true}, a, x, &v); rc != kRun)
        return rc;
    if (!sinks)
        return launch_decode_varlen_kv8_window(flavour_params<VarlenKv8WindowKernelParams, true, true, false>(v, x),
                                               a->dtype, a->head_dim, (hipStream_t)stream);
    return launch_decode_varlen_kv8_window_sinks(flavour_params<VarlenKv8WindowSinksKernelParams, true, true, true>(v, x),
                                                 a->dtype, a->head_dim, (hipStream_t)stream);
}

int sfa_kv8_quantize(void *dst, const void *src, const float *scale, int64_t rows, int num_heads_kv, int head_dim,
                     int64_t src_row_stride, int64_t src_head_stride, int64_t dst_row_stride, int64_t dst_head_stride,
                     int dtype, void *stream) {
    if (!dst || !src) return fail(SFA_ERR_NULL_POINTER, "sfa_kv8_quantize: dst/src must be non-NULL");
    if (rows < 0 || num_heads_kv <= 0)
        return fail(SFA_ERR_BAD_SHAPE, "sfa_kv8_quantize: rows=%lld num_heads_kv=%d", (long long)rows, num_heads_kv);
    if (head_dim != 64 && head_dim != 128)
        return fail(SFA_ERR_UNSUPPORTED_HEAD_DIM, "sfa_kv8_quantize: head_dim %d not in {64, 128}", head_dim);
    if (dtype != SFA_DTYPE_FP16 && dtype != SFA_DTYPE_BF16)
        return fail(SFA_ERR_BAD_DTYPE, "sfa_kv8_quantize: dtype %d is not fp16(0)/bf16(1)", dtype);
    const int64_t st[4] = {src_row_stride, src_head_stride, dst_row_stride, dst_head_stride};
    for (int i = 0; i < 4; ++i)
        if (st[i] < 0 || (st[i] % 16) != 0)
            return fail(SFA_ERR_BAD_SHAPE, "sfa_kv8_quantize: strides must be >= 0 and multiples of 16 elements");
    if (((uintptr_t)dst | (uintptr_t)src) & 15)
        return fail(SFA_ERR_BAD_SHAPE, "sfa_kv8_quantize: dst and src must be 16-byte aligned");
    if ((uintptr_t)scale & 3) return fail(SFA_ERR_BAD_SHAPE, "sfa_kv8_quantize: scale must be 4-byte aligned");
    return launch_kv8_quantize(dst, src, scale, rows, num_heads_kv, head_dim, src_row_stride, src_head_stride,
                               dst_row_stride, dst_head_stride, dtype, (hipStream_t)stream);
}

}  // extern "C"

namespace {

// What sfa_prefill_fwd, sfa_prefill_window_fwd and sfa_prefill_split_fwd check and marshal alike, under the name of the call.  d256:
// sfa_prefill_fwd itself -- head_dim 256 is served, and the K / V seq stride is checked by launch_prefill against the kernel
// it picks; the other two run prefill_stream.h's 64-key tiles (or forward to kernels with the same limit or a wider one)
// and check it here.  Returns a status; *launch is false where there is nothing to do (batch or seqlen_q of 0).  p->nq_tiles
// and p->bh_per_xcd are set for seqlen_k > 0.
int prefill_call(const char *name, const sfa_prefill_args *a, bool d256, PrefillKernelParams *pp, bool *launch) {
    *launch = false;
    if (!a) return fail(SFA_ERR_NULL_POINTER, "%s: args is NULL", name);
    if (!a->q || !a->k || !a->v || !a->o)
        return fail(SFA_ERR_NULL_POINTER, "%s: q/k/v/o must be non-NULL", name);
    if (a->batch < 0 || a->heads_q <= 0 || a->heads_kv <= 0 || a->seqlen_q < 0 || a->seqlen_k < 0)
        return fail(SFA_ERR_BAD_SHAPE, "%s: batch=%d heads_q=%d heads_kv=%d seqlen_q=%d seqlen_k=%d", name,
                    a->batch, a->heads_q, a->heads_kv, a->seqlen_q, a->seqlen_k);
    if (a->heads_q % a->heads_kv)
        return fail(SFA_ERR_BAD_SHAPE, "%s: heads_q=%d not a multiple of heads_kv=%d", name, a->heads_q, a->heads_kv);
    if (a->head_dim != 64 && a->head_dim != 128 && !(d256 && a->head_dim == 256))
        return fail(SFA_ERR_UNSUPPORTED_HEAD_DIM, "%s: head_dim %d not in {64, 128%s}", name, a->head_dim, d256 ? ", 256" : "");
    if (a->dtype != SFA_DTYPE_FP16 && a->dtype != SFA_DTYPE_BF16)
        return fail(SFA_ERR_BAD_DTYPE, "%s: dtype %d is not fp16(0)/bf16(1)", name, a->dtype);
    const int64_t *st[4] = {a->q_stride, a->k_stride, a->v_stride, a->o_stride};
    for (int t = 0; t < 4; ++t)
        for (int i = 0; i < 3; ++i)
            if (st[t][i] < 0 || (st[t][i] % 8) != 0)
                return fail(SFA_ERR_BAD_SHAPE, "%s: strides must be >= 0 and multiples of 8 elements", name);
    if (!d256)
        if (const int rc = check_prefill_kv_pitch(name, "seq", a->k_stride[2], a->v_stride[2], prefill::kBN, a->head_dim))
            return rc;
    if (((uintptr_t)a->q | (uintptr_t)a->k | (uintptr_t)a->v | (uintptr_t)a->o) & 15)
        return fail(SFA_ERR_BAD_SHAPE, "%s: tensors must be 16-byte aligned", name);
    if ((long long)a->batch * a->heads_q > (1ll << 24))
        return fail(SFA_ERR_BAD_SHAPE, "%s: batch*heads_q too large", name);
    if (a->batch == 0 || a->seqlen_q == 0) return SFA_OK;

    PrefillKernelParams &p = *pp;
    memset(&p, 0, sizeof(p));
    p.q = (const uint16_t *)a->q;
    p.k = (const uint16_t *)a->k;
    p.v = (const uint16_t *)a->v;
    p.o = (uint16_t *)a->o;
    p.lse = a->lse;
    p.fast_scale = a->fast_scale != 0 && a->lse == nullptr;
    p.B = a->batch;
    p.Hq = a->heads_q;
    p.Hkv = a->heads_kv;
    p.Sq = a->seqlen_q;
    p.Sk = a->seqlen_k;
    for (int i = 0; i < 3; ++i) {
        p.qs[i] = a->q_stride[i];
        p.ks[i] = a->k_stride[i];
        p.vs[i] = a->v_stride[i];
        p.os[i] = a->o_stride[i];
    }
    const float scale = a->softmax_scale > 0.f ? a->softmax_scale : 1.0f / std::sqrt((float)a->head_dim);
    p.scale_log2 = scale * 1.4426950408889634f;
    *launch = true;
    if (a->seqlen_k == 0) return SFA_OK;
    p.nq_tiles = (a->seqlen_q + 255) / 256;
    p.bh_per_xcd = (a->batch * a->heads_q + 7) / 8;
    if ((long long)8 * p.bh_per_xcd * p.nq_tiles > 0x7fffffffll)
        return fail(SFA_ERR_BAD_SHAPE, "%s: grid too large", name);
    return SFA_OK;
}

// ---- sfa_prefill_split_fwd: the partition, the workspace and the auto rule (include/star_flash_attn.h) ----
constexpr int kSplitTile = 64, kSplitRows = 256;    // prefill_split_kernel.hip's key tile and q-tile

int split_key_tiles(int seqlen_k) { return (seqlen_k + kSplitTile - 1) / kSplitTile; }
// a request for S >= 1 splits of nkt >= 1 tiles: C = ceil(nkt / S) tiles per split, S' = ceil(nkt / C) splits
int split_chunk(int nkt, int S) { return (nkt + S - 1) / S; }
int split_resolve(int nkt, int S) {
    if (nkt <= 0) return 1;
    const int C = split_chunk(nkt, S < nkt ? S : nkt);
    return (nkt + C - 1) / C;
}
// partial rows of `splits` resolved splits: every q-tile has 256 of them per split; each is head_dim + 2 floats
size_t split_bytes(int batch, int heads_q, int seqlen_q, int head_dim, int splits) {
    if (splits <= 1) return 0;
    const size_t rows = (size_t)batch * heads_q * ((seqlen_q + kSplitRows - 1) / kSplitRows) * splits * kSplitRows;
    return rows * (head_dim + 2) * sizeof(float);   // (a multiple of 256: rows is one of 256)
}

// The auto rule.  A split pays only while the grid leaves compute units idle: with batch * heads_q * q-tiles workgroups
// for 256 units it takes the smallest count that fills them, as long as every split keeps kSplitMinTiles key tiles, and at
// most kSplitMaxSplits.  Measured (tools/prefill_split_bench.py, profiles/prefill_split_sweep.txt, bf16, head_dim 128):
//   * The rule's count is the best or within 2 % of the best explicit count on every line where it splits: 64 q-tiles
//     against 32768 keys 4 splits (263 us; 2: 394, 8: 276; unsplit 624), against 8192 keys 4 (81; unsplit 159); 32
//     q-tiles against 32768 keys 8 (147; 4: 214, 16: 166; unsplit 619); 128 q-tiles of S = 4096, 2 (causal 67 against 84,
//     full 82 against 89).  From 256 q-tiles on every explicit count loses (S = 4096, 16 heads: +18 % causal, +29 % full
//     at 2 splits; 32 heads +69 % / +30 %; 4 x 32 heads +69 %), as it does where the persistent kernel already balances
//     a causal grid (4 heads of S = 16384: +39 %) and on short rows (4 x 16 heads of S = 1024, head_dim 64: +51 %):
//     the rule returns 1 on all of them.
//   * Minimum chunk (--probe: 8 workgroups, so every count fits the chip at once): chunks of 8 tiles are the best or
//     within 3 % of it at 16, 32, 64 and 128 key tiles (split / unsplit 0.98, 0.62, 0.40, 0.25); 4 tiles tie at 16 and 32
//     tiles and are 15 % slower at 64; 1 tile loses to the unsplit call (1.34).  So 8, the starting value, stays.
//   * Cap: 16 is the largest count any line measured (40.6 us against 42.5 at 8 for 8 q-tiles against 8192 keys); no
//     line has reached a larger one, so the cap is what has been measured, not the 32 it started from.
constexpr int kSplitMinTiles = 8, kSplitMaxSplits = 16;
int split_auto(int batch, int heads_q, int seqlen_q, int seqlen_k) {
    if (batch <= 0 || heads_q <= 0 || seqlen_q <= 0 || seqlen_k <= 0) return 1;
    const long long wgs = (long long)batch * heads_q * ((seqlen_q + kSplitRows - 1) / kSplitRows);
    if (wgs >= 256) return 1;
    const int nkt = split_key_tiles(seqlen_k);
    long long S = (256 + wgs - 1) / wgs;
    if (S > nkt / kSplitMinTiles) S = nkt / kSplitMinTiles;
    if (S > kSplitMaxSplits) S = kSplitMaxSplits;
    return S < 2 ? 1 : split_resolve(nkt, (int)S);
}

// ---- sfa_prefill_varlen_split_fwd: the partition, the workspace and the auto rule (include/star_flash_attn.h) ----
// (64-bit: max_seqlen_k is any int >= 1)
int varlen_split_key_tiles(int max_seqlen_k) { return (int)(((long long)max_seqlen_k + kSplitTile - 1) / kSplitTile); }
size_t varlen_plan_bytes(int batch, int total_q) {
    return align_up(((size_t)total_q / 256 + (size_t)batch) * sizeof(int2), 256);
}
// the three regions for `splits` resolved splits (1: the plan alone); saturates, a multiple of 256 all the same
size_t varlen_split_bytes(int batch, int heads_q, int total_q, int head_dim, int splits) {
    const size_t plan = varlen_plan_bytes(batch, total_q);
    if (splits <= 1) return plan;
    const size_t bound = (size_t)total_q / 256 + (size_t)batch;
    size_t items, rows, part, sum;
    if (__builtin_mul_overflow(bound * sizeof(int2), (size_t)splits, &items) ||
        __builtin_mul_overflow(bound * (size_t)heads_q, (size_t)splits * kSplitRows, &rows) ||
        __builtin_mul_overflow(rows, (size_t)(head_dim + 2) * sizeof(float), &part) ||      // (a multiple of 256: rows is)
        __builtin_add_overflow(part, plan + align_up(items, 256), &sum))
        return ~(size_t)255;
    return sum;
}
// split_auto's rule and constants on what the host knows of a packed batch: heads_q * ceil(total_q / 256) workgroups (the
// q-tiles of one sequence of total_q rows; the real count is up to batch - 1 larger) and ceil(max_seqlen_k / 64) tiles.
// The constants were measured on rectangular problems (above); what the packed sweep says about them is in DESIGN 5.24
// (tools/prefill_varlen_split_bench.py, profiles/prefill_varlen_split_sweep.txt).
int varlen_split_auto(int batch, int heads_q, int total_q, int max_seqlen_k) {
    if (batch <= 0) return 1;
    return split_auto(1, heads_q, total_q, max_seqlen_k < INT_MAX - kSplitTile ? max_seqlen_k : INT_MAX - kSplitTile);
}

// ---- sfa_prefill_varlen_fwd / sfa_prefill_varlen_window_fwd / sfa_prefill_varlen_split_fwd ----
struct PrefillVarlenWindow { int window; const float *sinks; };     // what the windowed call adds to the checks
// what the split call adds: its two arguments; out: the resolved count
struct PrefillVarlenSplit { int max_seqlen_k, num_splits; int resolved; };

// What the packed prefill calls check and marshal alike, under the name of the call; w: the windowed call's arguments,
// s: the split call's, checked directly after the alignment step.  With s the workspace checks are those of the resolved
// count (s->resolved), and the grid check covers the split's two grids.  Returns a status; *launch is false where there is
// nothing to do (batch or total_q of 0).
int prefill_varlen_call(const char *name, const sfa_prefill_varlen_args *a, const PrefillVarlenWindow *w,
                        PrefillVarlenSplit *s, void *workspace, size_t workspace_bytes, PrefillVarlenKernelParams *pp,
                        bool *launch) {
    *launch = false;
    if (!a) return fail(SFA_ERR_NULL_POINTER, "%s: args is NULL", name);
    if (!a->q || !a->k || !a->v || !a->o || !a->cu_seqlens_q || !a->cu_seqlens_k)
        return fail(SFA_ERR_NULL_POINTER, "%s: q/k/v/o/cu_seqlens_q/cu_seqlens_k must be non-NULL", name);
    if (a->batch < 0 || a->heads_q <= 0 || a->heads_kv <= 0 || a->total_q < 0 || a->total_k < 0)
        return fail(SFA_ERR_BAD_SHAPE, "%s: batch=%d heads_q=%d heads_kv=%d total_q=%d total_k=%d", name, a->batch,
                    a->heads_q, a->heads_kv, a->total_q, a->total_k);
    if (a->heads_q % a->heads_kv)
        return fail(SFA_ERR_BAD_SHAPE, "%s: heads_q=%d not a multiple of heads_kv=%d", name, a->heads_q, a->heads_kv);
    if (a->head_dim != 64 && a->head_dim != 128)
        return fail(SFA_ERR_UNSUPPORTED_HEAD_DIM, "%s: head_dim %d not in {64, 128}%s", name, a->head_dim,
                    a->head_dim == 256 ? " (sfa_prefill_fwd serves head_dim 256)" : "");
    if (a->dtype != SFA_DTYPE_FP16 && a->dtype != SFA_DTYPE_BF16)
        return fail(SFA_ERR_BAD_DTYPE, "%s: dtype %d is not fp16(0)/bf16(1)", name, a->dtype);
    const int64_t *st[4] = {a->q_stride, a->k_stride, a->v_stride, a->o_stride};
    for (int t = 0; t < 4; ++t)
        for (int i = 0; i < 2; ++i)
            if (st[t][i] < 0 || (st[t][i] % 8) != 0)
                return fail(SFA_ERR_BAD_SHAPE, "%s: strides must be >= 0 and multiples of 8 elements", name);
    // (the packed kernels all walk prefill_stream.h's 64-key tiles)
    if (const int rc = check_prefill_kv_pitch(name, "token", a->k_stride[0], a->v_stride[0], prefill::kBN, a->head_dim))
        return rc;
    if (((uintptr_t)a->q | (uintptr_t)a->k | (uintptr_t)a->v | (uintptr_t)a->o) & 15)
        return fail(SFA_ERR_BAD_SHAPE, "%s: tensors must be 16-byte aligned", name);
    if (((uintptr_t)a->cu_seqlens_q | (uintptr_t)a->cu_seqlens_k | (uintptr_t)a->lse) & 3)
        return fail(SFA_ERR_BAD_SHAPE, "%s: cu_seqlens_q, cu_seqlens_k and lse must be 4-byte aligned", name);
    if (w) {
        if ((uintptr_t)w->sinks & 3) return fail(SFA_ERR_BAD_SHAPE, "%s: sinks must be 4-byte aligned", name);
        if (!a->causal)
            return fail(SFA_ERR_BAD_SHAPE, "%s: causal must be non-zero (a two-sided window is not served)", name);
        if (w->window < 1) return fail(SFA_ERR_BAD_SHAPE, "%s: window=%d must be >= 1", name, w->window);
    }
    if (s && s->max_seqlen_k < 1)
        return fail(SFA_ERR_BAD_SHAPE, "%s: max_seqlen_k=%d must be >= 1", name, s->max_seqlen_k);
    if (a->batch == 0 || a->total_q == 0) return SFA_OK;
    int S = 1;      // the resolved split count
    if (s) {
        const int nkt = varlen_split_key_tiles(s->max_seqlen_k);
        if (s->num_splits >= 1) {
            S = split_resolve(nkt, s->num_splits);
        } else {
            // the library's choice, or the largest count the workspace holds (none: 1), as in sfa_prefill_split_fwd
            S = varlen_split_auto(a->batch, a->heads_q, a->total_q, s->max_seqlen_k);
            if (workspace || workspace_bytes == 0)
                while (S > 1 && varlen_split_bytes(a->batch, a->heads_q, a->total_q, a->head_dim, S) > workspace_bytes)
                    S = split_resolve(nkt, S - 1);
        }
        s->resolved = S;
    }
    if (!workspace) return fail(SFA_ERR_NULL_POINTER, "%s: workspace is NULL", name);
    if ((uintptr_t)workspace & 255) return fail(SFA_ERR_BAD_SHAPE, "%s: workspace must be 256-byte aligned", name);
    const size_t need = varlen_split_bytes(a->batch, a->heads_q, a->total_q, a->head_dim, S);
    if (workspace_bytes < need)
        return fail(SFA_ERR_WORKSPACE_TOO_SMALL, "%s: workspace has %zu bytes, need %zu", name, workspace_bytes, need);
    const long long bound = (long long)a->total_q / 256 + a->batch;
    // (with splits: an attention workgroup per item slot and head, head_dim / 4 combine blocks per plan slot and head)
    const long long per_wg = S > 1 ? (S > a->head_dim / 4 ? S : a->head_dim / 4) : 1;
    if (bound * a->heads_q > 0x7fffffffll || bound * a->heads_q * per_wg > 0x7fffffffll)
        return fail(SFA_ERR_BAD_SHAPE, "%s: grid too large", name);

    PrefillVarlenKernelParams &p = *pp;
    memset(&p, 0, sizeof(p));
    p.q = (const uint16_t *)a->q;
    p.k = (const uint16_t *)a->k;
    p.v = (const uint16_t *)a->v;
    p.o = (uint16_t *)a->o;
    p.lse = a->lse;
    p.cu_q = (const int32_t *)a->cu_seqlens_q;
    p.cu_k = (const int32_t *)a->cu_seqlens_k;
    p.plan = (int2 *)workspace;
    p.B = a->batch;
    p.Hq = a->heads_q;
    p.Hkv = a->heads_kv;
    p.total_q = a->total_q;
    p.total_k = a->total_k;
    p.bound = (int)bound;
    p.slices = a->heads_q % 8 == 0 ? 8 : 1;
    for (int i = 0; i < 2; ++i) {
        p.qs[i] = a->q_stride[i];
        p.ks[i] = a->k_stride[i];
        p.vs[i] = a->v_stride[i];
        p.os[i] = a->o_stride[i];
    }
    const float scale = a->softmax_scale > 0.f ? a->softmax_scale : 1.0f / std::sqrt((float)a->head_dim);
    p.scale_log2 = scale * 1.4426950408889634f;
    *launch = true;
    return SFA_OK;
}

}  // namespace

extern "C" {

size_t sfa_prefill_split_workspace_bytes(int batch, int heads_q, int seqlen_q, int seqlen_k, int head_dim, int causal,
                                         int num_splits) {
    (void)causal;
    if (batch <= 0 || heads_q <= 0 || seqlen_q <= 0 || seqlen_k <= 0 || (head_dim != 64 && head_dim != 128)) return 0;
    const int S = num_splits >= 1 ? split_resolve(split_key_tiles(seqlen_k), num_splits)
                                  : split_auto(batch, heads_q, seqlen_q, seqlen_k);
    return split_bytes(batch, heads_q, seqlen_q, head_dim, S);
}

int sfa_prefill_auto_splits(int batch, int heads_q, int seqlen_q, int seqlen_k, int head_dim, int causal) {
    (void)head_dim;
    (void)causal;
    return split_auto(batch, heads_q, seqlen_q, seqlen_k);
}

// sfa_prefill_fwd with each q-tile's key range cut into splits.  A resolved count of 1: the call is sfa_prefill_fwd's,
// launch and all
int sfa_prefill_split_fwd(const sfa_prefill_args *a, int num_splits, void *workspace, size_t workspace_bytes,
                          void *stream) {
    static const char *const name = "sfa_prefill_split_fwd";
    PrefillSplitKernelParams sp;
    bool launch;
    if (const int rc = prefill_call(name, a, false, &sp.base, &launch)) return rc;
    if (!launch) return SFA_OK;
    // ---- the resolved count ----
    const int nkt = split_key_tiles(a->seqlen_k);
    int S;
    if (num_splits >= 1) {
        S = split_resolve(nkt, num_splits);
    } else {
        // the library's choice, or the largest count the workspace holds (none: 1), as in the decode calls
        S = split_auto(a->batch, a->heads_q, a->seqlen_q, a->seqlen_k);
        if (workspace || workspace_bytes == 0)
            while (S > 1 && split_bytes(a->batch, a->heads_q, a->seqlen_q, a->head_dim, S) > workspace_bytes)
                S = split_resolve(nkt, S - 1);
    }
    if (S > 1) {
        if (!workspace) return fail(SFA_ERR_NULL_POINTER, "%s: workspace is NULL (%d splits)", name, S);
        if ((uintptr_t)workspace & 255) return fail(SFA_ERR_BAD_SHAPE, "%s: workspace must be 256-byte aligned", name);
        const size_t need = split_bytes(a->batch, a->heads_q, a->seqlen_q, a->head_dim, S);
        if (workspace_bytes < need)
            return fail(SFA_ERR_WORKSPACE_TOO_SMALL, "%s: workspace has %zu bytes, need %zu", name, workspace_bytes, need);
        const long long combine_blocks = (long long)a->batch * a->heads_q * ((a->seqlen_q + 7) / 8);
        if ((long long)8 * sp.base.bh_per_xcd * sp.base.nq_tiles * S > 0x7fffffffll || combine_blocks > 0x7fffffffll)
            return fail(SFA_ERR_BAD_SHAPE, "%s: grid too large", name);
    }
    g_knobs.last_prefill_splits.store(S, std::memory_order_relaxed);
    if (a->seqlen_k == 0)       // no keys: every row is empty -> zeros, lse = -inf
        return launch_prefill_no_keys(sp.base, a->head_dim, (hipStream_t)stream);
    if (S == 1) return launch_prefill(sp.base, a->dtype, a->head_dim, a->causal != 0, (hipStream_t)stream);
    sp.base.fast_scale = 0;
    sp.num_splits = S;
    sp.tiles_per_split = split_chunk(nkt, num_splits >= 1 && num_splits < nkt ? num_splits : S);
    const size_t rows = (size_t)a->batch * a->heads_q * sp.base.nq_tiles * S * kSplitRows;
    sp.part_o = (float *)workspace;
    sp.part_ml = (float2 *)((char *)workspace + rows * a->head_dim * sizeof(float));
    if (const int rc = launch_prefill_split(sp, a->dtype, a->head_dim, a->causal != 0, (hipStream_t)stream)) return rc;
    return launch_prefill_split_combine(sp, a->dtype, a->head_dim, a->causal != 0, (hipStream_t)stream);
}

// ---- sfa_prefill_varlen_fwd: packed sequences of different lengths (prefill_varlen_kernel.hip) ----
// The workspace is the plan alone: one int2 per work-item slot, total_q / 256 + batch of them (every sequence with rows
// has ceil(n_q / 256) <= n_q / 256 + 1 q-tiles, and the n_q / 256 sum to at most total_q / 256).
size_t sfa_prefill_varlen_workspace_bytes(int batch, int total_q) {
    if (batch <= 0 || total_q <= 0) return 0;
    return varlen_plan_bytes(batch, total_q);
}

int sfa_prefill_varlen_fwd(const sfa_prefill_varlen_args *a, void *workspace, size_t workspace_bytes, void *stream) {
    PrefillVarlenKernelParams p;
    bool launch;
    if (const int rc = prefill_varlen_call("sfa_prefill_varlen_fwd", a, nullptr, nullptr, workspace, workspace_bytes, &p, &launch))
        return rc;
    if (!launch) return SFA_OK;
    return launch_prefill_varlen(p, a->dtype, a->head_dim, a->causal != 0, (hipStream_t)stream);
}

// sfa_prefill_varlen_fwd under a sliding window, with an optional attention sink per query head.  No sink and a window
// that covers every key of the batch: the call is sfa_prefill_varlen_fwd's (causal), launch and all
int sfa_prefill_varlen_window_fwd(const sfa_prefill_varlen_args *a, int window, const float *sinks, void *workspace,
                                  size_t workspace_bytes, void *stream) {
    PrefillVarlenWindowKernelParams wp;
    const PrefillVarlenWindow w{window, sinks};
    bool launch;
    if (const int rc = prefill_varlen_call("sfa_prefill_varlen_window_fwd", a, &w, nullptr, workspace, workspace_bytes, &wp.base,
                                           &launch))
        return rc;
    if (!launch) return SFA_OK;
    if (!sinks && window >= a->total_k) return launch_prefill_varlen(wp.base, a->dtype, a->head_dim, true, (hipStream_t)stream);
    const int cap = a->total_k > 1 ? a->total_k : 1;    // a longer window is the causal mask of every sequence
    wp.window = window < cap ? window : cap;
    wp.sinks = sinks;
    return launch_prefill_varlen_window(wp, a->dtype, a->head_dim, (hipStream_t)stream);
}

// ---- sfa_prefill_varlen_split_fwd: the packed call with a split key range (prefill_varlen_split_kernel.hip) ----
size_t sfa_prefill_varlen_split_workspace_bytes(int batch, int heads_q, int total_q, int max_seqlen_k, int head_dim,
                                                int num_splits) {
    if (batch <= 0 || heads_q <= 0 || total_q <= 0 || max_seqlen_k <= 0 || (head_dim != 64 && head_dim != 128)) return 0;
    const int S = num_splits >= 1 ? split_resolve(varlen_split_key_tiles(max_seqlen_k), num_splits)
                                  : varlen_split_auto(batch, heads_q, total_q, max_seqlen_k);
    return varlen_split_bytes(batch, heads_q, total_q, head_dim, S);
}

int sfa_prefill_varlen_auto_splits(int batch, int heads_q, int total_q, int max_seqlen_k, int head_dim, int causal) {
    (void)head_dim;
    (void)causal;
    return varlen_split_auto(batch, heads_q, total_q, max_seqlen_k);
}

// sfa_prefill_varlen_fwd with each q-tile's key range cut into splits.  A resolved count of 1: the call is
// sfa_prefill_varlen_fwd's, launch and all
int sfa_prefill_varlen_split_fwd(const sfa_prefill_varlen_args *a, int max_seqlen_k, int num_splits, void *workspace,
                                 size_t workspace_bytes, void *stream) {
    PrefillVarlenSplitKernelParams sp;
    PrefillVarlenSplit s{max_seqlen_k, num_splits, 1};
    bool launch;
    if (const int rc = prefill_varlen_call("sfa_prefill_varlen_split_fwd", a, nullptr, &s, workspace, workspace_bytes,
                                           &sp.base, &launch))
        return rc;
    if (!launch) return SFA_OK;
    const int S = s.resolved;
    const bool causal = a->causal != 0;
    g_knobs.last_prefill_splits.store(S, std::memory_order_relaxed);
    if (S == 1) return launch_prefill_varlen(sp.base, a->dtype, a->head_dim, causal, (hipStream_t)stream);
    // the workspace: the plan, the items, the partials (O, then (m, l)), each from a 256-byte boundary
    const size_t bound = (size_t)sp.base.bound;
    char *ws = (char *)workspace + varlen_plan_bytes(a->batch, a->total_q);
    sp.items = (int2 *)ws;
    ws += align_up(bound * S * sizeof(int2), 256);
    const size_t rows = bound * a->heads_q * S * kSplitRows;
    sp.part_o = (float *)ws;
    sp.part_ml = (float2 *)(ws + rows * a->head_dim * sizeof(float));
    sp.num_splits = S;
    sp.tiles_per_split = split_chunk(varlen_split_key_tiles(max_seqlen_k), S);
    if (const int rc = launch_prefill_varlen_plan(sp.base, (hipStream_t)stream)) return rc;
    if (const int rc = launch_prefill_varlen_split_items(sp, causal, (hipStream_t)stream)) return rc;
    if (const int rc = launch_prefill_varlen_split(sp, a->dtype, a->head_dim, causal, (hipStream_t)stream)) return rc;
    return launch_prefill_varlen_split_combine(sp, a->dtype, a->head_dim, causal, (hipStream_t)stream);
}

int sfa_prefill_fwd(const sfa_prefill_args *a, void *stream) {
    PrefillKernelParams p;
    bool launch;
    if (const int rc = prefill_call("sfa_prefill_fwd", a, true, &p, &launch)) return rc;
    if (!launch) return SFA_OK;
    if (a->seqlen_k == 0)       // no keys: every row is empty -> zeros, lse = -inf (the header's promise)
        return launch_prefill_no_keys(p, a->head_dim, (hipStream_t)stream);
    return launch_prefill(p, a->dtype, a->head_dim, a->causal != 0, (hipStream_t)stream);
}

// sfa_prefill_fwd under a sliding window, with an optional attention sink per query head.  No sink and a window that
// covers every key: the call is sfa_prefill_fwd's (causal, exact scale), launch and all
int sfa_prefill_window_fwd(const sfa_prefill_args *a, int window, const float *sinks, void *stream) {
    static const char *const name = "sfa_prefill_window_fwd";
    PrefillWindowKernelParams wp;
    bool launch;
    if (a && ((uintptr_t)sinks & 3)) return fail(SFA_ERR_BAD_SHAPE, "%s: sinks must be 4-byte aligned", name);
    if (a && !a->causal) return fail(SFA_ERR_BAD_SHAPE, "%s: causal must be non-zero (a two-sided window is not served)", name);
    if (a && window < 1) return fail(SFA_ERR_BAD_SHAPE, "%s: window=%d must be >= 1", name, window);
    if (const int rc = prefill_call(name, a, false, &wp.base, &launch)) return rc;
    if (!launch) return SFA_OK;
    wp.base.fast_scale = 0;
    if (a->seqlen_k == 0)       // no keys: zeros and lse = -inf, sink or not
        return launch_prefill_no_keys(wp.base, a->head_dim, (hipStream_t)stream);
    if (!sinks && window >= a->seqlen_k) return launch_prefill(wp.base, a->dtype, a->head_dim, true, (hipStream_t)stream);
    wp.window = window < a->seqlen_k ? window : a->seqlen_k;    // a longer window is the causal mask
    wp.sinks = sinks;
    return launch_prefill_window(wp, a->dtype, a->head_dim, (hipStream_t)stream);
}

int sfa_compute_rotary_table(void *cos_table, void *sin_table, int max_seq_len, int rot_dim, int dtype,
                             void *stream) {
    if (!cos_table || !sin_table) return fail(SFA_ERR_NULL_POINTER, "sfa_compute_rotary_table: NULL table");
    if (max_seq_len < 0 || rot_dim < 0 || (rot_dim & 1))
        return fail(SFA_ERR_BAD_SHAPE, "sfa_compute_rotary_table: max_seq_len=%d rot_dim=%d", max_seq_len, rot_dim);
    return launch_rotary_table(cos_table, sin_table, max_seq_len, rot_dim, dtype, (hipStream_t)stream);
}

int sfa_fill_16bit(void *array, uint16_t bits, size_t n, void *stream) {
    if (!array && n) return fail(SFA_ERR_NULL_POINTER, "sfa_fill_16bit: NULL array");
    return launch_fill16(array, bits, n, (hipStream_t)stream);
}

}  // extern "C"
