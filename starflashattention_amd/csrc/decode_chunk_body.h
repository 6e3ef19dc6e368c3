// The three kernels of the multi-token decode step, shared by sfa_decode_chunk (decode_chunk_kernel.hip: the same n
// for every sequence) and sfa_decode_varlen (decode_varlen_kernel.hip: a ragged, packed batch).  What differs between
// the two -- how many tokens a sequence has, where its packed rows of qkv / o / the rotated Q / the partials are, and
// which (sequence, q-tile) a workgroup serves -- sits behind one policy, GEO:
//
//   using Params                       the kernel argument; chunk(gp) is its ChunkKernelParams
//   prologue(gp, b, t, n) -> bool      the (sequence, token) of this prologue workgroup and the sequence's token count;
//                                      false: the packed row belongs to no sequence, touch nothing
//   qkv_off(gp, b, t)                  element offset of token t of sequence b in qkv
//   attn(gp, b, qt, hs, n, R) -> bool  the (sequence, q-tile) and hs = kv head * S + split of this attention workgroup;
//                                      false: an empty plan slot
//   q_row(gp, b, hk, r)                row of the rotated Q that holds query row r = t*G + g of (b, hk)
//   part_row(gp, b, hk, split, r)      the same for the fp32 partials [.., S, ..]
//   o_tok(gp, b, t)                    row of o ([rows, H, D]) of token t of sequence b
//   combine(gp, row, ...) -> bool      the partial group / row / o token / head a combine thread merges
//
// With the uniform policy every one of these is the expression the chunk kernels used to spell out, and the kernels
// compile to the code they compiled to before the split (DESIGN.md lists the resource usage of both).
//
// A sliding window (sfa_decode_chunk_window / sfa_decode_varlen_window) is a compile-time property of the geometry:
// WindowGeo<BASE, P> below is BASE with `static constexpr bool kWindow = true` and window(gp).  Only chunk_attn_kernel
// looks at it; without the flag none of the window's code is compiled.
//
// An fp8 (e4m3) KV cache (sfa_decode_chunk_kv8 / sfa_decode_varlen_kv8) is the same kind of property: Kv8Geo<BASE, P> is
// BASE with `static constexpr bool kKv8 = true`, k_scale(gp) and v_scale(gp).  The prologue then stores q8(x / scale)
// bytes, the attention kernel stages bytes and converts them on their way into the same 16-bit LDS tiles, and the scales
// go into the score scale and the epilogue; the combine kernel does not look at the flag.  Without it none of the fp8
// code is compiled.
//
// The two properties are independent in the kernels, and Kv8WindowGeo<BASE, P> carries both
// (sfa_decode_chunk_kv8_window / sfa_decode_varlen_kv8_window).
//
// An attention sink (sfa_decode_chunk_window_sinks / sfa_decode_varlen_window_sinks) is a third property of that kind:
// WindowSinkGeo<BASE, P> is WindowGeo with `static constexpr bool kSink = true` and sinks(gp), one fp32 logit per query
// head.  Only chunk_attn_kernel's epilogue looks at it: the workgroups of split 0 fold the sink into their rows' state, so
// a row counts it once; the prologue and combine kernels do not look at the flag.
// Kv8WindowSinkGeo<BASE, P> carries all three (sfa_decode_chunk_kv8_window_sinks / sfa_decode_varlen_kv8_window_sinks,
// DESIGN.md 5.17).
#pragma once
#include "decode_chunk_common.h"
#include "kv8_convert.h"
#include "prefill_core.h"

namespace sfa {
namespace chunk {

using namespace prefill;
using decode::pack8;
using decode::unpack8;
using decode::dq8;
using decode::q8x8;

constexpr uint16_t nan_bits(int dtype_id) { return dtype_id == 0 ? 0x7e00 : 0x7fc0; }

// Does GEO carry a sliding window?
template <class GEO, class = void> struct geo_window : std::false_type {};
template <class GEO> struct geo_window<GEO, std::void_t<decltype(GEO::kWindow)>> : std::bool_constant<GEO::kWindow> {};

// Is GEO's cache e4m3 bytes with a scale per kv head?
template <class GEO, class = void> struct geo_kv8 : std::false_type {};
template <class GEO> struct geo_kv8<GEO, std::void_t<decltype(GEO::kKv8)>> : std::bool_constant<GEO::kKv8> {};

// Does GEO carry an attention sink per query head?
template <class GEO, class = void> struct geo_sink : std::false_type {};
template <class GEO> struct geo_sink<GEO, std::void_t<decltype(GEO::kSink)>> : std::bool_constant<GEO::kSink> {};

// BASE behind a parameter struct P that holds BASE's Params as `base`: what the wrappers below share
template <class BASE, class P>
struct ForwardGeo {
    using Params = P;
    static __device__ __forceinline__ const ChunkKernelParams &chunk(const P &gp) { return BASE::chunk(gp.base); }
    static __device__ __forceinline__ bool prologue(const P &gp, int &b, int &t, int &n) {
        return BASE::prologue(gp.base, b, t, n);
    }
    static __device__ __forceinline__ long long qkv_off(const P &gp, int b, int t) { return BASE::qkv_off(gp.base, b, t); }
    static __device__ __forceinline__ bool attn(const P &gp, int &b, int &qt, int &hs, int &n, int &R) {
        return BASE::attn(gp.base, b, qt, hs, n, R);
    }
    static __device__ __forceinline__ long long q_row(const P &gp, int b, int hk, long long r) {
        return BASE::q_row(gp.base, b, hk, r);
    }
    static __device__ __forceinline__ long long part_row(const P &gp, int b, int hk, int split, long long r) {
        return BASE::part_row(gp.base, b, hk, split, r);
    }
    static __device__ __forceinline__ long long o_tok(const P &gp, int b, int t) { return BASE::o_tok(gp.base, b, t); }
    static __device__ __forceinline__ bool combine(const P &gp, long long row, long long &grp, long long &rows,
                                                   long long &r, long long &tok, int &head) {
        return BASE::combine(gp.base, row, grp, rows, r, tok, head);
    }
};

// BASE with a window: P holds BASE's Params as `base` and the window (>= 1) as `window`
template <class BASE, class P>
struct WindowGeo : ForwardGeo<BASE, P> {
    static constexpr bool kWindow = true;
    static __device__ __forceinline__ int window(const P &gp) { return gp.window; }
};

// BASE over e4m3 caches: P holds BASE's Params as `base` and the per-kv-head scales (nullptr = 1.0) as `k_scale`, `v_scale`
template <class BASE, class P>
struct Kv8Geo : ForwardGeo<BASE, P> {
    static constexpr bool kKv8 = true;
    static __device__ __forceinline__ const float *k_scale(const P &gp) { return gp.k_scale; }
    static __device__ __forceinline__ const float *v_scale(const P &gp) { return gp.v_scale; }
};

// BASE with both: P holds BASE's Params as `base`, `window`, `k_scale` and `v_scale`.  One wrapper rather than one of the
// two above around the other: each of them forwards to ForwardGeo, so the outer one would hide the inner one's flag and
// accessors
template <class BASE, class P>
struct Kv8WindowGeo : ForwardGeo<BASE, P> {
    static constexpr bool kWindow = true;
    static constexpr bool kKv8 = true;
    static __device__ __forceinline__ int window(const P &gp) { return gp.window; }
    static __device__ __forceinline__ const float *k_scale(const P &gp) { return gp.k_scale; }
    static __device__ __forceinline__ const float *v_scale(const P &gp) { return gp.v_scale; }
};

// BASE with a window and an attention sink: P holds BASE's Params as `base`, `window` and `sinks` ([H] fp32, never
// nullptr).  One wrapper, for Kv8WindowGeo's reason: a sink wrapper around WindowGeo would hide its flag and accessor
template <class BASE, class P>
struct WindowSinkGeo : ForwardGeo<BASE, P> {
    static constexpr bool kWindow = true;
    static constexpr bool kSink = true;
    static __device__ __forceinline__ int window(const P &gp) { return gp.window; }
    static __device__ __forceinline__ const float *sinks(const P &gp) { return gp.sinks; }
};

// BASE over e4m3 caches with a window and an attention sink: P holds BASE's Params as `base`, `window`, `k_scale`,
// `v_scale` and `sinks`.  One wrapper again, for the same reason.  The three flags meet in chunk_attn_kernel's epilogue
// only, in an order that needs no fp8 case: the row's maximum carries k_scale already (c2), so the sink joins it
// unscaled, and v_scale multiplies the accumulator after the fold, to which the sink added 0
template <class BASE, class P>
struct Kv8WindowSinkGeo : ForwardGeo<BASE, P> {
    static constexpr bool kWindow = true;
    static constexpr bool kKv8 = true;
    static constexpr bool kSink = true;
    static __device__ __forceinline__ int window(const P &gp) { return gp.window; }
    static __device__ __forceinline__ const float *k_scale(const P &gp) { return gp.k_scale; }
    static __device__ __forceinline__ const float *v_scale(const P &gp) { return gp.v_scale; }
    static __device__ __forceinline__ const float *sinks(const P &gp) { return gp.sinks; }
};

// The window's lower mask of a half-tile of fresh scores (mask_half's register layout): keys below lo get -inf
__device__ __forceinline__ void mask_low(f32x16 &s, int kbase, int h2, int lo) {
#pragma unroll
    for (int r = 0; r < 16; ++r)
        if (kbase + (r & 3) + 8 * (r >> 2) + 4 * h2 < lo) s[r] = ninf();
}

template <class GEO, class Tr, int D, bool PAGED>
__global__ void __launch_bounds__(256)
chunk_prologue_kernel(const typename GEO::Params gp) {
    const ChunkKernelParams &cp = GEO::chunk(gp);
    const DecodeKernelParams &p = cp.d;
    constexpr int LPR = D / 8;                  // lanes (16 B each) per head row
    constexpr bool KV8 = geo_kv8<GEO>::value;   // the caches hold e4m3 bytes: strides and offsets in elements = bytes
    int t, b, n;
    if (!GEO::prologue(gp, b, t, n)) return;
    const int pos = p.seq_len[b];
    const int reject = chunk::reject_code<PAGED>(p, n, b, pos);
    if (reject) {
        if (t == 0 && threadIdx.x == 0) atomicOr(p.status, reject);
        return;
    }
    const int row = pos + t;                    // cache row and RoPE position of token t
    const int Hq = p.H, Hkv = p.Hkv, G = cp.G;
    const long long src = GEO::qkv_off(gp, b, t);
    long long kv_off = chunk::head_base<D, PAGED>(p, b, 0);
    if (PAGED) {
        const int pg = p.block_table[(long long)b * p.table_stride + (row >> p.page_shift)];   // checked above
        kv_off += pg * p.page_stride + (long long)(row & ((1 << p.page_shift) - 1)) * p.kv_row_stride;
    } else {
        kv_off += (long long)row * p.kv_row_stride;
    }
    // cos / sin of this token's pairs, once per workgroup (not once per head: the trig dominated the prologue)
    __shared__ float cs[D / 2], sn[D / 2];
    for (int j = threadIdx.x; j < (p.rot_dim >> 1); j += blockDim.x) chunk::rope_cs<Tr>(j, row, p, cs[j], sn[j]);
    __syncthreads();
    // KV8: 8 values -> q8(x / scale[h]), the 8 bytes at element offset `off` of an e4m3 cache
    auto store8 = [&](uint16_t *cache, long long off, const uint4 &pk, const float *scales, int h) {
        float x[8];
        unpack8<Tr>(pk, x);
        *reinterpret_cast<uint2 *>(reinterpret_cast<char *>(cache) + off) = q8x8(x, scales ? scales[h] : 1.0f);
    };
    const int items = (Hq + 2 * Hkv) * LPR;
    for (int i = threadIdx.x; i < items; i += blockDim.x) {
        const int hd = i / LPR, sub = i % LPR;
        const uint4 raw = *reinterpret_cast<const uint4 *>(p.qkv + src + (long long)hd * D + sub * 8);
        if (hd < Hq + Hkv) {                    // q head or k head: bias, RoPE, round
            const bool isq = hd < Hq;
            const int h = isq ? hd : hd - Hq;
            float x[8];
            unpack8<Tr>(raw, x);
            const uint16_t *bias = isq ? p.q_bias : p.k_bias;
            if (bias) chunk::add_bias8<Tr>(x, bias + (long long)h * D + sub * 8);
            chunk::rope8(x, sub, p.rot_dim, cs, sn);
            const uint4 pk = pack8<Tr>(x);
            if (isq) {
                const long long r = (long long)t * G + h % G;
                *reinterpret_cast<uint4 *>(cp.q_rot + GEO::q_row(gp, b, h / G, r) * D + sub * 8) = pk;
            } else if constexpr (KV8) {           // the rounded 16-bit k the 16-bit call stores, quantised
                store8(p.k_cache, kv_off + (long long)h * p.kv_head_stride + sub * 8, pk, GEO::k_scale(gp), h);
            } else {
                *reinterpret_cast<uint4 *>(p.k_cache + kv_off + (long long)h * p.kv_head_stride + sub * 8) = pk;
            }
        } else {                                // v head: bias only
            const int h = hd - Hq - Hkv;
            uint4 pk = raw;
            if (p.v_bias) {
                float x[8];
                unpack8<Tr>(raw, x);
                chunk::add_bias8<Tr>(x, p.v_bias + (long long)h * D + sub * 8);
                pk = pack8<Tr>(x);
            }
            if constexpr (KV8)
                store8(p.v_cache, kv_off + (long long)h * p.kv_head_stride + sub * 8, pk, GEO::v_scale(gp), h);
            else
                *reinterpret_cast<uint4 *>(p.v_cache + kv_off + (long long)h * p.kv_head_stride + sub * 8) = pk;
        }
    }
}

// Which (sequence, q-tile, kv head * S + split) a workgroup serves is GEO::attn's business (uniform: blockIdx x = q-tile,
// heaviest first, y = kv head * S + split, z = batch).
template <class GEO, class Tr, int D, bool PAGED>
__global__ void __launch_bounds__(kThreads, 2)
chunk_attn_kernel(const typename GEO::Params gp) {
    using Vec = typename Tr::mfma_vec;
    constexpr int NQB = 1, PF = 2, ORD = 2;     // one 32-row query block per wave, exact scale, staged softmax
    constexpr int NKS = D / 16;                 // k-steps of Q.K^T
    constexpr int NDB = D / 32;                 // 32-wide d blocks of O^T
    constexpr int NPV_ = 2 * NDB;
    // A staged chunk is CE elements of a cache row: 16 B of a 16-bit cache.  KV8 (EB = 1 byte per element): 16 B at
    // head_dim 128 and 8 B at head_dim 64, so that the 64 rows of a tile are one load per thread either way; the chunk
    // becomes 2 * CE bytes of the 16-bit LDS image at store_op.
    constexpr bool KV8 = geo_kv8<GEO>::value;
    constexpr int EB = KV8 ? 1 : 2;             // bytes per cache element
    constexpr int CE = KV8 && D == 128 ? 16 : 8;
    constexpr int CBG = CE * EB, CBL = CE * 2;  // bytes of a chunk in the cache / in LDS
    constexpr int CPR = D / CE;                 // chunks per row
    constexpr int NLD = kBN * CPR / kThreads;   // chunks staged per thread per tile (2 or 1)
    constexpr int ROWSTEP = kThreads / CPR;     // row distance between a thread's chunks
    constexpr int NPS = PAGED ? 4 : 1;          // page slots of a 64-row tile (page_size >= 16)
    using L = Lds<D>;
    static_assert(NLD >= 1 && NLD <= 2, "staging registers are named kr0, kr1");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const ChunkKernelParams &cp = GEO::chunk(gp);
    const DecodeKernelParams &p = cp.d;

    const int S = p.num_splits;
    int b, qt, hs, ntok, R;                     // ntok new tokens, R = ntok * G query rows per kv head
    if (!GEO::attn(gp, b, qt, hs, ntok, R)) return;
    const int hk = hs / S, split = hs % S;
    const int G = cp.G;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, h2 = lane >> 5;
    const int q0 = qt * kBM, wq0 = q0 + 32 * wave, qrow = wq0 + l31;
    const long long prow = GEO::part_row(gp, b, hk, split, 0);     // partial row 0 of (b, hk, split)
    auto out_row = [&](int r) -> uint16_t * {  // o[b, t, h, :] of query row r = t*G + g
        return p.o + (GEO::o_tok(gp, b, r / G) * p.H + (long long)hk * G + r % G) * D;
    };

    const int pos = p.seq_len[b];
    if (const int reject = chunk::reject_code<PAGED>(p, ntok, b, pos)) {
        (void)reject;                           // the prologue raised the flag
        if (qrow < R && h2 == 0) {
            if (S == 1) {
                const uint32_t w = nan_bits(Tr::id) * 0x10001u;
                uint16_t *orow = out_row(qrow);
#pragma unroll
                for (int c = 0; c < D / 8; ++c) *reinterpret_cast<uint4 *>(orow + 8 * c) = make_uint4(w, w, w, w);
            } else {
                p.part_ml[prow + qrow] = make_float2(0.f, __builtin_nanf(""));
            }
        }
        return;
    }

    // ---- the key range of this workgroup: tiles [ts0, wg_end) of the Kb = pos + n keys ----
    // WIN: the row with causal limit `lim` sees the keys [max(0, lim + 1 - window), lim].  No key below lo0, the lower
    // bound of the sequence's first token, is visible to any row, so the splits share the tiles [tlo, ntot) and a
    // workgroup starts at the tile of its q-tile's first row's lower bound, if that is later than its split's.
    constexpr bool WIN = geo_window<GEO>::value;
    int win = 0;
    if constexpr (WIN) win = GEO::window(gp);
    auto low_of = [&](int limit) -> int { return max(0, limit + 1 - win); };    // (WIN only)
    const int Kb = pos + ntok;
    const int ntot = (Kb + kBN - 1) / kBN;
    const int lo0 = WIN ? low_of(pos) : 0;
    const int tlo = lo0 / kBN;
    const int per = (ntot - tlo + S - 1) / S;   // tiles per split
    const int ts0s = tlo + split * per;         // the split's first tile
    const int ts0 = WIN ? max(ts0s, low_of(pos + q0 / G) / kBN) : ts0s;
    const int rlast = min(q0 + kBM, R) - 1;     // last query row of the q-tile
    const int wg_end = min(min(ntot, ts0s + per), (pos + rlast / G) / kBN + 1);
    const int nt = max(0, wg_end - ts0);        // tiles the workgroup stages (workgroup-uniform)
    int ntw = 0;                                // tiles this wave computes on (wave-uniform)
    if (wq0 < R) ntw = max(0, min(wg_end, (pos + min(wq0 + 31, R - 1) / G) / kBN + 1) - ts0);
    int lim[NQB];                               // last visible key of this lane's row
    lim[0] = pos + min(qrow, R - 1) / G;
    const int wlim = pos + min(wq0, R - 1) / G; // the smallest limit of the wave's rows
    // WIN: this lane's lower bound, the largest one of the wave's rows, and the leading tiles of the workgroup that lie
    // wholly below the smallest one: the wave only stages during those (the mirror of the idle steps at the end)
    const int lo_r = WIN ? low_of(lim[0]) : 0;
    const int wlo = WIN ? low_of(pos + min(wq0 + 31, R - 1) / G) : 0;
    const int tw0 = WIN ? min(max(0, low_of(wlim) / kBN - ts0), ntw) : 0;
    // bit 0 set: the 32 keys starting at KBASE need masking for this wave's rows (lim <= Kb - 1 always)
    auto mask_bits = [&](int kbase) -> int { return (kbase + 31 > wlim || (WIN && kbase < wlo)) ? 1 : 0; };
    // WIN: the lower mask, applied by h_block next to the causal one on the halves mask_bits flags
    auto low_mask = [&] {
        if constexpr (WIN) {
            return [&](f32x16 &s, int kbase, int) {
                if (kbase < wlo) mask_low(s, kbase, h2, lo_r);
            };
        } else {
            return NoLowMask();
        }
    }();

    // ---- staging: thread owns chunks (row st_row + i*ROWSTEP, chunk st_ch), i < NLD, of every tile ----
    const int st_row = tid / CPR, st_ch = tid % CPR;
    const long long rsb = EB * p.kv_row_stride; // bytes between cache rows (of one page)
    const long long hb = chunk::head_base<D, PAGED>(p, b, hk);
    const char *const kg = reinterpret_cast<const char *>(p.k_cache) + EB * hb;
    const char *const vg = reinterpret_cast<const char *>(p.v_cache) + EB * hb;
    char *const k_w = smem + L::KS * st_row + CBL * st_ch;
    char *const v_w = smem + L::V_BASE + L::VS * st_row + CBL * st_ch;
    uint4 kr0, kr1, vr0, vr1;       // plain scalars: arrays of these ended up in scratch (prefill_kernel.hip)
    kr0 = kr1 = vr0 = vr1 = make_uint4(0, 0, 0, 0);
    // a chunk from the cache (KV8: raw bytes, CBG of them) and into an LDS tile (KV8: converted, exact in both types)
    auto ld_chunk = [](const char *src) -> uint4 {
        if constexpr (CBG == 8) {
            const uint2 v = *reinterpret_cast<const uint2 *>(src);
            return make_uint4(v.x, v.y, 0, 0);
        } else {
            return *reinterpret_cast<const uint4 *>(src);
        }
    };
    auto st_chunk = [](char *dst, const uint4 &r) {
        if constexpr (KV8) {
            *reinterpret_cast<uint4 *>(dst) = dq8<Tr>(r.x, r.y);
            if constexpr (CE == 16) *reinterpret_cast<uint4 *>(dst + 16) = dq8<Tr>(r.z, r.w);
        } else {
            *reinterpret_cast<uint4 *>(dst) = r;
        }
    };
    // Rows of a tile: contiguous layouts and pages >= 64 rows hold the whole tile at one base; pages of 16 / 32 rows
    // split it into 4 / 2 page slots of 1 << psh rows.  Row r of the tile is at slot base (r >> psh) plus the
    // lane offset (r & (2^psh - 1)) * rsb.  The ragged last tile (Kb % 64 != 0) swaps in row-clamped offsets.
    const int psh = PAGED ? min(p.page_shift, 6) : 6;
    const int rmask = (1 << psh) - 1;
    const int ragged_tile = (Kb % kBN) ? ntot - 1 : -1;
    const int last0 = Kb - 1 - (ntot - 1) * kBN;            // last valid row of the last tile
    // WIN: the first tile (tlo) is clamped from below as well, to max(row, lo0): nothing below lo0 is read, in the
    // cache or in the table -- a masked key has weight 0, but 0 * NaN is NaN in P.V.  Its offsets are worked out per
    // tile from the clamped row rather than kept in a third and fourth set of registers.
    const int first0 = lo0 - tlo * kBN;                     // first valid row of the first tile
    const int row0_ = st_row, row1_ = st_row + ROWSTEP;
    const int rr0_ = min(row0_, last0), rr1_ = min(row1_, last0);
    // (32 bit: 64 rows * rsb < 2^31, checked by sfa_decode_chunk)
    auto lane_off = [&](int r) -> unsigned { return (unsigned)(r & rmask) * (unsigned)rsb + (unsigned)CBG * st_ch; };
    const unsigned ow0 = lane_off(row0_), ow1 = lane_off(row1_), or0 = lane_off(rr0_), or1 = lane_off(rr1_);
    const int sw0 = row0_ >> psh, sw1 = row1_ >> psh, sr0 = rr0_ >> psh, sr1 = rr1_ >> psh;
    const int32_t *tbl = PAGED ? p.block_table + (long long)b * p.table_stride : nullptr;
    const int pmask = PAGED ? (1 << p.page_shift) - 1 : 0;
    int bad_page = 0;
    // byte offsets (from kg / vg) of the page slots of tile `tile` -- scalar: table entries by s_load
    auto tile_base = [&](int tile, long long (&o)[NPS]) {
        const int r0 = tile * kBN;
        if (!PAGED) {
            o[0] = (long long)r0 * rsb;
            return;
        }
#pragma unroll
        for (int j = 0; j < NPS; ++j) {
            o[j] = 0;
            if ((j << psh) < kBN) {
                const int r = min(WIN ? max(r0 + (j << psh), lo0) : r0 + (j << psh), Kb - 1);
                int pg = tbl[r >> p.page_shift];
                if ((unsigned)pg >= (unsigned)p.num_pages) {    // a READ page outside the pool: not dereferenced
                    bad_page = 1;
                    pg = 0;
                }
                o[j] = pg * p.page_stride * EB + (long long)(r0 & pmask) * rsb;
            }
        }
    };
    auto sel = [&](const long long (&o)[NPS], int s) -> long long {
        if (NPS == 1) return o[0];
        return s == 0 ? o[0] : s == 1 ? o[1] : s == 2 ? o[2] : o[3];
    };
    constexpr int NOPS = 2 * NLD;   // op n: even = K chunk n/2, odd = V chunk n/2
    struct TileSrc { long long k[NPS], v[NPS]; bool rk, rv; int fk, fv; };      // fk / fv: WIN, first valid row
    auto tile_of = [&](int t) -> int { return min(ts0 + t, wg_end - 1); };  // past the end: re-read the last tile
    auto tile_src = [&](int pos_k, int pos_v) -> TileSrc {
        const int tk = tile_of(pos_k), tv = tile_of(pos_v);
        TileSrc ts;
        tile_base(tk, ts.k);
        tile_base(tv, ts.v);
        ts.rk = tk == ragged_tile;
        ts.rv = tv == ragged_tile;
        if constexpr (WIN) {
            ts.fk = tk == tlo ? first0 : 0;
            ts.fv = tv == tlo ? first0 : 0;
        }
        return ts;
    };
    auto win_off = [&](const long long (&o)[NPS], int i, int first, bool ragged) -> long long {
        const int r = min(max(i == 0 ? row0_ : row1_, first), ragged ? last0 : kBN - 1);
        return sel(o, r >> psh) + lane_off(r);
    };
    auto ld_k = [&](const TileSrc &ts, int i) -> uint4 {
        if constexpr (WIN) return ld_chunk(kg + win_off(ts.k, i, ts.fk, ts.rk));
        const long long off = i == 0 ? (ts.rk ? sel(ts.k, sr0) + or0 : sel(ts.k, sw0) + ow0)
                                     : (ts.rk ? sel(ts.k, sr1) + or1 : sel(ts.k, sw1) + ow1);
        return ld_chunk(kg + off);
    };
    auto ld_v = [&](const TileSrc &ts, int i) -> uint4 {
        if constexpr (WIN) return ld_chunk(vg + win_off(ts.v, i, ts.fv, ts.rv));
        const long long off = i == 0 ? (ts.rv ? sel(ts.v, sr0) + or0 : sel(ts.v, sw0) + ow0)
                                     : (ts.rv ? sel(ts.v, sr1) + or1 : sel(ts.v, sw1) + ow1);
        return ld_chunk(vg + off);
    };
    auto load_op = [&](int n, const TileSrc &ts) {
        if (n == 0) kr0 = ld_k(ts, 0);
        if (n == 1) vr0 = ld_v(ts, 0);
        if (NLD > 1 && n == 2) kr1 = ld_k(ts, 1);
        if (NLD > 1 && n == 3) vr1 = ld_v(ts, 1);
    };
    auto store_op = [&](int n, int kbuf, int vbuf) {
        if (n == 0) st_chunk(k_w + kbuf, kr0);
        if (n == 1) st_chunk(v_w + vbuf, vr0);
        if (NLD > 1 && n == 2) st_chunk(k_w + kbuf + ROWSTEP * L::KS, kr1);
        if (NLD > 1 && n == 3) st_chunk(v_w + vbuf + ROWSTEP * L::VS, vr1);
    };

    // KV8: the scales never touch a tile -- k_scale[hk] goes into the score scale, v_scale[hk] into the epilogue
    float ksc = 1.0f, vsc = 1.0f;
    if constexpr (KV8) {
        if (GEO::k_scale(gp)) ksc = GEO::k_scale(gp)[hk];
        if (GEO::v_scale(gp)) vsc = GEO::v_scale(gp)[hk];
    }
    const float c2 = KV8 ? p.scale_log2 * ksc : p.scale_log2;
    const char *const k_rd = smem + L::KS * l31 + 16 * h2;                 // K row l31, chunk h2
    const char *const v_rd = smem + L::V_BASE + L::VS * (4 * h2 + ((lane & 15) >> 2)) +
                             32 * ((lane >> 4) & 1) + 16 * ((lane & 3) >> 1) + 8 * (lane & 1);

    // ---- Q^T fragments (B operand) from the workspace: lane holds Q[row][16ks + 8*h2 .. +8] ----
    Vec qf[NQB][NKS];
    {
        const uint16_t *qp = cp.q_rot + GEO::q_row(gp, b, hk, min(qrow, R - 1)) * D + 8 * h2;
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) qf[0][ks] = bitcast<Vec>(*reinterpret_cast<const uint4 *>(qp + 16 * ks));
    }

    Acc<D, NQB> acc;
#pragma unroll
    for (int d = 0; d < NDB; ++d)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc.o[0][d][r] = 0.f;
    acc.msc[0] = ninf();
    acc.lsum[0] = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc.cinit[0][r] = 0.f;

    if (nt > 0) {
        // ---- staging prologue (prefill_kernel.hip): stream positions 0 and 1 into LDS, 2 (K) and 1 (V) in flight ----
        uint4 kx0, kx1;                         // K(1), prologue only
        {
            const TileSrc ts0_ = tile_src(0, 0);
#pragma unroll
            for (int n = 0; n < NOPS; ++n) load_op(n, ts0_);
            const TileSrc ts1_ = tile_src(1, 1);
            kx0 = ld_k(ts1_, 0);
            kx1 = NLD > 1 ? ld_k(ts1_, 1) : make_uint4(0, 0, 0, 0);
        }
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) asm volatile("" : "+v"(qf[0][ks]));   // launder: prefill_kernel.hip
#pragma unroll
        for (int n = 0; n < NOPS; ++n) store_op(n, 0, 0);
        st_chunk(k_w + L::KTILE, kx0);
        if (NLD > 1) st_chunk(k_w + L::KTILE + ROWSTEP * L::KS, kx1);
        __syncthreads();
        {
            const TileSrc ts1 = tile_src(2, 1);
#pragma unroll
            for (int n = 0; n < NOPS; ++n) load_op(n, ts1);
        }

        int kcur = 0, vcur = 0;     // byte offsets of the K and V buffers of stream position t
        int t = 0;                  // stream position (tile ts0 + t)
#define SFA_NEXT3(X, TILE) (((X) == 2 * (TILE)) ? 0 : (X) + (TILE))
#define SFA_ADVANCE()                                                                               \
    do {                                                                                            \
        kcur = SFA_NEXT3(kcur, L::KTILE);                                                           \
        vcur = SFA_NEXT3(vcur, L::VTILE);                                                           \
    } while (0)
#define SFA_STAGE_AND_SYNC(T)                                                                       \
    do {                                                                                            \
        const int k1_ = SFA_NEXT3(kcur, L::KTILE);                                                  \
        _Pragma("unroll") for (int n_ = 0; n_ < NOPS; ++n_)                                         \
            store_op(n_, SFA_NEXT3(k1_, L::KTILE), SFA_NEXT3(vcur, L::VTILE));                      \
        __syncthreads();                                                                            \
        const TileSrc ts_ = tile_src((T) + 3, (T) + 2);                                             \
        _Pragma("unroll") for (int n_ = 0; n_ < NOPS; ++n_) load_op(n_, ts_);                       \
        SFA_FENCE();                                                                                \
    } while (0)

        // ---- scores of the first half-tile, first fragments of the second ----
        f32x16 sA[NQB], sB[NQB];
        float mxA[NQB] = {ninf()}, mxB[NQB] = {ninf()};
#pragma unroll
        for (int r = 0; r < 16; ++r) { sA[0][r] = 0.f; sB[0][r] = 0.f; }
        Vec kpre[PF];
#pragma unroll
        for (int i = 0; i < PF; ++i) kpre[i] = bitcast<Vec>(make_uint4(0, 0, 0, 0));
        if constexpr (WIN) {                    // leading idle steps: tiles below every row of this wave
            for (; t < tw0; ++t) {
                SFA_STAGE_AND_SYNC(t);
                SFA_ADVANCE();
            }
        }
        if (WIN ? t < ntw : ntw > 0) {
#pragma unroll
            for (int ks = 0; ks < NKS; ++ks) {
                const Vec a = bitcast<Vec>(*reinterpret_cast<const uint4 *>(k_rd + kcur + 32 * ks));
                sA[0] = Tr::mfma32(a, qf[0][ks], sA[0]);
            }
#pragma unroll
            for (int i = 0; i < PF; ++i)
                kpre[i] = bitcast<Vec>(*reinterpret_cast<const uint4 *>(k_rd + kcur + L::KS * 32 + 32 * i));
            mxA[0] = lane_rowmax(sA[0]);
        }

        // ---- FULL steps: this wave needs the next tile as well (prefill_kernel.hip) ----
        for (; t + 1 < ntw; ++t) {
            const int k1 = SFA_NEXT3(kcur, L::KTILE), k2 = SFA_NEXT3(k1, L::KTILE);
            const int v1 = SFA_NEXT3(vcur, L::VTILE);
            const char *kb = k_rd + kcur, *vb = v_rd + vcur, *kb1 = k_rd + k1;
            const int kbase = (ts0 + t) * kBN;
            auto st_hook = [&](int j) {
#pragma unroll
                for (int n = j * NOPS / NPV_; n < (j + 1) * NOPS / NPV_; ++n) store_op(n, k2, v1);
            };
            h_block<Tr, D, NQB, PF, ORD, 1, 0, true, true>(kb, vb, kb1, qf, sB, sA, acc, c2, mxA, mxB,
                                                           mask_bits(kbase), kbase, h2, lim, kpre, NoHook(), st_hook, low_mask);
            __syncthreads();
            const TileSrc ts = tile_src(t + 3, t + 2);
            auto ld_hook = [&](int i) {
#pragma unroll
                for (int n = (i - 1) * NOPS / (NKS - 1); n < i * NOPS / (NKS - 1); ++n) load_op(n, ts);
            };
            h_block<Tr, D, NQB, PF, ORD, 0, 1, true, true>(kb1, vb, kb1, qf, sA, sB, acc, c2, mxB, mxA,
                                                           mask_bits(kbase + 32), kbase + 32, h2, lim, kpre, ld_hook, NoHook(), low_mask);
            SFA_ADVANCE();
        }
        // ---- TAIL step: this wave's last tile ----
        if (t < ntw) {
            const char *kb = k_rd + kcur, *vb = v_rd + vcur;
            const int kbase = (ts0 + t) * kBN;
            h_block<Tr, D, NQB, PF, ORD, 1, 0, true, false>(kb, vb, kb, qf, sB, sA, acc, c2, mxA, mxB,
                                                            mask_bits(kbase), kbase, h2, lim, kpre, NoHook(), NoHook(), low_mask);
            SFA_STAGE_AND_SYNC(t);
            h_block<Tr, D, NQB, PF, ORD, 0, 1, false, false>(kb, vb, kb, qf, sA, sB, acc, c2, mxB, mxA,
                                                             mask_bits(kbase + 32), kbase + 32, h2, lim, kpre, NoHook(), NoHook(),
                                                             low_mask);
            SFA_ADVANCE();
            ++t;
        }
        // ---- idle steps (tiles beyond this wave's causal limit): keep staging for the others ----
        for (; t < nt; ++t) {
            SFA_STAGE_AND_SYNC(t);
            SFA_ADVANCE();
        }
#undef SFA_NEXT3
#undef SFA_ADVANCE
#undef SFA_STAGE_AND_SYNC
    }

    // ---- epilogue ----
    float ltot = half_sum(acc.lsum[0]);
    // SINK: one more stream element of the row's query head -- max sinks[h] log2(e), sum 1, accumulator 0 -- folded in by
    // the workgroups of split 0 alone, tiles or none (msc = -inf, ltot = 0 then), so that a row counts it once
    if constexpr (geo_sink<GEO>::value) {
        if (split == 0) {
            // (laundered: contracted into `sk - ms` below as one fma, the product's rounding error would stand where 0
            // belongs when the sink is the max)
            float sk = GEO::sinks(gp)[hk * G + min(qrow, R - 1) % G] * 1.4426950408889634f;
            asm volatile("" : "+v"(sk));
            const float mn = fmaxf(acc.msc[0], sk);
            const float ms = (mn == ninf()) ? 0.f : mn;
            const float a1 = fast_exp2(acc.msc[0] - ms);
#pragma unroll
            for (int d = 0; d < NDB; ++d)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc.o[0][d][r] *= a1;
            ltot = __builtin_fmaf(ltot, a1, fast_exp2(sk - ms));
            acc.msc[0] = mn;
        }
    }
    if (PAGED && bad_page) {
        ltot = __builtin_nanf("");
        if (tid == 0) atomicOr(p.status, 2);
    }
    if (qrow < R) {
        if (S == 1) {
            // every row sees key 0 (pos >= 0; WIN: its own key), so ltot > 0 -- or NaN after a bad page
            store_o_row<Tr, D>(out_row(qrow), acc.o[0], (KV8 ? vsc : 1.0f) / ltot, h2);
        } else {
            // un-normalised O^T: lane (l31, h2) holds columns 32d + 8g + 4*h2 + {0..3} in registers 4g..4g+3
            float *po = p.part_o + (prow + qrow) * D;
            if constexpr (KV8) {                // v_scale once, on the fp32 accumulator: the combine is the 16-bit call's
#pragma unroll
                for (int d = 0; d < NDB; ++d)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc.o[0][d][r] *= vsc;
            }
#pragma unroll
            for (int d = 0; d < NDB; ++d)
#pragma unroll
                for (int g = 0; g < 4; ++g)
                    *reinterpret_cast<float4 *>(po + 32 * d + 8 * g + 4 * h2) =
                        make_float4(acc.o[0][d][4 * g], acc.o[0][d][4 * g + 1], acc.o[0][d][4 * g + 2],
                                    acc.o[0][d][4 * g + 3]);
            if (h2 == 0) p.part_ml[prow + qrow] = make_float2(acc.msc[0], ltot);
        }
    }
}

// o[b, t, h, :] = sum_s 2^(m_s - M) o_s / sum_s 2^(m_s - M) l_s    (fp32; an empty split has m = -inf, l = 0)
template <class GEO, class Tr, int D>
__global__ void __launch_bounds__(256)
chunk_combine_kernel(const typename GEO::Params gp) {
    const ChunkKernelParams &cp = GEO::chunk(gp);
    const DecodeKernelParams &p = cp.d;
    constexpr int LPR = D / 8;
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long row = gid / LPR;            // over the rows of the rotated Q
    const int sub = (int)(gid % LPR);
    // partials of the row: [grp, S, rows, D] at (grp, s, r); its output: o[tok, head, :]
    long long grp, rows, r, tok;
    int head;
    if (!GEO::combine(gp, row, grp, rows, r, tok, head)) return;
    const int S = p.num_splits;
    decode::Stream tot;
    tot.init();
    for (int s = 0; s < S; ++s) {
        const long long idx = (grp * S + s) * rows + r;
        const float2 ml = p.part_ml[idx];
        const float *po = p.part_o + idx * D + sub * 8;
        const float4 a = *reinterpret_cast<const float4 *>(po);
        const float4 c = *reinterpret_cast<const float4 *>(po + 4);
        const float a2[8] = {a.x, a.y, a.z, a.w, c.x, c.y, c.z, c.w};
        tot.merge(ml.x, ml.y, a2);
    }
    const float inv = 1.0f / tot.l;
    float y[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) y[j] = tot.acc[j] * inv;
    uint16_t *orow = p.o + (tok * p.H + head) * D;
    *reinterpret_cast<uint4 *>(orow + sub * 8) = pack8<Tr>(y);
}

// Host side.  The launches of one call, ordered by the stream alone: prologue, attention, and (num_splits > 1) the
// combine over combine_rows rows of the rotated Q.  The caller has the grids of its geometry.
template <class GEO, class Tr, int D, bool PAGED>
int launch_chunk_t(const typename GEO::Params &gp, int num_splits, dim3 prologue_grid, dim3 attn_grid, long long combine_rows,
                   hipStream_t stream) {
    hipLaunchKernelGGL((chunk_prologue_kernel<GEO, Tr, D, PAGED>), prologue_grid, dim3(256), 0, stream, gp);
    if (const int rc = check_launch("chunk_prologue_kernel")) return rc;

    const size_t lds = Lds<D>::TOTAL;          // K[3] + V[3], padded rows
    static DynLdsAttr attr;
    if (const int rc = attr.ensure(reinterpret_cast<const void *>(&chunk_attn_kernel<GEO, Tr, D, PAGED>), (int)lds,
                                   "chunk_attn_kernel"))
        return rc;
    hipLaunchKernelGGL((chunk_attn_kernel<GEO, Tr, D, PAGED>), attn_grid, dim3(kThreads), lds, stream, gp);
    if (const int rc = check_launch("chunk_attn_kernel")) return rc;

    if (num_splits > 1) {
        const long long threads = combine_rows * (D / 8);
        hipLaunchKernelGGL((chunk_combine_kernel<GEO, Tr, D>), dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, stream, gp);
        return check_launch("chunk_combine_kernel");
    }
    return SFA_OK;
}

// The instantiation for a validated call: fp16 / bf16, head_dim 64 / 128; p is the call's DecodeKernelParams
template <class GEO, class... Grids>
int launch_chunk(const typename GEO::Params &gp, const DecodeKernelParams &p, int dtype, int head_dim, Grids... grids) {
    const bool h = dtype == SFA_DTYPE_FP16, paged = p.block_table != nullptr;
    if (head_dim == 64) {
        if (paged) return h ? launch_chunk_t<GEO, Fp16, 64, true>(gp, p.num_splits, grids...) : launch_chunk_t<GEO, Bf16, 64, true>(gp, p.num_splits, grids...);
        return h ? launch_chunk_t<GEO, Fp16, 64, false>(gp, p.num_splits, grids...) : launch_chunk_t<GEO, Bf16, 64, false>(gp, p.num_splits, grids...);
    }
    if (paged) return h ? launch_chunk_t<GEO, Fp16, 128, true>(gp, p.num_splits, grids...) : launch_chunk_t<GEO, Bf16, 128, true>(gp, p.num_splits, grids...);
    return h ? launch_chunk_t<GEO, Fp16, 128, false>(gp, p.num_splits, grids...) : launch_chunk_t<GEO, Bf16, 128, false>(gp, p.num_splits, grids...);
}

}  // namespace chunk
}  // namespace sfa
