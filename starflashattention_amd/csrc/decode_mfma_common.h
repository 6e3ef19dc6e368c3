// What the matrix-core decode kernels share whatever the cache's element type (decode_mfma16.h: the 16-bit caches of
// decode_gqa_mfma_kernel.hip and, with a sliding window, decode_window_kernel.hip; decode_kv8_kernel.hip: e4m3 caches): one
// workgroup per (batch, kv head, split), four waves, 32-key tiles on v_mfma_f32_16x16x32, 16 query
// columns of which G are real, one online-softmax state per lane.  Lane coordinates: MFMA (c = lane & 15, g = lane >> 4);
// prologue / row-major (sub = lane % (D/8): which 8 dims, grp = lane / (D/8): which head or row of a pass).
// decode_mfma16.h and decode_kv8_kernel.hip keep what differs: how a tile of the caches reaches the K fragments and the
// wave's LDS V tile, the software pipeline, and the append store.  The design is described in decode_gqa_mfma_kernel.hip.
#pragma once
#include "decode_common.h"

namespace sfa {
namespace decode {

typedef __attribute__((address_space(3))) i16x4 lds_i16x4;

template <class Tr> struct Mfma16;
template <> struct Mfma16<Bf16> {
    static __device__ __forceinline__ f32x4 run(bf16x8 a, bf16x8 b, f32x4 c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
    }
};
template <> struct Mfma16<Fp16> {
    static __device__ __forceinline__ f32x4 run(f16x8 a, f16x8 b, f32x4 c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
    }
};

// max / sum over the four lanes {c, c+16, c+32, c+48} that share a query
__device__ __forceinline__ float quad_max(float x) { return row_pair_max(half_max(x)); }
__device__ __forceinline__ float quad_sum(float x) { return row_pair_sum(half_sum(x)); }

constexpr int kTile = 32;                       // keys per tile

// Dynamic LDS at head_dim D: per wave a V tile (also the Q / k_new re-layout area) and a K tile, both of 16-bit
// elements; the merge of the waves reuses the whole area.
template <int D> struct MfmaLds {
    static constexpr int VS = 2 * D + 32;       // row stride of the V tile (conflict-free transposed reads)
    static constexpr int VTILE = kTile * VS;
    static constexpr int KS = 2 * D + 16;       // row stride of the K tile
    static constexpr int KTILE = kTile * KS;
    static constexpr int WAVE_LDS = VTILE + KTILE;      // one tile of each: the next tiles wait in registers
    static constexpr int BYTES = kDecodeWaves * WAVE_LDS;               // 71,680 B at head_dim 128
    static_assert(BYTES >= kDecodeWaves * 16 * (D + 2) * 4, "merge area fits");
    static_assert(VTILE >= 17 * D * 2, "the query rows and the new key fit the V tile they are re-laid out in");
};

// sfa_decode's rejection contract (reject_code): poison the G output rows of this kv head, raise the status bit, touch
// nothing else.  True = the workgroup returns.
template <class Tr, int D, bool PAGED>
__device__ __forceinline__ bool rejected(const DecodeKernelParams &p, int b, int hk, int split, int G, int pos) {
    const int reject = reject_code<PAGED>(p, b, pos);
    if (!reject) return false;
    const int tid = threadIdx.x;
    if (split == 0) {
        for (int i = tid; i < G * D; i += kDecodeWaves * 64)
            p.o[((long long)b * p.H + (long long)hk * G) * D + i] = Tr::id == 0 ? 0x7e00 : 0x7fc0;
        if (tid == 0 && hk == 0) atomicOr(p.status, reject);
    }
    return true;
}

// Prologue, first half (every wave; lane `sub` owns dims 8 sub .. +8, lane group `grp` handles query heads grp,
// grp + 64 / (D/8), ...): bias, RoPE (fp32), round to storage.  The G query rows are parked in LDS at qs in [16][D] order
// (rows >= G zero); kpk / vpk = this lane's 8 dims of the new token's K and V as sfa_decode stores them.
// Pairs at or beyond rot_dim are rotated by (cos, sin) = (1, 0), not skipped.
template <class Tr, int D>
__device__ __forceinline__ void rotate_new_token(const DecodeKernelParams &p, int b, int hk, int G, int pos, uint16_t *qs,
                                                 uint4 &kpk, uint4 &vpk) {
    constexpr int LPR = D / 8, RPL = 64 / LPR;
    const int lane = threadIdx.x & 63, sub = lane % LPR, grp = lane / LPR;
    const int Hq = p.H, Hkv = p.Hkv;
    const long long row0 = (long long)b * p.qkv_stride + sub * 8;
    float cs[4], sn[4];
    const int rot = p.rot_dim;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int pj = sub * 4 + i;
        cs[i] = 1.f; sn[i] = 0.f;
        if (2 * pj < rot) rope_cs<Tr>(pj, pos, p, cs[i], sn[i]);
    }
    auto rope = [&](float (&x)[8]) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float a = x[2 * i], bb = x[2 * i + 1];
            x[2 * i] = a * cs[i] - bb * sn[i];
            x[2 * i + 1] = bb * cs[i] + a * sn[i];
        }
    };
    for (int q = grp; q < 16; q += RPL) {
        uint4 pk = make_uint4(0, 0, 0, 0);
        if (q < G) {
            float x[8];
            unpack8<Tr>(*reinterpret_cast<const uint4 *>(p.qkv + row0 + (long long)(hk * G + q) * D), x);
            if (p.q_bias) add_bias8<Tr>(x, p.q_bias + (long long)(hk * G + q) * D + sub * 8);
            rope(x);
            pk = pack8<Tr>(x);
        }
        *reinterpret_cast<uint4 *>(qs + q * D + sub * 8) = pk;
    }
    {
        float xk[8], xv[8];
        unpack8<Tr>(*reinterpret_cast<const uint4 *>(p.qkv + row0 + (long long)(Hq + hk) * D), xk);
        const uint4 v_raw = *reinterpret_cast<const uint4 *>(p.qkv + row0 + (long long)(Hq + Hkv + hk) * D);
        vpk = v_raw;
        if (p.k_bias) add_bias8<Tr>(xk, p.k_bias + (long long)hk * D + sub * 8);
        if (p.v_bias) {
            unpack8<Tr>(v_raw, xv);
            add_bias8<Tr>(xv, p.v_bias + (long long)hk * D + sub * 8);
            vpk = pack8<Tr>(xv);
        }
        rope(xk);
        kpk = pack8<Tr>(xk);
    }
}

// This wave's slice [w0, w1) of the cached rows [0, pos): split and wave boundaries are multiples of 32 rows.
__device__ __forceinline__ void wave_slice(int pos, int S, int split, int wave, int &w0, int &w1) {
    int rows_per_split = (pos + S - 1) / S;
    rows_per_split = (rows_per_split + kTile - 1) / kTile * kTile;     // paged: tiles never straddle 16-row halves
    const int r0 = min(pos, split * rows_per_split);
    const int r1 = min(pos, r0 + rows_per_split);
    int per_wave = (r1 - r0 + kDecodeWaves - 1) / kDecodeWaves;
    per_wave = (per_wave + kTile - 1) / kTile * kTile;
    w0 = __builtin_amdgcn_readfirstlane(min(r1, r0 + wave * per_wave));   // wave-uniform
    w1 = __builtin_amdgcn_readfirstlane(min(r1, w0 + per_wave));
}

// The same over the rows [lo, pos) of a sliding window (decode_window_kernel.hip): boundaries are multiples of 32 rows
// measured from lo & ~31, so a tile still starts on a multiple of 32 and its 16-row halves each lie in one page.  The
// first tile may begin below lo; a wave with no row at or above lo gets the empty slice w0 == w1.  lo = 0 is the
// partition above.
__device__ __forceinline__ void wave_slice(int lo, int pos, int S, int split, int wave, int &w0, int &w1) {
    const int base = lo & ~(kTile - 1);
    int rows_per_split = (pos - base + S - 1) / S;
    rows_per_split = (rows_per_split + kTile - 1) / kTile * kTile;
    const int r0 = min(pos, base + split * rows_per_split);
    const int r1 = min(pos, r0 + rows_per_split);
    int per_wave = (r1 - r0 + kDecodeWaves - 1) / kDecodeWaves;
    per_wave = (per_wave + kTile - 1) / kTile * kTile;
    const int a = min(r1, r0 + wave * per_wave);
    const int e = min(r1, a + per_wave);
    w0 = __builtin_amdgcn_readfirstlane(e > lo ? a : e);                // wave-uniform
    w1 = __builtin_amdgcn_readfirstlane(e);
}

// Offsets of cache rows from head_base(), in elements.  Paged: the rows 0-15 and 16-31 of a tile each lie in ONE page
// (page_size >= 16, and see wave_slice): two scalar table look-ups per tile and a compile-time choice per load, no
// per-lane select.  Rows past the wave's end are clamped to its last row; clamping the page INDEX the same way keeps
// their address on that row.
template <bool PAGED> struct Pages {
    // (its own copies of the parameters it needs: a reference to the parameter block cost 4 VGPRs at head_dim 64)
    const int32_t *const tbl;
    int32_t *const status;
    const long long page_stride;
    const int page_shift, num_pages;
    const long long rs;
    const int pmask;
    int bad = 0;
    long long po[2] = {0, 0};                   // offsets of the pages of the tile being loaded
    __device__ __forceinline__ Pages(const DecodeKernelParams &p, int b)
        : tbl(PAGED ? p.block_table + (long long)b * p.table_stride : nullptr), status(p.status),
          page_stride(p.page_stride), page_shift(p.page_shift), num_pages(p.num_pages), rs(p.kv_row_stride),
          pmask(PAGED ? (1 << p.page_shift) - 1 : 0) {}
    __device__ __forceinline__ long long page_of(int idx) {
        int pg = tbl[idx];
        if ((unsigned)pg >= (unsigned)num_pages) {
            if (threadIdx.x == 0) atomicOr(status, 2);
            bad = 1;            // a read page outside the pool: page 0 is read instead, the output becomes NaN
            pg = 0;
        }
        return pg * page_stride;
    }
    // the pages of the tile at row t of a wave whose rows end at w1
    __device__ __forceinline__ void set(int t, int w1) {
        if (!PAGED) return;
        const int last = (w1 - 1) >> page_shift;
        po[0] = page_of(min(t >> page_shift, last));
        po[1] = page_of(min((t + 16) >> page_shift, last));
    }
    // the same for a wave whose rows begin at lo (lo < w1): rows below lo are re-addressed to row lo by the caller, so
    // page indices below lo's page are re-addressed to that page and no entry below it is looked at
    __device__ __forceinline__ void set(int t, int lo, int w1) {
        if (!PAGED) return;
        const int first = lo >> page_shift, last = (w1 - 1) >> page_shift;
        po[0] = page_of(min(max(t >> page_shift, first), last));
        po[1] = page_of(min(max((t + 16) >> page_shift, first), last));
    }
    // a row of the tile of set(); half = which 16 rows of the tile it lies in
    __device__ __forceinline__ long long row_off(int row, int half) const {
        if (!PAGED) return (long long)row * rs;
        return po[half] + (long long)(row & pmask) * rs;
    }
    // the row the new token is appended to (rejected() has checked its page)
    __device__ __forceinline__ long long append_off(int pos) {
        if (!PAGED) return (long long)pos * rs;
        return page_of(pos >> page_shift) + (long long)(pos & pmask) * rs;
    }
};

// A wave's attention state: Q^T in registers for the whole kernel, the fragments of the new key, and the running
// output / max / sum of query c (replicated over the 4 lane groups, which hold disjoint keys).
template <class Tr, int D> struct Tiles {
    static constexpr int NKS = D / 32;          // k-steps of a QK^T accumulator
    static constexpr int NDT = D / 16;          // 16-wide d tiles of O^T
    static constexpr int VS = MfmaLds<D>::VS;
    using Vec = typename Tr::mfma_vec;
    Vec qf[NKS];
    uint4 knf[NKS];
    f32x4 o[NDT];
    float m, l;

    // Prologue, second half: qs = the [16][D] query rows of rotate_new_token, kpk = this lane's 8 dims of the new key
    // as the attention sees it.  The region is reused as a V tile afterwards.
    __device__ __forceinline__ void init(uint16_t *qs, const uint4 &kpk) {
        const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
        uint16_t *const kn = qs + 16 * D;
        if (lane < D / 8) *reinterpret_cast<uint4 *>(kn + lane * 8) = kpk;
        // Q^T fragments (B operand): lane holds Q[q = c][32 ks + 8 g .. +8]
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) qf[ks] = bitcast<Vec>(*reinterpret_cast<const uint4 *>(qs + c * D + 32 * ks + 8 * g));
        // K fragments of the new-token tile: key 0 of the tile = k_new (lanes c == 0), everything else masked
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) knf[ks] = *reinterpret_cast<const uint4 *>(kn + 32 * ks + 8 * g);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
            for (int r = 0; r < 4; ++r) o[dt][r] = 0.f;
        m = neg_inf(); l = 0.f;
    }

    // one 32-key tile: kk = K fragments, V tile at buf, the first nvalid keys are real, scores * scale in log2 units.
    // LOWER (a sliding window): the keys below nlo are masked as well.
    template <bool LOWER = false>
    __device__ __forceinline__ void tile(const uint4 (&kk)[2][NKS], const char *buf, int nvalid, float scale, int nlo = 0) {
        const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
        f32x4 s[2];
#pragma unroll
        for (int kt = 0; kt < 2; ++kt) {
#pragma unroll
            for (int r = 0; r < 4; ++r) s[kt][r] = 0.f;
#pragma unroll
            for (int ks = 0; ks < NKS; ++ks) s[kt] = Mfma16<Tr>::run(bitcast<Vec>(kk[kt][ks]), qf[ks], s[kt]);
        }
        float mx = neg_inf();
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {       // element r of tile kt = key 16 kt + 4 g + r
                const int key = 16 * kt + 4 * g + r;
                s[kt][r] = (key < nvalid && (!LOWER || key >= nlo)) ? s[kt][r] * scale : neg_inf();
                mx = fmaxf(mx, s[kt][r]);
            }
        mx = fmaxf(m, quad_max(mx));
        const float ms = (mx == neg_inf()) ? 0.f : mx;
        const float alpha = fast_exp2(m - ms);
        m = mx;
        if (__any(alpha != 1.0f)) {
#pragma unroll
            for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
                for (int r = 0; r < 4; ++r) o[dt][r] *= alpha;
        }
        uint32_t pb[4];
        float ps[2];
#pragma unroll
        for (int kt = 0; kt < 2; ++kt) {
            const float p0 = fast_exp2(s[kt][0] - ms), p1 = fast_exp2(s[kt][1] - ms);
            const float p2 = fast_exp2(s[kt][2] - ms), p3 = fast_exp2(s[kt][3] - ms);
            ps[kt] = (p0 + p1) + (p2 + p3);
            pb[2 * kt] = Tr::pack2(p0, p1);
            pb[2 * kt + 1] = Tr::pack2(p2, p3);
        }
        // one fma, written out: the contraction the compiler chose for `l * alpha + ps[0]` must not vary by call site
        l = __builtin_fmaf(l, alpha, ps[0]) + ps[1];
        const Vec pv = bitcast<Vec>(make_uint4(pb[0], pb[1], pb[2], pb[3]));
        // V^T fragments: lane (c, g) reads rows 4 g + (c >> 2) and 16 + ..., 8 bytes at column 16 dt + 4 (c & 3)
        const char *vr = buf + VS * (4 * g + (c >> 2)) + 8 * (c & 3);
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt) {
            const auto t0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_i16x4 *)(vr + 32 * dt));
            const auto t1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_i16x4 *)(vr + VS * 16 + 32 * dt));
            u32x4 av;
            const u32x2 a_lo = bitcast<u32x2>(t0), a_hi = bitcast<u32x2>(t1);
            av[0] = a_lo[0]; av[1] = a_lo[1]; av[2] = a_hi[0]; av[3] = a_hi[1];
            o[dt] = Mfma16<Tr>::run(bitcast<Vec>(av), pv, o[dt]);
        }
    }

    // the new token: a tile with one real key.  The caller has filled EVERY row of the V tile with v_new (rows 1.. get
    // weight 0, but 0 * stale LDS bits could be NaN)
    __device__ __forceinline__ void new_token_tile(const char *buf, float scale) {
        uint4 kk[2][NKS];
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) {
            kk[0][ks] = knf[ks];                // only the lanes with c == 0 matter (key 0); the rest is masked
            kk[1][ks] = make_uint4(0, 0, 0, 0);
        }
        tile(kk, buf, 1, scale);
    }

    // Merge the workgroup's waves through LDS (after every wave is done with its tiles) and write the G output rows
    // (num_splits == 1) or partials of this kv head, times out_scale.  bad_page: a page outside the pool was read.
    // SINK: sinks[h] (natural-log units, not scaled) is one more stream element of query head h -- max sinks[h] log2(e),
    // sum 1, accumulator 0 -- folded in after the waves' merge by split 0 alone, so a row counts it once whatever the
    // split count and whether or not split 0 had a tile; the output row and the partials both carry it, and the split
    // combine is the one of the kernels without a sink.
    template <bool SINK = false>
    __device__ __forceinline__ void merge_store(const DecodeKernelParams &p, char *smem, int b, int hk, int split, int G,
                                                bool bad_page, float out_scale, const float *sinks = nullptr) {
        constexpr int W = kDecodeWaves, LPR = D / 8;
        const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, c = lane & 15, g = lane >> 4;
        const int S = p.num_splits;
        if (bad_page) l = __builtin_nanf("");
        const float ltot = quad_sum(l);
        __syncthreads();
        float *const red = reinterpret_cast<float *>(smem);                 // [W][G][D + 2]
        if (c < G) {
#pragma unroll
            for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
                for (int r = 0; r < 4; ++r) red[(wave * G + c) * (D + 2) + 16 * dt + 4 * g + r] = o[dt][r];
            if (g == 0) { red[(wave * G + c) * (D + 2) + D] = m; red[(wave * G + c) * (D + 2) + D + 1] = ltot; }
        }
        __syncthreads();
        for (int idx = tid; idx < LPR * G; idx += W * 64) {
            const int q = idx / LPR, sb = idx % LPR;
            Stream tot;
            tot.init();
#pragma unroll
            for (int w = 0; w < W; ++w) {
                const float *rw = red + (w * G + q) * (D + 2);
                float a2[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) a2[j] = rw[sb * 8 + j];
                tot.merge(rw[D], rw[D + 1], a2);
            }
            if constexpr (SINK) {
                if (split == 0) {
                    const float zero[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                    // launder the product: contracted into the merge's `m2 - max` as one fma it leaves the product's
                    // rounding error where 0 belongs when the sink IS the max -- 2^(+-1e22) for a sink of -1e30
                    float sk = sinks[hk * G + q] * 1.4426950408889634f;
                    asm volatile("" : "+v"(sk));
                    tot.merge(sk, 1.0f, zero);
                }
            }
            const long long bh = (long long)b * p.H + hk * G + q;
            if (S == 1) {
                const float inv = out_scale / tot.l;     // l >= 1: the new token is always present
                float y[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) y[j] = tot.acc[j] * inv;
                *reinterpret_cast<uint4 *>(p.o + bh * D + sb * 8) = pack8<Tr>(y);
            } else {
                float *po = p.part_o + (bh * S + split) * D + sb * 8;
                *reinterpret_cast<float4 *>(po) = make_float4(tot.acc[0] * out_scale, tot.acc[1] * out_scale,
                                                              tot.acc[2] * out_scale, tot.acc[3] * out_scale);
                *reinterpret_cast<float4 *>(po + 4) = make_float4(tot.acc[4] * out_scale, tot.acc[5] * out_scale,
                                                                  tot.acc[6] * out_scale, tot.acc[7] * out_scale);
                if (sb == 0) p.part_ml[bh * S + split] = make_float2(tot.m, tot.l);
            }
        }
    }
};

}  // namespace decode
}  // namespace sfa
