// sfa_decode_kv8: sfa_decode over caches of one byte per element (OCP e4m3, torch's float8_e4m3fn), and
// sfa_kv8_quantize, which moves rows of a 16-bit cache into such a cache.
//
// One matrix-core kernel for every group size: decode_gqa_mfma_kernel.hip's design (one workgroup per (batch, kv head,
// split), four waves, 32-key tiles on v_mfma_f32_16x16x32, 16 query columns of which G = 1 .. 16 are real, one online
// softmax state per lane) on its row-major path for all three cache layouts:
//   a lane loads 16 bytes = 16 elements, so D/16 lanes cover a cache row and one load instruction of a wave 64/(D/16)
//   rows; the bytes are converted to the 16-bit dtype in registers (v_cvt_scalef32_pk_{bf16,f16}_fp8 with scale 1.0:
//   every e4m3 value is exact in fp16 and in bf16) and written to the wave-private K and V tiles in LDS, in the layouts
//   of decode_gqa_mfma_kernel.hip; from there on the tile math is that kernel's.
// The scales never touch the tiles: k_scale[hk] is folded into the fp32 score scale, v_scale[hk] multiplies the fp32
// accumulator once in the epilogue (before the partials are written when the key range is split, so
// decode_combine_kernel merges them unchanged).
// The new token is quantised first, q8(x16 / scale), and takes part in the attention through its dequantised value: the
// output is a function of the cache contents after the step.
// Two tiles per wave are in flight in registers (2 x 8 KB at head_dim 128, the bytes decode_gqa_mfma_kernel keeps in
// flight with one 16-bit tile).
#include "decode_common.h"

namespace sfa {

namespace {

using namespace decode;

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

// ---- e4m3 <-> 16 bit ----------------------------------------------------------------------------------------------
// two e4m3 bytes (the low or the high half of w) -> two 16-bit values, exact
template <class Tr, bool HI> __device__ __forceinline__ uint32_t dq2(uint32_t w);
template <> __device__ __forceinline__ uint32_t dq2<Bf16, false>(uint32_t w) {
    return bitcast<uint32_t>(__builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, 1.0f, false));
}
template <> __device__ __forceinline__ uint32_t dq2<Bf16, true>(uint32_t w) {
    return bitcast<uint32_t>(__builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, 1.0f, true));
}
template <> __device__ __forceinline__ uint32_t dq2<Fp16, false>(uint32_t w) {
    return bitcast<uint32_t>(__builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w, 1.0f, false));
}
template <> __device__ __forceinline__ uint32_t dq2<Fp16, true>(uint32_t w) {
    return bitcast<uint32_t>(__builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w, 1.0f, true));
}
// 8 bytes -> 8 16-bit values
template <class Tr> __device__ __forceinline__ uint4 dq8(uint32_t a, uint32_t b) {
    return make_uint4(dq2<Tr, false>(a), dq2<Tr, true>(a), dq2<Tr, false>(b), dq2<Tr, true>(b));
}

// q8 of four values: clamp to +-448 in fp32 (so the conversion's own overflow mode never matters), round to the nearest
// e4m3 with ties to even, NaN -> 0x7F
__device__ __forceinline__ uint32_t q8x4(float a, float b, float c, float d) {
    auto cl = [](float x) { return fminf(fmaxf(x, -448.f), 448.f); };
    int w = __builtin_amdgcn_cvt_pk_fp8_f32(cl(a), cl(b), 0, false);
    w = __builtin_amdgcn_cvt_pk_fp8_f32(cl(c), cl(d), w, true);
    uint32_t u = (uint32_t)w;
    if (a != a) u = (u & 0xffffff00u) | 0x0000007fu;
    if (b != b) u = (u & 0xffff00ffu) | 0x00007f00u;
    if (c != c) u = (u & 0xff00ffffu) | 0x007f0000u;
    if (d != d) u = (u & 0x00ffffffu) | 0x7f000000u;
    return u;
}
// q8(x[j] / scale) for 8 values (the division is the correctly rounded fp32 one)
__device__ __forceinline__ uint2 q8x8(const float (&x)[8], float scale) {
    return make_uint2(q8x4(x[0] / scale, x[1] / scale, x[2] / scale, x[3] / scale),
                      q8x4(x[4] / scale, x[5] / scale, x[6] / scale, x[7] / scale));
}

constexpr int kTile = 32;                       // keys per tile
constexpr int kInFlight = 2;                    // tiles a wave keeps in flight in registers (3 measured no better, and
                                                // 20-30 % slower through a paged cache: DESIGN.md 5.8)

template <class Tr, int D, bool NT, bool PAGED>
__global__ void __launch_bounds__(kDecodeWaves * 64)
decode_kv8_kernel(const Kv8KernelParams kp) {
    constexpr int W = kDecodeWaves;
    constexpr int LPR = D / 8;                  // prologue: lanes (8 16-bit elements each) per head row
    constexpr int RPL = 64 / LPR;               // prologue: heads one pass of a wave covers
    constexpr int LP8 = D / 16;                 // lanes (16-byte chunks = 16 elements) per cache row
    constexpr int RP8 = 64 / LP8;               // cache rows one load instruction of a wave covers
    constexpr int NL8 = kTile / RP8;            // loads per 32-row tile
    constexpr int NKS = D / 32;                 // k-steps of a QK^T accumulator
    constexpr int NDT = D / 16;                 // 16-wide d tiles of O^T
    constexpr int VS = 2 * D + 32;              // LDS row stride of the V tile (conflict-free transposed reads)
    constexpr int VTILE = kTile * VS;
    constexpr int KS = 2 * D + 16;              // LDS row stride of the K tile
    constexpr int KTILE = kTile * KS;
    constexpr int WAVE_LDS = VTILE + KTILE;
    using Vec = typename Tr::mfma_vec;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const DecodeKernelParams &p = kp.d;

    const int hk = blockIdx.x, split = blockIdx.y, b = blockIdx.z;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int c = lane & 15, g = lane >> 4;     // MFMA lane coordinates
    const int sub = lane % LPR, grp = lane / LPR;       // prologue coordinates: which 8 dims, which head of a pass
    const int sub8 = lane % LP8, grp8 = lane / LP8;     // cache coordinates: which 16 dims, which row of a load
    const int S = p.num_splits;
    const int Hq = p.H, Hkv = p.Hkv;
    const int G = Hq / Hkv;                     // 1 .. 16 real query columns

    const int pos = p.seq_len[b];
    const int reject = reject_code<PAGED>(p, b, pos);      // sfa_decode's contract: poison, flag, touch nothing
    if (reject) {
        if (split == 0) {
            for (int i = tid; i < G * D; i += W * 64)
                p.o[((long long)b * Hq + (long long)hk * G) * D + i] = Tr::id == 0 ? 0x7e00 : 0x7fc0;
            if (tid == 0 && hk == 0) atomicOr(p.status, reject);
        }
        return;
    }
    const float ksc = kp.k_scale ? kp.k_scale[hk] : 1.0f;
    const float vsc = kp.v_scale ? kp.v_scale[hk] : 1.0f;
    const float sl2 = p.scale_log2 * ksc;       // scores of the dequantised keys, in log2 units

    // wave-private LDS: a V tile (also the Q / k_new re-layout area) and a K tile
    char *const vbuf = smem + wave * WAVE_LDS;
    char *const kbuf = vbuf + VTILE;

    // ---- prologue (every wave; lane `sub` owns dims 8 sub .. +8, lane group `grp` handles query heads grp,
    // grp + RPL, ...): bias, RoPE (fp32), round to storage, park in LDS in [head][d] order ----
    const long long row0 = (long long)b * p.qkv_stride + sub * 8;
    float cs[4], sn[4];
    const int rot = p.rot_dim;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int pj = sub * 4 + i;
        cs[i] = 1.f; sn[i] = 0.f;
        if (2 * pj < rot) {
            if (p.cos_tab) {
                const long long ti = (long long)pos * (rot >> 1) + pj;
                cs[i] = Tr::to_f32(p.cos_tab[ti]);
                sn[i] = Tr::to_f32(p.sin_tab[ti]);
            } else {                            // same fp32 recipe as decode_kernel.hip
                const float inv_freq = 1.0f / powf(10000.0f, (float)(2 * pj) / (float)rot);
                sincosf((float)pos * inv_freq, &sn[i], &cs[i]);
            }
        }
    }
    auto rope = [&](float (&x)[8]) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float a = x[2 * i], bb = x[2 * i + 1];
            x[2 * i] = a * cs[i] - bb * sn[i];
            x[2 * i + 1] = bb * cs[i] + a * sn[i];
        }
    };
    uint16_t *const qs = reinterpret_cast<uint16_t *>(vbuf);            // [16][D] query rows (rows >= G zero)
    uint16_t *const kn = qs + 16 * D;                                   // [D] the new token's key, dequantised
    for (int q = grp; q < 16; q += RPL) {
        uint4 pk = make_uint4(0, 0, 0, 0);
        if (q < G) {
            float x[8];
            unpack8<Tr>(*reinterpret_cast<const uint4 *>(p.qkv + row0 + (long long)(hk * G + q) * D), x);
            if (p.q_bias) {
                float t[8];
                unpack8<Tr>(*reinterpret_cast<const uint4 *>(p.q_bias + (long long)(hk * G + q) * D + sub * 8), t);
#pragma unroll
                for (int j = 0; j < 8; ++j) x[j] += t[j];
            }
            rope(x);
            pk = pack8<Tr>(x);
        }
        *reinterpret_cast<uint4 *>(qs + q * D + sub * 8) = pk;
    }
    // the new token: k16 / v16 exactly as sfa_decode would store them, then quantised; kpk / vpk = the dequantised
    // 16-bit values the attention uses, k8 / v8 = the bytes the append stores
    uint2 k8, v8;
    uint4 kpk, vpk;
    {
        float xk[8], xv[8];
        unpack8<Tr>(*reinterpret_cast<const uint4 *>(p.qkv + row0 + (long long)(Hq + hk) * D), xk);
        uint4 v16 = *reinterpret_cast<const uint4 *>(p.qkv + row0 + (long long)(Hq + Hkv + hk) * D);
        if (p.k_bias) {
            float t[8]; unpack8<Tr>(*reinterpret_cast<const uint4 *>(p.k_bias + (long long)hk * D + sub * 8), t);
#pragma unroll
            for (int j = 0; j < 8; ++j) xk[j] += t[j];
        }
        if (p.v_bias) {
            float t[8]; unpack8<Tr>(*reinterpret_cast<const uint4 *>(p.v_bias + (long long)hk * D + sub * 8), t);
            unpack8<Tr>(v16, xv);
#pragma unroll
            for (int j = 0; j < 8; ++j) xv[j] += t[j];
            v16 = pack8<Tr>(xv);
        }
        rope(xk);
        unpack8<Tr>(pack8<Tr>(xk), xk);         // k16
        unpack8<Tr>(v16, xv);
        k8 = q8x8(xk, ksc);
        v8 = q8x8(xv, vsc);
        kpk = dq8<Tr>(k8.x, k8.y);
        vpk = dq8<Tr>(v8.x, v8.y);
        if (grp == 0) *reinterpret_cast<uint4 *>(kn + sub * 8) = kpk;
    }
    // Q^T fragments (B operand): lane holds Q[q = c][32 ks + 8 g .. +8]
    Vec qf[NKS];
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) qf[ks] = bitcast<Vec>(*reinterpret_cast<const uint4 *>(qs + c * D + 32 * ks + 8 * g));
    // K fragments of the new-token tile: key 0 of the tile = k_new (lanes c == 0), everything else masked
    uint4 knf[NKS];
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) knf[ks] = *reinterpret_cast<const uint4 *>(kn + 32 * ks + 8 * g);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // the region is reused as a V tile below

    // ---- this wave's slice of the cached rows [0, pos) ----
    int rows_per_split = (pos + S - 1) / S;
    rows_per_split = (rows_per_split + kTile - 1) / kTile * kTile;     // paged: tiles never straddle 16-row halves
    const int r0 = min(pos, split * rows_per_split);
    const int r1 = min(pos, r0 + rows_per_split);
    int per_wave = (r1 - r0 + W - 1) / W;
    per_wave = (per_wave + kTile - 1) / kTile * kTile;
    const int w0 = __builtin_amdgcn_readfirstlane(min(r1, r0 + wave * per_wave));   // wave-uniform
    const int w1 = __builtin_amdgcn_readfirstlane(min(r1, w0 + per_wave));

    // (strides and offsets are in elements = bytes)
    const long long rs = p.kv_row_stride;
    // paged: split and wave boundaries are multiples of 32 rows, so the rows 0-15 and 16-31 of a tile each lie in ONE
    // page (page_size >= 16): two scalar table look-ups per tile and a compile-time choice per load.  Rows past the
    // wave's end are clamped to its last row; clamping the page INDEX the same way keeps their address on that row.
    const long long head_base = PAGED ? (long long)p.layer * (rs << p.page_shift) + (long long)hk * p.kv_head_stride
                                      : ((long long)b * p.L + p.layer) * p.M * Hkv * D + hk * p.kv_head_stride;
    const int32_t *tbl = PAGED ? p.block_table + (long long)b * p.table_stride : nullptr;
    const int pmask = PAGED ? (1 << p.page_shift) - 1 : 0;
    int bad_page = 0;
    auto page_of = [&](int idx) -> long long {
        int pg = tbl[idx];
        if ((unsigned)pg >= (unsigned)p.num_pages) {
            if (tid == 0) atomicOr(p.status, 2);
            bad_page = 1;       // a read page outside the pool: page 0 is read instead, the output becomes NaN
            pg = 0;
        }
        return pg * p.page_stride;
    };
    long long po[2] = {0, 0};                   // offsets of the pages of the tile being loaded
    auto set_pages = [&](int t) {
        if (!PAGED) return;
        const int last = (w1 - 1) >> p.page_shift;
        po[0] = page_of(min(t >> p.page_shift, last));
        po[1] = page_of(min((t + 16) >> p.page_shift, last));
    };
    auto row_off = [&](int row, int half) -> long long {
        if (!PAGED) return (long long)row * rs;
        return po[half] + (long long)(row & pmask) * rs;
    };
    uint8_t *const kc = reinterpret_cast<uint8_t *>(p.k_cache) + head_base;
    uint8_t *const vc = reinterpret_cast<uint8_t *>(p.v_cache) + head_base;

    f32x4 o[NDT];
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
        for (int r = 0; r < 4; ++r) o[dt][r] = 0.f;
    float m = neg_inf(), l = 0.f;               // per lane: query c (replicated over the 4 lane groups)

    // a tile of both caches as it lies in memory: load i covers the rows RP8 i + grp8, this lane's 16 bytes of each
    struct Raw { uint4 k[NL8], v[NL8]; };
    auto load = [&](Raw &x, int t) {
        set_pages(t);
#pragma unroll
        for (int i = 0; i < NL8; ++i) {
            const int row = min(t + RP8 * i + grp8, w1 - 1);
            const long long off = row_off(row, (RP8 * i) >> 4) + 16 * sub8;
            x.k[i] = ld16<NT>(reinterpret_cast<const uint16_t *>(kc + off));
            x.v[i] = ld16<NT>(reinterpret_cast<const uint16_t *>(vc + off));
        }
    };
    // bytes -> 16 bit, row-major into the wave's LDS tiles; then the K fragments in operand layout
    auto stage = [&](const Raw &x, uint4 (&kf)[2][NKS]) {
#pragma unroll
        for (int i = 0; i < NL8; ++i) {
            char *const vd = vbuf + VS * (RP8 * i + grp8) + 32 * sub8;
            *reinterpret_cast<uint4 *>(vd) = dq8<Tr>(x.v[i].x, x.v[i].y);
            *reinterpret_cast<uint4 *>(vd + 16) = dq8<Tr>(x.v[i].z, x.v[i].w);
            char *const kd = kbuf + KS * (RP8 * i + grp8) + 32 * sub8;
            *reinterpret_cast<uint4 *>(kd) = dq8<Tr>(x.k[i].x, x.k[i].y);
            *reinterpret_cast<uint4 *>(kd + 16) = dq8<Tr>(x.k[i].z, x.k[i].w);
        }
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
            for (int ks = 0; ks < NKS; ++ks)
                kf[kt][ks] = *reinterpret_cast<const uint4 *>(kbuf + KS * (16 * kt + c) + 64 * ks + 16 * g);
    };
    // one 32-key tile: kk = K fragments, V tile at vbuf, keys [t, t + nvalid) are real
    auto tile = [&](const uint4 (&kk)[2][NKS], int nvalid) {
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
                s[kt][r] = (16 * kt + 4 * g + r < nvalid) ? s[kt][r] * sl2 : neg_inf();
                mx = fmaxf(mx, s[kt][r]);
            }
        mx = fmaxf(m, quad_max(mx));
        const float ms = (mx == neg_inf()) ? 0.f : mx;
        const float alpha = fast_exp2(m - ms);
        m = mx;
        l *= alpha;
        if (__any(alpha != 1.0f)) {
#pragma unroll
            for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
                for (int r = 0; r < 4; ++r) o[dt][r] *= alpha;
        }
        uint32_t pb[4];
#pragma unroll
        for (int kt = 0; kt < 2; ++kt) {
            const float p0 = fast_exp2(s[kt][0] - ms), p1 = fast_exp2(s[kt][1] - ms);
            const float p2 = fast_exp2(s[kt][2] - ms), p3 = fast_exp2(s[kt][3] - ms);
            l += (p0 + p1) + (p2 + p3);
            pb[2 * kt] = Tr::pack2(p0, p1);
            pb[2 * kt + 1] = Tr::pack2(p2, p3);
        }
        const Vec pv = bitcast<Vec>(make_uint4(pb[0], pb[1], pb[2], pb[3]));
        // V^T fragments: lane (c, g) reads rows 4 g + (c >> 2) and 16 + ..., 8 bytes at column 16 dt + 4 (c & 3)
        const char *vr = vbuf + VS * (4 * g + (c >> 2)) + 8 * (c & 3);
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt) {
            const auto t0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_i16x4 *)(vr + 32 * dt));
            const auto t1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_i16x4 *)(vr + VS * 16 + 32 * dt));
            u32x4 av;
            const u32x2 a_lo = bitcast<u32x2>(t0), a_hi = bitcast<u32x2>(t1);
            av[0] = a_lo[0]; av[1] = a_lo[1]; av[2] = a_hi[0]; av[3] = a_hi[1];
            o[dt] = Mfma16<Tr>::run(bitcast<Vec>(av), pv, o[dt]);
        }
    };

    if (w0 < w1) {
        // tiles t+1 .. t+kInFlight are in flight into registers while tile t is computed; the LDS tiles are single: a
        // wave's LDS operations execute in order, so staging tile t+1 cannot overtake the reads of tile t
        Raw x[kInFlight];
        uint4 kf[2][NKS];
#pragma unroll
        for (int j = 0; j < kInFlight; ++j)
            if (w0 + j * kTile < w1) load(x[j], w0 + j * kTile);
        for (int t = w0; t < w1; t += kInFlight * kTile) {
#pragma unroll
            for (int j = 0; j < kInFlight; ++j) {
                const int tj = t + j * kTile;
                if (tj < w1) {
                    stage(x[j], kf);
                    if (tj + kInFlight * kTile < w1) load(x[j], tj + kInFlight * kTile);
                    tile(kf, w1 - tj);
                }
            }
        }
    }

    // ---- the new token (position `pos`): last split, wave 0 -- a tile with one real key ----
    if (split == S - 1 && wave == 0) {
        // every row of the V tile = v_new (rows 1.. get weight 0, but 0 * stale LDS bits could be NaN)
        for (int r = grp; r < kTile; r += RPL) *reinterpret_cast<uint4 *>(vbuf + VS * r + 16 * sub) = vpk;
        uint4 kk[2][NKS];
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) {
            kk[0][ks] = knf[ks];                // only the lanes with c == 0 matter (key 0); the rest is masked
            kk[1][ks] = make_uint4(0, 0, 0, 0);
        }
        tile(kk, 1);
        if (grp == 0) {                         // append: LPR lanes x 8 B = one row of D bytes each
            long long roff = (long long)pos * rs + sub * 8;
            if (PAGED) roff = page_of(pos >> p.page_shift) + (long long)(pos & pmask) * rs + sub * 8;
            *reinterpret_cast<uint2 *>(kc + roff) = k8;
            *reinterpret_cast<uint2 *>(vc + roff) = v8;
        }
    }

    // ---- merge the workgroup's waves through LDS (after every wave is done with its tiles) ----
    if (PAGED && bad_page) l = __builtin_nanf("");
    const float ltot = quad_sum(l);             // the four lane groups hold disjoint keys of query c
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
        const long long bh = (long long)b * Hq + hk * G + q;
        // v_scale: once, on the fp32 accumulator
        if (S == 1) {
            const float inv = vsc / tot.l;           // l >= 1: the new token is always present
            float y[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) y[j] = tot.acc[j] * inv;
            *reinterpret_cast<uint4 *>(p.o + bh * D + sb * 8) = pack8<Tr>(y);
        } else {
            float *po2 = p.part_o + (bh * S + split) * D + sb * 8;
            *reinterpret_cast<float4 *>(po2) = make_float4(tot.acc[0] * vsc, tot.acc[1] * vsc, tot.acc[2] * vsc, tot.acc[3] * vsc);
            *reinterpret_cast<float4 *>(po2 + 4) = make_float4(tot.acc[4] * vsc, tot.acc[5] * vsc, tot.acc[6] * vsc, tot.acc[7] * vsc);
            if (sb == 0) p.part_ml[bh * S + split] = make_float2(tot.m, tot.l);
        }
    }
}

template <class Tr, int D, bool NT, bool PAGED>
int launch_k(const Kv8KernelParams &kp, hipStream_t stream) {
    const DecodeKernelParams &p = kp.d;
    dim3 grid(p.Hkv, p.num_splits, p.B), block(kDecodeWaves * 64);
    constexpr int lds = kDecodeWaves * kTile * ((2 * D + 32) + (2 * D + 16));       // 71,680 B at head_dim 128
    static_assert(lds >= kDecodeWaves * 16 * (D + 2) * 4, "merge area fits");
    static_assert(kTile * (2 * D + 32) >= 17 * D * 2, "the query rows and the new key fit the V tile they are re-laid out in");
    static DynLdsAttr attr;
    if (const int rc = attr.ensure(reinterpret_cast<const void *>(&decode_kv8_kernel<Tr, D, NT, PAGED>), lds,
                                   "decode_kv8_kernel"))
        return rc;
    hipLaunchKernelGGL((decode_kv8_kernel<Tr, D, NT, PAGED>), grid, block, lds, stream, kp);
    return check_launch("decode_kv8_kernel");
}

template <class Tr, int D>
int launch_d(const Kv8KernelParams &kp, bool nt, hipStream_t stream) {
    if (kp.d.block_table) return nt ? launch_k<Tr, D, true, true>(kp, stream) : launch_k<Tr, D, false, true>(kp, stream);
    return nt ? launch_k<Tr, D, true, false>(kp, stream) : launch_k<Tr, D, false, false>(kp, stream);
}

// ---- sfa_kv8_quantize: dst[r, h, d] = q8(src[r, h, d] / scale[h]).  A thread owns 16 elements: two 16-byte loads, one
// 16-byte store.
template <class Tr>
__global__ void __launch_bounds__(256)
kv8_quantize_kernel(uint8_t *dst, const uint16_t *src, const float *scale, long long rows, int Hkv, int chunks,
                    long long src_row, long long src_head, long long dst_row, long long dst_head) {
    const long long total = rows * Hkv * chunks;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int ch = (int)(i % chunks);
        const long long rh = i / chunks;
        const int h = (int)(rh % Hkv);
        const long long r = rh / Hkv;
        const uint16_t *s = src + r * src_row + h * src_head + 16 * ch;
        const float sc = scale ? scale[h] : 1.0f;
        float x[8], y[8];
        unpack8<Tr>(*reinterpret_cast<const uint4 *>(s), x);
        unpack8<Tr>(*reinterpret_cast<const uint4 *>(s + 8), y);
        const uint2 a = q8x8(x, sc), bq = q8x8(y, sc);
        *reinterpret_cast<uint4 *>(dst + r * dst_row + h * dst_head + 16 * ch) = make_uint4(a.x, a.y, bq.x, bq.y);
    }
}

}  // namespace

// head_dim 64 / 128, any cache layout, 1, 2, 4, 8 or 16 query heads per kv head; adds the split combine
int launch_decode_kv8(const Kv8KernelParams &kp, int dtype, int head_dim, hipStream_t stream) {
    const DecodeKernelParams &p = kp.d;
    // both caches, one byte per element, against the 256 MB Infinity Cache (decode_dispatch.hip)
    bool nt = 2ll * p.B * p.L * p.M * p.Hkv * head_dim > (256ll << 20);
    if (const int k = g_knobs.decode_nt.load(std::memory_order_relaxed); k >= 0) nt = k != 0;
    const bool h = dtype == SFA_DTYPE_FP16;
    const int rc = head_dim == 64 ? (h ? launch_d<Fp16, 64>(kp, nt, stream) : launch_d<Bf16, 64>(kp, nt, stream))
                                  : (h ? launch_d<Fp16, 128>(kp, nt, stream) : launch_d<Bf16, 128>(kp, nt, stream));
    if (rc != SFA_OK || p.num_splits <= 1) return rc;
    return launch_decode_combine(p, dtype, head_dim, stream);
}

int launch_kv8_quantize(void *dst, const void *src, const float *scale, long long rows, int Hkv, int head_dim,
                        long long src_row, long long src_head, long long dst_row, long long dst_head, int dtype,
                        hipStream_t stream) {
    const int chunks = head_dim / 16;
    const long long threads = rows * Hkv * chunks;
    if (threads == 0) return SFA_OK;
    const long long blocks = (threads + 255) / 256;
    dim3 grid((unsigned)(blocks < 65536 ? blocks : 65536)), block(256);
    if (dtype == SFA_DTYPE_FP16)
        hipLaunchKernelGGL((kv8_quantize_kernel<Fp16>), grid, block, 0, stream, (uint8_t *)dst, (const uint16_t *)src, scale,
                           rows, Hkv, chunks, src_row, src_head, dst_row, dst_head);
    else
        hipLaunchKernelGGL((kv8_quantize_kernel<Bf16>), grid, block, 0, stream, (uint8_t *)dst, (const uint16_t *)src, scale,
                           rows, Hkv, chunks, src_row, src_head, dst_row, dst_head);
    return check_launch("kv8_quantize_kernel");
}

}  // namespace sfa
