// sfa_decode_kv8: sfa_decode over caches of one byte per element (OCP e4m3, torch's float8_e4m3fn), and
// sfa_kv8_quantize, which moves rows of a 16-bit cache into such a cache.
//
// One matrix-core kernel for every group size: the design of decode_gqa_mfma_kernel.hip, whose body this kernel shares
// through decode_mfma_common.h (rejection, prologue, wave slice, paging, the tile math and the merge of the waves), with
// G = 1 .. 16 a run-time value.  What is this file's own: the caches are read on the row-major path in all three layouts,
//   a lane loads 16 bytes = 16 elements, so D/16 lanes cover a cache row and one load instruction of a wave 64/(D/16)
//   rows; the bytes are converted to the 16-bit dtype in registers (v_cvt_scalef32_pk_{bf16,f16}_fp8 with scale 1.0:
//   every e4m3 value is exact in fp16 and in bf16) and written to the wave-private K and V tiles in LDS;
// the software pipeline (kInFlight), the quantisation of the new token and its append, and kv8_quantize_kernel.
// The scales never touch the tiles: k_scale[hk] is folded into the fp32 score scale, v_scale[hk] multiplies the fp32
// accumulator once in the epilogue (before the partials are written when the key range is split, so
// decode_combine_kernel merges them unchanged).
// The new token is quantised first, q8(x16 / scale), and takes part in the attention through its dequantised value: the
// output is a function of the cache contents after the step.
// Two tiles per wave are in flight in registers (2 x 8 KB at head_dim 128, the bytes decode_gqa_mfma_kernel keeps in
// flight with one 16-bit tile).
#include "decode_mfma_common.h"

namespace sfa {

namespace {

using namespace decode;

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

constexpr int kInFlight = 2;                    // tiles a wave keeps in flight in registers (3 measured no better, and
                                                // 20-30 % slower through a paged cache: DESIGN.md 5.8)

template <class Tr, int D, bool NT, bool PAGED>
__global__ void __launch_bounds__(kDecodeWaves * 64)
decode_kv8_kernel(const Kv8KernelParams kp) {
    using Lds = MfmaLds<D>;
    constexpr int LPR = D / 8;                  // prologue: lanes (8 16-bit elements each) per head row
    constexpr int LP8 = D / 16;                 // lanes (16-byte chunks = 16 elements) per cache row
    constexpr int RP8 = 64 / LP8;               // cache rows one load instruction of a wave covers
    constexpr int NL8 = kTile / RP8;            // loads per 32-row tile
    constexpr int NKS = D / 32;                 // k-steps of a QK^T accumulator
    constexpr int VS = Lds::VS, KS = Lds::KS;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const DecodeKernelParams &p = kp.d;

    const int hk = blockIdx.x, split = blockIdx.y, b = blockIdx.z;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int c = lane & 15, g = lane >> 4;     // MFMA lane coordinates
    const int sub = lane % LPR, grp = lane / LPR;       // prologue coordinates: which 8 dims, which head of a pass
    const int sub8 = lane % LP8, grp8 = lane / LP8;     // cache coordinates: which 16 dims, which row of a load
    const int S = p.num_splits;
    const int G = p.H / p.Hkv;                  // 1 .. 16 real query columns

    const int pos = p.seq_len[b];
    if (rejected<Tr, D, PAGED>(p, b, hk, split, G, pos)) return;
    const float ksc = kp.k_scale ? kp.k_scale[hk] : 1.0f;
    const float vsc = kp.v_scale ? kp.v_scale[hk] : 1.0f;
    const float sl2 = p.scale_log2 * ksc;       // scores of the dequantised keys, in log2 units

    // wave-private LDS: a V tile (also the Q / k_new re-layout area) and a K tile
    char *const vbuf = smem + wave * Lds::WAVE_LDS;
    char *const kbuf = vbuf + Lds::VTILE;

    // the new token: k16 / v16 exactly as sfa_decode would store them, then quantised; kpk / vpk = the dequantised
    // 16-bit values the attention uses, k8 / v8 = the bytes the append stores
    uint2 k8, v8;
    uint4 kpk, vpk;
    rotate_new_token<Tr, D>(p, b, hk, G, pos, reinterpret_cast<uint16_t *>(vbuf), kpk, vpk);
    {
        float xk[8], xv[8];
        unpack8<Tr>(kpk, xk);
        unpack8<Tr>(vpk, xv);
        k8 = q8x8(xk, ksc);
        v8 = q8x8(xv, vsc);
        kpk = dq8<Tr>(k8.x, k8.y);
        vpk = dq8<Tr>(v8.x, v8.y);
    }
    Tiles<Tr, D> st;
    st.init(reinterpret_cast<uint16_t *>(vbuf), kpk);

    int w0, w1;
    wave_slice(pos, S, split, wave, w0, w1);
    Pages<PAGED> pg(p, b);                      // (strides and offsets are in elements = bytes)
    uint8_t *const kc = reinterpret_cast<uint8_t *>(p.k_cache) + head_base<D, PAGED>(p, b, hk);
    uint8_t *const vc = reinterpret_cast<uint8_t *>(p.v_cache) + head_base<D, PAGED>(p, b, hk);

    // a tile of both caches as it lies in memory: load i covers the rows RP8 i + grp8, this lane's 16 bytes of each
    struct Raw { uint4 k[NL8], v[NL8]; };
    auto load = [&](Raw &x, int t) {
        pg.set(t, w1);
#pragma unroll
        for (int i = 0; i < NL8; ++i) {
            const int row = min(t + RP8 * i + grp8, w1 - 1);
            const long long off = pg.row_off(row, (RP8 * i) >> 4) + 16 * sub8;
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
                    st.tile(kf, vbuf, w1 - tj, sl2);
                }
            }
        }
    }

    // ---- the new token (position `pos`): last split, wave 0 ----
    if (split == S - 1 && wave == 0) {
        // every row of the V tile = v_new (Tiles::new_token_tile)
        for (int r = grp; r < kTile; r += 64 / LPR) *reinterpret_cast<uint4 *>(vbuf + VS * r + 16 * sub) = vpk;
        st.new_token_tile(vbuf, sl2);
        if (grp == 0) {                         // append: LPR lanes x 8 B = one row of D bytes each
            const long long roff = pg.append_off(pos) + sub * 8;
            *reinterpret_cast<uint2 *>(kc + roff) = k8;
            *reinterpret_cast<uint2 *>(vc + roff) = v8;
        }
    }

    // v_scale: once, on the fp32 accumulator
    st.merge_store(p, smem, b, hk, split, G, PAGED && pg.bad, vsc);
}

template <class Tr, int D, bool NT, bool PAGED>
int launch_k(const Kv8KernelParams &kp, hipStream_t stream) {
    const DecodeKernelParams &p = kp.d;
    dim3 grid(p.Hkv, p.num_splits, p.B), block(kDecodeWaves * 64);
    constexpr int lds = MfmaLds<D>::BYTES;
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
    const bool nt = decode_nt(p, head_dim, 1);
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
