// The body of the matrix-core decode kernels over e4m3 caches, from the rejection to the merge of the waves: ONE copy for
// decode_kv8_kernel.hip (sfa_decode_kv8: the whole history) and decode_kv8_window_kernel.hip (sfa_decode_kv8_window), as
// decode_mfma16.h is for the 16-bit pair.  It is what decode_mfma_common.h leaves to the fp8 kernels: the byte loads of
// a tile, their staging into the wave's LDS tiles, the software pipeline (kInFlight), the quantisation of the new token
// and its append (the e4m3 conversions themselves are kv8_convert.h, shared with the multi-token step over an fp8
// cache).  The design is described in decode_kv8_kernel.hip.
//
// WINDOW: the token sees the rows [lo, pos), lo = max(0, pos + 1 - window), instead of [0, pos), exactly as in
// decode_mfma16.h:
//   the wave slice covers [lo, pos) with boundaries at multiples of 32 rows from lo & ~31 (wave_slice), so with lo = 0
//   the partition, and with it every bit of the result, is that of the kernel without a window;
//   the first tile of the window may begin below lo: those keys get a score of -inf (Tiles::tile<true>), and because
//   0 x NaN in the P V product is NaN -- and 0x7F is a NaN byte -- their rows are re-addressed to row lo, their page index
//   to lo's page (Pages::set(t, lo, w1)): row = min(max(row, lo), w1 - 1), the mirror of the clamp past the wave's end.
// Without WINDOW `window` is not looked at and no lower bound is computed anywhere.
//
// SINK (decode_kv8_window_sinks_kernel.hip): sinks[h] is one more logit of query head h's softmax, with a zero value row,
// exactly as in decode_mfma16.h: Tiles::merge_store folds it in once, after the merge of the waves, in split 0.  k_scale
// is in sl2, so the merged maximum is in the true log2 units the sink lives in and the sink is not scaled; v_scale
// multiplies the accumulator alone, to which the sink adds 0.  Without SINK `sinks` is not looked at.
#pragma once
#include "decode_mfma_common.h"
#include "kv8_convert.h"

namespace sfa {
namespace decode {

constexpr int kInFlight = 2;                    // tiles a wave keeps in flight in registers (3 measured no better, and
                                                // 20-30 % slower through a paged cache: DESIGN.md 5.8)

template <class Tr, int D, bool NT, bool PAGED, bool WINDOW, bool SINK = false>
__device__ __forceinline__ void kv8_decode(const Kv8KernelParams &kp, const int window, const float *sinks = nullptr) {
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
    // the first row the token sees (0 <= pos < M and window >= 1: no overflow, lo <= pos)
    const int lo = WINDOW ? __builtin_amdgcn_readfirstlane(max(0, pos - (window - 1))) : 0;
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

    int w0, w1;                                 // WINDOW: w0 < w1 implies lo < w1; only the window's first tile has w0 < lo
    if constexpr (WINDOW) wave_slice(lo, pos, S, split, wave, w0, w1);
    else wave_slice(pos, S, split, wave, w0, w1);
    Pages<PAGED> pg(p, b);                      // (strides and offsets are in elements = bytes)
    uint8_t *const kc = reinterpret_cast<uint8_t *>(p.k_cache) + head_base<D, PAGED>(p, b, hk);
    uint8_t *const vc = reinterpret_cast<uint8_t *>(p.v_cache) + head_base<D, PAGED>(p, b, hk);

    // a tile of both caches as it lies in memory: load i covers the rows RP8 i + grp8, this lane's 16 bytes of each
    struct Raw { uint4 k[NL8], v[NL8]; };
    auto load = [&](Raw &x, int t) {
        if constexpr (WINDOW) pg.set(t, lo, w1);
        else pg.set(t, w1);
#pragma unroll
        for (int i = 0; i < NL8; ++i) {
            // never past the wave's end and, WINDOW, never below lo
            const int r = t + RP8 * i + grp8;
            const int row = min(WINDOW ? max(r, lo) : r, w1 - 1);
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
                    if constexpr (WINDOW) st.template tile<true>(kf, vbuf, w1 - tj, sl2, lo - tj);
                    else st.tile(kf, vbuf, w1 - tj, sl2);
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

    // v_scale: once, on the fp32 accumulator (SINK: after the fold, whose accumulator is 0)
    st.template merge_store<SINK>(p, smem, b, hk, split, G, PAGED && pg.bad, vsc, sinks);
}

}  // namespace decode
}  // namespace sfa
