// The body of the matrix-core decode kernels over 16-bit caches, from the rejection to the merge of the waves: ONE copy
// for decode_gqa_mfma_kernel.hip (sfa_decode: the whole history, G a template constant of the kernel) and
// decode_window_kernel.hip (sfa_decode_window: G = H / Hkv).  It is what decode_mfma_common.h leaves to a kernel file:
// the cache loads (operand-layout or row-major through the K tile), the two-tile software pipeline, the fill of the new
// token's V tile and the append.  The design is described in decode_gqa_mfma_kernel.hip.
//
// WINDOW: the token sees the rows [lo, pos), lo = max(0, pos + 1 - window), instead of [0, pos):
//   the wave slice covers [lo, pos): its boundaries are multiples of 32 rows from lo & ~31 (wave_slice), so with lo = 0
//   the partition, and with it every bit of the result, is that of the kernel without a window;
//   the first tile of the window may begin below lo: those keys get a score of -inf (Tiles::tile<true>), and because
//   0 x NaN in the P V product is NaN their rows are re-addressed to row lo, their page index to lo's page
//   (Pages::set(t, lo, w1)): row = min(max(row, lo), w1 - 1), the mirror of the clamp past the wave's end.
// Without WINDOW `window` is not looked at and no lower bound is computed anywhere: lo is the literal 0 of an untaken
// branch, not a value the compiler would have to prove non-negative things about.
//
// SINK (decode_window_sinks_kernel.hip): sinks[h] is one more logit of query head h's softmax, with a zero value row.  It
// takes no part in the tiles: Tiles::merge_store folds it in once, after the merge of the waves, in split 0.  Without
// SINK `sinks` is not looked at.
#pragma once
#include "decode_mfma_common.h"

namespace sfa {
namespace decode {

template <class Tr, int D, bool NT, bool KLDS, bool PAGED, bool WINDOW, bool SINK = false>
__device__ __forceinline__ void mfma16_decode(const DecodeKernelParams &p, const int G, const int window,
                                              const float *sinks = nullptr) {
    using Lds = MfmaLds<D>;
    constexpr int LPR = D / 8;                  // lanes (16-byte chunks) per cache row
    constexpr int RPL = 64 / LPR;               // rows one load instruction of a wave covers
    constexpr int NLD = kTile / RPL;            // row-major loads per 32-row tile (= 2 NKS)
    constexpr int NKS = D / 32;                 // k-steps of a QK^T accumulator
    constexpr int VS = Lds::VS, KS = Lds::KS;
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int hk = blockIdx.x, split = blockIdx.y, b = blockIdx.z;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int c = lane & 15, g = lane >> 4;     // MFMA lane coordinates
    const int sub = lane % LPR, grp = lane / LPR;   // row-major coordinates: which 8 dims, which row of a load
    const int S = p.num_splits;

    const int pos = p.seq_len[b];
    if (rejected<Tr, D, PAGED>(p, b, hk, split, G, pos)) return;
    // the first row the token sees (0 <= pos < M and window >= 1: no overflow, lo <= pos)
    const int lo = WINDOW ? __builtin_amdgcn_readfirstlane(max(0, pos - (window - 1))) : 0;

    // wave-private LDS: a V tile (also the Q / k_new re-layout area) and a K tile (KLDS)
    char *const vbuf = smem + wave * Lds::WAVE_LDS;
    char *const kbuf = vbuf + Lds::VTILE;

    uint4 kpk, vpk;                             // the new token's K / V: attended to and appended as they are
    rotate_new_token<Tr, D>(p, b, hk, G, pos, reinterpret_cast<uint16_t *>(vbuf), kpk, vpk);
    Tiles<Tr, D> st;
    st.init(reinterpret_cast<uint16_t *>(vbuf), kpk);

    int w0, w1;                                 // WINDOW: w0 < w1 implies lo < w1; only the window's first tile has w0 < lo
    if constexpr (WINDOW) wave_slice(lo, pos, S, split, wave, w0, w1);
    else wave_slice(pos, S, split, wave, w0, w1);
    Pages<PAGED> pg(p, b);                      // paged: always with KLDS
    const long long rs = pg.rs;
    uint16_t *const kc = p.k_cache + head_base<D, PAGED>(p, b, hk);
    uint16_t *const vc = p.v_cache + head_base<D, PAGED>(p, b, hk);
    const uint16_t *const kb = kc + 8 * g;      // + row * rs + 32 ks: operand layout
    const uint16_t *const vb = vc + 8 * sub;    // + row * rs: row-major chunks

    // a row of the tile at t as it is addressed: never past the wave's end and, WINDOW, never below lo
    auto clamp = [&](int row) { return min(WINDOW ? max(row, lo) : row, w1 - 1); };
    auto load_k = [&](uint4 (&kk)[2][NKS], int t) {
        if constexpr (WINDOW) pg.set(t, lo, w1);        // load_v(.., t) follows and uses the same pages
        else pg.set(t, w1);
#pragma unroll
        for (int kt = 0; kt < 2; ++kt) {
            const int row = clamp(t + 16 * kt + c);
#pragma unroll
            for (int ks = 0; ks < NKS; ++ks) {
                if (KLDS) {     // row-major like V: load j = kt NKS + ks covers rows RPL j + grp, chunk sub
                    const int r2 = clamp(t + RPL * (kt * NKS + ks) + grp);
                    kk[kt][ks] = ld16<NT>(kc + pg.row_off(r2, kt) + 8 * sub);
                } else {        // directly in operand layout: 64-B pieces of 16 rows
                    kk[kt][ks] = ld16<NT>(kb + (long long)row * rs + 32 * ks);
                }
            }
        }
    };
    auto load_v = [&](uint4 (&vv)[NLD], int t) {        // lane: rows grp + RPL i, chunk sub
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            const int row = clamp(t + grp + RPL * i);
            vv[i] = ld16<NT>(vb + pg.row_off(row, (RPL * i) >> 4));
        }
    };
    auto store_v = [&](const uint4 (&vv)[NLD]) {
#pragma unroll
        for (int i = 0; i < NLD; ++i)
            *reinterpret_cast<uint4 *>(vbuf + VS * (grp + RPL * i) + 16 * sub) = vv[i];
    };
    // KLDS: the K tile came in row-major; lay it out as MFMA operands through the wave's LDS K tile
    auto to_operand = [&](uint4 (&kk)[2][NKS]) {
        if (!KLDS) return;
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
            for (int ks = 0; ks < NKS; ++ks)
                *reinterpret_cast<uint4 *>(kbuf + KS * (RPL * (kt * NKS + ks) + grp) + 16 * sub) = kk[kt][ks];
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
            for (int ks = 0; ks < NKS; ++ks)
                kk[kt][ks] = *reinterpret_cast<const uint4 *>(kbuf + KS * (16 * kt + c) + 64 * ks + 16 * g);
    };

    if (w0 < w1) {
        // tile t+1 is in flight into registers while tile t is computed; the LDS tiles are single: a wave's
        // LDS operations execute in order, so storing tile t+1 cannot overtake the reads of tile t
        uint4 ka[2][NKS], kb2[2][NKS], vr[NLD];
        load_k(ka, w0);
        load_v(vr, w0);
        for (int t = w0; t < w1; t += 2 * kTile) {
            store_v(vr);
            to_operand(ka);
            const bool more1 = t + kTile < w1;
            if (more1) { load_k(kb2, t + kTile); load_v(vr, t + kTile); }
            st.template tile<WINDOW>(ka, vbuf, w1 - t, p.scale_log2, lo - t);
            if (more1) {
                store_v(vr);
                to_operand(kb2);
                if (t + 2 * kTile < w1) { load_k(ka, t + 2 * kTile); load_v(vr, t + 2 * kTile); }
                st.template tile<WINDOW>(kb2, vbuf, w1 - t - kTile, p.scale_log2, lo - t - kTile);
            }
        }
    }

    // ---- the new token (position `pos`): last split, wave 0 ----
    if (split == S - 1 && wave == 0) {
        // every row of the V tile = v_new (Tiles::new_token_tile); stored as ONE vector value: as four words the
        // stores can come out as 12 + 4 bytes
        const u32x4 v = {vpk.x, vpk.y, vpk.z, vpk.w};
#pragma unroll
        for (int i = 0; i < NLD; ++i) *reinterpret_cast<u32x4 *>(vbuf + VS * (grp + RPL * i) + 16 * sub) = v;
        st.new_token_tile(vbuf, p.scale_log2);
        if (grp == 0) {                         // append: LPR lanes x 16 B = one row each
            const long long roff = pg.append_off(pos) + sub * 8;
            *reinterpret_cast<uint4 *>(kc + roff) = kpk;
            *reinterpret_cast<uint4 *>(vc + roff) = vpk;
        }
    }

    st.template merge_store<SINK>(p, smem, b, hk, split, G, PAGED && pg.bad, 1.0f, sinks);
}

}  // namespace decode
}  // namespace sfa
