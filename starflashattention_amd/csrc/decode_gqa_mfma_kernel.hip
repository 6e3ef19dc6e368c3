// Grouped-query decode on the matrix cores, for groups too large for the VALU kernel
// (decode_gqa_kernel.hip is VALU-bound from 8 query heads per kv head on: 4.1 of 6.5 TB/s).
// One workgroup per (batch, kv head, split), four waves, each wave walks its share of the cached rows
// in 32-key tiles on v_mfma_f32_16x16x32 (16 query columns of which G are real):
//   S^T[key][q] = K . Q^T     A = K rows: head-major caches are read from HBM DIRECTLY in operand layout
//                                 (lane (c = l & 15, g = l >> 4) loads K[t + 16kt + c][32ks + 8g .. +8]);
//                                 the reference layout is read row-major and re-laid out through a
//                                 wave-private LDS tile (64-B pieces of strided rows cost 8 %);
//                             B = Q^T held in registers for the whole kernel (re-laid out once through LDS);
//   O^T[d][q] += V^T . P^T    P^T = the exponentiated S^T accumulators, packed (no data movement);
//                             V^T through a wave-private LDS tile: row-major ds_write_b128 in, ds_read_b64_tr_b16
//                             out (no barrier: a wave's LDS operations execute in order).
// The query sits on the lane in both accumulators: one online-softmax state per lane, row max across the
// four 16-lane groups by v_permlane32_swap + v_permlane16_swap.  Scores are scaled in fp32 (exact).
// The new token is one more tile of one valid key whose K/V come from the prologue's registers.
// Per 32 keys a wave issues 16 MFMAs and ~60 VALU instructions for 16 KB of cache: HBM-bound for any G <= 16.
// The body that does not depend on the cache's element type (rejection, prologue, wave slice, paging, the tile math,
// the merge of the waves) is in decode_mfma_common.h and shared with decode_kv8_kernel.hip; this file keeps the cache
// loads (operand-layout or row-major through the K tile), the two-tile software pipeline and the append.
#include <cstdlib>

#include "decode_mfma_common.h"

namespace sfa {

namespace {

using namespace decode;

template <class Tr, int D, int G, bool NT, bool KLDS, bool PAGED = false>
__global__ void __launch_bounds__(kDecodeWaves * 64)
decode_gqa_mfma_kernel(const DecodeKernelParams p) {
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

    // wave-private LDS: a V tile (also the Q / k_new re-layout area) and a K tile (KLDS)
    char *const vbuf = smem + wave * Lds::WAVE_LDS;
    char *const kbuf = vbuf + Lds::VTILE;

    uint4 kpk, vpk;                             // the new token's K / V: attended to and appended as they are
    rotate_new_token<Tr, D>(p, b, hk, G, pos, reinterpret_cast<uint16_t *>(vbuf), kpk, vpk);
    Tiles<Tr, D> st;
    st.init(reinterpret_cast<uint16_t *>(vbuf), kpk);

    int w0, w1;
    wave_slice(pos, S, split, wave, w0, w1);
    Pages<PAGED> pg(p, b);                      // paged: always with KLDS
    const long long rs = pg.rs;
    uint16_t *const kc = p.k_cache + head_base<D, PAGED>(p, b, hk);
    uint16_t *const vc = p.v_cache + head_base<D, PAGED>(p, b, hk);
    const uint16_t *const kb = kc + 8 * g;      // + row * rs + 32 ks: operand layout
    const uint16_t *const vb = vc + 8 * sub;    // + row * rs: row-major chunks

    auto load_k = [&](uint4 (&kk)[2][NKS], int t) {
        pg.set(t, w1);                          // load_v(.., t) follows and uses the same pages
#pragma unroll
        for (int kt = 0; kt < 2; ++kt) {
            const int row = min(t + 16 * kt + c, w1 - 1);
#pragma unroll
            for (int ks = 0; ks < NKS; ++ks) {
                if (KLDS) {     // row-major like V: load j = kt NKS + ks covers rows RPL j + grp, chunk sub
                    const int r2 = min(t + RPL * (kt * NKS + ks) + grp, w1 - 1);
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
            const int row = min(t + grp + RPL * i, w1 - 1);
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
            st.tile(ka, vbuf, w1 - t, p.scale_log2);
            if (more1) {
                store_v(vr);
                to_operand(kb2);
                if (t + 2 * kTile < w1) { load_k(ka, t + 2 * kTile); load_v(vr, t + 2 * kTile); }
                st.tile(kb2, vbuf, w1 - t - kTile, p.scale_log2);
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

    st.merge_store(p, smem, b, hk, split, G, PAGED && pg.bad, 1.0f);
}

template <class Tr, int D, int G, bool NT, bool KLDS, bool PAGED = false>
int launch_k(const DecodeKernelParams &p, hipStream_t stream) {
    dim3 grid(p.Hkv, p.num_splits, p.B), block(kDecodeWaves * 64);
    constexpr int lds = MfmaLds<D>::BYTES;
    static DynLdsAttr attr;
    if (const int rc = attr.ensure(reinterpret_cast<const void *>(&decode_gqa_mfma_kernel<Tr, D, G, NT, KLDS, PAGED>), lds,
                                   "decode_gqa_mfma_kernel"))
        return rc;
    hipLaunchKernelGGL((decode_gqa_mfma_kernel<Tr, D, G, NT, KLDS, PAGED>), grid, block, lds, stream, p);
    return check_launch("decode_gqa_mfma_kernel");
}

template <class Tr, int D, int G>
int launch_g(const DecodeKernelParams &p, bool nt, hipStream_t stream) {
    // Reference layout: a K row of this head is a 256-B segment H*D*2 bytes from the next, and fetching it
    // as 64-B operand pieces costs 8 % (5.96 vs 6.44 TB/s): load row-major, re-lay out through LDS.
    // Head-major caches are contiguous, the operand-layout loads go straight to registers (6.7 TB/s).
    if (p.block_table)
        return nt ? launch_k<Tr, D, G, true, true, true>(p, stream) : launch_k<Tr, D, G, false, true, true>(p, stream);
    const bool klds = p.kv_row_stride != D;
    if (klds) return nt ? launch_k<Tr, D, G, true, true>(p, stream) : launch_k<Tr, D, G, false, true>(p, stream);
    return nt ? launch_k<Tr, D, G, true, false>(p, stream) : launch_k<Tr, D, G, false, false>(p, stream);
}

template <class Tr, int D>
int launch_d(const DecodeKernelParams &p, bool nt, hipStream_t stream) {
    if (p.H == 16 * p.Hkv) return launch_g<Tr, D, 16>(p, nt, stream);
    if (p.H == 4 * p.Hkv) return launch_g<Tr, D, 4>(p, nt, stream);
    return launch_g<Tr, D, 8>(p, nt, stream);
}

}  // namespace

// head_dim 64 / 128 / 256, any cache layout, 4, 8 or 16 query heads per kv head
int launch_decode_gqa_mfma(const DecodeKernelParams &p, int dtype, int head_dim, bool nt, hipStream_t stream) {
    const bool h = dtype == SFA_DTYPE_FP16;
    if (head_dim == 64) return h ? launch_d<Fp16, 64>(p, nt, stream) : launch_d<Bf16, 64>(p, nt, stream);
    if (head_dim == 256) return h ? launch_d<Fp16, 256>(p, nt, stream) : launch_d<Bf16, 256>(p, nt, stream);
    return h ? launch_d<Fp16, 128>(p, nt, stream) : launch_d<Bf16, 128>(p, nt, stream);
}

}  // namespace sfa
