// What the latent-attention decode kernels share (decode_mla_kernel.hip: one new token per sequence;
// decode_mla_chunk_kernel.hip: up to 32): the geometry of a cache row and of its LDS tile, the rotation of 8 rope
// elements, and the merge of the splits' partials.  The tile design is described in decode_mla_kernel.hip.
#pragma once
#include "decode_mfma_common.h"

namespace sfa {
namespace mla {

using namespace decode;

constexpr int kMlaD = 576;                      // elements of a cache row: the key
constexpr int kMlaDv = 512;                     // its first columns: the value
constexpr int kMlaNks = kMlaD / 32;             // k-steps of a score accumulator
constexpr int kMlaChunks = kMlaD / 8;           // 16-byte chunks per row
constexpr int kMlaLoads = kTile * kMlaChunks / (kDecodeWaves * 64);     // chunks per thread per tile
constexpr int kMlaRow = 2 * kMlaD + 96;         // LDS row stride, bytes
constexpr int kMlaTile = kTile * kMlaRow;       // 39,936 B
constexpr int kMlaLds = 2 * kMlaTile;           // 79,872 B: two workgroups fit a CU where the registers allow
static_assert(kMlaLoads * kDecodeWaves * 64 == kTile * kMlaChunks, "a tile is a whole number of loads per thread");
static_assert(kMlaRow % 16 == 0 && kMlaRow % 256 == 224, "aligned b128 rows; conflict-free transposed reads");

// 8 consecutive elements of the rope part (pairs pj0 .. pj0 + 3) rotated to position pos: rotate_new_token's recipe
template <class Tr>
__device__ __forceinline__ uint4 mla_rope8(const uint4 raw, int pj0, int pos, const DecodeKernelParams &p) {
    float x[8];
    unpack8<Tr>(raw, x);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        float cs, sn;
        rope_cs<Tr>(pj0 + i, pos, p, cs, sn);
        const float a = x[2 * i], bb = x[2 * i + 1];
        x[2 * i] = a * cs - bb * sn;
        x[2 * i + 1] = bb * cs + a * sn;
    }
    return pack8<Tr>(x);
}

// orow[8 sub .. +8] = sum_s 2^(m_s - M) o_s / sum_s 2^(m_s - M) l_s over the S partials of row `row` of part_o / part_ml:
// decode_combine_kernel's merge for rows of 512 (that kernel is instantiated for the head dims of sfa_decode only)
template <class Tr>
__device__ __forceinline__ void mla_combine_row(const DecodeKernelParams &p, long long row, int sub, uint16_t *orow) {
    const int S = p.num_splits;
    Stream tot;
    tot.init();
    for (int s = 0; s < S; ++s) {
        const float2 ml = p.part_ml[row * S + s];
        const float *po = p.part_o + (row * S + s) * kMlaDv + sub * 8;
        const float4 a = *reinterpret_cast<const float4 *>(po);
        const float4 c = *reinterpret_cast<const float4 *>(po + 4);
        const float a2[8] = {a.x, a.y, a.z, a.w, c.x, c.y, c.z, c.w};
        tot.merge(ml.x, ml.y, a2);
    }
    const float inv = 1.0f / tot.l;
    float y[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) y[j] = tot.acc[j] * inv;
    *reinterpret_cast<uint4 *>(orow + sub * 8) = pack8<Tr>(y);
}

}  // namespace mla
}  // namespace sfa
