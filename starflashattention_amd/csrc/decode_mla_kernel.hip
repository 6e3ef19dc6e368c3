// sfa_decode_mla: multi-head latent attention (MLA) decode in absorbed form, on the matrix cores.
// One cache row of 576 16-bit elements (a 512-wide latent and a 64-wide RoPE key) serves every query head: it is the key
// over all 576 columns and the value over its first 512.  The kernel is built around that double use:
//   grid   one workgroup of four waves per (head block of up to 64 heads, split, sequence);
//   tile   32 cache rows x 576 elements, loaded ONCE per workgroup by all 256 threads (9 x 16 B each, paged rows
//          resolved per 16-row half by Pages<>), parked row-major in LDS with a row stride of 1248 B, double-buffered:
//          the loads of tile i+1 are in flight in registers while tile i is computed, one barrier per tile;
//   S^T    = C . Q^T: the tile is the A operand, read with ds_read_b128 (row 16 kt + c, bytes 64 ks + 16 g), 18 k-steps
//          of v_mfma_f32_16x16x32 per 16 keys; Q^T of the wave's 16 heads stays in registers (18 x 4 VGPRs), loaded
//          from global memory directly in operand layout (lane (c, g) owns 8 consecutive dims, so the RoPE pairs of the
//          last 64 dims are rotated in the lane);
//   O^T    += V^T . P^T: the SAME LDS tile, columns 0..511, read through ds_read_b64_tr_b16; P^T is the exponentiated
//          S^T accumulator, packed to 16 bits -- no data movement, as in decode_mfma_common.h;
//   waves  with NHB = 1, 2 or 4 sixteen-head blocks in the workgroup, wave w owns head block w % NHB and the output dims
//          [512 NHB / 4 * (w / NHB), +512 NHB / 4): 8 NHB d-tiles, 32 NHB accumulator registers.  The waves that share a
//          head block compute its scores redundantly (36 MFMAs a tile), so every wave owns its outputs outright: there
//          is no cross-wave reduction, neither per tile nor at the end;
//   new    token: attended from the call's inputs (18 MFMAs for the score, a VALU axpy for the value) by the last split;
//          the workgroup of head block 0 of that split stores the row.
// The row stride 1248 = 1152 + 96 is 224 mod 256 bytes: the 16 lanes of a transposed read (4 rows x 32 B) and the next
// lane group (4 rows further = 128 B mod 256) fall on distinct banks.
// Partials of a split are un-normalised fp32; mla_combine_kernel merges them (skipped at one split).
#include "decode_mla_common.h"

namespace sfa {

namespace {

using namespace mla;

template <class Tr, int NHB, bool PAGED>
__global__ void __launch_bounds__(kDecodeWaves * 64)
mla_attn_kernel(const MlaKernelParams mp) {
    using Vec = typename Tr::mfma_vec;
    constexpr int NDT = 8 * NHB;                // 16-wide d tiles of O^T this wave owns
    constexpr int NKS = kMlaNks;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const DecodeKernelParams &p = mp.d;

    const int hblk = blockIdx.x, split = blockIdx.y, b = blockIdx.z;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int c = lane & 15, g = lane >> 4;     // MFMA lane coordinates
    const int S = p.num_splits, H = p.H;

    const int pos = p.seq_len[b];
    // sfa_decode's rejection contract: poison this block's output rows, raise the status bit, touch nothing else
    if (const int reject = reject_code<PAGED>(p, b, pos)) {
        if (split == 0) {
            const int h0 = hblk * 64, nh = min(64, H - h0);
            const uint32_t nan2 = Tr::id == 0 ? 0x7e007e00u : 0x7fc07fc0u;
            uint16_t *const ob = p.o + ((long long)b * H + h0) * kMlaDv;
            for (int i = tid; i < nh * (kMlaDv / 8); i += kDecodeWaves * 64)
                *reinterpret_cast<uint4 *>(ob + 8 * i) = make_uint4(nan2, nan2, nan2, nan2);
            if (tid == 0 && hblk == 0) atomicOr(p.status, reject);
        }
        return;
    }

    const int hb = wave % NHB, dpart = wave / NHB;
    const int head0 = hblk * 64 + hb * 16;      // this wave's 16 query heads (num_heads % 16 == 0: all real or none)
    const bool heads = head0 < H;
    const int dbase = dpart * NDT * 16;         // its first output dim
    const bool last = split == S - 1;           // the split that attends the new token

    // ---- prologue: Q^T fragments (B operand): lane holds Q[head0 + c][32 ks + 8 g .. +8], the rope part rotated ----
    Vec qf[NKS];
    {
        const uint16_t *const qrow = p.qkv + (long long)b * p.qkv_stride + (long long)(head0 + c) * kMlaD + 8 * g;
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) {
            uint4 v = make_uint4(0, 0, 0, 0);
            if (heads) {
                v = *reinterpret_cast<const uint4 *>(qrow + 32 * ks);
                if (32 * ks >= kMlaDv) v = mla_rope8<Tr>(v, (32 * ks - kMlaDv) / 2 + 4 * g, pos, p);
            }
            qf[ks] = bitcast<Vec>(v);
        }
    }

    f32x4 o[NDT];
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
        for (int r = 0; r < 4; ++r) o[dt][r] = 0.f;
    float m = neg_inf(), l = 0.f;               // query c's running max (log2 units) and this lane's share of its sum
    const float scale = p.scale_log2;

    // ---- this split's rows [r0, r1) of the cached rows [0, pos): whole tiles ----
    int rps = (pos + S - 1) / S;
    rps = (rps + kTile - 1) / kTile * kTile;    // paged: the 16-row halves of a tile each lie in one page
    const int r0 = min(pos, split * rps), r1 = min(pos, r0 + rps);
    const int ntiles = (r1 - r0 + kTile - 1) / kTile;

    Pages<PAGED> pg(p, b);
    uint16_t *const kc = p.k_cache + head_base<kMlaD, PAGED>(p, b, 0);

    // chunk j = tid + 256 i of a tile: row j / 72, 16 bytes at 16 (j % 72).  Rows past the split's end are re-addressed
    // to its last row (their scores are masked; the value product needs finite bits)
    auto load_tile = [&](uint4 (&st)[kMlaLoads], int t) {
        pg.set(t, r1);
#pragma unroll
        for (int i = 0; i < kMlaLoads; ++i) {
            const int j = tid + kDecodeWaves * 64 * i, row = j / kMlaChunks, ch = j - row * kMlaChunks;
            const int rr = min(t + row, r1 - 1);
            // (Pages::row_off with the half chosen by a select: indexing po[] by a lane's value would put it in scratch)
            const long long off = PAGED ? (row < 16 ? pg.po[0] : pg.po[1]) + (long long)(rr & pg.pmask) * pg.rs
                                        : (long long)rr * pg.rs;
            st[i] = ld16<false>(kc + off + 8 * ch);
        }
    };
    auto store_tile = [&](const uint4 (&st)[kMlaLoads], char *buf) {
#pragma unroll
        for (int i = 0; i < kMlaLoads; ++i) {
            const int j = tid + kDecodeWaves * 64 * i, row = j / kMlaChunks, ch = j - row * kMlaChunks;
            *reinterpret_cast<uint4 *>(buf + kMlaRow * row + 16 * ch) = st[i];
        }
    };

    // one 32-key tile at buf, the first nvalid keys real
    auto tile = [&](const char *buf, int nvalid) {
        f32x4 s[2];
        const char *kr = buf + kMlaRow * c + 16 * g;
#pragma unroll
        for (int kt = 0; kt < 2; ++kt) {
#pragma unroll
            for (int r = 0; r < 4; ++r) s[kt][r] = 0.f;
#pragma unroll
            for (int ks = 0; ks < NKS; ++ks) {
                const uint4 a = *reinterpret_cast<const uint4 *>(kr + kMlaRow * 16 * kt + 64 * ks);
                s[kt] = Mfma16<Tr>::run(bitcast<Vec>(a), qf[ks], s[kt]);
            }
        }
        float mx = neg_inf();
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {       // element r of accumulator kt = key 16 kt + 4 g + r
                s[kt][r] = (16 * kt + 4 * g + r < nvalid) ? s[kt][r] * scale : neg_inf();
                mx = fmaxf(mx, s[kt][r]);
            }
        mx = fmaxf(m, quad_max(mx));            // finite: key 0 of a tile is always real
        const float alpha = fast_exp2(m - mx);
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
            const float p0 = fast_exp2(s[kt][0] - mx), p1 = fast_exp2(s[kt][1] - mx);
            const float p2 = fast_exp2(s[kt][2] - mx), p3 = fast_exp2(s[kt][3] - mx);
            ps[kt] = (p0 + p1) + (p2 + p3);
            pb[2 * kt] = Tr::pack2(p0, p1);
            pb[2 * kt + 1] = Tr::pack2(p2, p3);
        }
        l = __builtin_fmaf(l, alpha, ps[0]) + ps[1];
        const Vec pv = bitcast<Vec>(make_uint4(pb[0], pb[1], pb[2], pb[3]));
        // V^T fragments: lane (c, g) reads rows 4 g + (c >> 2) and 16 + ..., 8 bytes at column dbase + 16 dt + 4 (c & 3)
        const char *vr = buf + kMlaRow * (4 * g + (c >> 2)) + 8 * (c & 3) + 2 * dbase;
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt) {
            const auto t0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_i16x4 *)(vr + 32 * dt));
            const auto t1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_i16x4 *)(vr + kMlaRow * 16 + 32 * dt));
            const u32x2 a_lo = bitcast<u32x2>(t0), a_hi = bitcast<u32x2>(t1);
            u32x4 av;
            av[0] = a_lo[0]; av[1] = a_lo[1]; av[2] = a_hi[0]; av[3] = a_hi[1];
            o[dt] = Mfma16<Tr>::run(bitcast<Vec>(av), pv, o[dt]);
        }
    };

    if (ntiles > 0) {
        uint4 st[kMlaLoads];
        load_tile(st, r0);
        store_tile(st, smem);
        __syncthreads();
        for (int i = 0; i < ntiles; ++i) {
            const int t = r0 + kTile * i;
            const bool more = i + 1 < ntiles;
            if (more) load_tile(st, t + kTile);         // in flight while tile i is computed
            tile(smem + (i & 1) * kMlaTile, r1 - t);
            // the other buffer was last read for tile i - 1, before the barrier that ended that iteration
            if (more) store_tile(st, smem + ((i + 1) & 1) * kMlaTile);
            __syncthreads();
        }
    }

    // ---- the new token (position pos), from the call's inputs ----
    const uint16_t *const kvn = mp.kv_new + (long long)b * mp.kv_new_stride;
    if (last) {
        // every row of the A operand is the new key: each accumulator element is q_c . k_new
        f32x4 s0 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) {
            uint4 a = *reinterpret_cast<const uint4 *>(kvn + 32 * ks + 8 * g);
            if (32 * ks >= kMlaDv) a = mla_rope8<Tr>(a, (32 * ks - kMlaDv) / 2 + 4 * g, pos, p);
            s0 = Mfma16<Tr>::run(bitcast<Vec>(a), qf[ks], s0);
        }
        const float sc = s0[0] * scale;
        const float mx = fmaxf(m, sc);
        const float alpha = fast_exp2(m - mx), pn = fast_exp2(sc - mx);
        m = mx;
        l = __builtin_fmaf(l, alpha, g == 0 ? pn : 0.f);       // the four lanes of a query share its sum
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt) {      // the latent is the value as it is: dims dbase + 16 dt + 4 g + r
            const uint2 v = *reinterpret_cast<const uint2 *>(kvn + dbase + 16 * dt + 4 * g);
            o[dt][0] = __builtin_fmaf(o[dt][0], alpha, pn * Tr::lo_f32(v.x));
            o[dt][1] = __builtin_fmaf(o[dt][1], alpha, pn * Tr::hi_f32(v.x));
            o[dt][2] = __builtin_fmaf(o[dt][2], alpha, pn * Tr::lo_f32(v.y));
            o[dt][3] = __builtin_fmaf(o[dt][3], alpha, pn * Tr::hi_f32(v.y));
        }
        if (hblk == 0 && tid < kMlaChunks) {    // append: exactly one workgroup per sequence, 72 lanes x 16 B
            uint4 v = *reinterpret_cast<const uint4 *>(kvn + 8 * tid);
            if (8 * tid >= kMlaDv) v = mla_rope8<Tr>(v, (8 * tid - kMlaDv) / 2, pos, p);
            *reinterpret_cast<uint4 *>(kc + pg.append_off(pos) + 8 * tid) = v;
        }
    }

    // ---- epilogue: the wave owns head block hb x dims [dbase, dbase + 16 NDT) ----
    float ltot = quad_sum(l);
    if (PAGED && pg.bad) ltot = __builtin_nanf("");     // a read page outside the pool
    if (!heads) return;
    const long long bh = (long long)b * H + head0 + c;
    if (S == 1) {
        const float inv = 1.0f / ltot;          // l >= 1: the new token is always present
        uint16_t *const orow = p.o + bh * kMlaDv + dbase + 4 * g;
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt)
            *reinterpret_cast<uint2 *>(orow + 16 * dt) =
                make_uint2(Tr::pack2(o[dt][0] * inv, o[dt][1] * inv), Tr::pack2(o[dt][2] * inv, o[dt][3] * inv));
    } else {
        float *const prow = p.part_o + (bh * S + split) * kMlaDv + dbase + 4 * g;
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt)
            *reinterpret_cast<float4 *>(prow + 16 * dt) = make_float4(o[dt][0], o[dt][1], o[dt][2], o[dt][3]);
        if (dpart == 0 && g == 0) p.part_ml[bh * S + split] = make_float2(m, ltot);
    }
}

// o[b, h, 0:512] = the merge of the splits' partials (mla_combine_row), 64 lanes a row
template <class Tr>
__global__ void __launch_bounds__(256)
mla_combine_kernel(const MlaKernelParams mp) {
    const DecodeKernelParams &p = mp.d;
    constexpr int LPR = kMlaDv / 8;
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long bh = gid / LPR;
    const int sub = (int)(gid % LPR);
    if (bh >= (long long)p.B * p.H) return;
    const int b = (int)(bh / p.H);
    const int pos = p.seq_len[b];
    if (p.block_table ? reject_code<true>(p, b, pos) : reject_code<false>(p, b, pos)) return;   // o[b] is already poisoned
    mla_combine_row<Tr>(p, bh, sub, p.o + bh * kMlaDv);
}

template <class Tr, int NHB, bool PAGED>
int mla_launch_k(const MlaKernelParams &mp, hipStream_t stream) {
    const DecodeKernelParams &p = mp.d;
    dim3 grid((p.H + 63) / 64, p.num_splits, p.B), block(kDecodeWaves * 64);
    static DynLdsAttr attr;
    if (const int rc = attr.ensure(reinterpret_cast<const void *>(&mla_attn_kernel<Tr, NHB, PAGED>), kMlaLds,
                                   "mla_attn_kernel"))
        return rc;
    hipLaunchKernelGGL((mla_attn_kernel<Tr, NHB, PAGED>), grid, block, kMlaLds, stream, mp);
    return check_launch("mla_attn_kernel");
}

template <class Tr>
int mla_launch_t(const MlaKernelParams &mp, hipStream_t stream) {
    const DecodeKernelParams &p = mp.d;
    const bool paged = p.block_table != nullptr;
    int rc;
    // 16 heads: every wave a quarter of the output dims; 32: a half; more: head blocks of up to 64, a wave each per
    // sixteen heads (a block of 48, or the 16 / 32 / 48 heads left after a full block, leaves waves without heads)
    if (p.H == 16) rc = paged ? mla_launch_k<Tr, 1, true>(mp, stream) : mla_launch_k<Tr, 1, false>(mp, stream);
    else if (p.H == 32) rc = paged ? mla_launch_k<Tr, 2, true>(mp, stream) : mla_launch_k<Tr, 2, false>(mp, stream);
    else rc = paged ? mla_launch_k<Tr, 4, true>(mp, stream) : mla_launch_k<Tr, 4, false>(mp, stream);
    if (rc || p.num_splits == 1) return rc;
    const long long threads = (long long)p.B * p.H * (kMlaDv / 8);
    hipLaunchKernelGGL((mla_combine_kernel<Tr>), dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, stream, mp);
    return check_launch("mla_combine_kernel");
}

}  // namespace

// validated dtype, num_heads in {16, 32, ..., 128}: the attention kernel, then (two or more splits) the combine
int launch_mla_decode(const MlaKernelParams &p, int dtype, hipStream_t stream) {
    return dtype == SFA_DTYPE_FP16 ? mla_launch_t<Fp16>(p, stream) : mla_launch_t<Bf16>(p, stream);
}

}  // namespace sfa
