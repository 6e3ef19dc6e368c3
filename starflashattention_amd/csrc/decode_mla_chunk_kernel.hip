// sfa_decode_mla_chunk: n <= 32 new tokens per sequence of multi-head latent attention (absorbed form) in one pass over
// the cache.  The tile machinery is decode_mla_kernel.hip's -- a 32 x 576 tile loaded once per workgroup by all 256
// threads, row-major in LDS at a stride of 1248 B, double-buffered with the next tile in registers and one barrier per
// tile, S^T = C . Q^T through ds_read_b128, O^T += V^T . P^T through ds_read_b64_tr_b16 over the same tile,
// v_mfma_f32_16x16x32 -- and what differs is how the work is split and how the new tokens are attended:
//   rows   the cache row is the key and the value of EVERY query row, so n tokens x H heads are n H query rows over one
//          tile stream.  num_heads % 16 == 0: a block of 16 query rows is (one token t, 16 heads), row block
//          rb = t (H / 16) + hb, R = n H / 16 of them per sequence;
//   grid   one workgroup of four waves per (group of NHB row blocks, split, sequence): R = 1 -> NHB = 1, R = 2 -> NHB = 2,
//          otherwise NHB = 4 over ceil(R / 4) groups.  Wave w owns row block w % NHB of its group and the output dims
//          [512 NHB / 4 * (w / NHB), +512 NHB / 4).  At H = 16, n = 4 the four waves own four tokens and no score is
//          computed twice; at H = 128, n = 2 four workgroups per (split, sequence) share the tile through L2;
//   t      the token of a wave, its head base, the RoPE position pos + t of its Q and its rows of o and of the partials
//          are wave-uniform.  A wave without a row block (R = 3, or the last group of R = 9) loads its share of every
//          tile and computes nothing;
//   new    tokens are ONE MORE TILE: after the cache tiles every workgroup of the last split stages kv_new[b] into LDS
//          buffer 0 -- the rope columns rotated to pos + row, rows n .. 31 zero -- and each wave runs the ordinary tile
//          body on it with nvalid = t + 1.  That one wave-uniform number is the causality inside the chunk.  Key 0 of
//          the tile is always real, so pos = 0 and an empty last split need nothing special.  The workgroup of group 0
//          stores the n rows to the cache from the registers it staged them from: one workgroup per sequence, never
//          re-read, pages resolved per row.
// Splits are whole tiles of [0, pos); an empty split leaves (-inf, 0).  Partials and the combine are sfa_decode_mla's
// over the B n H rows.  Rejection is chunk::reject_code: the workgroups of split 0 poison their own rows of o[b].
#include "decode_chunk_common.h"
#include "decode_mla_common.h"

namespace sfa {

namespace {

using namespace mla;

template <class Tr, int NHB, bool PAGED>
__global__ void __launch_bounds__(kDecodeWaves * 64)
mla_chunk_attn_kernel(const MlaChunkKernelParams cp) {
    using Vec = typename Tr::mfma_vec;
    constexpr int NDT = 8 * NHB;                // 16-wide d tiles of O^T this wave owns
    constexpr int NKS = kMlaNks;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const DecodeKernelParams &p = cp.m.d;

    const int grp = blockIdx.x, split = blockIdx.y, b = blockIdx.z;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c = lane & 15, g = lane >> 4;     // MFMA lane coordinates
    const int S = p.num_splits, H = p.H, n = cp.n;

    // ---- this wave's row block: token t, heads head0 .. +16 ----
    const int hpt = H >> 4, R = n * hpt;        // row blocks per token, per sequence
    const int hb = wave % NHB, dpart = wave / NHB;
    const int rb = grp * NHB + hb;
    const bool active = rb < R;
    const int t = active ? rb / hpt : 0;
    const int head0 = active ? (rb - t * hpt) * 16 : 0;
    const int dbase = dpart * NDT * 16;         // its first output dim
    const bool last = split == S - 1;           // the split that attends the new tokens
    // o[b, t, head0 .. +16, :]: 16 contiguous rows
    uint16_t *const ob = p.o + ((long long)b * n + t) * cp.o_tok_stride + (long long)head0 * kMlaDv;

    const int pos = p.seq_len[b];
    // sfa_decode_chunk's rejection contract: poison this workgroup's output rows, raise the status bit, touch nothing else
    if (const int reject = chunk::reject_code<PAGED>(p, n, b, pos)) {
        if (split == 0) {
            if (active && dpart == 0) {
                const uint32_t nan2 = Tr::id == 0 ? 0x7e007e00u : 0x7fc07fc0u;
                for (int i = lane; i < 16 * (kMlaDv / 8); i += 64)
                    *reinterpret_cast<uint4 *>(ob + 8 * i) = make_uint4(nan2, nan2, nan2, nan2);
            }
            if (tid == 0 && grp == 0) atomicOr(p.status, reject);
        }
        return;
    }

    // ---- prologue: Q^T fragments (B operand): lane holds Q[t][head0 + c][32 ks + 8 g .. +8], the rope part rotated ----
    Vec qf[NKS];
    {
        const uint16_t *const qrow = p.qkv + (long long)b * p.qkv_stride + (long long)t * cp.q_tok_stride +
                                     (long long)(head0 + c) * kMlaD + 8 * g;
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) {
            uint4 v = make_uint4(0, 0, 0, 0);
            if (active) {
                v = *reinterpret_cast<const uint4 *>(qrow + 32 * ks);
                if (32 * ks >= kMlaDv) v = mla_rope8<Tr>(v, (32 * ks - kMlaDv) / 2 + 4 * g, pos + t, p);
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
    auto load_tile = [&](uint4 (&st)[kMlaLoads], int row0) {
        pg.set(row0, r1);
#pragma unroll
        for (int i = 0; i < kMlaLoads; ++i) {
            const int j = tid + kDecodeWaves * 64 * i, row = j / kMlaChunks, ch = j - row * kMlaChunks;
            const int rr = min(row0 + row, r1 - 1);
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
            const int row0 = r0 + kTile * i;
            const bool more = i + 1 < ntiles;
            if (more) load_tile(st, row0 + kTile);      // in flight while tile i is computed
            if (active) tile(smem + (i & 1) * kMlaTile, r1 - row0);
            // the other buffer was last read for tile i - 1, before the barrier that ended that iteration
            if (more) store_tile(st, smem + ((i + 1) & 1) * kMlaTile);
            __syncthreads();
        }
    }

    // ---- the new tokens (positions pos .. pos + n - 1), from the call's inputs, as the tile of the rows pos .. pos + 31.
    // Both LDS buffers are free after the loop's last barrier.  Latent chunks: 32 rows x 64 chunks = 8 per thread, row
    // wave + 4 i (wave-uniform), chunk = lane; rope chunks: 32 rows x 8 = one per thread, and with it one rotation ----
    if (last) {
        const uint16_t *const kvn = cp.m.kv_new + (long long)b * cp.m.kv_new_stride;
        const bool store = grp == 0;            // the append: exactly one workgroup per sequence
        // (reject_code has checked the table entries of the pages of [pos, pos + n))
        auto cache_row = [&](int r) {
            if (!PAGED) return kc + (long long)r * pg.rs;
            return kc + pg.tbl[r >> pg.page_shift] * pg.page_stride + (long long)(r & pg.pmask) * pg.rs;
        };
#pragma unroll
        for (int i = 0; i < kTile / kDecodeWaves; ++i) {
            const int row = wave + kDecodeWaves * i;
            uint4 v = make_uint4(0, 0, 0, 0);   // rows n .. 31: zeros (masked scores; the value product needs finite bits)
            if (row < n) {
                v = *reinterpret_cast<const uint4 *>(kvn + (long long)row * cp.kv_tok_stride + 8 * lane);
                if (store) *reinterpret_cast<uint4 *>(cache_row(pos + row) + 8 * lane) = v;     // the latent, bit-exact
            }
            *reinterpret_cast<uint4 *>(smem + kMlaRow * row + 16 * lane) = v;
        }
        {
            const int row = tid >> 3, ch = kMlaDv / 8 + (tid & 7);
            uint4 v = make_uint4(0, 0, 0, 0);
            if (row < n) {
                v = *reinterpret_cast<const uint4 *>(kvn + (long long)row * cp.kv_tok_stride + 8 * ch);
                v = mla_rope8<Tr>(v, 4 * (tid & 7), pos + row, p);
                if (store) *reinterpret_cast<uint4 *>(cache_row(pos + row) + 8 * ch) = v;
            }
            *reinterpret_cast<uint4 *>(smem + kMlaRow * row + 16 * ch) = v;
        }
        __syncthreads();
        if (active) tile(smem, t + 1);          // token t sees the new tokens 0 .. t
    }

    // ---- epilogue: the wave owns row block rb x dims [dbase, dbase + 16 NDT) ----
    float ltot = quad_sum(l);
    if (PAGED && pg.bad) ltot = __builtin_nanf("");     // a read page outside the pool
    if (!active) return;
    if (S == 1) {
        const float inv = 1.0f / ltot;          // l >= 1: new token 0 is always present
        uint16_t *const orow = ob + c * kMlaDv + dbase + 4 * g;
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt)
            *reinterpret_cast<uint2 *>(orow + 16 * dt) =
                make_uint2(Tr::pack2(o[dt][0] * inv, o[dt][1] * inv), Tr::pack2(o[dt][2] * inv, o[dt][3] * inv));
    } else {
        const long long row = ((long long)b * n + t) * H + head0 + c;
        float *const prow = p.part_o + (row * S + split) * kMlaDv + dbase + 4 * g;
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt)
            *reinterpret_cast<float4 *>(prow + 16 * dt) = make_float4(o[dt][0], o[dt][1], o[dt][2], o[dt][3]);
        if (dpart == 0 && g == 0) p.part_ml[row * S + split] = make_float2(m, ltot);
    }
}

// o[b, t, h, 0:512] = the merge of the splits' partials of row (b n + t) H + h (mla_combine_row), 64 lanes a row.  n H is
// a multiple of 16 and a workgroup holds 4 rows: it lies in one sequence and the B n H rows fill the grid exactly, so
// the workgroup-collective reject_code is called by all its threads with one b.
template <class Tr>
__global__ void __launch_bounds__(256)
mla_chunk_combine_kernel(const MlaChunkKernelParams cp) {
    const DecodeKernelParams &p = cp.m.d;
    constexpr int LPR = kMlaDv / 8;
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long row = gid / LPR;
    const int sub = (int)(gid % LPR);
    const int n = cp.n, nh = n * p.H;
    const int b = (int)(row / nh);
    const int pos = p.seq_len[b];
    if (p.block_table ? chunk::reject_code<true>(p, n, b, pos) : chunk::reject_code<false>(p, n, b, pos))
        return;                                 // o[b] is already poisoned
    const int r = (int)(row - (long long)b * nh), t = r / p.H, h = r - t * p.H;
    mla_combine_row<Tr>(p, row, sub, p.o + ((long long)b * n + t) * cp.o_tok_stride + (long long)h * kMlaDv);
}

template <class Tr, int NHB, bool PAGED>
int mla_chunk_launch_k(const MlaChunkKernelParams &cp, int groups, hipStream_t stream) {
    const DecodeKernelParams &p = cp.m.d;
    dim3 grid(groups, p.num_splits, p.B), block(kDecodeWaves * 64);
    static DynLdsAttr attr;
    if (const int rc = attr.ensure(reinterpret_cast<const void *>(&mla_chunk_attn_kernel<Tr, NHB, PAGED>), kMlaLds,
                                   "mla_chunk_attn_kernel"))
        return rc;
    hipLaunchKernelGGL((mla_chunk_attn_kernel<Tr, NHB, PAGED>), grid, block, kMlaLds, stream, cp);
    return check_launch("mla_chunk_attn_kernel");
}

template <class Tr>
int mla_chunk_launch_t(const MlaChunkKernelParams &cp, hipStream_t stream) {
    const DecodeKernelParams &p = cp.m.d;
    const bool paged = p.block_table != nullptr;
    const int R = cp.n * (p.H / 16), groups = mla_chunk_groups(R);
    int rc;
    // one row block: every wave a quarter of the output dims; two: a half; more: groups of four, a wave each
    if (R == 1) rc = paged ? mla_chunk_launch_k<Tr, 1, true>(cp, groups, stream) : mla_chunk_launch_k<Tr, 1, false>(cp, groups, stream);
    else if (R == 2) rc = paged ? mla_chunk_launch_k<Tr, 2, true>(cp, groups, stream) : mla_chunk_launch_k<Tr, 2, false>(cp, groups, stream);
    else rc = paged ? mla_chunk_launch_k<Tr, 4, true>(cp, groups, stream) : mla_chunk_launch_k<Tr, 4, false>(cp, groups, stream);
    if (rc || p.num_splits == 1) return rc;
    const long long threads = (long long)p.B * cp.n * p.H * (kMlaDv / 8);
    hipLaunchKernelGGL((mla_chunk_combine_kernel<Tr>), dim3((unsigned)(threads / 256)), dim3(256), 0, stream, cp);
    return check_launch("mla_chunk_combine_kernel");
}

}  // namespace

// validated dtype, num_heads in {16, 32, ..., 128}, 1 <= n <= 32: the attention kernel, then (two or more splits) the combine
int launch_mla_decode_chunk(const MlaChunkKernelParams &p, int dtype, hipStream_t stream) {
    return dtype == SFA_DTYPE_FP16 ? mla_chunk_launch_t<Fp16>(p, stream) : mla_chunk_launch_t<Bf16>(p, stream);
}

}  // namespace sfa
