// Shared pieces of the gfx950 prefill kernels: tile geometry, the block -> (head, q-tile) map, the
// prefill_impl table and the launchers.  Design notes: prefill_kernel.hip.
#pragma once
#include "sfa_device.h"
#include "sfa_host.h"

namespace sfa {
namespace prefill {

constexpr int kBM = 256;      // query rows per workgroup
constexpr int kBN = 64;       // keys per tile
constexpr int kThreads = 512;

__device__ __forceinline__ float ninf() { return -__builtin_huge_valf(); }

typedef __attribute__((address_space(3))) i16x4 lds_i16x4;


// XCD-aware decode of blockIdx.x: XCD x (= bid % 8 under round-robin dispatch; a speed hint only)
// owns heads [x*bh_per_xcd, (x+1)*bh_per_xcd) and walks each head's q-tiles heaviest-first.
struct BlockCoord { int bh, qt; };
__device__ __forceinline__ BlockCoord block_coord(const PrefillKernelParams &p) {
    const int bid = blockIdx.x;
    const int xcd = bid & 7, slot = bid >> 3;
    BlockCoord c;
    c.bh = xcd * p.bh_per_xcd + slot / p.nq_tiles;
    c.qt = p.nq_tiles - 1 - (slot % p.nq_tiles);
    return c;
}

}  // namespace prefill

// sfa_debug_set("prefill_impl", id): the kernel launch_prefill runs (prefill_dispatch.hip).  Stable ids: tests, tools/,
// profiles/ and sfa_debug_get("last_prefill_kernel") cite them.  The diagnostic builds are in the A/B library only.
enum PrefillImpl : int {
    kPrefillAuto = -1,
    kPrefill8w = 1, kPrefill8wPrescaled = 3, kPrefill8wExact = 10,      // 8-wave 256-row kernel: by policy / forced
    kPrefill8wUnstaged = 2,                 // diagnostic: un-staged softmax slices (tools/prefill_ab.py)
    kPrefill8wStamps = 4,                   // diagnostic: in-kernel stamps into the lse buffer (tools/prefill_*stamps.py)
    kPrefillBm128 = 20, kPrefillBm128Prescaled = 21, kPrefillBm128Exact = 22,      // 128-row kernel
    kPrefillW4 = 40, kPrefillW4Prescaled = 41, kPrefillW4Exact = 42,    // 4-wave persistent kernel
    kPrefillW4Stamps = 43,                  // diagnostic: q-tile stamps into the lse buffer (tools/w4_seam_stamps.py)
    kPrefillW4Events = 44,                  // diagnostic: event log into the lse buffer (tools/w4_events.py)
    kPrefillD256W4 = 60, kPrefillD256 = 61, // head_dim 256: persistent kernel / compiler-scheduled fallback
};

// The launchers of the 8-wave, 128-row and 4-wave kernels.  force: 0 = flavour by policy (exact unless the caller opted
// into fast_scale), 1 = prescaled, 2 = exact; 3 / 4 = the diagnostic builds (A/B library only) of the enum above.
int launch_prefill_main(const PrefillKernelParams &p, int dtype, int head_dim, bool causal, hipStream_t stream,
                        int force = 0);
int launch_prefill_bm128(const PrefillKernelParams &p, int dtype, int head_dim, bool causal, hipStream_t stream,
                         int force = 0);
int launch_prefill_w4(const PrefillKernelParams &p, int dtype, int head_dim, bool causal, hipStream_t stream,
                      int force = 0);
// whether one head's Q / K / V rows fit the 32-bit buffer descriptors of the 4-wave kernel (else: the 8-wave kernel)
bool prefill_w4_serves(const PrefillKernelParams &p, int head_dim);
// The K / V row pitch (elements between two keys: the seq stride, the token stride of a packed call) the 8-wave kernels
// address.  They keep a tile's base in 64 bits and form a row's byte offset inside the tile in 32: row * 2 * pitch +
// 16 * chunk, row < tile_rows, chunk < head_dim / 8 (prefill_stream.h and prefill_kernel.hip: tiles of prefill::kBN
// keys; prefill_kernel_bm128.hip: of kBm128Keys).  The limit is the largest multiple of 8 at which the last chunk of a
// tile's last row stays below 2^32; the entry points reject what lies above it, the hot loops stay as they are.
// prefill_d256_kernel.hip indexes in 64 bits and has no such limit; the 4-wave kernels guard their descriptors
// (prefill_w4_serves, prefill_w4d_serves).
constexpr int kBm128Keys = 32;
constexpr long long prefill_max_kv_pitch(int tile_rows, int head_dim) {
    return ((1ll << 32) - 1 - 16 * (head_dim / 8 - 1)) / (2 * (tile_rows - 1)) / 8 * 8;
}
// SFA_OK, or SFA_ERR_BAD_SHAPE under the call's name `name`; what: "seq" or "token"
inline int check_prefill_kv_pitch(const char *name, const char *what, long long k_pitch, long long v_pitch, int tile_rows,
                                  int head_dim) {
    const long long limit = prefill_max_kv_pitch(tile_rows, head_dim);
    if (k_pitch <= limit && v_pitch <= limit) return SFA_OK;
    return fail(SFA_ERR_BAD_SHAPE, "%s: %s %s stride %lld exceeds %lld elements, the row pitch the %d-key tiles address at "
                "head_dim %d", name, k_pitch > limit ? "k" : "v", what, k_pitch > limit ? k_pitch : v_pitch, limit,
                tile_rows, head_dim);
}
// the flavours of the 4-wave kernel that live in translation units of their own (prefill_w4_kernel_p1..3.hip; bf16 exact
// scale is in prefill_w4_kernel.hip itself): called by launch_prefill_w4 only
int launch_prefill_w4_fp16_exact(const PrefillKernelParams &p, bool causal, hipStream_t stream);
int launch_prefill_w4_fp16_prescaled(const PrefillKernelParams &p, bool causal, hipStream_t stream);
int launch_prefill_w4_bf16_prescaled(const PrefillKernelParams &p, bool causal, hipStream_t stream);
// head_dim 256: the one-wave-per-SIMD persistent kernel (prefill_w4d_kernel.hip) wherever one head's rows fit its
// 32-bit buffer descriptors, the compiler-scheduled kernel (prefill_d256_kernel.hip) otherwise
int launch_prefill_w4d(const PrefillKernelParams &p, int dtype, bool causal, hipStream_t stream);
bool prefill_w4d_serves(const PrefillKernelParams &p);
int launch_prefill_d256(const PrefillKernelParams &p, int dtype, bool causal, hipStream_t stream);
// q-tiles (256 rows) a full-attention problem must have before the auto rule picks the persistent kernel: one per CU
constexpr long long kW4MinTiles = 256;

}  // namespace sfa
