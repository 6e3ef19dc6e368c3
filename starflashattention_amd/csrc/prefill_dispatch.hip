// Picks the prefill kernel: sfa_debug_set("prefill_impl", id) with an id of PrefillImpl (prefill_common.h), or the
// library's own choice (kPrefillAuto, the default).  Forced choices serve the tests and tools/ only -- the launch path
// reads no environment variable.
//   head_dim 256, whatever the id: prefill_w4d_kernel.hip (60: the 4-wave persistent structure, 32 query rows per wave);
//     prefill_d256_kernel.hip (61: compiler-scheduled) when forced or when a head's rows do not fit 32-bit descriptors.
//   auto, head_dim 64 / 128:
//     the 4-wave persistent kernel (40, prefill_w4_kernel.hip: one wave per SIMD, 64 query rows per wave, O^T in the
//     accumulator file, K/V by LDS-DMA, 256 persistent workgroups) whenever the problem has enough 256-row q-tiles to
//     feed the 256 CUs (and, under the causal mask, rows long enough to amortise its per-q-tile fixed costs: the rule
//     and its measurements are in auto_prefill_impl below);
//   otherwise:
//     the 8-wave 256-row software-pipelined kernel (1, prefill_kernel.hip) whenever the problem has enough of its
//     workgroups (a pair of 256-row q-tiles each) for about half the 256 CUs; smaller problems take the 128-row
//     geometry (20, prefill_kernel_bm128.hip: four times the workgroups).
//   Each geometry comes in two numeric flavours: exact scale (scores = fp32 QK^T times the scale in fp32) and
//   prescaled Q (Q * scale * log2 e rounded to 16 bit once per q-tile, the scale pass gone from the inner loop: +5 %,
//   score error growing with the logits).  Exact is the default; the prescaled flavour runs only for callers that set
//   sfa_prefill_args.fast_scale and want no log-sum-exp.  Within a flavour the geometries agree to fp32 summation order.
//   1 / 20 / 40 pick the flavour by that rule; 3 / 21 / 41 force prescaled, 10 / 22 / 42 exact.
//   2 / 4 / 43 / 44, the diagnostic builds, exist in the A/B library only (build_lib(variants=True)).  Any other id --
//   the retired generations' 0, 30..32 and 80..119 among them -- fails before any HIP call.
// last_prefill_kernel (sfa_debug_get) reports the id that ran, the flavour resolved (8-wave exact by policy: 1).
#include "prefill_common.h"

namespace sfa {

namespace {

// SFA_OK if this library serves prefill_impl `which` for this call.  The stamping builds need an lse buffer that holds
// what they write (u64 entries in the [B, Hq, Sq] float buffer).
int check_prefill_impl(int which, const PrefillKernelParams &p) {
    long long stamps = 0;
    switch (which) {
        case kPrefillAuto:
        case kPrefill8w: case kPrefill8wPrescaled: case kPrefill8wExact:
        case kPrefillBm128: case kPrefillBm128Prescaled: case kPrefillBm128Exact:
        case kPrefillW4: case kPrefillW4Prescaled: case kPrefillW4Exact:
        case kPrefillD256W4: case kPrefillD256:
            return SFA_OK;
#ifdef SFA_WITH_VARIANTS
        case kPrefill8wUnstaged: return SFA_OK;
        case kPrefill8wStamps: stamps = 1024 + 2048 * 4 * 2; break;     // step stamps below 1024, then 2048 wgs x 4 x 2
        case kPrefillW4Stamps: stamps = 4 * 16 * 8; break;              // 4 waves x 16 q-tiles x 8
        case kPrefillW4Events: stamps = 4 * 512; break;                 // 4 waves x 512 events
#else
        case kPrefill8wUnstaged: case kPrefill8wStamps: case kPrefillW4Stamps: case kPrefillW4Events:
            return fail(SFA_ERR_BAD_SHAPE, "prefill_impl %d needs the diagnostics build of the library "
                        "(build_lib(variants=True))", which);
#endif
        default:
            return fail(SFA_ERR_BAD_SHAPE, "prefill_impl %d: no such prefill kernel (prefill_common.h)", which);
    }
    if (!p.lse || (long long)p.B * p.Hq * p.Sq * (long long)sizeof(float) < stamps * 8)
        return fail(SFA_ERR_BAD_SHAPE, "prefill_impl %d is a stamping build: it needs an lse buffer of at least %lld bytes",
                    which, stamps * 8);
    return SFA_OK;
}

// The library's own choice for head_dim 64 / 128
int auto_prefill_impl(const PrefillKernelParams &p, int head_dim, bool causal) {
    const long long nq = (p.Sq + 255) / 256;
    const long long qtiles = (long long)p.B * p.Hq * nq;
    // Measured crossover of the 4-wave persistent kernel against the best of the other two (tools/prefill_crossover.sh,
    // round 3's kernel, profiles/r03_prefill_crossover.txt).  Full attention: from 256 q-tiles on (+10..25 %; 128: -3 %),
    // whatever the key count (8 x 32 x 4096 queries against 64 .. 1024 keys: +16..25 %).  Under the causal mask its
    // per-q-tile fixed costs weigh more on short rows: 16+ q-tiles per head from 256 q-tiles on (+2..7 %), 8 per head from
    // 1024 (512: -2 %, 2048: +8 %), 4 per head (seqlen 1024) from 2048 (+2 %; 4096: +11 %).  Fewer keys than queries
    // under the (bottom-right aligned) causal mask leaves q-tiles with few or no keys -- 8 x 32 x 4096 against 1024 keys
    // -20 %, against 2048 -6 % -- so those go to the other kernels.
    const bool w4_pays = !causal ? qtiles >= kW4MinTiles
                       : p.Sk < p.Sq ? false
                       : nq >= 16 ? qtiles >= 256 : nq >= 8 ? qtiles >= 1024 : nq >= 4 ? qtiles >= 2048 : false;
    if (w4_pays && prefill_w4_serves(p, head_dim)) return kPrefillW4;
    // the 8-wave kernel runs one workgroup per PAIR of q-tiles.  Measured crossover
    // (tools/prefill_small_grids.sh): causal, 64 pair-workgroups 128-row +18..39 %, 128: -10..+7 %,
    // 192+: 256-row +15 %; full attention (pairing balances nothing there), 128: 128-row +39 %, 192: -3 %
    const long long wgs = (long long)p.B * p.Hq * ((nq + 1) / 2);
    return wgs < (causal ? 128 : 192) ? kPrefillBm128 : kPrefill8w;
}

// Keys per tile of the kernel `which` names where that kernel forms a key row's offset in 32 bits (prefill_common.h's
// pitch limit), 0 where it does not: the 4-wave kernels check their own descriptors, an unknown id fails on its own.
int pitch_bound_tile(int which) {
    switch (which) {
        case kPrefill8w: case kPrefill8wPrescaled: case kPrefill8wExact: case kPrefill8wUnstaged: case kPrefill8wStamps:
            return prefill::kBN;
        case kPrefillBm128: case kPrefillBm128Prescaled: case kPrefillBm128Exact:
            return kBm128Keys;
        default:
            return 0;
    }
}

}  // namespace

int launch_prefill(const PrefillKernelParams &p, int dtype, int head_dim, bool causal, hipStream_t stream) {
    int which = g_knobs.prefill_impl.load(std::memory_order_relaxed);
    // The K / V row pitch against the kernel that would run: a check of the call's arguments, so it comes before those
    // of the debug knob.  (head_dim 256 has prefill_d256_kernel.hip, which indexes in 64 bits, behind the 4-wave kernel.)
    if (head_dim != 256)
        if (const int tile = pitch_bound_tile(which == kPrefillAuto ? auto_prefill_impl(p, head_dim, causal) : which))
            if (const int rc = check_prefill_kv_pitch("sfa_prefill_fwd", "seq", p.ks[2], p.vs[2], tile, head_dim)) return rc;
    if (const int rc = check_prefill_impl(which, p)) return rc;
    auto ran = [](int id) { g_knobs.last_prefill_kernel.store(id, std::memory_order_relaxed); };
    const int flavour = p.fast_scale ? 1 : 2;       // what "by policy" resolves to (1 prescaled, 2 exact)
    if (head_dim == 256) {
        if (which != kPrefillD256 && prefill_w4d_serves(p)) { ran(kPrefillD256W4); return launch_prefill_w4d(p, dtype, causal, stream); }
        ran(kPrefillD256);
        return launch_prefill_d256(p, dtype, causal, stream);
    }
    if (which == kPrefillAuto) which = auto_prefill_impl(p, head_dim, causal);
    switch (which) {
        case kPrefill8w:
            ran(p.fast_scale ? kPrefill8wPrescaled : kPrefill8w);
            return launch_prefill_main(p, dtype, head_dim, causal, stream, 0);
        case kPrefill8wPrescaled: ran(which); return launch_prefill_main(p, dtype, head_dim, causal, stream, 1);
        case kPrefill8wExact: ran(which); return launch_prefill_main(p, dtype, head_dim, causal, stream, 2);
        case kPrefill8wUnstaged: ran(which); return launch_prefill_main(p, dtype, head_dim, causal, stream, 3);
        case kPrefill8wStamps: ran(which); return launch_prefill_main(p, dtype, head_dim, causal, stream, 4);
        case kPrefillBm128: case kPrefillBm128Prescaled: case kPrefillBm128Exact:
            ran(which == kPrefillBm128 ? kPrefillBm128 + flavour : which);
            return launch_prefill_bm128(p, dtype, head_dim, causal, stream, which - kPrefillBm128);
        case kPrefillW4: case kPrefillW4Prescaled: case kPrefillW4Exact: case kPrefillW4Stamps: case kPrefillW4Events:
            ran(which == kPrefillW4 ? kPrefillW4 + flavour : which);
            return launch_prefill_w4(p, dtype, head_dim, causal, stream, which - kPrefillW4);
        default:        // 60 / 61
            return fail(SFA_ERR_BAD_SHAPE, "prefill_impl %d serves head_dim 256 only (got %d)", which, head_dim);
    }
}

}  // namespace sfa
