// mm_plan.hpp — the launch plan of the matrix product (matmul.hip) as pure functions: which MAC kernel multiplies, how many block rows share a launch, the layout
// and size of the plaintext panel, whether the transposition rides; and the passes of a whole product (mm_range_plan).  Arithmetic on the moduli, four integers, the configuration and two byte counts: standard
// library only, so that every decision runs on a CPU (tests/host/host_mmplan_test.cpp).  matmul.hip asks the device for the two byte counts and executes the plan.
#pragma once
#include "consts.hpp"
#include <algorithm>
#include <cstdint>

// ---------------------------------------------------------------- the moduli of a product: q[0..L)
// small: below 2^36 (one fp64 plane, five int8 digit planes, packed-limb plaintext rows); big: 46/47-bit (two fp64 planes, six digit planes)
struct ModSplit {
    int L = 0, nsmall = 0, nbig = 0;
    int l_big = -1, l_small0 = -1;        // the first big modulus, the first small one
    int small_runs = 0;                   // runs of consecutive small moduli (the MAC multiplies run by run of like moduli)
    int fp64_planes = 0, digit_planes = 0;   // of all L moduli: 1 / 2 and 5 / 6 per modulus
    int plane_of[SFG_MAXMOD] = {0}, is_big[SFG_MAXMOD] = {0};
    unsigned packed_mask_all = 0;         // bit l: modulus l is small
    bool too_big = false;                 // a modulus >= 2^47: unsupported by the fp64 limb schedule
    ModSplit() {}
    ModSplit(const unsigned long long *q, int L_) : L(L_) {
        for (int l = 0; l < L; l++) {
            if (q[l] >= (1ULL << 47)) too_big = true;
            is_big[l] = q[l] >= (1ULL << 36); plane_of[l] = fp64_planes;
            fp64_planes += is_big[l] ? 2 : 1; digit_planes += is_big[l] ? 6 : 5;
            if (is_big[l]) { if (l_big < 0) l_big = l; nbig++; }
            else { if (l_small0 < 0) l_small0 = l; nsmall++; packed_mask_all |= 1u << l; if (l == 0 || is_big[l - 1]) small_runs++; }
        }
    }
    bool all_small() const { return nbig == 0; }
};

// ---------------------------------------------------------------- byte models of the int8 MAC (mac_i8.hip)
// the two operand streams and the tile-ordered results of one launch
inline size_t mac_i8_stream_bytes(int K, int nl, int ND, int copies_of_rot) {
    const size_t N = SFG_N, H = N / 2, nch = ((size_t)K + 63) / 64;
    return (size_t)nl * (N * nch * 2 * ND * 1024 * copies_of_rot + H * 6 * nch * ND * 1024 + H * 2 * 6 * 2 * 256 * 8);
}
// the plaintext tile buffer of `nl` moduli with ND digits for K' contraction steps
inline size_t mac_i8_tile_bytes(int Kp, int nl, int ND) { return (size_t)nl * (SFG_N / 2) * 6 * (((size_t)Kp + 63) / 64) * ND * 1024; }
// the transposed rot tiles of one MAC group (launch_i8_pack_rot_to)
inline size_t mac_i8_rot_tile_bytes(int K, int nl, int ND) { return (size_t)nl * SFG_N * (((size_t)K + 63) / 64) * 2 * ND * 1024; }

// ---------------------------------------------------------------- the plan of one matmul_accumulate call
enum class RotSrc { own, f64_cache, i8_tiles };   // the call key-switches its rotations itself / the caller holds them as fp64 operand rows / as int8 tiles (I8RotPre)
struct MmPlanIn {
    int mm_group = 8; bool mm_group_auto = true, mac_i8 = true, mac_i8_big = true, pt_compact = true, pt_kmajor = true; int pt_ride = 192; bool no_overlap = true;   // SfgConfig
    bool dma = true;                      // the LDS-DMA / broadcast MAC (false: the A/B build's register-staged kernel)
    unsigned packed_mask = 0;             // mac_dma_packed_mask
    ModSplit mods;
    int s = 0, L = 0, nblockrows = 0, ncolb = 0;
    RotSrc rot = RotSrc::own; int pre_G = 0;       // pre_G: the group size of the caller's int8 tiles
    size_t mem_search = 0;                // free HBM + the pool's regrowable mm.pt / mm.rotf / mi8.* bytes: what the group search may spend
    size_t mem_keep = 0;                  // free HBM + the held mi8.A* bytes: what the transposed copies of all groups (keep_all) may spend
    bool mem_failed = false;              // the device did not answer
};
struct MmPlan {
    int G = 0, ngroups = 0;               // block rows per MAC launch (K = G * 91), launches per block column
    bool keep_all = false;                // a caller's rotation cache of up to 16 groups whose transposed copies all fit: the association scan
    bool use_i8 = false, use_i8_big = false;   // the small moduli / the 46-bit modulus too on the int8 matrix core
    bool compact = false, kmajor = false; int pt_layout = 0, pt_planes = 0;    // MacStrides::pt_layout; digit planes per plaintext (compact)
    size_t prow = 0, plw = 0, panel_words = 0;     // words per plaintext modulus row, per plaintext, per panel
    size_t grp_slices = 0;                // k-slices of one group's fp64 rotation cache (+ 3: see launch_mac_dma)
    bool pipelined = false;               // the next group's key switching on the auxiliary stream
    bool ride_want = false;               // the riding transposition (needs a second panel: matmul.hip probes for it)
    unsigned enc_flags = 0;               // the flag word of launch_encode_rows
};

// Everything downstream of a group size.
// The int8 MAC multiplies with a k-contiguous copy of a group's rot operand, transposed when the operand changes and kept for two operands.  That pays when
// the copy is reused: several block columns in this call, or so few groups that the copies survive from call to call (a caller's rotation cache multiplied one
// block column at a time).  The association scan - one block column per batch against a 62-block-row cache - takes the fp64 kernel unless all copies fit (keep_all).
inline MmPlan plan_at(const MmPlanIn &in, int G) {
    const int N = SFG_N, d = SFG_D, nb = in.nblockrows;
    const bool pre8 = in.rot == RotSrc::i8_tiles, own = in.rot == RotSrc::own;
    MmPlan p;
    p.G = G; p.ngroups = (nb + G - 1) / G;
    p.prow = in.dma ? (size_t)N / 2 : (size_t)N;
    if (in.dma && in.mac_i8 && in.packed_mask && in.rot == RotSrc::f64_cache && p.ngroups <= 16 && !in.mem_failed) {
        const size_t all = mac_i8_stream_bytes(G * d, in.mods.nsmall, 5, 0), per = mac_i8_stream_bytes(G * d, in.mods.nsmall, 5, 1) - all;
        p.keep_all = in.mem_keep >= (size_t)p.ngroups * per + all + SFG_I8_KEEP_RESERVE;     // (the panel, accumulators and key-switch scratch of the call are still to be allocated the first time)
    }
    p.use_i8 = pre8 || (in.dma && in.mac_i8 && in.packed_mask && (p.ngroups <= 2 || in.ncolb >= 4 || p.keep_all));
    p.use_i8_big = pre8 || (p.use_i8 && in.mac_i8_big);        // six digit planes, its own pair of transposed rot copies
    const bool all_i8 = p.use_i8 && (p.use_i8_big || in.mods.all_small());       // every modulus of the product multiplies on the int8 matrix core
    p.grp_slices = (size_t)G * d + 3;
    p.pipelined = in.dma && own && nb > G && !in.no_overlap;
    // Compact panel rows: nothing but digit planes - five (six) planes of N/2 bytes per modulus, back to back: 208 KiB per plaintext at L = 5 instead of five rows
    // of N/2 words (320 KiB).  Room for the second panel of the riding transposition.
    p.compact = in.pt_compact && in.dma && all_i8;
    p.plw = (size_t)in.L * p.prow;
    if (p.compact) { p.pt_planes = in.mods.digit_planes; p.plw = (size_t)p.pt_planes * ((size_t)N / 2) / 8; }
    // K-major panel: the compact panel's bytes ordered [column][plane][128-byte coefficient block][k][128 B], so that the 16 k of a transposition unit's
    // column are one 2 KiB run (32-bit byte offsets inside a plane)
    p.kmajor = p.compact && in.pt_kmajor && (size_t)G * d * 128 * 64 * 32 < (1ULL << 31);
    p.pt_layout = p.kmajor ? 2 : p.compact ? 1 : 0;
    p.panel_words = (size_t)G * d * d * p.plw;               // 91 * 91 = 8281 >= 8192 slots per block row: the tail stays zero
    // The riding transposition (kernels.hpp PtRide): a launch rides in the encode of the NEXT block column of its group - or of the next group's first column
    // where the rot tiles of every group are the caller's: nothing is rebuilt between groups then
    p.ride_want = all_i8 && in.pt_ride > 0 && (in.ncolb >= 2 || (pre8 && nb > G));
    if (in.dma) p.enc_flags = in.packed_mask | (p.use_i8 ? PT_DIGITS : 0u) | (p.use_i8_big ? PT_DIGITS_BIG : 0u) | (p.compact ? PT_COMPACT : 0u) | (p.kmajor ? PT_KMAJOR : 0u);
    return p;
}
// What the group search believes a group of G2 block rows costs in HBM.  The panel, the rotation cache and its pipelining are plan_at's.  Kept as the search has
// always estimated them, NOT as plan_at decides (another estimate is another G on some machine - a speed and memory change):
//  - the second panel is counted wherever the int8 MAC and the ride are configured and the call has two block columns (plan_at's ride_want also needs this call
//    to multiply every modulus on int8: packed rows, few groups or four columns, the 46-bit modulus included);
//  - the int8 MAC's streams are counted wherever it is configured, whether or not this call uses it, with one transposed rot copy (a group's copy is recycled);
//  - a caller's int8 tiles never reach the search, and keep_all cannot matter in it (a caller's cache is searched with four columns or more: int8 anyway).
inline size_t mm_search_estimate(const MmPlanIn &in, int G2) {
    const MmPlan p = plan_at(in, G2);
    const bool ride2 = in.mac_i8 && in.pt_ride > 0 && in.ncolb >= 2;
    size_t need = p.panel_words * 8 * (ride2 ? 2 : 1);
    if (in.rot == RotSrc::own) need += p.grp_slices * in.s * 2 * (size_t)in.mods.fp64_planes * SFG_N * 8 * (p.pipelined ? 2 : 1);
    if (in.mac_i8) {
        need += mac_i8_stream_bytes(G2 * SFG_D, in.mods.nsmall, 5, 1);
        if (in.mac_i8_big && in.mods.nbig) need += mac_i8_stream_bytes(G2 * SFG_D, 1, 6, 1);
    }
    return need;
}
// G block rows share one MAC launch (K = G * 91): accumulators are written once per group instead of read-modify-written per block.
// 16 (24) block rows per launch halve (third) the accumulator read-modify-writes and the per-launch prologues (16: -1.7 % at 100k x 1M, identical bits) but
// need a 43 (65) GB plaintext panel and, for the pipelined rotation caches, 2 x 34.5 (52) GB of operands: taken only when that fits beside what is resident
// (not for fewer than four block columns against a caller's rotation cache - the association scan: fewer launches save a few accumulator passes there, and the
//  larger panel competes with the 115 GB cache for HBM: measured 0.49 s instead of 0.31 s per batch)
inline int mm_group_size(const MmPlanIn &in) {
    const int nb = in.nblockrows;
    if (!in.dma) return 1;
    int G = in.rot == RotSrc::i8_tiles ? in.pre_G : in.mm_group;
    if (in.rot != RotSrc::i8_tiles && in.mm_group_auto && nb > G && (in.ncolb >= 4 || in.rot == RotSrc::own) && in.mods.fp64_planes > 0 && !in.mods.too_big && !in.mem_failed)
        for (int cand : {24, 20, 16, 14, 12, 10}) {
            const int G2 = std::min(cand, nb);
            if (G2 <= G) break;
            if (mm_search_estimate(in, G2) + (12ULL << 30) <= in.mem_search) { G = G2; break; }
        }
    return std::min(G, nb);
}
inline MmPlan mm_plan(const MmPlanIn &in) {
    if (in.nblockrows <= 0 || in.ncolb <= 0) return MmPlan();          // nothing to multiply
    return plan_at(in, mm_group_size(in));
}
// whether mm_plan reads mem_search / mem_keep at all (the caller asks the device only then)
inline bool mm_plan_reads_memory(const MmPlanIn &in) {
    return in.dma && ((in.rot != RotSrc::i8_tiles && in.mm_group_auto && in.nblockrows > in.mm_group) || (in.rot == RotSrc::f64_cache && in.mac_i8 && in.packed_mask));
}

// ---------------------------------------------------------------- the plan of one matmul_resident_range call: the accumulate + finalize passes over block columns
// Several passes would each rebuild the rotation cache of every block row (91 key switches per input ciphertext): when the cache of the whole range fits the
// cap (Q*X at 100k x 1M: 13 block rows = 28 GB) the call builds it once and multiplies as with a caller's cache.  Without key switching in the passes the
// giant-step alignment of pass k runs on the auxiliary stream beside the encode + MAC of pass k + 1: two accumulator buffers of half the budget each.
struct MmRangeIn {
    int s = 0, L = 0, nl = 0, rows = 0, cols = 0, fp64_planes = 0;   // nl: the operand's moduli after the level drop; block rows and columns of the range; ModSplit::fp64_planes
    size_t acc_budget = 0; bool no_overlap = true, dma = true; RotSrc rot = RotSrc::own;      // SfgConfig: acc_budget, no_overlap
};
struct MmRangePlan {
    int jg = 1, npasses = 0;              // block columns per pass, passes
    bool whole_cache = false, overlap = false;         // the call builds the fp64 rotation cache of all its block rows first
    size_t cache_bytes = 0, acc_bytes = 0;             // that cache (3 k-slices of tail included); "mm.acc"
};
inline MmRangePlan mm_range_plan(const MmRangeIn &in) {
    const size_t N = SFG_N, d = SFG_D, per_col = d * in.s * 2 * in.L * N * 8, rowf = (size_t)in.fp64_planes * N;
    MmRangePlan p;
    int jg0 = (int)(in.acc_budget / per_col); if (jg0 < 1) jg0 = 1;
    p.cache_bytes = ((size_t)in.rows * d * in.s * 2 * rowf + 3 * (size_t)in.s * 2 * rowf) * 8;
    p.whole_cache = in.rot == RotSrc::own && in.dma && in.cols > jg0 && in.rows > 0 && in.nl >= in.L && p.cache_bytes <= SFG_MM_WHOLE_CACHE_CAP;
    p.overlap = (p.whole_cache || in.rot != RotSrc::own) && !in.no_overlap;
    p.jg = p.overlap ? (jg0 + 1) / 2 : jg0;
    p.npasses = in.cols > 0 ? (in.cols + p.jg - 1) / p.jg : 0;
    p.acc_bytes = (size_t)p.jg * per_col * (p.overlap ? 2 : 1);
    return p;
}

// The group size of a caller's rotation cache held as int8 rot tiles (i8_rotpre_build), or 0: not taken - the moduli are not one run of small ones plus at most one
// big one, or the tiles of all nbr block rows exceed budget_bytes or one MAC launch.  16 (12) block rows per group where the HBM (mem_search: free + the pool's own
// regrowable bytes) takes the larger plaintext panel (two of them: the encode of a launch runs beside the previous launch's MAC) and plaintext tiles: half the
// launches, half the accumulator read-modify-writes (0.256 against 0.272 s per batch at 500 000 samples, 8 batches)
inline size_t i8pre_tile_bytes(const ModSplit &m, int nbr, int G) {
    size_t t = 0;
    for (int b = 0; b < nbr; b += G) { const int ng = std::min(G, nbr - b); t += mac_i8_rot_tile_bytes(ng * SFG_D, m.nsmall, 5) + (m.nbig ? mac_i8_rot_tile_bytes(ng * SFG_D, 1, 6) : 0); }
    return t;
}
inline int i8pre_group_size(const ModSplit &m, int mm_group, bool mm_group_auto, int s, int nbr, bool mem_failed, size_t mem_search, size_t budget_bytes) {
    const int d = SFG_D;
    if (m.too_big || m.nbig > 1 || m.small_runs != 1) return 0;
    int G = std::min(mm_group, nbr);
    if (mm_group_auto && nbr > G && !mem_failed)
        for (int cand : {16, 12}) {
            const int G2 = std::min(cand, nbr);
            if (G2 <= G) break;
            const size_t panel = (size_t)G2 * d * d * m.L * (SFG_N / 2) * 8 * 2, rotf = ((size_t)G2 * d + 3) * s * 2 * m.fp64_planes * SFG_N * 8;
            const size_t need = i8pre_tile_bytes(m, nbr, G2) + panel + rotf + mac_i8_stream_bytes(G2 * d, m.nsmall, 5, 0) + (m.nbig ? mac_i8_stream_bytes(G2 * d, 1, 6, 0) : 0) + (24ULL << 30);
            if (need <= mem_search && i8pre_tile_bytes(m, nbr, G2) <= budget_bytes) { G = G2; break; }
        }
    if ((long long)G * d * 6 >= 131072 || i8pre_tile_bytes(m, nbr, G) > budget_bytes) return 0;
    return G;
}
