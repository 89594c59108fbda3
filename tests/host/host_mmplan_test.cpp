// The product's launch plan (sfgwas_amd/csrc/mm_plan.hpp) on the CPU: the full MmPlan of a table of named cases, the invariants every plan keeps, the group-size
// chooser of a caller's int8 tiles, and the range plan of a whole product (mm_range_plan).  Stand-alone: includes the header, links nothing of the library.
// The expected rows were recorded from the decision statements matmul_accumulate held inline before they moved into the header.
#include "../../sfgwas_amd/csrc/mm_plan.hpp"
#include <cstdio>
#include <string>
#include <vector>

static const unsigned long long Q_PRODUCT[5] = {0x200000440001ULL, 0x7fff80001ULL, 0x800280001ULL, 0x7ffd80001ULL, 0x7ffc80001ULL};   // PN14QP438, L = 5: one 46-bit + four 35/36-bit
static const unsigned long long Q_SMALL3[3] = {0x7fff80001ULL, 0x800280001ULL, 0x7ffd80001ULL};
static const unsigned long long Q_TWO_BIG[3] = {0x200000440001ULL, 0x7fff80001ULL, 0x200000440001ULL};
static const unsigned long long Q_TWO_RUNS[3] = {0x7fff80001ULL, 0x200000440001ULL, 0x800280001ULL};
constexpr size_t GB = 1000000000ULL;

struct Case { std::string name; const unsigned long long *q; MmPlanIn in; };
struct Want { int G, ngroups; bool keep_all, use_i8, use_i8_big, compact, kmajor; int pt_layout, pt_planes; size_t prow, plw, panel_words, grp_slices; bool pipelined, ride_want; unsigned enc_flags; };

static MmPlanIn with_moduli(MmPlanIn in, const unsigned long long *q, int L) { in.L = L; in.mods = ModSplit(q, L); in.packed_mask = in.dma ? in.mods.packed_mask_all : 0u; return in; }
static std::vector<Case> cases() {
    std::vector<Case> v;
    MmPlanIn b;                                   // case 1: the 100k x 1M product's column pass
    b.s = 15; b.nblockrows = 13; b.ncolb = 14; b.rot = RotSrc::own; b.mem_search = b.mem_keep = 180 * GB;
    b = with_moduli(b, Q_PRODUCT, 5);
    auto add = [&](const char *name, MmPlanIn in, const unsigned long long *q = Q_PRODUCT) { v.push_back(Case{name, q, in}); };
    add("1 column pass, 180 GB", b);
    { MmPlanIn c = b; c.mem_search = c.mem_keep = 20 * GB; add("2 column pass, 20 GB: automatic group refused", c); }
    MmPlanIn g3 = b; g3.mm_group_auto = false; g3.mm_group = 3;
    add("3 mm_group = 3: more than two groups", g3);
    { MmPlanIn c = g3; c.ncolb = 1; add("4 mm_group = 3, one block column: fp64 MAC", c); }
    MmPlanIn scan = b; scan.rot = RotSrc::f64_cache; scan.nblockrows = 62; scan.ncolb = 1; scan.s = 13;
    { MmPlanIn c = scan; c.mem_keep = 250 * GB; add("5a association scan, all copies fit", c); }
    { MmPlanIn c = scan; c.mem_keep = 100 * GB; add("5b association scan, copies do not fit", c); }
    { MmPlanIn c = scan; c.nblockrows = 137; c.mem_keep = 290 * GB; add("5c association scan, more than 16 groups", c); }
    { MmPlanIn c = b; c.rot = RotSrc::i8_tiles; c.pre_G = 16; c.nblockrows = 32; c.ncolb = 1; add("6 caller's int8 tiles, G = 16", c); }
    { MmPlanIn c = b; c.nblockrows = 1; c.ncolb = 1; add("7 one block", c); }
    { MmPlanIn c = b; c.nblockrows = 1; c.ncolb = 2; add("8 two block columns: riding wanted", c); }
    { MmPlanIn c = b; c.mac_i8_big = false; add("9 mac_i8_big off", c); }
    { MmPlanIn c = with_moduli(b, Q_SMALL3, 3); add("10 all small, L = 3", c, Q_SMALL3); }
    { MmPlanIn c = b; c.pt_compact = false; add("11 pt_compact off", c); }
    { MmPlanIn c = b; c.pt_kmajor = false; add("12 pt_kmajor off", c); }
    { MmPlanIn c = b; c.pt_ride = 0; add("13 pt_ride = 0", c); }
    { MmPlanIn c = b; c.mm_group_auto = false; c.mm_group = 100; c.nblockrows = 100; add("14 group of 100: K-major refused", c); }
    { MmPlanIn c = b; c.dma = false; c = with_moduli(c, Q_PRODUCT, 5); add("15 register-staged MAC", c); }
    { MmPlanIn c = g3; c.no_overlap = false; add("16 overlap on, several groups: pipelined", c); }
    { MmPlanIn c = b; c.nblockrows = 0; add("17a no block rows", c); }
    { MmPlanIn c = b; c.ncolb = 0; add("17b no block columns", c); }
    { MmPlanIn c = b; c.mem_failed = true; add("21 memory query failed", c); }
    { MmPlanIn c = b; c.rot = RotSrc::f64_cache; c.ncolb = 5; add("22 product-wide cache, five columns: automatic group", c); }
    { MmPlanIn c = b; c.mac_i8 = false; add("23 mac_i8 off", c); }
    return v;
}
// recorded from the parent's statements, in the order of cases()
static const Want WANT[] = {
    {13, 1, false, true, true, true, true, 2, 26, 8192, 26624, 2866153472ULL, 1186, false, true, 0xf000001eu},      // 1 column pass, 180 GB
    {8, 2, false, true, true, true, true, 2, 26, 8192, 26624, 1763786752ULL, 731, false, true, 0xf000001eu},      // 2 column pass, 20 GB: automatic group refused
    {3, 5, false, true, true, true, true, 2, 26, 8192, 26624, 661420032ULL, 276, false, true, 0xf000001eu},      // 3 mm_group = 3: more than two groups
    {3, 5, false, false, false, false, false, 0, 0, 8192, 40960, 1017569280ULL, 276, false, false, 0x1eu},      // 4 mm_group = 3, one block column: fp64 MAC
    {8, 8, true, true, true, true, true, 2, 26, 8192, 26624, 1763786752ULL, 731, false, false, 0xf000001eu},      // 5a association scan, all copies fit
    {8, 8, false, false, false, false, false, 0, 0, 8192, 40960, 2713518080ULL, 731, false, false, 0x1eu},      // 5b association scan, copies do not fit
    {8, 18, false, false, false, false, false, 0, 0, 8192, 40960, 2713518080ULL, 731, false, false, 0x1eu},      // 5c association scan, more than 16 groups
    {16, 2, false, true, true, true, true, 2, 26, 8192, 26624, 3527573504ULL, 1459, false, true, 0xf000001eu},      // 6 caller's int8 tiles, G = 16
    {1, 1, false, true, true, true, true, 2, 26, 8192, 26624, 220473344ULL, 94, false, false, 0xf000001eu},      // 7 one block
    {1, 1, false, true, true, true, true, 2, 26, 8192, 26624, 220473344ULL, 94, false, true, 0xf000001eu},      // 8 two block columns: riding wanted
    {13, 1, false, true, false, false, false, 0, 0, 8192, 40960, 4409466880ULL, 1186, false, false, 0x8000001eu},      // 9 mac_i8_big off
    {13, 1, false, true, true, true, true, 2, 15, 8192, 15360, 1653550080ULL, 1186, false, true, 0xf0000007u},      // 10 all small, L = 3
    {13, 1, false, true, true, false, false, 0, 0, 8192, 40960, 4409466880ULL, 1186, false, true, 0xc000001eu},      // 11 pt_compact off
    {13, 1, false, true, true, true, false, 1, 26, 8192, 26624, 2866153472ULL, 1186, false, true, 0xe000001eu},      // 12 pt_kmajor off
    {13, 1, false, true, true, true, true, 2, 26, 8192, 26624, 2866153472ULL, 1186, false, false, 0xf000001eu},      // 13 pt_ride = 0
    {100, 1, false, true, true, true, false, 1, 26, 8192, 26624, 22047334400ULL, 9103, false, true, 0xe000001eu},      // 14 group of 100: K-major refused
    {1, 13, false, false, false, false, false, 0, 0, 16384, 81920, 678379520ULL, 94, false, false, 0x0u},      // 15 register-staged MAC
    {3, 5, false, true, true, true, true, 2, 26, 8192, 26624, 661420032ULL, 276, true, true, 0xf000001eu},      // 16 overlap on, several groups: pipelined
    {0, 0, false, false, false, false, false, 0, 0, 0, 0, 0, 0, false, false, 0x0u},      // 17a no block rows (the parent returns before deciding)
    {0, 0, false, false, false, false, false, 0, 0, 0, 0, 0, 0, false, false, 0x0u},      // 17b no block columns (the parent returns before deciding)
    {8, 2, false, true, true, true, true, 2, 26, 8192, 26624, 1763786752ULL, 731, false, true, 0xf000001eu},      // 21 memory query failed
    {13, 1, true, true, true, true, true, 2, 26, 8192, 26624, 2866153472ULL, 1186, false, true, 0xf000001eu},      // 22 product-wide cache, five columns: automatic group
    {13, 1, false, false, false, false, false, 0, 0, 8192, 40960, 4409466880ULL, 1186, false, false, 0x1eu},      // 23 mac_i8 off
};

static int fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { fails++; printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

// mm_range_plan, derived by hand from its statements.  N = 16384, s = 15, L = nl = 5, 6 fp64 planes (one 46-bit + four small moduli), a 24 GiB budget:
//   per_col = 91 * 15 * 2 * 5 * 16384 * 8 = 1 789 132 800;  jg0 = floor(25 769 803 776 / 1 789 132 800) = 14;  rowf = 6 * 16384 = 98 304
//   cache_bytes(rows) = (rows * 91 * 15 * 2 * 98304 + 3 * 15 * 2 * 98304) * 8 = (rows * 2730 + 90) * 786 432;  the cap is 48 GiB = 51 539 607 552
static MmRangePlan range_case(const char *n, const MmRangeIn &in) {
    const MmRangePlan p = mm_range_plan(in);
    const size_t per_col = (size_t)91 * in.s * 2 * in.L * 16384 * 8;
    CHECK(p.jg >= 1, "%s: jg = %d", n, p.jg);
    CHECK(p.npasses == (in.cols + p.jg - 1) / p.jg, "%s: %d passes of %d columns over %d", n, p.npasses, p.jg, in.cols);
    CHECK(p.acc_bytes == (size_t)p.jg * per_col * (p.overlap ? 2 : 1), "%s: acc bytes %zu", n, p.acc_bytes);
    CHECK(!p.whole_cache || in.rot == RotSrc::own, "%s: a whole-range cache beside a caller's rotations", n);
    return p;
}
static void range_plan_cases() {
    MmRangeIn b;
    b.s = 15; b.L = b.nl = 5; b.rows = 13; b.cols = 123; b.fp64_planes = 6; b.acc_budget = 24ULL << 30; b.no_overlap = true; b.dma = true; b.rot = RotSrc::own;
#define RANGE(name, in, WC, CB, OV, JG, NP, AB) do { const MmRangePlan p = range_case(name, in); \
        CHECK(p.whole_cache == (WC) && p.overlap == (OV) && p.jg == (JG) && p.npasses == (NP) && p.acc_bytes == (size_t)(AB) && (!(CB) || p.cache_bytes == (size_t)(CB)), \
              "%s: whole_cache %d (%zu bytes), overlap %d, jg %d, %d passes, acc %zu", name, p.whole_cache, p.cache_bytes, p.overlap, p.jg, p.npasses, p.acc_bytes); } while (0)
    // R1: 13 x 123, one queue.  123 > 14 columns, cache (13 * 2730 + 90) * 786432 = 35580 * 786432 = 27 981 250 560 <= cap: taken.  no_overlap: jg = 14,
    // ceil(123 / 14) = 9 passes, acc 14 * 1 789 132 800 = 25 047 859 200
    RANGE("R1 13 x 123, one queue", b, true, 27981250560ULL, false, 14, 9, 25047859200ULL);
    // R2: two queues: overlap, jg = (14 + 1) / 2 = 7, ceil(123 / 7) = 18 passes, acc 7 * per_col * 2 = 25 047 859 200
    MmRangeIn two = b; two.no_overlap = false;
    RANGE("R2 13 x 123, two queues", two, true, 27981250560ULL, true, 7, 18, 25047859200ULL);
    // R3: the cap's edge.  23 rows: (62790 + 90) * 786432 = 49 450 844 160 <= 51 539 607 552; 24 rows: (65520 + 90) * 786432 = 51 597 803 520 > cap
    { MmRangeIn c = b; c.rows = 23; RANGE("R3a 23 rows: at the cap", c, true, 49450844160ULL, false, 14, 9, 25047859200ULL); }
    { MmRangeIn c = b; c.rows = 24; RANGE("R3b 24 rows: past the cap", c, false, 51597803520ULL, false, 14, 9, 25047859200ULL); }
    { MmRangeIn c = two; c.rows = 24; RANGE("R3c 24 rows, two queues: own rotations in every pass, no overlap", c, false, 51597803520ULL, false, 14, 9, 25047859200ULL); }
    // R4: 14 columns fit one pass (cols > jg0 fails): no cache; 1 pass
    { MmRangeIn c = b; c.cols = 14; RANGE("R4a 14 columns", c, false, 0, false, 14, 1, 25047859200ULL); }
    { MmRangeIn c = two; c.cols = 5; RANGE("R4b 5 columns, two queues", c, false, 0, false, 14, 1, 25047859200ULL); }
    // R5: the operand has fewer moduli than the product after the level drop (the accumulate phase refuses it): no cache
    { MmRangeIn c = b; c.nl = 4; RANGE("R5 nl < L", c, false, 0, false, 14, 9, 25047859200ULL); }
    // R6: a caller's rotations: never a cache of the call's own; overlap is !no_overlap alone
    for (RotSrc r : {RotSrc::f64_cache, RotSrc::i8_tiles}) {
        MmRangeIn c = b; c.rot = r; RANGE("R6a caller's rotations, one queue", c, false, 0, false, 14, 9, 25047859200ULL);
        c.no_overlap = false; RANGE("R6b caller's rotations, two queues", c, false, 0, true, 7, 18, 25047859200ULL);
        c.cols = 1; RANGE("R6c caller's rotations, one column, two queues", c, false, 0, true, 7, 1, 25047859200ULL);
    }
    // R7: the register-staged MAC has no fp64 operand rows: no cache
    { MmRangeIn c = two; c.dma = false; RANGE("R7 dma off", c, false, 0, false, 14, 9, 25047859200ULL); }
    // R8: a budget below one column (1 GiB < 1 789 132 800): jg = 1, 123 passes of one column; with the cache and two queues (1 + 1) / 2 = 1, two buffers
    { MmRangeIn c = b; c.acc_budget = 1ULL << 30; RANGE("R8a budget below one column", c, true, 27981250560ULL, false, 1, 123, 1789132800ULL);
      c.no_overlap = false; RANGE("R8b the same, two queues", c, true, 27981250560ULL, true, 1, 123, 3578265600ULL); }
    // R9: no block rows (an empty X^T range): no cache; no block columns: no pass
    { MmRangeIn c = two; c.rows = 0; RANGE("R9a no rows", c, false, 0, false, 14, 9, 25047859200ULL); }
    { MmRangeIn c = b; c.cols = 0; RANGE("R9b no columns", c, false, 0, false, 14, 0, 25047859200ULL); }
#undef RANGE
}

int main() {
    const std::vector<Case> cs = cases();
    CHECK(cs.size() == sizeof WANT / sizeof WANT[0], "%zu cases, %zu expected rows", cs.size(), sizeof WANT / sizeof WANT[0]);
    for (size_t i = 0; i < cs.size() && i < sizeof WANT / sizeof WANT[0]; i++) {
        const MmPlanIn &in = cs[i].in; const MmPlan p = mm_plan(in); const Want &w = WANT[i]; const char *n = cs[i].name.c_str();
#define FIELD(f, fmt) CHECK(p.f == w.f, "%s: " #f " = " fmt ", expected " fmt, n, p.f, w.f)
        FIELD(G, "%d"); FIELD(ngroups, "%d"); FIELD(keep_all, "%d"); FIELD(use_i8, "%d"); FIELD(use_i8_big, "%d"); FIELD(compact, "%d"); FIELD(kmajor, "%d");
        FIELD(pt_layout, "%d"); FIELD(pt_planes, "%d"); FIELD(prow, "%zu"); FIELD(plw, "%zu"); FIELD(panel_words, "%zu"); FIELD(grp_slices, "%zu");
        FIELD(pipelined, "%d"); FIELD(ride_want, "%d"); FIELD(enc_flags, "%x");
#undef FIELD
        // invariants of every plan
        CHECK(p.G <= in.nblockrows, "%s: G = %d above %d block rows", n, p.G, in.nblockrows);
        CHECK(p.ngroups == (p.G ? (in.nblockrows + p.G - 1) / p.G : 0), "%s: ngroups = %d", n, p.ngroups);
        CHECK(!p.compact || p.use_i8, "%s: compact without the int8 MAC", n);
        CHECK(!p.kmajor || p.compact, "%s: K-major without compact rows", n);
        CHECK(!p.ride_want || p.use_i8, "%s: riding without the int8 MAC", n);
        CHECK(!p.pipelined || in.rot == RotSrc::own, "%s: pipelined with a caller's rotations", n);
        CHECK(p.pt_layout == (p.kmajor ? 2 : p.compact ? 1 : 0), "%s: pt_layout", n);
        if (in.L == 5 && in.dma && p.G) CHECK(p.plw * 8 == (p.compact ? 208u : 320u) * 1024u, "%s: %zu bytes per plaintext", n, p.plw * 8);     // the figures README and DESIGN state
        // mm_plan is plan_at of the chosen group size
        if (p.G) { const MmPlan a = plan_at(in, p.G); CHECK(a.enc_flags == p.enc_flags && a.panel_words == p.panel_words && a.use_i8 == p.use_i8, "%s: plan_at(G) differs", n); }
    }
    // 18: i8pre_group_size, 20 block rows of the product's moduli at s = 13: the candidates 16 and 12, the fallback, a budget below the tiles
    const ModSplit prod(Q_PRODUCT, 5);
    const size_t tiles16 = i8pre_tile_bytes(prod, 20, 16), tiles8 = i8pre_tile_bytes(prod, 20, 8);
    CHECK(i8pre_group_size(prod, 8, true, 13, 20, false, 300 * GB, 200 * GB) == 16, "18: generous memory");
    CHECK(i8pre_group_size(prod, 8, true, 13, 20, false, 180 * GB, 200 * GB) == 12, "18: memory for 12, not 16: got %d", i8pre_group_size(prod, 8, true, 13, 20, false, 180 * GB, 200 * GB));
    CHECK(i8pre_group_size(prod, 8, true, 13, 20, false, 100 * GB, 200 * GB) == 8, "18: fallback to mm_group");
    CHECK(i8pre_group_size(prod, 8, true, 13, 20, true, 300 * GB, 200 * GB) == 8, "18: memory query failed");
    CHECK(i8pre_group_size(prod, 8, false, 13, 20, false, 300 * GB, 200 * GB) == 8, "18: a caller's group size");
    CHECK(i8pre_group_size(prod, 8, true, 13, 20, false, 300 * GB, tiles16) == 16 && i8pre_group_size(prod, 8, true, 13, 20, false, 300 * GB, tiles16 - 1) == 0, "18: budget at / below the tiles of 16");
    CHECK(tiles16 < tiles8 && i8pre_group_size(prod, 8, true, 13, 20, false, 100 * GB, tiles8 - 1) == 0, "18: tight budget at the fallback");
    CHECK(i8pre_group_size(prod, 240, false, 13, 300, false, 300 * GB, ~(size_t)0) == 240 && i8pre_group_size(prod, 241, false, 13, 300, false, 300 * GB, ~(size_t)0) == 0, "18: K * 6 digits at / past one MAC launch");
    // 19: not one run of small moduli plus at most one big one
    CHECK(i8pre_group_size(ModSplit(Q_TWO_BIG, 3), 8, true, 13, 20, false, 300 * GB, 200 * GB) == 0, "19: two 46-bit moduli");
    CHECK(i8pre_group_size(ModSplit(Q_TWO_RUNS, 3), 8, true, 13, 20, false, 300 * GB, 200 * GB) == 0, "19: two runs of small moduli");
    range_plan_cases();
    // ModSplit of the product's moduli
    CHECK(prod.nsmall == 4 && prod.nbig == 1 && prod.l_big == 0 && prod.l_small0 == 1 && prod.small_runs == 1 && prod.fp64_planes == 6 && prod.digit_planes == 26 &&
          prod.packed_mask_all == 0x1eu && !prod.too_big && prod.plane_of[1] == 2 && prod.is_big[0] == 1, "ModSplit of the product's moduli");
    const unsigned long long q47[1] = {1ULL << 47};
    CHECK(ModSplit(q47, 1).too_big, "ModSplit: 2^47");
    printf(fails ? "FAILED (%d)\n" : "OK\n", fails);
    return fails ? 1 : 0;
}
