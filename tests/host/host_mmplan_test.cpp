// The product's launch plan (sfgwas_amd/csrc/mm_plan.hpp) on the CPU: the full MmPlan of a table of named cases, the invariants every plan keeps, and the two
// other group-size choosers.  Stand-alone: includes the header, links nothing of the library.
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
    { MmPlanIn c = b; c.rot = RotSrc::f64_cache; c.ncolb = 5; add("22 product-wide cache, five columns: automatic group above the rot-sum group", c); }
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
    {13, 1, true, true, true, true, true, 2, 26, 8192, 26624, 2866153472ULL, 1186, false, true, 0xf000001eu},      // 22 product-wide cache, five columns: automatic group above the rot-sum group
    {13, 1, false, false, false, false, false, 0, 0, 8192, 40960, 4409466880ULL, 1186, false, false, 0x1eu},      // 23 mac_i8 off
};

static int fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { fails++; printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

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
        // mm_plan is plan_at of the chosen group size, and never groups fewer block rows than the rot sums of a product-wide cache
        if (p.G) { const MmPlan a = plan_at(in, p.G); CHECK(a.enc_flags == p.enc_flags && a.panel_words == p.panel_words && a.use_i8 == p.use_i8, "%s: plan_at(G) differs", n); }
        if (p.G && in.dma) CHECK(p.G >= rotsum_group_size(in.mm_group, in.nblockrows), "%s: G below the rot-sum group", n);
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
    // 20
    CHECK(rotsum_group_size(8, 13) == 8 && rotsum_group_size(8, 5) == 5, "20: rotsum_group_size");
    // ModSplit of the product's moduli
    CHECK(prod.nsmall == 4 && prod.nbig == 1 && prod.l_big == 0 && prod.l_small0 == 1 && prod.small_runs == 1 && prod.fp64_planes == 6 && prod.digit_planes == 26 &&
          prod.packed_mask_all == 0x1eu && !prod.too_big && prod.plane_of[1] == 2 && prod.is_big[0] == 1, "ModSplit of the product's moduli");
    const unsigned long long q47[1] = {1ULL << 47};
    CHECK(ModSplit(q47, 1).too_big, "ModSplit: 2^47");
    printf(fails ? "FAILED (%d)\n" : "OK\n", fails);
    return fails ? 1 : 0;
}
