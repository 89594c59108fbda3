// The multi-GPU engine's host arithmetic (sfgwas_amd/csrc/mg_plan.hpp) on the CPU: the SNP-block shard, the sizes and the exchange schedule of one rank's Q' * X^T,
// the host-form offsets and the re-shard segment table.  Stand-alone: includes the header, links nothing of the library.
// The reference is a literal restatement of the expressions and loops mgpu.hip held inline before they moved into the header (sfg_mgpu_shard, rank_contract's
// declarations, its prepare() and its exchange() loop, the row copies of sfg_mgpu_matmul, the segment loop of sfg_mgpu_geno_filter); the invariants are asserted
// directly as well.
#include "../../sfgwas_amd/csrc/mg_plan.hpp"
#include <cstdio>
#include <string>
#include <vector>

static int fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { fails++; printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

constexpr size_t SLOTS = 8192;

// ---------------------------------------------------------------- the reference: the parent's statements, word for word
struct RefShard { size_t b0, b1, c0, c1; };
static RefShard ref_shard(int world, size_t ncol, int rank) {
    const size_t nblk = (ncol + SLOTS - 1) / SLOTS, b0 = nblk * (size_t)rank / (size_t)world, b1 = nblk * ((size_t)rank + 1) / (size_t)world;
    return {b0, b1, b0 * SLOTS, std::min(b1 * (size_t)SLOTS, ncol)};
}
// rank_contract: what it asked the scratch pools for, what it handed the two reductions and the all-reduce, and its exchange loop as a trace
struct RefStep { int j, je, ev; bool wait, mul; size_t buf; };              // ev: the index of ev_acc / ev_rs the step records
struct RefRs { int c; size_t src, dst; };
struct RefContract {
    int gpr, g_lo, PW; bool pipe;
    size_t outw, accw, col, colp, mine, mine_bytes, ar_bytes, acc2_bytes, cache_bytes, red_mine, red_out, ar_words;
    int first_j0, first_j1;                                                 // the columns multiplied in prepare()
    std::vector<RefStep> steps; std::vector<RefRs> rs;
};
static RefContract ref_contract(int world, int rank, int s, int L, int nbr_x, int nloc, bool direct, bool G, size_t cache_w, size_t cache_budget) {
    RefContract o;
    const int d = 91, N = 16384;
    const size_t outw = (size_t)2 * L * N, accw = (size_t)s * outw;
    const int gpr = (d + world - 1) / world, g_lo = rank * gpr;
    const size_t col = (size_t)d * accw, colp = (size_t)world * gpr * accw, mine = (size_t)gpr * accw;
    bool pipe = false;
    int PW = 1;
    size_t acc_w = 0;
    pipe = !nloc || G || cache_w * 8 <= cache_budget;
    o.mine_bytes = (size_t)nbr_x * mine * 8;
    o.ar_bytes = direct ? (size_t)s * nbr_x * outw * 8 : 0;
    o.cache_bytes = 0;
    if (pipe) {
        PW = G ? 2 : 1;
        const size_t acc2_bytes = (size_t)2 * PW * colp * 8;
        o.acc2_bytes = acc2_bytes;
        if (nloc && !G) o.cache_bytes = cache_w * 8;
        o.first_j0 = 0; o.first_j1 = G ? std::min(PW, nbr_x) : 1;
    } else {
        acc_w = ((size_t)nbr_x * d + ((size_t)world * gpr - d)) * accw;
        o.acc2_bytes = acc_w * 8;
        o.first_j0 = 0; o.first_j1 = nbr_x;
    }
    if (pipe) {
        for (int j = 0, p = 0; j < nbr_x; j += PW, p++) {
            const int je = std::min(nbr_x, j + PW);
            const size_t buf = (size_t)(p & 1) * PW * colp;
            o.steps.push_back({j, je, p & 1, p >= 2, j > 0, buf});
            for (int c = j; c < je; c++) o.rs.push_back({c, buf + (size_t)(c - j) * colp, (size_t)c * mine});
        }
    } else {
        o.steps.push_back({0, nbr_x, 0, false, false, 0});
        for (int j = 0; j < nbr_x; j++) o.rs.push_back({j, (size_t)j * col, (size_t)j * mine});
    }
    o.red_mine = (size_t)nbr_x * gpr * s * 2; o.red_out = (size_t)s * nbr_x * 2; o.ar_words = (size_t)s * nbr_x * outw;
    o.gpr = gpr; o.g_lo = g_lo; o.PW = PW; o.pipe = pipe; o.outw = outw; o.accw = accw; o.col = col; o.colp = colp; o.mine = mine;
    return o;
}
// sfg_mgpu_geno_filter's segment loop over the old shards (present, blk0, ncol) of the local ranks
struct RefOld { bool present; size_t blk0, ncol; };
struct RefSeg { size_t j; unsigned gcol0, out0; };
static bool ref_segments(const std::vector<unsigned> &cols, size_t c0, size_t c1, const std::vector<RefOld> &shard, std::vector<RefSeg> &t) {
    const size_t n = shard.size();
    t.clear();
    size_t served = 0;
    for (size_t j = 0; j < n && c1 > c0; j++) {
        if (!shard[j].present) continue;
        const size_t o0 = shard[j].blk0 * SLOTS, o1 = o0 + shard[j].ncol;                  // the old window of local rank j
        const auto wb = cols.begin() + (ptrdiff_t)c0, we = cols.begin() + (ptrdiff_t)c1;
        const size_t lo = (size_t)(std::lower_bound(wb, we, o0) - wb), hi = (size_t)(std::lower_bound(wb, we, o1) - wb);
        if (hi == lo) continue;
        if (lo != served) break;
        t.push_back({j, (unsigned)o0, (unsigned)lo});
        served = hi;
    }
    return served == c1 - c0;
}

// ---------------------------------------------------------------- the shard
static void check_shards() {
    for (size_t nblk = 1; nblk <= 40; nblk++) for (size_t ncol : {(nblk - 1) * SLOTS + 1, nblk * SLOTS - 77, nblk * SLOTS}) for (int world = 1; world <= 64; world++) {
        size_t nxt_blk = 0, nxt_col = 0, empty = 0;
        for (int r = 0; r < world; r++) {
            const MgShard sh = mg_shard(world, ncol, r); const RefShard w = ref_shard(world, ncol, r);
            CHECK(sh.blk0 == w.b0 && sh.blk1 == w.b1 && sh.col0 == w.c0 && sh.col1 == w.c1, "shard(%d, %zu, %d) = {%zu, %zu, %zu, %zu}", world, ncol, r, sh.blk0, sh.blk1, sh.col0, sh.col1);
            CHECK(sh.blk0 == nxt_blk && sh.col0 == nxt_col, "shard(%d, %zu, %d) is not contiguous with its predecessor", world, ncol, r);
            CHECK(sh.blk0 <= sh.blk1 && sh.col0 <= sh.col1 && (sh.col1 > sh.col0) == (sh.blk1 > sh.blk0), "shard(%d, %zu, %d): blocks and columns disagree", world, ncol, r);
            CHECK(sh.blk1 - sh.blk0 == nblk / (size_t)world || sh.blk1 - sh.blk0 == (nblk + (size_t)world - 1) / (size_t)world, "shard(%d, %zu, %d) holds %zu blocks", world, ncol, r, sh.blk1 - sh.blk0);
            nxt_blk = sh.blk1; nxt_col = sh.col1; empty += sh.blk1 == sh.blk0;
        }
        CHECK(nxt_blk == nblk && nxt_col == ncol, "world %d, %zu columns: the shards end at block %zu, column %zu", world, ncol, nxt_blk, nxt_col);
        CHECK(empty == ((size_t)world > nblk ? (size_t)world - nblk : 0), "world %d, %zu blocks: %zu empty ranks", world, nblk, empty);
    }
}

// ---------------------------------------------------------------- the contraction plan
static void check_contract(const MgContractIn &in) {
    char name[160];
    snprintf(name, sizeof name, "world %d rank %d s %d L %d nbr_x %d nloc %d %s%s cache %zu/%zu", in.world, in.rank, in.s, in.L, in.nbr_x, in.nloc, in.direct ? "direct " : "", in.tiles ? "tiles" : "rows",
             in.cache_words * 8, in.cache_budget);
    const MgContractPlan p = mg_contract_plan(in);
    const RefContract r = ref_contract(in.world, in.rank, in.s, in.L, in.nbr_x, in.nloc, in.direct, in.tiles, in.cache_words, in.cache_budget);
    // against the reference
    CHECK(p.gpr == r.gpr && p.g_lo == r.g_lo && p.PW == r.PW && p.pipe == r.pipe, "%s: gpr %d g_lo %d PW %d pipe %d", name, p.gpr, p.g_lo, p.PW, (int)p.pipe);
    CHECK(p.outw == r.outw && p.accw == r.accw && p.col == r.col && p.colp == r.colp && p.mine == r.mine, "%s: outw %zu accw %zu col %zu colp %zu mine %zu", name, p.outw, p.accw, p.col, p.colp, p.mine);
    CHECK(p.mine_bytes == r.mine_bytes && p.ar_bytes == r.ar_bytes && p.acc2_bytes == r.acc2_bytes && p.cache_bytes == r.cache_bytes, "%s: bytes mine %zu ar %zu acc2 %zu cache %zu", name,
          p.mine_bytes, p.ar_bytes, p.acc2_bytes, p.cache_bytes);
    CHECK(p.reduce_mine_rows == r.red_mine && p.reduce_out_rows == r.red_out && p.allreduce_words == r.ar_words, "%s: reduce %zu / %zu rows, all-reduce %zu words", name, p.reduce_mine_rows,
          p.reduce_out_rows, p.allreduce_words);
    CHECK(p.steps.size() == r.steps.size() && p.rs.size() == (size_t)in.nbr_x && r.rs.size() == (size_t)in.nbr_x, "%s: %zu steps (reference %zu), %zu columns", name, p.steps.size(), r.steps.size(), p.rs.size());
    if (p.steps.size() != r.steps.size() || p.rs.size() != r.rs.size() || p.steps.empty()) return;
    CHECK(p.steps[0].j == r.first_j0 && p.steps[0].je == r.first_j1, "%s: the first step is columns [%d, %d), prepare() multiplied [%d, %d)", name, p.steps[0].j, p.steps[0].je, r.first_j0, r.first_j1);
    for (size_t k = 0; k < p.steps.size(); k++) {
        const MgStep &a = p.steps[k]; const RefStep &b = r.steps[k];
        CHECK(a.j == b.j && a.je == b.je && a.half == b.ev && a.wait_rs == b.wait && a.multiply == b.mul && p.buf_words(a) == b.buf, "%s: step %zu = {%d, %d, %d, %d, %d} at %zu", name, k, a.j, a.je,
              a.half, (int)a.wait_rs, (int)a.multiply, p.buf_words(a));
    }
    for (size_t k = 0; k < r.rs.size(); k++) {               // the reference's reduce-scatters in the order it issued them: columns 0, 1, 2, ...
        CHECK(r.rs[k].c == (int)k, "%s: the reference's reduce-scatter %zu is column %d", name, k, r.rs[k].c);
        CHECK(p.rs[k].src_words == r.rs[k].src && p.rs[k].dst_words == r.rs[k].dst, "%s: column %zu from %zu to %zu", name, k, p.rs[k].src_words, p.rs[k].dst_words);
    }
    // sizes
    CHECK(in.world * p.gpr >= SFG_D && in.world * p.gpr - SFG_D < in.world, "%s: %d padded giant slots", name, in.world * p.gpr);
    CHECK(p.mine * (size_t)in.world == p.colp && p.colp >= p.col && p.col == (size_t)SFG_D * p.accw, "%s: mine * world = %zu, colp %zu, col %zu", name, p.mine * (size_t)in.world, p.colp, p.col);
    CHECK(p.PW == (in.tiles ? 2 : 1) && (p.pipe || (in.nloc && !in.tiles)), "%s: form", name);
    CHECK((p.ar_bytes != 0) == in.direct && (p.cache_bytes != 0) == (p.pipe && in.nloc && !in.tiles), "%s: which buffers are requested", name);
    CHECK(p.ar_bytes == 0 || p.ar_bytes == p.allreduce_words * 8, "%s: the direct all-reduce's copy holds what is all-reduced", name);
    CHECK(p.reduce_mine_rows * (size_t)in.L * SFG_N * 8 == p.mine_bytes && p.reduce_out_rows * (size_t)in.L * SFG_N == p.allreduce_words, "%s: the reductions cover mg.mine and the output", name);
    // schedule
    std::vector<int> seen((size_t)in.nbr_x, 0);
    const size_t half_words = (size_t)p.PW * p.colp;
    int next = 0;
    for (size_t k = 0; k < p.steps.size(); k++) {
        const MgStep &st = p.steps[k];
        CHECK(st.j == next && st.je > st.j && st.je <= in.nbr_x, "%s: step %zu covers [%d, %d)", name, k, st.j, st.je);
        next = st.je;
        for (int c = st.j; c < st.je; c++) {
            seen[(size_t)c]++;
            const MgRsCol &rc = p.rs[(size_t)c];
            CHECK(rc.dst_words == (size_t)c * p.mine && rc.dst_words + p.mine <= p.mine_bytes / 8, "%s: column %d lands at %zu", name, c, rc.dst_words);
            if (p.pipe) CHECK(rc.src_words >= (size_t)st.half * half_words && rc.src_words + p.mine * (size_t)in.world <= (size_t)(st.half + 1) * half_words, "%s: column %d reads %zu, outside half %d", name, c, rc.src_words, st.half);
            else CHECK(rc.src_words == (size_t)c * p.col && rc.src_words + p.mine * (size_t)in.world <= p.acc2_bytes / 8, "%s: column %d reads %zu of %zu words", name, c, rc.src_words, p.acc2_bytes / 8);
        }
        if (p.pipe) {
            CHECK(st.half == (int)(k & 1) && st.wait_rs == (k >= 2) && st.multiply == (st.j > 0), "%s: step %zu half %d wait %d multiply %d", name, k, st.half, (int)st.wait_rs, (int)st.multiply);
            CHECK(st.je - st.j == p.PW || (k + 1 == p.steps.size() && p.PW == 2 && in.nbr_x % 2 == 1 && st.je - st.j == 1), "%s: step %zu holds %d columns", name, k, st.je - st.j);
            CHECK(p.buf_words(st) + (size_t)(st.je - st.j) * p.colp <= p.acc2_bytes / 8, "%s: step %zu multiplies past mg.acc2", name, k);
        }
    }
    CHECK(next == in.nbr_x, "%s: the steps end at column %d", name, next);
    for (int c = 0; c < in.nbr_x; c++) CHECK(seen[(size_t)c] == 1, "%s: column %d is reduce-scattered %d times", name, c, seen[(size_t)c]);
    if (p.pipe) {
        CHECK(p.acc2_bytes == 2 * half_words * 8 && p.steps.size() == ((size_t)in.nbr_x + (size_t)p.PW - 1) / (size_t)p.PW, "%s: two halves, %zu steps", name, p.steps.size());
        if (p.PW == 2 && in.nbr_x % 2 == 1) CHECK(p.steps.back().je - p.steps.back().j == 1, "%s: the last step is not ragged", name);
    } else {
        CHECK(p.steps.size() == 1 && !p.steps[0].wait_rs && !p.steps[0].multiply && p.steps[0].j == 0 && p.steps[0].je == in.nbr_x && p.buf_words(p.steps[0]) == 0, "%s: the unpipelined form is one step", name);
        CHECK((size_t)(in.nbr_x - 1) * p.col + p.mine * (size_t)in.world == p.acc2_bytes / 8, "%s: the last window ends at %zu of %zu words", name, (size_t)(in.nbr_x - 1) * p.col + p.mine * (size_t)in.world, p.acc2_bytes / 8);
    }
}
static void check_contracts() {
    const size_t jobw = 1000, tailw = 77, big = (size_t)72 << 30;
    for (int world : {1, 2, 3, 4, 8, 14, 24, 64}) for (int nbr_x : {1, 2, 3, 4, 5, 7}) for (int nloc : {0, 1, 3}) for (int s : {1, 2, 15}) for (int L : {1, 5}) {
        const size_t cache_words = (size_t)nloc * s * jobw + tailw;
        for (int rank : {0, world / 2, world - 1}) for (int direct = 0; direct < 2; direct++) {
            if (nloc) check_contract({world, rank, s, L, nbr_x, nloc, direct != 0, true, cache_words, big});            // tiles: PW = 2
            check_contract({world, rank, s, L, nbr_x, nloc, direct != 0, false, cache_words, big});                       // fp64 cache: PW = 1
            check_contract({world, rank, s, L, nbr_x, nloc, direct != 0, false, cache_words, cache_words * 8});           // ... exactly at the budget
            check_contract({world, rank, s, L, nbr_x, nloc, direct != 0, false, cache_words, cache_words * 8 - 1});       // one byte over: unpipelined (pipelined all the same when the rank holds no block)
            check_contract({world, rank, s, L, nbr_x, nloc, direct != 0, false, cache_words, 0});
        }
    }
    // the forms, stated once
    const MgContractPlan t = mg_contract_plan({2, 1, 1, 5, 5, 1, true, true, 1077, big});
    CHECK(t.pipe && t.PW == 2 && t.gpr == 46 && t.g_lo == 46 && t.steps.size() == 3 && t.steps[2].j == 4 && t.steps[2].je == 5 && t.steps[2].half == 0 && t.steps[2].wait_rs, "tiles, 5 columns: three steps, the last ragged and waiting");
    CHECK(t.acc2_bytes == (size_t)2 * 2 * 92 * 2 * 5 * SFG_N * 8 && t.cache_bytes == 0 && t.ar_bytes == (size_t)5 * 2 * 5 * SFG_N * 8, "tiles, 5 columns: %zu bytes of mg.acc2", t.acc2_bytes);
    const MgContractPlan u = mg_contract_plan({2, 0, 1, 5, 5, 1, true, false, 1077, 0});
    CHECK(!u.pipe && u.PW == 1 && u.steps.size() == 1 && u.acc2_bytes == (size_t)(5 * 91 + 1) * 2 * 5 * SFG_N * 8 && u.rs[4].src_words == 4 * u.col, "unpipelined, 5 columns: %zu bytes of mg.acc2", u.acc2_bytes);
    const MgContractPlan e = mg_contract_plan({3, 0, 2, 5, 3, 0, true, false, 77, 0});
    CHECK(e.pipe && e.PW == 1 && e.cache_bytes == 0 && e.steps.size() == 3, "a rank without a block pipelines whatever the budget");
    // a rank that holds padding slots only has the sizes of its peers
    const MgContractPlan a = mg_contract_plan({14, 13, 2, 5, 3, 1, false, true, 2077, big}), b = mg_contract_plan({14, 0, 2, 5, 3, 1, false, true, 2077, big});
    CHECK(a.gpr == 7 && a.g_lo == 91 && a.g_lo >= SFG_D && b.g_lo == 0, "world 14: rank 13 starts at giant slot %d", a.g_lo);
    CHECK(a.mine == b.mine && a.colp == b.colp && a.mine_bytes == b.mine_bytes && a.acc2_bytes == b.acc2_bytes && a.allreduce_words == b.allreduce_words && a.reduce_mine_rows == b.reduce_mine_rows &&
          a.steps.size() == b.steps.size() && a.rs[2].src_words == b.rs[2].src_words && a.rs[2].dst_words == b.rs[2].dst_words, "world 14: rank 13's plan differs from rank 0's in more than g_lo");
}

// ---------------------------------------------------------------- host-form offsets
static void check_slices() {
    for (int world : {1, 2, 3, 8, 14}) for (size_t mct : {(size_t)1, (size_t)3, (size_t)13}) for (size_t ctw : {(size_t)2 * 6 * SFG_N, (size_t)2 * 5 * SFG_N}) for (size_t r : {(size_t)0, (size_t)2}) {
        size_t next = r * mct * ctw;
        for (int rank = 0; rank < world; rank++) {
            const MgShard sh = mg_shard(world, mct * SLOTS - 5, rank);
            const size_t nloc = sh.blk1 - sh.blk0;
            const MgSlice sl = mg_row_slice(r, mct, sh.blk0, nloc, ctw);
            CHECK(sl.host_words == ((size_t)r * mct + sh.blk0) * ctw && sl.dev_words == (size_t)r * nloc * ctw && sl.words == nloc * ctw, "row slice(%zu, %zu, %zu, %zu, %zu)", r, mct, sh.blk0, nloc, ctw);
            CHECK(sl.host_words == next, "world %d, %zu blocks: rank %d's slice of row %zu starts at %zu, its predecessor ended at %zu", world, mct, rank, r, sl.host_words, next);
            CHECK(sl.dev_words + sl.words <= 3 * nloc * ctw, "world %d: rank %d's slice of row %zu leaves its [3][%zu] device grid", world, rank, r, nloc);
            next = sl.host_words + sl.words;
        }
        CHECK(next == (r + 1) * mct * ctw, "world %d, %zu blocks: the slices of row %zu end at %zu", world, mct, r, next);      // [0, mct) of the row, exactly
    }
    const size_t ctw = (size_t)2 * 5 * SFG_N;
    for (size_t cap : {(size_t)1, (size_t)9}) for (size_t r : {(size_t)0, (size_t)2}) for (size_t first = 0; first < cap; first += 4) {
        const size_t count = cap - first;
        const MgSlice sl = mg_assoc_slice(r, cap, first, count, ctw);
        CHECK(sl.host_words == ((size_t)r * cap + first) * ctw && sl.dev_words == ((size_t)r * cap + first) * ctw && sl.words == count * ctw, "assoc slice(%zu, %zu, %zu, %zu)", r, cap, first, count);
        CHECK(sl.host_words + sl.words <= (r + 1) * cap * ctw, "assoc slice(%zu, %zu, %zu, %zu) leaves its row", r, cap, first, count);
    }
}

// ---------------------------------------------------------------- re-shard segments
static void check_reshard(const char *name, int world, const std::vector<RefOld> &shard, const std::vector<uint8_t> &keep, bool want_covered = true) {
    std::vector<unsigned> cols;
    for (size_t j = 0; j < keep.size(); j++) if (keep[j]) cols.push_back((unsigned)j);
    std::vector<std::pair<size_t, size_t>> old(shard.size(), {0, 0});
    for (size_t j = 0; j < shard.size(); j++) if (shard[j].present) old[j] = {shard[j].blk0 * SLOTS, shard[j].blk0 * SLOTS + shard[j].ncol};
    bool all_covered = true;
    for (int rank = 0; rank < world; rank++) {
        const MgShard w = mg_shard(world, cols.size(), rank);
        std::vector<MgSeg> got; std::vector<RefSeg> want;
        const bool ok = mg_reshard_segments(cols.data(), w.col0, w.col1, old, got), rok = ref_segments(cols, w.col0, w.col1, shard, want);
        CHECK(ok == rok, "%s world %d rank %d: covered %d, reference %d", name, world, rank, (int)ok, (int)rok);
        all_covered = all_covered && ok;
        if (!ok || !rok) continue;
        CHECK(got.size() == want.size(), "%s world %d rank %d: %zu segments, reference %zu", name, world, rank, got.size(), want.size());
        for (size_t k = 0; k < got.size() && k < want.size(); k++)
            CHECK((size_t)got[k].old == want[k].j && got[k].gcol0 == want[k].gcol0 && got[k].out0 == want[k].out0, "%s world %d rank %d: segment %zu = {%d, %zu, %zu}", name, world, rank, k, got[k].old, got[k].gcol0, got[k].out0);
        CHECK((w.col1 > w.col0) == !got.empty() && (got.empty() || got[0].out0 == 0), "%s world %d rank %d: the first segment", name, world, rank);
        for (size_t k = 0; k < got.size(); k++) {            // every column of the window lies in the old window of its segment
            const size_t end = k + 1 < got.size() ? got[k + 1].out0 : w.col1 - w.col0;
            CHECK(end > got[k].out0 && got[k].gcol0 == old[(size_t)got[k].old].first, "%s world %d rank %d: segment %zu serves [%zu, %zu)", name, world, rank, k, got[k].out0, end);
            for (size_t x = got[k].out0; x < end; x++) if (cols[w.col0 + x] < old[(size_t)got[k].old].first || cols[w.col0 + x] >= old[(size_t)got[k].old].second) {
                CHECK(false, "%s world %d rank %d: column %u is not in the window of old rank %d", name, world, rank, cols[w.col0 + x], got[k].old); break; }
        }
    }
    CHECK(all_covered == want_covered, "%s world %d: covered %d", name, world, (int)all_covered);
}
static void check_reshards() {
    for (int world : {1, 2, 3, 8}) for (size_t ncol : {9 * SLOTS + 77, 2 * SLOTS - 100}) {          // 10 blocks; 2 blocks (worlds 3 and 8: ranks without a shard)
        std::vector<RefOld> shard;
        for (int r = 0; r < world; r++) { const MgShard sh = mg_shard(world, ncol, r); shard.push_back({sh.col1 > sh.col0, sh.blk0, sh.col1 - sh.col0}); }
        std::vector<uint8_t> all(ncol, 1), odd(ncol, 0), ends(ncol, 0), few(ncol, 0), drop(ncol, 1);
        for (size_t j = 0; j < ncol; j += 2) odd[j] = 1;
        ends[0] = ends[ncol - 1] = 1;
        for (size_t j = 50; j < 150; j++) few[j] = 1;                                                // one block: fewer blocks than ranks from world 2 on
        const MgShard gone = mg_shard(world, ncol, world / 2);                                       // one whole old window dropped (an empty one: nothing dropped)
        for (size_t j = gone.col0; j < gone.col1 && world > 1; j++) drop[j] = 0;
        check_reshard("all", world, shard, all); check_reshard("every other", world, shard, odd); check_reshard("first and last", world, shard, ends);
        check_reshard("few", world, shard, few); check_reshard("window dropped", world, shard, drop);
    }
    // old windows that leave a hole: columns [8192, 16384) belong to nobody
    const std::vector<RefOld> holed = {{true, 0, SLOTS}, {true, 2, 3616}};
    check_reshard("holed", 2, holed, std::vector<uint8_t>(20000, 1), false);
    std::vector<MgSeg> got;
    const std::vector<unsigned> one = {5};
    CHECK(mg_reshard_segments(one.data(), 1, 1, {{0, SLOTS}}, got) && got.empty(), "an empty window is covered by no segment");
}

int main() {
    check_shards();
    check_contracts();
    check_slices();
    check_reshards();
    printf(fails ? "FAILED (%d)\n" : "OK\n", fails);
    return fails ? 1 : 0;
}
