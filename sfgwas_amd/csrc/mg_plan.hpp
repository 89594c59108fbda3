// mg_plan.hpp — the host arithmetic of the multi-GPU engine (mgpu.hip) as pure functions: a rank's SNP-block window, the sizes and the exchange schedule of one
// rank's Q' * X^T, where a rank's slice sits in the host form of a ciphertext grid, and which old windows serve a rank's new window when a filter re-shards.
// Standard library only, so that all of it runs on a CPU (tests/host/host_mgplan_test.cpp).
#pragma once
#include "consts.hpp"
#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

// ---------------------------------------------------------------- the SNP-block shard (sfgwas_amd/sharding.py: snp_block_range)
struct MgShard { size_t blk0, blk1, col0, col1; };         // block columns [blk0, blk1) = columns [col0, col1) of a matrix of ncol columns; empty when world > blocks
inline MgShard mg_shard(int world, size_t ncol, int rank) {
    const size_t nblk = (ncol + SFG_SLOTS - 1) / SFG_SLOTS, b0 = nblk * (size_t)rank / (size_t)world, b1 = nblk * ((size_t)rank + 1) / (size_t)world;
    return {b0, b1, b0 * SFG_SLOTS, std::min(b1 * (size_t)SFG_SLOTS, ncol)};
}

// ---------------------------------------------------------------- one rank's Q' * X^T (rank_contract)
// The canonical accumulators of an output block column are [giant][s][2][L][N] words.  The giant axis is padded from 91 to world * gpr slots and rank r receives
// the sum of slots [r gpr, r gpr + gpr) - `mine` words - of every column, into column c's place of "mg.mine".
// Pipelined (the rank's own rotations fit: as int8 rot tiles, PW = 2 columns per multiply, or as fp64 rows, PW = 1): "mg.acc2" is two halves of PW padded columns;
// step p multiplies columns [j, je) into half p & 1 while the collectives' queue reduce-scatters the other half, and from p = 2 on first waits for the reduce-scatters
// of step p - 2 to have read its half.  The first step's columns are multiplied before the ranks' agreement.
// Unpipelined: "mg.acc2" is the dense [column][91 giants] product plus the padding behind the last column; ONE step after the whole product, and column j's window
// of world * gpr slots starts at j * col and runs into the next column (those slots are ignored by the finalize).
struct MgContractIn {
    int world, rank, s, L, nbr_x, nloc;       // nbr_x: output block columns (block rows of X); nloc: SNP blocks of this rank
    bool direct, tiles;                       // direct transport; the rank's rotations are held as int8 rot tiles (I8RotPre::G != 0)
    size_t cache_words, cache_budget;         // words of the rank's fp64 rotation cache (nloc * s * jobw + tailw of sfg_rotcache_layout); bytes it may take
};
struct MgStep { int j, je, half; bool wait_rs, multiply; };
struct MgRsCol { size_t src_words, dst_words; };           // reduce-scatter of one output column: from "mg.acc2" + src_words into "mg.mine" + dst_words, `mine` words
struct MgContractPlan {
    int gpr = 0, g_lo = 0, PW = 1;            // giant slots per rank, this rank's first one (>= 91: padding only), columns per multiply call
    bool pipe = false;
    size_t outw = 0, accw = 0, col = 0, colp = 0, mine = 0;      // words of: an output ciphertext, s of them (one giant slot), 91 slots, world * gpr slots, gpr slots
    size_t mine_bytes = 0, ar_bytes = 0, acc2_bytes = 0, cache_bytes = 0;      // scratch requests; ar: direct transport only, cache: the fp64 pipelined form only, else 0
    size_t reduce_mine_rows = 0, reduce_out_rows = 0, allreduce_words = 0;     // rows of L moduli reduced after the reduce-scatters / after the all-reduce; its words
    std::vector<MgStep> steps;
    std::vector<MgRsCol> rs;                  // [nbr_x]
    size_t buf_words(const MgStep &st) const { return (size_t)st.half * PW * colp; }      // where step st multiplies, from "mg.acc2"
};
inline MgContractPlan mg_contract_plan(const MgContractIn &in) {
    MgContractPlan p;
    const size_t d = SFG_D, world = (size_t)in.world, s = (size_t)in.s, nbr_x = (size_t)in.nbr_x;
    p.outw = (size_t)2 * in.L * SFG_N; p.accw = s * p.outw;
    p.gpr = (SFG_D + in.world - 1) / in.world; p.g_lo = in.rank * p.gpr;
    p.col = d * p.accw; p.colp = world * p.gpr * p.accw; p.mine = (size_t)p.gpr * p.accw;
    p.pipe = !in.nloc || in.tiles || in.cache_words * 8 <= in.cache_budget;
    p.PW = p.pipe && in.tiles ? 2 : 1;
    p.mine_bytes = nbr_x * p.mine * 8;
    p.ar_bytes = in.direct ? s * nbr_x * p.outw * 8 : 0;
    p.acc2_bytes = p.pipe ? (size_t)2 * p.PW * p.colp * 8 : (nbr_x * d + (world * p.gpr - d)) * p.accw * 8;
    p.cache_bytes = p.pipe && in.nloc && !in.tiles ? in.cache_words * 8 : 0;
    p.reduce_mine_rows = nbr_x * p.gpr * s * 2; p.reduce_out_rows = s * nbr_x * 2; p.allreduce_words = s * nbr_x * p.outw;
    p.rs.resize(nbr_x);
    if (p.pipe) {
        for (int j = 0, n = 0; j < in.nbr_x; j += p.PW, n++) {
            const MgStep st = {j, std::min(in.nbr_x, j + p.PW), n & 1, n >= 2, j > 0};
            for (int c = st.j; c < st.je; c++) p.rs[(size_t)c] = {p.buf_words(st) + (size_t)(c - j) * p.colp, (size_t)c * p.mine};
            p.steps.push_back(st);
        }
    } else {
        p.steps.push_back({0, in.nbr_x, 0, false, false});
        for (size_t j = 0; j < nbr_x; j++) p.rs[j] = {j * p.col, j * p.mine};
    }
    return p;
}

// ---------------------------------------------------------------- host-form offsets (sfg_mgpu_matmul, mgpu_assoc)
// Row r of a host grid [s][mct] of ciphertexts of ctw words, and the rank's blocks [blk0, blk0 + nloc) of it, which the rank holds densely as [s][nloc]: the
// inputs of Q' * X^T and the outputs of Q * X
struct MgSlice { size_t host_words, dev_words, words; };
inline MgSlice mg_row_slice(size_t r, size_t mct, size_t blk0, size_t nloc, size_t ctw) { return {(r * mct + blk0) * ctw, r * nloc * ctw, nloc * ctw}; }
// The association scan keeps the host's layout [s][capacity] on the device: the `count` output ciphertexts from `first` on of row r, at the same offset on both sides
inline MgSlice mg_assoc_slice(size_t r, size_t capacity, size_t first, size_t count, size_t ctw) { return {(r * capacity + first) * ctw, (r * capacity + first) * ctw, count * ctw}; }

// ---------------------------------------------------------------- re-shard segments (sfg_mgpu_geno_filter)
// cols: the kept global columns, increasing.  A rank's new window is cols[c0, c1); old[j] = the global columns [first, second) that old local rank j holds (empty:
// it holds none).  Kept columns stay in order, so the window draws on a run of old windows: segment {old rank, global column of its first stored column, first
// output column of the window it serves}, listed only where it serves at least one column.  false: the old windows do not cover the window.
struct MgSeg { int old; size_t gcol0, out0; };
inline bool mg_reshard_segments(const unsigned *cols, size_t c0, size_t c1, const std::vector<std::pair<size_t, size_t>> &old, std::vector<MgSeg> &segs) {
    segs.clear();
    size_t served = 0;
    const unsigned *wb = cols + c0, *we = cols + c1;
    for (size_t j = 0; j < old.size() && c1 > c0; j++) {
        const size_t lo = (size_t)(std::lower_bound(wb, we, old[j].first) - wb), hi = (size_t)(std::lower_bound(wb, we, old[j].second) - wb);
        if (hi == lo) continue;
        if (lo != served) break;                           // (the old windows leave a hole)
        segs.push_back({(int)j, old[j].first, lo});
        served = hi;
    }
    return served == c1 - c0;
}
