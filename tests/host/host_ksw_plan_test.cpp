// host_ksw_plan_test.cpp — the key switch's job planning (sfgwas_amd/csrc/ksw_plan.hpp) on the CPU: the header rotate.hip includes, compiled for the host
// (with AddressSanitizer + UBSan where the runtimes exist) as a plain executable.  It reads a script (tests/test_ksw_plan.py writes it), one call per line, and
// prints what the planner returns; the Python side holds every line against a literal restatement.  The invariants a kernel relies on - every job in exactly one
// tile, a tile within one key and one table, every job of a chunk in exactly one segment and in chunk order, every job in the group of its input, the regions of
// the workspace apart and aligned - are checked here as well, on every line.
//   R nout                         forget which outputs of a sum have been written            -> "R"
//   J T nb (key tab){nb}           ksw_job_tiles                                              -> "J ntiles (start count){ntiles}"
//   C nb (group){nb}               ksw_plan_segments for one chunk                            -> "C nseg (out start count first){nseg} | segjobs{nb}"
//   S nl np nt beta nin nr nout budget N      ksw_plan_sizes; checked here: the thirteen regions in order, aligned, not overlapping, inside the total, the total in closed form
//                                  -> "S in_grp chunk ext_rows ext2_rows acc_rows | c2 ext acc ext2 extT ext2T (words) | keys idx out segs inidx segjobs tiles (bytes) | bytes"
//   G T in_grp chunk nin nr (in key tab){nr}  ksw_plan_groups; checked here: every job in the one group of its input, list order, chunks partition, tiles as in J and
//                                  no more per group than jobs   -> "G ngroups { | i0 ni nj job{nj} ; nchunks { , c0 nb ntiles (start count){ntiles}}}"
//   P q w U V                    fp64mod.hpp inv_last_pair for N = 2^14 with the constants as the kernels form them (ctx.hip ModConst, rotate.hip inv_last_of);
//                                  w: the last inverse stage's twiddle                        -> "P r0 r1 want0 want1" (want: 128-bit integers)
#include "fp64mod.hpp"
#include "ksw_plan.hpp"

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>

static void fail(const char *what, size_t line) {
    std::fprintf(stderr, "line %zu: %s\n", line, what);
    std::exit(1);
}

int main(int argc, char **argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: %s script\n", argv[0]); return 2; }
    std::ifstream f(argv[1]);
    if (!f) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    std::string line; size_t ln = 0;
    std::vector<char> seen; int nout = 0;
    while (std::getline(f, line)) {
        ln++;
        std::istringstream is(line);
        char op; is >> op;
        if (op == 'R') {
            is >> nout;
            if (!is || nout < 0) fail("bad R", ln);
            seen.assign((size_t)nout, 0);
            std::cout << "R\n";
        } else if (op == 'J') {
            int T, nb; is >> T >> nb;
            if (!is || nb < 0) fail("bad J", ln);
            std::vector<long> key((size_t)nb), tab((size_t)nb);
            for (int k = 0; k < nb; k++) is >> key[(size_t)k] >> tab[(size_t)k];
            if (!is) fail("short J", ln);
            std::vector<KswTile> tiles;
            ksw_job_tiles(key.data(), tab.data(), nb, T, tiles);
            int next = 0;
            for (const KswTile &t : tiles) {
                if (t.start != next || t.count < 1 || t.count > (T < 1 ? 1 : T)) fail("tiles do not cover the jobs in order", ln);
                for (int j = 1; j < t.count; j++)
                    if (key[(size_t)(t.start + j)] != key[(size_t)t.start] || tab[(size_t)(t.start + j)] != tab[(size_t)t.start]) fail("tile spans two keys or tables", ln);
                next += t.count;
            }
            if (next != nb) fail("tiles do not cover the jobs", ln);
            std::cout << "J " << tiles.size();
            for (const KswTile &t : tiles) std::cout << ' ' << t.start << ' ' << t.count;
            std::cout << '\n';
        } else if (op == 'C') {
            int nb; is >> nb;
            if (!is || nb < 0) fail("bad C", ln);
            std::vector<int> group((size_t)nb);
            for (int k = 0; k < nb; k++) {
                is >> group[(size_t)k];
                if (!is || group[(size_t)k] < 0 || group[(size_t)k] >= nout) fail("group out of range", ln);
            }
            std::vector<KswSegPlan> segs; std::vector<int> segjobs;
            ksw_plan_segments(group.data(), nb, nout, seen, segs, segjobs);
            std::vector<int> hit((size_t)nb, 0);
            int at = 0;
            for (const KswSegPlan &s : segs) {
                if (s.start != at || s.count < 0 || s.out < 0 || s.out >= nout) fail("segments are not laid end to end", ln);
                for (int k = 0; k < s.count; k++) {
                    const int j = segjobs[(size_t)(s.start + k)];
                    if (j < 0 || j >= nb || group[(size_t)j] != s.out || hit[(size_t)j]++) fail("a segment holds a job that is not its own", ln);
                    if (k && segjobs[(size_t)(s.start + k - 1)] >= j) fail("a segment's jobs are out of chunk order", ln);
                }
                at += s.count;
            }
            if (at != nb) fail("segments do not cover the chunk", ln);
            std::cout << "C " << segs.size();
            for (const KswSegPlan &s : segs) std::cout << ' ' << s.out << ' ' << s.start << ' ' << s.count << ' ' << s.first;
            std::cout << " |";
            for (int j : segjobs) std::cout << ' ' << j;
            std::cout << '\n';
        } else if (op == 'S') {
            long long nl, np, nt, beta, nin, nr, no, budget, N; is >> nl >> np >> nt >> beta >> nin >> nr >> no >> budget >> N;
            if (!is || nl < 1 || np < 1 || nt < 1 || beta < 1 || nin < 0 || nr < 0 || no < 0 || budget < 0 || N < 1) fail("bad S", ln);
            const KswSizes s = ksw_plan_sizes((int)nl, (int)np, (int)nt, (int)beta, (int)nin, (int)nr, (int)no, (size_t)budget, (size_t)N);
            const KswLayout &a = s.at;
            const size_t w = 8, n = (size_t)N, r = (size_t)nr;
            // the thirteen regions in bytes: start, size, alignment of the element
            const size_t reg[13][3] = {{a.c2 * w, (size_t)s.in_grp * nl * n * w, n * w}, {a.ext * w, s.ext_rows * n * w, n * w}, {a.acc * w, s.acc_rows * n * w, n * w},
                                       {a.ext2 * w, s.ext2_rows * n * w, n * w}, {a.extT * w, s.ext_rows * n * w, n * w}, {a.ext2T * w, s.ext2_rows * n * w, n * w},
                                       {a.keys, r * 8, 8}, {a.idx, r * 8, 8}, {a.out, r * 8, 8}, {a.segs, (size_t)no * 32, 8}, {a.inidx, r * 4, 4}, {a.segjobs, r * 4, 4},
                                       {a.tiles, r * sizeof(KswTile), alignof(KswTile)}};
            for (int k = 0; k < 13; k++) {
                if (reg[k][0] % reg[k][2]) fail("a region is misaligned", ln);
                if (reg[k][0] + reg[k][1] > (k < 12 ? reg[k + 1][0] : a.bytes)) fail("a region overlaps the next or passes the end", ln);
            }
            if (a.c2 != 0) fail("the workspace does not start with c2", ln);
            if (s.in_grp < 0 || s.in_grp > nin || s.chunk < 0 || s.chunk > nr || (nin && s.in_grp < 1) || (nr && s.chunk < 1)) fail("group or chunk size out of range", ln);
            if (s.ext_rows != (size_t)s.in_grp * beta * nt || s.ext2_rows != (size_t)s.chunk * 2 * nl || s.acc_rows != (size_t)s.chunk * 2 * np) fail("row counts", ln);
            const size_t in_rows = (size_t)nl + (size_t)beta * nt;
            if (a.bytes != (in_rows * s.in_grp + s.acc_rows + 2 * s.ext2_rows + s.ext_rows) * n * 8 + r * (3 * 8 + 2 * 4 + 8) + (size_t)no * 32 + 256) fail("total differs from the closed form", ln);
            std::cout << "S " << s.in_grp << ' ' << s.chunk << ' ' << s.ext_rows << ' ' << s.ext2_rows << ' ' << s.acc_rows << " | " << a.c2 << ' ' << a.ext << ' ' << a.acc << ' '
                      << a.ext2 << ' ' << a.extT << ' ' << a.ext2T << " | " << a.keys << ' ' << a.idx << ' ' << a.out << ' ' << a.segs << ' ' << a.inidx << ' ' << a.segjobs << ' '
                      << a.tiles << " | " << a.bytes << '\n';
        } else if (op == 'G') {
            int T, in_grp, chunk, nin, nr; is >> T >> in_grp >> chunk >> nin >> nr;
            if (!is || nin < 0 || nr < 0 || in_grp < 0 || chunk < 0) fail("bad G", ln);
            std::vector<int> in((size_t)nr); std::vector<long> key((size_t)nr), tab((size_t)nr);
            for (int k = 0; k < nr; k++) {
                is >> in[(size_t)k] >> key[(size_t)k] >> tab[(size_t)k];
                if (!is || in[(size_t)k] < 0 || in[(size_t)k] >= nin) fail("short G or input out of range", ln);
            }
            std::vector<KswGroup> groups;
            ksw_plan_groups(in.data(), key.data(), tab.data(), nr, nin, in_grp, chunk, T, groups);
            std::vector<int> hit((size_t)nr, 0);
            int last_i0 = -1;
            for (const KswGroup &g : groups) {
                if (g.i0 <= last_i0 || g.i0 % in_grp || g.i0 >= nin || g.ni != (nin - g.i0 < in_grp ? nin - g.i0 : in_grp)) fail("a group's inputs", ln);
                last_i0 = g.i0;
                if (g.jobs.empty()) fail("a group without a job", ln);
                for (size_t k = 0; k < g.jobs.size(); k++) {
                    const int j = g.jobs[k];
                    if (j < 0 || j >= nr || in[(size_t)j] < g.i0 || in[(size_t)j] >= g.i0 + g.ni || hit[(size_t)j]++) fail("a group holds a job that is not its own", ln);
                    if (k && g.jobs[k - 1] >= j) fail("a group's jobs are out of list order", ln);
                }
                if (g.tiles.size() > g.jobs.size()) fail("more tiles than the layout has room for", ln);
                int at = 0, tat = 0;
                for (const KswChunk &c : g.chunks) {
                    if (c.c0 != at || c.nb < 1 || c.nb > chunk || c.tile0 != tat || c.ntiles < 1 || (size_t)(c.tile0 + c.ntiles) > g.tiles.size()) fail("chunks do not partition the group", ln);
                    int next = 0;
                    for (int i = 0; i < c.ntiles; i++) {                      // what the J lines check, on chunk-local numbers
                        const KswTile &t = g.tiles[(size_t)(c.tile0 + i)];
                        if (t.start != next || t.count < 1 || t.count > (T < 1 ? 1 : T)) fail("tiles do not cover the chunk in order", ln);
                        const int j0 = g.jobs[(size_t)(c.c0 + t.start)];
                        for (int j = 1; j < t.count; j++) {
                            const int jj = g.jobs[(size_t)(c.c0 + t.start + j)];
                            if (key[(size_t)jj] != key[(size_t)j0] || tab[(size_t)jj] != tab[(size_t)j0]) fail("tile spans two keys or tables", ln);
                        }
                        next += t.count;
                    }
                    if (next != c.nb) fail("tiles do not cover the chunk", ln);
                    at += c.nb; tat += c.ntiles;
                }
                if (at != (int)g.jobs.size() || tat != (int)g.tiles.size()) fail("chunks do not cover the group", ln);
            }
            for (int k = 0; k < nr; k++) if (!hit[(size_t)k] && in_grp > 0 && chunk > 0) fail("a job is in no group", ln);
            std::cout << "G " << groups.size();
            for (const KswGroup &g : groups) {
                std::cout << " | " << g.i0 << ' ' << g.ni << ' ' << g.jobs.size();
                for (int j : g.jobs) std::cout << ' ' << j;
                std::cout << " ; " << g.chunks.size();
                for (const KswChunk &c : g.chunks) {
                    std::cout << " , " << c.c0 << ' ' << c.nb << ' ' << c.ntiles;
                    for (int i = 0; i < c.ntiles; i++) std::cout << ' ' << g.tiles[(size_t)(c.tile0 + i)].start << ' ' << g.tiles[(size_t)(c.tile0 + i)].count;
                }
            }
            std::cout << '\n';
        } else if (op == 'P') {
            unsigned long long q, w, U, V; is >> q >> w >> U >> V;
            if (!is || q < 3 || w >= q || U >= q || V >= q) fail("bad P", ln);
            typedef unsigned __int128 u128;
            unsigned long long ninv = 1;                                  // N^-1 = ((q + 1) / 2)^14 mod q
            for (int k = 0; k < 14; k++) ninv = (unsigned long long)((u128)ninv * ((q + 1) / 2) % q);
            const double qd = (double)q, qinv = 1.0 / qd, nd = (double)ninv, nq = nd / qd;
            const double wn = canon(mulmod_lazy((double)w, nd, nq, qd), qd, qinv);
            double r0, r1;
            inv_last_pair((double)U, (double)V, nd, nq, wn, wn * qinv, qd, qinv, r0, r1);
            const unsigned long long w0 = (unsigned long long)((u128)((U + V) % q) * ninv % q);
            const unsigned long long w1 = (unsigned long long)((u128)((U + q - V) % q) * (unsigned long long)((u128)w * ninv % q) % q);
            if (r0 < 0 || r1 < 0 || r0 >= qd || r1 >= qd || (unsigned long long)r0 != w0 || (unsigned long long)r1 != w1) fail("inv_last_pair differs from the integers", ln);
            std::cout << "P " << (unsigned long long)r0 << ' ' << (unsigned long long)r1 << ' ' << w0 << ' ' << w1 << '\n';
        } else fail("unknown line", ln);
    }
    std::cout << "OK\n";
    return 0;
}
