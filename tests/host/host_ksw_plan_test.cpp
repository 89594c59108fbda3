// host_ksw_plan_test.cpp — the key switch's job planning (sfgwas_amd/csrc/ksw_plan.hpp) on the CPU: the header rotate.hip includes, compiled for the host
// (with AddressSanitizer + UBSan where the runtimes exist) as a plain executable.  It reads a script (tests/test_ksw_plan.py writes it), one call per line, and
// prints what the planner returns; the Python side holds every line against a literal restatement.  The invariants a kernel relies on - every job in exactly one
// tile, a tile within one key and one table, every job of a chunk in exactly one segment and in chunk order - are checked here as well, on every line.
//   R nout                         forget which outputs of a sum have been written            -> "R"
//   J T nb (key tab){nb}           ksw_job_tiles                                              -> "J ntiles (start count){ntiles}"
//   C nb (group){nb}               ksw_plan_segments for one chunk                            -> "C nseg (out start count first){nseg} | segjobs{nb}"
//   P q w U V                      fp64mod.hpp inv_last_pair for N = 2^14 with the constants as the kernels form them (ctx.hip ModConst, rotate.hip inv_last_of);
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
