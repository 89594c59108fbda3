// host_gring_mm_test.cpp - sfgwas_amd/csrc/gring_matmul_plan.hpp on the CPU: the shift tables, the rotation list, the fold bound and the folded sum, the workspace
// layout and the chunk plans, printed for tests/test_ring_mm_plan.py to compare with its Python restatements.  One command per line of the script given as argv[1]:
//   S rows cols slots bi                      -> "S" baby giant shift (strings of 0 / 1) and nr
//   R rows cols slots b0 b1 babies giants     -> "R" the left rotations
//   F q                                       -> "F" fold_terms(q)
//   A q fold n                                -> "A" the folded sum of n terms a_k b_k, a_k = q - 1 - k % 5, b_k = q - 1 - k % 3, folding every `fold` terms
//   L d nl L m_ct N sc vc with_acc            -> "L" the twelve offsets of the layout
//   P s d nl L m_ct N with_acc budget nd      -> "P" sc nsc vc bytes, then "c" first count per chunk of s, then "b" first count per batch of nd diagonals
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include "gring_matmul_plan.hpp"

static std::string bits(const std::vector<uint8_t> &v) { std::string s; for (uint8_t b : v) s += b ? '1' : '0'; return s; }

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s script\n", argv[0]); return 2; }
    std::ifstream in(argv[1]);
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream ss(line);
        char cmd; ss >> cmd;
        if (cmd == 'S') {
            size_t rows, cols; int slots, bi; ss >> rows >> cols >> slots >> bi;
            const MmShifts t = mm_shifts(rows, cols, slots, bi);
            printf("S %s %s %s %d %d\n", bits(t.baby).c_str(), bits(t.giant).c_str(), bits(t.shift).c_str(), t.nr, t.d);
        } else if (cmd == 'R') {
            size_t rows, cols; int slots, b0, b1, bb, gg; ss >> rows >> cols >> slots >> b0 >> b1 >> bb >> gg;
            printf("R");
            for (int k : mm_rotations(rows, cols, slots, b0, b1, bb != 0, gg != 0)) printf(" %d", k);
            printf("\n");
        } else if (cmd == 'F') {
            unsigned long long q; ss >> q;
            printf("F %llu\n", (unsigned long long)mm_fold_terms(q));
        } else if (cmd == 'A') {
            unsigned long long q, fold, n; ss >> q >> fold >> n;
            const gr::u128 u = ~(gr::u128)0 / q;
            const gr::u64 w = mm_sum_terms((size_t)n, fold, [&](size_t k) { return q - 1 - k % 5; }, [&](size_t k) { return q - 1 - k % 3; }, q, (gr::u64)(u >> 64), (gr::u64)u);
            printf("A %llu\n", w);
        } else if (cmd == 'L') {
            int d, nl, L, m_ct, with_acc; size_t N, sc, vc; ss >> d >> nl >> L >> m_ct >> N >> sc >> vc >> with_acc;
            const MmLayout l = mm_layout(d, nl, L, m_ct, N, sc, vc, with_acc != 0);
            printf("L %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", l.rot, l.acc, l.dft, l.pt, l.vecs, l.first, l.jobs, l.glist, l.sums, l.band, l.flags, l.end);
        } else if (cmd == 'P') {
            size_t s, N, budget, nd; int d, nl, L, m_ct, with_acc; ss >> s >> d >> nl >> L >> m_ct >> N >> with_acc >> budget >> nd;
            const MmPlan p = mm_plan(s, d, nl, L, m_ct, N, with_acc != 0, budget);
            printf("P %zu %zu %zu %zu\n", p.sc, p.nsc, p.vc, p.bytes);
            for (size_t c = 0; c < p.nsc; c++) printf("c %zu %zu\n", p.first(c), p.count(c, s));
            for (size_t b = 0; b < p.nbatches(nd); b++) printf("b %zu %zu\n", p.bfirst(b), p.bcount(b, nd));
        } else if (cmd == 'D') {
            int slots; ss >> slots;
            printf("D %d\n", mm_d(slots));
        }
    }
    printf("OK\n");
    return 0;
}
