// host_gring_tie_test.cpp - sfgwas_amd/csrc/gring_tie.hpp on the CPU: the cosine table's builder, the fold, the multi-word sum and the decision function the
// resolver kernel (gring_matmul.hip: k_gr_mm_tie) runs, printed for tests/test_ring_tie_ref.py to compare with Python integers, mpmath and tests/exactref.py.
// One command per line of the script given as argv[1]; every number that is not a count is hexadecimal:
//   T logN                                   -> one line per table entry k = 0 .. N / 2: its value as one hexadecimal integer
//   F N a                                    -> "F" index neg
//   D x3 x2 x1 x0 m e logn A                 -> "D" status p          (x3 .. x0: the sum's words, most significant first; e, logn decimal and signed)
//   C logN j scalebits k t_1 v_1 .. t_k v_k  -> "C" status p          (the coefficient j of the vector with v_t at slot t, zero elsewhere; scalebits: the double's bits)
//   U logN j scalebits v                     -> "U" status p          (every slot holds v)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <sstream>
#include <string>
#include "gring_tie.hpp"

static const std::vector<gr::u64> &table(int logN) {
    static std::map<int, std::vector<gr::u64>> tabs;
    auto it = tabs.find(logN);
    if (it == tabs.end()) it = tabs.emplace(logN, gtie::build_table(logN)).first;
    return it->second;
}
static double from_bits(unsigned long long b) { double d; memcpy(&d, &b, 8); return d; }

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s script\n", argv[0]); return 2; }
    std::ifstream in(argv[1]);
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream ss(line);
        char cmd; ss >> cmd;
        if (cmd == 'T') {
            int logN; ss >> logN;
            const std::vector<gr::u64> &t = table(logN);
            for (size_t k = 0; k * gtie::kWords < t.size(); k++) printf("%llx%016llx%016llx\n", t[k * 3 + 2], t[k * 3 + 1], t[k * 3]);
        } else if (cmd == 'F') {
            unsigned N, a; ss >> N >> a;
            bool neg; const unsigned k = gtie::fold(a, N, neg);
            printf("F %u %d\n", k, (int)neg);
        } else if (cmd == 'D') {
            gr::u64 X[4], m, A; int e, logn;
            ss >> std::hex >> X[3] >> X[2] >> X[1] >> X[0] >> m >> std::dec >> e >> logn >> std::hex >> A;
            long long p; const int st = gtie::decide(X, m, e, logn, A, p);
            printf("D %d %lld\n", st, p);
        } else if (cmd == 'C' || cmd == 'U') {
            int logN; unsigned j; unsigned long long sb; ss >> logN >> j >> std::hex >> sb >> std::dec;
            std::vector<int> v((size_t)1 << (logN - 1), 0);
            if (cmd == 'C') { int k; ss >> k; for (int i = 0; i < k; i++) { size_t t; int x; ss >> t >> x; if (t >= v.size()) { fprintf(stderr, "slot out of range\n"); return 2; } v[t] = x; } }
            else { int x; ss >> x; for (int &y : v) y = x; }
            long long p; const int st = gtie::coefficient(table(logN), logN, v.data(), j, from_bits(sb), p);
            printf("%c %d %lld\n", cmd, st, p);
        } else if (!line.empty()) { fprintf(stderr, "unknown command: %s\n", line.c_str()); return 2; }
        if (ss.fail()) { fprintf(stderr, "bad line: %s\n", line.c_str()); return 2; }
    }
    printf("OK\n");
    return 0;
}
