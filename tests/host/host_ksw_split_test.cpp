// The helper of the key switch's split forward transform (sfgwas_amd/csrc/fp64mod.hpp fwd_stage1_pair) and the fp64-held modular primitives it is built
// from, on the CPU: the very functions the kernels run, against a literal restatement with 128-bit integers.  Stand-alone: includes the one header, links
// nothing of the library.  tests/test_ksw_split.py writes the script and compares every printed word with Python integers as well.
//   S q W v0 v1      the pair (v0, v1) of positions x, x + N/2 through stage 1 with the twiddle W: r0 = v0 + W v1, r1 = v0 - W v1 mod q, as the
//                    function gives them and as 128-bit integers give them
//   C q x            canon(x) for the signed integer x, |x| < 2^51, and x mod q
#include "fp64mod.hpp"
#include <cinttypes>
#include <cstdio>
#include <cstring>

typedef unsigned long long u64;
typedef __int128 i128;

static u64 mod128(i128 x, u64 q) { i128 r = x % (i128)q; if (r < 0) r += (i128)q; return (u64)r; }

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: host_ksw_split_test SCRIPT\n"); return 2; }
    FILE *f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 2; }
    char op[8]; int bad = 0;
    while (fscanf(f, "%7s", op) == 1) {
        if (!strcmp(op, "S")) {
            u64 q, W, v0, v1; if (fscanf(f, "%llu %llu %llu %llu", &q, &W, &v0, &v1) != 4 || v0 >= q || v1 >= q || W >= q) return 3;
            const double qd = (double)q, qinv = 1.0 / qd, Wd = (double)W;
            double r0, r1;
            fwd_stage1_pair((double)v0, (double)v1, Wd, Wd * qinv, qd, qinv, r0, r1);
            const u64 w0 = mod128((i128)v0 + (i128)W * v1, q), w1 = mod128((i128)v0 - (i128)W * v1, q);
            if (r0 != (double)w0 || r1 != (double)w1) bad++;
            printf("S %llu %llu %llu %llu %.0f %.0f %llu %llu\n", q, W, v0, v1, r0, r1, w0, w1);
        } else if (!strcmp(op, "C")) {
            u64 q; long long x; if (fscanf(f, "%llu %lld", &q, &x) != 2) return 3;
            const double qd = (double)q, r = canon((double)x, qd, 1.0 / qd);
            const u64 w = mod128((i128)x, q);
            if (r != (double)w) bad++;
            printf("C %llu %lld %.0f %llu\n", q, x, r, w);
        } else return 3;
    }
    fclose(f);
    printf("%s\n", bad ? "MISMATCH" : "OK");
    return bad ? 1 : 0;
}
