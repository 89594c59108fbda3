// The per-element arithmetic of the general ring's key generation (sfgwas_amd/csrc/gring_keygen_arith.hpp) and its host planner (gring_keygen_plan.hpp) on the CPU:
// the very functions the kernels of gring_keygen.hip run, on the operands a script names.  Stand-alone: includes the two headers, links nothing of the library.
// tests/test_ring_keygen_ref.py writes the script, compares every printed word with Python integers and checks that planted mistakes change the output.
//   S eh a b s with_g pg q                the share epilogue eh - a b (+ pg s) modulo q
//   H eh a s q                            round 1's h1: eh + s a
//   R eh h0 h1 s uh q                     round 2: eh + s h0 + (uh - s) h1
//   LS a b q                              lift(a) + lift(b) modulo q of two int32
//   G digit m nq np                       whether g_i applies to modulus m
//   I g logN                              the index table a rotation share for g reads sk through (N entries on one line)
//   J g logN                              the index table of g itself (what installation stores)
//   M q                                   the common reference map's mask
//   K q w0 .. w15                         the first candidate of a block below q: found, value
//   P nkeys beta nmod N budget with_u     the plan: chunk, chunks, index bytes, the Galois list's offset, u bytes, then first and count of every chunk
#include "gring_keygen_arith.hpp"
#include "gring_keygen_plan.hpp"
#include <cinttypes>
#include <cstdio>
#include <cstring>

using gr::u64;
using gr::u128;

struct Mod { u64 q, uhi, ulo; };
static Mod mod_of(u64 q) { const u128 u = ~(u128)0 / q; return Mod{q, (u64)(u >> 64), (u64)u}; }      // floor((2^128 - 1) / q) = floor(2^128 / q): q is odd
static u64 shoup_of(u64 w, u64 q) { return (u64)(((u128)w << 64) / q); }

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: host_gring_keygen_test SCRIPT\n"); return 2; }
    FILE *f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 2; }
    char op[8];
    while (fscanf(f, "%7s", op) == 1) {
        if (!strcmp(op, "S")) {
            u64 eh, a, b, s, pg, q; int wg;
            if (fscanf(f, "%llu %llu %llu %llu %d %llu %llu", &eh, &a, &b, &s, &wg, &pg, &q) != 7) return 3;
            const Mod m = mod_of(q);
            printf("S %llu %llu %llu %llu %d %llu %llu %llu\n", eh, a, b, s, wg, pg, q, gkg::share(eh, a, b, s, wg != 0, pg, shoup_of(pg, q), q, m.uhi, m.ulo));
        } else if (!strcmp(op, "H")) {
            u64 eh, a, s, q; if (fscanf(f, "%llu %llu %llu %llu", &eh, &a, &s, &q) != 4) return 3;
            const Mod m = mod_of(q);
            printf("H %llu %llu %llu %llu %llu\n", eh, a, s, q, gkg::round1_h1(eh, a, s, q, m.uhi, m.ulo));
        } else if (!strcmp(op, "R")) {
            u64 eh, h0, h1, s, uh, q; if (fscanf(f, "%llu %llu %llu %llu %llu %llu", &eh, &h0, &h1, &s, &uh, &q) != 6) return 3;
            const Mod m = mod_of(q);
            printf("R %llu %llu %llu %llu %llu %llu %llu\n", eh, h0, h1, s, uh, q, gkg::round2(eh, h0, h1, s, uh, q, m.uhi, m.ulo));
        } else if (!strcmp(op, "LS")) {
            long long a, b; u64 q; if (fscanf(f, "%lld %lld %llu", &a, &b, &q) != 3) return 3;
            printf("LS %lld %lld %llu %llu\n", a, b, q, gkg::lift_sum((int32_t)a, (int32_t)b, q));
        } else if (!strcmp(op, "G")) {
            int d, m, nq, np; if (fscanf(f, "%d %d %d %d", &d, &m, &nq, &np) != 4) return 3;
            printf("G %d %d %d %d %d\n", d, m, nq, np, gkg::g_applies(d, m, nq, np) ? 1 : 0);
        } else if (!strcmp(op, "I") || !strcmp(op, "J")) {
            u64 g; int logN; if (fscanf(f, "%llu %d", &g, &logN) != 2 || logN < 1 || logN > 16) return 3;
            const u64 ge = op[0] == 'I' ? gkg::share_galois(g, logN) : g;
            printf("%s %llu %d", op, g, logN);
            for (int i = 0; i < (1 << logN); i++) printf(" %u", gkg::index_entry(ge, i, logN));
            printf("\n");
        } else if (!strcmp(op, "M")) {
            u64 q; if (fscanf(f, "%llu", &q) != 1 || q < 3) return 3;
            printf("M %llu %llu\n", q, gkg::crp_mask(q));
        } else if (!strcmp(op, "K")) {
            u64 q; unsigned w[16]; if (fscanf(f, "%llu", &q) != 1) return 3;
            for (int i = 0; i < 16; i++) if (fscanf(f, "%u", &w[i]) != 1) return 3;
            u64 val = 0; const bool found = gkg::crp_pick(w, q, gkg::crp_mask(q), val);
            printf("K %llu %d %llu\n", q, found ? 1 : 0, found ? val : 0ULL);
        } else if (!strcmp(op, "P")) {
            size_t nkeys, N, budget; int beta, nmod, with_u;
            if (fscanf(f, "%zu %d %d %zu %zu %d", &nkeys, &beta, &nmod, &N, &budget, &with_u) != 6) return 3;
            const GrkPlan p = grk_plan(nkeys, beta, nmod, N, with_u != 0, budget);
            printf("P %zu %d %d %zu %zu %d %zu %zu %zu %zu %zu", nkeys, beta, nmod, N, budget, with_u, p.chunk, p.nchunks, p.index_bytes, p.galois_at, p.u_bytes);
            for (size_t c = 0; c < p.nchunks; c++) printf(" %zu %zu", p.first(c), p.count(c, nkeys));
            printf("\n");
        } else { fprintf(stderr, "unknown op %s\n", op); return 3; }
    }
    fclose(f);
    printf("OK\n");
    return 0;
}
