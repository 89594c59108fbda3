// The per-coefficient arithmetic of the general ring's collective bootstrap (sfgwas_amd/csrc/gring_refresh_arith.hpp) and its host planner
// (gring_refresh_plan.hpp) on the CPU: the very functions the kernels of gring_refresh.hip run, over accessors of a vector, on the operands a script names.
// Stand-alone: includes the two headers, links nothing of the library.  tests/test_ring_refresh_ref.py writes the script and compares every printed word with
// Python integers.
//   R W n mo mi sh e nmod q_0.. limb_0..limb_(W-1)     one coefficient of a share: the sign, the magnitude's W limbs, (mask + e) mod q_j; then, n > 0, the n limbs of
//                                                      the rescaled magnitude and (mask' + e) mod q_j
//   X nl nq n mo mi sh q_0..q_(nq-1) d_0..d_(nl-1)     one coefficient of the finish from its mixed-radix digits: the sign, the unscaled rows at the new moduli;
//                                                      then, n > 0, the n limbs of x, of the rescaled magnitude, and its residue at all nq moduli
//   S bits                                             a scale (the bits of a double): scale_ok, and Int(f) = m 2^e
//   F bits W sh                                        fits_q, fits_mask, limbs_for(bits, sh), limbs_for(64 W, sh)
//   PS nct nl nq N budget                              the share call's plan, its layout at the plan's chunk, first and count of every chunk
//   PF nct nl nq scaled N budget                       likewise the finish
#include "gring_refresh_arith.hpp"
#include "gring_refresh_plan.hpp"
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

using gr::u128;
using gr::u64;

struct Mod { u64 q, uhi, ulo; };
static Mod mod_of(u64 q) { const u128 u = ~(u128)0 / q; Mod m; m.q = q; m.uhi = (u64)(u >> 64); m.ulo = (u64)u; return m; }   // q is odd: floor((2^128 - 1) / q) = floor(2^128 / q)
static bool read_words(FILE *f, std::vector<u64> &v) { for (u64 &w : v) if (fscanf(f, "%llu", &w) != 1) return false; return true; }
static void print_words(const std::vector<u64> &v, size_t n) { for (size_t i = 0; i < n; i++) printf(" %llu", v[i]); }
static void print_plan(const GrfPlan &p, size_t nct) {
    printf(" %zu %zu %zu %zu %zu", p.words_per_ct, p.chunk, p.nchunks, p.bytes, p.reserve());
    for (size_t c = 0; c < p.nchunks; c++) printf(" %zu %zu", p.first(c), p.count(c, nct));
}

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: host_gring_refresh_test SCRIPT\n"); return 2; }
    FILE *f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 2; }
    char op[8];
    while (fscanf(f, "%7s", op) == 1) {
        if (!strcmp(op, "R")) {
            int W, n, sh, nmod; long long e; grf::Ratio r;
            if (fscanf(f, "%d %d %llu %llu %d %lld %d", &W, &n, &r.mo, &r.mi, &sh, &e, &nmod) != 7 || W < 1 || W > grf::kBigLimbs || (n && n < W) || n > grf::kBigLimbs || nmod < 1) return 3;
            r.sh = sh;
            std::vector<u64> q(nmod), a(n > W ? n : W, 0), in(W);
            if (!read_words(f, q) || !read_words(f, in)) return 3;
            for (int i = 0; i < W; i++) a[i] = in[i];
            auto L = [&](int i) { return a.at(i); };
            auto S = [&](int i, u64 v) { a.at(i) = v; };
            const bool neg = grf::to_magnitude(W, L, S);
            printf("R %d", neg ? 1 : 0); print_words(a, W);
            for (int j = 0; j < nmod; j++) { const Mod m = mod_of(q[j]); printf(" %llu", grf::add_small(grf::signed_residue(grf::limbs_mod(W, L, m.q, m.uhi, m.ulo), neg, m.q), (int32_t)e, m.q)); }
            if (n) {
                grf::rescale(n, L, S, r);
                print_words(a, n);
                for (int j = 0; j < nmod; j++) { const Mod m = mod_of(q[j]); printf(" %llu", grf::add_small(grf::signed_residue(grf::limbs_mod(n, L, m.q, m.uhi, m.ulo), neg, m.q), (int32_t)e, m.q)); }
            }
            printf("\n");
        } else if (!strcmp(op, "X")) {
            int nl, nq, n, sh; grf::Ratio r;
            if (fscanf(f, "%d %d %d %llu %llu %d", &nl, &nq, &n, &r.mo, &r.mi, &sh) != 6 || nl < 1 || nq < nl || nq > gr::kMaxMod || n < 0 || n > grf::kBigLimbs) return 3;
            r.sh = sh;
            std::vector<u64> q(nq), d(nl), half(nl), a(n ? n : 1, 0), Q(grf::kBigLimbs, 0);
            if (!read_words(f, q) || !read_words(f, d)) return 3;
            u64 rem = 0;                                                             // the digits of floor(Q / 2), as gring_io.hip's table builds them
            for (int i = nl - 1; i >= 0; i--) { const u128 cur = (u128)rem * q[i] + (q[i] - 1); half[i] = (u64)(cur >> 1); rem = (u64)(cur & 1); }
            auto D = [&](int i) { return d.at(i); };
            const bool neg = grf::is_negative(nl, D, [&](int i) { return half.at(i); });
            printf("X %d", neg ? 1 : 0);
            for (int j = nl; j < nq; j++) {
                const Mod m = mod_of(q[j]); u64 Qm = 1 % m.q;
                for (int i = 0; i < nl; i++) Qm = (u64)((u128)Qm * (q[i] % m.q) % m.q);
                const u64 v = grf::digits_mod(nl, D, [&](int i) { return q[i] % m.q; }, m.q, m.uhi, m.ulo);
                printf(" %llu", grf::recode_new(v, neg, Qm, m.q));
            }
            if (n) {
                Q[0] = 1;
                for (int i = 0; i < nl; i++) (void)grf::mul_add(grf::kBigLimbs, [&](int k) { return Q.at(k); }, [&](int k, u64 v) { Q.at(k) = v; }, q[i], 0);
                auto L = [&](int i) { return a.at(i); };
                auto S = [&](int i, u64 v) { a.at(i) = v; };
                grf::digits_to_limbs(nl, D, [&](int i) { return q.at(i); }, n, L, S);
                print_words(a, n);
                if (neg) grf::rsub(n, L, [&](int i) { return Q.at(i); }, S);
                grf::rescale(n, L, S, r);
                print_words(a, n);
                for (int j = 0; j < nq; j++) { const Mod m = mod_of(q[j]); printf(" %llu", grf::signed_residue(grf::limbs_mod(n, L, m.q, m.uhi, m.ulo), neg, m.q)); }
            }
            printf("\n");
        } else if (!strcmp(op, "S")) {
            u64 bits; if (fscanf(f, "%llu", &bits) != 1) return 3;
            double s; memcpy(&s, &bits, 8);
            u64 m = 0; int e = 0; const bool ok = grf::scale_ok(s);
            if (ok) grf::scale_int(s, m, e);
            printf("S %llu %d %llu %d\n", bits, ok ? 1 : 0, m, e);
        } else if (!strcmp(op, "F")) {
            int bits, W, sh; if (fscanf(f, "%d %d %d", &bits, &W, &sh) != 3) return 3;
            printf("F %d %d %d %d %d %d %d\n", bits, W, sh, grf::fits_q(bits, sh) ? 1 : 0, grf::fits_mask(W, sh) ? 1 : 0, grf::limbs_for(bits, sh), grf::limbs_for(64 * W, sh));
        } else if (!strcmp(op, "PS")) {
            size_t nct, N, budget; int nl, nq;
            if (fscanf(f, "%zu %d %d %zu %zu", &nct, &nl, &nq, &N, &budget) != 5) return 3;
            const GrfPlan p = grf_shares_plan(nct, nl, nq, N, budget);
            const GrfSharesLayout l = grf_shares_layout(nl, nq, N, p.chunk);
            printf("PS %zu %d %d %zu %zu", nct, nl, nq, N, budget); print_plan(p, nct);
            printf(" | %zu %zu %zu\n", l.R0, l.R1, l.end);
        } else if (!strcmp(op, "PF")) {
            size_t nct, N, budget; int nl, nq, scaled;
            if (fscanf(f, "%zu %d %d %d %zu %zu", &nct, &nl, &nq, &scaled, &N, &budget) != 6) return 3;
            const GrfPlan p = grf_finish_plan(nct, nl, nq, scaled != 0, N, budget);
            const GrfFinishLayout l = grf_finish_layout(nl, nq, scaled != 0, N, p.chunk);
            printf("PF %zu %d %d %d %zu %zu", nct, nl, nq, scaled, N, budget); print_plan(p, nct);
            printf(" | %d %zu %zu %zu %zu\n", grf_new_rows(nl, nq, scaled != 0), l.X, l.Y, l.S, l.end);
        } else { fprintf(stderr, "unknown op %s\n", op); return 3; }
    }
    fclose(f);
    printf("OK\n");
    return 0;
}
