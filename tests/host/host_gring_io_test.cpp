// The per-element arithmetic of the general ring's two ends (sfgwas_amd/csrc/gring_io_arith.hpp) and their host planner (gring_io_plan.hpp) on the CPU: the very
// functions the kernels of gring_io.hip run, on the operands a script names.  Stand-alone: includes the two headers, links nothing of the library.
// tests/test_ring_io_ref.py writes the script, compares every printed word with Python integers and checks that planted mistakes change the output.
//   L v q                                  the lift of the signed sample v modulo q
//   T r shift                              the ternary sample of bits shift, shift + 1 of r
//   J j                                    the sampler's places of coefficient j: t, a, u block, u word, u shift, e block, e word
//   N logN                                 the block counts of one polynomial of 2^logN coefficients, and the largest block any coefficient reads
//   C nct nl np npoly with_u N budget      the chunks of a call
//   G k q_0..q_(k-1) x_0..x_(k-1) bits      one decoded coefficient from its residues and the scale (a double's bits): the mixed-radix digits, the sign, the
//                                          magnitude's digits, the bits of the double returned
//   K nct nl N budget                      the decoder's chunks
//   CL nct nl np npoly with_u N budget     the encryption core's workspace: its plan, the layout at the plan's chunk, first and count of every chunk
//   KL | EL | VL  nct nl N budget          likewise the coefficient decoder's, the encoder's and the vector decoder's
//   R hi lo band                          (bits of three doubles) the encoder's rounding of the pair hi + lo with its band test: status, p
//   Q p q                                  the signed integer p, |p| < 2^62, modulo q
//   B S                                    (bits) the band of a vector whose scaled slot sum is S
#include "gring_io_arith.hpp"
#include "gring_io_plan.hpp"
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

using gr::u64;

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: host_gring_io_test SCRIPT\n"); return 2; }
    FILE *f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 2; }
    char op[8];
    while (fscanf(f, "%7s", op) == 1) {
        if (!strcmp(op, "L")) {
            long long v; u64 q; if (fscanf(f, "%lld %llu", &v, &q) != 2) return 3;
            printf("L %lld %llu %llu\n", v, q, gio::lift((int32_t)v, q));
        } else if (!strcmp(op, "T")) {
            u64 r; int sh; if (fscanf(f, "%llu %d", &r, &sh) != 2 || sh < 0 || sh > 62) return 3;
            printf("T %llu %d %d\n", r, sh, gio::samp_ternary(r, sh));
        } else if (!strcmp(op, "J")) {
            int j; if (fscanf(f, "%d", &j) != 1 || j < 0) return 3;
            const int t = gio::samp_t(j), a = gio::samp_a(j);
            printf("J %d %d %d %u %d %d %u %d\n", j, t, a, gio::samp_u_block(t, a), gio::samp_u_word(t), gio::samp_u_shift(a), gio::samp_e_block(t, a), gio::samp_e_word(a));
        } else if (!strcmp(op, "N")) {
            int logN; if (fscanf(f, "%d", &logN) != 1 || logN < 12 || logN > 16) return 3;
            const int N = 1 << logN; unsigned mu = 0, me = 0;
            for (int j = 0; j < N; j++) {
                const int t = gio::samp_t(j), a = gio::samp_a(j);
                if (gio::samp_u_block(t, a) > mu) mu = gio::samp_u_block(t, a);
                if (gio::samp_e_block(t, a) > me) me = gio::samp_e_block(t, a);
            }
            printf("N %d %u %u %u %u\n", logN, gio::samp_u_blocks(N), gio::samp_e_blocks(N), mu, me);
        } else if (!strcmp(op, "C")) {
            int nct, nl, np, npoly, with_u; size_t N, budget;
            if (fscanf(f, "%d %d %d %d %d %zu %zu", &nct, &nl, &np, &npoly, &with_u, &N, &budget) != 7) return 3;
            const GriPlan p = gri_plan(nct, nl, np, npoly, with_u != 0, N, budget);
            printf("C %d %d %d %d %d %zu %zu %zu %d %d %zu", nct, nl, np, npoly, with_u, N, budget, p.words_per_ct, p.chunk, p.nchunks, p.bytes);
            for (int c = 0; c < p.nchunks; c++) printf(" %d %d", p.first(c), p.count(c, nct));
            printf("\n");
        } else if (!strcmp(op, "G")) {
            int k; if (fscanf(f, "%d", &k) != 1 || k < 1 || k > gr::kMaxMod) return 3;
            std::vector<u64> q(k), x(k), d(k), half(k); u64 bits;
            for (int i = 0; i < k; i++) if (fscanf(f, "%llu", &q[i]) != 1) return 3;
            for (int i = 0; i < k; i++) if (fscanf(f, "%llu", &x[i]) != 1) return 3;
            if (fscanf(f, "%llu", &bits) != 1) return 3;
            double scale; memcpy(&scale, &bits, 8);
            for (int i = 0; i < k; i++) {                                    // what gring_io.hip's gri_dec_tab and k_gri_garner do
                const gr::u128 u = ~(gr::u128)0 / q[i]; u64 W = 1 % q[i], acc = 0;
                for (int j = 0; j < i; j++) W = (u64)(((gr::u128)W * (q[j] % q[i])) % q[i]);
                u64 inv = 1 % q[i], b = W, e = q[i] - 2;
                while (e) { if (e & 1) inv = (u64)(((gr::u128)inv * b) % q[i]); b = (u64)(((gr::u128)b * b) % q[i]); e >>= 1; }
                for (int j = i - 1; j >= 0; j--) acc = gio::garner_acc(acc, d[j], q[j] % q[i], q[i], (u64)(u >> 64), (u64)u);
                d[i] = gio::garner_digit(x[i], acc, inv, (u64)(((gr::u128)inv << 64) / q[i]), q[i]);
            }
            u64 rem = 0;
            for (int i = k - 1; i >= 0; i--) { const gr::u128 cur = (gr::u128)rem * q[i] + (q[i] - 1); half[i] = (u64)(cur >> 1); rem = (u64)(cur & 1); }
            printf("G %d", k);
            for (int i = 0; i < k; i++) printf(" %llu", d[i]);
            std::vector<u64> m = d;
            const double r = gio::decode_digits(k, [&](int i) { return m[i]; }, [&](int i, u64 v) { m[i] = v; }, [&](int i) { return q[i]; }, [&](int i) { return half[i]; }, scale);
            u64 rb; memcpy(&rb, &r, 8);
            for (int i = 0; i < k; i++) printf(" %llu", m[i]);
            printf(" %llu\n", rb);
        } else if (!strcmp(op, "K")) {
            int nct, nl; size_t N, budget;
            if (fscanf(f, "%d %d %zu %zu", &nct, &nl, &N, &budget) != 4) return 3;
            const GriPlan p = gri_decode_plan(nct, nl, N, budget);
            printf("K %d %d %zu %zu %zu %d %d %zu\n", nct, nl, N, budget, p.words_per_ct, p.chunk, p.nchunks, p.bytes);
        } else if (!strcmp(op, "CL") || !strcmp(op, "KL") || !strcmp(op, "EL") || !strcmp(op, "VL")) {
            // a workspace's plan, then its layout at the plan's chunk, then first and count of every chunk
            int nct, nl, np = 0, npoly = 0, with_u = 0; size_t N, budget;
            if (fscanf(f, "%d %d", &nct, &nl) != 2) return 3;
            if (op[0] == 'C' && fscanf(f, "%d %d %d", &np, &npoly, &with_u) != 3) return 3;
            if (fscanf(f, "%zu %zu", &N, &budget) != 2) return 3;
            GriPlan p; std::vector<size_t> at;
            if (op[0] == 'C') {
                p = gri_plan(nct, nl, np, npoly, with_u != 0, N, budget);
                const GriCoreLayout l = gri_core_layout(nl, np, npoly, with_u != 0, N, (size_t)p.chunk); at = {l.UQ, l.UP, l.TQ, l.TP, l.Y2, l.ext, l.V2, l.end};
            } else if (op[0] == 'K') {
                p = gri_decode_plan(nct, nl, N, budget);
                const GriDecodeLayout l = gri_decode_layout(nl, N, (size_t)p.chunk); at = {l.X, l.out, l.end};
            } else if (op[0] == 'E') {
                p = gri_encode_plan(nct, nl, N, budget);
                const GriEncodeLayout l = gri_encode_layout(nl, N, (size_t)p.chunk); at = {l.A, l.vals, l.R, l.band, l.flags, l.end};
            } else {
                p = gri_vectors_plan(nct, nl, N, budget);
                const GriVectorsLayout l = gri_vectors_layout(nl, N, (size_t)p.chunk); at = {l.A, l.Wd, l.X, l.re, l.im, l.end};
            }
            printf("%s %d %d %d %d %d %zu %zu %zu %d %d %zu %zu %zu", op, nct, nl, np, npoly, with_u, N, budget, p.words_per_ct, p.chunk, p.nchunks, p.bytes, p.reserve(), at.size());
            for (size_t o : at) printf(" %zu", o);
            for (int c = 0; c < p.nchunks; c++) printf(" %d %d", p.first(c), p.count(c, nct));
            printf("\n");
        } else if (!strcmp(op, "R")) {
            u64 b[3]; double v[3];
            if (fscanf(f, "%llu %llu %llu", &b[0], &b[1], &b[2]) != 3) return 3;
            memcpy(v, b, 24);
            gio::dd x; x.hi = v[0]; x.lo = v[1];
            long long pp; const int st = gio::round_half_away(x, v[2], pp);
            printf("R %llu %llu %llu %d %lld\n", b[0], b[1], b[2], st, pp);
        } else if (!strcmp(op, "Q")) {
            long long pp; u64 q; if (fscanf(f, "%lld %llu", &pp, &q) != 2) return 3;
            const gr::u128 u = ~(gr::u128)0 / q;
            printf("Q %lld %llu %llu\n", pp, q, gio::reduce_i62(pp, q, (u64)(u >> 64), (u64)u));
        } else if (!strcmp(op, "B")) {
            u64 b; double S; if (fscanf(f, "%llu", &b) != 1) return 3;
            memcpy(&S, &b, 8);
            const double band = gio::enc_band(S); u64 ob; memcpy(&ob, &band, 8);
            printf("B %llu %llu\n", b, ob);
        } else return 3;
    }
    fclose(f);
    printf("OK\n");
    return 0;
}
