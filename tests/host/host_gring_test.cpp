// The general ring's per-element arithmetic (sfgwas_amd/csrc/gring_arith.hpp) and its host planner (gring_plan.hpp) on the CPU: the very functions the kernels
// run, on the operands a script names.  Stand-alone: includes the two headers, links nothing of the library.  tests/test_ring_ref.py writes the script, compares
// every printed word with Python integers and checks that three planted mistakes change the output.
//   M q                              directed operands of one modulus: Shoup and Barrett products, lazy butterflies, canonical reduction
//   E k q_1..q_k x_1..x_k qt         one basis-extension element: y_1..y_k, v, the residue at qt
//   D y                              the bits of (double)y
//   P logN                           the transform's stage split
//   G level np                       the digits of the key switch
//   W njobs level np N budget        the key switch's workspace: bytes of an item, chunk, chunks, bytes to reserve; the layout at that chunk; first and count of every chunk
//   Z nct level N budget             the rescale's workspace, likewise
//   X n cap                          the pieces of gr_split
//   U nmod                           the launch caps
#include "gring_arith.hpp"
#include "gring_plan.hpp"
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

using gr::u64;
using gr::u128;

static u64 mulm(u64 a, u64 b, u64 q) { return (u64)(((u128)a * b) % q); }
static u64 powm(u64 a, u64 e, u64 q) { u64 r = 1 % q; a %= q; while (e) { if (e & 1) r = mulm(r, a, q); a = mulm(a, a, q); e >>= 1; } return r; }
static u64 shoup_of(u64 w, u64 q) { return (u64)(((u128)w << 64) / q); }

static void per_modulus(u64 q) {
    const u128 u = ~(u128)0 / q; const u64 uhi = (u64)(u >> 64), ulo = (u64)u;
    const u64 carry = 0xFFFFFFFFFFFFFFFFULL, lo32 = 0x00000000FFFFFFFFULL, hi32 = 0xFFFFFFFF00000000ULL, mix = 0xFFFFFFFF00000001ULL;
    // every product of two of these carries out of each 32-bit piece of the 128-bit result
    const u64 any[] = {0, 1, q - 1, q, q + 1, 2 * q - 1, 2 * q, 4 * q - 1, lo32, hi32, mix, carry, carry - 1, (1ULL << 63) - 1, 1ULL << 63};
    const u64 ws[] = {0, 1, 2, q - 1, q - 2, carry % q, hi32 % q, mix % q, q / 2, q / 2 + 1};
    for (u64 a : any) for (u64 w : ws) {
        const u64 wsh = shoup_of(w, q);
        printf("S %llu %llu %llu %llu %llu\n", q, a, w, gr::shoup_lazy(a, w, wsh, q), gr::shoup(a, w, wsh, q));
    }
    const u64 can[] = {0, 1, 2, q - 1, q - 2, q / 2, q / 2 + 1, carry % q, lo32 % q, hi32 % q, mix % q};
    for (u64 a : can) for (u64 b : can) printf("B %llu %llu %llu %llu\n", q, a, b, gr::mulmod(a, b, q, uhi, ulo));
    // raw 128-bit words: multiples of q (the estimate of the quotient is one short there), the extremes, carries in every piece
    const u128 raw[] = {(u128)0, (u128)q - 1, (u128)q, (u128)q + 1, (u128)2 * q - 1, (u128)2 * q, (u128)q * q, (u128)q * q - 1, (u128)q * carry, (u128)q * carry + (q - 1),
                        ~(u128)0, ~(u128)0 - 1, ((u128)carry << 64), (u128)carry, ((u128)hi32 << 64) | lo32, ((u128)lo32 << 64) | hi32, ((u128)mix << 64) | mix,
                        (u128)(q - 1) * (q - 1) * 48};
    for (u128 x : raw) printf("R %llu %llu %llu %llu\n", q, (u64)(x >> 64), (u64)x, gr::barrett128((u64)(x >> 64), (u64)x, q, uhi, ulo));
    const u64 lazy4[] = {0, 1, q - 1, q, 2 * q - 1, 2 * q, 3 * q, 4 * q - 1}, lazy2[] = {0, 1, q - 1, q, q + 1, 2 * q - 1};
    const u64 tw[] = {1, q - 1, carry % q, q / 2 + 1};
    for (u64 w : tw) {
        const u64 wsh = shoup_of(w, q);
        for (u64 X : lazy4) for (u64 Y : lazy4) { u64 x = X, y = Y; gr::bfly_fwd(x, y, w, wsh, q); printf("F %llu %llu %llu %llu %llu %llu\n", q, X, Y, w, x, y); }
        for (u64 X : lazy2) for (u64 Y : lazy2) { u64 x = X, y = Y; gr::bfly_inv(x, y, w, wsh, q); printf("I %llu %llu %llu %llu %llu %llu\n", q, X, Y, w, x, y); }
    }
    for (u64 x : lazy4) printf("C %llu %llu %llu\n", q, x, gr::canon4(x, q));
    const u64 ab[] = {0, 1, q - 1, q / 2, q / 2 + 1};
    for (u64 a : ab) for (u64 b : ab) printf("A %llu %llu %llu %llu %llu\n", q, a, b, gr::addmod(a, b, q), gr::submod(a, b, q));
}

static void ext_element(int k, const std::vector<u64> &qs, const std::vector<u64> &xs, u64 qt) {
    const u128 u = ~(u128)0 / qt; const u64 uhi = (u64)(u >> 64), ulo = (u64)u;
    double vf = 0.0; u128 S = 0; u64 D_t = 1 % qt;
    printf("E");
    for (int m = 0; m < k; m++) {
        u64 h = 1, ht = 1 % qt;
        for (int j = 0; j < k; j++) if (j != m) { h = mulm(h, qs[j] % qs[m], qs[m]); ht = mulm(ht, qs[j] % qt, qt); }
        const u64 inv = powm(h, qs[m] - 2, qs[m]);
        const u64 y = gr::shoup(xs[m], inv, shoup_of(inv, qs[m]), qs[m]);
        vf = gr::ext_accumulate(vf, y, qs[m]);
        S += (u128)y * ht;
        D_t = mulm(D_t, qs[m] % qt, qt);
        printf(" %llu", y);
    }
    const u64 v = k == 1 ? 0 : gr::ext_truncate(vf);
    printf(" %llu %llu\n", v, gr::ext_finish(S, v, D_t, qt, uhi, ulo));
}

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: host_gring_test SCRIPT\n"); return 2; }
    FILE *f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 2; }
    char op[8];
    while (fscanf(f, "%7s", op) == 1) {
        if (!strcmp(op, "M")) { u64 q; if (fscanf(f, "%llu", &q) != 1) return 3; per_modulus(q); }
        else if (!strcmp(op, "E")) {
            int k; if (fscanf(f, "%d", &k) != 1 || k < 1 || k > gr::kMaxMod) return 3;
            std::vector<u64> qs(k), xs(k); u64 qt;
            for (int m = 0; m < k; m++) if (fscanf(f, "%llu", &qs[m]) != 1) return 3;
            for (int m = 0; m < k; m++) if (fscanf(f, "%llu", &xs[m]) != 1) return 3;
            if (fscanf(f, "%llu", &qt) != 1) return 3;
            ext_element(k, qs, xs, qt);
        } else if (!strcmp(op, "D")) {
            u64 y; if (fscanf(f, "%llu", &y) != 1) return 3;
            const double d = gr::to_double(y); u64 bits; memcpy(&bits, &d, 8);
            printf("D %llu %llu\n", y, bits);
        } else if (!strcmp(op, "P")) {
            int logN; if (fscanf(f, "%d", &logN) != 1) return 3;
            const GrNttPlan p = gr_ntt_plan(logN);
            printf("P %d %d %d %d %d %d %d %zu %zu\n", logN, p.ok ? 1 : 0, p.a, p.b, p.col_run, p.chunks, p.tiles_per_row, p.col_stride, p.lds_bytes);
        } else if (!strcmp(op, "G")) {
            int level, np; if (fscanf(f, "%d %d", &level, &np) != 2) return 3;
            const GrDigits d = gr_digits(level, np);
            printf("G %d %d %d %d %d\n", level, np, d.alpha, d.beta, d.nl);
        } else if (!strcmp(op, "W")) {
            size_t njobs, N, budget; int level, np;
            if (fscanf(f, "%zu %d %d %zu %zu", &njobs, &level, &np, &N, &budget) != 5) return 3;
            const GrChunks p = gr_ks_plan(njobs, level, np, N, budget);
            const GrKsLayout l = gr_ks_layout(level, np, N, p.chunk);
            printf("W %zu %d %d %zu %zu %zu %zu %zu %zu", njobs, level, np, N, budget, p.per_item, p.chunk, p.nchunks, p.bytes);
            printf(" %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu", l.c2, l.Y, l.ext, l.accQ, l.accP, l.Y2, l.ext2, l.V, l.V2, l.jobs, l.end);
            for (size_t c = 0; c < p.nchunks; c++) printf(" %zu %zu", p.first(c), p.count(c, njobs));
            printf("\n");
        } else if (!strcmp(op, "Z")) {
            size_t nct, N, budget; int level;
            if (fscanf(f, "%zu %d %zu %zu", &nct, &level, &N, &budget) != 4) return 3;
            const GrChunks p = gr_rescale_plan(nct, level, N, budget);
            const GrRescaleLayout l = gr_rescale_layout(level, N, p.chunk);
            printf("Z %zu %d %zu %zu %zu %zu %zu %zu %zu %zu %zu", nct, level, N, budget, p.per_item, p.chunk, p.nchunks, p.bytes, l.T, l.tmp, l.end);
            for (size_t c = 0; c < p.nchunks; c++) printf(" %zu %zu", p.first(c), p.count(c, nct));
            printf("\n");
        } else if (!strcmp(op, "X")) {
            size_t n, cap; if (fscanf(f, "%zu %zu", &n, &cap) != 2 || cap < 1) return 3;
            printf("X %zu %zu", n, cap);
            gr_split(n, cap, [](size_t i0, size_t cnt) { printf(" %zu %zu", i0, cnt); return 0; });
            printf("\n");
        } else if (!strcmp(op, "U")) {
            int nmod; if (fscanf(f, "%d", &nmod) != 1 || nmod < 1) return 3;
            printf("U %d %zu %zu %zu %zu\n", nmod, kGrLaunchCap, kGrEwCap, kGrKsJobCap, gr_from_mont_cap(nmod));
        } else return 3;
    }
    fclose(f);
    printf("OK\n");
    return 0;
}
