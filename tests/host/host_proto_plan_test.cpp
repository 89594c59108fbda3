// host_proto_plan_test.cpp — the chunk rule of the fixed-ring protocol ends (sfgwas_amd/csrc/batch_plan.hpp) on the CPU: the header encrypt.hip, decrypt.hip,
// refresh.hip, rvec.hip and keygen.hip take their chunks and scratch sizes from, compiled for the host (with AddressSanitizer + UBSan where the runtimes exist) as a
// plain executable.  It reads a script (tests/test_proto_plan.py writes it), one call per line, and prints what the planner returns; the Python side holds every
// line against a literal restatement.  Checked here on every line: the chunks cover [0, n) exactly once and in order, none is empty or larger than the plan's
// chunk, and `bytes` is the chunk's scratch.  Every line ends with "| chunk nchunks bytes (first count){nchunks}".
//   B n words budget cap           batch_plan                                  -> "B | ..."
//   E nct nl np N                  enc_core_plan (encrypt_run)                 -> "E words | ..."
//   P nct nl N                     pcks_share_plan (sfg_pcks_gen_share_dev)    -> "P words | ..."
//   D nvec nl N coeff host parts   decode_plan (decode_run)                    -> "D x w out x_bytes w_bytes out_bytes | ..."   (words an item, bytes a chunk)
//   V nct W nl N                   rvec_batch_plan (ring-vector encode/decode) -> "V fft coef fft_bytes coef_bytes | ..."
//   G n                            grid_rows_plan without scratch (sfg_pcks_finish_dev, sfg_crp_fill_dev, refresh_gen_shares)   -> "G | ..."
//   F nct nl N                     refresh_finish: grid_rows_plan over x       -> "F x | ..."
//   S nct nl N                     sfg_ckks_to_ss_share_dev: over zero_e       -> "S zero_e | ..."
//   K                              the named constants -> "K budget pcks_cap decode_cap rvec_cap grid_cap grid_dim_max"
#include "batch_plan.hpp"

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

// the covering invariants, then the common tail of a line
static void tail(const BatchPlan &p, int n, size_t words, size_t ln) {
    if (n <= 0) { if (p.chunk || p.nchunks || p.bytes) fail("an empty call with a plan", ln); }
    else if (p.chunk < 1 || p.chunk > n || p.nchunks < 1) fail("chunk outside [1, n]", ln);
    if (p.bytes != (size_t)p.chunk * words * 8 || p.bytes != p.bytes_of(words)) fail("bytes is not the chunk's scratch", ln);
    std::cout << " | " << p.chunk << " " << p.nchunks << " " << p.bytes;
    long long next = 0;
    for (int c = 0; c < p.nchunks; c++) {
        const int first = p.first(c), count = p.count(c, n);
        if (first != next) fail("chunks out of order or not adjacent", ln);
        if (count < 1 || count > p.chunk) fail("a chunk empty or above the plan's chunk", ln);
        if (c + 1 < p.nchunks && count != p.chunk) fail("a short chunk before the last", ln);
        next += count;
        std::cout << " " << first << " " << count;
    }
    if (next != (n > 0 ? n : 0)) fail("chunks do not cover [0, n)", ln);
    std::cout << "\n";
}

int main(int argc, char **argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: %s script\n", argv[0]); return 2; }
    std::ifstream f(argv[1]);
    if (!f) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    std::string line; size_t ln = 0;
    while (std::getline(f, line)) {
        ln++;
        std::istringstream is(line);
        char op; is >> op;
        if (op == 'B') {
            int n, cap; size_t words, budget; is >> n >> words >> budget >> cap;
            if (!is) fail("bad B", ln);
            std::cout << "B";
            tail(batch_plan(n, words, budget, cap), n, words, ln);
        } else if (op == 'E') {
            int nct, nl, np; size_t N; is >> nct >> nl >> np >> N;
            if (!is) fail("bad E", ln);
            std::cout << "E " << enc_core_words(nl, np, N);
            tail(enc_core_plan(nct, nl, np, N), nct, enc_core_words(nl, np, N), ln);
        } else if (op == 'P') {
            int nct, nl; size_t N; is >> nct >> nl >> N;
            if (!is) fail("bad P", ln);
            std::cout << "P " << pcks_share_words(nl, N);
            tail(pcks_share_plan(nct, nl, N), nct, pcks_share_words(nl, N), ln);
        } else if (op == 'D') {
            int nvec, nl, coeff, host, parts; size_t N; is >> nvec >> nl >> N >> coeff >> host >> parts;
            if (!is) fail("bad D", ln);
            const DecodeWords d = decode_words(nl, N, coeff != 0, host != 0, parts);
            const BatchPlan p = decode_plan(nvec, d);
            if (p.bytes_of(d.x) + p.bytes_of(d.w) + p.bytes_of(d.out) != p.bytes) fail("the three buffers are not the chunk's scratch", ln);
            std::cout << "D " << d.x << " " << d.w << " " << d.out << " " << p.bytes_of(d.x) << " " << p.bytes_of(d.w) << " " << p.bytes_of(d.out);
            tail(p, nvec, d.total(), ln);
        } else if (op == 'V') {
            int nct, W, nl; size_t N; is >> nct >> W >> nl >> N;
            if (!is) fail("bad V", ln);
            const RvecWords r = rvec_words(W, nl, N);
            const BatchPlan p = rvec_batch_plan(nct, r);
            if (p.bytes_of(r.fft) + p.bytes_of(r.coef) != p.bytes) fail("the two buffers are not the chunk's scratch", ln);
            std::cout << "V " << r.fft << " " << r.coef << " " << p.bytes_of(r.fft) << " " << p.bytes_of(r.coef);
            tail(p, nct, r.total(), ln);
        } else if (op == 'G') {
            int n; is >> n;
            if (!is) fail("bad G", ln);
            std::cout << "G";
            tail(grid_rows_plan(n), n, 0, ln);
        } else if (op == 'F' || op == 'S') {
            int nct, nl; size_t N; is >> nct >> nl >> N;
            if (!is) fail("bad F or S", ln);
            const RefreshWords r = refresh_words(nl, N);
            const size_t words = op == 'F' ? r.x : r.zero_e;
            std::cout << op << " " << words;
            tail(grid_rows_plan(nct, words), nct, words, ln);
        } else if (op == 'K') {
            std::cout << "K " << kEncBudgetBytes << " " << kPcksShareMaxChunk << " " << kDecodeMaxChunk << " " << kRvecMaxChunk << " " << kGridRowsMaxChunk << " " << kGridDimMax << "\n";
        } else fail("unknown op", ln);
    }
    std::cout << "OK\n";
    return 0;
}
