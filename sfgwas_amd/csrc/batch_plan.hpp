// batch_plan.hpp - host-only chunking of a call over n independent items (ciphertexts, plaintexts, rows): ONE rule - items per chunk are what a byte budget
// holds, clamped to [1, cap] and to n - and, per entry-point family of the fixed-ring protocol ends (encrypt.hip, decrypt.hip, refresh.hip, rvec.hip, keygen.hip),
// the per-item words of each named scratch buffer, the budget and the cap.  The executors loop `for c in [0, nchunks)` with first(c) and count(c, n) and size every
// buffer with bytes_of().  (The general ring's planner, gring_io_plan.hpp, states the same rule at a cap of 256 for itself: tests hold that header on its own.)
// Standard library only and on its own: tests/host/host_proto_plan_test.cpp holds it on the CPU.
#pragma once
#include <cstddef>

struct BatchPlan {
    int chunk = 0;                             // items per chunk
    int nchunks = 0;
    size_t bytes = 0;                          // scratch of one chunk: chunk * words_per_item * 8
    int first(int c) const { return c * chunk; }
    int count(int c, int n) const { const int left = n - c * chunk; return left < chunk ? left : chunk; }
    size_t bytes_of(size_t words_per_item) const { return (size_t)chunk * words_per_item * 8; }      // one named buffer of a chunk
};
constexpr size_t kNoBudget = ~(size_t)0;       // no scratch bounds the chunk
constexpr int kNoCap = 0;
// chunks of n items of `words_per_item` 64-bit words each (0: the pass has no scratch of its own); max_chunk <= 0: no cap
inline BatchPlan batch_plan(int n, size_t words_per_item, size_t budget_bytes, int max_chunk) {
    BatchPlan p;
    if (n <= 0) return p;
    size_t fit = words_per_item ? budget_bytes / (words_per_item * 8) : (size_t)n;
    if (fit < 1) fit = 1;                                                   // one item always runs: the budget is a preference, the allocation decides
    if (max_chunk > 0 && fit > (size_t)max_chunk) fit = (size_t)max_chunk;
    p.chunk = (size_t)n < fit ? n : (int)fit;
    p.nchunks = n / p.chunk + (n % p.chunk ? 1 : 0);
    p.bytes = p.bytes_of(words_per_item);
    return p;
}

constexpr int kGridDimMax = 65535;             // what grid.y and grid.z of a launch hold; every plan below puts `chunk` items there, one grid row per item

// The encryption core (encrypt.hip encrypt_run), nl = level + 1 moduli of Q and np of P: T [chunk][2][nl + np][N] ("encrypt.T").  Its launches are grid.x only.
constexpr size_t kEncBudgetBytes = (size_t)1 << 30;      // as chosen before; not re-tuned here
inline size_t enc_core_words(int nl, int np, size_t N) { return (size_t)2 * ((size_t)nl + np) * N; }
inline BatchPlan enc_core_plan(int nct, int nl, int np, size_t N) { return batch_plan(nct, enc_core_words(nl, np, N), kEncBudgetBytes, kNoCap); }

// sfg_pcks_gen_share_dev: T [chunk][2][nl][N] ("decrypt.share"), the ModDown of the error pairs before the share kernel
constexpr int kPcksShareMaxChunk = 256;        // grid.z of the share kernel = chunk: far below 65535
inline size_t pcks_share_words(int nl, size_t N) { return (size_t)2 * nl * N; }
inline BatchPlan pcks_share_plan(int nct, int nl, size_t N) { return batch_plan(nct, pcks_share_words(nl, N), kNoBudget, kPcksShareMaxChunk); }

// The decoder (decrypt.hip decode_run): x [chunk][nl][N] residues ("decrypt.x"); w [chunk][N] double-double coefficients ("decrypt.w"), absent for the coefficient
// form; out ("decrypt.out"), the staging of a host call: N doubles a plaintext for the coefficient form, else n = N / 2 slots times parts (1: real, 2: complex)
constexpr int kDecodeMaxChunk = 512;           // as chosen before; not re-tuned here
struct DecodeWords { size_t x = 0, w = 0, out = 0; size_t total() const { return x + w + out; } };
inline DecodeWords decode_words(int nl, size_t N, bool coeff_form, bool host_out, int parts) {
    DecodeWords d;
    d.x = (size_t)nl * N;
    d.w = coeff_form ? 0 : 2 * N;
    d.out = !host_out ? 0 : coeff_form ? N : (N / 2) * (size_t)parts;
    return d;
}
inline BatchPlan decode_plan(int nvec, const DecodeWords &d) { return batch_plan(nvec, d.total(), kNoBudget, kDecodeMaxChunk); }

// The ring-vector encoder and decoder (rvec.hip) at W words a fixed-point number: fft [chunk][2][W][n] ("rvec.fft"), coef [chunk][nl][N] ("rvec.coef")
constexpr int kRvecMaxChunk = 64;              // as chosen before; not re-tuned here
struct RvecWords { size_t fft = 0, coef = 0; size_t total() const { return fft + coef; } };
inline RvecWords rvec_words(int W, int nl, size_t N) { RvecWords r; r.fft = (size_t)2 * W * (N / 2); r.coef = (size_t)nl * N; return r; }
inline BatchPlan rvec_batch_plan(int nct, const RvecWords &r) { return batch_plan(nct, r.total(), kNoBudget, kRvecMaxChunk); }

// Grid-bound row passes: launches of grid (N / 256, rows, chunk) or (N / 256, chunk) with no budget - sfg_pcks_finish_dev, sfg_crp_fill_dev and the three refresh
// entry points.  refresh_finish keeps x [chunk][nl][N] ("refresh.x"), sfg_ckks_to_ss_share_dev N 32-bit zeros an item ("refresh.zero_e"); the others have no scratch.
constexpr int kGridRowsMaxChunk = 32768;       // grid.z (grid.y) = chunk: at most 65535
struct RefreshWords { size_t x = 0, zero_e = 0; };
inline RefreshWords refresh_words(int nl, size_t N) { RefreshWords r; r.x = (size_t)nl * N; r.zero_e = N / 2; return r; }
inline BatchPlan grid_rows_plan(int n, size_t words_per_item = 0) { return batch_plan(n, words_per_item, kNoBudget, kGridRowsMaxChunk); }
