// gring_io_plan.hpp - host-only planning of the general ring's encryption core (gring_io.hip): the workspace of one ciphertext and the chunks of a call.
// Standard library only (like gring_plan.hpp): tests/host/host_gring_io_test.cpp holds it on the CPU.
#pragma once
#include <cstddef>

// Workspace of ONE ciphertext of the core at nl = level + 1 moduli of Q and np of P, npoly = 1 (a share whose second polynomial nobody wants) or 2, in 64-bit words:
//   U   [nl + np][N]            NTT(u) at every target (absent when u drops out: the zero public key of the collective key switch)
//   T   [npoly][nl + np][N]     NTT(e_i), then t_i
//   Y2  [npoly][np][N]          the ModDown's y rows
//   ext [npoly][nl][N]          the extension of the P rows to Q
//   V2  [npoly][N] 32-bit       the float correction
struct GriPlan {
    static constexpr int kMaxChunk = 256;      // ciphertexts per chunk at most: grid.z = chunk * npoly stays far below 65536
    size_t words_per_ct = 0;
    int chunk = 0;                             // ciphertexts per chunk
    int nchunks = 0;
    size_t bytes = 0;                          // of the workspace: chunk * words_per_ct * 8
    int first(int c) const { return c * chunk; }
    int count(int c, int nct) const { int left = nct - c * chunk; return left < chunk ? left : chunk; }
};
inline size_t gri_words_per_ct(int nl, int np, int npoly, bool with_u, size_t N) {
    const size_t nt = (size_t)nl + np;
    return ((with_u ? nt : 0) + (size_t)npoly * nt + (size_t)npoly * np + (size_t)npoly * nl) * N + ((size_t)npoly * N + 1) / 2;
}
// chunks of nct items of `words` 64-bit words each
inline GriPlan gri_plan_words(int nct, size_t words, size_t budget_bytes) {
    GriPlan p;
    p.words_per_ct = words;
    if (nct <= 0) return p;
    size_t fit = budget_bytes / (p.words_per_ct * 8);
    if (fit < 1) fit = 1;                                                   // one ciphertext always runs: the budget is a preference, the allocation decides
    if (fit > (size_t)GriPlan::kMaxChunk) fit = GriPlan::kMaxChunk;
    p.chunk = (size_t)nct < fit ? nct : (int)fit;
    p.nchunks = (nct + p.chunk - 1) / p.chunk;
    p.bytes = (size_t)p.chunk * p.words_per_ct * 8;
    return p;
}
inline GriPlan gri_plan(int nct, int nl, int np, int npoly, bool with_u, size_t N, size_t budget_bytes) { return gri_plan_words(nct, gri_words_per_ct(nl, np, npoly, with_u, N), budget_bytes); }
// the decoder's workspace of one plaintext: its nl rows (residues, then digits in place) and N doubles of results
inline GriPlan gri_decode_plan(int nct, int nl, size_t N, size_t budget_bytes) { return gri_plan_words(nct, ((size_t)nl + 1) * N, budget_bytes); }
