// gring_io_plan.hpp - host-only planning of the general ring's two ends (gring_io.hip): for each of its workspaces (the encryption core, the coefficient decoder,
// the encoder, the vector decoder) ONE layout - the offset of every region of a chunk of J items, in 64-bit words - and ONE plan - the chunk, the chunks of a
// call and the bytes to reserve.  The executors take every pointer from the layout.
// Standard library only and on its own (like gring_plan.hpp, which it does not include): tests/host/host_gring_io_test.cpp holds it on the CPU.
#pragma once
#include <cstddef>

struct GriCarve { size_t at = 0; size_t take(size_t words) { const size_t o = at; at += words; return o; } };      // the next region of a layout

struct GriPlan {
    static constexpr int kMaxChunk = 256;      // items per chunk at most: grid.z = chunk * npoly stays far below 65536
    static constexpr size_t kSlackBytes = 64;  // reserved beyond the chunk and never carved
    size_t words_per_ct = 0;                   // the figure that sizes a chunk
    int chunk = 0;                             // items per chunk
    int nchunks = 0;
    size_t bytes = 0;                          // of the chunk: chunk * words_per_ct * 8
    size_t reserve() const { return bytes + kSlackBytes; }
    int first(int c) const { return c * chunk; }
    int count(int c, int nct) const { int left = nct - c * chunk; return left < chunk ? left : chunk; }
};
// chunks of nct items of `words` 64-bit words each
inline GriPlan gri_plan_words(int nct, size_t words, size_t budget_bytes) {
    GriPlan p;
    p.words_per_ct = words;
    if (nct <= 0) return p;
    size_t fit = budget_bytes / (p.words_per_ct * 8);
    if (fit < 1) fit = 1;                                                   // one item always runs: the budget is a preference, the allocation decides
    if (fit > (size_t)GriPlan::kMaxChunk) fit = GriPlan::kMaxChunk;
    p.chunk = (size_t)nct < fit ? nct : (int)fit;
    p.nchunks = (nct + p.chunk - 1) / p.chunk;
    p.bytes = (size_t)p.chunk * p.words_per_ct * 8;
    return p;
}

// The encryption core, J ciphertexts at nl = level + 1 moduli of Q and np of P, npoly = 1 (a share whose second polynomial nobody wants) or 2:
//   UQ [J][nl][N], UP [J][np][N]              NTT(u) at every target (absent when u drops out: the zero public key of the collective key switch)
//   TQ [J][npoly][nl][N], TP [J][npoly][np][N]  NTT(e_i), then t_i
//   Y2 [J][npoly][np][N]                      the ModDown's y rows
//   ext [J][npoly][nl][N]                     the extension of the P rows to Q
//   V2 [J][npoly][N] 32-bit                   the float correction
struct GriCoreLayout { size_t UQ, UP, TQ, TP, Y2, ext, V2, end; };
inline GriCoreLayout gri_core_layout(int nl, int np, int npoly, bool with_u, size_t N, size_t J) {
    GriCoreLayout l; GriCarve c;
    l.UQ = c.take(with_u ? J * nl * N : 0); l.UP = c.take(with_u ? J * np * N : 0);
    l.TQ = c.take(J * npoly * nl * N); l.TP = c.take(J * npoly * np * N);
    l.Y2 = c.take(J * npoly * np * N); l.ext = c.take(J * npoly * nl * N);
    l.V2 = c.take((J * npoly * N + 1) / 2);
    l.end = c.at;
    return l;
}
inline size_t gri_words_per_ct(int nl, int np, int npoly, bool with_u, size_t N) {
    const size_t nt = (size_t)nl + np;
    return ((with_u ? nt : 0) + (size_t)npoly * nt + (size_t)npoly * np + (size_t)npoly * nl) * N + ((size_t)npoly * N + 1) / 2;
}
inline GriPlan gri_plan(int nct, int nl, int np, int npoly, bool with_u, size_t N, size_t budget_bytes) { return gri_plan_words(nct, gri_words_per_ct(nl, np, npoly, with_u, N), budget_bytes); }

// The coefficient decoder, J plaintexts: X [J][nl][N] (residues, then digits in place), out [J][N] doubles
struct GriDecodeLayout { size_t X, out, end; };
inline GriDecodeLayout gri_decode_layout(int nl, size_t N, size_t J) {
    GriDecodeLayout l; GriCarve c;
    l.X = c.take(J * nl * N); l.out = c.take(J * N);
    l.end = c.at;
    return l;
}
inline GriPlan gri_decode_plan(int nct, int nl, size_t N, size_t budget_bytes) { return gri_plan_words(nct, ((size_t)nl + 1) * N, budget_bytes); }

// The encoder, J vectors of n = N / 2 slots: A [J][n] points of 4 doubles, vals [J][n] doubles, R [J][nl][N] rows, band [J] doubles, flags: two 32-bit counters
struct GriEncodeLayout { size_t A, vals, R, band, flags, end; };
inline GriEncodeLayout gri_encode_layout(int nl, size_t N, size_t J) {
    const size_t n = N / 2;
    GriEncodeLayout l; GriCarve c;
    l.A = c.take(J * n * 4); l.vals = c.take(J * n); l.R = c.take(J * nl * N); l.band = c.take(J); l.flags = c.take(1);
    l.end = c.at;
    return l;
}
// 8 words a vector for the tail: one is its band, the counters take one word of a call, the rest is slack
inline GriPlan gri_encode_plan(int nvec, int nl, size_t N, size_t budget_bytes) { return gri_plan_words(nvec, N / 2 + 4 * (N / 2) + (size_t)nl * N + 8, budget_bytes); }

// The vector decoder, J plaintexts: A [J][n] points, Wd [J][N] pairs of doubles, X [J][nl][N], re [J][n] and im [J][n] doubles (the results of a host call)
struct GriVectorsLayout { size_t A, Wd, X, re, im, end; };
inline GriVectorsLayout gri_vectors_layout(int nl, size_t N, size_t J) {
    const size_t n = N / 2;
    GriVectorsLayout l; GriCarve c;
    l.A = c.take(J * n * 4); l.Wd = c.take(J * N * 2); l.X = c.take(J * nl * N); l.re = c.take(J * n); l.im = c.take(J * n);
    l.end = c.at;
    return l;
}
inline GriPlan gri_vectors_plan(int nct, int nl, size_t N, size_t budget_bytes) { return gri_plan_words(nct, (size_t)nl * N + 2 * N + 4 * (N / 2) + N, budget_bytes); }
