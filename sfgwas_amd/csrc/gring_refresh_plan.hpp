// gring_refresh_plan.hpp - host-only planning of the general ring's collective bootstrap (gring_refresh.hip): for each of its two calls ONE layout - the offset
// of every region of a chunk of J ciphertexts, in 64-bit words - and ONE plan - the chunk, the chunks of a call and the bytes to reserve in the ring's wiping
// workspace (the rows hold mask + e and the masked plaintext).  The executors take every pointer and every count from here.
// Standard library only and on its own (like gring_io_plan.hpp): tests/host/host_gring_refresh_test.cpp holds it on the CPU.
#pragma once
#include <cstddef>

constexpr size_t kGrfMaxChunk = 1024;          // ciphertexts of one chunk at most: grid.z = chunk stays far below 65536; the transform splits its own rows
constexpr size_t kGrfSlackBytes = 64;          // reserved beyond the chunk and never carved

struct GrfCarve { size_t at = 0; size_t take(size_t words) { const size_t o = at; at += words; return o; } };
struct GrfPlan {
    size_t words_per_ct = 0;                   // the figure that sizes a chunk
    size_t chunk = 0, nchunks = 0;
    size_t bytes = 0;                          // of the chunk: chunk * words_per_ct * 8
    size_t reserve() const { return bytes ? bytes + kGrfSlackBytes : 0; }
    size_t first(size_t c) const { return c * chunk; }
    size_t count(size_t c, size_t n) const { const size_t left = n - c * chunk; return left < chunk ? left : chunk; }
};
// as many items as the budget holds, at least one (the budget is a preference, the allocation decides), at most the cap
inline GrfPlan grf_plan_words(size_t nct, size_t words, size_t budget_bytes) {
    GrfPlan p; p.words_per_ct = words;
    if (nct == 0 || words == 0) return p;
    size_t fit = budget_bytes / (words * 8);
    if (fit > kGrfMaxChunk) fit = kGrfMaxChunk;
    if (fit > nct) fit = nct;
    if (fit < 1) fit = 1;
    p.chunk = fit; p.nchunks = (nct + fit - 1) / fit; p.bytes = fit * words * 8;
    return p;
}

// Share generation, J ciphertexts at nl = level + 1 of nq moduli:  R0 [J][nl][N] (mask + e0, then its transform)   R1 [J][nq][N] (mask' + e1, then its transform)
struct GrfSharesLayout { size_t R0, R1, end; };
inline GrfSharesLayout grf_shares_layout(int nl, int nq, size_t N, size_t J) {
    GrfSharesLayout l; GrfCarve c;
    l.R0 = c.take(J * nl * N); l.R1 = c.take(J * nq * N);
    l.end = c.at;
    return l;
}
inline GrfPlan grf_shares_plan(size_t nct, int nl, int nq, size_t N, size_t budget_bytes) { return grf_plan_words(nct, ((size_t)nl + nq) * N, budget_bytes); }

// The finish.  ny rows of x a ciphertext are formed anew: the nq - nl moduli above the level in the unscaled form (rows below it are c0 + h0 themselves), all nq in
// the target-scale form.  ny == 0 (unscaled at the top level): nothing is carved and no workspace is reserved.
//   X [J][nl][N]   c0 + h0, its inverse transform, then the mixed-radix digits in place
//   Y [J][ny][N]   the new rows, then their transform
//   S [J][N] bytes the sign of every coefficient (unscaled form: decided once, read by every new row), N / 8 words a ciphertext
struct GrfFinishLayout { size_t X, Y, S, end; };
inline int grf_new_rows(int nl, int nq, bool scaled) { return scaled ? nq : nq - nl; }
inline GrfFinishLayout grf_finish_layout(int nl, int nq, bool scaled, size_t N, size_t J) {
    const size_t ny = (size_t)grf_new_rows(nl, nq, scaled);
    GrfFinishLayout l; GrfCarve c;
    l.X = c.take(ny ? J * nl * N : 0); l.Y = c.take(J * ny * N); l.S = c.take(ny && !scaled ? J * (N / 8) : 0);
    l.end = c.at;
    return l;
}
inline size_t grf_finish_words(int nl, int nq, bool scaled, size_t N) {
    const size_t ny = (size_t)grf_new_rows(nl, nq, scaled);
    return ny ? ((size_t)nl + ny) * N + (scaled ? 0 : N / 8) : 0;
}
// ny == 0 still runs in chunks (of the cap): one element-wise launch each
inline GrfPlan grf_finish_plan(size_t nct, int nl, int nq, bool scaled, size_t N, size_t budget_bytes) {
    const size_t w = grf_finish_words(nl, nq, scaled, N);
    if (w) return grf_plan_words(nct, w, budget_bytes);
    GrfPlan p;
    if (nct == 0) return p;
    p.chunk = nct < kGrfMaxChunk ? nct : kGrfMaxChunk; p.nchunks = (nct + p.chunk - 1) / p.chunk;
    return p;
}
