// gring_matmul_plan.hpp - host-only planning of the general ring's matrix products (gring_matmul.hip): the shift table of a block row, the rotations a product
// needs, the bound after which the MAC folds its 128-bit sum, the launch caps, ONE layout of the products' workspace and ONE plan of its two chunks (over the
// ciphertexts and over a giant step's diagonals).  The executors take every pointer and every count from here.
// Standard library only (gring_arith.hpp is plain C++): tests/host/host_gring_mm_test.cpp holds it on the CPU.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>
#include "gring_arith.hpp"

// ---------------------------------------------------------------- shapes
// d = ceil(sqrt(slots)) (matmult.go:1249), by integers: the smallest d with d d >= slots
inline int mm_d(int slots) { int d = 1; while ((long long)d * d < slots) d++; return d; }
inline int mm_blocks(size_t rows, int slots) { return (int)((rows - 1) / (size_t)slots) + 1; }
inline int mm_block_len(size_t rows, int slots, int b) { const size_t lo = (size_t)b * slots, hi = lo + slots < rows ? lo + slots : rows; return (int)(hi - lo); }
// matmult.go:627-631 (getDiagBool) at index = -shift: does the diagonal of `shift` of an nr x nc block exist
inline bool mm_diag_exists(int nr, int nc, int slots, int shift) {
    const int index = shift == 0 ? 0 : slots - shift;
    return slots + 1 - nr <= index || index <= nc - 1;
}

// The shift table of operand block row bi (matmult.go:1329-1336): a shift is active when some block column has its diagonal;
// its baby = shift % d and its giant = shift / d then are.  rows x cols is the OPERAND (the resident matrix or its transpose).
struct MmShifts {
    int d = 0, slots = 0, nr = 0;
    std::vector<uint8_t> baby, giant, shift;                   // [d], [d], [slots]
    int babies_of(int g) const { int n = 0; for (int b = 0; b < d; b++) { const int s = g * d + b; if (s < slots && shift[s]) n++; } return n; }
};
inline MmShifts mm_shifts(size_t rows, size_t cols, int slots, int bi) {
    MmShifts t; t.d = mm_d(slots); t.slots = slots; t.nr = mm_block_len(rows, slots, bi);
    t.baby.assign(t.d, 0); t.giant.assign(t.d, 0); t.shift.assign(slots, 0);
    const int m_ct = mm_blocks(cols, slots);
    for (int s = 0; s < slots; s++) {
        bool any = false;
        for (int bj = 0; bj < m_ct && !any; bj++) any = mm_diag_exists(t.nr, mm_block_len(cols, slots, bj), slots, s);
        if (any) { t.baby[s % t.d] = 1; t.giant[s / t.d] = 1; t.shift[s] = 1; }
    }
    return t;
}
// the left rotations a product over block rows [b0, b1) needs keys for: the active babies > 0, then d g for the active giants g > 0
inline std::vector<int> mm_rotations(size_t rows, size_t cols, int slots, int b0, int b1, bool babies, bool giants) {
    const int d = mm_d(slots);
    std::vector<uint8_t> bb(d, 0), gg(d, 0);
    for (int bi = b0; bi < b1; bi++) { const MmShifts t = mm_shifts(rows, cols, slots, bi); for (int k = 0; k < d; k++) { bb[k] |= t.baby[k]; gg[k] |= t.giant[k]; } }
    std::vector<int> out;
    if (babies) for (int k = 1; k < d; k++) if (bb[k]) out.push_back(k);
    if (giants) for (int k = 1; k < d; k++) if (gg[k]) out.push_back(k * d);
    return out;
}

// ---------------------------------------------------------------- the fold
// A sum of `terms` products of canonical words is at most terms (q - 1)^2; started from a folded word (< q) it stays below 2^128 as long as
// q - 1 + terms (q - 1)^2 <= 2^128 - 1: terms <= fold_terms(q) = floor((2^128 - q) / (q - 1)^2).  55-bit words: 2^18 terms; 61-bit words: 64.
inline uint64_t mm_fold_terms(gr::u64 q) {
    const gr::u128 sq = (gr::u128)(q - 1) * (q - 1), top = (gr::u128)0 - (gr::u128)q;         // 2^128 - q
    const gr::u128 t = top / sq;
    return t > 0xFFFFFFFFu ? 0xFFFFFFFFu : (uint64_t)t;                                        // more terms than a product ever has
}
// One thread's sum of one accumulator, as the kernel runs it: add() before every term, word() at the end.  The result is the exact sum modulo q.
struct MmSum {
    gr::u128 S = 0;
    GR_HD void fold(gr::u64 q, gr::u64 uhi, gr::u64 ulo) { S = gr::barrett128((gr::u64)(S >> 64), (gr::u64)S, q, uhi, ulo); }
    GR_HD void mac(gr::u64 a, gr::u64 b) { S += (gr::u128)a * b; }
    GR_HD gr::u64 word(gr::u64 q, gr::u64 uhi, gr::u64 ulo) const { return gr::barrett128((gr::u64)(S >> 64), (gr::u64)S, q, uhi, ulo); }
};
// the walk of one thread over `n` terms with the fold every `fold` terms (the kernel's loop, on one accumulator): host restatement for the tests
template <class GetA, class GetB>
inline gr::u64 mm_sum_terms(size_t n, uint64_t fold, GetA A, GetB B, gr::u64 q, gr::u64 uhi, gr::u64 ulo) {
    MmSum s; uint64_t terms = 0;
    for (size_t k = 0; k < n; k++) {
        if (terms == fold) { s.fold(q, uhi, ulo); terms = 0; }
        s.mac(A(k), B(k)); terms++;
    }
    return s.word(q, uhi, ulo);
}

// ---------------------------------------------------------------- launch caps
constexpr int kMmTile = 4;                          // S_T: ciphertexts whose 2 S_T accumulators one MAC thread keeps (DESIGN.md section 18 has the compiler's figures)
constexpr size_t kMmVecCap = 4096;                  // diagonals of one encode batch: grid.z of the extraction and of the encoder's kernels
constexpr size_t kMmMacZCap = 32768;                // grid.z of one MAC launch: block columns x ciphertext tiles
constexpr size_t kMmSlackBytes = 256;               // reserved beyond the regions and never carved

// ---------------------------------------------------------------- workspace: one layout, one plan
// For a chunk of sc ciphertexts and batches of vc diagonals, at nl moduli of the dropped level and L = max_level rows of a plaintext, in 64-bit words:
//   rot  [sc][d][2][nl][N]   the rotation cache of one block row; the finalize reuses it for its rotated accumulators [sc][d - 1][2][L][N] (L <= nl)
//   acc  [m_ct][d][sc][2][L][N]  the accumulator of sfg_ring_matmul_dev (absent when the caller holds it)
//   dft  [vc][N / 2] points of four doubles    pt [vc][L][N]
//   vecs [vc] of 16 bytes    first [m_ct + 1] 32-bit    jobs [sc d] of 24 bytes (a rotation's source, index table and slot)    glist [d] 32-bit (the finalize's giants)
//   sums [vc] 32-bit    band [vc] doubles    flags: one word
struct MmLayout { size_t rot, acc, dft, pt, vecs, first, jobs, glist, sums, band, flags, end; };
struct MmCarve { size_t at = 0; size_t take(size_t words) { const size_t o = at; at += words; return o; } };
inline MmLayout mm_layout(int d, int nl, int L, int m_ct, size_t N, size_t sc, size_t vc, bool with_acc) {
    MmLayout l; MmCarve c;
    l.rot = c.take(sc * d * 2 * nl * N);
    l.acc = c.take(with_acc ? (size_t)m_ct * d * sc * 2 * L * N : 0);
    l.dft = c.take(vc * (N / 2) * 4); l.pt = c.take(vc * L * N);
    l.vecs = c.take(vc * 2); l.first = c.take(((size_t)m_ct + 2) / 2);
    l.jobs = c.take(sc * d * 3); l.glist = c.take(((size_t)d + 1) / 2);
    l.sums = c.take((vc + 1) / 2); l.band = c.take(vc); l.flags = c.take(1);
    l.end = c.at;
    return l;
}
struct MmPlan {
    size_t sc = 0, nsc = 0;                    // ciphertexts per chunk, chunks of s
    size_t vc = 0;                             // diagonals per encode batch at most
    size_t bytes = 0;                          // to reserve
    size_t first(size_t c) const { return c * sc; }
    size_t count(size_t c, size_t s) const { const size_t left = s - c * sc; return left < sc ? left : sc; }
    // a giant's nd diagonals in batches of vc
    size_t nbatches(size_t nd) const { return (nd + vc - 1) / vc; }
    size_t bfirst(size_t b) const { return b * vc; }
    size_t bcount(size_t b, size_t nd) const { const size_t left = nd - b * vc; return left < vc ? left : vc; }
};
// The diagonals of a batch come first: a whole giant's d m_ct (at most the cap) when they fit half the budget, else what half the budget holds, at least one.  What
// is left goes to the ciphertexts of a chunk, at least one (the budget is a preference, the allocation decides): every chunk of ciphertexts encodes the diagonals
// again, so a chunk is as large as the budget lets it be.
constexpr size_t kMmBudgetBytes = (size_t)32 << 30;       // the products' own default: one 8192 x 8192 block of PN14QP438 at s = 64 runs in one chunk (29 GiB)
inline size_t mm_bytes_per_ct(int d, int nl, int L, int m_ct, size_t N, bool with_acc) { return ((size_t)d * 2 * nl * N + (with_acc ? (size_t)m_ct * d * 2 * L * N : 0) + 3 * (size_t)d) * 8; }
inline size_t mm_bytes_per_vec(int L, size_t N) { return ((N / 2) * 4 + (size_t)L * N + 2 + 1 + 1) * 8; }
inline MmPlan mm_plan(size_t s, int d, int nl, int L, int m_ct, size_t N, bool with_acc, size_t budget_bytes) {
    MmPlan p;
    if (s == 0) return p;
    const size_t per_ct = mm_bytes_per_ct(d, nl, L, m_ct, N, with_acc), per_vec = mm_bytes_per_vec(L, N);
    size_t vc = (size_t)d * m_ct < kMmVecCap ? (size_t)d * m_ct : kMmVecCap;
    if (vc * per_vec > budget_bytes / 2) vc = budget_bytes / 2 / per_vec;
    if (vc < 1) vc = 1;
    p.vc = vc;
    const size_t left = budget_bytes > vc * per_vec ? budget_bytes - vc * per_vec : 0;
    size_t fit = left / per_ct;
    if (fit > s) fit = s;
    if (fit < 1) fit = 1;
    p.sc = fit; p.nsc = (s + fit - 1) / fit;
    p.bytes = mm_layout(d, nl, L, m_ct, N, p.sc, p.vc, with_acc).end * 8 + kMmSlackBytes;
    return p;
}
