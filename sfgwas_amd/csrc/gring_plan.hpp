// gring_plan.hpp - host-only planning of the general ring (gring.hip): the stage split of the two-launch transform, the digits of the hybrid key switch, the
// launch caps, and the layout and chunk plan of the evaluator's two workspaces (key switch, rescale).
// Standard library only (like mm_plan.hpp): tests/host/host_gring_test.cpp holds it on the CPU.
#pragma once
#include <cstddef>

// The transform of a row of N = 2^logN words is two launches that split the logN radix-2 stages as logN = a + b, a, b <= 8.  Seen as a [2^a][2^b] matrix, the
// `a` stages of stride >= 2^b join words of one column (the strided "columns" pass) and the `b` stages of stride < 2^b stay inside one row of 2^b adjacent
// words (the contiguous pass).  Forward runs columns then contiguous, inverse the other way round.  Every workgroup of either pass owns one tile of
// kTileWords words in LDS (32 KiB), read once and written once: a row crosses HBM twice per transform.
//   columns pass:    2^a rows of a run of col_run = kTileWords / 2^a adjacent columns (col_run * 8 >= 128 contiguous bytes per row segment)
//   contiguous pass: chunks = kTileWords / 2^b adjacent sub-transforms of 2^b words (one contiguous 32 KiB stretch)
// logN 12..14 would fit one launch's LDS (32..128 KiB a row) only up to 13 under the 64 KiB bound; one code path for every logN was preferred to a second kernel.
struct GrNttPlan {
    static constexpr int kTileWords = 4096, kThreads = 256;
    int logN = 0, a = 0, b = 0;
    int col_run = 0;          // adjacent columns per workgroup of the columns pass
    int chunks = 0;           // sub-transforms per workgroup of the contiguous pass
    int tiles_per_row = 0;    // grid.x of both passes (grid.y = rows)
    size_t col_stride = 0;    // words between two rows of the columns pass: 2^b
    size_t lds_bytes = 0;
    bool ok = false;
};
inline GrNttPlan gr_ntt_plan(int logN) {
    GrNttPlan p;
    if (logN < 12 || logN > 16) return p;
    p.logN = logN; p.a = logN / 2; p.b = logN - p.a;                       // 12: 6+6, 13: 6+7, 14: 7+7, 15: 7+8, 16: 8+8
    p.col_run = GrNttPlan::kTileWords >> p.a; p.chunks = GrNttPlan::kTileWords >> p.b;
    p.tiles_per_row = (1 << logN) / GrNttPlan::kTileWords;
    p.col_stride = (size_t)1 << p.b;
    p.lds_bytes = (size_t)GrNttPlan::kTileWords * 8;
    p.ok = p.a <= 8 && p.b <= 8 && p.col_run >= 16 && p.col_run <= (1 << p.b) && p.chunks >= 1;
    return p;
}

// digits of the hybrid key switch at a level: alpha = np moduli per digit, beta = ceil((level + 1) / alpha) digits, the last one short
struct GrDigits { int alpha = 0, beta = 0, nl = 0; int start(int i) const { return i * alpha; } int len(int i) const { int e = (i + 1) * alpha; return (e > nl ? nl : e) - i * alpha; } };
inline GrDigits gr_digits(int level, int np) { GrDigits d; d.alpha = np; d.nl = level + 1; d.beta = (d.nl + np - 1) / np; return d; }

// ---------------------------------------------------------------- launch caps and the one way they are applied
constexpr size_t kGrLaunchCap = 32768;              // rows of one transform launch (grid.y) and items of one grid.z of the io kernels
constexpr size_t kGrEwCap = kGrLaunchCap / 2;       // ciphertexts of one element-wise launch: grid.z = 2 per ciphertext
constexpr size_t kGrKsJobCap = 32767;               // key switches of one chunk: the finish runs grid.z = 2 per job, below 65536
inline size_t gr_from_mont_cap(int nmod) { return kGrLaunchCap / (size_t)nmod * (size_t)nmod; }    // whole groups of nmod rows: blockIdx.y % nmod stays the row's modulus
// f(first, count) on consecutive pieces of at most cap items; stops at the first non-zero result and returns it
template <class F> inline int gr_split(size_t n, size_t cap, F f) {
    for (size_t i0 = 0; i0 < n; i0 += cap) { const int rc = f(i0, n - i0 < cap ? n - i0 : cap); if (rc) return rc; }
    return 0;
}

// ---------------------------------------------------------------- workspaces: one layout and one plan each
// A layout gives the offset of every region of a chunk of J items in 64-bit words, in order, and `end`; a plan gives the chunk and the bytes to reserve.  The
// executors take every pointer from the layout.  Items of one chunk are as many as the budget holds, at least one (the budget is a preference, the allocation
// decides), at most the launch cap.
struct GrCarve { size_t at = 0; size_t take(size_t words) { const size_t o = at; at += words; return o; } };
struct GrChunks {
    size_t per_item = 0;                       // bytes that size a chunk
    size_t chunk = 0, nchunks = 0;
    size_t bytes = 0;                          // to reserve: chunk * per_item + slack
    size_t first(size_t c) const { return c * chunk; }
    size_t count(size_t c, size_t n) const { const size_t left = n - c * chunk; return left < chunk ? left : chunk; }
};
inline GrChunks gr_chunks(size_t n, size_t per_item, size_t cap, size_t budget_bytes, size_t slack_bytes) {
    GrChunks p; p.per_item = per_item;
    if (n == 0) return p;
    size_t fit = budget_bytes / per_item;
    if (fit > cap) fit = cap;
    if (fit > n) fit = n;
    if (fit < 1) fit = 1;
    p.chunk = fit; p.nchunks = (n + fit - 1) / fit; p.bytes = fit * per_item + slack_bytes;
    return p;
}

// The key switch, J jobs at nl = level + 1 moduli of Q, np of P, nt = nl + np targets, beta digits:
//   c2 [J][nl][N]  Y [J][nl][N]  ext [J][beta][nt][N]  accQ [J][2][nl][N]  accP [J][2][np][N]  Y2 [J][2][np][N]  ext2 [J][2][nl][N]
//   V [J][beta][N] and V2 [J][2][N] 32-bit (N is even: both start on a word)  jobs [J] of kGrJobBytes
constexpr size_t kGrJobBytes = 24;                  // sizeof(GrJob), asserted in gring_dev.hpp
constexpr size_t kGrKsSlackBytes = 256;             // reserved beyond the chunk and never carved
struct GrKsLayout { size_t c2, Y, ext, accQ, accP, Y2, ext2, V, V2, jobs, end; };
inline GrKsLayout gr_ks_layout(int level, int np, size_t N, size_t J) {
    const GrDigits d = gr_digits(level, np); const size_t nl = d.nl, nt = nl + np, beta = d.beta;
    GrKsLayout l; GrCarve c;
    l.c2 = c.take(J * nl * N); l.Y = c.take(J * nl * N); l.ext = c.take(J * beta * nt * N); l.accQ = c.take(J * 2 * nl * N); l.accP = c.take(J * 2 * np * N);
    l.Y2 = c.take(J * 2 * np * N); l.ext2 = c.take(J * 2 * nl * N);
    l.V = c.take(J * beta * N / 2); l.V2 = c.take(J * 2 * N / 2);
    l.jobs = c.take(J * kGrJobBytes / 8);
    l.end = c.at;
    return l;
}
// words of one job.  The last term sizes V and V2: (beta + 2) / 2 rows are carved, (beta + 3) / 2 + 1 rows are counted - up to a row and a half of slack a job
inline size_t gr_ks_words_per_job(int level, int np, size_t N) {
    const GrDigits d = gr_digits(level, np); const size_t nl = d.nl, nt = nl + np, beta = d.beta;
    return (nl * 2 + beta * nt + 2 * nl + 2 * np + 2 * np + 2 * nl + (beta + 2 + 1) / 2 + 1) * N;
}
inline GrChunks gr_ks_plan(size_t njobs, int level, int np, size_t N, size_t budget_bytes) {
    return gr_chunks(njobs, gr_ks_words_per_job(level, np, N) * 8 + kGrJobBytes, kGrKsJobCap, budget_bytes, kGrKsSlackBytes);
}

// The rescale, J ciphertexts at level >= 1: T [J][2][N] the last modulus' rows, tmp [J][2][level][N] their image at the others.  No slack.
struct GrRescaleLayout { size_t T, tmp, end; };
inline GrRescaleLayout gr_rescale_layout(int level, size_t N, size_t J) {
    GrRescaleLayout l; GrCarve c;
    l.T = c.take(J * 2 * N); l.tmp = c.take(J * 2 * (size_t)level * N);
    l.end = c.at;
    return l;
}
inline GrChunks gr_rescale_plan(size_t nct, int level, size_t N, size_t budget_bytes) { return gr_chunks(nct, (size_t)2 * (level + 1) * N * 8, kGrEwCap, budget_bytes, 0); }
