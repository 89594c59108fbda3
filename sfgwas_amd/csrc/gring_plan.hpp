// gring_plan.hpp - host-only planning of the general ring (gring.hip): the stage split of the two-launch transform and the digits of the hybrid key switch.
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
