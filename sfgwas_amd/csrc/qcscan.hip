// qcscan.hip — quality control on the resident genotype matrix: the three local scans of gwas/qualcontrol.go (SNPMissFilter :339-378,
// IndividualMissAndHetFilters :36-81, SNPMAFAndHWEFilters :416-463) as ONE pass over the matrix bytes, and the row / column filter that follows them
// (FilterMatrixFile, utilities.go:154 -> scripts/filterMatrix.py) as a resident-to-resident gather.
//
// The scan.  A workgroup of 256 threads takes a tile of 4096 columns x rc rows (rc <= 1984, a multiple of 8): a thread owns 16 columns - one 16-byte load per
// row of an int8 matrix, one dword of sixteen 2-bit codes of a packed one - so a row of the tile is one fully coalesced load of the workgroup, no two threads share a
// column, and a row's counts are reduced over 4096 columns before they meet a global atomic.
//   columns  per thread and cohort three counters per column (value 1, value 2, missing; value 0 is what is left of the kept rows and is derived on the host),
//            kept in lanes as narrow as the data: 8-bit lanes for int8 (the mask of a byte test is added as it is), 2-bit -> 4-bit -> 8-bit lanes for packed codes.
//            Every lane width is widened before it can wrap: 2-bit after 3 rows, 4-bit after 8, 8-bit after 31 batches of 8 rows = 248, 16-bit lanes hold the
//            whole chunk (rc <= 1984).  At the end the 16-bit lanes go through LDS, so that a wave adds 64 consecutive columns with one atomic instruction.
//   rows     popcounts of the missing / het masks, (miss | het << 16) per thread and row; eight rows at a time are summed over the wave by a transposing
//            butterfly (10 lane exchanges for 8 rows), lanes 0..7 add the wave's totals into the chunk's row table in LDS, and the table leaves with one atomic
//            per row, count and 4096-column tile.
// All partial counts are integers combined with atomicAdd on uint32: the result does not depend on the order.  Temporaries are O(nrow + ncol).
#include "common.hpp"
#include "kernels.hpp"
#include <algorithm>

namespace {
constexpr int QC_COLS = 4096;                         // columns of a tile = 256 threads x 16
constexpr int QC_BATCH = 8;                           // rows loaded before any is counted
constexpr int QC_FLUSH = 31;                          // batches between two widenings of the 8-bit lanes: 31 * 8 = 248 <= 255
constexpr int QC_RC_MAX = QC_BATCH * QC_FLUSH * 8;    // 1984 rows per chunk at most: the 16-bit lanes and the packed row table (counts <= 4096) cannot wrap
constexpr int QC_RC_MIN = 256;
constexpr int QC_LDS = QC_COLS + QC_COLS / 16;           // the column exchange, one pad word per 16: a thread's 16 words start on its own bank

struct QcArgs {
    const void *dev; size_t nrow, ncol, ld;           // ld in bytes
    const uint8_t *rowf, *colf, *ctrl;                // device copies of the filters (nullptr = keep all / no controls)
    unsigned *col_out;                                // [2][3][ncol]: cohort, {value 1, value 2, missing}
    unsigned *row_miss, *row_het, *bad;
    unsigned rc, strips;                              // rows per chunk; 4096-column strips.  The grid is flat: block = chunk * strips + strip
};

// v[j]: this lane's packed count of row j of a batch -> the wave's total of row (lane & 7), valid in every lane
__device__ __forceinline__ unsigned wave_rows8(const unsigned (&v)[8], int lane) {
    unsigned w[4], u[2];
#pragma unroll
    for (int k = 0; k < 4; k++) { const bool hi = lane & 1; w[k] = (hi ? v[2 * k + 1] : v[2 * k]) + __shfl_xor(hi ? v[2 * k] : v[2 * k + 1], 1); }
#pragma unroll
    for (int k = 0; k < 2; k++) { const bool hi = lane & 2; u[k] = (hi ? w[2 * k + 1] : w[2 * k]) + __shfl_xor(hi ? w[2 * k] : w[2 * k + 1], 2); }
    const bool hi = lane & 4;
    unsigned t = (hi ? u[1] : u[0]) + __shfl_xor(hi ? u[0] : u[1], 4);
    t += __shfl_xor(t, 8); t += __shfl_xor(t, 16); t += __shfl_xor(t, 32);
    return t;
}
struct Acc16 { unsigned v[2][3][4][2]; };             // [cohort][counter][dword of 8-bit lanes][even / odd byte]: two 16-bit lanes each
__device__ __forceinline__ void widen8(unsigned (&a8)[2][3][4], Acc16 &a16, bool hasc) {
#pragma unroll
    for (int c = 0; c < 2; c++) {
        if (c && !hasc) continue;
#pragma unroll
        for (int k = 0; k < 3; k++)
#pragma unroll
            for (int q = 0; q < 4; q++) { const unsigned a = a8[c][k][q]; a16.v[c][k][q][0] += a & 0x00FF00FFu; a16.v[c][k][q][1] += (a >> 8) & 0x00FF00FFu; a8[c][k][q] = 0; }
    }
}
// the thread's 16 columns x 6 counters leave through LDS: 64 consecutive columns per atomic wave-instruction.  Word n of the tile lies at n + n / 16, so neither
// the write (lane stride 17) nor the read (consecutive) piles lanes onto one bank.  PACKED selects which column a lane stands for:
// int8: dword q, byte b = column 4 q + b; packed (after the two widenings): dword s, byte b = column 4 b + s.
template <bool PACKED>
__device__ __forceinline__ void flush_cols(const Acc16 &a16, unsigned *lds, const QcArgs &a, size_t c0, int tid, bool hasc) {
#pragma unroll
    for (int c = 0; c < 2; c++) {
        if (c && !hasc) continue;
#pragma unroll
        for (int k = 0; k < 3; k++) {
#pragma unroll
            for (int q = 0; q < 4; q++)
#pragma unroll
                for (int h = 0; h < 2; h++)
#pragma unroll
                    for (int t = 0; t < 2; t++) {
                        const int b = 2 * t + h, col = PACKED ? 4 * b + q : 4 * q + b;
                        lds[tid * 17 + col] = (a16.v[c][k][q][h] >> (16 * t)) & 0xFFFFu;
                    }
            __syncthreads();
            unsigned *dst = a.col_out + (size_t)(c * 3 + k) * a.ncol;
#pragma unroll 4
            for (int i = 0; i < 16; i++) { const int n = i * 256 + tid; const unsigned v = lds[n + (n >> 4)]; const size_t j = c0 + (size_t)i * 256 + tid; if (v && j < a.ncol) atomicAdd(&dst[j], v); }
            __syncthreads();
        }
    }
}
__device__ __forceinline__ void flush_rows(const unsigned *rowacc, const QcArgs &a, size_t r0, size_t r1, int tid) {
    for (size_t i = tid; r0 + i < r1; i += 256) {
        const unsigned v = rowacc[i];
        if ((v & 0xFFFFu) && a.row_miss) atomicAdd(&a.row_miss[r0 + i], v & 0xFFFFu);
        if ((v >> 16) && a.row_het) atomicAdd(&a.row_het[r0 + i], v >> 16);
    }
}

// int8 matrix.  grid ceil(ncol / 4096) * ceil(nrow / rc), flat, so the number of row chunks is not held to a grid dimension.  A kept byte w (column mask cm: 0x01 per kept column of the dword):
//   missing = bit 7;  among the others: value 1 = bit 0, value 2 = bit 1 (exact for values 0..2), value above 2 <=> (w & 0x7F) + 0x7D reaches bit 7
template <bool ROWS, bool COLS, bool HASC>
__global__ void __launch_bounds__(256) k_qc_scan_i8(const QcArgs a) {
    __shared__ unsigned lds[QC_LDS];
    __shared__ unsigned rowacc[QC_RC_MAX];
    const int tid = threadIdx.x, lane = tid & 63;
    const int8_t *g = (const int8_t *)a.dev;
    const size_t bx = blockIdx.x % a.strips, by = blockIdx.x / a.strips;
    const size_t c0 = bx * QC_COLS, col = c0 + (size_t)tid * 16, r0 = by * a.rc, r1 = r0 + a.rc < a.nrow ? r0 + a.rc : a.nrow;
    if (ROWS) for (unsigned i = tid; i < a.rc; i += 256) rowacc[i] = 0;
    unsigned cm[4] = {0, 0, 0, 0}, cm7[4];
    for (int k = 0; k < 16; k++) if (col + k < a.ncol && (!a.colf || a.colf[col + k])) cm[k >> 2] |= 1u << (8 * (k & 3));
#pragma unroll
    for (int q = 0; q < 4; q++) cm7[q] = cm[q] << 7;
    const bool vec = col + 16 <= a.ncol && ((reinterpret_cast<uintptr_t>(g) | a.ld) & 15) == 0;
    auto load = [&](size_t i) -> uint4 {
        if (vec) return *reinterpret_cast<const uint4 *>(g + i * a.ld + col);
        uint4 v = make_uint4(0, 0, 0, 0);
        if (col < a.ncol) { int8_t b[16]; for (int k = 0; k < 16; k++) b[k] = col + k < a.ncol ? g[i * a.ld + col + k] : (int8_t)0; v = *reinterpret_cast<uint4 *>(b); }
        return v;
    };
    unsigned a8[2][3][4]; Acc16 a16; unsigned nbad = 0;
#pragma unroll
    for (int c = 0; c < 2; c++)
#pragma unroll
        for (int k = 0; k < 3; k++)
#pragma unroll
            for (int q = 0; q < 4; q++) { a8[c][k][q] = 0; a16.v[c][k][q][0] = a16.v[c][k][q][1] = 0; }
    __syncthreads();
    int nb = 0;
    for (size_t rb = r0; rb < r1; rb += QC_BATCH) {
        uint4 v[QC_BATCH]; bool keep[QC_BATCH], ct[QC_BATCH]; bool any = false;
#pragma unroll
        for (int j = 0; j < QC_BATCH; j++) {
            const size_t r = rb + j;
            keep[j] = r < r1 && (!a.rowf || a.rowf[r]);
            ct[j] = HASC && keep[j] && a.ctrl[r];
            any |= keep[j];
            v[j] = keep[j] ? load(r) : make_uint4(0, 0, 0, 0);
        }
        if (!any) continue;                                      // (uniform; nothing was added to any lane)
        unsigned rv[QC_BATCH];
#pragma unroll
        for (int j = 0; j < QC_BATCH; j++) {
            rv[j] = 0;
            if (!keep[j]) continue;
            const unsigned w4[4] = {v[j].x, v[j].y, v[j].z, v[j].w};
            unsigned miss = 0, het = 0;
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const unsigned w = w4[q], neg7 = w & cm7[q], ok7 = cm7[q] ^ neg7, okm = ok7 >> 7;
                const unsigned b0 = w & okm, b1 = (w >> 1) & okm;
                nbad += __popc(((w & 0x7F7F7F7Fu) + 0x7D7D7D7Du) & ok7);
                if (ROWS) { miss += __popc(neg7); het += __popc(b0); }
                if (COLS) {
                    const unsigned neg = neg7 >> 7;
                    a8[0][0][q] += b0; a8[0][1][q] += b1; a8[0][2][q] += neg;
                    if (HASC && ct[j]) { a8[1][0][q] += b0; a8[1][1][q] += b1; a8[1][2][q] += neg; }
                }
            }
            rv[j] = miss | het << 16;
        }
        if (ROWS) { const unsigned t = wave_rows8(rv, lane); if (lane < 8 && t) atomicAdd(&rowacc[rb - r0 + lane], t); }
        if (COLS && ++nb == QC_FLUSH) { widen8(a8, a16, HASC); nb = 0; }
    }
    if (nbad) atomicAdd(a.bad, nbad);
    __syncthreads();
    if (ROWS) flush_rows(rowacc, a, r0, r1, tid);
    if (COLS) { widen8(a8, a16, HASC); flush_cols<false>(a16, lds, a, c0, tid, HASC); }
}

// 2-bit packed matrix, scanned in place: thread = one dword = 16 codes per row.  lo = x & 0x5555.., hi = (x >> 1) & 0x5555..: missing = lo & hi, value 1 = lo
// alone, value 2 = hi alone; cm has 01 in the field of every kept column (padding codes past ncol are never kept).
template <bool ROWS, bool COLS, bool HASC>
__global__ void __launch_bounds__(256) k_qc_scan_p2(const QcArgs a) {
    __shared__ unsigned lds[QC_LDS];
    __shared__ unsigned rowacc[QC_RC_MAX];
    const int tid = threadIdx.x, lane = tid & 63;
    const unsigned *g = (const unsigned *)a.dev;
    const size_t bx = blockIdx.x % a.strips, by = blockIdx.x / a.strips;
    const size_t ldw = a.ld / 4, wi = bx * 256 + tid, c0 = bx * QC_COLS, col = wi * 16;
    const size_t r0 = by * a.rc, r1 = r0 + a.rc < a.nrow ? r0 + a.rc : a.nrow;
    if (ROWS) for (unsigned i = tid; i < a.rc; i += 256) rowacc[i] = 0;
    unsigned cm = 0;
    for (int k = 0; k < 16; k++) if (col + k < a.ncol && (!a.colf || a.colf[col + k])) cm |= 1u << (2 * k);
    const bool inside = wi < ldw && col < a.ncol;
    unsigned a2[2][3], a4[2][3][2], a8[2][3][4]; Acc16 a16;
#pragma unroll
    for (int c = 0; c < 2; c++)
#pragma unroll
        for (int k = 0; k < 3; k++) {
            a2[c][k] = 0; a4[c][k][0] = a4[c][k][1] = 0;
#pragma unroll
            for (int q = 0; q < 4; q++) { a8[c][k][q] = 0; a16.v[c][k][q][0] = a16.v[c][k][q][1] = 0; }
        }
    __syncthreads();
    int nb = 0;
    for (size_t rb = r0; rb < r1; rb += QC_BATCH) {
        unsigned x[QC_BATCH]; bool keep[QC_BATCH], ct[QC_BATCH]; bool any = false;
#pragma unroll
        for (int j = 0; j < QC_BATCH; j++) {
            const size_t r = rb + j;
            keep[j] = r < r1 && (!a.rowf || a.rowf[r]);
            ct[j] = HASC && keep[j] && a.ctrl[r];
            any |= keep[j];
            x[j] = keep[j] && inside ? g[r * ldw + wi] : 0u;
        }
        if (!any) continue;
        unsigned rv[QC_BATCH];
#pragma unroll
        for (int j = 0; j < QC_BATCH; j++) {
            rv[j] = 0;
            if (keep[j]) {
                const unsigned lo = x[j] & 0x55555555u, hi = (x[j] >> 1) & 0x55555555u, t = lo & hi;
                const unsigned ms = t & cm, on = (lo ^ t) & cm, tw = (hi ^ t) & cm;
                if (ROWS) rv[j] = __popc(ms) | __popc(on) << 16;
                if (COLS) {
                    a2[0][0] += on; a2[0][1] += tw; a2[0][2] += ms;
                    if (HASC && ct[j]) { a2[1][0] += on; a2[1][1] += tw; a2[1][2] += ms; }
                }
            }
            if (COLS && (j == 2 || j == 5 || j == 7)) {            // 2-bit lanes hold at most 3 rows -> 4-bit lanes: field m of a4[e] = column 2 m + e
#pragma unroll
                for (int c = 0; c < 2; c++) {
                    if (c && !HASC) continue;
#pragma unroll
                    for (int k = 0; k < 3; k++) { const unsigned v = a2[c][k]; a4[c][k][0] += v & 0x33333333u; a4[c][k][1] += (v >> 2) & 0x33333333u; a2[c][k] = 0; }
                }
            }
        }
        if (COLS) {                                                // 4-bit lanes hold the 8 rows of a batch -> 8-bit lanes: byte b of a8[e + 2 f] = column 4 b + 2 f + e
#pragma unroll
            for (int c = 0; c < 2; c++) {
                if (c && !HASC) continue;
#pragma unroll
                for (int k = 0; k < 3; k++)
#pragma unroll
                    for (int e = 0; e < 2; e++) { const unsigned v = a4[c][k][e]; a8[c][k][e] += v & 0x0F0F0F0Fu; a8[c][k][e + 2] += (v >> 4) & 0x0F0F0F0Fu; a4[c][k][e] = 0; }
            }
        }
        if (ROWS) { const unsigned t = wave_rows8(rv, lane); if (lane < 8 && t) atomicAdd(&rowacc[rb - r0 + lane], t); }
        if (COLS && ++nb == QC_FLUSH) { widen8(a8, a16, HASC); nb = 0; }
    }
    __syncthreads();
    if (ROWS) flush_rows(rowacc, a, r0, r1, tid);
    if (COLS) { widen8(a8, a16, HASC); flush_cols<true>(a16, lds, a, c0, tid, HASC); }
}

template <bool ROWS, bool COLS, bool HASC>
void launch_qc(const QcArgs &a, bool packed, dim3 grid, hipStream_t st) {
    if (packed) hipLaunchKernelGGL((k_qc_scan_p2<ROWS, COLS, HASC>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((k_qc_scan_i8<ROWS, COLS, HASC>), grid, dim3(256), 0, st, a);
}

// ---- the filtered matrix.  ridx / cidx: the kept rows / columns in order (nullptr = all).  grid (ceil(width / 256), min(nr, 65535)): the rows are walked with a
// stride of gridDim.y, so any number of rows is served
__global__ void __launch_bounds__(256) k_filter_i8(const int8_t *in, size_t ld, const unsigned *ridx, const unsigned *cidx, size_t nr, size_t nc, int8_t *out) {
    const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= nc) return;
    const size_t sc = cidx ? cidx[c] : c;
    for (size_t r = blockIdx.y; r < nr; r += gridDim.y) out[r * nc + c] = in[(size_t)(ridx ? ridx[r] : r) * ld + sc];
}
// packed -> packed: thread = one output dword = 16 kept columns, each code fetched from its source byte; padding codes are 0
__global__ void __launch_bounds__(256) k_filter_p2(const uint8_t *in, size_t ld, const unsigned *ridx, const unsigned *cidx, size_t nr, size_t nc, unsigned *out, size_t ldw) {
    const size_t w = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= ldw) return;
    unsigned sc[16]; int n = 0;
    for (; n < 16 && w * 16 + n < nc; n++) sc[n] = cidx ? cidx[w * 16 + n] : (unsigned)(w * 16 + n);
    for (size_t r = blockIdx.y; r < nr; r += gridDim.y) {
        const uint8_t *row = in + (size_t)(ridx ? ridx[r] : r) * ld;
        unsigned v = 0;
#pragma unroll
        for (int k = 0; k < 16; k++) if (k < n) v |= ((row[sc[k] >> 2] >> (2 * (sc[k] & 3))) & 3u) << (2 * k);
        out[r * ldw + w] = v;
    }
}
}  // namespace

extern "C" int sfg_geno_qc_scan(sfg_ctx *ctx, const sfg_geno *g, const uint8_t *row_filter, const uint8_t *col_filter, const uint8_t *row_ctrl,
                                uint32_t *col_counts_host, uint32_t *row_miss_host, uint32_t *row_het_host) {
    if (!ctx) return 1;
    if (!g) SFG_FAIL(ctx, "sfg_geno_qc_scan: null matrix");
    if (!col_counts_host && !row_miss_host && !row_het_host) SFG_FAIL(ctx, "sfg_geno_qc_scan: no output requested");
    const size_t nrow = g->nrow, ncol = g->ncol;
    if (nrow >= (1ULL << 32) || ncol >= (1ULL << 32)) SFG_FAIL(ctx, "sfg_geno_qc_scan: dimension too large for 32-bit counts");
    if (g->packed && ((reinterpret_cast<uintptr_t>(g->dev) | g->ld) & 3)) SFG_FAIL(ctx, "sfg_geno_qc_scan: packed matrix is not dword aligned");
    if (!nrow || !ncol) {                                        // nothing to look at: the counts are zeros (col_counts has no entries when ncol == 0)
        if (col_counts_host) std::fill(col_counts_host, col_counts_host + 8 * ncol, 0u);
        if (row_miss_host) std::fill(row_miss_host, row_miss_host + nrow, 0u);
        if (row_het_host) std::fill(row_het_host, row_het_host + nrow, 0u);
        return 0;
    }
    SFG_HIP(ctx, hipSetDevice(ctx->device));
    ApiScope scope(ctx);
    const bool want_rows = row_miss_host || row_het_host, want_cols = col_counts_host != nullptr, hasc = want_cols && row_ctrl;
    // one scratch buffer, O(nrow + ncol): [bad, pad][6 ncol counts][2 nrow counts] as uint32, then the three filters as bytes
    const size_t nwords = 4 + 6 * ncol + 2 * nrow, bytes = nwords * 4 + 2 * nrow + ncol;
    unsigned *buf = nullptr;
    SFG_TRY(sfg_scratch(ctx, "qc.scan", bytes, (void **)&buf));
    uint8_t *fb = (uint8_t *)(buf + nwords);
    QcArgs a;
    a.dev = g->dev; a.nrow = nrow; a.ncol = ncol; a.ld = g->ld;
    a.bad = buf; a.col_out = buf + 4; a.row_miss = buf + 4 + 6 * ncol; a.row_het = a.row_miss + nrow;
    a.rowf = row_filter ? fb : nullptr; a.ctrl = hasc ? fb + nrow : nullptr; a.colf = col_filter ? fb + 2 * nrow : nullptr;
    SFG_HIP(ctx, hipMemsetAsync(buf, 0, nwords * 4, ctx->stream));
    if (row_filter) SFG_HIP(ctx, hipMemcpyAsync(fb, row_filter, nrow, hipMemcpyHostToDevice, ctx->stream));
    if (hasc) SFG_HIP(ctx, hipMemcpyAsync(fb + nrow, row_ctrl, nrow, hipMemcpyHostToDevice, ctx->stream));
    if (col_filter) SFG_HIP(ctx, hipMemcpyAsync(fb + 2 * nrow, col_filter, ncol, hipMemcpyHostToDevice, ctx->stream));
    // rows per chunk: as many as the narrow lanes allow once the grid has a few thousand workgroups
    const size_t strips = (ncol + QC_COLS - 1) / QC_COLS, want = (4096 + strips - 1) / strips;
    size_t rc = ((nrow + want - 1) / want + 7) / 8 * 8;
    rc = std::min<size_t>(QC_RC_MAX, std::max<size_t>(QC_RC_MIN, rc));
    a.rc = (unsigned)rc; a.strips = (unsigned)strips;
    const size_t chunks = (nrow + rc - 1) / rc;                  // < 2^24 and strips < 2^20: the flat grid passes 2^31 - 1 only past 2^50 matrix bytes
    if (strips * chunks > 0x7FFFFFFFu) SFG_FAIL(ctx, "sfg_geno_qc_scan: matrix too large for one launch");
    const dim3 grid((unsigned)(strips * chunks));
    const bool p = g->packed; hipStream_t st = ctx->stream;
    if (want_rows && want_cols) { if (hasc) launch_qc<true, true, true>(a, p, grid, st); else launch_qc<true, true, false>(a, p, grid, st); }
    else if (want_cols) { if (hasc) launch_qc<false, true, true>(a, p, grid, st); else launch_qc<false, true, false>(a, p, grid, st); }
    else launch_qc<true, false, false>(a, p, grid, st);
    SFG_HIP(ctx, hipGetLastError());
    unsigned hbad = 0;
    std::vector<uint32_t> cnt(want_cols ? 6 * ncol : 0);
    SFG_HIP(ctx, hipMemcpyAsync(&hbad, a.bad, 4, hipMemcpyDeviceToHost, ctx->stream));
    if (want_cols) SFG_HIP(ctx, hipMemcpyAsync(cnt.data(), a.col_out, 6 * ncol * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (row_miss_host) SFG_HIP(ctx, hipMemcpyAsync(row_miss_host, a.row_miss, nrow * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (row_het_host) SFG_HIP(ctx, hipMemcpyAsync(row_het_host, a.row_het, nrow * 4, hipMemcpyDeviceToHost, ctx->stream));
    SFG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (hbad) SFG_FAIL(ctx, "sfg_geno_qc_scan: %u values above 2 at kept positions (genotypes are 0, 1, 2 or negative = missing)", hbad);
    if (want_cols) {
        // value 0 = the kept rows of the cohort that are neither 1, 2 nor missing (every kept value is one of the four once no value above 2 was seen)
        uint32_t kept[2] = {0, 0};
        for (size_t i = 0; i < nrow; i++) if (!row_filter || row_filter[i]) { kept[0]++; if (row_ctrl && row_ctrl[i]) kept[1]++; }
        for (int c = 0; c < 2; c++) {
            const uint32_t *n1 = cnt.data() + (size_t)(c * 3) * ncol, *n2 = n1 + ncol, *nm = n2 + ncol;
            uint32_t *o = col_counts_host + (size_t)c * 4 * ncol;
            for (size_t j = 0; j < ncol; j++) {
                const bool k = !col_filter || col_filter[j];
                o[j] = k ? kept[c] - n1[j] - n2[j] - nm[j] : 0; o[ncol + j] = n1[j]; o[2 * ncol + j] = n2[j]; o[3 * ncol + j] = nm[j];
            }
        }
    }
    return 0;
}

extern "C" int sfg_geno_filter(sfg_ctx *ctx, const sfg_geno *g, const uint8_t *row_filter, const uint8_t *col_filter, sfg_geno **out) {
    if (!ctx) return 1;
    if (!g || !out) SFG_FAIL(ctx, "sfg_geno_filter: null matrix / result pointer");
    *out = nullptr;
    if (g->nrow >= (1ULL << 32) || g->ncol >= (1ULL << 32)) SFG_FAIL(ctx, "sfg_geno_filter: dimension too large");
    std::vector<unsigned> idx;                                   // kept rows, then kept columns
    size_t nr = g->nrow, nc = g->ncol;
    if (row_filter) { for (size_t i = 0; i < g->nrow; i++) if (row_filter[i]) idx.push_back((unsigned)i); nr = idx.size(); }
    if (col_filter) { for (size_t j = 0; j < g->ncol; j++) if (col_filter[j]) idx.push_back((unsigned)j); nc = idx.size() - (row_filter ? nr : 0); }
    if (!nr || !nc) SFG_FAIL(ctx, "sfg_geno_filter: filters keep nothing (%zu rows, %zu columns)", nr, nc);
    SFG_HIP(ctx, hipSetDevice(ctx->device));
    ApiScope scope(ctx);
    unsigned *didx = nullptr;
    if (!idx.empty()) {
        SFG_TRY(sfg_scratch(ctx, "qc.idx", idx.size() * 4, (void **)&didx));
        SFG_HIP(ctx, hipMemcpyAsync(didx, idx.data(), idx.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    }
    const unsigned *ridx = row_filter ? didx : nullptr, *cidx = col_filter ? didx + (row_filter ? nr : 0) : nullptr;
    const size_t ldw = (nc + 15) / 16, width = g->packed ? ldw : nc;
    void *d = nullptr;
    SFG_TRY(sfg_malloc(ctx, &d, g->packed ? nr * ldw * 4 : nr * nc));
    const dim3 grid((unsigned)((width + 255) / 256), (unsigned)std::min<size_t>(nr, 65535));
    if (g->packed) hipLaunchKernelGGL(k_filter_p2, grid, dim3(256), 0, ctx->stream, (const uint8_t *)g->dev, g->ld, ridx, cidx, nr, nc, (unsigned *)d, ldw);
    else hipLaunchKernelGGL(k_filter_i8, grid, dim3(256), 0, ctx->stream, g->dev, g->ld, ridx, cidx, nr, nc, (int8_t *)d);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) { (void)hipFree(d); SFG_HIP(ctx, e); }
    sfg_geno *f = new sfg_geno(); f->dev = (const int8_t *)d; f->nrow = nr; f->ncol = nc; f->ld = g->packed ? ldw * 4 : nc; f->owned = true; f->packed = g->packed;
    *out = f; return 0;
}
