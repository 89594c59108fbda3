// reshard.hip — the row / column filter of the SHARDED resident matrix (sfg_mgpu_geno_filter, mgpu.hip): FilterMatrixFile (gwas/utilities.go:154) and the filters
// GeneratePCAInput reads through (gwas/gwas.go:545), for a matrix that lies in the HBM of G ranks.  A rank's filtered window is no whole number of 8192-column
// blocks, so the result is re-sharded: every rank gathers the window sfg_mgpu_shard gives it over the KEPT columns out of the old windows of the ranks that hold
// those columns.  The old windows are only read, so a rank needs nothing from its peers but their addresses.
//
// A thread owns one output dword - 4 consecutive columns of an int8 window, 16 codes of a packed one - for a run of kept rows, so every store is a dword and a
// workgroup's stores of a row are one contiguous kilobyte (k_filter_i8 stores single bytes).  Three tables: the segments (by value: which old shard serves which
// output columns), the global source column of every output column, the kept rows.  Which segment a column lies in is found once, before the row loop.  A
// workgroup whose 256 dwords lie in ONE segment - all of them at world 1, all but the few that straddle an old rank boundary otherwise - walks the rows with a
// row pointer that is the same for the whole workgroup and a 32-bit offset per column; the others carry a pointer and a stride per column (a packed dword may
// take its 16 codes from two old ranks, or more when a rank keeps fewer than 16 columns).  The grid is flat, block = row lane * strips + strip, and a block takes
// the rows lane, lane + lanes, ...: no grid dimension bounds the row count.
#include "reshard.hpp"
#include "kernels.hpp"
#include <algorithm>

namespace {
// the segment of output column c: the last one whose out0 <= c.  The loop index is uniform, so the table is read with scalar loads; only the selects are per lane.
struct Located { int seg; const uint8_t *base; size_t ld; unsigned gcol0; };
__device__ __forceinline__ Located locate(const ReshardSegs &t, size_t c) {
    Located l = {0, t.s[0].base, t.s[0].ld, t.s[0].gcol0};
    for (int j = 1; j < t.n; j++) if (c >= t.s[j].out0) { l.seg = j; l.base = t.s[j].base; l.ld = t.s[j].ld; l.gcol0 = t.s[j].gcol0; }
    return l;
}
// CODES columns per output dword: 4 (int8, a byte each) or 16 (packed, two bits each)
template <int CODES>
__device__ __forceinline__ unsigned fetch(const uint8_t *row, unsigned off, int k) {
    if (CODES == 4) return (unsigned)row[off] << (8 * k);
    return ((row[off >> 2] >> (2 * (off & 3))) & 3u) << (2 * k);
}
// the rows lane0, lane0 + lanes, ... of output dword w, 32 / CODES of them at a time: their 32 byte loads are in flight together before the first store waits for
// one.  A batch's rows past the end read row lane0 again and are not stored.
template <int CODES, class G>
__device__ __forceinline__ void walk_rows(const unsigned *__restrict__ ridx, size_t nr, size_t lane0, size_t lanes, unsigned *__restrict__ out, size_t ldw, size_t w,
                                          unsigned keep, G gather) {
    constexpr int R = 32 / CODES;
    for (size_t r = lane0; r < nr; r += lanes * R) {
        unsigned v[R];
#pragma unroll
        for (int j = 0; j < R; j++) { const size_t rr = r + j * lanes; v[j] = gather(ridx[rr < nr ? rr : lane0]); }
#pragma unroll
        for (int j = 0; j < R; j++) { const size_t rr = r + j * lanes; if (rr < nr) out[rr * ldw + w] = v[j] & keep; }
    }
}
// cidx [nc]: global source column per output column; ridx [nr]: kept rows; out [nr][ldw] dwords; lanes: row lanes of the flat grid
template <int CODES>
__device__ __forceinline__ void reshard_body(const ReshardSegs &t, const unsigned *__restrict__ cidx, const unsigned *__restrict__ ridx, size_t nr, size_t nc,
                                             unsigned *__restrict__ out, size_t ldw, unsigned strips, unsigned lanes) {
    const unsigned strip = blockIdx.x % strips, lane0 = blockIdx.x / strips;
    const size_t w = (size_t)strip * 256 + threadIdx.x;                  // this thread's output dword
    const size_t cb0 = (size_t)strip * 256 * CODES, cb1 = std::min(cb0 + 256 * CODES, nc) - 1;      // the workgroup's first and last column (cb0 < nc: strips cover ldw)
    if (w >= ldw) return;
    // columns past nc (padding) read what column nc - 1 reads and are masked out: no load is conditional
    int n = 0;
    unsigned gc[CODES];
#pragma unroll
    for (int k = 0; k < CODES; k++) { const size_t c = w * CODES + k; if (c < nc) n++; gc[k] = cidx[std::min(c, nc - 1)]; }
    const unsigned bits = 32 / CODES, keep = n == CODES ? ~0u : (1u << (bits * n)) - 1u;
    const Located a = locate(t, cb0), b = locate(t, cb1);                // uniform over the workgroup
    if (a.seg == b.seg) {                                                // one old shard serves the whole workgroup
#pragma unroll
        for (int k = 0; k < CODES; k++) gc[k] -= a.gcol0;                // the column inside the old shard
        walk_rows<CODES>(ridx, nr, lane0, lanes, out, ldw, w, keep, [&](size_t sr) {
            const uint8_t *row = a.base + sr * a.ld;
            unsigned v = 0;
#pragma unroll
            for (int k = 0; k < CODES; k++) v |= fetch<CODES>(row, gc[k], k);
            return v;
        });
        return;
    }
    const uint8_t *p[CODES]; size_t ld[CODES]; unsigned sh[CODES];
#pragma unroll
    for (int k = 0; k < CODES; k++) {
        const Located l = locate(t, std::min(w * CODES + k, nc - 1));
        const unsigned off = gc[k] - l.gcol0;
        p[k] = l.base + (CODES == 4 ? off : off >> 2); sh[k] = 2 * (off & 3); ld[k] = l.ld;
    }
    walk_rows<CODES>(ridx, nr, lane0, lanes, out, ldw, w, keep, [&](size_t sr) {
        unsigned v = 0;
#pragma unroll
        for (int k = 0; k < CODES; k++) {
            const unsigned x = p[k][sr * ld[k]];
            v |= CODES == 4 ? x << (8 * k) : ((x >> sh[k]) & 3u) << (2 * k);
        }
        return v;
    });
}
__global__ void __launch_bounds__(256) k_reshard_i8(const ReshardSegs t, const unsigned *__restrict__ cidx, const unsigned *__restrict__ ridx, size_t nr, size_t nc,
                                                    unsigned *__restrict__ out, size_t ldw, unsigned strips, unsigned lanes) {
    reshard_body<4>(t, cidx, ridx, nr, nc, out, ldw, strips, lanes);
}
__global__ void __launch_bounds__(256) k_reshard_p2(const ReshardSegs t, const unsigned *__restrict__ cidx, const unsigned *__restrict__ ridx, size_t nr, size_t nc,
                                                    unsigned *__restrict__ out, size_t ldw, unsigned strips, unsigned lanes) {
    reshard_body<16>(t, cidx, ridx, nr, nc, out, ldw, strips, lanes);
}
}  // namespace

int sfg_reshard_window(sfg_ctx *ctx, const ReshardSegs &segs, const unsigned *cols_host, size_t wcols, const unsigned *rows_host, size_t nr, bool packed, sfg_geno **out) {
    *out = nullptr;
    if (!wcols || !nr || segs.n < 1 || segs.n > RESHARD_MAX_SEGS) SFG_FAIL(ctx, "sfg_mgpu_geno_filter: empty window or segment table");
    SFG_HIP(ctx, hipSetDevice(ctx->device));
    ApiScope scope(ctx);
    unsigned *tab = nullptr;                                     // the index tables: O(window columns + kept rows)
    SFG_TRY(sfg_scratch(ctx, "qc.reshard", (wcols + nr) * 4, (void **)&tab));
    // a row of the result: whole dwords.  int8 rows are padded to 16 bytes, so that a scan reads them with 16-byte loads; packed rows as sfg_geno_pack lays them out
    const size_t ldw = (wcols + 15) / 16 * (packed ? 1 : 4);
    void *d = nullptr;
    SFG_TRY(sfg_malloc(ctx, &d, nr * ldw * 4));
    // a few ten thousand workgroups (the last round of them is then a small share of the call), each with at least 16 rows to spread its set-up over
    const size_t strips = (ldw + 255) / 256;                     // < 2^22
    const size_t lanes = std::max<size_t>(1, std::min((32768 + strips - 1) / strips, (nr + 15) / 16));
    hipError_t e = hipMemcpyAsync(tab, cols_host, wcols * 4, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(tab + wcols, rows_host, nr * 4, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) {
        const dim3 grid((unsigned)(strips * lanes));             // <= 2^22 + 2^15
        if (packed) hipLaunchKernelGGL(k_reshard_p2, grid, dim3(256), 0, ctx->stream, segs, tab, tab + wcols, nr, wcols, (unsigned *)d, ldw, (unsigned)strips, (unsigned)lanes);
        else hipLaunchKernelGGL(k_reshard_i8, grid, dim3(256), 0, ctx->stream, segs, tab, tab + wcols, nr, wcols, (unsigned *)d, ldw, (unsigned)strips, (unsigned)lanes);
        e = hipGetLastError();
    }
    const hipError_t es = hipStreamSynchronize(ctx->stream);      // (also when an enqueue failed: the host tables are the caller's)
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) { (void)hipFree(d); SFG_HIP(ctx, e); }
    sfg_geno *f = new sfg_geno(); f->dev = (const int8_t *)d; f->nrow = nr; f->ncol = wcols; f->ld = ldw * 4; f->owned = true; f->packed = packed;
    *out = f; return 0;
}
