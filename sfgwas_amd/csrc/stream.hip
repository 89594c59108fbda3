// stream.hip — the association scan's genotype batches streamed from storage (BASELINE config 5).
//
// Reference (gwas/assoc.go:340-420): GenoBlockMult walks the SNPs of a chromosome file; every `pgenBatchSize` KEPT SNPs it shells out to
// plink2 + Python (scripts/filterMatrixPgen.sh, plinkBedToBinary.py, transposeMatrix.py) to materialise an int8 [numInd x batch] temp file,
// opens it as a GenoFileStream, calls MatMult4Stream(cps, mat, X, 5, false, square, nproc) and concatenates the batch outputs
// (crypto.ConcatCipherMatrix).  Here the SNP-major 2-bit PLINK .bed IS the input: a batch is one contiguous byte range of the file
// (bps = ceil(num_sample / 4) bytes per SNP), read with pread() into pinned memory by a reader thread while the GPU works on the previous
// batch, copied to HBM as packed 2-bit codes (4x less than int8 over PCIe), decoded / filtered / transposed on the device
// (k_bed_decode, pinned by the reference scripts' outputs in tests/test_input_formats.py), multiplied, concatenated.  A .pgen file is
// converted once with `plink2 --make-bed` (the reference already depends on plink2 for this path), or decoded natively (pgen.hip).
//
// Every batch multiplies the SAME ciphertext matrix `mat` (GenoBlockMult(b, concat, ...) walks all chromosome batches with one concat, assoc.go:714-718;
// gWY's four calls per block likewise), and the reference recomputes rotCache[i][baby] = RotateRight(mat[i][bi], -baby) inside every MatMult4Stream call
// (matmult.go:1373-1377) - 90 key switches per input ciphertext, which at one block column per batch are the LARGEST item of a batch (47 % of the kernel
// time at 500 000 x 8192, s = 13).  The rotations depend on `mat` only, so one call builds the baby-step rotation cache once (the same key switches, the
// same bits; 1.86 GB per block row at s = 13: 115 GB for 500 000 samples) and every batch multiplies against it (SFG_ASSOC_ROTCACHE_MB=0 restores the
// per-batch rebuild; a cache that exceeds the budget falls back to it).
#include "common.hpp"
#include <chrono>
#include "kernels.hpp"
#include "pgen.hpp"
#include <algorithm>
#include <condition_variable>
#include <cerrno>
#include <fcntl.h>
#include <mutex>
#include <sys/stat.h>
#include <thread>
#include <unistd.h>

namespace {
struct Span { off_t off; size_t bytes; };              // the bytes of a batch in the file
struct Reader {                                        // fills pinned slot k & 1 with the bytes of batch k, one batch ahead of the consumer
    int fd; const std::vector<Span> *bt; uint8_t *slot[2];
    bool direct = false; size_t lead[2] = {0, 0};       // O_DIRECT: 4096-byte aligned file ranges; the batch starts `lead` bytes into its slot
    std::mutex mu; std::condition_variable cv; long filled = -1, released = -1; bool failed = false; std::string err;
    void run() {
        for (size_t k = 0; k < bt->size(); k++) {
            { std::unique_lock<std::mutex> lk(mu); cv.wait(lk, [&] { return (long)k - 2 <= released; }); }      // slot k & 1 was last used by batch k - 2
            const Span &b = (*bt)[k]; const off_t off = b.off, a0 = direct ? off & ~(off_t)4095 : off;
            const size_t ld = (size_t)(off - a0), want = ld + b.bytes, want_al = direct ? (want + 4095) & ~(size_t)4095 : want; size_t got = 0;
            while (got < want) {
                ssize_t r = pread(fd, slot[k & 1] + got, want_al - got, a0 + (off_t)got);
                if (r <= 0) { std::lock_guard<std::mutex> lk(mu); failed = true; err = "short read from the genotype file"; cv.notify_all(); return; }
                got += (size_t)r;
            }
            lead[k & 1] = ld;
            { std::lock_guard<std::mutex> lk(mu); filled = (long)k; }
            cv.notify_all();
        }
    }
    bool wait_filled(size_t k) { std::unique_lock<std::mutex> lk(mu); cv.wait(lk, [&] { return failed || filled >= (long)k; }); return !failed; }
    void release(size_t k) { { std::lock_guard<std::mutex> lk(mu); released = (long)k; } cv.notify_all(); }
};
// Ends the reader on every way out of the scan: released past the last batch it runs out without waiting for a slot, then it is joined (the pinned slots it
// fills are context scratch that outlives the call)
struct ReaderEnd { Reader &rd; std::thread &th; ~ReaderEnd() { rd.release(rd.bt->size() + 2); th.join(); } };
// both queues of the scan idle before anything they use is given back
struct QueuesIdle { sfg_ctx *ctx; const StreamOwner &copy; ~QueuesIdle() { (void)hipStreamSynchronize(ctx->stream); if (copy.h) (void)hipStreamSynchronize(copy.h); } };
}  // namespace

// The baby-step rotation cache of the ciphertext matrix every batch of an association scan multiplies (see the header comment): *out = nullptr when the
// cache is switched off, does not fit the budget or the device (the caller then lets every product build its own rotations).  widths: the distinct
// block-column widths of the batches, for the active-baby tables (matmult.go:1326-1336).  *out is the context's scratch entry "assoc.rotf" (kept for the next call).
int assoc_build_rotcache(sfg_ctx *ctx, const u64 *A_dev, int s, int in_level, int max_level, size_t nr, const std::vector<size_t> &widths, double **out) {
    *out = nullptr;
    const size_t slots = SFG_SLOTS;
    size_t jobw = 0, tailw = 0;
    const int nbr = (int)((nr + slots - 1) / slots);
    if (!ctx->cfg.assoc_cache_budget || !mac_use_dma(ctx) || sfg_rotcache_layout(ctx, s, max_level, &jobw, &tailw)) { ctx->err.clear(); return 0; }
    const size_t words = (size_t)nbr * s * jobw + tailw;
    if (words * 8 > ctx->cfg.assoc_cache_budget) return 0;
    double *buf = nullptr;
    if (sfg_scratch(ctx, "assoc.rotf", words * 8, (void **)&buf)) { ctx->err.clear(); return 0; }      // no room even without the buffers of earlier calls: per-batch rotations
    std::vector<std::vector<uint8_t>> tabs; assoc_baby_tabs(nr, widths, tabs);
    SFG_TRY(rotcache_build_rows_tab(ctx, A_dev, s, in_level, max_level, nbr, 0, nbr, &tabs, buf));
    *out = buf; return 0;
}
// The cache in the form the context multiplies with: the int8 MAC's rot tiles where every modulus runs on the matrix core (round 4: the scan's MAC leaves the
// fp64 kernel, the cache shrinks from 1.86 to 1.3 GB per block row at s = 13), else the fp64 operand rows, else nothing (every product rotates for itself).
int assoc_build_rot(sfg_ctx *ctx, const u64 *A_dev, int s, int in_level, int max_level, size_t nr, const std::vector<size_t> &widths, AssocRot &out) {
    out = AssocRot();
    out.op = RotOperand::own(A_dev, in_level);
    if (ctx->cfg.assoc_cache_budget) {
        std::vector<std::vector<uint8_t>> tabs; assoc_baby_tabs(nr, widths, tabs);
        SFG_TRY(i8_rotpre_build(ctx, A_dev, s, in_level, max_level, (int)tabs.size(), &tabs, ctx->cfg.assoc_cache_budget, "assoc.rot8", out.pre));
        if (out.pre.G) { out.op = RotOperand::i8_tiles(&out.pre); return 0; }
    }
    double *rows = nullptr;
    SFG_TRY(assoc_build_rotcache(ctx, A_dev, s, in_level, max_level, nr, widths, &rows));
    if (rows) out.op = RotOperand::f64_cache(rows);
    return 0;
}
void assoc_free_rot(AssocRot &r) { i8_rotpre_free(r.pre); r = AssocRot(); }        // (the buffers are the context's scratch: see i8_rotpre_free)
// the product of one batch: all nct block columns of the batch's matrix
int assoc_product(sfg_ctx *ctx, const AssocRot &r, int s, int max_level, const sfg_geno *g, unsigned flags, int nct, uint64_t *out) {
    return matmul_resident_range(ctx, r.op, {g, flags, s, max_level, 0, nct, out});
}

// The tail of a batch, shared by the streamed scan and sfg_assoc_pgen: the s rows of the product (tmp: [s][nct] ciphertexts of ctw words) copied to their place
// in out_dev at out_shift, the padded sums of the batch zeroed, its column sums added (dosageSum[outShift + c], assoc.go:404-405)
int assoc_batch_tail(sfg_ctx *ctx, const u64 *tmp, const sfg_geno *g, int s, size_t nct, size_t ctw, uint64_t *out_dev, size_t out_ct_capacity, size_t out_shift,
                     double *sum_host, double *sqsum_host) {
    const size_t slots = SFG_SLOTS;
    for (int i = 0; i < s; i++)
        SFG_HIP(ctx, hipMemcpyAsync(out_dev + ((size_t)i * out_ct_capacity + out_shift) * ctw, tmp + (size_t)i * nct * ctw, nct * ctw * 8, hipMemcpyDeviceToDevice, ctx->stream));
    if (!sum_host && !sqsum_host) return 0;
    if (sum_host) std::fill(sum_host + out_shift * slots, sum_host + (out_shift + nct) * slots, 0.0);
    if (sqsum_host) std::fill(sqsum_host + out_shift * slots, sqsum_host + (out_shift + nct) * slots, 0.0);
    return sfg_geno_colsums(ctx, g, sum_host ? sum_host + out_shift * slots : nullptr, sqsum_host ? sqsum_host + out_shift * slots : nullptr);
}

// out_dev: [s][out_ct_capacity][2][max_level][N]; *out_ct = sum over batches of ceil(kept / slots) (the width ConcatCipherMatrix would give).
// sum_host / sqsum_host: optional [*out_ct * slots] column sums in the reference's padded layout (dosageSum[outShift + c], assoc.go:404-405).
// One engine for both on-disk formats: a batch is a contiguous byte range of the file (.bed: nsnp * bps bytes; .pgen: the variant records of the batch, preceded by
// the LD base its first records may need), read ahead by the reader thread, copied as it is, decoded on the copy queue into the batch's int8 matrix.
// part / nparts (multi-GPU scans, mgpu.hip): this call multiplies the batches k with k % nparts == part (AssocPlan, assoc_plan.hpp) and leaves the output
// ciphertexts and sums of the other batches untouched; `ranges` (optional) receives (first output ciphertext, count) of every batch it multiplied.
enum { FMT_BED = 0, FMT_PGEN = 1 };
int assoc_stream_part(sfg_ctx *ctx, int fmt, const char *path, size_t num_sample, size_t num_snp, const uint8_t *row_filter, const uint8_t *col_filter,
                      size_t batch_snps, const uint64_t *A_dev, int s, int in_level, int max_level, unsigned flags,
                      uint64_t *out_dev, size_t out_ct_capacity, size_t *out_ct, double *sum_host, double *sqsum_host,
                      int part, int nparts, std::vector<std::pair<size_t, size_t>> *ranges) {
    SFG_HIP(ctx, hipSetDevice(ctx->device));
    const char *who = fmt == FMT_BED ? "assoc_stream_bed" : "assoc_stream_pgen";
    if (!batch_snps) SFG_FAIL(ctx, "%s: bad dimensions", who);
    if (flags & SFG_TRANSPOSE) SFG_FAIL(ctx, "%s: batches are multiplied as X (samples x SNPs)", who);
    const size_t N = SFG_N, L = (size_t)max_level;
    const bool direct = (flags & SFG_STREAM_DIRECT) != 0;                                        // bypass the page cache: what a 5 TB scan from NVMe sees
    FdOwner file(open(path, O_RDONLY));                                                          // closed last, after everything that reads from it is gone
    if (file.fd < 0) SFG_FAIL(ctx, "%s: cannot open %s", who, path);                             // os.Open panics in the reference (filestream.go:59-61)
    flags &= ~SFG_STREAM_DIRECT;
    struct stat stt; uint8_t head[12] = {0};
    if (fstat(file.fd, &stt) || pread(file.fd, head, 12, 0) < 3) SFG_FAIL(ctx, "%s: cannot read %s", who, path);
    PgenIndex ix; std::vector<PgenWindow> win;
    size_t bps = 0, pitch = 0;
    if (fmt == FMT_BED) {
        if (!num_sample || !num_snp) SFG_FAIL(ctx, "%s: bad dimensions", who);
        bps = (num_sample + 3) / 4; pitch = bps;
        if ((size_t)stt.st_size != 3 + num_snp * bps) SFG_FAIL(ctx, "%s: file holds %zu bytes, expected 3 + %zu x %zu", who, (size_t)stt.st_size, num_snp, bps);
        if (head[0] != 0x6C || head[1] != 0x1B || head[2] != 0x01) SFG_FAIL(ctx, "%s: not a SNP-major PLINK .bed", who);
    } else {
        const size_t hb = (size_t)stt.st_size >= 12 ? pgen_header_bytes(head) : 0;
        if (!hb || hb > (size_t)stt.st_size) SFG_FAIL(ctx, "%s: %s is not a PLINK 2 .pgen in a supported storage mode", who, path);
        std::vector<uint8_t> hdr(hb);
        if (pread(file.fd, hdr.data(), hb, 0) != (ssize_t)hb) SFG_FAIL(ctx, "%s: cannot read the header of %s", who, path);
        SFG_TRY(pgen_index(ctx, hdr.data(), hb, (size_t)stt.st_size, ix));
        num_sample = ix.ns; num_snp = ix.nv; pitch = pgen_pitch(ix);
    }
    if (direct) {                                      // the header was read through the page cache; the batches go around it
        file.reset(open(path, O_RDONLY | O_DIRECT));
        if (file.fd < 0) SFG_FAIL(ctx, "%s: the file system of %s does not support O_DIRECT", who, path);
    }
    if (nparts < 1 || part < 0 || part >= nparts) SFG_FAIL(ctx, "%s: bad part", who);
    const AssocPlan plan = assoc_plan(col_filter, num_snp, batch_snps, part, nparts);
    const std::vector<AssocBatch> &bt = plan.bt;
    if (out_ct) *out_ct = plan.total_ct;
    if (plan.total_ct > out_ct_capacity) SFG_FAIL(ctx, "%s: output needs %zu ciphertexts per row, capacity %zu", who, plan.total_ct, out_ct_capacity);
    if (ranges) ranges->clear();
    std::vector<Span> span(bt.size()); size_t max_bytes = 0, max_rows = 0;
    if (fmt == FMT_PGEN) win.resize(bt.size());
    for (size_t k = 0; k < bt.size(); k++) {
        const AssocBatch &b = bt[k];
        if (fmt == FMT_BED) { span[k] = {3 + (off_t)(b.snp0 * bps), b.nsnp * bps}; max_rows = std::max(max_rows, b.nsnp); }
        else {
            SFG_TRY(pgen_window(ctx, ix, (size_t)stt.st_size, b.snp0, b.snp0 + b.nsnp, win[k]));
            span[k] = {(off_t)win[k].f0, (size_t)(win[k].f1 - win[k].f0)}; max_rows = std::max(max_rows, win[k].nr);
        }
        max_bytes = std::max(max_bytes, span[k].bytes);
    }
    if (bt.empty()) return 0;
    // row map once; column maps per batch
    std::vector<int32_t> rmap_h(num_sample), cmap_h(plan.max_nsnp);
    const size_t nr = filter_map(row_filter, num_sample, rmap_h.data());
    if (!nr) SFG_FAIL(ctx, "%s: the row filter keeps nothing", who);
    const size_t ctw = 2 * L * N, max_ct = assoc_cts(plan.max_kept);
    const bool trace = ctx->cfg.assoc_trace;       // (A/B build, SFG_ASSOC_TRACE: wall times of the cache build and of every batch's product, each synchronised)
    const auto t_call = std::chrono::steady_clock::now(); auto t_end = t_call;
    // The owners of the body are declared so that leaving it, on every path, gives this order: reader released and joined, compute queue synchronised, copy queue
    // synchronised, events destroyed, assoc_free_rot, copy queue destroyed - and, after the body, `file` closed.
    const int rc = [&]() -> int {
        StreamOwner copy; AssocRotScope rot; EventOwner ev_h2d[2], ev_ready[2], ev_free[2];
        QueuesIdle idle{ctx, copy};
        // every buffer of the call is scratch of the context (device pool / pinned host pool): the next call of the scan - gWY makes four per block - finds them in place
        int32_t *rmap = nullptr, *cmap[2]; uint8_t *hb[2], *db[2], *rows[2] = {nullptr, nullptr}, *desc[2] = {nullptr, nullptr}; int8_t *gb[2]; int *herr = nullptr; u64 *tmp = nullptr;
        SFG_TRY(sfg_scratch(ctx, "assoc.rmap", num_sample * sizeof(int32_t), (void **)&rmap));
        SFG_HIP(ctx, hipMemcpy(rmap, rmap_h.data(), num_sample * sizeof(int32_t), hipMemcpyHostToDevice));
        SFG_TRY(sfg_scratch(ctx, "assoc.tmp", (size_t)s * max_ct * ctw * 8, (void **)&tmp));
        SFG_HIP(ctx, hipStreamCreateWithFlags(&copy.h, hipStreamNonBlocking));
        if (fmt == FMT_PGEN) SFG_TRY(sfg_host_scratch(ctx, "assoc.herr", 2 * sizeof(int), (void **)&herr));
        for (int i = 0; i < 2; i++) {
            const std::string sx = std::to_string(i);
            SFG_TRY(sfg_host_scratch(ctx, ("assoc.hb" + sx).c_str(), max_bytes + 8192, (void **)&hb[i]));       // + the alignment slack of O_DIRECT ranges
            SFG_TRY(sfg_scratch(ctx, ("assoc.db" + sx).c_str(), max_bytes + 16, (void **)&db[i]));
            SFG_TRY(sfg_scratch(ctx, ("assoc.gb" + sx).c_str(), nr * plan.max_kept, (void **)&gb[i]));
            SFG_TRY(sfg_scratch(ctx, ("assoc.cmap" + sx).c_str(), plan.max_nsnp * sizeof(int32_t), (void **)&cmap[i]));
            if (fmt == FMT_PGEN) {
                SFG_TRY(sfg_scratch(ctx, ("assoc.rows" + sx).c_str(), max_rows * pitch, (void **)&rows[i]));
                SFG_TRY(sfg_scratch(ctx, ("assoc.desc" + sx).c_str(), PgenDesc(max_rows).bytes, (void **)&desc[i]));
            }
            SFG_HIP(ctx, hipEventCreateWithFlags(&ev_h2d[i].h, hipEventDisableTiming));
            SFG_HIP(ctx, hipEventCreateWithFlags(&ev_ready[i].h, hipEventDisableTiming));
            SFG_HIP(ctx, hipEventCreateWithFlags(&ev_free[i].h, hipEventDisableTiming));
        }
        if (trace) fprintf(stderr, "[assoc] buffers: %.1f ms\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_call).count());
        // the reader fills the first two slots while the rotation cache is built
        Reader rd; rd.fd = file.fd; rd.bt = &span; rd.slot[0] = hb[0]; rd.slot[1] = hb[1]; rd.direct = direct;
        std::thread reader([&rd] { rd.run(); });
        ReaderEnd reader_end{rd, reader};
        // ---- the baby-step rotation cache of `mat`, once for all batches of the call
        {
            const auto t0 = std::chrono::steady_clock::now();
            SFG_TRY(assoc_build_rot(ctx, (const u64 *)A_dev, s, in_level, max_level, nr, plan.widths, rot.r));
            if (trace) { (void)hipStreamSynchronize(ctx->stream); fprintf(stderr, "[assoc] rotation cache (%s): %.1f ms\n", rot.r.op.src == RotSrc::i8_tiles ? "int8 tiles" : rot.r.op.src == RotSrc::f64_cache ? "fp64 rows" : "none",
                                                                           std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count()); }
        }
        for (size_t k = 0; k < bt.size(); k++) {
            const AssocBatch &b = bt[k]; const int sl = (int)(k & 1);
            const size_t out_shift = plan.shift_of[k], nct = assoc_cts(b.kept);
            if (!rd.wait_filled(k)) { ctx->err = std::string(who) + ": " + rd.err; return 1; }
            filter_map(col_filter ? col_filter + b.snp0 : nullptr, b.nsnp, cmap_h.data());
            // copy queue: file bytes and column map of batch k into slot sl (free once the product of batch k - 2 has run), decode into gb[sl]
            if (k >= 2) SFG_HIP(ctx, hipStreamWaitEvent(copy.h, ev_free[sl].h, 0));
            SFG_HIP(ctx, hipMemcpyAsync(db[sl], hb[sl] + rd.lead[sl], span[k].bytes, hipMemcpyHostToDevice, copy.h));
            SFG_HIP(ctx, hipMemcpyAsync(cmap[sl], cmap_h.data(), b.nsnp * sizeof(int32_t), hipMemcpyHostToDevice, copy.h));
            if (fmt == FMT_PGEN) SFG_TRY(pgen_upload_desc(ctx, copy.h, ix, win[k], desc[sl]));
            SFG_HIP(ctx, hipEventRecord(ev_h2d[sl].h, copy.h));
            if (fmt == FMT_BED) SFG_TRY(launch_bed_decode(ctx, copy.h, db[sl], bps, num_sample, b.nsnp, rmap, cmap[sl], gb[sl], b.kept));
            else {
                const int *err_dev = nullptr;
                SFG_TRY(launch_pgen_decode(ctx, copy.h, db[sl], desc[sl], win[k].nr, ix.ns, pitch, rows[sl], &err_dev));
                SFG_TRY(launch_bed_decode_lut(ctx, copy.h, rows[sl] + win[k].lead * pitch, pitch, num_sample, b.nsnp, rmap, cmap[sl], gb[sl], b.kept, 0xFF020100u));
                SFG_HIP(ctx, hipMemcpyAsync(&herr[sl], err_dev, sizeof(int), hipMemcpyDeviceToHost, copy.h));
            }
            SFG_HIP(ctx, hipEventRecord(ev_ready[sl].h, copy.h));
            SFG_HIP(ctx, hipEventSynchronize(fmt == FMT_PGEN ? ev_ready[sl].h : ev_h2d[sl].h));   // the pinned slot (and cmap_h, the descriptors) may be refilled; the previous product is still running
            rd.release(k);
            if (fmt == FMT_PGEN) SFG_TRY(pgen_decode_error(ctx, herr[sl]));
            // compute queue: the product of batch k (MatMult4Stream(cps, mat, X, maxLevel, false, square, nproc), assoc.go:395), rows copied into place
            SFG_HIP(ctx, hipStreamWaitEvent(ctx->stream, ev_ready[sl].h, 0));
            sfg_geno g; g.dev = gb[sl]; g.nrow = nr; g.ncol = b.kept; g.ld = b.kept; g.owned = false;
            const auto tb = std::chrono::steady_clock::now();
            SFG_TRY(assoc_product(ctx, rot.r, s, max_level, &g, flags, (int)nct, (uint64_t *)tmp));
            if (trace) { const double t_enq = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tb).count(); (void)hipStreamSynchronize(ctx->stream);
                         fprintf(stderr, "[assoc] batch %zu: enqueued in %.1f ms, done after %.1f ms\n", k, t_enq, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tb).count()); }
            SFG_TRY(assoc_batch_tail(ctx, tmp, &g, s, nct, ctw, out_dev, out_ct_capacity, out_shift, sum_host, sqsum_host));
            SFG_HIP(ctx, hipEventRecord(ev_free[sl].h, ctx->stream));
            if (ranges) ranges->push_back({out_shift, nct});
        }
        t_end = std::chrono::steady_clock::now();
        return 0;
    }();
    if (trace) fprintf(stderr, "[assoc] call: %.1f ms until the last batch is enqueued, %.1f ms with the queues drained\n", std::chrono::duration<double, std::milli>(t_end - t_call).count(),
                       std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_call).count());
    return rc;
}
extern "C" int sfg_assoc_stream_bed(sfg_ctx *ctx, const char *bed_path, size_t num_sample, size_t num_snp, const uint8_t *row_filter, const uint8_t *col_filter,
                                    size_t batch_snps, const uint64_t *A_dev, int s, int in_level, int max_level, unsigned flags,
                                    uint64_t *out_dev, size_t out_ct_capacity, size_t *out_ct, double *sum_host, double *sqsum_host) {
    ApiScope api_scope(ctx);
    return assoc_stream_part(ctx, FMT_BED, bed_path, num_sample, num_snp, row_filter, col_filter, batch_snps, A_dev, s, in_level, max_level, flags, out_dev, out_ct_capacity, out_ct,
                             sum_host, sqsum_host, 0, 1, nullptr);
}
// the same scan straight from a PLINK 2 .pgen on disk (the reference's input at config 5: 10 M SNPs per party do not fit host memory as one image); sample and
// variant counts come from the file's header
extern "C" int sfg_assoc_stream_pgen(sfg_ctx *ctx, const char *pgen_path, const uint8_t *row_filter, const uint8_t *col_filter,
                                     size_t batch_snps, const uint64_t *A_dev, int s, int in_level, int max_level, unsigned flags,
                                     uint64_t *out_dev, size_t out_ct_capacity, size_t *out_ct, double *sum_host, double *sqsum_host) {
    ApiScope api_scope(ctx);
    return assoc_stream_part(ctx, FMT_PGEN, pgen_path, 0, 0, row_filter, col_filter, batch_snps, A_dev, s, in_level, max_level, flags, out_dev, out_ct_capacity, out_ct,
                             sum_host, sqsum_host, 0, 1, nullptr);
}
