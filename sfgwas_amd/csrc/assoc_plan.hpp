// assoc_plan.hpp — the host arithmetic of the association scan's three genotype input paths (stream.hip, pgen.hip, genoio.hip, mgpu.hip) as pure functions:
// which SNPs form a batch, which batches a part multiplies and where their outputs land, a byte filter as an index map, the active-baby tables, the layout of a
// .pgen window's descriptor block.  Standard library only, so that all of it runs on a CPU (tests/host/host_assocplan_test.cpp).
#pragma once
#include "consts.hpp"
#include <algorithm>
#include <cstdint>
#include <vector>

inline int diag_bool(int r, int c, int dim, int index) {          // GetDiagBool, matmult.go:627-631
    index %= dim; if (index < 0) index += dim;
    return (dim + 1 - r) <= index || index <= c - 1;
}
inline size_t assoc_cts(size_t n) { return (n + SFG_SLOTS - 1) / SFG_SLOTS; }      // ciphertexts of 8192 slots that hold n values: the output block columns of a batch, the block rows of the input

// ---------------------------------------------------------------- a byte filter as an index map
// map[i] = position of element i among the kept ones, -1 = dropped; filt == NULL keeps everything (the identity).  Returns the kept count; map == NULL: counts only.
inline size_t filter_map(const uint8_t *filt, size_t n, int32_t *map) {
    size_t k = 0;
    for (size_t i = 0; i < n; i++) { const bool keep = !filt || filt[i]; if (map) map[i] = keep ? (int32_t)k : -1; k += keep; }
    return k;
}

// ---------------------------------------------------------------- batches
struct AssocBatch { size_t snp0, nsnp, kept; };            // file SNPs [snp0, snp0 + nsnp), `kept` of them pass the filter
// assoc.go:371-416: a batch closes when `batch_snps` kept SNPs have been seen or the file ends with a non-empty batch
inline std::vector<AssocBatch> assoc_batches(const uint8_t *col_filter, size_t num_snp, size_t batch_snps) {
    std::vector<AssocBatch> b; size_t start = 0, counter = 0;
    for (size_t idx = 0; idx < num_snp; idx++) {
        if (!col_filter || col_filter[idx]) counter++;
        if (counter == batch_snps || (idx == num_snp - 1 && counter > 0)) { b.push_back({start, idx + 1 - start, counter}); start = idx + 1; counter = 0; }
    }
    return b;
}
// One call of the scan.  part / nparts (multi-GPU scans, mgpu.hip): the call multiplies the batches k of the file with k % nparts == part - the reference's
// dispatcher hands batches to assoc_num_blocks_parallel workers the same way (assoc.go:360-408) - and leaves the outputs of the other batches untouched.
struct AssocPlan {
    std::vector<AssocBatch> bt;           // this part's batches
    std::vector<size_t> shift_of;         // first output ciphertext of each of them: positions count EVERY batch of the file (the width ConcatCipherMatrix would give)
    size_t total_ct = 0;                  // output ciphertexts per row of the whole file, the same in every part
    std::vector<size_t> widths;           // distinct block-column widths of this part's batches, first seen first: for the active-baby tables (matmult.go:1326-1336)
    size_t max_kept = 0, max_nsnp = 0;
};
inline AssocPlan assoc_plan(const uint8_t *col_filter, size_t num_snp, size_t batch_snps, int part = 0, int nparts = 1) {
    AssocPlan p; const size_t slots = SFG_SLOTS;
    const std::vector<AssocBatch> all = assoc_batches(col_filter, num_snp, batch_snps);
    for (size_t k = 0; k < all.size(); k++) {
        const AssocBatch &b = all[k];
        if ((int)(k % (size_t)nparts) == part) {
            p.bt.push_back(b); p.shift_of.push_back(p.total_ct);
            p.max_kept = std::max(p.max_kept, b.kept); p.max_nsnp = std::max(p.max_nsnp, b.nsnp);
            for (size_t c0 = 0; c0 < b.kept; c0 += slots) { const size_t w = std::min(slots, b.kept - c0); if (std::find(p.widths.begin(), p.widths.end(), w) == p.widths.end()) p.widths.push_back(w); }
        }
        p.total_ct += assoc_cts(b.kept);
    }
    return p;
}

// ---------------------------------------------------------------- active babies
// tabs[bi][baby]: some diagonal shift = giant * 91 + baby of block row bi exists for one of the block-column widths (nr rows in all)
inline void assoc_baby_tabs(size_t nr, const std::vector<size_t> &widths, std::vector<std::vector<uint8_t>> &tabs) {
    const size_t slots = SFG_SLOTS;
    const int nbr = (int)((nr + slots - 1) / slots);
    tabs.assign(nbr, std::vector<uint8_t>(SFG_D, 0));
    for (int bi = 0; bi < nbr; bi++) {
        const int rows = (int)(std::min((size_t)(bi + 1) * slots, nr) - (size_t)bi * slots);
        for (int shift = 0; shift < SFG_SLOTS; shift++) {
            if (tabs[bi][shift % SFG_D]) continue;
            for (size_t w : widths) if (diag_bool(rows, (int)w, SFG_SLOTS, -shift)) { tabs[bi][shift % SFG_D] = 1; break; }
        }
    }
}

// ---------------------------------------------------------------- descriptor block of a .pgen window of nr records on the device
// off (8 B per record, at 0) | len (4 B) | vrt (1 B) | ldbase (4 B) | err (one int), every section 256-aligned
inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }
struct PgenDesc {
    size_t len, vrt, ldb, err, bytes;
    explicit PgenDesc(size_t nr) : len(align256(nr * 8)), vrt(len + align256(nr * 4)), ldb(vrt + align256(nr)), err(ldb + align256(nr * 4)), bytes(err + 256) {}
};
