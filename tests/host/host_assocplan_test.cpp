// The association scan's host arithmetic (sfgwas_amd/csrc/assoc_plan.hpp) on the CPU: batches, the plan of a call and of its parts, filter maps, diag_bool, the
// active-baby tables and the .pgen descriptor layout.  Stand-alone: includes the header, links nothing of the library.
// The reference is a literal restatement of the loops the scan held inline before they moved into the header (make_batches and the `sh += ceil(kept / slots)` walk
// of assoc_stream_part - the loop tests/test_gpu_stream.py::batches states in Python); the invariants are asserted directly as well.
#include "../../sfgwas_amd/csrc/assoc_plan.hpp"
#include <cstdio>
#include <string>
#include <vector>

static int fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { fails++; printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

constexpr size_t SLOTS = 8192;
typedef std::vector<uint8_t> Filt;

// ---------------------------------------------------------------- the reference: the parent's statements, word for word
struct RefBatch { size_t snp0, nsnp, kept; };
static std::vector<RefBatch> ref_batches(const uint8_t *col_filter, size_t num_snp, size_t batch_snps) {
    std::vector<RefBatch> b; size_t start = 0, counter = 0;
    for (size_t idx = 0; idx < num_snp; idx++) {
        if (!col_filter || col_filter[idx]) counter++;
        if (counter == batch_snps || (idx == num_snp - 1 && counter > 0)) { b.push_back({start, idx + 1 - start, counter}); start = idx + 1; counter = 0; }
    }
    return b;
}
struct RefPlan { std::vector<RefBatch> bt; std::vector<size_t> shift_of, widths; size_t total = 0, max_kept = 0, max_nsnp = 0; };
static RefPlan ref_plan(const uint8_t *col_filter, size_t num_snp, size_t batch_snps, int part, int nparts) {
    RefPlan p; const std::vector<RefBatch> bt_all = ref_batches(col_filter, num_snp, batch_snps);
    size_t sh = 0;
    for (size_t k = 0; k < bt_all.size(); k++) {
        if ((int)(k % (size_t)nparts) == part) { p.bt.push_back(bt_all[k]); p.shift_of.push_back(sh); }
        sh += (bt_all[k].kept + SLOTS - 1) / SLOTS;
    }
    p.total = sh;
    for (const RefBatch &b : p.bt) {
        p.max_nsnp = std::max(p.max_nsnp, b.nsnp); p.max_kept = std::max(p.max_kept, b.kept);
        for (size_t c0 = 0; c0 < b.kept; c0 += SLOTS) { const size_t w = std::min(SLOTS, b.kept - c0); if (std::find(p.widths.begin(), p.widths.end(), w) == p.widths.end()) p.widths.push_back(w); }
    }
    return p;
}
static int ref_diag_bool(int r, int c, int dim, int index) {          // matmul.hip's statement of GetDiagBool (matmult.go:627-631)
    index %= dim; if (index < 0) index += dim;
    return (dim + 1 - r) <= index || index <= c - 1;
}
static size_t ref_desc_bytes(size_t nr) { auto al = [](size_t x) { return (x + 255) & ~(size_t)255; }; return al(nr * 8) + al(nr * 4) + al(nr) + al(nr * 4) + 256; }

// ---------------------------------------------------------------- header against reference + invariants, for every part of a call; returns the nparts = 1 plan
static AssocPlan check_call(const char *name, const Filt *filt, size_t num_snp, size_t batch_snps, int nparts = 1) {
    const uint8_t *f = filt ? filt->data() : nullptr;
    const std::vector<AssocBatch> all = assoc_batches(f, num_snp, batch_snps);
    const std::vector<RefBatch> rall = ref_batches(f, num_snp, batch_snps);
    CHECK(all.size() == rall.size(), "%s: %zu batches, reference %zu", name, all.size(), rall.size());
    size_t end = 0, kept_sum = 0, set_in_batches = 0;
    for (size_t k = 0; k < all.size() && k < rall.size(); k++) {
        const AssocBatch &b = all[k];
        CHECK(b.snp0 == rall[k].snp0 && b.nsnp == rall[k].nsnp && b.kept == rall[k].kept, "%s: batch %zu = {%zu, %zu, %zu}", name, k, b.snp0, b.nsnp, b.kept);
        CHECK(b.snp0 >= end && b.nsnp > 0 && b.snp0 + b.nsnp <= num_snp, "%s: batch %zu overlaps its predecessor or leaves the file", name, k);      // disjoint and ordered
        CHECK(b.kept > 0 && b.kept <= batch_snps, "%s: batch %zu keeps %zu", name, k, b.kept);
        end = b.snp0 + b.nsnp; kept_sum += b.kept;
        for (size_t j = b.snp0; j < b.snp0 + b.nsnp; j++) set_in_batches += !f || f[j];
    }
    CHECK(kept_sum == set_in_batches, "%s: sum(kept) = %zu, %zu set filter bytes in the batches", name, kept_sum, set_in_batches);
    const AssocPlan whole = assoc_plan(f, num_snp, batch_snps);
    CHECK(whole.bt.size() == all.size(), "%s: the plan of one part holds %zu of %zu batches", name, whole.bt.size(), all.size());
    std::vector<int> seen(all.size(), 0);
    for (int part = 0; part < nparts; part++) {
        const AssocPlan p = assoc_plan(f, num_snp, batch_snps, part, nparts);
        const RefPlan r = ref_plan(f, num_snp, batch_snps, part, nparts);
        CHECK(p.bt.size() == r.bt.size() && p.shift_of.size() == p.bt.size(), "%s part %d/%d: %zu batches, reference %zu", name, part, nparts, p.bt.size(), r.bt.size());
        CHECK(p.shift_of == r.shift_of && p.widths == r.widths, "%s part %d/%d: positions or widths differ from the reference", name, part, nparts);
        CHECK(p.total_ct == r.total && p.max_kept == r.max_kept && p.max_nsnp == r.max_nsnp, "%s part %d/%d: total %zu, max_kept %zu, max_nsnp %zu", name, part, nparts, p.total_ct, p.max_kept, p.max_nsnp);
        CHECK(p.total_ct == whole.total_ct, "%s part %d/%d: total %zu, %zu in the whole file", name, part, nparts, p.total_ct, whole.total_ct);
        for (size_t i = 0; i < p.bt.size() && i < r.bt.size(); i++) {
            CHECK(p.bt[i].snp0 == r.bt[i].snp0 && p.bt[i].nsnp == r.bt[i].nsnp && p.bt[i].kept == r.bt[i].kept, "%s part %d/%d: batch %zu differs from the reference", name, part, nparts, i);
            size_t k = 0; while (k < whole.bt.size() && whole.bt[k].snp0 != p.bt[i].snp0) k++;
            CHECK(k < whole.bt.size() && (int)(k % (size_t)nparts) == part, "%s part %d/%d: batch %zu is not one of its round-robin share", name, part, nparts, i);
            if (k < whole.bt.size()) { seen[k]++; CHECK(p.shift_of[i] == whole.shift_of[k], "%s part %d/%d: batch %zu at %zu, at %zu in the whole file", name, part, nparts, k, p.shift_of[i], whole.shift_of[k]); }
        }
    }
    for (size_t k = 0; k < seen.size(); k++) CHECK(seen[k] == 1, "%s: batch %zu belongs to %d of %d parts", name, k, seen[k], nparts);      // the parts partition the batches
    return whole;
}

int main() {
    const Filt f10100 = {1, 0, 1, 0, 0}, f11010 = {1, 1, 0, 1, 0};
    {   // 1: no SNPs
        const AssocPlan p = check_call("1", nullptr, 0, 4);
        CHECK(p.bt.empty() && p.total_ct == 0 && p.widths.empty(), "1: num_snp = 0");
    }
    {   // 2: filter all zero
        const Filt z(7, 0); const AssocPlan p = check_call("2", &z, z.size(), 3);
        CHECK(p.bt.empty() && p.total_ct == 0, "2: an all-zero filter makes %zu batches", p.bt.size());
    }
    {   // 3: the trailing filtered SNPs after the last full batch belong to no batch
        const AssocPlan p = check_call("3", &f10100, 5, 1);
        CHECK(p.bt.size() == 2 && p.bt[0].snp0 == 0 && p.bt[0].nsnp == 1 && p.bt[1].snp0 == 1 && p.bt[1].nsnp == 2 && p.bt[1].kept == 1, "3: batches");
        CHECK(p.total_ct == 2 && p.shift_of == std::vector<size_t>({0, 1}) && p.widths == std::vector<size_t>({1}), "3: positions");
    }
    {   // 4: one batch of exactly batch_snps that closes on SNP index 3
        const AssocPlan p = check_call("4", &f11010, 5, 3);
        CHECK(p.bt.size() == 1 && p.bt[0].snp0 == 0 && p.bt[0].nsnp == 4 && p.bt[0].kept == 3, "4: batch");
    }
    {   // 5: the batch closes only at the end of the file, nsnp covers the trailing zero
        const AssocPlan p = check_call("5", &f11010, 5, 4);
        CHECK(p.bt.size() == 1 && p.bt[0].snp0 == 0 && p.bt[0].nsnp == 5 && p.bt[0].kept == 3 && p.max_nsnp == 5 && p.max_kept == 3, "5: batch");
    }
    {   // 6: kept count an exact multiple of batch_snps: no empty last batch
        const Filt f = {1, 1, 0, 1, 1, 1, 1}; const AssocPlan p = check_call("6", &f, f.size(), 3);
        CHECK(p.bt.size() == 2 && p.bt[1].snp0 == 4 && p.bt[1].nsnp == 3 && p.bt[1].kept == 3, "6: batches");
        const AssocPlan q = check_call("6 NULL", nullptr, 6, 3);
        CHECK(q.bt.size() == 2 && q.total_ct == 2, "6: NULL filter, 6 SNPs in batches of 3");
    }
    {   // 7: a batch wider than one ciphertext
        const AssocPlan p = check_call("7", nullptr, 8193 + 5, 8193);
        CHECK(p.bt.size() == 2 && p.bt[0].kept == 8193 && p.bt[1].kept == 5 && p.bt[1].snp0 == 8193, "7: batches");
        CHECK(p.shift_of == std::vector<size_t>({0, 2}) && p.total_ct == 3, "7: the first batch takes 2 ciphertexts, the second 1");
        CHECK(p.widths == std::vector<size_t>({8192, 1, 5}), "7: widths");
        CHECK(p.max_kept == 8193 && p.max_nsnp == 8193 && assoc_cts(p.max_kept) == 2 && assoc_cts(8192) == 1 && assoc_cts(1) == 1 && assoc_cts(0) == 0, "7: maxima");
    }
    {   // 8: seven batches over three parts (kept counts 2, 2, 2, 2, 2, 2, 1 under a filter with holes)
        Filt f; for (int i = 0; i < 19; i++) f.push_back(i % 3 != 2); const AssocPlan p = check_call("8", &f, f.size(), 2, 3);
        CHECK(p.bt.size() == 7 && p.total_ct == 7, "8: %zu batches", p.bt.size());
        CHECK(assoc_plan(f.data(), f.size(), 2, 0, 3).bt.size() == 3 && assoc_plan(f.data(), f.size(), 2, 1, 3).bt.size() == 2 && assoc_plan(f.data(), f.size(), 2, 2, 3).bt.size() == 2, "8: 3 + 2 + 2");
        CHECK(assoc_plan(f.data(), f.size(), 2, 1, 3).shift_of == std::vector<size_t>({1, 4}), "8: part 1 writes at 1 and 4");
    }
    {   // 9: more parts than batches
        const AssocPlan whole = check_call("9", nullptr, 6, 3, 4);
        for (int part = 2; part < 4; part++) { const AssocPlan p = assoc_plan(nullptr, 6, 3, part, 4); CHECK(p.bt.empty() && p.widths.empty() && p.max_kept == 0 && p.total_ct == whole.total_ct && p.total_ct == 2, "9: part %d", part); }
    }
    // 10: diag_bool against the three-line statement; the baby tables against the literal double loop over it
    const int dims[5] = {1, 2, 91, 8191, 8192}, idx[7] = {0, 1, -1, 91, -91, 8191, -8191};
    for (int r : dims) for (int c : dims) for (int i : idx) CHECK(diag_bool(r, c, 8192, i) == ref_diag_bool(r, c, 8192, i), "10: diag_bool(%d, %d, 8192, %d)", r, c, i);
    struct TabCase { size_t nr; std::vector<size_t> widths; };
    for (const TabCase &t : {TabCase{100, {100}}, TabCase{8192 + 7, {8192, 1}}}) {
        std::vector<std::vector<uint8_t>> tabs; assoc_baby_tabs(t.nr, t.widths, tabs);
        const size_t nbr = (t.nr + SLOTS - 1) / SLOTS;
        CHECK(tabs.size() == nbr, "10: %zu block rows of %zu rows", tabs.size(), t.nr);
        for (size_t bi = 0; bi < nbr && bi < tabs.size(); bi++) {
            const int rows = (int)(std::min((bi + 1) * SLOTS, t.nr) - bi * SLOTS);
            std::vector<uint8_t> want(91, 0);
            for (int shift = 0; shift < 8192; shift++) for (size_t w : t.widths) if (ref_diag_bool(rows, (int)w, 8192, -shift)) want[shift % 91] = 1;
            CHECK(tabs[bi] == want, "10: baby table of block row %zu of %zu rows", bi, t.nr);
        }
    }
    // 11: filter maps
    for (size_t n : {(size_t)1, (size_t)5}) {
        const Filt ones(n, 1), zeros(n, 0); Filt alt(n); for (size_t i = 0; i < n; i++) alt[i] = (uint8_t)(i % 2 == 0 ? 3 : 0);      // any non-zero byte keeps
        const Filt *fs[4] = {nullptr, &ones, &zeros, &alt};
        for (const Filt *f : fs) {
            std::vector<int32_t> m(n, 77), want(n); size_t k = 0;
            for (size_t i = 0; i < n; i++) want[i] = (!f || (*f)[i]) ? (int32_t)k++ : -1;
            const size_t kept = filter_map(f ? f->data() : nullptr, n, m.data());
            CHECK(kept == k && m == want, "11: filter map of length %zu keeps %zu, expected %zu", n, kept, k);
            CHECK(filter_map(f ? f->data() : nullptr, n, nullptr) == k, "11: count without a map, length %zu", n);
            CHECK(kept == (f == &zeros ? 0 : f == &alt ? (n + 1) / 2 : n), "11: kept %zu of %zu", kept, n);
        }
    }
    // 11: the descriptor block of a .pgen window: off | len | vrt | ldbase | err
    for (size_t nr : {(size_t)1, (size_t)63, (size_t)64, (size_t)65, (size_t)257}) {
        const PgenDesc o(nr);
        const size_t begin[5] = {0, o.len, o.vrt, o.ldb, o.err}, size[5] = {nr * 8, nr * 4, nr, nr * 4, sizeof(int)};
        for (int i = 0; i < 5; i++) {
            CHECK(begin[i] % 256 == 0, "11: section %d of %zu records starts at %zu", i, nr, begin[i]);
            CHECK(begin[i] + size[i] <= (i < 4 ? begin[i + 1] : o.bytes), "11: section %d of %zu records runs into the next", i, nr);
        }
        CHECK(o.bytes == ref_desc_bytes(nr), "11: %zu bytes for %zu records, expected %zu", o.bytes, nr, ref_desc_bytes(nr));
        CHECK(align256(0) == 0 && align256(1) == 256 && align256(256) == 256 && align256(257) == 512, "11: align256");
    }
    printf(fails ? "FAILED (%d)\n" : "OK\n", fails);
    return fails ? 1 : 0;
}
