// From quality control to the PCA on a party's node through the host mirror: gwas::qc::FilterResidentSharded, SketchSharded and ColSumsSharded on a sharded
// resident matrix (every rank on device 0), and the same entry points through the C-ABI; tests/test_host_reshard.py supplies the case and compares every number.
// Usage: host_reshard_test <casedir>   (case.txt: nrow ncol world kp; geno.bin int8; rowfilt.bin, colfilt.bin bytes; bucket.bin int32; sgn.bin int8)
#include "../../sfgwas_amd/host/gwas.hpp"
#include <fstream>
#include <iostream>
template <class T> static std::vector<T> readAll(const std::string &fn) {
    std::ifstream f(fn, std::ios::binary | std::ios::ate); if (!f) throw std::runtime_error("cannot open " + fn);
    size_t n = (size_t)f.tellg() / sizeof(T); f.seekg(0); std::vector<T> v(n); f.read((char *)v.data(), n * sizeof(T)); return v;
}
template <class V> static void line(const char *name, const V &v) { std::cout << name; for (auto x : v) std::cout << " " << (long long)x; std::cout << "\n"; }
// every shard of a sharded matrix: "<name> <local rank> <nrow> <ncol> values..." (nrow = ncol = 0: the rank has no window)
static void shards(const char *name, sfg_mgpu *mg, const sfg_mgeno *m) {
    for (int i = 0; i < sfg_mgpu_nlocal(mg); i++) {
        const sfg_geno *sh = sfg_mgpu_geno_shard(m, i);
        size_t nr = 0, nc = 0; std::vector<int8_t> back;
        if (sh) {
            if (sfg_geno_dims(sh, &nr, &nc)) throw std::runtime_error("sfg_geno_dims");
            back.resize(nr * nc);
            if (sfg_geno_download(sfg_mgpu_ctx(mg, i), sh, back.data())) throw std::runtime_error(std::string("sfg_geno_download: ") + sfg_last_error(sfg_mgpu_ctx(mg, i)));
        }
        std::cout << name << " " << i << " " << nr << " " << nc; for (auto x : back) std::cout << " " << (int)x; std::cout << "\n";
    }
}
int main(int argc, char **argv) {
    try {
        if (argc < 2) throw std::runtime_error("usage: host_reshard_test <casedir>");
        const std::string dir = argv[1];
        std::ifstream cs(dir + "/case.txt"); size_t nrow, ncol; int world, kp;
        cs >> nrow >> ncol >> world >> kp;
        auto mod = readAll<uint64_t>(dir + "/moduli.bin"); int nq = (int)mod[0], np = (int)mod[1];
        std::vector<uint64_t> qi(mod.begin() + 2, mod.begin() + 2 + nq), pi(mod.begin() + 2 + nq, mod.begin() + 2 + nq + np);
        auto cps = crypto::NewCryptoParamsMulti(std::vector<int>((size_t)world, 0), 14, qi, pi, nullptr, 17179869184.0);
        sfg_mgpu *mg = cps->mg;
        auto geno = readAll<int8_t>(dir + "/geno.bin");
        if (geno.size() != nrow * ncol) throw std::runtime_error("geno.bin: wrong size");
        auto rfb = readAll<uint8_t>(dir + "/rowfilt.bin"), cfb = readAll<uint8_t>(dir + "/colfilt.bin");
        std::vector<bool> rowFilt(rfb.begin(), rfb.end()), colFilt(cfb.begin(), cfb.end());
        auto bucket = readAll<int32_t>(dir + "/bucket.bin"); auto sgn = readAll<int8_t>(dir + "/sgn.bin");
        sfg_mgeno *g = nullptr;
        if (sfg_mgpu_geno_upload(mg, geno.data(), nrow, ncol, ncol, &g)) throw std::runtime_error(std::string("sfg_mgpu_geno_upload: ") + sfg_mgpu_last_error(mg));
        // the wrappers, the way GeneratePCAInput's caller would: filter, free the source at once, then sketch and moments of the PCA input
        sfg_mgeno *f = gwas::qc::FilterResidentSharded(cps.get(), g, rowFilt, colFilt);
        bool refused = false;                         // a filter of the wrong length is the reference's "Invalid length of input array"
        try { gwas::qc::FilterResidentSharded(cps.get(), g, rowFilt, std::vector<bool>(ncol + 1, true)); } catch (const std::exception &) { refused = true; }
        if (!refused) throw std::runtime_error("FilterResidentSharded took a column filter of the wrong length");
        // the C-ABI itself: no filters = a copy with the same windows; filters that keep nothing = an error that leaves *out NULL
        sfg_mgeno *copy = nullptr;
        if (sfg_mgpu_geno_filter(mg, g, nullptr, nullptr, &copy)) throw std::runtime_error(std::string("sfg_mgpu_geno_filter: ") + sfg_mgpu_last_error(mg));
        std::vector<uint8_t> none(ncol, 0);
        sfg_mgeno *bad = (sfg_mgeno *)(uintptr_t)1;
        if (!sfg_mgpu_geno_filter(mg, g, nullptr, none.data(), &bad) || bad != nullptr) throw std::runtime_error("a filter that keeps nothing was not refused");
        if (std::string(sfg_mgpu_last_error(mg)).find("keep nothing") == std::string::npos) throw std::runtime_error("unexpected message for a filter that keeps nothing");
        sfg_mgpu_geno_free(mg, g);
        shards("copy", mg, copy);
        sfg_mgpu_geno_free(mg, copy);
        shards("filtered", mg, f);
        std::vector<int32_t> fb; std::vector<int8_t> fs;                    // bucket and sign of the kept rows
        for (size_t i = 0; i < nrow; i++) if (rowFilt[i]) { fb.push_back(bucket[i]); fs.push_back(sgn[i]); }
        gwas::qc::SketchResult sk = gwas::qc::SketchSharded(cps.get(), f, fb, fs, kp);
        line("sketch", sk.sketch); line("xsum", sk.xsum); line("x2sum", sk.x2sum);
        std::vector<double> sum, sq;
        gwas::qc::ColSumsSharded(cps.get(), f, sum, sq);
        line("colsum", sum); line("colsq", sq);
        // NULL outputs through the C-ABI
        std::vector<double> sum2(sum.size());
        if (sfg_mgpu_geno_colsums(mg, f, sum2.data(), nullptr) || sum2 != sum) throw std::runtime_error("sfg_mgpu_geno_colsums with a NULL output differs");
        std::vector<uint64_t> xs2(sk.xsum.size());
        if (sfg_mgpu_sketch(mg, f, fb.data(), fs.data(), kp, nullptr, xs2.data(), nullptr) || xs2 != sk.xsum) throw std::runtime_error("sfg_mgpu_sketch with NULL outputs differs");
        sfg_mgpu_geno_free(mg, f);
        std::cout << "OK" << std::endl;
        return 0;
    } catch (const std::exception &e) { std::cerr << "ERROR: " << e.what() << std::endl; return 1; }
}
