// Quality control through the host mirror: gwas::qc::SNPMissCounts, IndividualMissAndHetFilters, SNPMAFAndHWECounts and FilterResident on a resident matrix,
// driven the way the Go callers of gwas/qualcontrol.go would; tests/test_host_qc.py supplies the case and compares every printed number.
// Usage: host_qc_test <casedir>   (case.txt: nrow ncol numSnps indMissBound hetLower hetUpper; geno.bin int8; rowfilt.bin, colfilt.bin bytes; pheno.bin doubles)
#include "../../sfgwas_amd/host/gwas.hpp"
#include <fstream>
#include <iostream>
template <class T> static std::vector<T> readAll(const std::string &fn) {
    std::ifstream f(fn, std::ios::binary | std::ios::ate); if (!f) throw std::runtime_error("cannot open " + fn);
    size_t n = (size_t)f.tellg() / sizeof(T); f.seekg(0); std::vector<T> v(n); f.read((char *)v.data(), n * sizeof(T)); return v;
}
template <class V> static void line(const char *name, const V &v) { std::cout << name; for (auto x : v) std::cout << " " << (long long)x; std::cout << "\n"; }
int main(int argc, char **argv) {
    try {
        if (argc < 2) throw std::runtime_error("usage: host_qc_test <casedir>");
        const std::string dir = argv[1];
        std::ifstream cs(dir + "/case.txt"); size_t nrow, ncol; int numSnps; gwas::qc::FilterParams fp;
        cs >> nrow >> ncol >> numSnps >> fp.IndMissBound >> fp.HetLowerBound >> fp.HetUpperBound;
        auto mod = readAll<uint64_t>(dir + "/moduli.bin"); int nq = (int)mod[0], np = (int)mod[1];
        std::vector<uint64_t> qi(mod.begin() + 2, mod.begin() + 2 + nq), pi(mod.begin() + 2 + nq, mod.begin() + 2 + nq + np);
        auto cps = crypto::NewCryptoParams(0, 14, qi, pi, nullptr, 17179869184.0);
        auto geno = readAll<int8_t>(dir + "/geno.bin");
        if (geno.size() != nrow * ncol) throw std::runtime_error("geno.bin: wrong size");
        auto rfb = readAll<uint8_t>(dir + "/rowfilt.bin"), cfb = readAll<uint8_t>(dir + "/colfilt.bin");
        std::vector<bool> rowFilt(rfb.begin(), rfb.end()), colFilt(cfb.begin(), cfb.end());
        auto pheno = readAll<double>(dir + "/pheno.bin");
        sfg_geno *g = nullptr;
        cps->check(sfg_geno_upload(cps->ctx, geno.data(), nrow, ncol, ncol, &g), "sfg_geno_upload");
        line("snpmiss", gwas::qc::SNPMissCounts(cps.get(), g));
        std::vector<bool> ikeep = gwas::qc::IndividualMissAndHetFilters(cps.get(), g, colFilt, numSnps, fp);
        line("ikeep", ikeep);
        // the reference goes on with ikeep AND its earlier row filter; here the case's own row filter stands for that product
        gwas::qc::MAFAndHWECounts c = gwas::qc::SNPMAFAndHWECounts(cps.get(), g, rowFilt, colFilt, pheno);
        line("xsum", c.xSum); line("xcount", c.xCount); line("xsumctrl", c.xSumCtrl); line("xcountctrl", c.xCountCtrl);
        for (int k = 0; k < 3; k++) line("obsctrl", c.genoObservedCtrl[k]);
        sfg_geno *f = gwas::qc::FilterResident(cps.get(), g, rowFilt, colFilt);
        size_t fr, fc; cps->check(sfg_geno_dims(f, &fr, &fc), "sfg_geno_dims");
        std::vector<int8_t> back(fr * fc);
        cps->check(sfg_geno_download(cps->ctx, f, back.data()), "sfg_geno_download");
        std::cout << "filtered " << fr << " " << fc; for (auto x : back) std::cout << " " << (int)x; std::cout << "\n";
        bool refused = false;                         // a filter of the wrong length is the reference's "Invalid length of input array"
        try { gwas::qc::FilterResident(cps.get(), g, std::vector<bool>(nrow + 1, true), colFilt); } catch (const std::exception &) { refused = true; }
        if (!refused) throw std::runtime_error("FilterResident took a row filter of the wrong length");
        sfg_geno_free(cps->ctx, f); sfg_geno_free(cps->ctx, g);
        std::cout << "OK" << std::endl;
        return 0;
    } catch (const std::exception &e) { std::cerr << "ERROR: " << e.what() << std::endl; return 1; }
}
