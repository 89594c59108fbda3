// C6 on the device through the host mirror: crypto::CAddFreshZeroDev (CZeroMat + Add, matmult.go:1174,1225) on a resident matrix, then
// crypto::EncryptFloatMatrixRowDev (crypto.go:364-388) and crypto::CZerosDev; tests/test_host_encrypt.py replays the same calls in the same order through
// the C ABI under the same sampler key and compares every word.
// Usage: host_encrypt_test <casedir>   (M: rows x cols ciphertexts at level `level`; vals: vrows x vlen doubles)
#include "../../sfgwas_amd/host/gwas.hpp"
#include <fstream>
#include <iostream>
static std::vector<uint64_t> readU64(const std::string &fn) {
    std::ifstream f(fn, std::ios::binary | std::ios::ate); if (!f) throw std::runtime_error("cannot open " + fn);
    size_t n = (size_t)f.tellg() / 8; f.seekg(0); std::vector<uint64_t> v(n); f.read((char *)v.data(), n * 8); return v;
}
static void dump(const std::string &fn, const crypto::CipherMatrix &m) {
    std::ofstream f(fn, std::ios::binary);
    for (auto &row : m) for (auto &c : row) f.write((const char *)c.data.data(), c.data.size() * 8);
}
int main(int argc, char **argv) {
    try {
        const std::string dir = argv[1];
        std::ifstream cs(dir + "/case.txt"); int rows, cols, level, vrows, vlen, vlevel; cs >> rows >> cols >> level >> vrows >> vlen >> vlevel;
        auto mod = readU64(dir + "/moduli.bin"); int nq = (int)mod[0], np = (int)mod[1];
        std::vector<uint64_t> qi(mod.begin() + 2, mod.begin() + 2 + nq), pi(mod.begin() + 2 + nq, mod.begin() + 2 + nq + np);
        const double SC = 17179869184.0;
        auto cps = crypto::NewCryptoParams(0, 14, qi, pi, nullptr, SC);
        const int N = cps->N();
        crypto::DevCipherMatrix M = crypto::ToDevice(cps.get(), gwas::unflatten(readU64(dir + "/M.bin"), rows, cols, level, SC, N));
        bool refused = false;                                     // without a key nothing is encrypted
        try { crypto::CAddFreshZeroDev(cps.get(), M); } catch (const std::exception &) { refused = true; }
        if (!refused || crypto::HasPublicKey(cps.get())) throw std::runtime_error("CAddFreshZeroDev ran without a public key");
        crypto::LoadPublicKey(cps.get(), readU64(dir + "/pk.bin"), false);
        auto kw = readU64(dir + "/key.bin"); std::vector<uint8_t> key((const uint8_t *)kw.data(), (const uint8_t *)kw.data() + 32);
        crypto::SeedEncryptor(cps.get(), key);
        dump(dir + "/finished.bin", crypto::ToHost(crypto::CAddFreshZeroDev(cps.get(), M)));
        auto vw = readU64(dir + "/vals.bin"); const double *vd = (const double *)vw.data();
        std::vector<std::vector<double>> vals(vrows);
        for (int i = 0; i < vrows; i++) vals[i].assign(vd + (size_t)i * vlen, vd + (size_t)(i + 1) * vlen);
        crypto::DevCipherMatrix E = crypto::EncryptFloatMatrixRowDev(cps.get(), vals, vlevel);
        if ((int)E.rows != vrows || E.level != vlevel || E.scale != SC) throw std::runtime_error("EncryptFloatMatrixRowDev: wrong shape");
        dump(dir + "/encrypted.bin", crypto::ToHost(E));
        dump(dir + "/zeros.bin", {crypto::ToHost(crypto::CZerosDev(cps.get(), 2, vlevel))});
        uint64_t next = 0; cps->check(sfg_ctx_encryptor_next_index(cps->ctx, &next), "next_index");
        std::cout << "OK " << next << std::endl;
        return 0;
    } catch (const std::exception &e) { std::cerr << "ERROR: " << e.what() << std::endl; return 1; }
}
