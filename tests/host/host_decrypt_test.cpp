// The way back out through the host mirror: crypto::DecodeFloatVector(crypto::EncodeFloatVector(v)) and crypto::DecryptFloatVectorDev /
// DecryptFloatMatrixDev(crypto::EncryptFloatMatrixRowDev(v)) round trips; tests/test_host_decrypt.py supplies the keys and checks the printed worst errors
// against the derived bounds.
// Usage: host_decrypt_test <casedir>   (vals: vrows x vlen doubles; pk, sk: a key pair; level)
#include "../../sfgwas_amd/host/gwas.hpp"
#include <cmath>
#include <fstream>
#include <iostream>
static std::vector<uint64_t> readU64(const std::string &fn) {
    std::ifstream f(fn, std::ios::binary | std::ios::ate); if (!f) throw std::runtime_error("cannot open " + fn);
    size_t n = (size_t)f.tellg() / 8; f.seekg(0); std::vector<uint64_t> v(n); f.read((char *)v.data(), n * 8); return v;
}
int main(int argc, char **argv) {
    try {
        const std::string dir = argv[1];
        std::ifstream cs(dir + "/case.txt"); int vrows, vlen, level; cs >> vrows >> vlen >> level;
        auto mod = readU64(dir + "/moduli.bin"); int nq = (int)mod[0], np = (int)mod[1];
        std::vector<uint64_t> qi(mod.begin() + 2, mod.begin() + 2 + nq), pi(mod.begin() + 2 + nq, mod.begin() + 2 + nq + np);
        const double SC = 17179869184.0;
        auto cps = crypto::NewCryptoParams(0, 14, qi, pi, nullptr, SC);
        auto vw = readU64(dir + "/vals.bin"); const double *vd = (const double *)vw.data();
        std::vector<std::vector<double>> vals(vrows);
        for (int i = 0; i < vrows; i++) vals[i].assign(vd + (size_t)i * vlen, vd + (size_t)(i + 1) * vlen);
        // decode(encode(v))
        double worst_code = 0;
        for (int i = 0; i < vrows; i++) {
            std::vector<double> back = crypto::DecodeFloatVector(cps.get(), crypto::EncodeFloatVector(cps.get(), vals[i], level));
            if (back.size() < (size_t)vlen) throw std::runtime_error("DecodeFloatVector: too few values");
            for (int k = 0; k < vlen; k++) worst_code = std::max(worst_code, std::fabs(back[k] - vals[i][k]));
            for (size_t k = vlen; k < back.size(); k++) worst_code = std::max(worst_code, std::fabs(back[k]));      // the padding decodes to zero
        }
        // decrypt(encrypt(v)): refused without a secret key
        crypto::LoadPublicKey(cps.get(), readU64(dir + "/pk.bin"), false);
        auto kw = readU64(dir + "/key.bin"); std::vector<uint8_t> key((const uint8_t *)kw.data(), (const uint8_t *)kw.data() + 32);
        crypto::SeedEncryptor(cps.get(), key);
        crypto::DevCipherMatrix E = crypto::EncryptFloatMatrixRowDev(cps.get(), vals, level);
        bool refused = false;
        try { crypto::DecryptFloatMatrixDev(cps.get(), E, (size_t)vlen); } catch (const std::exception &) { refused = true; }
        if (!refused) throw std::runtime_error("DecryptFloatMatrixDev ran without a secret key");
        crypto::LoadSecretKey(cps.get(), readU64(dir + "/sk.bin"), false);
        auto D = crypto::DecryptFloatMatrixDev(cps.get(), E, (size_t)vlen);
        double worst_crypt = 0;
        for (int i = 0; i < vrows; i++) {
            if (D[i].size() != (size_t)vlen) throw std::runtime_error("DecryptFloatMatrixDev: wrong length");
            for (int k = 0; k < vlen; k++) worst_crypt = std::max(worst_crypt, std::fabs(D[i][k] - vals[i][k]));
        }
        std::vector<double> one = crypto::DecryptFloatVectorDev(cps.get(), E.row(0), (size_t)vlen);
        for (int k = 0; k < vlen; k++) if (one[k] != D[0][k]) throw std::runtime_error("DecryptFloatVectorDev differs from the matrix call");
        std::cout.precision(17);
        std::cout << "OK " << worst_code << " " << worst_crypt << std::endl;
        return 0;
    } catch (const std::exception &e) { std::cerr << "ERROR: " << e.what() << std::endl; return 1; }
}
