// Secret shares to one ciphertext and back through the host mirror (sfgwas_amd/host/gwas.hpp: mpc::SSToCMatMask / SSToCMatFinish / CMatToSSShares / CMatToSSFinish),
// two parties in one program the way the Go callers would drive them: the hub holds the secret key, the other party the zero key (the two sum to the key the public
// key belongs to); this program plays the network - the reveal is the sum of the masked shares, the aggregations are word-wise sums mod q_i.
// tests/test_host_ss.py supplies the keys and checks the printed worst deviations against the derived bound.
// Usage: host_ss_test <casedir>   (moduli, pk, sk, key; case.txt: level n_elem)
#include "../../sfgwas_amd/host/gwas.hpp"
#include <cmath>
#include <fstream>
#include <iostream>
typedef unsigned __int128 u128;
static std::vector<uint64_t> readU64(const std::string &fn) {
    std::ifstream f(fn, std::ios::binary | std::ios::ate); if (!f) throw std::runtime_error("cannot open " + fn);
    size_t n = (size_t)f.tellg() / 8; f.seekg(0); std::vector<uint64_t> v(n); f.read((char *)v.data(), n * 8); return v;
}
static uint64_t rng_state = 0x243F6A8885A308D3ULL;
static uint64_t rnd64() { uint64_t z = (rng_state += 0x9E3779B97F4A7C15ULL); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL; z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL; return z ^ (z >> 31); }
static std::shared_ptr<crypto::detail::DevBuf> up(crypto::CryptoParams *cps, const void *src, size_t bytes) {
    auto d = std::make_shared<crypto::detail::DevBuf>(cps, bytes);
    cps->check(sfg_memcpy_h2d(cps->ctx, d->p, src, bytes), "h2d");
    return d;
}
static std::vector<uint64_t> down(crypto::CryptoParams *cps, const uint64_t *src, size_t words) {
    std::vector<uint64_t> v(words);
    cps->check(sfg_memcpy_d2h(cps->ctx, v.data(), src, words * 8), "d2h");
    return v;
}
static std::vector<u128> wide(const std::vector<uint64_t> &w) { std::vector<u128> v(w.size() / 2); for (size_t i = 0; i < v.size(); i++) v[i] = ((u128)w[2 * i + 1] << 64) | w[2 * i]; return v; }
static std::vector<uint64_t> narrow(const std::vector<u128> &v) { std::vector<uint64_t> w(v.size() * 2); for (size_t i = 0; i < v.size(); i++) { w[2 * i] = (uint64_t)v[i]; w[2 * i + 1] = (uint64_t)(v[i] >> 64); } return w; }

int main(int argc, char **argv) {
    try {
        const std::string dir = argv[1];
        std::ifstream cs(dir + "/case.txt"); int level, nElem; cs >> level >> nElem;
        auto mod = readU64(dir + "/moduli.bin"); int nq = (int)mod[0], np = (int)mod[1];
        std::vector<uint64_t> qi(mod.begin() + 2, mod.begin() + 2 + nq), pi(mod.begin() + 2 + nq, mod.begin() + 2 + nq + np);
        const double SC = 17179869184.0;
        const int fracBits = 30, limbs = 2, nparty = 2;
        const u128 P = (u128)0 - 159;                                           // 2^128 - 159
        auto addp = [&](u128 a, u128 b) { const u128 s = a + b; return (s < a || s >= P) ? s - P : s; };        // a, b < p
        auto subp = [&](u128 a, u128 b) { return a >= b ? a - b : a + (P - b); };
        std::vector<std::unique_ptr<crypto::CryptoParams>> cps;
        auto pk = readU64(dir + "/pk.bin"), sk = readU64(dir + "/sk.bin");
        auto kw = readU64(dir + "/key.bin");
        for (int i = 0; i < nparty; i++) {
            cps.push_back(crypto::NewCryptoParams(0, 14, qi, pi, nullptr, SC));
            crypto::LoadPublicKey(cps[i].get(), pk, false);
            std::vector<uint8_t> key((const uint8_t *)kw.data(), (const uint8_t *)kw.data() + 32); key[0] ^= (uint8_t)(i + 1);
            crypto::SeedEncryptor(cps[i].get(), key);
            crypto::LoadSecretKey(cps[i].get(), i == 0 ? sk : std::vector<uint64_t>(sk.size(), 0), false);
        }
        const size_t N = (size_t)cps[0]->N(), nl = (size_t)level + 1;
        std::vector<mpc::MPC> party;
        for (int i = 0; i < nparty; i++) party.push_back(mpc::MPC{cps[i].get(), i + 1, narrow({P})});
        // x, |x| < 2^50, additively shared mod p
        std::vector<long long> x(nElem);
        std::vector<u128> rm[2] = {std::vector<u128>(nElem), std::vector<u128>(nElem)}, rand[2] = {std::vector<u128>(nElem), std::vector<u128>(nElem)};
        for (int t = 0; t < nElem; t++) {
            x[t] = (long long)(rnd64() >> 13) - (1LL << 50);
            const u128 xe = x[t] < 0 ? P - (u128)(-x[t]) : (u128)x[t];
            rm[0][t] = (((u128)(rnd64() >> 1)) << 64) | rnd64();                  // below 2^127 < p
            rm[1][t] = subp(xe, rm[0][t]);
            for (int i = 0; i < 2; i++) rand[i][t] = (((u128)(rnd64() >> 3)) << 64) | rnd64();      // below 2^125 < bound
        }
        const u128 bound = P / (4 * (nparty - 1));
        // ---- SSToCMat
        std::vector<mpc::SSMasked> masked;
        std::vector<u128> revealed(nElem, 0);
        for (int i = 0; i < nparty; i++) {
            auto drm = up(cps[i].get(), narrow(rm[i]).data(), (size_t)nElem * 16), drand = up(cps[i].get(), narrow(rand[i]).data(), (size_t)nElem * 16);
            masked.push_back(mpc::SSToCMatMask(&party[i], drm->u(), drand->u(), narrow({bound}), (size_t)nElem));
            auto m = wide(down(cps[i].get(), masked[i].masked->u(), (size_t)nElem * 2));
            for (int t = 0; t < nElem; t++) revealed[t] = addp(revealed[t], m[t]);          // RevealSym
        }
        auto drev = up(cps[0].get(), narrow(revealed).data(), (size_t)nElem * 16);
        std::vector<uint64_t> ct(2 * nl * N, 0);
        for (int i = 0; i < nparty; i++) {
            crypto::DevCipherVector c = mpc::SSToCMatFinish(&party[i], masked[i], i == 0 ? drev->u() : nullptr, i == 0, nElem, level, fracBits);
            if (c.n != 1 || c.level != level) throw std::runtime_error("SSToCMatFinish: wrong shape");
            auto w = down(cps[i].get(), c.ptr(), ct.size());
            for (size_t k = 0; k < ct.size(); k++) ct[k] = (ct[k] + w[k]) % qi[(k / N) % nl];   // AggregateCMat
        }
        std::vector<crypto::DevCipherVector> cv;
        for (int i = 0; i < nparty; i++) {
            crypto::DevCipherVector v = crypto::NewDevCipherVector(cps[i].get(), 1, level, SC);
            cps[i]->check(sfg_memcpy_h2d(cps[i]->ctx, v.ptr(), ct.data(), ct.size() * 8), "h2d");
            cv.push_back(v);
        }
        std::vector<double> dec = crypto::DecryptFloatVectorDev(cps[0].get(), cv[0], (size_t)nElem);      // the hub's key is the whole key here
        double worst_ct = 0;
        for (int t = 0; t < nElem; t++) worst_ct = std::max(worst_ct, std::fabs(dec[t] * 1073741824.0 - (double)x[t]));
        // ---- CMatToSS: masks below 2^285 (Q_level / 4 > 2^287 from level 7 on), no error term
        const int W = 5;
        std::vector<mpc::CKKSToSSShares> sh;
        std::vector<uint64_t> h0agg(nl * N, 0);
        for (int i = 0; i < nparty; i++) {
            std::vector<uint64_t> mk(N * W);
            for (size_t c = 0; c < N; c++) { for (int k = 0; k < W - 1; k++) mk[c * W + k] = rnd64(); mk[c * W + W - 1] = rnd64() >> 35; }
            auto dmk = up(cps[i].get(), mk.data(), mk.size() * 8);
            std::vector<int32_t> e0(N, 0);
            auto de0 = up(cps[i].get(), e0.data(), N * 4);
            sh.push_back(mpc::CMatToSSShares(cps[i].get(), cv[i], dmk->u(), W, (const int32_t *)de0->p));
            auto w = down(cps[i].get(), sh[i].h0->u(), h0agg.size());
            for (size_t k = 0; k < h0agg.size(); k++) h0agg[k] = (h0agg[k] + w[k]) % qi[(k / N) % nl];   // AggregateRefreshShareVec
        }
        auto dagg = up(cps[0].get(), h0agg.data(), h0agg.size() * 8);
        std::vector<u128> sum(nElem, 0);
        for (int i = 0; i < nparty; i++) {
            mpc::DevWords o = mpc::CMatToSSFinish(&party[i], cv[i], sh[i], i == 0 ? dagg->u() : nullptr, i == 0, nElem, fracBits);
            auto s = wide(down(cps[i].get(), o->u(), (size_t)nElem * 2));
            for (int t = 0; t < nElem; t++) sum[t] = addp(sum[t], s[t]);
        }
        double worst_ss = 0;
        for (int t = 0; t < nElem; t++) {
            const bool neg = sum[t] > (P - 1) / 2;
            const u128 mag = neg ? P - sum[t] : sum[t];
            if (mag >> 62) throw std::runtime_error("CMatToSS: the shares do not add up to a small number");
            const double back = neg ? -(double)(long long)mag : (double)(long long)mag;
            worst_ss = std::max(worst_ss, std::fabs(back - (double)x[t]));
        }
        std::cout.precision(17);
        std::cout << "OK " << worst_ct << " " << worst_ss << std::endl;
        return 0;
    } catch (const std::exception &e) { std::cerr << "ERROR: " << e.what() << std::endl; return 1; }
}
