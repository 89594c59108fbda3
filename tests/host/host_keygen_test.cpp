// Collective key generation through the host mirror, two parties in one program: mpc::CollectivePubKeyGenShare / Finish, CollectiveRotKeyGenShares / Finish,
// CollectiveRelinKeyGenRound1 / Round2 / Finish with the aggregation done the way the Go side hands it over (shares summed modulus by modulus, the sums given back as
// device rows), the keys installed on a third context that holds s1 + s2; a vector encrypted there is rotated and squared and decrypted.  Also crypto::GenerateRotKeys +
// GaloisElementsForRotKeys against a literal restatement of GenerateRotKeys(8192, 20, true) plus the conjugate.  tests/test_host_keygen.py supplies the secrets
// and checks the printed worst errors against the derived bounds.
// Usage: host_keygen_test <casedir>   (moduli; sk1, sk2, skS: [nq+np][N] NTT rows; vals: slots doubles; case.txt: level, right rotation)
#include "../../sfgwas_amd/host/gwas.hpp"
#include <cmath>
#include <fstream>
#include <iostream>
#include <set>
static std::vector<uint64_t> readU64(const std::string &fn) {
    std::ifstream f(fn, std::ios::binary | std::ios::ate); if (!f) throw std::runtime_error("cannot open " + fn);
    size_t n = (size_t)f.tellg() / 8; f.seekg(0); std::vector<uint64_t> v(n); f.read((char *)v.data(), n * 8); return v;
}
using crypto::CryptoParams;
// the aggregation hand-off: rows [..][nq+np][N] of every party summed modulus by modulus, the sum placed in the memory of `dst`
static mpc::KeyBuf aggregate(const std::vector<CryptoParams *> &parties, const std::vector<mpc::KeyBuf> &shares, size_t words, const std::vector<uint64_t> &mod, CryptoParams *dst) {
    const size_t N = (size_t)dst->N(), nmod = mod.size();
    std::vector<uint64_t> acc(words, 0), one(words);
    for (size_t p = 0; p < parties.size(); p++) {
        parties[p]->check(sfg_memcpy_d2h(parties[p]->ctx, one.data(), shares[p]->u(), words * 8), "d2h");
        for (size_t i = 0; i < words; i++) { const uint64_t q = mod[(i / N) % nmod]; uint64_t v = acc[i] + one[i]; acc[i] = v >= q ? v - q : v; }
    }
    auto out = std::make_shared<crypto::detail::DevBuf>(dst, words * 8);
    dst->check(sfg_memcpy_h2d(dst->ctx, out->u(), acc.data(), words * 8), "h2d");
    return out;
}
int main(int argc, char **argv) {
    try {
        const std::string dir = argv[1];
        std::ifstream cs(dir + "/case.txt"); int level, nrot; cs >> level >> nrot;
        auto mod = readU64(dir + "/moduli.bin"); int nq = (int)mod[0], np = (int)mod[1];
        std::vector<uint64_t> qi(mod.begin() + 2, mod.begin() + 2 + nq), pi(mod.begin() + 2 + nq, mod.begin() + 2 + nq + np), all(mod.begin() + 2, mod.begin() + 2 + nq + np);
        const double SC = 17179869184.0;
        auto A = crypto::NewCryptoParams(0, 14, qi, pi, nullptr, SC), B = crypto::NewCryptoParams(0, 14, qi, pi, nullptr, SC), T = crypto::NewCryptoParams(0, 14, qi, pi, nullptr, SC);
        std::vector<CryptoParams *> parties = {A.get(), B.get()};

        // the Galois set of CollectiveInit (mhe.go:70-73): GenerateRotKeys(slots, 20, true), literally restated
        std::set<int> shifts;
        { int rot = 1; for (int i = 0; i < 13; i++) { shifts.insert(rot); shifts.insert(8192 - rot); rot *= 2; } }
        for (int i = 1; i < 91; i++) { shifts.insert(i); shifts.insert(i * 91); }
        for (int i = 1; i < 20; i++) shifts.insert(8192 - i);
        std::vector<uint64_t> want;
        for (int s : shifts) { uint64_t g = 1; for (int i = 0; i < s; i++) g = g * 5 % 32768; want.push_back(g); }
        want.push_back(32767);
        std::sort(want.begin(), want.end());
        const std::vector<uint64_t> gElems = crypto::GaloisElementsForRotKeys(T.get(), crypto::GenerateRotKeys(T->GetSlots(), 20, true));
        if (gElems != want) throw std::runtime_error("GaloisElementsForRotKeys differs from the restated GenerateRotKeys(8192, 20, true) + conjugate");
        if (std::set<uint64_t>(gElems.begin(), gElems.end()).size() != gElems.size() || gElems.front() != 5) throw std::runtime_error("Galois set: duplicates or wrong order");

        // secrets and sampler keys
        crypto::LoadSecretKeyQP(A.get(), readU64(dir + "/sk1.bin"), false);
        crypto::LoadSecretKeyQP(B.get(), readU64(dir + "/sk2.bin"), false);
        crypto::LoadSecretKeyQP(T.get(), readU64(dir + "/skS.bin"), false);
        crypto::SeedEncryptor(A.get(), std::vector<uint8_t>(32, 0x11)); crypto::SeedEncryptor(B.get(), std::vector<uint8_t>(32, 0x22)); crypto::SeedEncryptor(T.get(), std::vector<uint8_t>(32, 0x33));
        bool refused = false;
        { auto bare = crypto::NewCryptoParams(0, 14, qi, pi, nullptr, SC); auto c = mpc::CommonReferencePolys(bare.get(), std::vector<uint8_t>(32, 7), 0, 1);
          try { mpc::CollectivePubKeyGenShare(bare.get(), c->u()); } catch (const std::exception &) { refused = true; } }
        if (!refused) throw std::runtime_error("CollectivePubKeyGenShare ran without a secret key");

        const std::vector<uint8_t> seed(32, 0x5A);
        const size_t pw = mpc::keyPolyWords(T.get()); const int beta = mpc::keyBeta(T.get());
        // the common reference stream: polynomial 0 the public key's, 1..beta the relinearisation key's, then beta per rotation key
        std::vector<CryptoParams *> everyone = {A.get(), B.get(), T.get()};
        std::vector<mpc::KeyBuf> crpPk, crpRl, crpRt;
        for (CryptoParams *c : everyone) { crpPk.push_back(mpc::CommonReferencePolys(c, seed, 0, 1)); crpRl.push_back(mpc::CommonReferencePolys(c, seed, 1, beta)); crpRt.push_back(mpc::CommonReferencePolys(c, seed, 1 + beta, beta)); }

        // public key
        std::vector<mpc::KeyBuf> sh;
        for (int p = 0; p < 2; p++) sh.push_back(mpc::CollectivePubKeyGenShare(parties[p], crpPk[p]->u()).h);
        mpc::KeyBuf pkAgg = aggregate(parties, sh, pw, all, T.get());
        mpc::CollectivePubKeyGenFinish(T.get(), pkAgg->u(), crpPk[2]->u());
        if (!crypto::HasPublicKey(T.get())) throw std::runtime_error("no public key after CollectivePubKeyGenFinish");
        // one rotation key: the right rotation by nrot is the left rotation by slots - nrot
        const std::vector<uint64_t> g1 = {sfg_galois_for_rotation(T->ctx, T->GetSlots() - nrot)};
        sh.clear();
        for (int p = 0; p < 2; p++) sh.push_back(mpc::CollectiveRotKeyGenShares(parties[p], g1, crpRt[p]->u()).h);
        mpc::KeyBuf rtAgg = aggregate(parties, sh, beta * pw, all, T.get());
        mpc::CollectiveRotKeyGenFinish(T.get(), g1, rtAgg->u(), crpRt[2]->u());
        // relinearisation key, two rounds
        std::vector<mpc::RelinRound1Shares> r1;
        for (int p = 0; p < 2; p++) r1.push_back(mpc::CollectiveRelinKeyGenRound1(parties[p], crpRl[p]->u()));
        std::vector<mpc::KeyBuf> H0, H1, r2;
        for (int p = 0; p < 2; p++) { H0.push_back(aggregate(parties, {r1[0].h0, r1[1].h0}, beta * pw, all, parties[p])); H1.push_back(aggregate(parties, {r1[0].h1, r1[1].h1}, beta * pw, all, parties[p])); }
        for (int p = 0; p < 2; p++) r2.push_back(mpc::CollectiveRelinKeyGenRound2(parties[p], r1[p], H0[p]->u(), H1[p]->u()).h);
        mpc::KeyBuf r2Agg = aggregate(parties, r2, beta * pw, all, T.get()), H1T = aggregate(parties, {r1[0].h1, r1[1].h1}, beta * pw, all, T.get());
        mpc::CollectiveRelinKeyGenFinish(T.get(), r2Agg->u(), H1T->u());

        // a vector through the keys
        auto vw = readU64(dir + "/vals.bin"); const double *vd = (const double *)vw.data(); const size_t slots = (size_t)T->GetSlots();
        std::vector<double> vals(vd, vd + slots);
        crypto::DevCipherVector E = crypto::EncryptFloatVectorDev(T.get(), vals, level);
        crypto::Ciphertext rot = crypto::RotateRight(T.get(), crypto::ToHost(E)[0], nrot);
        std::vector<double> dr = crypto::DecryptFloatVectorDev(T.get(), crypto::ToDevice(T.get(), {rot}), slots);
        double worst_rot = 0, worst_sq = 0;
        for (size_t t = 0; t < slots; t++) worst_rot = std::max(worst_rot, std::fabs(dr[t] - vals[(t + slots - nrot) % slots]));
        crypto::DevCipherVector Q = crypto::CMultDev(T.get(), E, E, qi);       // lattigo's Rescale rule decides whether the product drops a level (the bound covers both)
        if (Q.level != level && Q.level != level - 1) throw std::runtime_error("CMult: unexpected level");
        std::vector<double> dq = crypto::DecryptFloatVectorDev(T.get(), Q, slots);
        for (size_t t = 0; t < slots; t++) worst_sq = std::max(worst_sq, std::fabs(dq[t] - vals[t] * vals[t]));
        std::cout.precision(17);
        std::cout << "OK " << worst_rot << " " << worst_sq << " " << gElems.size() << std::endl;
        return 0;
    } catch (const std::exception &e) { std::cerr << "ERROR: " << e.what() << std::endl; return 1; }
}
