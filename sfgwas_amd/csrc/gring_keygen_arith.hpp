// gring_keygen_arith.hpp - per-element arithmetic of the general ring's key generation (gring_keygen.hip): where the g_i term applies, the epilogues that form a
// share word from the transformed error and the operands, the lift of a sum of two errors, and the common reference polynomials' candidate map.  Every function
// is __host__ __device__ and plain C++ over gring_arith.hpp (canonical u64 residues, q < 2^61), so tests/host/host_gring_keygen_test.cpp runs on the CPU the very
// functions the kernels run.  Each bound is written beside the code that needs it.  DESIGN.md section 16.
#pragma once
#include "gring_arith.hpp"
#include "gring_io_arith.hpp"

namespace gkg {
using gr::u64;
using gr::u128;

// g_i at modulus m is P mod q_m when m is one of Q's moduli and belongs to digit i (digits of np consecutive moduli), else 0
GR_HD bool g_applies(int digit, int m, int nq, int np) { return m < nq && m / np == digit; }

// public-key and rotation-key shares, and h0 of the relinearisation key's round 1:   eh - a b (+ P s)
//   shares: a = crp, b = sk read through the index of g^-1 (the public key: sk itself), s = sk;   round 1: a = crp, b = NTT(u), s = sk
// eh, a, b, s canonical (< q); pg = P mod q < q with its Shoup quotient.  mulmod returns [0, q); submod of two canonical words is canonical; shoup returns
// [0, q) for every 64-bit argument; addmod of two canonical words: the sum is below 2q < 2^62.
GR_HD u64 share(u64 eh, u64 a, u64 b, u64 s, bool with_g, u64 pg, u64 pg_sh, u64 q, u64 uhi, u64 ulo) {
    u64 r = gr::submod(eh, gr::mulmod(a, b, q, uhi, ulo), q);
    if (with_g) r = gr::addmod(r, gr::shoup(s, pg, pg_sh, q), q);
    return r;
}
// h1 of round 1:   eh + s a   (s = sk, a = crp)
GR_HD u64 round1_h1(u64 eh, u64 a, u64 s, u64 q, u64 uhi, u64 ulo) { return gr::addmod(eh, gr::mulmod(s, a, q, uhi, ulo), q); }
// round 2:   eh + s h0 + (u - s) h1   with eh = NTT(e2 + e3).  The two products are below q^2 < 2^122 each, their sum below 2^123 fits 128 bits and takes ONE
// reduction; u - s is canonical by submod.
GR_HD u64 round2(u64 eh, u64 h0, u64 h1, u64 s, u64 uh, u64 q, u64 uhi, u64 ulo) {
    const u128 S = (u128)s * h0 + (u128)gr::submod(uh, s, q) * h1;
    return gr::addmod(eh, gr::barrett128((u64)(S >> 64), (u64)S, q, uhi, ulo), q);
}
// e2 + e3 as one canonical residue: each is lifted on its own and the residues are added (the sum of two int32 may leave int32)
GR_HD u64 lift_sum(int32_t a, int32_t b, u64 q) { return gr::addmod(gio::lift(a, q), gio::lift(b, q), q); }

// ---- the automorphism index (lattigo ring.PermuteNTTIndex, what sfg_ring_load_rotkey builds): out[i] = in[index[i]] is phi_g in the NTT domain
// the low `bits` bits of x reversed (1 <= bits <= 32): five swaps reverse all 32, the shift drops the rest
GR_HD uint32_t brev(uint32_t x, int bits) {
    x = (x >> 16) | (x << 16);
    x = ((x & 0xFF00FF00u) >> 8) | ((x & 0x00FF00FFu) << 8);
    x = ((x & 0xF0F0F0F0u) >> 4) | ((x & 0x0F0F0F0Fu) << 4);
    x = ((x & 0xCCCCCCCCu) >> 2) | ((x & 0x33333333u) << 2);
    x = ((x & 0xAAAAAAAAu) >> 1) | ((x & 0x55555555u) << 1);
    return x >> (32 - bits);
}
// g odd and below 2N, i < N: g t1 & mask is odd, so t2 < N and the entry is below N
GR_HD uint32_t index_entry(u64 g, int i, int logN) {
    const u64 mask = (2ULL << logN) - 1;
    const u64 t1 = 2ULL * brev((uint32_t)i, logN) + 1, t2 = ((g * t1 & mask) - 1) >> 1;
    return brev((uint32_t)t2, logN);
}
// g^-1 mod 2N, g odd: g g == 1 mod 8, and Newton's iteration doubles the correct low bits (3 -> 6 -> 12 -> 24 >= 17)
GR_HD u64 galois_inverse(u64 g, int logN) {
    const u64 mask = (2ULL << logN) - 1; u64 x = g;
    for (int i = 0; i < 4; i++) x = (x * (2 - g * x)) & mask;
    return x;
}
// the element whose index table a rotation share for g reads sk through: the key switches from phi_{g^-1}(s)
GR_HD u64 share_galois(u64 g, int logN) { return galois_inverse(g, logN); }

// ---- the common reference polynomials (DESIGN.md section 11's map, unchanged): a candidate is 64 stream bits masked to bitlen(q) bits
GR_HD u64 crp_mask(u64 q) { return ~0ULL >> __builtin_clzll(q); }                                  // q >= 3: bitlen(q) ones; q <= mask < 2q, so a candidate passes with probability > 1/2
// the first of the block's eight candidates (word 2k low, 2k + 1 high) below q; false when none is (the caller takes the next try)
GR_HD bool crp_pick(const unsigned (&w)[16], u64 q, u64 mask, u64 &val) {
    bool found = false;
    for (int k = 7; k >= 0; k--) { const u64 cand = (((u64)w[2 * k + 1] << 32) | w[2 * k]) & mask; if (cand < q) { val = cand; found = true; } }
    return found;
}
}  // namespace gkg
