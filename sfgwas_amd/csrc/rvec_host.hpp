// rvec_host.hpp — the host arithmetic of the ring-vector encoder / decoder (rvec.hip): the base roots of rvec_roots.hpp brought to the table's fixed point, the
// split of the scale, the limb count W and the binary point of a call, and the static refusals.  Plain C++ (no HIP): tests/host/host_rvec_test.cpp runs it on the CPU.
#pragma once
#include <cmath>
#include <cstdint>
#include "rvec_roots.hpp"

constexpr int RVEC_TW_LIMBS = 9;            // words of a table entry: two's complement, 64 * 9 - 2 = 574 fractional bits (1.0 = 2^574)
constexpr int RVEC_WMAX = 8;                // widest data word the kernels are instantiated for
constexpr int RVEC_WMIN = 2;
constexpr int RVEC_GUARD = 48;              // fractional bits kept below the 2^-32 contract: the worst-case error of the transform is below 2^16 units
constexpr int RVEC_LOGN_SLOTS = 13;
constexpr int RVEC_MAX_FRAC = 62;

// scale = mant * 2^exp exactly, 2^52 <= mant < 2^53;  floor(log2 scale), ceil(log2 scale)
struct RvecScale { uint64_t mant; int exp, floor_log2, ceil_log2; };
inline bool rvec_scale_split(double scale, RvecScale &s) {          // false: not a finite double >= 1
    if (!(scale >= 1.0) || !std::isfinite(scale)) return false;
    int e = 0;
    const double m = std::frexp(scale, &e);                         // scale = m 2^e, 0.5 <= m < 1
    s.mant = (uint64_t)std::ldexp(m, 53);
    s.exp = e - 53;
    s.floor_log2 = e - 1;
    s.ceil_log2 = m == 0.5 ? e - 1 : e;
    return true;
}
inline int rvec_bitlen(const uint64_t *w, int nw) {
    for (int i = nw - 1; i >= 0; i--) if (w[i]) return 64 * i + 64 - __builtin_clzll(w[i]);
    return 0;
}
// bit length of q_0 q_1 ... q_level (at most 16 moduli below 2^62)
inline int rvec_chain_bitlen(const uint64_t *q, int level) {
    uint64_t acc[17] = {1};
    int nw = 1;
    for (int i = 0; i <= level && i < 16; i++) {
        uint64_t carry = 0;
        for (int k = 0; k < nw; k++) { const unsigned __int128 m = (unsigned __int128)acc[k] * q[i] + carry; acc[k] = (uint64_t)m; carry = (uint64_t)(m >> 64); }
        if (carry) acc[nw++] = carry;
    }
    return rvec_bitlen(acc, nw);
}
// base root exp(i pi / 2^k), k = 1..15, at the table's fixed point: the committed 576-bit words shifted down by two (truncated)
inline void rvec_root_words(int k, uint64_t (&c)[RVEC_TW_LIMBS], uint64_t (&s)[RVEC_TW_LIMBS]) {
    static_assert(RVEC_ROOT_FRAC_BITS == 64 * RVEC_TW_LIMBS && RVEC_ROOT_WORDS == RVEC_TW_LIMBS + 1, "root format");
    for (int i = 0; i < RVEC_TW_LIMBS; i++) {
        c[i] = (RVEC_ROOT_COS[k - 1][i] >> 2) | (RVEC_ROOT_COS[k - 1][i + 1] << 62);
        s[i] = (RVEC_ROOT_SIN[k - 1][i] >> 2) | (RVEC_ROOT_SIN[k - 1][i + 1] << 62);
    }
}

// what a call runs with: W 64-bit words per real number, g fractional bits, and the final shift
//   encode: p = round(|y| mant 2^-shift)                   shift = g + f + 13 - exp > 0
//   decode: r = floor((|y| 2^shift + mant) / (2 mant))     shift = f - g - exp + 1, either sign
struct RvecPlan { int W, g, shift; RvecScale sc; };

inline const char *rvec_check_field(int limbs, const uint64_t *mod) {
    if (limbs != 2 && limbs != 4) return "field elements of 2 or 4 words only";
    if (!mod) return "no field modulus";
    if (!(mod[0] & 1)) return "the field modulus must be odd";
    if (rvec_bitlen(mod, limbs) < 2) return "the field modulus must be at least 3";
    return nullptr;
}
inline const char *rvec_check_common(int n_elem, int level, int nq, double scale, int frac_bits, RvecScale &sc) {
    if (n_elem < 1 || n_elem > (1 << RVEC_LOGN_SLOTS)) return "element count out of range (1..8192)";
    if (level < 0 || level >= nq) return "level out of range";
    if (!rvec_scale_split(scale, sc)) return "the scale must be finite and at least 1";
    if (frac_bits < 0 || frac_bits > RVEC_MAX_FRAC) return "frac_bits out of range (0..62)";
    return nullptr;
}
inline int rvec_words_for(int bits) { const int w = (bits + 63) / 64; return w < RVEC_WMIN ? RVEC_WMIN : w; }

inline const char *rvec_plan_encode(int limbs, const uint64_t *mod, const uint64_t *q, int nq, int n_elem, int level, double scale, int frac_bits, RvecPlan &pl) {
    if (const char *e = rvec_check_field(limbs, mod)) return e;
    if (const char *e = rvec_check_common(n_elem, level, nq, scale, frac_bits, pl.sc)) return e;
    const int pb = rvec_bitlen(mod, limbs), qb = rvec_chain_bitlen(q, level);
    // |p_c| <= scale 2^-f max |s_t| < 2^(pb - 1 - f + ceil log2 scale) must stay below Q_level / 2 with a bit to spare
    if (!(pb - 1 - frac_bits + pl.sc.ceil_log2 + 1 < qb - 1)) return "level too small for the field at this scale and frac_bits";
    const int amp = pl.sc.ceil_log2 - frac_bits - RVEC_LOGN_SLOTS;                    // log2 of output units per unit of the transform
    pl.g = RVEC_GUARD + (amp > 0 ? amp : 0);
    pl.W = rvec_words_for((pb - 1) + RVEC_LOGN_SLOTS + 2 + pl.g + 1);                 // magnitude, growth of the sum, binary point, sign
    if (pl.W > RVEC_WMAX) return "scale and frac_bits need more than 8 words of precision";
    pl.shift = pl.g + frac_bits + RVEC_LOGN_SLOTS - pl.sc.exp;
    return nullptr;
}
inline const char *rvec_plan_decode(int limbs, const uint64_t *mod, const uint64_t *q, int nq, int n_elem, int level, double scale, int frac_bits, RvecPlan &pl) {
    if (const char *e = rvec_check_field(limbs, mod)) return e;
    if (const char *e = rvec_check_common(n_elem, level, nq, scale, frac_bits, pl.sc)) return e;
    const int qb = rvec_chain_bitlen(q, level);
    const int amp = frac_bits - pl.sc.floor_log2;
    pl.g = RVEC_GUARD + (amp > 0 ? amp : 0);
    pl.W = rvec_words_for(qb + (RVEC_LOGN_SLOTS + 1) + 2 + pl.g + 1);
    if (pl.W > RVEC_WMAX) return "scale and frac_bits need more than 8 words of precision";
    pl.shift = frac_bits - pl.g - pl.sc.exp + 1;
    return nullptr;
}
