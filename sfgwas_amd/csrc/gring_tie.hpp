// gring_tie.hpp - the exact re-derivation of a diagonal coefficient that the double-double encoder cannot prove rounded (gring_matmul.hip: k_gr_mm_tie; DESIGN.md
// section 18): the fixed-point cosine table of a ring and its builder, the fold of an angle to the table, the multi-word signed sum of one coefficient and the way
// from that sum to the rounded integer or to "unproven".  What the kernel runs is GR_HD and plain C++ (128-bit integers, no intrinsic); the builder is host code on
// the standard library alone: tests/host/host_gring_tie_test.cpp holds all of it on the CPU.
//
// The statement (tests/exactref.py's): p_j = (scale / n) sum_t v_t cos(pi (5^t j mod 2N) / N), j < N, rounded half away from zero, v_t integers in -128 .. 127.
//   * cos(pi k / N), k = 0 .. N / 2, is kept as round(cos 2^F), F = 191, in three 64-bit words (1 = 2^191 fits); every entry is within ONE unit 2^-F of the cosine
//     (kTabErr; the builder's bound is beside it).  The other angles by symmetry: cos(2 pi - x) = cos x, cos(pi - x) = -cos x.
//   * X = sum_t v_t c_t is a signed 256-bit integer: |X| <= 2^7 n 2^F <= 2^213.
//   * scale = m 2^e with the integer m in [2^52, 2^53): Y = m |X| < 2^267 in five words, and |p| = Y / 2^sh exactly as the table has it, sh = F + log2 n - e.
//   * The table's error is all that is left: |X - X_true| <= kTabErr A, A = sum_t |v_t|, so |Y - Y_true| <= M = m kTabErr A (< 2^76), in units 2^-sh of p:
//     S 2^-F kTabErr with S = scale A / n.  A coefficient is PROVEN when its distance from the tie, in those units, is strictly above M; an exact tie (distance 0)
//     never is.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>
#include "gring_arith.hpp"
#include "gring_tie_roots.hpp"

namespace gtie {
using gr::u64;
using gr::u128;

constexpr int kFrac = 191;                  // F: fractional bits of a table entry
constexpr int kWords = 3;                   // 64-bit words of a table entry
constexpr u64 kTabErr = 1;                  // every entry is within kTabErr 2^-F of the cosine
constexpr int kCap = 512;                   // entries of the list of flagged coefficients of one batch of diagonals; an entry past it counts as unproven

// ---------------------------------------------------------------- the fold: an angle pi a / N, 0 <= a < 2N, to the table index k <= N / 2 and a sign
GR_HD unsigned fold(unsigned a, unsigned N, bool &neg) {
    if (a > N) a = 2 * N - a;               // cos(2 pi - x) = cos x
    neg = a > N / 2;                        // cos(pi - x) = -cos x
    return neg ? N - a : a;
}

// ---------------------------------------------------------------- the sum: 256 bits, two's complement; |sum| <= 2^213 at every prefix
struct Acc {
    u64 w[4];
    GR_HD void zero() { w[0] = w[1] = w[2] = w[3] = 0; }
    // += v c, |v| <= 2^7, c the three words of a table entry (v c < 2^199)
    GR_HD void addmul(const u64 *c, int v, bool neg) {
        const u64 mag = (u64)(v < 0 ? -v : v);
        if (v < 0) neg = !neg;
        u128 t = (u128)c[0] * mag; u64 p0 = (u64)t;
        t = (t >> 64) + (u128)c[1] * mag; u64 p1 = (u64)t;
        t = (t >> 64) + (u128)c[2] * mag; u64 p2 = (u64)t, p3 = (u64)(t >> 64);
        if (neg) { p0 = ~p0; p1 = ~p1; p2 = ~p2; p3 = ~p3; }               // -x = ~x + 1
        u128 s = (u128)w[0] + p0 + (neg ? 1u : 0u); w[0] = (u64)s;
        s = (s >> 64) + w[1] + p1; w[1] = (u64)s;
        s = (s >> 64) + w[2] + p2; w[2] = (u64)s;
        s = (s >> 64) + w[3] + p3; w[3] = (u64)s;
    }
};

// ---------------------------------------------------------------- five-word helpers: every index is a constant after unrolling (no array leaves the registers)
// is any bit at position >= k set (k >= 0)
GR_HD bool any_above(const u64 *Y, int k) {
    bool r = false;
    for (int i = 0; i < 5; i++) {
        const int lo = 64 * i;
        if (k <= lo) r = r || Y[i] != 0;
        else if (k < lo + 64) r = r || (Y[i] >> (k - lo)) != 0;
    }
    return r;
}
// the 64 bits at positions pos .. pos + 63 (0 <= pos < 320; bits beyond the fifth word are zero)
GR_HD u64 bits_at(const u64 *Y, int pos) {
    u64 r = 0;
    for (int i = 0; i < 5; i++) {
        const int lo = 64 * i;
        if (pos >= lo && pos < lo + 64) {
            const int s = pos - lo;
            r = Y[i] >> s;
            if (s && i + 1 < 5) r |= Y[i + 1] << (64 - s);
        }
    }
    return r;
}
// g = Y mod 2^k (0 <= k <= 320)
GR_HD void low_bits(const u64 *Y, int k, u64 *g) {
    for (int i = 0; i < 5; i++) {
        const int lo = 64 * i;
        g[i] = k >= lo + 64 ? Y[i] : k <= lo ? 0 : Y[i] & ((1ULL << (k - lo)) - 1);
    }
}

// ---------------------------------------------------------------- the decision
// X: the sum (two's complement, |X| <= 2^213); scale = m 2^e, 2^52 <= m < 2^53; A = sum |v_t| <= 2^22.
// 0 = proven, p set (round half away from zero, |p| < 2^62); 1 = too close to a tie to prove (an exact tie included); 2 = outside the domain |p| < 2^62.
GR_HD int decide(const u64 *X, u64 m, int e, int logn, u64 A, long long &p) {
    p = 0;
    const bool neg = (X[3] >> 63) != 0;
    u64 a[4];
    if (neg) {
        u128 s = (u128)(~X[0]) + 1; a[0] = (u64)s;
        s = (s >> 64) + (~X[1]); a[1] = (u64)s;
        s = (s >> 64) + (~X[2]); a[2] = (u64)s;
        s = (s >> 64) + (~X[3]); a[3] = (u64)s;
    } else { a[0] = X[0]; a[1] = X[1]; a[2] = X[2]; a[3] = X[3]; }
    u64 Y[5];
    u128 t = (u128)a[0] * m; Y[0] = (u64)t;
    t = (t >> 64) + (u128)a[1] * m; Y[1] = (u64)t;
    t = (t >> 64) + (u128)a[2] * m; Y[2] = (u64)t;
    t = (t >> 64) + (u128)a[3] * m; Y[3] = (u64)t; Y[4] = (u64)(t >> 64);
    if (!(Y[0] | Y[1] | Y[2] | Y[3] | Y[4])) return 0;                      // an exact zero: half a unit from either tie
    const int sh = kFrac + logn - e;                                        // |p| = Y / 2^sh; e >= -52 (scale >= 1) keeps sh <= 258
    if (sh <= 0) {                                                          // Y 2^-sh is an integer: no rounding, no tie
        if (-sh >= 62 || any_above(Y, 62 + sh)) return 2;
        const long long v = (long long)(Y[0] << -sh);
        p = neg ? -v : v;
        return 0;
    }
    if (sh + 62 < 320 && any_above(Y, sh + 62)) return 2;                   // the integer part is at least 2^62
    u64 ip = sh < 320 ? bits_at(Y, sh) : 0;                                 // below 2^62
    const bool up = (bits_at(Y, sh - 1) & 1) != 0;                          // the fraction is at least one half
    // distance from the tie, units 2^-sh: g = Y mod 2^(sh-1) above it when `up`, 2^(sh-1) - g below it otherwise; proven when it exceeds M
    u64 g[5]; low_bits(Y, sh - 1, g);
    const u128 M = (u128)m * (kTabErr * A);
    bool proven;
    if (up) proven = (g[2] | g[3] | g[4]) != 0 || (((u128)g[1] << 64) | g[0]) > M;
    else {                                                                  // 2^(sh-1) - g > M  <=>  g + M < 2^(sh-1)
        u64 s5[5];
        u128 s = (u128)g[0] + (u64)M; s5[0] = (u64)s;
        s = (s >> 64) + g[1] + (u64)(M >> 64); s5[1] = (u64)s;
        s = (s >> 64) + g[2]; s5[2] = (u64)s;
        s = (s >> 64) + g[3]; s5[3] = (u64)s;
        s = (s >> 64) + g[4]; s5[4] = (u64)s;                               // g < 2^257, M < 2^76: no carry out
        proven = !any_above(s5, sh - 1);
    }
    if (up) ip += 1;
    if (ip >= (1ULL << 62)) return 2;
    p = neg ? -(long long)ip : (long long)ip;
    return proven ? 0 : 1;
}

// ---------------------------------------------------------------- host only from here
// scale = m 2^e, m an integer in [2^52, 2^53); scale finite and positive
inline void split_scale(double scale, u64 &m, int &e) {
    int ex; const double fr = std::frexp(scale, &ex);                       // scale = fr 2^ex, 1/2 <= fr < 1
    m = (u64)std::ldexp(fr, 53); e = ex - 53;
}

// The table of a ring: entry k = round(cos(pi k / N) 2^F), k = 0 .. N / 2, kWords words each, little endian.  logN = 12 .. 16.
// Built at 256 fractional bits (five words, 1 = 2^256) from the committed base roots exp(i pi / 2^r), r = 1 .. 16 (each component within 2^-257):
// z_j = z_(j - h) root(h), h the highest bit of j, so an entry is reached by at most 15 complex products.  A product's four word products are truncated (below
// 2^-256 each, two a component) and carry the operands' errors E_a, E_b times |c| + |s| <= sqrt 2:  E' <= sqrt 2 (E_a + 2^-257) + 2^-255 < sqrt 2 E_a + 2^-254,
// below 2^-245 after 15 of them.  The rounding to F bits adds 2^-192: every entry is within 2^-192 + 2^-245 < kTabErr 2^-191 of the cosine.  All angles lie in
// [0, pi / 2]: cosine and sine are non-negative, and the one difference c1 c2 - s1 s2 is a cosine of at least sin(pi / N) > 2^-15, far above the error (the
// angle pi / 2 itself is a base root and is not multiplied).
struct Fx5 { u64 w[5]; };
inline Fx5 fx5_mul(const Fx5 &a, const Fx5 &b) {                             // floor(a b / 2^256), a, b <= 2^256
    u64 prod[10] = {0};
    for (int i = 0; i < 5; i++) {
        u64 carry = 0;
        for (int k = 0; k < 5; k++) { const u128 t = (u128)a.w[i] * b.w[k] + prod[i + k] + carry; prod[i + k] = (u64)t; carry = (u64)(t >> 64); }
        prod[i + 5] = carry;
    }
    Fx5 r; for (int i = 0; i < 5; i++) r.w[i] = prod[i + 4];
    return r;
}
inline Fx5 fx5_add(const Fx5 &a, const Fx5 &b) { Fx5 r; u128 s = 0; for (int i = 0; i < 5; i++) { s = (s >> 64) + a.w[i] + b.w[i]; r.w[i] = (u64)s; } return r; }
inline Fx5 fx5_sub_clamped(const Fx5 &a, const Fx5 &b) {                     // a - b, zero where the difference would be negative
    Fx5 r; u64 borrow = 0;
    for (int i = 0; i < 5; i++) { const u128 d = (u128)a.w[i] - b.w[i] - borrow; r.w[i] = (u64)d; borrow = (u64)(d >> 64) & 1; }
    if (borrow) for (int i = 0; i < 5; i++) r.w[i] = 0;
    return r;
}
inline std::vector<u64> build_table(int logN) {
    static_assert(GRING_TIE_ROOT_FRAC_BITS == 256 && GRING_TIE_ROOT_WORDS == 5 && GRING_TIE_NROOTS >= 16, "the builder's fixed point");
    const size_t N = (size_t)1 << logN, half = N / 2;
    std::vector<Fx5> c(half + 1), s(half + 1);
    for (int i = 0; i < 5; i++) { c[0].w[i] = i == 4 ? 1 : 0; s[0].w[i] = 0; }
    for (size_t j = 1; j <= half; j++) {
        int b = 0; while (((size_t)2 << b) <= j) b++;                        // 2^b the highest bit of j: the angle pi 2^b / N = pi / 2^(logN - b)
        Fx5 rc, rs; for (int i = 0; i < 5; i++) { rc.w[i] = GRING_TIE_ROOT_COS[logN - b - 1][i]; rs.w[i] = GRING_TIE_ROOT_SIN[logN - b - 1][i]; }
        const size_t rest = j - ((size_t)1 << b);
        if (!rest) { c[j] = rc; s[j] = rs; continue; }
        c[j] = fx5_sub_clamped(fx5_mul(c[rest], rc), fx5_mul(s[rest], rs));
        s[j] = fx5_add(fx5_mul(s[rest], rc), fx5_mul(c[rest], rs));
    }
    std::vector<u64> tab((half + 1) * kWords);
    constexpr int drop = GRING_TIE_ROOT_FRAC_BITS - kFrac;                   // 65: add half a unit, drop the bits
    static_assert(drop > 64 && drop < 128, "the rounding below shifts by one word and a part");
    for (size_t j = 0; j <= half; j++) {
        Fx5 v = c[j]; u128 t = (u128)v.w[1] + ((u64)1 << (drop - 64 - 1));    // + 2^(drop - 1)
        v.w[1] = (u64)t;
        for (int i = 2; i < 5; i++) { t = (t >> 64) + v.w[i]; v.w[i] = (u64)t; }
        for (int i = 0; i < kWords; i++) tab[j * kWords + i] = (v.w[i + 1] >> (drop - 64)) | (i + 2 < 5 ? v.w[i + 2] << (128 - drop) : 0);
    }
    return tab;
}
// one coefficient from the slot values as the kernel forms it (the kernel strides the same terms over a workgroup): 0 / 1 / 2 as decide()
inline int coefficient(const std::vector<u64> &tab, int logN, const int *v, unsigned j, double scale, long long &p) {
    const unsigned N = 1u << logN, n = N / 2;
    Acc X; X.zero(); u64 A = 0; unsigned g = 1;
    for (unsigned t = 0; t < n; t++, g = g * 5 % (2 * N)) {
        if (!v[t]) continue;
        bool neg; const unsigned k = fold((unsigned)(((u64)g * j) % (2 * N)), N, neg);
        X.addmul(&tab[(size_t)k * kWords], v[t], neg);
        A += (u64)(v[t] < 0 ? -v[t] : v[t]);
    }
    u64 m; int e; split_scale(scale, m, e);
    return decide(X.w, m, e, logN - 1, A, p);
}
}  // namespace gtie
