// rvec_fx.hpp — the W-word fixed-point arithmetic of the ring-vector encoder / decoder and what one thread of each kernel of rvec.hip does to one element.
// Host and device: the kernels of rvec.hip only add the addressing, and tests/host/host_rvec_test.cpp runs the same functions over a whole transform on the CPU.
// A real number is a two's-complement integer of W 64-bit words with g fractional bits; a twiddle has 64 W - 2 fractional bits.  Integer arithmetic only.
#pragma once
#include <cstdint>
#include "rvec_host.hpp"

#ifdef __HIPCC__
#define RVEC_HD __host__ __device__ __forceinline__
#define RVEC_UNROLL _Pragma("unroll")
#else
#define RVEC_HD inline
#define RVEC_UNROLL
#endif
typedef unsigned long long rv_u64;
typedef unsigned __int128 rv_u128;

struct RvecField { rv_u64 p[4], half[4]; int limbs; };                      // half = (p - 1) / 2, words above `limbs` zero
inline void rvec_field(int limbs, const uint64_t *mod, RvecField &f) {
    for (int i = 0; i < 4; i++) f.p[i] = i < limbs ? mod[i] : 0;
    for (int i = 0; i < 4; i++) f.half[i] = (f.p[i] >> 1) | (i + 1 < 4 ? f.p[i + 1] << 63 : 0);          // p odd
    f.limbs = limbs;
}

template <int W> RVEC_HD bool fx_isneg(const rv_u64 (&x)[W]) { return (long long)x[W - 1] < 0; }
template <int W> RVEC_HD void fx_negate(rv_u64 (&x)[W]) {
    bool c = true;
    RVEC_UNROLL
    for (int i = 0; i < W; i++) { const rv_u64 v = ~x[i] + (c ? 1ULL : 0ULL); c = c && v == 0; x[i] = v; }
}
template <int W> RVEC_HD void fx_add(const rv_u64 (&a)[W], const rv_u64 (&b)[W], rv_u64 (&r)[W]) {
    rv_u64 c = 0;
    RVEC_UNROLL
    for (int i = 0; i < W; i++) { const rv_u64 s = a[i] + b[i]; const rv_u64 c1 = s < a[i]; const rv_u64 s2 = s + c; c = c1 | (rv_u64)(s2 < s); r[i] = s2; }
}
template <int W> RVEC_HD void fx_sub(const rv_u64 (&a)[W], const rv_u64 (&b)[W], rv_u64 (&r)[W]) {
    rv_u64 br = 0;
    RVEC_UNROLL
    for (int i = 0; i < W; i++) { const rv_u64 d = a[i] - b[i]; const rv_u64 b1 = a[i] < b[i]; const rv_u64 d2 = d - br; br = b1 | (rv_u64)(d < br); r[i] = d2; }
}
template <int W> RVEC_HD int fx_cmp(const rv_u64 (&a)[W], const rv_u64 (&b)[W]) {      // unsigned compare: -1, 0, 1
    for (int i = W - 1; i >= 0; i--) if (a[i] != b[i]) return a[i] > b[i] ? 1 : -1;
    return 0;
}
// r = x t 2^-(64 W - 2), truncated towards zero: x any W-word integer, t a twiddle (|t| <= 2^(64 W - 2)).  Sign-magnitude: the full 2 W-word product of the
// magnitudes (W^2 64 x 64 -> 128-bit multiply-adds, 32-bit multiply-add chains on the device), shifted down once.
template <int W> RVEC_HD void fx_mul_tw(const rv_u64 (&x)[W], const rv_u64 (&t)[W], rv_u64 (&r)[W]) {
    rv_u64 ax[W], at[W], p[2 * W];
    const bool sx = fx_isneg<W>(x), st = fx_isneg<W>(t);
    RVEC_UNROLL
    for (int i = 0; i < W; i++) { ax[i] = x[i]; at[i] = t[i]; p[i] = 0; p[W + i] = 0; }
    if (sx) fx_negate<W>(ax);
    if (st) fx_negate<W>(at);
    RVEC_UNROLL
    for (int i = 0; i < W; i++) {
        rv_u64 c = 0;
        RVEC_UNROLL
        for (int j = 0; j < W; j++) { const rv_u128 m = (rv_u128)ax[i] * at[j] + p[i + j] + c; p[i + j] = (rv_u64)m; c = (rv_u64)(m >> 64); }
        p[i + W] = c;
    }
    RVEC_UNROLL
    for (int k = 0; k < W; k++) r[k] = (p[W - 1 + k] >> 62) | (p[W + k] << 2);
    if (sx != st) fx_negate<W>(r);
}
// (xr + i xi) (tr + i ti)
template <int W> RVEC_HD void fx_cmul(const rv_u64 (&xr)[W], const rv_u64 (&xi)[W], const rv_u64 (&tr)[W], const rv_u64 (&ti)[W], rv_u64 (&yr)[W], rv_u64 (&yi)[W]) {
    rv_u64 a[W], b[W];
    fx_mul_tw<W>(xr, tr, a); fx_mul_tw<W>(xi, ti, b); fx_sub<W>(a, b, yr);
    fx_mul_tw<W>(xr, ti, a); fx_mul_tw<W>(xi, tr, b); fx_add<W>(a, b, yi);
}
// r (NR words) = a (NA words, unsigned) shifted left by sh >= 0 bits; bits beyond NR words are lost (the callers' bounds exclude that)
template <int NA, int NR> RVEC_HD void mp_shl(const rv_u64 (&a)[NA], int sh, rv_u64 (&r)[NR]) {
    const int ws = sh >> 6, bs = sh & 63;
    RVEC_UNROLL
    for (int k = 0; k < NR; k++) {
        rv_u64 v = 0;
        RVEC_UNROLL
        for (int i = 0; i < NA; i++) {
            if (i + ws == k) v |= a[i] << bs;
            if (bs && i + ws + 1 == k) v |= a[i] >> (64 - bs);
        }
        r[k] = v;
    }
}
// r = a shifted right by sh >= 0 bits (floor; zero from 64 NA bits on)
template <int NA> RVEC_HD void mp_shr(const rv_u64 (&a)[NA], int sh, rv_u64 (&r)[NA]) {
    const int ws = sh >> 6, bs = sh & 63;
    RVEC_UNROLL
    for (int k = 0; k < NA; k++) {
        rv_u64 v = 0;
        RVEC_UNROLL
        for (int i = 0; i < NA; i++) {
            if (i - ws == k) v |= a[i] >> bs;
            if (bs && i - ws - 1 == k) v |= a[i] << (64 - bs);
        }
        r[k] = v;
    }
}

// ---------------------------------------------------------------- the table: zeta^j from the base roots, roots [14][2][9] words, root b = zeta^(2^b)
RVEC_HD void rvec_table_entry(const rv_u64 *roots, int j, rv_u64 (&ar)[RVEC_TW_LIMBS], rv_u64 (&ai)[RVEC_TW_LIMBS]) {
    constexpr int T = RVEC_TW_LIMBS;
    RVEC_UNROLL
    for (int k = 0; k < T; k++) { ar[k] = 0; ai[k] = 0; }
    ar[T - 1] = 1ULL << 62;                                              // 1.0
    for (int b = 0; b < 14; b++) {
        if (!((j >> b) & 1)) continue;
        rv_u64 rr[T], ri[T], yr[T], yi[T];
        RVEC_UNROLL
        for (int k = 0; k < T; k++) { rr[k] = roots[(b * 2) * T + k]; ri[k] = roots[(b * 2 + 1) * T + k]; }
        fx_cmul<T>(ar, ai, rr, ri, yr, yi);
        RVEC_UNROLL
        for (int k = 0; k < T; k++) { ar[k] = yr[k]; ai[k] = yi[k]; }
    }
}
inline void rvec_host_roots(rv_u64 *roots /* [14][2][9] */) {
    for (int b = 0; b < 14; b++) {
        uint64_t c[RVEC_TW_LIMBS], s[RVEC_TW_LIMBS];
        rvec_root_words(14 - b, c, s);
        for (int k = 0; k < RVEC_TW_LIMBS; k++) { roots[(b * 2) * RVEC_TW_LIMBS + k] = c[k]; roots[(b * 2 + 1) * RVEC_TW_LIMBS + k] = s[k]; }
    }
}

// ---------------------------------------------------------------- one butterfly, in place: (a, b) <- (a + b w, a - b w)
template <int W> RVEC_HD void rvec_butterfly(rv_u64 (&ar)[W], rv_u64 (&ai)[W], rv_u64 (&br)[W], rv_u64 (&bi)[W], const rv_u64 (&tr)[W], const rv_u64 (&ti)[W]) {
    rv_u64 yr[W], yi[W], sr[W], si[W];
    fx_cmul<W>(br, bi, tr, ti, yr, yi);
    fx_sub<W>(ar, yr, br); fx_sub<W>(ai, yi, bi);
    fx_add<W>(ar, yr, sr); fx_add<W>(ai, yi, si);
    RVEC_UNROLL
    for (int k = 0; k < W; k++) { ar[k] = sr[k]; ai[k] = si[k]; }
}

// ---------------------------------------------------------------- encode, pre-pass: v = centre(x) 2^g
template <int W> RVEC_HD void rvec_centre_place(const rv_u64 (&xin)[4], const RvecField &f, int g, rv_u64 (&v)[W]) {
    rv_u64 x[4] = {xin[0], xin[1], xin[2], xin[3]};
    const bool neg = fx_cmp<4>(x, f.half) > 0;                             // x > (p - 1)/2: the value is x - p
    if (neg) { rv_u64 d[4]; fx_sub<4>(f.p, x, d); for (int i = 0; i < 4; i++) x[i] = d[i]; }
    mp_shl<4, W>(x, g, v);
    if (neg) fx_negate<W>(v);
}
// ---------------------------------------------------------------- encode, post-pass: |rd| = round(|y| mant 2^-shift), ties away from zero; returns the sign
template <int W> RVEC_HD bool rvec_scale_round(const rv_u64 (&y)[W], rv_u64 mant, int shift, rv_u64 (&rd)[W + 1]) {
    rv_u64 a[W], pr[W + 1], hb[W + 1], sm[W + 1], one[1] = {1};
    RVEC_UNROLL
    for (int k = 0; k < W; k++) a[k] = y[k];
    const bool neg = fx_isneg<W>(a);
    if (neg) fx_negate<W>(a);
    rv_u64 cy = 0;
    RVEC_UNROLL
    for (int k = 0; k < W; k++) { const rv_u128 m = (rv_u128)a[k] * mant + cy; pr[k] = (rv_u64)m; cy = (rv_u64)(m >> 64); }
    pr[W] = cy;
    mp_shl<1, W + 1>(one, shift - 1, hb);                               // half a unit
    fx_add<W + 1>(pr, hb, sm);
    mp_shr<W + 1>(sm, shift, rd);
    return neg;
}
// the canonical residue mod q < 2^47 of the signed integer (neg, |rd|): Horner over 16-bit digits, every partial value x below 2^63, reduced by Barrett's
// quotient estimate floor(x floor(2^64 / q) / 2^64), which is floor(x / q) or one less: one conditional subtraction, one division per modulus
template <int NW> RVEC_HD rv_u64 rvec_mod_q(const rv_u64 (&rd)[NW], bool neg, rv_u64 q) {
    const rv_u64 m = ~0ULL / q;                                            // floor(2^64 / q): q is odd and above 1, so it does not divide 2^64
    rv_u64 rem = 0;
    RVEC_UNROLL
    for (int k = NW - 1; k >= 0; k--) {
        RVEC_UNROLL
        for (int h = 3; h >= 0; h--) {
            const rv_u64 x = (rem << 16) | ((rd[k] >> (16 * h)) & 0xFFFFULL);
            const rv_u64 r = x - (rv_u64)(((rv_u128)x * m) >> 64) * q;
            rem = r >= q ? r - q : r;
        }
    }
    return neg && rem ? q - rem : rem;
}
// ---------------------------------------------------------------- decode, pre-pass: the signed integer (neg, digits v_i of |p| in the mixed radix q_0, q_1, ...) times 2^g
template <int W> RVEC_HD void rvec_from_digits(const rv_u64 *digit, const rv_u64 *q, int nl, bool neg, int g, rv_u64 (&out)[W]) {
    rv_u64 acc[W];
    RVEC_UNROLL
    for (int k = 0; k < W; k++) acc[k] = 0;
    acc[0] = digit[nl - 1];
    for (int i = nl - 2; i >= 0; i--) {                                  // |p| = v0 + q0 (v1 + q1 (v2 + ...))
        rv_u64 cy = digit[i];
        RVEC_UNROLL
        for (int k = 0; k < W; k++) { const rv_u128 m = (rv_u128)acc[k] * q[i] + cy; acc[k] = (rv_u64)m; cy = (rv_u64)(m >> 64); }
    }
    mp_shl<W, W>(acc, g, out);
    if (neg) fx_negate<W>(out);
}
// ---------------------------------------------------------------- decode, post-pass: r = round(|y| 2^(shift - 1) / mant) mod p with the sign of y, ties away from zero:
// floor((floor(|y| 2^shift) + mant) / (2 mant)), the quotient bits fed straight into the reduction mod p (both bit by bit: no wide division on the device)
template <int W> RVEC_HD void rvec_div_mod_p(const rv_u64 (&y)[W], rv_u64 mant, int shift, const RvecField &f, rv_u64 (&r)[4]) {
    rv_u64 a[W + 1], sh[W + 1], mt[W + 1], num[W + 1];
    {
        rv_u64 t[W];
        RVEC_UNROLL
        for (int k = 0; k < W; k++) t[k] = y[k];
        if (fx_isneg<W>(y)) fx_negate<W>(t);
        RVEC_UNROLL
        for (int k = 0; k < W; k++) a[k] = t[k];
        a[W] = 0;
    }
    const bool neg = fx_isneg<W>(y);
    if (shift >= 0) mp_shl<W + 1, W + 1>(a, shift, sh); else mp_shr<W + 1>(a, -shift, sh);
    RVEC_UNROLL
    for (int k = 0; k <= W; k++) mt[k] = 0;
    mt[0] = mant;
    fx_add<W + 1>(sh, mt, num);
    const rv_u64 den = mant << 1;                                               // < 2^54
    rv_u64 rem = 0;
    r[0] = r[1] = r[2] = r[3] = 0;
    for (int k = W; k >= 0; k--) {
        const rv_u64 word = num[k];
        for (int bit = 63; bit >= 0; bit--) {
            rem = (rem << 1) | ((word >> bit) & 1);
            const rv_u64 qb = rem >= den ? 1ULL : 0ULL;
            if (qb) rem -= den;
            const rv_u64 top = r[3] >> 63;                                      // r = (2 r + qb) mod p
            r[3] = (r[3] << 1) | (r[2] >> 63); r[2] = (r[2] << 1) | (r[1] >> 63); r[1] = (r[1] << 1) | (r[0] >> 63); r[0] = (r[0] << 1) | qb;
            if (top || fx_cmp<4>(r, f.p) >= 0) { rv_u64 d[4]; fx_sub<4>(r, f.p, d); r[0] = d[0]; r[1] = d[1]; r[2] = d[2]; r[3] = d[3]; }
        }
    }
    if (neg && (r[0] | r[1] | r[2] | r[3])) { rv_u64 d[4]; fx_sub<4>(f.p, r, d); r[0] = d[0]; r[1] = d[1]; r[2] = d[2]; r[3] = d[3]; }
}
// a - b mod p (canonical in, canonical out)
RVEC_HD void rvec_field_sub(const rv_u64 (&x)[4], const rv_u64 (&y)[4], const RvecField &f, rv_u64 (&d)[4]) {
    const bool lt = fx_cmp<4>(x, y) < 0;
    fx_sub<4>(x, y, d);
    if (lt) { rv_u64 s[4]; fx_add<4>(d, f.p, s); for (int i = 0; i < 4; i++) d[i] = s[i]; }
}
