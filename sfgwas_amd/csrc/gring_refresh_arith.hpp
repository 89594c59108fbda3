// gring_refresh_arith.hpp - per-coefficient arithmetic of the general ring's collective bootstrap (gring_refresh.hip): a signed big integer of up to kBigLimbs
// 64-bit limbs reduced modulo a word modulus, its two's-complement negation, the rescale |a| <- floor(|a| mo 2^sh / mi) of the target-scale form (one product by a
// 53-bit mantissa, one shift, one short division), b - a, the sign rule of the recode, mixed-radix digits -> limbs, and the digits' Horner modulo a new modulus.
// Every multi-limb function is written over ACCESSORS (L(i) reads limb i, S(i, v) stores it), as gio::decode_digits takes accessors: the kernel decides where the
// limbs live (LDS planes, one coefficient a lane), the host test hands accessors of a vector.  Every function is __host__ __device__ and plain C++ (like
// gring_io_arith.hpp), so tests/host/host_gring_refresh_test.cpp runs on the CPU the very functions the kernels run.  Each bound is derived beside its code.
// PARITY UNPINNED, like refresh.hip: the semantics are lattigo v2.1.0 / v2.2.0 dckks/refresh.go as the CPU checker under oracle/ restates them.
#pragma once
#include <cstdint>
#include "gring_arith.hpp"
#include "gring_io_arith.hpp"

namespace grf {
using gr::u64;
using gr::u128;

// limbs of the device big integer: 3072 bits.  The widest Q_level a ring admits is 47 moduli below 2^61: 2867 bits; a rescale multiplies by a mantissa below 2^53
// and shifts left by sh: 2867 + 53 + sh bits.  The entry points check the fit (grf::fits_*), so no function below ever carries out of limb n - 1.
constexpr int kBigLimbs = 48;
constexpr int kBigBits = 64 * kBigLimbs;
constexpr double kMaxScale = 0x1p400;

// ---- a magnitude of n limbs modulo q < 2^61, Horner from the top limb: acc < q < 2^61, so acc 2^64 + limb < 2^125 is a legal argument of gr::barrett128
GR_HD u64 horner_limb(u64 acc, u64 limb, u64 q, u64 uhi, u64 ulo) { return gr::barrett128(acc, limb, q, uhi, ulo); }
template <class GetL>
GR_HD u64 limbs_mod(int n, GetL L, u64 q, u64 uhi, u64 ulo) {
    u64 acc = 0;
    for (int i = n - 1; i >= 0; i--) acc = horner_limb(acc, L(i), q, uhi, ulo);
    return acc;
}
// the residue of a signed value from its magnitude's: a negative value whose magnitude is == 0 mod q gives 0, not q
GR_HD u64 signed_residue(u64 m, bool neg, u64 q) { return (neg && m) ? q - m : m; }
// residue of the magnitude + a small signed e (an error coefficient): gio::lift covers q < |e|
GR_HD u64 add_small(u64 m, int32_t e, u64 q) { return gr::addmod(m, gio::lift(e, q), q); }

// ---- two's complement of W limbs -> sign and magnitude in place: |v| = ~v + 1 for a negative v; -2^(64W-1) has the magnitude 2^(64W-1), which fits W limbs
// unsigned (the carry never leaves limb W - 1: ~v + 1 = 2^(64W) only for v = 0, which is not negative).  Returns the sign.
template <class GetL, class SetL>
GR_HD bool to_magnitude(int W, GetL L, SetL S) {
    const bool neg = (L(W - 1) >> 63) != 0;
    if (neg) { u64 cy = 1; for (int i = 0; i < W; i++) { const u64 v = ~L(i) + cy; cy = (cy && v == 0) ? 1 : 0; S(i, v); } }
    return neg;
}

// ---- a <- a m + add over n limbs (m, add any words).  Returns the carry out of limb n - 1 (zero when the caller's fit check holds).
// a[i] m + c <= (2^64 - 1)^2 + 2^64 - 1 < 2^128: the 128-bit sum never wraps.
template <class GetL, class SetL>
GR_HD u64 mul_add(int n, GetL L, SetL S, u64 m, u64 add) {
    u64 c = add;
    for (int i = 0; i < n; i++) { const u128 t = (u128)L(i) * m + c; S(i, (u64)t); c = (u64)(t >> 64); }
    return c;
}
// ---- shift in place over n limbs; sh > 0 left (bits above limb n - 1 are lost: the fit check keeps them zero), sh < 0 right (floor).
// Left walks from the top limb down and reads limbs i - ws and i - ws - 1 <= i: not yet written.  Right walks up and reads i + ws, i + ws + 1 >= i.
template <class GetL, class SetL>
GR_HD void shift(int n, GetL L, SetL S, int sh) {
    if (sh == 0) return;
    const int k = sh > 0 ? sh : -sh, ws = k >> 6, bs = k & 63;
    if (sh > 0) {
        for (int i = n - 1; i >= 0; i--) {
            const int s0 = i - ws; const u64 hi = s0 >= 0 ? L(s0) : 0, lo = s0 - 1 >= 0 ? L(s0 - 1) : 0;
            S(i, bs ? (hi << bs) | (lo >> (64 - bs)) : hi);
        }
    } else {
        for (int i = 0; i < n; i++) {
            const int s0 = i + ws; const u64 lo = s0 < n ? L(s0) : 0, hi = s0 + 1 < n ? L(s0 + 1) : 0;
            S(i, bs ? (lo >> bs) | (hi << (64 - bs)) : lo);
        }
    }
}
// ---- a <- floor(a / d), 1 <= d < 2^53, a byte at a time from the top: the running remainder r < d < 2^53, so r 2^8 + byte < 2^61 stays in a word and the
// quotient byte (r 2^8 + byte) / d < 2^8.  d == 1 returns at once (Int(ct scale) = 1).
template <class GetL, class SetL>
GR_HD void div_small(int n, GetL L, SetL S, u64 d) {
    if (d == 1) return;
    u64 r = 0;
    for (int i = n - 1; i >= 0; i--) {
        const u64 w = L(i); u64 q = 0;
        for (int b = 7; b >= 0; b--) { r = (r << 8) | ((w >> (8 * b)) & 0xFF); const u64 qb = r / d; r -= qb * d; q = (q << 8) | qb; }
        S(i, q);
    }
}
// |a| <- floor(|a| mo 2^sh / mi): big.Int.Quo truncates towards zero, i.e. floor on the magnitude with the sign kept (a negative value that rescales to 0 is 0).
// A right shift before the division loses nothing: floor(floor(x / 2^k) / mi) = floor(x / (2^k mi)).
struct Ratio { u64 mo, mi; int sh; };
template <class GetL, class SetL>
GR_HD void rescale(int n, GetL L, SetL S, const Ratio &r) { (void)mul_add(n, L, S, r.mo, 0); shift(n, L, S, r.sh); div_small(n, L, S, r.mi); }

// ---- a <- b - a over n limbs, b >= a (b = Q_level, a = x with Q / 2 <= x < Q): the borrow never leaves limb n - 1
template <class GetL, class GetB, class SetL>
GR_HD void rsub(int n, GetL L, GetB B, SetL S) {
    u64 br = 0;
    for (int i = 0; i < n; i++) { const u64 bi = B(i), ai = L(i), d = bi - ai, d2 = d - br; br = (u64)((bi < ai) | (d < br)); S(i, d2); }
}

// ---- the sign of the recode, on mixed-radix digits from the top: lattigo's refresh takes x >= floor(Q / 2) as negative ("all digits equal counts as negative"),
// where the decoder (gio::cmp_step users) takes x > floor(Q / 2).  The walk and the half-digit table are the decoder's; the comparison of the result is not.
GR_HD bool negative_from_cmp(int state) { return state >= 0; }
template <class GetD, class GetH>
GR_HD bool is_negative(int nl, GetD D, GetH H) {
    int st = 0;
    for (int i = nl - 1; i >= 0; i--) st = gio::cmp_step(st, D(i), H(i));
    return negative_from_cmp(st);
}

// ---- mixed-radix digits -> limbs: x = d_0 + q_0 (d_1 + q_1 (...)), Horner from the top digit.  After k digits x < 2^(61 k) occupies at most k limbs, so the
// product runs over the limbs written so far and the carry opens the next one; the value fits n limbs (x < Q_level, n >= limbs of Q_level), so a carry at
// len == n is zero.  Limbs len .. n - 1 are cleared at the end.
template <class GetD, class GetQ, class GetL, class SetL>
GR_HD void digits_to_limbs(int nl, GetD D, GetQ Q, int n, GetL L, SetL S) {
    S(0, D(nl - 1)); int len = 1;
    for (int i = nl - 2; i >= 0; i--) {
        const u64 c = mul_add(len, L, S, Q(i), D(i));
        if (len < n) { S(len, c); len++; }
    }
    for (int i = len; i < n; i++) S(i, 0);
}

// ---- the unscaled recode at a new modulus q_j: x mod q_j by Horner over the digits with (q_i mod q_j), then - (Q_level mod q_j) when x is negative (x - Q).
// A digit d_i < q_i may exceed q_j: gio::garner_acc's 128-bit step reduces acc (q_i mod q_j) + d_i < 2^122 + 2^61 whatever d_i is.
template <class GetD, class GetM>
GR_HD u64 digits_mod(int nl, GetD D, GetM QM, u64 q, u64 uhi, u64 ulo) {
    u64 acc = 0;
    for (int i = nl - 1; i >= 0; i--) acc = gio::garner_acc(acc, D(i), QM(i), q, uhi, ulo);
    return acc;
}
GR_HD u64 recode_new(u64 xmod, bool neg, u64 Qmod, u64 q) { return neg ? gr::submod(xmod, Qmod, q) : xmod; }

// ---- host side of the scale pair (no device use, but plain C++ all the same): Int(big.Float(f)) = m 2^e, m < 2^53, for a finite f >= 1; e = 0 below 2^53
inline bool scale_ok(double f) { return f >= 1.0 && f <= kMaxScale; }       // false for NaN
inline void scale_int(double f, u64 &m, int &e) {
    int ex = 0; double fr = f;
    while (fr >= 2.0) { fr *= 0.5; ex++; }                                   // f = fr 2^ex, 1 <= fr < 2, exact
    m = (u64)(fr * 0x1p52); e = ex - 52;                                      // fr 2^52 is an integer below 2^53
    if (e < 0) { m >>= -e; e = 0; }
}
inline Ratio scale_ratio(double ct_scale, double target_scale) {
    u64 mo, mi; int eo, ei; scale_int(target_scale, mo, eo); scale_int(ct_scale, mi, ei);
    Ratio r; r.mo = mo; r.mi = mi; r.sh = eo - ei; return r;
}
// The two fit checks.  A magnitude below 2^bits times mo < 2^53 is below 2^(bits + 53); shifted left by up = max(sh, 0) below 2^(bits + 53 + up); one bit of
// headroom as PN14 keeps it (54), and for Q_level two more (the recentred x and Q itself share the buffer): bits(Q_level) + 54 + up <= 64 kBigLimbs - 2.
// A mask of W limbs has a magnitude of at most 2^(64 W - 1) < 2^(64 W): 64 W + 54 + up <= 64 kBigLimbs.
inline bool fits_q(int q_bits, int sh) { return q_bits + 54 + (sh > 0 ? sh : 0) <= kBigBits - 2; }
inline bool fits_mask(int W, int sh) { return 64 * W + 54 + (sh > 0 ? sh : 0) <= kBigBits; }
// limbs the kernels run over: what the bound above occupies, so that small rings pay for small integers
inline int limbs_for(int bits, int sh) { return (bits + 54 + (sh > 0 ? sh : 0) + 63) / 64; }
}  // namespace grf
