// gring_io_arith.hpp - per-element arithmetic of the general ring's two ends (gring_io.hip): the lift of a signed sample to a residue, the sampler's map from a
// coefficient index to its place in the keyed stream at any N = 2^12 .. 2^16, the decoder's way from residues to one double (or one pair) per coefficient, the
// double-double butterfly of the transform between slots and coefficients, and the encoder's rounding with its band - each bound derived beside its code.  Every
// function is __host__ __device__ and plain C++ (like gring_arith.hpp), so tests/host/host_gring_io_test.cpp runs on the CPU the very functions the kernels run.
#pragma once
#include <cstdint>
#include "gring_arith.hpp"

namespace gio {
using gr::u64;

// ---- a signed small integer (a ternary or Gaussian sample, or a caller's error coefficient) as a canonical residue modulo q, 3 <= q < 2^61
// |v| <= 2^31 < 2^61, but q may be smaller than |v| (q >= 2N + 1 only): the magnitude is reduced first.  v = -2^31 is negated in 64 bits.
GR_HD u64 lift(int32_t v, u64 q) {
    const long long w = v;
    const u64 m = (u64)(w < 0 ? -w : w) % q;
    return (w < 0 && m) ? q - m : m;
}

// ---- the sampler's map (section 9 states it for N = 16384).  Coefficient j = 512 a + t, t < 512, a < N / 512.
// ChaCha20 block, nonce layout (64-bit encryption index, polynomial id 0 = u, 1 = e0, 2 = e1) and the Gaussian table are sampler.hpp's, unchanged.
//   u_j: block (t >> 3) + 64 (a >> 5) of polynomial 0; r = w[2 (t & 7)] | w[2 (t & 7) + 1] << 32; bits 2 (a & 31), 2 (a & 31) + 1 = (b0, b1): b0 ? (b1 ? -1 : +1) : 0
//   e_j: block t + 512 (a >> 3) of polynomial 1 / 2; r = w[2 (a & 7)] | w[2 (a & 7) + 1] << 32 -> gauss_from_bits
// At N = 16384 (a < 32) this is sampler.hpp's enc_sample_thread word for word.  Block counters stay below 2^32: at N = 65536, a < 128, u uses blocks 0..255 and e blocks 0..8191.
constexpr int kSampT = 512;                                   // coefficients that share one value of a
GR_HD int samp_t(int j) { return j & (kSampT - 1); }
GR_HD int samp_a(int j) { return j >> 9; }
GR_HD unsigned samp_u_block(int t, int a) { return (unsigned)((t >> 3) + 64 * (a >> 5)); }
GR_HD int samp_u_word(int t) { return 2 * (t & 7); }
GR_HD int samp_u_shift(int a) { return 2 * (a & 31); }
GR_HD int samp_ternary(u64 r, int shift) { const unsigned two = (unsigned)(r >> shift) & 3u; return (two & 1u) ? ((two & 2u) ? -1 : 1) : 0; }
GR_HD unsigned samp_e_block(int t, int a) { return (unsigned)(t + kSampT * (a >> 3)); }
GR_HD int samp_e_word(int a) { return 2 * (a & 7); }
// how many blocks of the stream one polynomial of N coefficients reads
GR_HD unsigned samp_u_blocks(int N) { return 64u * (unsigned)((N / kSampT + 31) / 32); }
GR_HD unsigned samp_e_blocks(int N) { return (unsigned)kSampT * (unsigned)(N / kSampT / 8); }

// ---- the decoder's coefficients: residues -> mixed-radix digits -> the centred integer's sign and magnitude -> a double-double -> / scale -> one double
// Mixed radix (Garner): X = sum_i d_i W_i, W_i = q_0 .. q_(i-1), 0 <= d_i < q_i.  Digit i from the residue x_i and the lower digits:
//   acc = (d_0 + d_1 q_0 + .. + d_(i-1) W_(i-1)) mod q_i by Horner from d_(i-1) down (garner_acc with q_j mod q_i), then d_i = (x_i - acc) W_i^-1 mod q_i.
// acc < q_i < 2^61, (q_j mod q_i) < 2^61, d_j < 2^61: acc (q_j mod q_i) + d_j < 2^122 + 2^61 fits 128 bits.
GR_HD u64 garner_acc(u64 acc, u64 d_j, u64 qj_mod_qi, u64 q_i, u64 uhi, u64 ulo) {
    const gr::u128 s = (gr::u128)acc * qj_mod_qi + d_j;
    return gr::barrett128((u64)(s >> 64), (u64)s, q_i, uhi, ulo);
}
GR_HD u64 garner_digit(u64 x_i, u64 acc, u64 winv, u64 winv_sh, u64 q_i) { return gr::shoup(gr::submod(x_i, acc, q_i), winv, winv_sh, q_i); }
// lattigo's rule: x.Cmp(QHalf) > 0 -> x - Q, QHalf = floor(Q / 2) (Q is odd): the comparison walks the digits from the top; state 0 = equal so far, +1 / -1 decided
GR_HD int cmp_step(int state, u64 d, u64 h) { return state ? state : (d > h ? 1 : (d < h ? -1 : 0)); }
// the magnitude Q - X digit by digit, from digit 0 up: Q = sum (q_i - 1) W_i + 1, so Q - X = sum (q_i - 1 - d_i) W_i + 1: the complement, plus one with the carry
// walked up (a digit that reaches q_i becomes 0 and carries).  carry starts at 1.  X > Q / 2 > 0 keeps the carry from leaving the top digit.
GR_HD u64 neg_digit(u64 d, u64 q, unsigned &carry) {
    u64 m = (q - 1 - d) + carry;
    if (m == q) { m = 0; carry = 1; } else carry = 0;
    return m;
}

// double-double, non-negative operands only in the decoder's Horner (no cancellation).  u = 2^-53.
struct dd { double hi, lo; };
GR_HD dd dd_quick(double a, double b) { const double s = a + b; dd r; r.hi = s; r.lo = b - (s - a); return r; }                  // exact for |b| <= |a|
GR_HD dd dd_two_sum(double a, double b) { const double s = a + b, bb = s - a; dd r; r.hi = s; r.lo = (a - (s - bb)) + (b - bb); return r; }   // exact
// a word below 2^61 as an exact pair: hi = the nearest double (a multiple of 2^8 at most 2^61), lo = x - hi, |lo| <= 2^7, an integer
GR_HD dd dd_from_u64(u64 x) { dd r; r.hi = gr::to_double(x); r.lo = (double)((long long)x - (long long)r.hi); return r; }
// product: p + e with e = the exact error of hi hi, plus the two cross terms; lo lo (<= u^2 |a b|) is dropped, the two fused sums round once each at <= u |e| <= 3 u^2 |a b|:
// relative error <= 7 u^2 < 2^-103
GR_HD dd dd_mul(dd a, dd b) {
    const double p = a.hi * b.hi; double e = __builtin_fma(a.hi, b.hi, -p);
    e = __builtin_fma(a.hi, b.lo, e); e = __builtin_fma(a.lo, b.hi, e);
    return dd_quick(p, e);
}
// sum of two non-negative pairs: the high parts add exactly; lo = s.lo + (a.lo + b.lo) rounds twice, each below 2 u^2 (a + b): relative error <= 4 u^2 = 2^-104
GR_HD dd dd_add(dd a, dd b) { dd s = dd_two_sum(a.hi, b.hi); s.lo += a.lo + b.lo; return dd_quick(s.hi, s.lo); }
// pair / double: q1 = fl(a.hi / s); the remainder a - q1 s is formed exactly in its leading part (q1 s = p + e exactly; a.hi - p is exact, the two are within
// two ulps), q2 = fl(rem / s): |q2| <= 2 u |q1|, so its own rounding and the remainder's are below 8 u^2 |q|: relative error <= 2^-103
GR_HD dd dd_div_d(dd a, double s) {
    const double q1 = a.hi / s, p = q1 * s, e = __builtin_fma(q1, s, -p);
    const double rem = ((a.hi - p) - e) + a.lo;
    return dd_quick(q1, rem / s);
}
// One Horner step v <- v q + d on non-negative operands: <= 2^-103 + 2^-104 (+ second order) < 1.6 * 2^-103 relative.  The first step is exact (dd_from_u64), so the
// magnitude of up to 48 digits carries at most 47 * 1.6 * 2^-103 < 2^-96.7, the division 2^-103 more: the pair handed to the final rounding is within
//   kDecodeRel = 2^-96
// relative of the exact quotient.  Its high part IS the pair rounded to nearest (dd_quick), so the double returned is the correctly rounded quotient unless the exact
// quotient lies within 2^-96 relative of a rounding boundary (the midpoint of two adjacent doubles).  (Section 10's 2^-100 is this bound at ten digits.)
// Range: the walk stops and returns infinity once the running value exceeds 2^960 (a further step stays below 2^1022: no NaN is ever formed).
constexpr double kDecodeRel = 0x1p-96;
constexpr double kDecodeHuge = 0x1p960;
GR_HD dd horner_step(dd v, dd q, dd d) { return dd_add(dd_mul(v, q), d); }
// One coefficient from its nl mixed-radix digits: sign by the comparison with floor(Q / 2), the magnitude's digits written back in place of a negative value's,
// Horner from the top digit, the division, the sign.  D(i) reads digit i, S(i, v) stores it, Q(i) is modulus i, H(i) digit i of floor(Q / 2): the kernel hands
// accessors of rows in device memory (no per-thread digit array), the host test accessors of a vector.
template <class GetD, class SetD, class GetQ, class GetH>
GR_HD double decode_digits(int nl, GetD D, SetD S, GetQ Q, GetH H, double scale) {
    int st = 0;
    for (int i = nl - 1; i >= 0; i--) st = cmp_step(st, D(i), H(i));
    const bool neg = st > 0;
    if (neg) { unsigned carry = 1; for (int i = 0; i < nl; i++) S(i, neg_digit(D(i), Q(i), carry)); }
    dd v = dd_from_u64(D(nl - 1));
    for (int i = nl - 2; i >= 0; i--) {
        if (v.hi > kDecodeHuge) return neg ? -__builtin_inf() : __builtin_inf();
        v = horner_step(v, dd_from_u64(Q(i)), dd_from_u64(D(i)));
    }
    const dd r = dd_div_d(v, scale);
    return neg ? -r.hi : r.hi;
}
// the same walk, the signed quotient handed out as a pair (the decoder's embedding rounds once, at its end); beyond 2^960: an infinity in hi
template <class GetD, class SetD, class GetQ, class GetH>
GR_HD dd decode_digits_dd(int nl, GetD D, SetD S, GetQ Q, GetH H, double scale) {
    int st = 0;
    for (int i = nl - 1; i >= 0; i--) st = cmp_step(st, D(i), H(i));
    const bool neg = st > 0;
    if (neg) { unsigned carry = 1; for (int i = 0; i < nl; i++) S(i, neg_digit(D(i), Q(i), carry)); }
    dd v = dd_from_u64(D(nl - 1));
    for (int i = nl - 2; i >= 0; i--) {
        if (v.hi > kDecodeHuge) { dd r; r.hi = neg ? -__builtin_inf() : __builtin_inf(); r.lo = 0.0; return r; }
        v = horner_step(v, dd_from_u64(Q(i)), dd_from_u64(D(i)));
    }
    dd r = dd_div_d(v, scale);
    if (neg) { r.hi = -r.hi; r.lo = -r.lo; }
    return r;
}

// ---- the double-double transform between slots and coefficients (gring_io.hip: k_gdd_cols, k_gdd_contig) and the encoder's rounding
GR_HD dd dd_neg(dd a) { dd r; r.hi = -a.hi; r.lo = -a.lo; return r; }
GR_HD dd dd_sub(dd a, dd b) { return dd_add(a, dd_neg(b)); }           // dd_add's algorithm is sign-agnostic: its error is <= 2^-104 (|a| + |b|)
GR_HD dd dd_mul_d(dd a, double b) { const double p = a.hi * b; double e = __builtin_fma(a.hi, b, -p); e = __builtin_fma(a.lo, b, e); return dd_quick(p, e); }   // <= 2^-104
struct cdd { dd re, im; };
GR_HD cdd cdd_add(cdd a, cdd b) { cdd r; r.re = dd_add(a.re, b.re); r.im = dd_add(a.im, b.im); return r; }
GR_HD cdd cdd_sub(cdd a, cdd b) { cdd r; r.re = dd_sub(a.re, b.re); r.im = dd_sub(a.im, b.im); return r; }
GR_HD cdd cdd_mul(cdd a, cdd b) { cdd r; r.re = dd_sub(dd_mul(a.re, b.re), dd_mul(a.im, b.im)); r.im = dd_add(dd_mul(a.re, b.im), dd_mul(a.im, b.re)); return r; }
GR_HD cdd cdd_conj(cdd a) { a.im = dd_neg(a.im); return a; }
// decimation-in-frequency butterfly of the forward DFT (kernel exp(-2 pi i m c / n)): (x, y) -> (x + y, (x - y) w)
GR_HD void bfly_dif(cdd &x, cdd &y, cdd w) { const cdd s = cdd_add(x, y), d = cdd_sub(x, y); x = s; y = cdd_mul(d, w); }
// Error of the transform, the band B_enc and the slot bound B (DESIGN.md section 14 repeats this).  u2 = 2^-104.
//   * A component sum or difference errs by <= u2 (|a| + |b|); a complex product by a twiddle |w| <= 1 errs, per component, by <= 2 * 2^-103 + u2 on products whose
//     magnitudes sum to <= sqrt(2) |d|: below 2^-101 |d|.  The twiddle itself (host table: Taylor series of 14 terms on an octant-reduced angle pi r, r exact) is within
//     2^-100 of exp(-i pi r).  One butterfly therefore errs by less than eps = 2^-99 times (|x| + |y|).
//   * Every value of stage s that feeds one output depends on a set of inputs, the sets of one stage partition the inputs, and |value| <= the sum of |inputs| of its
//     set (twiddles have modulus 1).  An error made at a stage reaches the output with modulus <= 1.  So one output errs by at most eps S1 per stage, S1 = sum |input|,
//     and by L eps S1 after the L = log2 n <= 15 stages: < 2^-95 S1.  The twist by zeta^-c (one more product, same table accuracy) and the scaling by the double
//     scale / n add 2^-99 each.  In units of a coefficient p, with S = scale S1 / n >= every |scale w_c|:   |error| <= 2^-94 S.
//   * S in terms of the output: v_t = sum_c w_c zeta^(5^t c) gives sum_t |v_t| <= n sum_c |w_c|, and |scale Re w_c| <= |p_c| + 1/2, so S <= Sp + N / 2 with
//     Sp = sum over all N coefficients of |p_c|.
//   B_enc(Sp, n) = max(2^-50, 2^-93 (Sp + n)): twice the bound; the floor covers the 2^-53 the band test itself can lose when it forms the distance.
// The library applies the band with S computed on the host from the input (S <= Sp + n, so its band is never wider than B_enc(Sp, n)): a coefficient whose value lies
// within the band of a rounding tie k + 1/2 is unproven and the call fails; every other coefficient is the exactly rounded integer.
//   Decoder: inputs a_c = conj(w_c) zeta^-c carry 2^-96 (decode_digits) + 2^-99 relative; the transform adds 2^-95 sum_c |a_c|; by Parseval sum_c |w_c| <=
//   sqrt(n) |w|_2 = |v|_2 <= sqrt(n) max_t |v_t| with sqrt(n) <= 2^7.5: absolute error <= 2^-94 * 2^7.5 max|v| < 2^-86 max|v|, and the one rounding to double adds
//   2^-53 |v_t|:   |d_t - v_t| <= B max_t |v_t|,  B = 2^-53 + 2^-86.
constexpr double kEncBandFloor = 0x1p-50, kEncBandRel = 0x1p-93, kDomain = 0x1p62;
GR_HD double enc_band(double S) { const double b = kEncBandRel * S; return b > kEncBandFloor ? b : kEncBandFloor; }
// round half away from zero of the pair x, |x| < 2^62 required for a result: 0 = proven (p set), 1 = within `band` of a tie (p set to the nearest anyway), 2 = outside
// the domain (not finite or |x| >= 2^62).  
GR_HD int round_half_away(dd x, double band, long long &p) {
    p = 0;
    if (!(x.hi <= kDomain && x.hi >= -kDomain)) return 2;                // NaN fails both comparisons; hi = 2^62 with lo < 0 is still inside (2^62 - 1 rounds there)
    const bool neg = x.hi < 0.0 || (x.hi == 0.0 && x.lo < 0.0);
    const double hi = neg ? -x.hi : x.hi, lo = neg ? -x.lo : x.lo;
    // |x| = m + 1/2 + d with an integer m and d in [-1/2, 1/2): d is the signed distance from the tie.  hi - floor(hi) and that minus 1/2 are exact; lo keeps its
    // integer part only when it has one (above 2^53 hi is an integer and lo may be as large as 2^8), so that a tiny lo enters d unrounded: next to a tie
    // (hi's fraction exactly 1/2) d IS lo's fraction, exactly; elsewhere the one sum rounds by at most 2^-53 |d|.
    const double fh = __builtin_floor(hi), il = (lo < 0.5 && lo > -0.5) ? 0.0 : __builtin_floor(lo);
    double d = ((hi - fh) - 0.5) + (lo - il);                             // in (-1, 3/2)
    long long m = (long long)fh + (long long)il;
    if (d >= 0.5) { d -= 1.0; m += 1; } else if (d < -0.5) { d += 1.0; m -= 1; }
    m += d >= 0.0 ? 1 : 0;                                                // a tie (d == 0) goes away from zero
    if (m >= (1LL << 62)) return 2;
    p = neg ? -m : m;
    return (d < 0.0 ? -d : d) <= band ? 1 : 0;
}
// a signed integer |p| < 2^62 modulo q < 2^61, canonical: the magnitude through the 128-bit Barrett step, then the sign
GR_HD u64 reduce_i62(long long p, u64 q, u64 uhi, u64 ulo) {
    const u64 m = gr::barrett128(0, (u64)(p < 0 ? -p : p), q, uhi, ulo);
    return (p < 0 && m) ? q - m : m;
}
constexpr double kSlotBound = 0x1p-53 + 0x1p-86;                         // B
}  // namespace gio
