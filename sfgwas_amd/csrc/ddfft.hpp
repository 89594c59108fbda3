// ddfft.hpp — double-double arithmetic, the encoder tables and the radix-8 FFT pass shared by the encoder (encode.hip) and the decoder (decrypt.hip).
#pragma once
#include "common.hpp"
#include <cmath>
#include <type_traits>

// ---------------------------------------------------------------- double-double (host + device)
struct dd { double hi, lo; };
__host__ __device__ static inline dd dd_make(double h, double l) { dd r; r.hi = h; r.lo = l; return r; }
__host__ __device__ static inline dd dd_quick(double a, double b) { double s = a + b; return dd_make(s, b - (s - a)); }
__host__ __device__ static inline dd dd_two_sum(double a, double b) { double s = a + b, bb = s - a; return dd_make(s, (a - (s - bb)) + (b - bb)); }
__host__ __device__ static inline dd dd_add(dd a, dd b) { dd s = dd_two_sum(a.hi, b.hi); s.lo += a.lo + b.lo; return dd_quick(s.hi, s.lo); }
__host__ __device__ static inline dd dd_neg(dd a) { return dd_make(-a.hi, -a.lo); }
// sum without the final renormalisation (8 flops instead of 11): the high parts are added exactly, the low part may grow to a
// few ulps of the high part.  Every consumer below (two_sum on the high parts, dd_mul / dd_dot2 cross terms) is exact or
// first-order correct for such pairs, so a chain of k lazy sums costs log2(k) of the ~106 bits; results are renormalised by the
// next product or by the recombination.
__host__ __device__ static inline dd dd_add_lazy(dd a, dd b) { dd s = dd_two_sum(a.hi, b.hi); s.lo += a.lo + b.lo; return s; }
__host__ __device__ static inline dd dd_sub_lazy(dd a, dd b) { dd s = dd_two_sum(a.hi, -b.hi); s.lo += a.lo - b.lo; return s; }
__host__ __device__ static inline dd dd_sub(dd a, dd b) { return dd_add(a, dd_neg(b)); }
__host__ __device__ static inline dd dd_mul(dd a, dd b) {
    double p = a.hi * b.hi, e = fma(a.hi, b.hi, -p);
    e = fma(a.hi, b.lo, e); e = fma(a.lo, b.hi, e);
    return dd_quick(p, e);
}
__host__ __device__ static inline dd dd_mul_d(dd a, double b) {
    double p = a.hi * b, e = fma(a.hi, b, -p);
    e = fma(a.lo, b, e);
    return dd_quick(p, e);
}
// accurate host-only add (table construction)
static inline dd dd_add_acc(dd a, dd b) {
    dd s = dd_two_sum(a.hi, b.hi), t = dd_two_sum(a.lo, b.lo);
    s.lo += t.hi; s = dd_quick(s.hi, s.lo); s.lo += t.lo; return dd_quick(s.hi, s.lo);
}
struct cdd { dd re, im; };
__host__ __device__ static inline cdd cdd_mul(cdd a, cdd b) {
    cdd r; r.re = dd_sub(dd_mul(a.re, b.re), dd_mul(a.im, b.im)); r.im = dd_add(dd_mul(a.re, b.im), dd_mul(a.im, b.re)); return r;
}

constexpr int ENC_H = SFG_SLOTS / 2;         // 4096-point complex FFT
constexpr int ENC_TW = 16384;                // zeta^-k is built for k = 0..16384, zeta = exp(2 pi i / 32768)
// device twiddle table (double4 entries): the three twiddled radix-8 passes, then the recombination lists
constexpr int ENC_TB_P512 = 0, ENC_TB_P64 = ENC_TB_P512 + 7 * 512, ENC_TB_P8 = ENC_TB_P64 + 7 * 64;
constexpr int ENC_TB_RLEN = ENC_H / 2 + 1;   // c = 0..h/2
constexpr int ENC_TB_RW = ENC_TB_P8 + 7 * 8, ENC_TB_RZ = ENC_TB_RW + ENC_TB_RLEN, ENC_TB_RZ2 = ENC_TB_RZ + ENC_TB_RLEN;
constexpr int ENC_TB_SIZE = ENC_TB_RZ2 + ENC_TB_RLEN;

struct EncTables {                // immutable, shared by a context and its forks
    double4 *tb = nullptr;        // twiddles {re.hi, re.lo, im.hi, im.lo} of zeta^-k = exp(-2 pi i k / 32768), laid out in the order the kernel's lanes read them (ENC_TB_*)
    uint16_t *tinv = nullptr;     // [n] slot index t with (5^t - 1)/4 mod n == m
    double2 *costab = nullptr;    // [8193] cos(2 pi k / 32768) as {hi, lo}: the exact re-derivation of a coefficient next to a rounding tie (k_fft_encode)
    int sexp = -1;                // log2(Delta / n) when that is a power of two (every preset), else -1: no re-derivation
    double4 *dec = nullptr;       // decoder (decrypt.hip): [0, h) zeta^c / 2, [h, 2h) omega^c = zeta^4c, c < h = n/2, as {re.hi, re.lo, im.hi, im.lo}
};

// cos/sin(theta) for small theta by Taylor series in double-double
static inline void dd_sincos_small(dd theta, dd &s, dd &c) {
    dd t2 = dd_mul(theta, theta);
    dd term = theta; s = theta;
    for (int k = 1; k < 14; k++) {            // sin: term *= -t2 / ((2k)(2k+1))
        term = dd_mul(term, t2); term = dd_mul_d(term, -1.0);
        double den = (double)(2 * k) * (double)(2 * k + 1);
        // divide by an exactly representable small integer: one Newton-free step via hi/lo correction
        dd q; q.hi = term.hi / den; double rem = fma(-q.hi, den, term.hi); q.lo = (rem + term.lo) / den; term = dd_quick(q.hi, q.lo);
        s = dd_add_acc(s, term);
    }
    term = dd_make(1.0, 0.0); c = term;
    for (int k = 1; k < 14; k++) {            // cos: term *= -t2 / ((2k-1)(2k))
        term = dd_mul(term, t2); term = dd_mul_d(term, -1.0);
        double den = (double)(2 * k - 1) * (double)(2 * k);
        dd q; q.hi = term.hi / den; double rem = fma(-q.hi, den, term.hi); q.lo = (rem + term.lo) / den; term = dd_quick(q.hi, q.lo);
        c = dd_add_acc(c, term);
    }
}

// Exchange images are indexed through an XOR swizzle instead of padding: address bits 0..4 (the 32 eight-byte bank pairs of a 256-byte bank
// sweep) are XORed with index bits 3..7.  Every access pattern of the kernel - 64 lanes that vary any six of the index bits 0..7 with the others
// fixed (contiguous, stride 4, stride 32, bit-reversed) - then maps onto all 32 bank pairs exactly twice, the minimum for 512 bytes.
__device__ __forceinline__ int padj(int j) { return j ^ ((j >> 3) & 31); }
// the last exchange (bit-reversed writers: 32 lanes vary index bits 4..8; readers take consecutive words) uses index bits 5..8 instead
__device__ __forceinline__ int padj_fin(int j) { return j ^ ((j >> 5) & 15); }

// (ar + i ai) * (wr + i wi) with each component as ONE double-double dot product (two products share the final
// renormalisation): 19 flops per component instead of 2 dd_mul + 1 dd_add = 25.
__device__ __forceinline__ dd dd_dot2(dd a, dd w, dd b, dd x, double sgn) {          // a*w + sgn*b*x, sgn = +-1
    const double p1 = a.hi * w.hi, e1 = fma(a.hi, w.hi, -p1);
    const double bh = sgn * b.hi, bl = sgn * b.lo;
    const double p2 = bh * x.hi, e2 = fma(bh, x.hi, -p2);
    dd s = dd_two_sum(p1, p2);
    double lo = e1 + e2;
    lo = fma(a.hi, w.lo, lo); lo = fma(a.lo, w.hi, lo);
    lo = fma(bh, x.lo, lo); lo = fma(bl, x.hi, lo);
    return dd_quick(s.hi, s.lo + lo);
}
// ---- fixed-grid double-double for the FFT of GENOTYPE rows.  Every intermediate of that transform is bounded by sum |z_m| <= 4096 * |128 + 128i| < 2^20
// for ANY int8 row (genotypes after missing -> 0 and squaring are <= 4: < 2^15), so the high parts can live on the fixed grid 2^-31 Z (|hi| < 2^20:
// 51 bits): two grid numbers add EXACTLY in one plain addition, the low parts (|lo| <= 2^-32 after a product, <= 2^-29 after the three add levels of
// a radix-8 pass) in another - 2 flops per sum instead of 8.  Only products leave the grid; they are put back by the magic-number split
// hi' = (p + M) - M, lo' = (p - hi') + e with M = 1.5 * 2^21 (4 flops, which replace the 3 of the renormalisation they had).  Absolute error: low-part
// sums 2^-83 each, products 2^-85: ~2^-80 after four passes, ~2^-59 on a scaled coefficient - far inside the 2^-40 band of the near-tie audit.
// Arbitrary real slot vectors (F64IN) are unbounded and keep the general path.
constexpr double GRID_M = 3145728.0;                      // 1.5 * 2^21: ulp(M) = 2^-31
__device__ __forceinline__ dd grid_split(double p, double e) { const double h = (p + GRID_M) - GRID_M; return dd_make(h, (p - h) + e); }
template <bool GRID> __device__ __forceinline__ dd fx_add(dd a, dd b) { return GRID ? dd_make(a.hi + b.hi, a.lo + b.lo) : dd_add_lazy(a, b); }
template <bool GRID> __device__ __forceinline__ dd fx_sub(dd a, dd b) { return GRID ? dd_make(a.hi - b.hi, a.lo - b.lo) : dd_sub_lazy(a, b); }
template <bool GRID> __device__ __forceinline__ dd fx_mul(dd a, dd b) {          // dd_mul, result on the grid
    double p = a.hi * b.hi, e = fma(a.hi, b.hi, -p);
    e = fma(a.hi, b.lo, e); e = fma(a.lo, b.hi, e);
    return GRID ? grid_split(p, e) : dd_quick(p, e);
}
template <bool GRID> __device__ __forceinline__ dd fx_dot2(dd a, dd w, dd b, dd x, double sgn) {   // dd_dot2, result on the grid
    const double p1 = a.hi * w.hi, e1 = fma(a.hi, w.hi, -p1);
    const double bh = sgn * b.hi, bl = sgn * b.lo;
    const double p2 = bh * x.hi, e2 = fma(bh, x.hi, -p2);
    if (GRID) {
        // each product is split on the grid by itself (the remainders p - h are exact, |.| <= 2^-32), the grid parts add exactly: no two_sum
        const double h1 = (p1 + GRID_M) - GRID_M, h2 = (p2 + GRID_M) - GRID_M;
        double lo = (p1 - h1) + (p2 - h2);
        lo += e1 + e2;
        lo = fma(a.hi, w.lo, lo); lo = fma(a.lo, w.hi, lo);
        lo = fma(bh, x.lo, lo); lo = fma(bl, x.hi, lo);
        return dd_make(h1 + h2, lo);
    }
    dd s = dd_two_sum(p1, p2);
    double lo = e1 + e2;
    lo = fma(a.hi, w.lo, lo); lo = fma(a.lo, w.hi, lo);
    lo = fma(bh, x.lo, lo); lo = fma(bl, x.hi, lo);
    return dd_quick(s.hi, s.lo + lo);
}
#ifndef SFG_ENC_DIAG
#define SFG_ENC_DIAG 0          // timing diagnostics only (wrong results): 1 no pass-twiddle loads, 2 no recombination arithmetic, 4 no exchanges, 8 no twiddle products, 16 no recombination-twiddle loads
#endif
__device__ __forceinline__ void tw_at(const double4 *tab, int idx, dd &wr, dd &wi) {
    if (SFG_ENC_DIAG & 1) { wr = dd_make(0.7 + idx * 1e-9, 1e-18); wi = dd_make(0.3 - idx * 1e-9, 2e-18); return; }
    const double4 w = tab[idx];
    wr = dd_make(w.x, w.y); wi = dd_make(w.z, w.w);
}
// One radix-8 DIF pass on 8 register-resident points at stride S of a sub-transform of length 8S: identical to three
// radix-2 DIF stages (pairs (i,i+4), (i,i+2), (i,i+1)) with the twiddles regrouped - the 12 twiddle products of the
// radix-2 form become 7 output products W^(e t), e = bitrev(r), plus two rotations by 1/8 turn; t = j mod S.
template <int S, bool GRID>
__device__ __forceinline__ void dif_radix8(dd (&xr)[8], dd (&xi)[8], const double4 *tab, int t) {          // tab: this pass's [7][S] twiddle list
    const dd rs = dd_make(7.071067811865475727e-01, -4.833646656726456726e-17);      // 1/sqrt(2) in double-double
    dd ur[4], ui[4], dr[4], di[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        ur[i] = fx_add<GRID>(xr[i], xr[i + 4]); ui[i] = fx_add<GRID>(xi[i], xi[i + 4]);
        dr[i] = fx_sub<GRID>(xr[i], xr[i + 4]); di[i] = fx_sub<GRID>(xi[i], xi[i + 4]);
    }
    {   // d1 *= W8 = (1 - i)/sqrt2: (a + bi) -> ((a + b) + (b - a) i)/sqrt2
        dd a = dr[1], b = di[1];
        dr[1] = fx_mul<GRID>(fx_add<GRID>(a, b), rs); di[1] = fx_mul<GRID>(fx_sub<GRID>(b, a), rs);
    }
    {   // d2 *= -i: (a + bi) -> (b - ai)
        dd a = dr[2]; dr[2] = di[2]; di[2] = dd_neg(a);
    }
    {   // d3 *= W8^3 = (-1 - i)/sqrt2: (a + bi) -> ((b - a) - (a + b) i)/sqrt2
        dd a = dr[3], b = di[3];
        dr[3] = fx_mul<GRID>(fx_sub<GRID>(b, a), rs); di[3] = dd_neg(fx_mul<GRID>(fx_add<GRID>(a, b), rs));
    }
    auto quad = [&](dd (&hr)[4], dd (&hi)[4], int o) {
        dd p0r = fx_add<GRID>(hr[0], hr[2]), p0i = fx_add<GRID>(hi[0], hi[2]);
        dd p1r = fx_add<GRID>(hr[1], hr[3]), p1i = fx_add<GRID>(hi[1], hi[3]);
        dd q0r = fx_sub<GRID>(hr[0], hr[2]), q0i = fx_sub<GRID>(hi[0], hi[2]);
        dd t1r = fx_sub<GRID>(hr[1], hr[3]), t1i = fx_sub<GRID>(hi[1], hi[3]);
        dd q1r = t1i, q1i = dd_neg(t1r);                                               // * -i
        xr[o + 0] = fx_add<GRID>(p0r, p1r); xi[o + 0] = fx_add<GRID>(p0i, p1i);
        xr[o + 1] = fx_sub<GRID>(p0r, p1r); xi[o + 1] = fx_sub<GRID>(p0i, p1i);
        xr[o + 2] = fx_add<GRID>(q0r, q1r); xi[o + 2] = fx_add<GRID>(q0i, q1i);
        xr[o + 3] = fx_sub<GRID>(q0r, q1r); xi[o + 3] = fx_sub<GRID>(q0i, q1i);
    };
    quad(ur, ui, 0);
    quad(dr, di, 4);
    if (S > 1) {                                                                       // S == 1: t = 0, every output twiddle is 1
#pragma unroll
        for (int r = 1; r < 8; r++) {                                                  // output r carries W_{8S}^(bitrev3(r) t)
            if (SFG_ENC_DIAG & 8) continue;
            dd wr, wi; tw_at(tab, (r - 1) * S + t, wr, wi);
            const dd pr = fx_dot2<GRID>(xr[r], wr, xi[r], wi, -1.0), pi = fx_dot2<GRID>(xr[r], wi, xi[r], wr, 1.0);
            xr[r] = pr; xi[r] = pi;
        }
    }
}
