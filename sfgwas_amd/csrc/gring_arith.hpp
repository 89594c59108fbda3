// gring_arith.hpp - per-element arithmetic of the general ring (gring.hip): canonical u64 residues, any modulus q < 2^61 with q == 1 mod 2N.
// Every function is __host__ __device__ and plain C++ (128-bit integers, no intrinsic), so tests/host/host_gring_test.cpp runs on the CPU the very
// functions the kernels run.  Each bound is written beside the code that needs it.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GR_HD __host__ __device__ __forceinline__
#else
#define GR_HD inline
#endif

namespace gr {
typedef unsigned long long u64;
typedef unsigned __int128 u128;

constexpr int kMaxMod = 48;                       // nq + np of one ring
constexpr u64 kMaxModulus = 1ULL << 61;           // lattigo's bound; 4q < 2^63 keeps every lazy word and every 2q-offset difference inside a u64

GR_HD u64 mulhi(u64 a, u64 b) { return (u64)(((u128)a * b) >> 64); }

// ---- Shoup (Harvey) product by a precomputed constant w < q with w' = floor(w 2^64 / q)
// r = a w - floor(a w' / 2^64) q computed mod 2^64.  With w 2^64 = w' q + e, 0 <= e < q:  a w - (a w' / 2^64) q = a e / 2^64 < q, and the floor drops less
// than one q more: 0 <= r < 2q for EVERY a < 2^64.  2q < 2^62, so the wrap-around arithmetic returns the true value.
GR_HD u64 shoup_lazy(u64 a, u64 w, u64 wsh, u64 q) { return a * w - mulhi(a, wsh) * q; }
// canonical: one conditional subtraction takes [0, 2q) to [0, q)
GR_HD u64 shoup(u64 a, u64 w, u64 wsh, u64 q) { u64 r = shoup_lazy(a, w, wsh, q); return r >= q ? r - q : r; }

// ---- Barrett reduction of a full 128-bit word x = hi 2^64 + lo by u = floor(2^128 / q) = uhi 2^64 + ulo (lattigo ring.BRedParams)
// qhat = floor(x u / 2^128) is computed exactly (nested floors of integers are exact): x / q - x u / 2^128 = x (2^128 / q - u) / 2^128 < 1, so
// qhat is floor(x / q) or one less and r = x - qhat q lies in [0, 2q), below 2^62: only the low 64 bits of qhat and of the difference are needed.
GR_HD u64 barrett128(u64 hi, u64 lo, u64 q, u64 uhi, u64 ulo) {
    u128 mid = (u128)hi * ulo + mulhi(lo, ulo);                 // < 2^128: (2^64 - 1)^2 + 2^64 - 1
    u128 m2 = (u128)lo * uhi;
    u64 carry = (u64)(((u128)(u64)mid + (u64)m2) >> 64);        // carry of the two low halves
    u64 qhat = hi * uhi + (u64)(mid >> 64) + (u64)(m2 >> 64) + carry;   // low 64 bits of floor(x u / 2^128)
    u64 r = lo - qhat * q;
    return r >= q ? r - q : r;                                  // the last conditional subtraction: [0, 2q) -> [0, q)
}
// product of two variable words a, b < 2^64 (a b < 2^128 always fits)
GR_HD u64 mulmod(u64 a, u64 b, u64 q, u64 uhi, u64 ulo) { u128 p = (u128)a * b; return barrett128((u64)(p >> 64), (u64)p, q, uhi, ulo); }

// ---- canonical helpers on [0, q)
GR_HD u64 addmod(u64 a, u64 b, u64 q) { u64 s = a + b; return s >= q ? s - q : s; }       // a + b < 2q < 2^62
GR_HD u64 submod(u64 a, u64 b, u64 q) { return a >= b ? a - b : a + q - b; }
// one canonical reduction of a lazy word in [0, 4q)
GR_HD u64 canon4(u64 x, u64 q) { u64 q2 = 2 * q; if (x >= q2) x -= q2; return x >= q ? x - q : x; }

// ---- lazy butterflies (Harvey): words stay in [0, 4q) forward and [0, 2q) inverse; 4q < 2^63
// forward Cooley-Tukey: X, Y in [0, 4q) -> X + wY, X - wY in [0, 4q).  X' = X - 2q if X >= 2q is in [0, 2q); T = shoup_lazy(Y) in [0, 2q):
// X' + T < 4q and X' - T + 2q in (0, 4q).
GR_HD void bfly_fwd(u64 &X, u64 &Y, u64 w, u64 wsh, u64 q) {
    const u64 q2 = 2 * q;
    u64 x = X >= q2 ? X - q2 : X;
    u64 t = shoup_lazy(Y, w, wsh, q);
    X = x + t; Y = x - t + q2;
}
// inverse Gentleman-Sande: X, Y in [0, 2q) -> X + Y, w (X - Y) in [0, 2q).  X + Y < 4q takes one subtraction of 2q; X - Y + 2q in (0, 4q) < 2^63 is
// a legal argument of shoup_lazy, whose result is in [0, 2q).
GR_HD void bfly_inv(u64 &X, u64 &Y, u64 w, u64 wsh, u64 q) {
    const u64 q2 = 2 * q;
    u64 s = X + Y, d = X - Y + q2;
    X = s >= q2 ? s - q2 : s;
    Y = shoup_lazy(d, w, wsh, q);
}

// ---- the float-corrected basis extension (lattigo FastBasisExtender.modUpExact)
// (double) of a word < 2^64, rounded to nearest even as the C conversion rounds: both halves convert exactly, the scaling by 2^32 is exact, and the one
// addition rounds once (a fused multiply-add would round the same exact sum, so contraction cannot change it).
GR_HD double to_double(u64 y) { return (double)(uint32_t)(y >> 32) * 4294967296.0 + (double)(uint32_t)y; }
// one term of the correction: vf += (double)y / (double)q with the IEEE division, nothing fused into the sum
GR_HD double ext_accumulate(double vf, u64 y, u64 q) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    double d = to_double(y) / to_double(q);
    return vf + d;
}
// v = uint64(vf): truncation, not rounding
GR_HD u64 ext_truncate(double vf) { return (u64)vf; }
// the extension's residue at a target from the 128-bit sum S = sum_m y_m (D / q_m mod qt) (alpha <= 47 terms below 2^122: S < 2^128) and v:
// S mod qt - (v D mod qt); v <= alpha and D mod qt < 2^61, so v D < 2^67 goes through the same 128-bit reduction.
GR_HD u64 ext_finish(u128 S, u64 v, u64 D_t, u64 qt, u64 uhi, u64 ulo) {
    u64 acc = barrett128((u64)(S >> 64), (u64)S, qt, uhi, ulo);
    u64 sub = mulmod(v, D_t, qt, uhi, ulo);
    return submod(acc, sub, qt);
}
}  // namespace gr
