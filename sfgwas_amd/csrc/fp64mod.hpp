// fp64mod.hpp — the ring arithmetic on exact integers held in fp64 (|x| < 2^53) that every kernel of the PN14 path runs, and the helper of the key
// switch's split forward transform built from it.  Plain C++ and __host__ __device__ (like gring_arith.hpp), so tests/host/host_ksw_split_test.cpp runs on the CPU
// the very functions the kernels run.  Compile with -ffp-contract=off (csrc/Makefile does): every product below is meant to round once, every fma is explicit.
// measured on gfx950 v_fma_f64 and v_mad_u64_u32 issue at the same rate (profiles/r01_ubench_*.txt), and the fp64 form needs no carry chains.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SFG_HD __host__ __device__ __forceinline__
#else
#define SFG_HD inline
#endif

// x*w mod q, result in (-q, q) (not canonical). Requires |x|*w < 2^105, |x| < 2^51, wq = w/q (rounded).
SFG_HD double mulmod_lazy(double x, double w, double wq, double q) {
    double qh = __builtin_rint(x * wq);
    double h = x * w;
    double l = __builtin_fma(x, w, -h);
    double r = __builtin_fma(-qh, q, h);
    return r + l;
}
// The same product with the quotient estimated from the rounded high part: needs only 1/q, not w/q, so butterflies that take a fresh twiddle
// spend no multiply on w * (1/q).  |x * w / q| < 2^41 keeps the estimate within 1/2 + 2^-11 of the true quotient: result in (-q, q).
SFG_HD double mulmod_lazy_q(double x, double w, double q, double qinv) {
    double h = x * w;
    double qh = __builtin_rint(h * qinv);
    double l = __builtin_fma(x, w, -h);
    double r = __builtin_fma(-qh, q, h);
    return r + l;
}
// canonical representative in [0, q) of an integer-valued double |x| < 2^51.
// y = fl(x * fl(1/q)) is within |x/q| * 2^-52 (1 + 2^-53) of x/q.  Write x = k q + e, 0 <= e < q: for e >= 1 both e/q and (q - e)/q exceed
// that error (e >= 1 > |x| 2^-51), so floor(y) = k; for e = 0, y = k (1 + d) may fall just below k, floor(y) = k - 1 and the exact
// remainder fma(-floor(y), q, x) is q.  One equality test is therefore the whole fix-up.
SFG_HD double canon(double x, double q, double qinv) {
    const double r = __builtin_fma(-__builtin_floor(x * qinv), q, x);
    return r == q ? 0.0 : r;
}
// the same without the fix-up: a representative in [0, q] (q itself only for multiples of q).  Enough wherever the value is an operand of further
// lazy arithmetic and merely has to be congruent, non-negative and <= q - e.g. the packed-limb plaintext words the MAC reads (q < 2^36 fits the limbs).
SFG_HD double canon_le(double x, double q, double qinv) {
    return __builtin_fma(-__builtin_floor(x * qinv), q, x);
}
// partial reduction to (-q, q): cheap, for lazy sums that would otherwise grow
SFG_HD double pred(double x, double q, double qinv) {
    double qh = __builtin_rint(x * qinv);
    return __builtin_fma(-qh, q, x);
}

// ---- the key switch's split forward transform (ntt.hip k_ntt_fwd_split): two half-row workgroups per row, half h owns positions [h N/2, (h + 1) N/2)
// Stage 1 of the forward transform done by the WRITER of a coefficient-domain row: the canonical pair (v0, v1) at positions x and x + N/2 becomes
// r_x = v0 + W v1 and r_(x + N/2) = v0 - W v1 (W = psi^(N/2), entry 1 of the modulus' forward table; Wq = W / q rounded), both canonical.  The split
// transform then loads only its own half of the row and starts at stage 2: the same residues, hence the same canonical output.  |v0 +- p| < 2q.
SFG_HD void fwd_stage1_pair(double v0, double v1, double W, double Wq, double q, double qinv, double &r0, double &r1) {
    const double p = mulmod_lazy(v1, W, Wq, q);
    r0 = canon(v0 + p, q, qinv); r1 = canon(v0 - p, q, qinv);
}
// ---- the key switch's split inverse transform (ntt.hip k_ntt_inv_split): each half-row workgroup runs the 13 Gentleman-Sande stages that stay inside its half
// and writes canonical words, without the 1/N factor.  The LAST stage and the scaling are done by the READER of the row: from the canonical pair (U, V) at
// positions x and x + N/2 it forms c_x = (U + V) N^-1 and c_(x + N/2) = (U - V) w N^-1, both canonical (w = psi^-(N/2), entry 1 of the modulus' inverse table;
// ninv = N^-1, wn = w N^-1 mod q, ninv_q and wn_q those over q, rounded): the words the one-workgroup transform stores.  |U +- V| < 2q.
SFG_HD void inv_last_pair(double U, double V, double ninv, double ninv_q, double wn, double wn_q, double q, double qinv, double &r0, double &r1) {
    r0 = canon(mulmod_lazy(U + V, ninv, ninv_q, q), q, qinv); r1 = canon(mulmod_lazy(U - V, wn, wn_q, q), q, qinv);
}
