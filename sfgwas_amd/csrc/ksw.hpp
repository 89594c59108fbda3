// ksw.hpp — constants and device helpers of the hybrid key switch's basis extensions (rotate.hip), shared with the public-key
// encryption (encrypt.hip), whose ModDown is the key switch's.
#pragma once
#include "common.hpp"

constexpr int KSW_MAXA = 4;       // max primes per digit (= max np)
constexpr int KSW_MAXDIG = 8;

struct ExtConst {
    int a;                                        // source moduli in this digit at this level
    int src[KSW_MAXA];                            // their global modulus indices
    double qhat_inv[KSW_MAXA], qhat_inv_q[KSW_MAXA];          // (D/q_m)^-1 mod q_m, and that / q_m
    double qhat_t[SFG_MAXMOD][KSW_MAXA], qhat_t_q[SFG_MAXMOD][KSW_MAXA];   // (D/q_m) mod q_t, / q_t  (t = global modulus index)
    double D_t[SFG_MAXMOD], D_t_q[SFG_MAXMOD];    // D mod q_t, / q_t
};
struct KswConst {
    int level, nl, np, nt, beta, alpha;
    int tmod[SFG_MAXMOD];                         // target slot -> global modulus index (Q_0..level then P)
    int digit_of[SFG_MAXMOD];                     // target slot -> digit that contains it (or -1 for P targets)
    ExtConst dig[KSW_MAXDIG];
    ExtConst pq;                                  // special primes -> Q (ModDown)
    double pinv[SFG_MAXMOD], pinv_q[SFG_MAXMOD];  // P^-1 mod q_t by global modulus index
};
// per-level constants, built once: the host copy and its device copy, owned by the context (sfg_ctx::ksw_cache, freed in ctx.hip); rotate.hip
struct KswLevel { KswConst host; KswConst *dev = nullptr; };
int get_ksw(sfg_ctx *ctx, int level, const KswConst **dev, const KswConst **host);

#ifdef __HIPCC__
// general modular product of two canonical residues held in fp64 (both variable): result in (-q, q)
__device__ __forceinline__ double mulmod2(double a, double b, double q, double qinv) {
    double h = a * b;
    double l = __builtin_fma(a, b, -h);
    double qh = __builtin_rint(h * qinv);
    double r = __builtin_fma(-qh, q, h);
    return r + l;
}

// y_m, v and the extension to one target modulus (lattigo reconstructRNS + multSum restated)
__device__ __forceinline__ void ext_prepare(const ExtConst &e, const ModConst *modc, const double (&x)[KSW_MAXA], double (&y)[KSW_MAXA], double &v) {
    double vf = 0.0;
#pragma unroll
    for (int m = 0; m < KSW_MAXA; m++) {
        if (m < e.a) {
            const ModConst mc = modc[e.src[m]];
            y[m] = canon(mulmod_lazy(x[m], e.qhat_inv[m], e.qhat_inv_q[m], mc.q), mc.q, mc.qinv);
            vf += y[m] / mc.q;                                  // IEEE division, accumulated in modulus order
        }
    }
    v = (double)(u64)vf;
}
__device__ __forceinline__ double ext_target(const ExtConst &e, int tg, double qt, double qtinv, const double (&y)[KSW_MAXA], double v) {
    double acc = -mulmod_lazy(v, e.D_t[tg], e.D_t_q[tg], qt);
#pragma unroll
    for (int m = 0; m < KSW_MAXA; m++) if (m < e.a) acc += mulmod_lazy(y[m], e.qhat_t[tg][m], e.qhat_t_q[tg][m], qt);
    return canon(acc, qt, qtinv);
}
#endif
