// recode.hpp — what the collective bootstrap (refresh.hip) and the collective decryption / decoder (decrypt.hip) share: the per-level CRT constants, the Garner
// mixed-radix digits with lattigo's Cmp(QHalf) centring rule, and the share word sk (.) c1 + row.
#pragma once
#include "common.hpp"

constexpr int RF_MAXL = 12;       // moduli of the input level
struct RecodeConst {
    int nl, nq;
    double inv[RF_MAXL][RF_MAXL];         // inv[i][t] = q_t^-1 mod q_i, t < i
    double half[RF_MAXL];                 // mixed-radix digits of floor(Q_level / 2)
    double qm[SFG_MAXMOD][RF_MAXL];       // q_i mod q_j for the new moduli j >= nl
    double Qmod[SFG_MAXMOD];              // Q_level mod q_j
};
void recode_constants(const sfg_ctx *ctx, int level, RecodeConst &rc);      // refresh.hip

#ifdef __HIPCC__
// Garner: x = v0 + v1 q0 + v2 q0 q1 + ..., 0 <= v_i < q_i, from the residues r_i = x mod q_i
__device__ __forceinline__ void garner_digits(const double (&r)[RF_MAXL], double (&v)[RF_MAXL], int nl, const RecodeConst &rc, const ModConst *modc) {
    for (int i = 0; i < nl; i++) {
        const double q = modc[i].q, qinv = modc[i].qinv;
        double t = r[i];
        for (int s = 0; s < i; s++) {
            const double d = t - canon(v[s], q, qinv);                         // (-q, q)
            t = canon(mulmod_lazy(d, rc.inv[i][s], rc.inv[i][s] * qinv, q), q, qinv);
        }
        v[i] = t;
    }
}
// x >= floor(Q/2)  (lattigo: Cmp(QHalf) is 1 or 0)  ->  the represented value is x - Q
__device__ __forceinline__ bool garner_negative(const double (&v)[RF_MAXL], int nl, const RecodeConst &rc) {
    bool neg = true;                                                           // all digits equal: x == QHalf counts as negative
    for (int i = nl - 1; i >= 0; i--) if (v[i] != rc.half[i]) { neg = v[i] > rc.half[i]; break; }
    return neg;
}
// sk (.) c1 + row (mod q), canonical: s, v, row canonical residues
__device__ __forceinline__ double share_word(double s, double v, double row, double q, double qinv) {
    const double hh = s * v, ll = __builtin_fma(s, v, -hh);
    double r = canon(__builtin_fma(-__builtin_rint(hh * qinv), q, hh) + ll, q, qinv) + row;
    return r >= q ? r - q : r;
}
#endif
