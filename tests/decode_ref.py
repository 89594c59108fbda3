"""Exact reference for the decoder (sfgwas_amd/csrc/decrypt.hip), independent of the kernels and of the C oracle.

decode(p, N, scale) computes, for every slot t in [0, n) (n = N/2, zeta = exp(2 pi i / 2N)),
    v_t = sum_c w_c zeta^(5^t c),   w_c = (p_c + i p_{c+n}) / scale
from the integer coefficients p and a scale given as an exact rational.  With 5^t = 4 m + 1 (mod 2N) the sum is the length-n DFT with kernel exp(+2 pi i m c / n) of
a_c = w_c zeta^c, taken here as the conjugate of the exp(-...) transform of conj(a): the radix-2 integer FFT and the mpmath twiddles (rounded to 2^-240) of
tests/exactref.py.  The inputs are exact integers shifted left by _GUARD bits; every butterfly truncates once at 2^-(240 + _GUARD) of a unit of p, so after
log2(n) stages and the twist the absolute error of a value is below 2^(log2(n) + 3 - 240 - _GUARD) max |p| / scale... in fact far below: see `err`.  Relative to
max_t |v_t| >= sqrt(sum |w_c|^2) that is more than 150 bits for every input whose largest coefficient is below 2^(_GUARD + 60) times its 2-norm.
"""
from fractions import Fraction

import numpy as np

import exactref

_GUARD = 100


def decode(p, N, scale):
    """-> (re, im, err): two lists of n Fractions (slot order) and a bound on the absolute error of each, as a Fraction."""
    n = N // 2
    scale = Fraction(scale)
    assert len(p) == N and scale > 0
    slot, perm, wr, wi, zr, zi = exactref._tables(N)
    T = exactref._TW_BITS
    pr = np.array([int(x) << _GUARD for x in p[:n]], dtype=object)
    pi = np.array([-(int(x) << _GUARD) for x in p[n:]], dtype=object)          # conj(w)
    # conj(a_c) = conj(w_c) zeta^-c, scaled by 2^T (exact products, no truncation)
    xr, xi = pr * zr - pi * zi, pr * zi + pi * zr
    xr, xi = xr[perm].copy(), xi[perm].copy()
    half = 1
    while half < n:
        step = n // (2 * half)
        tr, ti = wr[::step][:half], wi[::step][:half]
        ar, ai = xr.reshape(-1, 2, half), xi.reshape(-1, 2, half)
        br, bi = ar[:, 1, :], ai[:, 1, :]
        qr = (br * tr - bi * ti) >> T
        qi = (br * ti + bi * tr) >> T
        lr, li = ar[:, 0, :], ai[:, 0, :]
        xr = np.concatenate([lr + qr, lr - qr], axis=1).reshape(-1)
        xi = np.concatenate([li + qi, li - qi], axis=1).reshape(-1)
        half *= 2
    den = (1 << (T + _GUARD)) * scale.numerator
    mul = scale.denominator
    re, im = [None] * n, [None] * n
    for m in range(n):
        t = int(slot[m])
        re[t] = Fraction(int(xr[m]) * mul, den)
        im[t] = Fraction(-int(xi[m]) * mul, den)                                # V_m = conj(X_m)
    # units of 2^-(T + _GUARD) p: twiddles off by 1/2 unit of 2^-T relative (|x| <= sum |p| 2^(T + _GUARD) -> n max|p| 2^_GUARD per stage and point feeding an output),
    # one truncation per butterfly.  Bounded by (log2(n) + 1) * (n max|p| 2^_GUARD + n) units.
    pmax = max(1, max(abs(int(x)) for x in p))
    logn = n.bit_length() - 1
    err = Fraction((logn + 1) * (n * pmax * (1 << _GUARD) + n) * mul, den)
    return re, im, err
