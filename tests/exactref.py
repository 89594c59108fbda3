"""Exact references for the real-slot encoder and the plaintext NTT, independent of the kernels and of the C oracle.

encode(v, N, scale) computes, for every c in [0, n) (n = N/2 slots, zeta = exp(2 pi i / 2N)),
    w_c = (1/n) sum_t v_t zeta^(-5^t c),   p_c = round(scale Re w_c),   p_{c+n} = round(scale Im w_c)
rounded half away from zero (lattigo's rule), for the doubles v_t actually given.  With 5^t = 4 m + 1 (mod 2N) the sum is
zeta^-c times a length-n DFT of u_m = v_t, done here as a plain radix-2 FFT on integers: the inputs are fixed point with
200 bits below max |v|, the twiddles are mpmath values (dps 70) rounded to 2^-240.  All N coefficients come out of the
full complex transform; nothing assumes the antisymmetry p_{N-c} = -p_c.  The error of the fixed-point values is returned
(`err`, a bound in units of p); every coefficient also carries its distance to the nearest rounding tie.

ntt(rows, q, psi) is the negacyclic NTT mod q in lattigo's bit-reversed output order, out[i] = p(psi^(2 brev(i) + 1)),
on exact uint64 integers (vectorised over rows; products by 16-bit limbs): O(N log N).
"""
from fractions import Fraction
import functools
import math

import numpy as np

_TW_BITS = 240          # twiddle fixed point
_IN_BITS = 200          # input fixed point below the largest |v_t|


def _brev(x, bits):
    r = 0
    for _ in range(bits):
        r = (r << 1) | (x & 1)
        x >>= 1
    return r


@functools.lru_cache(maxsize=None)
def _tables(N):
    """(slot of each FFT input m, bit-reversal permutation, stage twiddles exp(-2 pi i k / n), twist zeta^-c) as fixed-point ints."""
    import mpmath as mp
    n, M = N // 2, 2 * N
    logn = n.bit_length() - 1
    slot = [0] * n
    g = 1
    for t in range(n):
        slot[((g - 1) // 4) % n] = t
        g = g * 5 % M
    one = 1 << _TW_BITS
    with mp.workdps(70):
        def fx(x):
            return int(mp.nint(x * one))
        # exp(-2 pi i k / n), k < n/2
        wr = [fx(mp.cospi(mp.mpf(2 * k) / n)) for k in range(n // 2)]
        wi = [-fx(mp.sinpi(mp.mpf(2 * k) / n)) for k in range(n // 2)]
        # zeta^-c = exp(-pi i c / N), c < n
        zr = [fx(mp.cospi(mp.mpf(c) / N)) for c in range(n)]
        zi = [-fx(mp.sinpi(mp.mpf(c) / N)) for c in range(n)]
    perm = np.array([_brev(i, logn) for i in range(n)], dtype=np.int64)
    obj = lambda a: np.array(a, dtype=object)      # noqa: E731
    return np.array(slot, dtype=np.int64), perm, obj(wr), obj(wi), obj(zr), obj(zi)


def _fft_fixed(ur, N):
    """DFT_n (kernel exp(-2 pi i m c / n)) of the integer vector ur (object array), times zeta^-c: (re, im) scaled by 2^_TW_BITS."""
    n = N // 2
    _, perm, wr, wi, zr, zi = _tables(N)
    xr = ur[perm].copy()
    xi = np.zeros(n, dtype=object)
    xi[:] = 0
    half = 1
    while half < n:
        step = n // (2 * half)
        tr, ti = wr[::step][:half], wi[::step][:half]
        ar, ai = xr.reshape(-1, 2, half), xi.reshape(-1, 2, half)
        br, bi = ar[:, 1, :], ai[:, 1, :]
        pr = (br * tr - bi * ti) >> _TW_BITS
        pi = (br * ti + bi * tr) >> _TW_BITS
        lr, li = ar[:, 0, :], ai[:, 0, :]
        xr = np.concatenate([lr + pr, lr - pr], axis=1).reshape(-1)
        xi = np.concatenate([li + pi, li - pi], axis=1).reshape(-1)
        half *= 2
    return xr * zr - xi * zi, xr * zi + xi * zr


def _round_away(num, den):
    """(p, tie distance) for num / den, den > 0: p rounded half away from zero, distance of num/den from the nearest tie."""
    a = -num if num < 0 else num
    p = (2 * a + den) // (2 * den)
    r = a % den
    dist = abs(2 * r - den) / (2 * den)
    return (-p if num < 0 else p), dist


def encode(v, N, scale):
    """-> (p: list of N Python ints, tie: float array [N] distance to the nearest rounding tie, err: bound on the fixed-point error, units of p)."""
    return encode_scaled(v, N, [scale])[0]


def encode_scaled(v, N, scales):
    """encode(v, N, s) for every s in scales from ONE transform (the fixed-point values are exact multiples of the scale)."""
    n = N // 2
    v = np.asarray(v, dtype=np.float64)
    assert v.shape == (n,) and np.all(np.isfinite(v))
    slot = _tables(N)[0]
    vmax = float(np.max(np.abs(v)))
    if vmax == 0.0:
        return [([0] * N, np.full(N, 0.5), 0.0) for _ in scales]
    G = _IN_BITS - math.frexp(vmax)[1]                 # |u_m| <= 2^_IN_BITS
    u = np.array([int(Fraction(float(x)) * (Fraction(2) ** G)) for x in v[slot]], dtype=object)
    re, im = _fft_fixed(u, N)
    re, im = [int(x) for x in re], [int(x) for x in im]
    return [_rounded(re, im, G, Fraction(s), N) for s in scales]


def _rounded(re, im, G, sc, N):
    n = N // 2
    den = n * (1 << _TW_BITS) * sc.denominator
    if G >= 0:
        den <<= G
        mul = sc.numerator
    else:
        mul = sc.numerator << -G
    p, tie = [0] * N, np.zeros(N)
    for c in range(n):
        p[c], tie[c] = _round_away(re[c] * mul, den)
        p[c + n], tie[c + n] = _round_away(im[c] * mul, den)
    # error, units of 2^-G in u: inputs (truncated toward zero) < n, each of the log2(n) stages < 2 per point feeding an output (2^(j+1) of them
    # at depth j), twiddle rounding ~2^-200 relative; the twist adds one more unit.  Bounded by 2^17 units, scaled by scale / n.
    err = float(sc) / n * 2.0 ** (17 - G)
    return p, tie, err


@functools.lru_cache(maxsize=None)
def psi_for(q, N):
    """the 2N-th root of unity lattigo's NTT uses: g^((q - 1) / 2N) for the smallest primitive root g of q"""
    from sympy.ntheory import primitive_root
    return pow(primitive_root(q), (q - 1) // (2 * N), q)


@functools.lru_cache(maxsize=64)
def _psi_rev(q, psi, N):
    logN = N.bit_length() - 1
    pw = [1] * N
    for k in range(1, N):
        pw[k] = pw[k - 1] * psi % q
    return np.array([pw[_brev(k, logN)] for k in range(N)], dtype=np.uint64)


def _mulmod(a, w, q):
    """a * w mod q for uint64 arrays a, w < q < 2^47, exactly: Horner over the 16-bit limbs of w (every partial sum < 2^63)."""
    t = np.zeros_like(a)
    for k in (2, 1, 0):
        wk = (w >> np.uint64(16 * k)) & np.uint64(0xFFFF)
        t = ((t << np.uint64(16)) + a * wk) % q
    return t


def ntt(rows, q, psi):
    """rows: [R][N] integers (any sign) -> [R][N] canonical NTT words mod q (uint64)."""
    assert q < 1 << 47
    a = np.array([[int(x) % q for x in r] for r in rows], dtype=np.uint64)
    R, N = a.shape
    S = _psi_rev(q, psi, N)
    qq = np.uint64(q)
    m, t = 1, N
    while m < N:
        t //= 2
        b = a.reshape(R, m, 2, t)
        U = b[:, :, 0, :]
        V = _mulmod(b[:, :, 1, :], np.broadcast_to(S[m:2 * m][None, :, None], U.shape), qq)
        a = np.stack([(U + V) % qq, (U + qq - V) % qq], axis=2).reshape(R, N)
        m *= 2
    return a
