"""Exact reference for the ring-vector encoder and decoder (sfgwas_amd/csrc/rvec.hip), independent of the kernels and of the C oracle.

N a power of two, n = N/2 slots, zeta = exp(2 pi i / 2N), slot t <-> 5^t = 4 m_t + 1 (mod 2N); p an odd field modulus, centre(x) = x if x <= (p - 1)/2 else x - p;
scale an exact rational >= 1, f = frac_bits.

    encode(x, p, N, scale, f):  s_t = centre(x_t) (zero beyond len(x)),  w_c = (1/n) sum_t s_t zeta^(-5^t c),
                                p_c = round(scale 2^-f Re w_c),  p_{c+n} = round(scale 2^-f Im w_c)
    decode(c, p, N, scale, f, n_elem):  v_t = sum_c (c_c + i c_{c+n}) zeta^(5^t c),  r_t = round(2^f / scale Re v_t) mod p,  t < n_elem

Both are length-n DFTs behind a twist (5^t c = 4 m_t c + c), done as a radix-2 FFT on Python integers in the structure of exactref._fft_fixed and decode_ref.decode:
the inputs are exact integers shifted left by _GUARD bits, the twiddles are mpmath values rounded to 2^-_TW_BITS (640 bits: the 240-bit tables of exactref are too
short for 360-bit inputs), every product is floored once at 2^-_GUARD of an input unit.

Error accounting (the model is the docstring of decode_ref.py), in units of 2^-_GUARD of a transform value: a complex product floors two real products per component
(< 2 units) and its twiddle is off by at most 2^-_TW_BITS per component, which on an operand of modulus <= B costs at most 2 * 2^-_TW_BITS B per component.  Every
intermediate that feeds an output is a sum over a subset of the inputs with unit-modulus weights, so B <= n A 2^_GUARD with A the largest input modulus.  An output
collects the errors of every product of its tree - fewer than 2 n products, the twist's included - with unit gain:  E = 2 n (2 + 2^(1 - _TW_BITS) n A 2^_GUARD)
units per component, far below one unit of the result after scaling for every input the tests use.  Every result carries that bound (`err`, in units of the
rounded output) and its distance to the nearest rounding tie; a comparison is exact wherever the distance exceeds the bound of the device plus `err`.
"""
from fractions import Fraction
import functools

import numpy as np

_TW_BITS = 640
_GUARD = 160


def _brev(x, bits):
    r = 0
    for _ in range(bits):
        r = (r << 1) | (x & 1)
        x >>= 1
    return r


@functools.lru_cache(maxsize=None)
def tables(N):
    """(m_t for every slot t, bit-reversal permutation, zeta^j for j < N as two object arrays of integers scaled by 2^_TW_BITS)"""
    import mpmath as mp
    n, M = N // 2, 2 * N
    logn = n.bit_length() - 1
    m_of = [0] * n
    g = 1
    for t in range(n):
        m_of[t] = ((g - 1) // 4) % n
        g = g * 5 % M
    one = 1 << _TW_BITS
    with mp.workdps(_TW_BITS // 3 + 30):
        C = [int(mp.nint(mp.cospi(mp.mpf(j) / N) * one)) for j in range(n + 1)]        # cos(pi j / N), j <= N/2
    cos = [C[j] if j <= n else -C[N - j] for j in range(N)]
    sin = [C[n - j] if j <= n else C[j - n] for j in range(N)]
    perm = np.array([_brev(i, logn) for i in range(n)], dtype=np.int64)
    obj = lambda a: np.array(a, dtype=object)      # noqa: E731
    return np.array(m_of, dtype=np.int64), perm, obj(cos), obj(sin)


def _fft(xr, xi, N, sign):
    """DFT_n with kernel exp(sign 2 pi i m c / n) of the integer vectors (object arrays, natural order in, natural order out), floored once per product"""
    n = N // 2
    _, perm, cos, sin = tables(N)
    xr, xi = xr[perm].copy(), xi[perm].copy()
    half = 1
    while half < n:
        idx = (np.arange(half) * (N // half))
        tr, ti = cos[idx], sin[idx] * sign
        ar, ai = xr.reshape(-1, 2, half), xi.reshape(-1, 2, half)
        br, bi = ar[:, 1, :], ai[:, 1, :]
        qr = (br * tr - bi * ti) >> _TW_BITS
        qi = (br * ti + bi * tr) >> _TW_BITS
        lr, li = ar[:, 0, :], ai[:, 0, :]
        xr = np.concatenate([lr + qr, lr - qr], axis=1).reshape(-1)
        xi = np.concatenate([li + qi, li - qi], axis=1).reshape(-1)
        half *= 2
    return xr, xi


def _err_units(n, amax):
    return 2 * n * (2 + Fraction(n * max(1, amax) << _GUARD, 1 << (_TW_BITS - 1)))


def _round(num, den):
    """(nearest integer to num / den, den > 0, ties away from zero; distance of num / den to the nearest tie as a Fraction)"""
    a = -num if num < 0 else num
    r = (2 * a + den) // (2 * den)
    dist = abs(Fraction(2 * (a % den) - den, 2 * den))
    return (-r if num < 0 else r), dist


def centre(x, p):
    return x if x <= (p - 1) // 2 else x - p


def encode(x, p, N, scale, f):
    """x: up to n field elements in [0, p) -> (coefficients: list of N ints, tie: list of N Fractions, err: Fraction, units of a coefficient)"""
    n = N // 2
    scale = Fraction(scale)
    assert len(x) <= n and p % 2 == 1 and scale >= 1 and 0 <= f <= 62
    m_of, _, cos, sin = tables(N)
    s = [centre(int(v), p) for v in x]
    assert all(0 <= int(v) < p for v in x)
    ur = np.zeros(n, dtype=object)
    ur[:] = 0
    for t, v in enumerate(s):
        ur[m_of[t]] = v << _GUARD
    ui = np.zeros(n, dtype=object)
    ui[:] = 0
    xr, xi = _fft(ur, ui, N, -1)
    zr, zi = cos[:n], -sin[:n]                                   # zeta^-c
    yr = (xr * zr - xi * zi) >> _TW_BITS
    yi = (xr * zi + xi * zr) >> _TW_BITS
    den = n * (1 << (_GUARD + f)) * scale.denominator
    out, tie = [0] * N, [None] * N
    for c in range(n):
        out[c], tie[c] = _round(int(yr[c]) * scale.numerator, den)
        out[c + n], tie[c + n] = _round(int(yi[c]) * scale.numerator, den)
    amax = max([abs(v) for v in s] + [1])
    err = _err_units(n, amax) * scale / (n * (1 << (_GUARD + f)))
    return out, tie, err


def decode_int(c, N, scale, f, n_elem=None):
    """c: N integer coefficients -> (round(2^f / scale Re v_t) as signed ints, t < n_elem; tie: list of Fractions; err: Fraction, units of the result)"""
    n = N // 2
    n_elem = n if n_elem is None else n_elem
    scale = Fraction(scale)
    assert len(c) == N and scale >= 1 and 0 <= f <= 62 and 1 <= n_elem <= n
    m_of, _, cos, sin = tables(N)
    pr = np.array([int(v) << _GUARD for v in c[:n]], dtype=object)
    pi = np.array([int(v) << _GUARD for v in c[n:]], dtype=object)
    zr, zi = cos[:n], sin[:n]                                    # zeta^c
    ar = (pr * zr - pi * zi) >> _TW_BITS
    ai = (pr * zi + pi * zr) >> _TW_BITS
    xr, _ = _fft(ar, ai, N, +1)
    den = (1 << _GUARD) * scale.numerator
    mul = (1 << f) * scale.denominator
    r, tie = [0] * n_elem, [None] * n_elem
    for t in range(n_elem):
        r[t], tie[t] = _round(int(xr[m_of[t]]) * mul, den)
    amax = max(1, max(abs(int(v)) for v in c)) * 2               # |c_c + i c_{c+n}| <= sqrt 2 max |c|
    err = _err_units(n, amax) * Fraction(mul, den)
    return r, tie, err


def decode(c, p, N, scale, f, n_elem=None):
    """the same reduced into [0, p): what the library returns"""
    assert p % 2 == 1
    r, tie, err = decode_int(c, N, scale, f, n_elem)
    return [v % p for v in r], tie, err


def centred_crt(x, Q):
    """the integer a residue x of Q stands for under lattigo's Cmp(QHalf) rule (recode.hpp garner_negative): x >= floor(Q / 2) is x - Q"""
    x %= Q
    return x - Q if x >= Q // 2 else x


def literal_encode_value(x, p, N, c, dps=120):
    """w_c of the definition by the literal O(n) mpmath sum: (Re, Im) as mpf"""
    import mpmath as mp
    n = N // 2
    with mp.workdps(dps):
        acc = mp.mpc(0)
        g = 1
        for t in range(n):
            if t < len(x):
                acc += centre(int(x[t]), p) * mp.expjpi(-mp.mpf(g * c % (2 * N)) / N)
            g = g * 5 % (2 * N)
        acc /= n
        return +acc.real, +acc.imag


def literal_decode_value(c, N, t, dps=120):
    """Re v_t of the definition by the literal O(n) mpmath sum"""
    import mpmath as mp
    n = N // 2
    with mp.workdps(dps):
        g = pow(5, t, 2 * N)
        acc = mp.mpc(0)
        for k in range(n):
            acc += mp.mpc(int(c[k]), int(c[k + n])) * mp.expjpi(mp.mpf(g * k % (2 * N)) / N)
        return +acc.real


def q_product(q, level):
    Q = 1
    for v in q[:level + 1]:
        Q *= int(v)
    return Q


def plan(direction, pbits, qbits, scale, f):
    """(W, g) the library picks (rvec_host.hpp), restated: the tests list which widths their cases reach"""
    import math
    scale = Fraction(scale)
    fl = scale.numerator.bit_length() - scale.denominator.bit_length()
    if Fraction(2) ** fl > scale:
        fl -= 1
    cl = fl if Fraction(2) ** fl == scale else fl + 1
    if direction == "enc":
        g = 48 + max(0, cl - f - 13)
        bits = (pbits - 1) + 13 + 2 + g + 1
    else:
        g = 48 + max(0, f - fl)
        bits = qbits + 14 + 2 + g + 1
    return max(2, math.ceil(bits / 64)), g
