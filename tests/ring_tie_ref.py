"""Python-integer restatement of sfgwas_amd/csrc/gring_tie.hpp (the exact re-derivation of near-tie diagonal coefficients in the general ring's products) and
the constructors of directed near-ties that tests/test_ring_tie_ref.py (CPU) and tests/test_gpu_ring_tie.py (GPU) share.

The statement is tests/exactref.py's: p_j = (scale / n) sum_t v_t cos(pi (5^t j mod 2N) / N), rounded half away from zero."""
import functools
import math
import struct

FRAC = 191          # gtie::kFrac
TAB_ERR = 1         # gtie::kTabErr, units of 2^-FRAC
CAP = 512           # gtie::kCap


@functools.lru_cache(maxsize=None)
def table(N):
    """round(cos(pi k / N) 2^FRAC), k = 0 .. N / 2, from mpmath"""
    import mpmath as mp
    with mp.workdps(90):
        one = mp.mpf(2) ** FRAC
        return [int(mp.nint(mp.cospi(mp.mpf(k) / N) * one)) for k in range(N // 2 + 1)]


def fold(a, N):
    """angle pi a / N, 0 <= a < 2N -> (table index <= N / 2, negative?)"""
    if a > N:
        a = 2 * N - a
    return (N - a, True) if a > N // 2 else (a, False)


def split_scale(scale):
    """scale = m 2^e, m an integer in [2^52, 2^53)"""
    fr, ex = math.frexp(scale)
    m = int(math.ldexp(fr, 53))
    assert m * 2.0 ** (ex - 53) == scale and 1 << 52 <= m < 1 << 53
    return m, ex - 53


def decide(X, m, e, logn, A):
    """-> (status, p): 0 proven, 1 unproven, 2 outside |p| < 2^62; p is meaningful at status 0"""
    neg, Y = X < 0, m * abs(X)
    if Y == 0:
        return 0, 0
    sh = FRAC + logn - e
    num, den = (Y, 1 << sh) if sh > 0 else (Y << -sh, 1)
    ip, rem = divmod(num, den)
    up = 2 * rem >= den
    p = ip + (1 if up else 0)
    if p >= 1 << 62:
        return 2, 0
    proven = den == 1 or abs(2 * rem - den) > 2 * m * TAB_ERR * A
    return (0 if proven else 1), (-p if neg else p)


def sum_terms(tab, N, v, j):
    """(X, A) for the slot values v: {t: v_t} or a full list"""
    items = v.items() if isinstance(v, dict) else enumerate(v)
    X = A = 0
    for t, x in items:
        if not x:
            continue
        k, neg = fold(pow(5, t, 2 * N) * j % (2 * N), N)
        X += -x * tab[k] if neg else x * tab[k]
        A += abs(x)
    return X, A


def coefficient(tab, N, v, j, scale):
    X, A = sum_terms(tab, N, v, j)
    m, e = split_scale(scale)
    return decide(X, m, e, N.bit_length() - 2, A)


def bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def step(x, ulps):
    return struct.unpack("<d", struct.pack("<Q", bits(x) + ulps))[0]


def directed_scale(N, t0, j, K):
    """the double nearest n (K + 1/2) / |cos(pi 5^t0 j / N)|: a vector with a single 1 at slot t0 then has p_j (and p_(N-j)) within a few 2^-53 K of a tie"""
    import mpmath as mp
    n = N // 2
    with mp.workdps(60):
        c = abs(mp.cospi(mp.mpf(pow(5, t0, 2 * N) * j % (2 * N)) / N))
        return float(n * (mp.mpf(K) + mp.mpf(1) / 2) / c)


# (t0, j, K) at N = 4096: exactly {j, N - j} fall inside 2^-50 of a tie, at the directed scale and one ulp either side, where both roundings are reached
# (two and three ulps away some coefficients already leave the band)
DIRECTED_4096 = [(5, 1, 2), (17, 2049, 1), (100, 4095, 3), (7, 1000, 0)]
ULPS = (-1, 0, 1)
