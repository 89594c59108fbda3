"""Pins tests/decode_ref.py, the exact decoder the device tests measure against (and the big-integer statement of the collective key switch they use)."""
import random
from fractions import Fraction

import numpy as np

import decode_ref
import encrypt_ref as er
import exactref
import pyref
from test_encrypt_ref import _primes


def test_against_the_direct_mpmath_sum_at_n64():
    import mpmath as mp
    N, n, M = 64, 32, 128
    rnd = random.Random(3)
    for scale in (Fraction(2) ** 34, Fraction(2 ** 68, 34359410689), Fraction(7, 3)):
        p = [rnd.randrange(-(1 << 90), 1 << 90) for _ in range(N)]
        re, im, err = decode_ref.decode(p, N, scale)
        with mp.workdps(120):
            sc = mp.mpf(scale.numerator) / mp.mpf(scale.denominator)
            big = max(abs(x) for x in p) / sc
            for t in range(n):
                g = pow(5, t, M)
                acc = mp.mpc(0)
                for c in range(n):
                    acc += mp.mpc(p[c], p[c + n]) * mp.expjpi(mp.mpf(2 * ((g * c) % M)) / M)
                acc /= sc
                got = mp.mpc(mp.mpf(re[t].numerator) / mp.mpf(re[t].denominator), mp.mpf(im[t].numerator) / mp.mpf(im[t].denominator))
                assert abs(got - acc) <= big * mp.mpf(2) ** -150, (scale, t)
        assert err <= Fraction(max(abs(x) for x in p)) / scale / (1 << 150)


def test_round_trip_at_n16384_within_the_encoders_rounding():
    N, n = 1 << 14, 1 << 13
    scale = 2.0 ** 34
    v = np.random.default_rng(5).uniform(-100, 100, n)
    p, _, _ = exactref.encode(v, N, scale)
    re, im, err = decode_ref.decode(p, N, Fraction(scale))
    bound = Fraction(n) * Fraction(14142135623730951, 10 ** 16) / (2 * Fraction(scale)) + 2 * err     # n sqrt(2) / (2 scale)
    worst = max(max(abs(re[t] - Fraction(float(v[t]))), abs(im[t])) for t in range(n))
    print(f"round trip: max |decode(encode(v)) - v| = {float(worst):.3e}, bound {float(bound):.3e}")
    assert worst <= bound


def test_slot_order_is_pyrefs():
    N, n = 256, 128
    rnd = random.Random(9)
    p = [rnd.randrange(-(1 << 40), 1 << 40) for _ in range(N)]
    scale = 2.0 ** 30
    re, im, _ = decode_ref.decode(p, N, Fraction(scale))
    want = pyref.decode(np.array([float(x) / scale for x in p]), N)
    got = np.array([float(x) for x in re]) + 1j * np.array([float(x) for x in im])
    assert np.abs(got - want).max() <= 1e-10 * np.abs(want).max()
    assert np.abs(want - want[::-1]).max() > 1e-3 * np.abs(want).max()            # (an order mistake would show)


def test_two_party_collective_key_switch_statement_on_a_tiny_ring():
    """c0 + sum_i h0_i = c0 + s c1 + sum_i ModDown(e0_i), s = s1 + s2, with h0_i = ModDown_P(NTT_QP(e0_i)) + s_i (.) c1 - the zero public key's GenShare, in big integers"""
    rnd = random.Random(21)
    logN, N = 4, 16
    q, p = _primes(2 * N, 20, 3), _primes(2 * N, 12, 2)
    ring = er.TinyRing(logN, q, p)
    level = 2
    s_i = [[rnd.choice((-1, 0, 1)) for _ in range(N)] for _ in range(2)]
    s = [a + b for a, b in zip(*s_i)]
    zero_pk = [[np.array([0] * N, dtype=object) for _ in ring.moduli] for _ in range(2)]
    c0 = [[rnd.randrange(m) for _ in range(N)] for m in q]                       # coefficient domain
    c1 = [[rnd.randrange(m) for _ in range(N)] for m in q]
    e = [[[rnd.randint(-38, 38) for _ in range(N)] for _ in range(2)] for _ in range(2)]
    for m, mod in enumerate(q):
        c1h = ring.ntt(m, c1[m])
        agg = ring.ntt(m, c0[m])
        noise = np.array([0] * N, dtype=object)
        for i in range(2):
            md = er.encrypt_bigint(ring, level, zero_pk, [0] * N, e[i][0], e[i][1])[m]
            h0 = (md[0] + ring.ntt(m, [x % mod for x in s_i[i]]) * c1h) % mod
            agg = (agg + h0) % mod
            noise = (noise + ring.intt(m, md[0])) % mod
        want = (np.array(c0[m], dtype=object) + np.array(er.negacyclic(s, c1[m]), dtype=object) + noise) % mod
        assert list(ring.intt(m, agg)) == list(want), m
