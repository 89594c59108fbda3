"""Pinning of tests/exactref.py (the exact reference of the real-slot encoder and the plaintext NTT) against the pure-Python definitions in
pyref and against closed forms.  CPU only."""
import mpmath as mp
import numpy as np
import pytest

import exactref
import pyref


@pytest.mark.parametrize("logN", [4, 6, 8])
def test_encode_matches_direct_sum(logN):
    N = 1 << logN
    rnd = np.random.default_rng(logN)
    for scale_exp in (0, 17, 40):
        v = rnd.normal(size=N // 2) * 10.0 ** scale_exp
        p, tie, err = exactref.encode(v, N, 2.0 ** 34)
        assert p == pyref.encode_exact(v, N, 2.0 ** 34)
        assert tie.min() > err


def test_encode_scaled_is_encode_at_each_scale():
    N = 64
    v = np.random.default_rng(1).normal(size=N // 2)
    many = exactref.encode_scaled(v, N, [2.0 ** 34, 2.0 ** 50, 3.0])
    for s, got in zip([2.0 ** 34, 2.0 ** 50, 3.0], many):
        assert got[0] == exactref.encode(v, N, s)[0] == pyref.encode_exact(v, N, s)


def test_constant_vector_is_p0_only():
    N, scale = 16384, 2.0 ** 34
    for c in (1.0, -3.25, 123456.75, 2.0 ** 18 + 0.5):
        p, _, _ = exactref.encode(np.full(N // 2, c), N, scale)
        assert p[0] == int(c * scale) and not any(p[1:])


def test_single_slot_is_cosines():
    N, scale, n = 16384, 2.0 ** 34, 8192
    t0, a = 777, 1.0e5 + 0.375
    v = np.zeros(n)
    v[t0] = a
    p, _, _ = exactref.encode(v, N, scale)
    e = pow(5, t0, 2 * N)
    with mp.workdps(60):
        for c in (0, 1, 2, 1234, 4096, 8191):
            ang = mp.mpf(e * c % (2 * N)) / N               # zeta^(-5^t0 c) = exp(-i pi ang)
            re, im = a * scale / n * mp.cospi(ang), -a * scale / n * mp.sinpi(ang)
            rnd = lambda x: int(mp.sign(x) * mp.floor(abs(x) + mp.mpf(0.5)))       # noqa: E731
            assert p[c] == rnd(re) and p[c + n] == rnd(im), c


def test_tie_distance_and_half_away_rounding():
    N = 16
    p, tie, _ = exactref.encode(np.full(8, 2.5), N, 1.0)            # p_0 = 2.5 exactly: a tie, rounded away from zero
    assert p[0] == 3 and tie[0] == 0.0
    p, tie, _ = exactref.encode(np.full(8, -2.5), N, 1.0)
    assert p[0] == -3 and tie[0] == 0.0
    p, tie, _ = exactref.encode(np.full(8, 2.25), N, 1.0)
    assert p[0] == 2 and tie[0] == 0.25


@pytest.mark.parametrize("logN,q", [(4, 7681), (5, 7681), (6, 12289)])
def test_ntt_matches_direct_evaluation(logN, q):
    N = 1 << logN
    psi = exactref.psi_for(q, N)
    assert pow(psi, N, q) == q - 1
    rnd = np.random.default_rng(logN)
    rows = [rnd.integers(-2 ** 53, 2 ** 53, N) for _ in range(3)]
    got = exactref.ntt(rows, q, psi)
    for r, g in zip(rows, got):
        assert [int(x) for x in g] == pyref.ntt_direct([int(x) % q for x in r], psi, q, logN)


def test_ntt_large_modulus_products_are_exact():
    """a 46-bit modulus (the size of q0): the limb products must not overflow"""
    from sfgwas_amd.params import Q_PN14
    q, logN = Q_PN14[0], 5
    N = 1 << logN
    g = exactref.psi_for(q, 1 << 14)
    psi = pow(g, (1 << 14) // N, q)                      # a primitive 2N-th root for the small size
    rnd = np.random.default_rng(9)
    row = [int(x) for x in rnd.integers(0, q, N)]
    assert [int(x) for x in exactref.ntt([row], q, psi)[0]] == pyref.ntt_direct(row, psi, q, logN)
