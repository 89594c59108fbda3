"""Inputs of the ring-vector encoder / decoder tests, shared by the CPU test of the host arithmetic (test_rvec_ref.py) and the device test (test_gpu_rvec.py).

Every input is seeded or directed; the seeds were chosen with tests/rvec_ref.py alone so that no output of any of them lies within 2^-32 of a rounding tie (the tests
assert that again: the near-tie rule can then hide nothing).
"""
from fractions import Fraction

import numpy as np

N = 1 << 14
n = N // 2
F = 30
SCALE = Fraction(2 ** 34)
SCALE_ODD = Fraction(float(2.0 ** 34 * 1.2345678901))        # a double that is not a power of two, taken exactly
FIELDS = {2: 2 ** 128 - 159, 4: 2 ** 256 - 189}               # both in field_ref's lists
TIE_BAND = Fraction(1, 2 ** 32)


def limbs_of(vals, limbs):
    """ints -> uint64 [len][limbs], little-endian words"""
    return np.array([[(int(v) >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(limbs)] for v in vals], dtype=np.uint64).reshape(len(vals), limbs)


def ints_of(words):
    """uint64 [k][limbs] -> list of ints"""
    return [sum(int(w) << (64 * i) for i, w in enumerate(row)) for row in words]


def modulus_words(p, limbs):
    return limbs_of([p], limbs)[0].copy()


def uniform_elems(p, count, seed):
    rnd = np.random.default_rng(seed)
    nb = (p.bit_length() + 7) // 8 + 8
    return [int.from_bytes(rnd.bytes(nb), "little") % p for _ in range(count)]


def encode_inputs(p):
    """name -> list of field elements (len = n_elem).  max = (p - 1)/2 is the largest centred value, (p + 1)/2 stands for -max."""
    hi, lo = (p - 1) // 2, (p + 1) // 2
    boundary = [0, 1, p - 1, hi, lo]
    one = [0] * n
    one[4097] = uniform_elems(p, 1, 5)[0]
    # the +- pattern aligned to the root of c = n/2: zeta^(5^t n/2) = +-exp(i pi/4) with the sign of 5^t mod 8, so w_{n/2} = max exp(-i pi/4) takes the whole sum
    pattern, g = [], 1
    for _ in range(n):
        pattern.append(hi if g % 8 == 1 else lo)
        g = g * 5 % (2 * N)
    return {
        "uniform": uniform_elems(p, n, 11),
        "uniform_8191": uniform_elems(p, n - 1, 12),
        "uniform_1": uniform_elems(p, 1, 13),
        "boundary": [boundary[t % 5] for t in range(n)],
        "all_max": [hi] * n,
        "all_min": [lo] * n,
        "one_slot": one,
        "pattern": pattern,
    }


def decode_inputs(Q):
    """name -> list of N residues of Q (what the plaintext rows hold); the integer each stands for is rvec_ref.centred_crt's"""
    h = Q // 2
    rnd = np.random.default_rng(21)
    nb = (Q.bit_length() + 7) // 8 + 8
    uni = [int.from_bytes(rnd.bytes(nb), "little") % Q for _ in range(N)]
    single = [0] * N
    single[n + 77] = (Q - uni[0] // 3) % Q
    single_tie = [0] * N
    single_tie[3] = h
    return {
        "uniform": uni,
        "all_half_tie": [h] * N,              # the residue floor(Q/2): lattigo's rule makes it negative, -(Q + 1)/2
        "all_pos_max": [h - 1] * N,           # the largest positive value
        "all_neg": [(-h + 1) % Q] * N,        # -floor(Q/2) + 1
        "zero": [0] * N,
        "single": single,
        "single_tie": single_tie,             # one coefficient at the residue garner_negative treats as the tie x = floor(Q/2)
    }
