"""The modulus chains of the general ring's tests (sfgwas_amd/csrc/gring.hip), shared by tests/test_ring_ref.py and tests/test_gpu_ring.py.

name   logN  q (bits)             p (bits)   what it is there for
G12    12    37, 32               38         PN12-shaped; np = 1; a raw-copy digit whose source modulus exceeds its target
G13    13    33, 5 x 30           35         PN13-shaped; odd logN; six single-modulus digits
W15    15    50, 3 x 40           3 x 50     PN15-shaped; a row no longer fits LDS; np = 3 > moduli at levels 0-1; q0 and P are distinct 50-bit primes
W16    16    55, 2 x 45           2 x 55     PN16-shaped; the largest row; ragged last digit
X12    12    3 just below 2^61    2          the widest words: 4q near 2^63, (double)y rounds
X15    15    3 just below 2^61    2
L19    12    17 x 36              2 x 36     19 moduli, more than the oracle ring holds; beta = 9
P14    14    Q_PN14               P_PN14     both paths on the same parameters
"""
import functools

import numpy as np

import oracle_lib as ol


@functools.lru_cache(maxsize=None)
def chain(name):
    """-> (logN, q, p)"""
    sp = ol.small_primes
    if name == "G12":
        return 12, sp(12, 37, 1) + sp(12, 32, 1), sp(12, 38, 1)
    if name == "G13":
        return 13, sp(13, 33, 1) + sp(13, 30, 5), sp(13, 35, 1)
    if name == "W15":
        return 15, sp(15, 50, 1) + sp(15, 40, 3), sp(15, 50, 3, skip=1)
    if name == "W16":
        return 16, sp(16, 55, 1) + sp(16, 45, 2), sp(16, 55, 2, skip=1)
    if name in ("X12", "X15"):
        logN = int(name[1:])
        return logN, sp(logN, 61, 3), sp(logN, 61, 2, skip=3)
    if name == "L19":
        return 12, sp(12, 36, 17), sp(12, 36, 2, skip=17)
    if name == "P14":
        return 14, list(ol.Q_PN14), list(ol.P_PN14)
    raise KeyError(name)


NAMES = ["G12", "G13", "W15", "W16", "X12", "X15", "L19", "P14"]


def levels(name):
    """top, one in the middle, 0 (W15: 3, 1, 0 - both sides of np = 3 > level + 1)"""
    if name == "W15":
        return [3, 1, 0]
    top = len(chain(name)[1]) - 1
    return sorted({top, top // 2, 0}, reverse=True)


def all_moduli():
    out = []
    for n in NAMES:
        _, q, p = chain(n)
        out += [m for m in q + p if m not in out]
    return out


def directed_rows(q, N):
    """all q - 1, all 0, one-hot at 0 and at N - 1, alternating 0, q - 1"""
    rows = np.zeros((5, N), dtype=np.uint64)
    rows[0] = q - 1
    rows[2, 0] = 1
    rows[3, N - 1] = 1
    rows[4, 1::2] = q - 1
    return rows


def digits(level, alpha):
    nl = level + 1
    return [list(range(s, min(s + alpha, nl))) for s in range(0, nl, alpha)]
