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

EDGE_NAMES (tests/test_ring_edges_ref.py, tests/test_gpu_ring_edges.py; all at logN 12 - what is at stake is the chain, not N):
R21    12    18 x 61              3 x 61     PN15's digit shape with the widest words: alpha = 3, beta = 6, every digit full at the top level
R38    12    34 x 61              4 x 61     PN16's shape: alpha = 4, beta = 9, a last digit of 2; the float sum can round DOWN from alpha = 4 on
M48    12    47 x 61              1 x 61     beta = 47 single-modulus digits: the key sum's ceiling (also the bootstrap's widest chain, tests/ring_refresh_ref.py)
A48    12    1 x 61               47 x 61    alpha = 47: one ModDown digit of 47 moduli, v up to 46 - the extension sum's ceiling
V12    12    30, 61, 45           2 x 61     rescale and raw-copy digits whose source modulus is 2^31 times the target
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
    if name == "R21":
        m = sp(12, 61, 21)
        return 12, m[:18], m[18:]
    if name == "R38":
        m = sp(12, 61, 38)
        return 12, m[:34], m[34:]
    if name == "M48":
        m = sp(12, 61, 48)
        return 12, m[:47], m[47:]
    if name == "A48":
        m = sp(12, 61, 48)
        return 12, m[:1], m[1:]
    if name == "V12":
        return 12, sp(12, 30, 1) + sp(12, 61, 1) + sp(12, 45, 1), sp(12, 61, 2, skip=1)
    raise KeyError(name)


NAMES = ["G12", "G13", "W15", "W16", "X12", "X15", "L19", "P14"]
EDGE_NAMES = ["R21", "R38", "M48", "A48", "V12"]              # chains of the edge tests only: NAMES parametrises the other files and stays as it is

# (chain, level) of the edge tests.  EDGE_KS: the directed rotation and product under a uniform key - W15 on both sides of np = 3 > level + 1, X15 at logN 15 (tiles
# that span workgroups), R21 at its top and at level 9 (digits of 3, 3, 3, 1), R38's nine digits, V12's raw copies 61 -> 30 and 61 -> 45 bits and, at level 0,
# 30 -> 61 alone, A48's ModDown digit of 47 moduli.
# EDGE_MODDOWN: the same ciphertexts under ring_ref.identity_key.
EDGE_KS = [("W15", 3), ("W15", 1), ("W16", 2), ("X12", 2), ("X15", 2), ("L19", 16), ("P14", 9), ("P14", 4), ("R21", 17), ("R21", 9), ("R38", 33), ("V12", 2), ("V12", 0),
           ("A48", 0)]
EDGE_MODDOWN = [("W15", 3), ("X12", 2), ("R21", 17), ("R38", 33), ("A48", 0)]
EDGE_RESCALE = [("V12", 2), ("V12", 1), ("R21", 17), ("M48", 46)]


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
