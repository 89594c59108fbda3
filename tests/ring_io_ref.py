"""Test-side statements of the general ring's two ends (sfgwas_amd/csrc/gring_io.hip) that do not exist elsewhere:

  * the sampler's map at general N, in numpy on encrypt_ref.chacha20_blocks (at N = 16384 it must be encrypt_ref.sample_u / sample_e: tests/test_ring_io_ref.py);
  * a key pair for any ring of the tests, ring_ref.SplitRing included, and the secret key's NTT-domain rows;
  * the collective decryption's share, stated through encrypt_ref.encrypt_bigint with the zero public key;
  * the decoder's coefficients: the centred CRT, mixed-radix digits, the exact quotient by the scale as a Fraction, its correct rounding and its distance from a
    rounding boundary, and the directed coefficients of a chain.
"""
import numpy as np

import encrypt_ref as er


# ---------------------------------------------------------------- the sampler at general N: coefficient j = 512 a + t, t < 512, a < N / 512
def sample_u(key32, index, N):
    """block (t >> 3) + 64 (a >> 5) of polynomial 0, r = w[2 (t & 7)] | w[2 (t & 7) + 1] << 32, bits 2 (a & 31), 2 (a & 31) + 1 = (b0, b1): b0 ? (b1 ? -1 : 1) : 0"""
    nblk = 64 * ((N // 512 + 31) // 32)
    W = er.chacha20_blocks(key32, np.arange(nblk), er.nonce_of(index, 0)).astype(np.uint64)
    j = np.arange(N); a, t = j >> 9, j & 511
    blk = (t >> 3) + 64 * (a >> 5)
    r = W[blk, 2 * (t & 7)] | (W[blk, 2 * (t & 7) + 1] << np.uint64(32))
    two = (r >> (2 * (a & 31)).astype(np.uint64)) & np.uint64(3)
    return np.where(two & np.uint64(1), np.where(two & np.uint64(2), -1, 1), 0).astype(np.int8)


def sample_e(key32, index, poly, N):
    """block t + 512 (a >> 3) of polynomial `poly`, word pair a & 7, through the committed table"""
    W = er.chacha20_blocks(key32, np.arange(512 * (N // 4096)), er.nonce_of(index, poly)).astype(np.uint64)
    j = np.arange(N); a, t = j >> 9, j & 511
    blk, k = t + 512 * (a >> 3), a & 7
    r = W[blk, 2 * k] | (W[blk, 2 * k + 1] << np.uint64(32))
    mag = np.searchsorted(np.array(er.GAUSS_CUM, dtype=np.uint64), r >> np.uint64(1), side="right").astype(np.int32)
    return np.where(r & np.uint64(1), -mag, mag).astype(np.int32)


def transcript(key32, first_index, nct, N):
    idx = [first_index + i for i in range(nct)]
    return (np.stack([sample_u(key32, i, N) for i in idx]), np.stack([sample_e(key32, i, 1, N) for i in idx]), np.stack([sample_e(key32, i, 2, N) for i in idx]))


def sample_one_literal(key32, index, poly, j):
    """coefficient j of polynomial `poly` (0 = u) by a literal walk of the map: one block, one word pair, one shift (N does not enter: the map has no wrap)"""
    a, t = j >> 9, j & 511
    if poly == 0:
        w = [int(x) for x in er.chacha20_blocks(key32, [(t >> 3) + 64 * (a >> 5)], er.nonce_of(index, 0))[0]]
        r = w[2 * (t & 7)] | (w[2 * (t & 7) + 1] << 32)
        b0, b1 = (r >> (2 * (a & 31))) & 1, (r >> (2 * (a & 31) + 1)) & 1
        return (-1 if b1 else 1) if b0 else 0
    w = [int(x) for x in er.chacha20_blocks(key32, [t + 512 * (a >> 3)], er.nonce_of(index, poly))[0]]
    r = w[2 * (a & 7)] | (w[2 * (a & 7) + 1] << 32)
    mag = sum(1 for c in er.GAUSS_CUM if (r >> 1) >= c)
    return -mag if r & 1 else mag


# ---------------------------------------------------------------- keys
class _WithSecret:
    """a ring of the tests plus gen_secret, which encrypt_ref.make_keypair needs and ring_ref.SplitRing lacks: the secret of its first part (same N)"""

    def __init__(self, ring):
        self._ring = ring
        self.N, self.moduli = ring.N, ring.moduli

    def gen_secret(self, seed):
        r = self._ring
        return r.gen_secret(seed) if hasattr(r, "gen_secret") else r.parts[0][1].gen_secret(seed)

    def ntt(self, mod, a):
        return self._ring.ntt(mod, a)


def keypair(ring, seed):
    """-> (s int8 [N] ternary, pk uint64 [2][nq+np][N]) for oracle_lib.Ring and ring_ref.SplitRing alike"""
    return er.make_keypair(_WithSecret(ring), seed)


def sk_rows(ring, s, nrows=None):
    """the secret's NTT-domain rows [nq][N] (what sfg_ring_load_secret_key takes)"""
    nrows = ring.nq if nrows is None else nrows
    return np.stack([ring.ntt(m, np.array([int(x) % ring.moduli[m] for x in s], dtype=np.uint64)) for m in range(nrows)])


def split_secret(s, seed):
    """two additive ternary-free shares of s as small signed integers: s = s1 + s2 with s1 uniform in {-1, 0, 1}"""
    rnd = np.random.default_rng(seed)
    s1 = rnd.integers(-1, 2, len(s)).astype(np.int64)
    return s1, s.astype(np.int64) - s1


# ---------------------------------------------------------------- the share of the collective key switch (zero public key: u drops out)
def pcks_share_bigint(ring, level, sk_ntt, ct, e0, e1):
    """h0 = ModDown_P(NTT_QP(e0)) + sk (.) c1, h1 = ModDown_P(NTT_QP(e1)) -> uint64 [level+1][N] each; sk_ntt [>= level+1][N], ct [2][level+1][N]"""
    zero_pk = np.zeros((2, len(ring.moduli), ring.N), dtype=np.uint64)
    c = er.encrypt_bigint(ring, level, zero_pk, np.zeros(ring.N, dtype=np.int64), e0, e1)
    h0, h1 = np.zeros((level + 1, ring.N), dtype=np.uint64), np.zeros((level + 1, ring.N), dtype=np.uint64)
    for m in range(level + 1):
        q = ring.moduli[m]
        sc = np.array([int(a) * int(b) for a, b in zip(sk_ntt[m], ct[1, m])], dtype=object)
        h0[m] = ((c[m][0] + sc) % q).astype(np.uint64)
        h1[m] = (c[m][1] % q).astype(np.uint64)
    return h0, h1


def ct_rows(enc, level):
    """encrypt_bigint's {row: (c0, c1)} -> uint64 [2][level+1][N]"""
    return np.stack([np.stack([np.array(enc[m][p], dtype=np.uint64) for m in range(level + 1)]) for p in range(2)])


# ---------------------------------------------------------------- the decoder's coefficients: centred CRT, the exact quotient by the scale
from fractions import Fraction  # noqa: E402
from math import prod  # noqa: E402


def crt_centred(residues, moduli):
    """one coefficient: residues x_i mod q_i -> the integer in (-Q/2, Q/2] (lattigo: x.Cmp(QHalf) > 0 -> x - Q with QHalf = Q // 2)"""
    Q = prod(moduli)
    x = sum(int(r) * (Q // q) * pow(Q // q, -1, q) for r, q in zip(residues, moduli)) % Q
    return x - Q if x > Q // 2 else x


def mixed_radix(x, moduli):
    """digits d_i of 0 <= x < Q: x = sum d_i q_0 .. q_(i-1)"""
    out = []
    for q in moduli:
        out.append(x % q)
        x //= q
    assert x == 0
    return out


def quotient(p, scale):
    """the exact quotient of the integer p by the double `scale`, as a Fraction"""
    return Fraction(int(p)) / Fraction(float(scale))


def rounded(x):
    """a Fraction correctly rounded to double, ties to even (Python's integer true division rounds correctly); beyond the range: an infinity"""
    try:
        return x.numerator / x.denominator
    except OverflowError:
        return float("inf") if x > 0 else float("-inf")


def boundary_distance(x):
    """relative distance of the Fraction x != 0 from the nearest rounding boundary (the midpoint of two adjacent doubles)"""
    import math
    f = rounded(x)
    lo, hi = Fraction(math.nextafter(f, -math.inf)), Fraction(math.nextafter(f, math.inf))
    return min(abs(x - (Fraction(f) + lo) / 2), abs(x - (Fraction(f) + hi) / 2)) / abs(x)


DECODE_REL = Fraction(1, 1 << 96)      # gring_io_arith.hpp: kDecodeRel, derived there for up to 48 digits


def directed_coefficients(moduli):
    """signed integers in (-Q/2, Q/2] at the decoder's edges: 0, +-1, +-(2^62 - 1), Q/2 and its neighbours on both sides of the centring, a negative value whose
    complement's carry runs to the top digit (x = (q_top - 1) W_top: all lower digits 0), one whose carry stops at once, and both ends of the range"""
    Q = prod(moduli)
    h, Wtop = Q // 2, Q // moduli[-1]
    vals = [0, 1, -1, 2, -2, h, h - 1, -h, -h + 1, -Wtop, Wtop, -(Wtop - 1), -(Wtop + 1), moduli[0], -moduli[0], moduli[0] - 1, -(moduli[0] - 1)]
    vals += [v for v in ((1 << 62) - 1, -((1 << 62) - 1)) if -h <= v <= h]
    return [v for v in vals if -h <= v <= h]
