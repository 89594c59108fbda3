"""Test-side reference of the baby-step rotation cache as an object (sfg_rotcache_*, include/sfgwas_hip.h): the MAC's fp64 operand form of a ciphertext
and the addressing of the cache and of the job-major staging buffer, in Python integers.  Nothing here loads the library or the oracle.

The operand form (mm_plan.hpp ModSplit, mac_dma.hip k_rot_to_f64, rotate.hip store_rot_f64): of a ciphertext [2][nl][N] the first L moduli are kept.  A modulus
>= 2^36 is big and takes two planes of N doubles, a smaller one takes one; plane_of is the running plane count and rowf = planes * N doubles hold one polynomial.
  * small modulus: the word w - or, where the product centres its small words (it does whenever the L moduli include a small one, under the default
    configuration), w - q for w > q >> 1: the representative in (-q/2, q/2];
  * big modulus: wc = w - q for w > q >> 1, else w; lo = ((wc + 2^22) mod 2^23) - 2^22, hi = (wc - lo) >> 23; {lo, hi} interleaved per coefficient.  The MAC's
    exactness bound rests on |lo| <= 2^22 and |hi| <= (q >> 24) + 1.

The cache of block rows [row0, row0 + nrows):  cache[bi - row0][baby < 91][i < s][poly < 2][rowf], then 3 * s * 2 * rowf zero doubles (the k-slices a ragged last
MAC chunk reads).  The staging buffer of jobs [job0, job1):  staged[job - job0][baby][poly][rowf], job = bi * s + i."""
import numpy as np

D = 91
BIG = 1 << 36
HALF, BASE = 1 << 22, 1 << 23


class ModSplit:
    """mm_plan.hpp ModSplit of the first L of `moduli`"""

    def __init__(self, moduli, L):
        self.L, self.q = L, [int(q) for q in moduli[:L]]
        assert len(self.q) == L and all(q < 1 << 47 for q in self.q)
        self.is_big = [q >= BIG for q in self.q]
        self.plane_of, planes = [], 0
        for big in self.is_big:
            self.plane_of.append(planes)
            planes += 2 if big else 1
        self.planes = planes
        self.centre = not all(self.is_big)              # mac_dma_packed_mask != 0 under the default configuration


def layout(moduli, L, s, n):
    """(rowf, job_doubles, tail_doubles) of sfg_rotcache_layout"""
    rowf = ModSplit(moduli, L).planes * n
    return rowf, D * 2 * rowf, 3 * s * 2 * rowf


# ---------------------------------------------------------------- one word, Python integers
def encode_word(w, q, big, centre):
    """the doubles of the canonical word w of modulus q, as exact integers: (v,) for a small modulus, (lo, hi) for a big one"""
    assert 0 <= w < q
    if not big:
        return (w - q if centre and w > q >> 1 else w,)
    wc = w - q if w > q >> 1 else w
    lo = (wc + HALF) % BASE - HALF
    return (lo, (wc - lo) >> 23)


def decode_word(vals, q, big):
    return (vals[1] * BASE + vals[0]) % q if big else vals[0] % q


# ---------------------------------------------------------------- rows, numpy (every intermediate below 2^47: exact in int64 and in float64)
def encode_rows(words, moduli, L):
    """words [2][nl >= L][N] uint64 canonical -> float64 [2][rowf]"""
    m = ModSplit(moduli, L)
    words = np.asarray(words)
    n = words.shape[-1]
    out = np.zeros((2, m.planes * n), dtype=np.float64)
    for l in range(L):
        q, w = m.q[l], words[:, l, :].astype(np.int64)
        o = out[:, m.plane_of[l] * n:(m.plane_of[l] + (2 if m.is_big[l] else 1)) * n]
        if m.is_big[l]:
            wc = np.where(w > q >> 1, w - q, w)
            lo = (wc + HALF) % BASE - HALF
            o[:, 0::2] = lo
            o[:, 1::2] = (wc - lo) >> 23
        else:
            o[:] = np.where(w > q >> 1, w - q, w) if m.centre else w
    return out


def decode_rows(rows, moduli, L):
    """the inverse: float64 [2][rowf] -> uint64 [2][L][N]"""
    m = ModSplit(moduli, L)
    rows = np.asarray(rows)
    n = rows.shape[-1] // m.planes
    assert np.array_equal(rows, np.rint(rows))
    r = rows.astype(np.int64)
    out = np.zeros((2, L, n), dtype=np.uint64)
    for l in range(L):
        q, p = m.q[l], r[:, m.plane_of[l] * n:(m.plane_of[l] + (2 if m.is_big[l] else 1)) * n]
        out[:, l, :] = ((p[:, 1::2] * BASE + p[:, 0::2]) % q if m.is_big[l] else p % q).astype(np.uint64)
    return out


def boundary_words(q):
    """canonical words on the branch boundaries of the form: the centring boundary and, for a big modulus, the signed 23-bit split"""
    ws = [0, 1, q >> 1, (q >> 1) + 1, q - 1]
    if q >= BIG:
        top = q >> 24
        cs = [HALF - 1, HALF, HALF + 1] + [k * BASE + e for k in (1, 2, 3, top - 1) for e in (-HALF - 1, -HALF, -HALF + 1, HALF - 1, HALF, HALF + 1)]
        ws += [c % q for c in cs if c <= q >> 1] + [-c % q for c in cs if c <= q >> 1]
    return ws


# ---------------------------------------------------------------- addressing
def job_of(bi, i, s):
    return bi * s + i


def cache_view(flat, nrows, s, rowf):
    """(cache [nrows][91][s][2][rowf], tail [3 * s * 2 * rowf], whatever follows) of a flat array"""
    body, tail = nrows * D * s * 2 * rowf, 3 * s * 2 * rowf
    return flat[:body].reshape(nrows, D, s, 2, rowf), flat[body:body + tail], flat[body + tail:]


def staged_view(flat, njobs, rowf):
    """(staged [njobs][91][2][rowf], whatever follows)"""
    body = njobs * D * 2 * rowf
    return flat[:body].reshape(njobs, D, 2, rowf), flat[body:]


def scatter(staged, job0, job1, row0, nrows, s, cache):
    """sfg_rotcache_scatter_dev on host views: staged [job1 - job0][91][2][rowf] into cache [nrows][91][s][2][rowf]"""
    assert row0 * s <= job0 <= job1 <= (row0 + nrows) * s
    for job in range(job0, job1):
        cache[job // s - row0, :, job % s] = staged[job - job0]
