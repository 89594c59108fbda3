"""tests/rotcache_ref.py against itself and against the bounds the MAC's exactness rests on, for every modulus of PN14QP438 and of the chains S1, S3 and S4:
decode(encode(w)) == w, |lo| <= 2^22, |hi| <= (q >> 24) + 1, centred small words in (-q/2, q/2] - on the centring boundary, on the signed 23-bit split and on
random words; the vectorised rows equal the word-by-word form; the layout arithmetic of sfg_rotcache_layout for L = 1 .. nq.  No GPU, no library."""
import math

import numpy as np
import pytest

import rotcache_ref as rr
from sfgwas_amd.params import P_PN14, Q_PN14
from test_ksw_split import S1, S3, S4

CHAINS = {"PN14": (Q_PN14, P_PN14), "S1": S1, "S3": S3, "S4": S4}
MODULI = sorted({q for qs, ps in CHAINS.values() for q in qs + ps})
N = 256


def words_of(q, rnd, count=2000):
    return rr.boundary_words(q) + [int(x) for x in rnd.integers(0, q, count)]


@pytest.mark.parametrize("q", MODULI, ids=hex)
def test_word_round_trip_and_bounds(q):
    rnd = np.random.default_rng(q % 1000003)
    big = q >= rr.BIG
    bw = rr.boundary_words(q)
    assert {0, 1, q >> 1, (q >> 1) + 1, q - 1} <= set(bw) and all(0 <= w < q for w in bw)
    los = set()
    for w in words_of(q, rnd):
        for centre in (True, False):
            v = rr.encode_word(w, q, big, centre)
            assert rr.decode_word(v, q, big) == w
            assert all(float(x) == x for x in v)                       # every stored double is the integer itself
            if big:
                lo, hi = v
                assert abs(lo) <= rr.HALF and abs(hi) <= (q >> 24) + 1
                assert -rr.HALF <= lo < rr.HALF                        # the split is the half-open one: + 2^22 belongs to the next hi
                los.add(lo)
            elif centre:
                assert -q < 2 * v[0] <= q
            else:
                assert v[0] == w
    if big:
        assert {-rr.HALF, -rr.HALF + 1, rr.HALF - 1, 0, 1, -1} <= los          # the directed words reach both ends of the split


def fp64_floor_form(w, q, big, centre):
    """rotate.hip store_rot_f64 restated in IEEE doubles (Python floats): the encoder of baby steps 1 to 90"""
    v, qf = float(w), float(q)
    if big:
        wc = v - qf if v > math.floor(qf * 0.5) else v
        hi = math.floor((wc + 4194304.0) * 2.0 ** -23)
        return (wc - hi * 8388608.0, float(hi))
    return (v - qf if centre and v > math.floor(qf * 0.5) else v,)


@pytest.mark.parametrize("q", MODULI, ids=hex)
def test_the_fp64_floor_form_is_the_integer_form(q):
    """the two encoders of the library compute the form with integers (baby step 0) and with fp64 floors (the key switch's finish): one statement of each, equal
    on every directed and random word, signed zeros included"""
    rnd = np.random.default_rng(q % 999983)
    big = q >= rr.BIG
    for w in words_of(q, rnd):
        for centre in (True, False):
            a, b = rr.encode_word(w, q, big, centre), fp64_floor_form(w, q, big, centre)
            assert tuple(float(x) for x in a) == b and not any(math.copysign(1.0, x) < 0 and x == 0 for x in b), (w, a, b)


@pytest.mark.parametrize("name", sorted(CHAINS))
def test_rows_round_trip_and_equal_the_word_form(name):
    q = CHAINS[name][0]
    rnd = np.random.default_rng(len(name) + q[0] % 97)
    for L in range(1, len(q) + 1):
        m = rr.ModSplit(q, L)
        assert m.planes == sum(2 if x >= rr.BIG else 1 for x in q[:L]) and m.centre == any(x < rr.BIG for x in q[:L])
        assert m.plane_of == [sum(2 if x >= rr.BIG else 1 for x in q[:l]) for l in range(L)]
        nl = min(L + 1, len(q))
        words = np.zeros((2, nl, N), dtype=np.uint64)
        for l in range(nl):
            bw = rr.boundary_words(q[l])
            col = (bw * (N // len(bw) + 1))[:N // 2] + [int(x) for x in rnd.integers(0, q[l], N - N // 2)]
            words[0, l], words[1, l] = col, col[::-1]
        rows = rr.encode_rows(words, q, L)
        assert rows.shape == (2, m.planes * N) and rows.dtype == np.float64
        assert np.array_equal(rr.decode_rows(rows, q, L), words[:, :L])
        for p in range(2):
            for l in range(L):
                for x in range(N):
                    v = rr.encode_word(int(words[p, l, x]), q[l], m.is_big[l], m.centre)
                    o = m.plane_of[l] * N
                    got = (rows[p, o + 2 * x], rows[p, o + 2 * x + 1]) if m.is_big[l] else (rows[p, o + x],)
                    assert got == v


@pytest.mark.parametrize("name", sorted(CHAINS))
def test_layout_arithmetic(name):
    q = CHAINS[name][0]
    n = 1 << 14
    for L in range(1, len(q) + 1):
        for s in (1, 2, 16, 33):
            rowf, jobw, tailw = rr.layout(q, L, s, n)
            assert rowf == rr.ModSplit(q, L).planes * n and jobw == 91 * 2 * rowf and tailw == 3 * s * 2 * rowf


def test_addressing_views_and_scatter():
    """cache[bi - row0][baby][i][poly][rowf] and staged[job - job0][baby][poly][rowf] with job = bi * s + i, on labelled doubles"""
    s, nrows, row0, rowf = 3, 2, 1, 4
    body = nrows * rr.D * s * 2 * rowf
    flat = np.arange(body + 3 * s * 2 * rowf + 5, dtype=np.float64)
    cache, tail, rest = rr.cache_view(flat, nrows, s, rowf)
    assert tail.size == 3 * s * 2 * rowf and rest.size == 5 and tail[0] == body
    bi, baby, i, poly = 2, 17, 1, 1
    assert cache[bi - row0, baby, i, poly, 0] == ((((bi - row0) * rr.D + baby) * s + i) * 2 + poly) * rowf
    job0, job1 = 4, 9                                                   # (bi 1, i 1) .. (bi 2, i 2)
    sflat = -np.arange(1, (job1 - job0) * rr.D * 2 * rowf + 1, dtype=np.float64)
    staged, srest = rr.staged_view(sflat, job1 - job0, rowf)
    assert srest.size == 0 and staged[2, 5, 1, 3] == -(((2 * rr.D + 5) * 2 + 1) * rowf + 3 + 1)
    before = cache.copy()
    rr.scatter(staged, job0, job1, row0, nrows, s, cache)
    for job in range(row0 * s, (row0 + nrows) * s):
        b, k = job // s - row0, job % s
        assert rr.job_of(job // s, k, s) == job
        if job0 <= job < job1:
            assert np.array_equal(cache[b, :, k], staged[job - job0])
        else:
            assert np.array_equal(cache[b, :, k], before[b, :, k])     # a slot of a job outside the range keeps what it held
