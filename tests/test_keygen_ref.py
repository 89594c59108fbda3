"""Pins tests/keygen_ref.py (CPU only): on a tiny ring the aggregated keys of 2 and 3 parties satisfy the key equations EXACTLY with the noise the algebra predicts
from the transcripts, and the common-reference map equals a literal loop, the t + 1 path included."""
import os
import re

import numpy as np
import pytest

import encrypt_ref as er
import keygen_ref as kr

LOGN, N = 4, 16
Q_TINY, P_TINY = [97, 193, 257], [353]                 # all == 1 mod 2N = 32; nq = 3, np = 1: beta = 3


@pytest.fixture(scope="module")
def ring():
    return er.TinyRing(LOGN, Q_TINY, P_TINY)


def party_material(rnd, ring, nparty):
    beta = kr.beta_of(ring)
    return [dict(s=rnd.integers(-1, 2, N), u=rnd.integers(-1, 2, N), e=rnd.integers(-19, 20, N), ert=rnd.integers(-19, 20, (beta, N)),
                 e0=rnd.integers(-19, 20, (beta, N)), e1=rnd.integers(-19, 20, (beta, N)), e2=rnd.integers(-19, 20, (beta, N)), e3=rnd.integers(-19, 20, (beta, N)))
            for _ in range(nparty)]


def uniform_rows(rnd, ring, lead):
    return np.array([[[int(rnd.integers(0, q)) for _ in range(N)] for q in ring.moduli] for _ in range(lead)], dtype=object)


def poly_sum(polys):
    return [sum(int(p[c]) for p in polys) for c in range(N)]


@pytest.mark.parametrize("nparty", [2, 3])
def test_public_key_equation(ring, nparty):
    rnd = np.random.default_rng(100 + nparty)
    parties = party_material(rnd, ring, nparty)
    crp = uniform_rows(rnd, ring, 1)[0]
    pk0 = kr.aggregate(ring, [kr.ckg_share(ring, p["s"], crp, p["e"]) for p in parties])
    S, E = poly_sum([p["s"] for p in parties]), poly_sum([p["e"] for p in parties])
    Sh, Eh = kr.rows_of(ring, S), kr.rows_of(ring, E)
    for m, q in enumerate(ring.moduli):
        assert np.array_equal((pk0[m] + crp[m] * Sh[m]) % q, Eh[m]), m                   # pk0 + pk1 S = NTT(sum e)


@pytest.mark.parametrize("nparty", [2, 3])
@pytest.mark.parametrize("g", [5, 3, 2 * N - 1, pow(5, N // 4, 2 * N)])                        # rotation by 1, a non-power element, the conjugate, the rotation by slots / 2
def test_rotation_key_equation(ring, nparty, g):
    rnd = np.random.default_rng(200 + nparty)
    parties = party_material(rnd, ring, nparty)
    beta = kr.beta_of(ring)
    crp = uniform_rows(rnd, ring, beta)
    b = kr.aggregate(ring, [kr.rtg_share(ring, p["s"], g, crp, p["ert"]) for p in parties])
    S = poly_sum([p["s"] for p in parties])
    Sh, Sg = kr.rows_of(ring, S), kr.rows_of(ring, kr.automorphism(S, kr.galois_inverse(g, N), N))
    assert kr.automorphism(kr.automorphism(S, g, N), kr.galois_inverse(g, N), N) == S
    for i in range(beta):
        Eh = kr.rows_of(ring, poly_sum([p["ert"][i] for p in parties]))
        for m, q in enumerate(ring.moduli):
            gi = kr.g_term(ring, i, m)
            assert (gi != 0) == (m == i)                                                  # np = 1: digit i is modulus i
            assert np.array_equal((b[i][m] + crp[i][m] * Sg[m] - gi * Sh[m]) % q, Eh[m]), (i, m)


@pytest.mark.parametrize("nparty", [2, 3])
def test_relinearisation_key_equation(ring, nparty):
    """b_i + a_i S - g_i S^2 = S E0_i + U E1_i + E2_i + E3_i  (capitals: sums over the parties; a_i = H1agg_i = S crp_i + E1_i)"""
    rnd = np.random.default_rng(300 + nparty)
    parties = party_material(rnd, ring, nparty)
    beta = kr.beta_of(ring)
    crp = uniform_rows(rnd, ring, beta)
    r1 = [kr.rkg_round1(ring, p["s"], crp, p["u"], p["e0"], p["e1"]) for p in parties]
    H0, H1 = kr.aggregate(ring, [x[0] for x in r1]), kr.aggregate(ring, [x[1] for x in r1])
    b = kr.aggregate(ring, [kr.rkg_round2(ring, p["s"], H0, H1, p["u"], p["e2"], p["e3"]) for p in parties])
    S, U = poly_sum([p["s"] for p in parties]), poly_sum([p["u"] for p in parties])
    Sh = kr.rows_of(ring, S)
    for i in range(beta):
        E = [poly_sum([p[k][i] for p in parties]) for k in ("e0", "e1", "e2", "e3")]
        noise = [x + y + z + w for x, y, z, w in zip(er.negacyclic(S, E[0]), er.negacyclic(U, E[1]), E[2], E[3])]
        assert max(abs(x) for x in noise) <= nparty * nparty * 19 * 2 * N + 2 * nparty * 19
        Nh = kr.rows_of(ring, noise)
        for m, q in enumerate(ring.moduli):
            gi = kr.g_term(ring, i, m)
            assert np.array_equal((b[i][m] + H1[i][m] * Sh[m] - gi * Sh[m] * Sh[m]) % q, Nh[m]), (i, m)


def test_g_term_of_a_ragged_digit():
    class R:                                        # nq = 3, np = 2: beta = 2, the last digit holds one modulus
        nq, np_, moduli = 3, 2, [97, 193, 257, 353, 449]
    assert kr.beta_of(R) == 2
    P = 353 * 449
    assert [[kr.g_term(R, i, m) for m in range(5)] for i in range(2)] == [[P % 97, P % 193, 0, 0, 0], [0, 0, P % 257, 0, 0]]


# ---------------------------------------------------------------- the common reference map against a literal loop
def crp_literal(key32, row, q, j):
    bits = int(q).bit_length()
    t = 0
    while True:
        w = [int(x) for x in er.chacha20_blocks(key32, [j], (row & 0xFFFFFFFF, row >> 32, t))[0]]
        for k in range(8):
            cand = (w[2 * k] | (w[2 * k + 1] << 32)) & ((1 << bits) - 1)
            if cand < q:
                return cand, t
        t += 1


Q_ABOVE_POW2 = 0x800280001          # 2^35 + 2621441: 36 bits, a candidate is accepted with probability 0.50004, a try fails with 2^-8
CRP_ROW = (1 << 32) + 5             # a row number wider than 32 bits; under the test key its coefficient 6 needs a second try


def test_crp_map_against_a_literal_loop_including_the_retry_path():
    key = er.TEST_KEY
    got, tries = kr.crp_row(key, CRP_ROW, Q_ABOVE_POW2, 100, want_tries=True)
    lit = [crp_literal(key, CRP_ROW, Q_ABOVE_POW2, j) for j in range(100)]
    assert [int(x) for x in got] == [v for v, _ in lit] and [int(t) for t in tries] == [t for _, t in lit]
    assert max(t for _, t in lit) >= 1, "the t + 1 path is not reached in the first hundred coefficients: choose another row"
    assert got.max() < Q_ABOVE_POW2
    # a modulus just below a power of two (almost nothing rejected) and a tiny one
    for q, row in ((0x7fff80001, 0), (97, 7)):
        got = kr.crp_row(key, row, q, 40)
        assert [int(x) for x in got] == [crp_literal(key, row, q, j)[0] for j in range(40)]
    # rows and keys matter; a row does not depend on how many coefficients are asked for
    assert not np.array_equal(kr.crp_row(key, 0, Q_ABOVE_POW2, 64), kr.crp_row(key, 1, Q_ABOVE_POW2, 64))
    assert not np.array_equal(kr.crp_row(key, 0, Q_ABOVE_POW2, 64), kr.crp_row(bytes(32), 0, Q_ABOVE_POW2, 64))
    assert np.array_equal(kr.crp_row(key, 5, Q_ABOVE_POW2, 64)[:16], kr.crp_row(key, 5, Q_ABOVE_POW2, 16))
    rows = kr.crp_rows(key, 9, [1, 0], [97, Q_ABOVE_POW2], 32)
    assert np.array_equal(rows[0], kr.crp_row(key, 9, Q_ABOVE_POW2, 32)) and np.array_equal(rows[1], kr.crp_row(key, 10, 97, 32))


def test_the_shared_sampler_header_holds_the_documented_gaussian_table():
    """the sampler moved into a header both encrypt.hip and keygen.hip compile: its table is the one tests/encrypt_ref.py derives, entry by entry and in order"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = open(os.path.join(root, "sfgwas_amd", "csrc", "sampler.hpp")).read()
    body = txt[txt.index("ENC_GAUSS_CUM[20] = {"):]
    body = body[:body.index("};")]
    assert [int(h, 16) for h in re.findall(r"0x([0-9a-fA-F]{16})ULL", body)] == er.GAUSS_CUM
