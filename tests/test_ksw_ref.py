"""CPU side of the key-switch pinning beyond PN14 (tests/ksw_ref.py): the chains' stated properties, the oracle's basis extension against
Python integers at one to four primes per digit, the classes the directed inputs reach, and what the oracle's key switch MEANS at
alpha = 1, 3 and 4 (the GPU files only compare the device with it)."""
import numpy as np
import pytest

import ksw_ref as kr
import oracle_lib as ol
import pyref


# ---------------------------------------------------------------- the chains
@pytest.mark.parametrize("name", sorted(kr.CHAINS))
def test_chain_moduli_are_ntt_primes_with_arm_moduli_in_front(name):
    from sympy import isprime
    q, p, levels = kr.CHAINS[name]
    assert len(q) + len(p) <= 16 and len(set(q + p)) == len(q + p)
    for m in q + p:
        assert isprime(m) and m % (1 << 15) == 1 and m < 1 << 47, hex(m)
    assert [i for i, m in enumerate(q) if kr.ARM(m)] == kr.ARM_INDICES[name]
    assert not any(kr.ARM(m) for m in p)
    assert max(levels) < len(q)


def test_arm_moduli_of_pn14_and_of_the_top_of_the_range():
    """canon()'s fix-up is reachable for exactly one PN14 modulus (index 7, above the levels the rotation tests use) and for few of the
    largest 47-bit NTT primes - S4 starts with the first two of them and fills up with primes that lack the property"""
    assert [i for i, m in enumerate(ol.Q_PN14 + ol.P_PN14) if kr.ARM(m)] == [7]
    top = ol.small_primes(14, 47, 16)
    assert [hex(m) for m in top if kr.ARM(m)][:2] == ["0x7fffffda0001", "0x7fffffc48001"]
    assert sum(kr.ARM(m) for m in top) <= 4 and set(kr.S4[0] + kr.S4[1]) <= set(ol.small_primes(14, 47, 24))


def test_canon_model_and_where_its_fixup_matters():
    """canon() is x mod q on every modulus of the chains and of PN14 at the multiples of q and beside them.  Without the fix-up (canon_le) it
    returns q instead of 0, at multiples k q only: at k = 1 exactly for the ARM moduli; at other k - negative ones too, where the rounded
    product falls below k when fl(1/q) is too LARGE - for some non-ARM moduli as well (0x7ffc80001 of PN14 is one).  A word that is q instead of
    0 is absorbed by the next canon() it meets (canon(d + q) == canon(d)): only a LAST canon() without the fix-up shows."""
    needs = {}
    for q in sorted(set(sum((c[0] + c[1] for c in kr.CHAINS.values()), [])) | set(ol.Q_PN14 + ol.P_PN14)):
        wrong = []
        for k in list(range(-15, 16)) + [(1 << 50) // q]:
            for e in (-1, 0, 1, q // 2):
                x = k * q + e
                assert kr.canon_model(x, q) == x % q, (hex(q), k, e)
                if kr.canon_model(x, q, fixup=False) != x % q:
                    assert e == 0 and k != 0 and kr.canon_model(x, q, fixup=False) == q
                    wrong.append(k)
        assert (1 in wrong) == kr.ARM(q), (hex(q), wrong)
        if wrong:
            needs[q] = wrong
    assert 0x7ffc80001 in needs and max(needs[0x7ffc80001]) < 0 and not kr.ARM(0x7ffc80001)
    assert all(k > 0 for q, w in needs.items() if kr.ARM(q) for k in w)


def test_chain_shapes_reach_the_key_switch_limits():
    q, p, _ = kr.S1
    assert len(kr.digits(7, len(p))) == 8 and len(kr.digits(8, len(p))) == 9                 # KSW_MAXDIG and one beyond
    assert [len(d) for d in kr.digits(6, 3)] == [3, 3, 1] and [len(d) for d in kr.digits(4, 3)] == [3, 2]
    assert [len(d) for d in kr.digits(7, 4)] == [4, 4] and [len(d) for d in kr.digits(5, 4)] == [4, 2]


# ---------------------------------------------------------------- the float correction: classes of the directed words
NEG_DIGITS = {("S3", 6, 0), ("S3", 6, 1), ("S3", 4, 0), ("S4", 7, 0), ("S4", 7, 1), ("S4", 5, 0), ("S4", 2, 0)}


@pytest.mark.parametrize("name", sorted(kr.CHAINS))
def test_directed_words_reach_every_class_of_the_float_correction(name):
    """v_float - v_exact over the directed words: +1 and 0 on every multi-prime digit, -1 on the digits of NEG_DIGITS - which are all the
    digits where ANY word 1..199 undershoots (searched here), so no reachable class is left out"""
    q, p, levels = kr.CHAINS[name]
    multi = 0
    for level in levels:
        for i, cls in enumerate(kr.classify(q, len(p), level)):
            if cls is None:
                continue
            multi += 1
            seen = set(cls.values())
            assert seen <= {-1, 0, 1} and {0, 1} <= seen, (name, level, i, seen)
            qs = [q[m] for m in kr.digits(level, len(p))[i]]
            under = [x for x in range(1, 200) if (lambda r: r[1] < r[2])(kr.ext_model([x % m for m in qs], qs))]
            assert (-1 in seen) == ((name, level, i) in NEG_DIGITS) == bool(under), (name, level, i, under[:4])
    assert multi == {"S1": 0, "S3": 5, "S4": 5}[name]          # S1's digits are single primes: a raw copy, no correction


@pytest.mark.parametrize("name", ["S3", "S4"])
def test_reciprocal_in_place_of_division_changes_a_directed_word(name):
    """y * fl(1/q) in place of y / q moves v on directed words of S3 and S4 - and v enters every target as v * D, D != 0 mod q_t - so the GPU
    parity on the directed ciphertext sees that mistake.  S1 has no float correction to get wrong (previous test)."""
    q, p, levels = kr.CHAINS[name]
    changed = 0
    for level in levels:
        a, b = kr.classify(q, len(p), level), kr.classify(q, len(p), level, recip=True)
        changed += sum(ca[k] != cb[k] for ca, cb in zip(a, b) if ca is not None for k in ca)
    assert changed >= 4, changed


def test_random_words_stay_in_class_zero():
    """why the directed words are needed: none of 2000 uniformly random digit words leaves class 0"""
    import random
    rnd = random.Random(5)
    q = kr.S4[0]
    qs = q[:4]
    for _ in range(2000):
        _, vf, ve = kr.ext_model([rnd.randrange(m) for m in qs], qs)
        assert vf == ve


# ---------------------------------------------------------------- the oracle's extension against Python integers, a = 1..4
@pytest.mark.parametrize("alpha", [1, 2, 3, 4])
def test_oracle_keyswitch_is_the_integer_model_on_a_tiny_ring(alpha):
    """orc_keyswitch == keyswitch_model (Python integers, the float v restated) on logN = 4, digits of alpha, alpha and 1 primes, 35- and
    47-bit moduli mixed, on directed words (every class) and random ones"""
    big, small = ol.small_primes(4, 47, 2 * alpha + 2), ol.small_primes(4, 35, alpha + 1)
    q = [(big if m % 2 else small)[m // 2] for m in range(2 * alpha + 1)]
    p = big[alpha + 1:2 * alpha + 1]
    ring = ol.Ring(4, q, p)
    level = len(q) - 1
    from sfgwas_amd import capi
    key = capi.random_rotkey(ring.moduli, ring.beta, ring.N, 9)
    vals = kr.directed_values(q, alpha, level)
    seen = set()
    for cls in kr.classify(q, alpha, level):
        seen |= set(cls.values()) if cls else set()
    assert alpha == 1 or {0, 1} <= seen
    inputs = [kr.directed_rows(q, vals, ring.N, shift) for shift in range(0, len(vals), ring.N)]
    inputs.append(ring.fill_uniform(level, 3)[1])
    for rows in inputs:
        cx = np.stack([ring.ntt(m, rows[m]) for m in range(level + 1)])
        d0, d1 = np.zeros_like(cx), np.zeros_like(cx)
        ol.lib().orc_keyswitch(ring.h, level, ol.p64(cx), ol.p64(key), ol.p64(d0), ol.p64(d1))
        w0, w1 = kr.keyswitch_model(ring, level, cx, key)
        assert np.array_equal(d0, w0) and np.array_equal(d1, w1)


# ---------------------------------------------------------------- what the oracle's key switch means at alpha = 1, 3, 4
def _centered(v, q0):
    return np.array([int(x) - q0 if int(x) > q0 // 2 else int(x) for x in v])


@pytest.mark.parametrize("name", sorted(kr.CHAINS))
def test_oracle_rotation_and_conjugation_decrypt_to_the_permuted_message(name):
    """a rotation (X -> X^(5^3)) and the conjugation (X -> X^(2N-1)) under valid keys from the oracle's generator, N = 16384, at the top level
    and at level 1: the decryption is the message under the automorphism up to key-switch noise.  Measured largest coefficient error:
    S1 221 (top) / 219 (level 1), S3 239 / 218, S4 776 / 234 - below 2^10; the bound allows three more bits."""
    q, p, _ = kr.CHAINS[name]
    ring = ol.Ring(14, q, p)
    s = ring.gen_secret(5)
    keys = ol.RotKeys(ring)
    elements = [ring.galois(3), 2 * ring.N - 1]
    for g in elements:
        keys.add(g, ring.gen_rotkey(s, g, 1 + g))
    m = np.random.default_rng(2).integers(-(1 << 20), 1 << 20, ring.N)
    q0 = q[0]
    for level in (len(q) - 1, 1):
        ct = ring.encrypt(s, level, m, 31)
        for g in elements:
            out = np.zeros_like(ct)
            assert ol.lib().orc_apply_galois(ring.h, keys.h, level, ol.p64(ct), g, ol.p64(out)) == 0
            dec = _centered(ring.decrypt_residues(s, level, out)[0], q0)
            want = _centered(pyref.automorphism_coeffs([int(x) % q0 for x in m], g, q0), q0)
            noise = int(np.max(np.abs(dec - want)))
            print(f"{name} level {level} galois {g}: noise {noise}")
            assert noise < 1 << 13, (name, level, g, noise)
