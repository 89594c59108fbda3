"""CPU side of the general ring's edge tests (tests/test_gpu_ring_edges.py): what holds the reference of tests/ring_ref.py before the device is compared with it.

  * the chains R21, R38, M48, A48, V12 of tests/ring_cases.py are what their table says, and SplitRing serves every modulus of them;
  * the hoisted, vectorised extend_rows equals ksw_ref.ext_model / ext_value (one word at a time, Fractions) on every digit shape of the new chains, mistakes included;
  * keyswitch and rescale_model equal the oracle where the oracle holds the chain;
  * COVERAGE, read from the model's trace: on every (chain, level) the GPU file runs, every multi-modulus digit has words of class v_float - v_exact = +1 and 0, every
    digit of four or more moduli also -1, and under identity_key ModDown's own sum has +1 and 0 in both planes;
  * DISCRIMINATION: each of three mistakes made in the MODEL changes the expected output of those runs, so a kernel that made it would fail the GPU file;
  * M48's planted input really drives the unreduced key sums past 2^125.
"""
from math import prod

import numpy as np
import pytest

import ksw_ref
import oracle_lib as ol
import ring_cases as rc
import ring_ref as rr

KEY_SEED, CT_SEED = rr.KEY_SEED, rr.CT_SEED   # the GPU file uses the same key and ciphertexts

# (chain, level) -> digits on which y * fl(1/q) in place of y / q moves v on a word of the directed cycle: the 50- and 55-bit digits, and the last digits of the
# 36- and 35-bit chains (L19's digit 5 through the word -7 that directed_values' search adds).  No 61-bit digit has such a word in its cycle, nor among
# |k| < 20000, so on X12, X15, R21, R38 and V12 only the other two mistakes are shown to be caught.
RECIP_DIGITS = {("W15", 3): [0], ("W16", 2): [0], ("L19", 16): [5, 6, 7], ("P14", 9): [3, 4]}


def classes_of(cls):
    return set(cls.tolist())


# ---------------------------------------------------------------- the chains and the ring that serves them
def test_edge_chains_are_what_their_table_says():
    from sympy import isprime
    shapes = {"R21": ([61] * 18, [61] * 3), "R38": ([61] * 34, [61] * 4), "M48": ([61] * 47, [61]), "A48": ([61], [61] * 47), "V12": ([30, 61, 45], [61, 61])}
    assert sorted(shapes) == sorted(rc.EDGE_NAMES) and not set(rc.EDGE_NAMES) & set(rc.NAMES)
    for name, (qb, pb) in shapes.items():
        logN, q, p = rc.chain(name)
        assert logN == 12 and [m.bit_length() for m in q] == qb and [m.bit_length() for m in p] == pb
        assert len(set(q + p)) == len(q + p) <= 48 and all(isprime(m) and m % 8192 == 1 for m in q + p)
    import ring_refresh_ref
    assert ring_refresh_ref.chain("M48") == rc.chain("M48")
    assert [len(d) for d in rc.digits(17, 3)] == [3] * 6 and [len(d) for d in rc.digits(9, 3)] == [3, 3, 3, 1]
    assert [len(d) for d in rc.digits(33, 4)] == [4] * 8 + [2] and [len(d) for d in rc.digits(46, 1)] == [1] * 47 and rc.digits(0, 47) == [[0]]
    _, q, _ = rc.chain("V12")
    assert q[1] > q[0] << 30 and q[1] > q[2] << 15            # the dropped or copied 61-bit word is up to 2^31 times its target


@pytest.mark.parametrize("name", ["L19", "R21", "R38", "M48", "A48"])
def test_split_ring_serves_every_modulus_with_the_oracles_transform(name):
    """groups of at most 15, none of one; every modulus transforms as it does in an oracle ring of its own, both ways"""
    logN, q, p = rc.chain(name)
    ring = rr.chain_ring(name)
    sizes = [len(r.moduli) for _, r in ring.parts]
    assert len(sizes) == -(-len(ring.moduli) // 15) and sum(sizes) == len(ring.moduli) and 2 <= min(sizes) and max(sizes) <= 15 and max(sizes) - min(sizes) <= 1
    assert sum((r.moduli for _, r in ring.parts), []) == ring.moduli
    rnd = np.random.default_rng(1)
    for m in sorted({0, len(ring.moduli) - 1} | {off + d for off, _ in ring.parts for d in (-1, 0) if off + d >= 0}):
        qm = ring.moduli[m]
        row = rnd.integers(0, qm, ring.N, dtype=np.uint64)
        own = ol.Ring(logN, [qm], [ring.moduli[m - 1]])
        assert np.array_equal(ring.ntt(m, row), own.ntt(0, row)) and np.array_equal(ring.intt(m, ring.ntt(m, row)), row), (name, m)


# ---------------------------------------------------------------- the hoisted extension against the word-by-word one
def digit_shapes():
    """(chain, moduli of the digit, two targets) for every distinct digit length of the new chains at the levels the GPU file runs, and their ModDown digit"""
    out = []
    for name, levels in (("R21", [17, 9]), ("R38", [33]), ("M48", [46]), ("A48", [0]), ("V12", [2, 0])):
        _, q, p = rc.chain(name)
        groups = [list(p)]
        for level in levels:
            digs = rc.digits(level, len(p))
            groups += [[q[m] for m in dg] for dg in (digs[0], digs[-1])]
        for qs in groups:
            others = [m for m in q + p if m not in qs]
            if (name, qs) not in [(n, g) for n, g, _ in out]:
                out.append((name, qs, [others[0], others[-1]]))
    return out


@pytest.mark.parametrize("name,qs,targets", digit_shapes(), ids=lambda v: v if isinstance(v, str) else str(len(v)))
def test_hoisted_extension_equals_the_word_by_word_model(name, qs, targets):
    """64 words: the boundary words X = k, D - k, D // 2, D // 2 + 1 and uniform ones; y, v_float, v_exact and the residue at two targets, and v under each mistake"""
    D = prod(qs)
    rnd = np.random.default_rng(len(qs))
    words = [k for k in ksw_ref.SMALL if abs(k) < D] + [D // 2, D // 2 + 1, D - 1, 37, -37, 199, -199]
    words = [w % D for w in words]
    while len(words) < 64:
        words.append(int.from_bytes(rnd.bytes(400), "little") % D)
    rows = [np.array([w % q for w in words], dtype=np.uint64) for q in qs]
    ext, cls = rr.extend_rows(rows, qs, targets, classes=True)
    if len(qs) == 1:
        assert cls is None and all(ext[qt].tolist() == [w % qt for w in words] for qt in targets)
        return
    wrong = {m: rr.extend_rows(rows, qs, targets, mistake=m) for m in rr.MISTAKES}
    for x, w in enumerate(words):
        xs = [w % q for q in qs]
        y, vf, ve = ksw_ref.ext_model(xs, qs)
        assert cls[x] == vf - ve
        v_wrong = {"recip": ksw_ref.ext_model(xs, qs, recip=True)[1], "round": int(sum_in_order(y, qs) + 0.5), "exact": ve}
        for qt in targets:
            assert int(ext[qt][x]) == ksw_ref.ext_value(y, vf, qs, qt), (name, len(qs), x)
            for m in rr.MISTAKES:
                assert int(wrong[m][qt][x]) == ksw_ref.ext_value(y, v_wrong[m], qs, qt), (name, len(qs), x, m)
    assert {0, 1} <= classes_of(cls)                            # the comparison above is not one of class-0 words alone


def sum_in_order(y, qs):
    vf = 0.0
    for ym, q in zip(y, qs):
        vf += float(ym) / float(q)
    return vf


# ---------------------------------------------------------------- the model against the oracle
@pytest.mark.parametrize("name", ["G13", "W15", "X12"])
def test_keyswitch_equals_the_oracle_on_every_level_with_directed_words(name):
    ring = rr.chain_ring(name)
    key = rr.uniform_key(ring, KEY_SEED)
    for level in range(ring.nq):
        cx = rr.directed_ct(ring, level, CT_SEED + level)[1]
        d0, d1 = np.zeros_like(cx), np.zeros_like(cx)
        ol.lib().orc_keyswitch(ring.h, level, ol.p64(cx), ol.p64(key), ol.p64(d0), ol.p64(d1))
        w0, w1 = rr.keyswitch(ring, level, cx, key)
        assert np.array_equal(d0, w0) and np.array_equal(d1, w1), (name, level)


@pytest.mark.parametrize("name", ["V12", "W15", "G12"])
def test_rescale_model_equals_the_oracle(name):
    ring = rr.chain_ring(name)
    for level in range(1, ring.nq):
        for ct in (rr.uniform_ct(ring, level, level), rr.boundary_last_row(ring, level, rr.uniform_ct(ring, level, 9 + level))):
            want = np.zeros((2, level, ring.N), dtype=np.uint64)
            ol.lib().orc_rescale(ring.h, level, ol.p64(np.ascontiguousarray(ct)), ol.p64(want))
            assert np.array_equal(rr.rescale_model(ring, level, ct), want), (name, level)


# ---------------------------------------------------------------- coverage and discrimination
@pytest.mark.parametrize("name,level", rc.EDGE_KS)
def test_directed_words_reach_the_classes_and_expose_three_mistakes(name, level):
    """COVERAGE from the trace of the very key switch whose output the GPU file compares: +1 and 0 on every multi-modulus digit, -1 too on every digit of four or more
    moduli.  DISCRIMINATION: v rounded, v exact, and - where the cycle holds a word it moves, RECIP_DIGITS - y * fl(1/q) each change the expected output when
    made in the digits' extensions alone (made in ModDown's too, rounding would show on half of its uniform words whatever the digits do).  The uniform key makes
    ModDown's words uniform: its classes are all 0 here, and the identity key below covers it."""
    ring = rr.chain_ring(name)
    key = rr.uniform_key(ring, KEY_SEED)
    cx = rr.directed_ct(ring, level, CT_SEED)[1]
    d0, d1, tr = rr.keyswitch(ring, level, cx, key, trace=True)
    digs = ksw_ref.digits(level, ring.np_)
    multi = [i for i, dg in enumerate(digs) if len(dg) > 1]
    assert [i for i, c in enumerate(tr["digits"]) if c is not None] == multi
    for i in multi:
        seen = classes_of(tr["digits"][i])
        assert {0, 1} <= seen <= {-1, 0, 1}, (name, level, i, seen)
        assert len(digs[i]) < 4 or -1 in seen, (name, level, i, seen)
    vals = rr.directed_values(ring.moduli[:ring.nq], ring.np_, level)
    recip = [i for i in multi if (rr.word_classes(vals, [ring.moduli[m] for m in digs[i]]) != rr.word_classes(vals, [ring.moduli[m] for m in digs[i]], "recip")).any()]
    assert recip == RECIP_DIGITS.get((name, level), []), (name, level, recip)
    if not multi:
        assert (name, level) in (("V12", 0), ("A48", 0))       # one raw copy: no float correction to get wrong before ModDown
        return
    for mistake in rr.MISTAKES:
        if mistake == "recip" and not recip:
            continue
        w0, w1 = rr.keyswitch(ring, level, cx, key, mistake=mistake, where="digits")
        assert not np.array_equal(w0, d0) and not np.array_equal(w1, d1), (name, level, mistake)


@pytest.mark.parametrize("name,level", rc.EDGE_MODDOWN)
def test_identity_key_puts_moddown_on_both_boundaries_and_exposes_its_mistakes(name, level):
    """Under identity_key the P rows are +X0 (plane 0) and -X0 (plane 1) extended to P.  Where digit 0 has several moduli its float correction takes X0 = D0 - k to
    -k, so both planes hold words k and P - k: classes +1 and 0 in both.  A48's digit 0 is a raw copy of a word below q0, a 2^-2800-th of P: plane 0 holds k and
    q0 - k, never a word next to P, so class +1 cannot occur there; it has 0 and -1 (the sum of 47 quotients rounding down), and plane 1 = P - X0 has +1 and 0.
    The exact v in ModDown's extension alone changes both output polynomials.  (Rounding there is what the uniform keys catch: these words lie within 2^-20
    of an integer, where rounding and the float truncation agree.)  What comes out is itself a check of the model: floor(X / P) + class, X the signed word,
    which is 0 wherever the float correction does what it is there for, so the expected rows here are sparse and small."""
    ring = rr.chain_ring(name)
    key = rr.identity_key(ring)
    cx = rr.directed_ct(ring, level, CT_SEED)[1]
    d0, d1, tr = rr.keyswitch(ring, level, cx, key, trace=True)
    seen = [classes_of(c) for c in tr["moddown"]]
    if name == "A48":
        assert seen == [{-1, 0}, {0, 1}], seen
    else:
        assert all({0, 1} <= s <= {-1, 0, 1} for s in seen), (name, seen)
    w0, w1 = rr.keyswitch(ring, level, cx, key, mistake="exact", where="moddown")
    assert not np.array_equal(w0, d0) and not np.array_equal(w1, d1), name
    skipped = rr.keyswitch(ring, level, cx, key)                # without the trace the all-zero digits are skipped: the same words
    assert np.array_equal(skipped[0], d0) and np.array_equal(skipped[1], d1)


# ---------------------------------------------------------------- the key sum's ceiling
def test_m48_planted_maximum_drives_the_key_sums_past_2_to_125():
    """k_gr_keyip adds beta = 47 products in 128 bits before its one reduction.  Only a digit's OWN-modulus term can be steered to (q - 1)^2: at any other target
    the word is the digit's word reduced modulo that target, and the digit's word is set through its own residue.  With every input and key row all q - 1 (the
    NTT of the constant -1) digit i's word is q_i - 1, and at target t it is q_i - 1 itself where q_i < q_t - the moduli descend, so for every i > t - and
    q_i - 1 - q_t, a few thousand, where q_i > q_t.  Target t thus sums 47 - t terms of about 2^122: past 2^125 for every t < 38, more than half of the 48 rows, and
    the first row holds 47 of them, above 2^127.5.  Asserted on the model's unreduced sums, in Python integers."""
    ring = rr.chain_ring("M48")
    cx, key = rr.planted_maximum(ring, 46)
    sums = rr.key_sums(ring, 46, cx, key)
    flat = np.concatenate([row for plane in sums for row in plane])
    assert len(flat) == 2 * 48 * ring.N
    assert sum(int(s) > 1 << 125 for s in flat) * 2 > len(flat)
    top = max(int(s) for s in flat)
    assert 1 << 127 < top < 1 << 128 and top >= 46 * ((1 << 61) - (1 << 24)) ** 2
    assert all(int(s) > 1 << 125 for plane in sums for row in plane[:38] for s in row[:8])
