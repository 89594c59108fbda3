"""CPU checks of tests/refresh_ref.py: the word-exact model of refresh.hip's arithmetic equals the Python integers on every directed and random
coefficient of every case, the oracle equals them too (zero key, zero crs, zero aggregated shares, read back through ring.intt), the directed
inputs reach every branch class the model calls reachable - at 8 coefficients or more, while the seeded random fill takes none of the rare
ones - and the inputs have teeth: each mutant of the model is caught by the directed inputs and missed by the random fill at the
reference's scale pairs, which is all that tests/test_refresh.py ran.  The GPU side is tests/test_gpu_refresh_edges.py."""
from functools import lru_cache
from math import prod

import numpy as np
import pytest

import ksw_ref as kr
import oracle_lib as ol
import refresh_ref as rr

IDS = [rr.case_id(c) for c in rr.CASES]
# the cases the mutants run on: every shift class, both forms of the recode with new moduli, a 47-bit chain, the 12-modulus level
MUTANT_CASES = [c for c in rr.CASES if rr.case_id(c) in ("PN14-L6-W7-unscaled", "PN14-L6-W7-ref", "PN14-L9-W7-r64", "PN14-L9-W6-l64", "PN14-L9-W5-l75",
                                                         "PN14-L9-W7-np2_up", "PN14-L9-W6-np2_l48", "S4-L7-W7-ref", "R13-L11-W7-ref")]
OLD_CASES = [c for c in MUTANT_CASES if c[0] == "PN14" and (c[3] is None or c[3] in rr.REFERENCE_PAIRS)]     # what tests/test_refresh.py ran


@lru_cache(maxsize=None)
def run(case, mutant=None):
    """the model over a case: (h0 rows, h1 rows before the negation, recode rows), and the classes of the mask path and of the recode"""
    c = rr.case_inputs(case)
    h0, c0 = rr.model_rows(c.limbs, c.e, c.q[:c.level + 1], None, mutant)
    h1, c1 = rr.model_rows(c.limbs, c.e, c.q, c.scales, mutant)
    x, cx = rr.model_recode(c.x_res, c.level, c.q, c.scales, mutant)
    for k, v in c0.items():                                     # in a scaled case h0 is another kernel's work: its classes carry the prefix u_
        k = k if rr.ratio(c.scales) is None else "u_" + k
        c1[k] = c1[k] | v if k in c1 else v
    return (h0, h1, x), c1, cx


def wrong(case, mutant):
    """(directed, fill) coefficients at which the mutant's values are not the Python integers'"""
    c = rr.case_inputs(case)
    (h0, h1, x), _, _ = run(case, mutant)
    bad_m = np.any(h0 != c.want_h0, axis=0) | np.any(h1 != c.want_h1, axis=0)
    bad_x = np.any(x != c.want_x, axis=0)
    return int((bad_m & c.mask_directed).sum() + (bad_x & c.x_directed).sum()), int((bad_m & ~c.mask_directed).sum() + (bad_x & ~c.x_directed).sum())


def test_scale_parts_keep_the_mantissa():
    assert rr.scale_parts(2.0 ** 34) == (1 << 34, 0) and rr.scale_parts(2.0 ** 68) == (1 << 52, 16) and rr.scale_parts(1.0) == (1, 0)
    assert rr.scale_parts(2.0 ** 53 + 2) == ((1 << 52) + 1, 1) and rr.scale_parts(2.0 ** 60) == (1 << 52, 8) and rr.scale_parts(1.5) == (1, 0)
    assert [rr.ratio(rr.PAIRS[k])[2] for k in ("ref", "i98", "i104", "r64", "r70", "l45", "l64", "l75", "c60", "m1", "d1", "np2_up", "np2_l48")] == [-16, -46, -52, -64, -70, 45, 64, 75, -7, -1, 0, 0, 48]
    assert rr.ratio(rr.PAIRS["one"]) is None and rr.ratio(None) is None
    assert rr.quo(-7, 2) == -3 and rr.quo(7, 2) == 3 and rr.quo(-1, 1 << 34) == 0


def test_case_table_covers_every_class_of_the_launch():
    """what is uniform per launch is covered by the table, not by coefficients: every class of bg_shift, both exits of bg_div_small, W = 1, 7 and 16,
    the three chains at the levels of the issue, level 11 = RF_MAXL - 1, and every case passes the library's fit checks"""
    assert all(rr.fits(c) for c in rr.CASES) and len(set(rr.CASES)) == len(rr.CASES)
    shifts = {rr.shift_class(rr.ratio(rr.scales_of(c))[2]) for c in rr.CASES if rr.ratio(rr.scales_of(c))}
    assert shifts == {"shift_none", "shift_right_ws0_bs", "shift_right_ws1_bs", "shift_right_ws1_bs0", "shift_left_ws0_bs", "shift_left_ws1_bs", "shift_left_ws1_bs0"}
    assert {rr.ratio(rr.scales_of(c))[1] == 1 for c in rr.CASES if rr.ratio(rr.scales_of(c))} == {True, False}
    assert {1, 7, 16} <= {c[2] for c in rr.CASES}
    assert {(c[0], c[1]) for c in rr.CASES} == {("PN14", 9), ("PN14", 6), ("PN14", 0), ("S4", 7), ("S4", 0), ("R13", 11)}
    assert set(rr.PAIRS) == {c[3] for c in rr.CASES if c[3]}
    q, p = rr.chain("R13")
    assert len(q) == 13 and len(p) == 1 and rr.RF_MAXL == 12 and all(v.bit_length() == 36 for v in q)
    assert all(v.bit_length() == 47 for v in rr.chain("S4")[0])
    assert not rr.fits(("PN14", 9, 6, "l75")) and rr.fits(("PN14", 9, 5, "l75"))


def test_digit_helper_and_placement():
    mods = rr.chain("PN14")[0][:4]
    Q = prod(mods)
    for x in (0, 1, Q - 1, Q >> 1, 123456789 ** 4 % Q):
        d = rr.to_digits(x, mods)
        assert rr.from_digits(d, mods) == x and all(0 <= v < q for v, q in zip(d, mods))
    assert rr.from_digits([1, 2, 3], [5, 7, 11]) == 1 + 5 * (2 + 7 * 3)
    items, flag = rr.place(list(range(100, 110)), [-1] * rr.N, 4)
    assert [items[i] for i in (0, 255, 256, rr.N - 1)] == [100, 101, 102, 103] and flag.sum() == 10 * rr.REPS
    assert sorted(v for v in items if v >= 0) == sorted(list(range(100, 110)) * rr.REPS)


def test_canon_fix_up_counts_on_pn14_modulus_7():
    """the figure of the issue: canon(k q) needs its equality fix-up for 1532 of k = 1 .. 1999 on PN14's modulus 7"""
    q = ol.Q_PN14[7]
    assert sum(1 for k in range(1, 2000) if kr.canon_model(k * q, q, fixup=False) == q) == 1532


@pytest.mark.parametrize("case", rr.CASES, ids=IDS)
def test_model_equals_python_integers(case):
    """every directed and random coefficient; the classes that are unreachable by construction (refresh_ref's docstring) stay empty"""
    c = rr.case_inputs(case)
    (h0, h1, x), cm, cx = run(case)
    assert np.array_equal(h0, c.want_h0) and np.array_equal(h1, c.want_h1) and np.array_equal(x, c.want_x)
    for cls in (cm, cx):
        assert not any(cls[p + k].any() for k in rr.DEAD for p in ("", "u_") if p + k in cls)
    assert not cm.get(f"cy_limb{c.W - 1}", np.zeros(1)).any()
    assert np.array_equal(rr.model_small_rows(c.e, c.q), rr.expected_rows([0] * rr.N, c.e, c.q))


@pytest.mark.parametrize("case", rr.CASES, ids=IDS)
def test_directed_inputs_reach_every_reachable_class(case):
    """coverage is a condition: at least 8 directed coefficients in every class required(case) names, none of the fill's in a rare one"""
    c = rr.case_inputs(case)
    _, cm, cx = run(case)
    need_m, need_x = rr.required(case)
    assert c.mask_directed.sum() >= 8 * 100 and c.x_directed.sum() >= 8 * 10
    for need, cls, d in ((need_m, cm, c.mask_directed), (need_x, cx, c.x_directed)):
        for k in need:
            assert k in cls and int((cls[k] & d).sum()) >= 8, k
        for k in rr.rare_in(case):
            for k in (k, "u_" + k):
                assert k not in cls or not (cls[k] & ~d).any(), k


def test_share_tail_negates_unless_zero():
    q = ol.Q_PN14[3]
    r = np.array([0, 1, q - 1, 0, 12345], dtype=np.uint64)
    out, cls = rr.model_share_tail(r, q, 1)
    assert [int(v) for v in out] == [0, q - 1, 1, 0, q - 12345] and cls["share_neg_zero"].sum() == 2
    assert [int(v) for v in rr.model_share_tail(r, q, 1, "no_zero_guard")[0]] == [q, q - 1, 1, q, q - 12345]
    assert np.array_equal(rr.model_share_tail(r, q, 0)[0], r)


@pytest.mark.parametrize("mutant", rr.MUTANTS)
def test_mutants_are_caught_by_the_directed_inputs_and_missed_by_the_random_fill(mutant):
    """one mistake at a time.  Caught: on some case the mutant's values differ from the Python integers at directed coefficients.  Missed: at the
    reference's scale pairs and the unscaled form on PN14 (OLD_CASES) the seeded random fill - what the suite had - sees no difference.  (At the new scale
    pairs a broken shift is wrong on every coefficient, random ones included: there the pair is the directed input.)"""
    hits = {rr.case_id(c): wrong(c, mutant) for c in MUTANT_CASES}
    assert sum(d for d, _ in hits.values()) >= 8, hits
    assert all(hits[rr.case_id(c)][1] == 0 for c in OLD_CASES), hits


def test_each_mutant_is_wrong_exactly_on_its_class():
    """the live guards: every coefficient of the class is wrong without the guard, and no other.  (The tie is invisible where the ratio is an
    integer R and the level has every modulus: (x - Q) R and x R agree modulo the moduli of Q.)"""
    for case in MUTANT_CASES:
        c = rr.case_inputs(case)
        if rr.ratio(c.scales) is None:
            continue
        (_, _, x), _, cx = run(case, "no_zero_guard")
        assert np.array_equal(np.any(x != c.want_x, axis=0), cx["recode_neg_zero"])
        (_, _, x), _, _ = run(case, "tie_strict")
        bad, tie = np.any(x != c.want_x, axis=0), run(case)[2]["tie_all_equal"]
        assert not (bad & ~tie).any()
        if int(c.scales[1]) % int(c.scales[0]) or c.level + 1 < len(c.q):
            assert np.array_equal(bad, tie)


@pytest.mark.parametrize("case", rr.CASES, ids=IDS)
def test_oracle_equals_python_integers(case):
    """orc_refresh_gen_shares / _finish and their scaled forms with zero key, zero crs and zero aggregated shares, read back through ring.intt"""
    c = rr.case_inputs(case)
    ring = rr.ring_of(case[0])
    nl, nq = c.level + 1, ring.nq
    zsk, zcrs = np.zeros((nq, ring.N), dtype=np.uint64), np.zeros((nq, ring.N), dtype=np.uint64)
    ct = ring.fill_uniform(c.level, 9)
    if c.scales is None:
        h0, h1 = ol.refresh_gen_shares(ring, c.level, ct, zsk, zcrs, c.limbs, c.e, c.e)
    else:
        h0, h1 = ol.refresh_gen_shares_scaled(ring, c.level, ct, c.scales[0], c.scales[1], zsk, zcrs, c.limbs, c.e, c.e)
    for j in range(nl):
        assert np.array_equal(ring.intt(j, h0[j]), c.want_h0[j]), f"h0 modulus {j}"
    for j in range(nq):
        q = np.uint64(ring.moduli[j])
        assert np.array_equal(ring.intt(j, h1[j]), (q - c.want_h1[j]) % q), f"h1 modulus {j}"
    ct[0] = np.stack([ring.ntt(j, c.x_res[j]) for j in range(nl)])
    z0 = np.zeros((nl, ring.N), dtype=np.uint64)
    if c.scales is None:
        out = ol.refresh_finish(ring, c.level, ct, z0, zcrs, zcrs)
    else:
        out = ol.refresh_finish_scaled(ring, c.level, ct, c.scales[0], c.scales[1], z0, zcrs, zcrs)
    for j in range(nq):
        assert np.array_equal(ring.intt(j, out[0, j]), c.want_x[j]), f"recode modulus {j}"
    assert not out[1].any()
