"""CPU checks of the ring-vector encoder / decoder (sfgwas_amd/csrc/rvec.hip): the Python-integer reference tests/rvec_ref.py against the literal mpmath sums of the
definitions and against the float-vector references (exactref.encode, decode_ref.decode) on inputs small enough for those; the round trip and the additivity that
make the share conversion work; the committed base roots digit for digit; and the host C++ of the feature (rvec_host.hpp: constant parsing, limb-count selection,
refusal arithmetic; rvec_fx.hpp: the arithmetic every kernel runs per element) as a stand-alone program under AddressSanitizer and UBSan, word for word against the
reference over whole 8192-point transforms.  No GPU."""
from fractions import Fraction
import os
import shutil
import subprocess

import numpy as np
import pytest

import rvec_cases as rc
import rvec_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P2, P4 = rc.FIELDS[2], rc.FIELDS[4]


@pytest.mark.parametrize("p", [P2, P4])
def test_reference_matches_the_literal_sums_on_a_small_ring(p):
    """N = 64: every coefficient of encode and every slot of decode against the O(n^2) mpmath sum of the definition (120 digits; the values have at most 80).
    f = 28: with scale 2^34 coefficient 0 is twice the sum of the centred elements, an integer, not the half-integer f = 30 makes of it on so small a ring."""
    import mpmath as mp
    N, n, f = 64, 32, 28
    for scale in (rc.SCALE, rc.SCALE_ODD):
        x = rc.uniform_elems(p, n - 3, 3)
        out, tie, err = rr.encode(x, p, N, scale, f)
        assert err < Fraction(1, 2 ** 100) and min(tie) > Fraction(1, 2 ** 40)
        for c in range(n):
            re, im = rr.literal_encode_value(x, p, N, c)
            with mp.workdps(150):
                k = mp.mpf(scale.numerator) / scale.denominator / 2 ** f
                assert out[c] == int(mp.nint(re * k)) and out[c + n] == int(mp.nint(im * k)), c
        Q = 2 ** 300 + 157
        coeffs = [rr.centred_crt(v, Q) for v in rc.uniform_elems(Q, N, 4)]
        r, tie, err = rr.decode(coeffs, p, N, scale, f, n - 1)
        assert err < Fraction(1, 2 ** 100) and min(tie) > Fraction(1, 2 ** 40) and len(r) == n - 1
        for t in range(n - 1):
            with mp.workdps(150):
                v = rr.literal_decode_value(coeffs, N, t, dps=150) * 2 ** f * scale.denominator / scale.numerator
                assert r[t] == int(mp.nint(v)) % p, t


def test_reference_matches_the_float_vector_references_on_small_inputs():
    """small integers as doubles: exactref.encode (f = 0 there) and decode_ref.decode compute the same sums with 240-bit tables"""
    import decode_ref
    import exactref
    N, n = 64, 32
    rnd = np.random.default_rng(8)
    v = rnd.integers(-2 ** 40, 2 ** 40, n)
    want, _, _ = exactref.encode(v.astype(np.float64), N, 2.0 ** 20)
    got, tie, _ = rr.encode([int(a) % P2 for a in v], P2, N, Fraction(2 ** 20), 0)
    assert min(tie) > Fraction(1, 2 ** 30) and got == [int(a) for a in want]
    coeffs = [int(a) for a in rnd.integers(-2 ** 45, 2 ** 45, N)]
    re, _, derr = decode_ref.decode(coeffs, N, 2 ** 10)
    got, tie, _ = rr.decode_int(coeffs, N, Fraction(2 ** 10), 4)
    for t in range(n):
        exact = re[t] * 16
        assert abs(exact - got[t]) <= Fraction(1, 2) + derr * 16, t


@pytest.mark.parametrize("p", [P2, P4])
def test_decode_of_encode_is_the_identity_when_the_scale_outweighs_the_coefficient_roundings(p):
    """Each of the N coefficients is rounded by at most 1/2, and a slot sums all of them with weights |cos| + |sin| <= sqrt 2 per complex coefficient: the decoded
    value is off by at most n sqrt(2) / 2 * 2^f / scale before its own rounding.  That is below 1/2 - the round trip is exact - once scale > 2^f n sqrt 2, i.e. from
    scale = 2^(f + log2 N) on.  (At the shipped f = 30, scale = 2^34 the deviation is a few units: it is part of the end-to-end bound)"""
    for N, scale in ((64, Fraction(2 ** (30 + 6))), (rc.N, Fraction(2 ** (30 + 14)))):
        n = N // 2
        assert n * Fraction(1414214, 10 ** 6) / 2 * 2 ** 30 / scale < Fraction(1, 2)
        x = rc.uniform_elems(p, n, 31)
        out, _, _ = rr.encode(x, p, N, scale, 30)
        back, _, _ = rr.decode(out, p, N, scale, 30)
        assert back == x


@pytest.mark.parametrize("p", [P2, P4])
def test_encodings_of_two_shares_add_up_to_the_encoding_of_the_secret(p):
    """a + b = x (mod p), |centre(x)| < 2^60, a uniform: centre(a) + centre(b) = centre(x) over the integers (the two centrings cancel unless a lies within 2^60 of
    0 or p/2), the map before the rounding is linear, so the sum of the two rounded encodings differs from the rounded encoding of x by at most 1 per coefficient"""
    rnd = np.random.default_rng(41)
    xs = [int(v) % p for v in rnd.integers(-2 ** 60 + 1, 2 ** 60, rc.n)]
    a = rc.uniform_elems(p, rc.n, 42)
    b = [(x - s) % p for x, s in zip(xs, a)]
    ea, eb, ex = (rr.encode(v, p, rc.N, rc.SCALE, rc.F)[0] for v in (a, b, xs))
    worst = max(abs(u + v - w) for u, v, w in zip(ea, eb, ex))
    assert worst <= 1
    assert max(abs(w) for w in ex) < 2 ** 65                          # and it is the encoding of a SMALL vector: the shares' 2^127 cancelled


def _header_roots():
    import re
    txt = open(os.path.join(ROOT, "sfgwas_amd", "csrc", "rvec_roots.hpp")).read()
    out = {}
    for name in ("RVEC_ROOT_COS", "RVEC_ROOT_SIN"):
        body = txt[txt.index(name + "[RVEC_NROOTS]"):]
        body = body[body.index("{") + 1:body.index("};")]
        rows = re.findall(r"\{([^{}]*)\}", body)
        out[name] = [sum(int(w.strip().rstrip("UL"), 16) << (64 * i) for i, w in enumerate(r.split(","))) for r in rows]
    return out


def test_committed_base_roots_equal_mpmath_digit_for_digit():
    import mpmath as mp
    roots = _header_roots()
    assert len(roots["RVEC_ROOT_COS"]) == 15 and len(roots["RVEC_ROOT_SIN"]) == 15
    with mp.workdps(300):
        for k in range(1, 16):
            x = mp.mpf(1) / (1 << k)
            assert roots["RVEC_ROOT_COS"][k - 1] == int(mp.nint(mp.cospi(x) * mp.mpf(2) ** 576)), k
            assert roots["RVEC_ROOT_SIN"][k - 1] == int(mp.nint(mp.sinpi(x) * mp.mpf(2) ** 576)), k
    # and the committed file is what the committed generator writes
    gen = subprocess.run(["python3", os.path.join(ROOT, "tools", "gen_rvec_roots.py")], capture_output=True, text=True, check=True).stdout
    assert gen == open(os.path.join(ROOT, "sfgwas_amd", "csrc", "rvec_roots.hpp")).read()


# ---------------------------------------------------------------- the host C++ under the sanitizers
@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("rvec_host") / "host_rvec_test")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tests", "host", "host_rvec_test.cpp")])
    return exe


def _run(exe, tmp_path, cmd):
    (tmp_path / "cmd.txt").write_text(cmd)
    out = subprocess.run([exe, str(tmp_path / "cmd.txt"), str(tmp_path / "out.txt")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    return (tmp_path / "out.txt").read_text().split("\n")


def _case(limbs, p, f, n_elem, scale, level):
    from sfgwas_amd.params import Q_PN14
    words = " ".join(str((p >> (64 * i)) & (2 ** 64 - 1)) for i in range(max(1, min(limbs, 8))))
    return f"{limbs} {f} {n_elem} {float(scale).hex()} {level} {len(Q_PN14)} {' '.join(map(str, Q_PN14))} {words}"


def test_host_roots_and_table_stay_within_the_derived_error(host_exe, tmp_path):
    """the base roots at the table's 574 fractional bits are the committed words shifted down by two; a table entry zeta^j is at most 13 truncating complex products of
    them: each adds 2 units of truncation per component and passes on the operands' errors (one unit per base-root component) with unit gain - fewer than
    13 * 6 + 2 < 2^7 units of 2^-574 on either component.  Checked on the powers of two, the all-ones index, both ends and seeded indices."""
    import mpmath as mp
    roots = _header_roots()
    lines = _run(host_exe, tmp_path, "roots")
    for k in range(1, 16):
        kk, c, s = lines[k - 1].split()
        assert int(kk) == k and int(c, 16) == roots["RVEC_ROOT_COS"][k - 1] >> 2 and int(s, 16) == roots["RVEC_ROOT_SIN"][k - 1] >> 2
    js = sorted({0, 1, 2, 3, 8191, 8192, 8193, 16383, 0x2AAA, 0x1555} | {1 << b for b in range(14)} | {int(v) for v in np.random.default_rng(2).integers(0, rc.N, 40)})
    lines = _run(host_exe, tmp_path, f"table {len(js)} " + " ".join(map(str, js)))
    with mp.workdps(300):
        for j, line in zip(js, lines):
            jj, re, im = line.split()
            assert int(jj) == j
            x = mp.mpf(j) / rc.N
            assert abs(int(re, 16) - mp.cospi(x) * mp.mpf(2) ** 574) < 2 ** 7, j
            assert abs(int(im, 16) - mp.sinpi(x) * mp.mpf(2) ** 574) < 2 ** 7, j


def test_host_plan_and_refusals(host_exe, tmp_path):
    """limb-count selection against its restatement in rvec_ref.plan, the level rule bitlen(p) - 1 - f + ceil(log2 scale) + 1 < bitlen(Q_level) - 1 at its edges
    (PN14QP438: bitlen(Q_level) = 46 + 35 level or one less; f = 30, scale 2^34: limbs 2 from level 3, limbs 4 from level 7), and every static refusal"""
    from sfgwas_amd.params import Q_PN14
    qbits = [rr.q_product(Q_PN14, lv).bit_length() for lv in range(len(Q_PN14))]
    assert qbits == [46, 80, 116, 150, 185, 220, 255, 290, 325, 360]                 # (46 + 35 level, less one bit where the product falls short)

    def plan(direction, limbs, p, f, n_elem, scale, level):
        return _run(host_exe, tmp_path, f"plan {direction} " + _case(limbs, p, f, n_elem, scale, level))[0].split(" ", 1)

    for limbs, p, first in ((2, P2, 3), (4, P4, 7)):
        assert plan("enc", limbs, p, 30, 8192, 2.0 ** 34, first - 1)[0] == "refused"
        for level in (first, 9):
            st, rest = plan("enc", limbs, p, 30, 8192, 2.0 ** 34, level)
            assert st == "ok" and tuple(map(int, rest.split()[:2])) == rr.plan("enc", p.bit_length(), qbits[level], Fraction(2 ** 34), 30)
        for level in range(10):
            for scale, f in ((2.0 ** 34, 30), (float(rc.SCALE_ODD), 30), (2.0 ** 20, 40), (1.0, 0)):
                st, rest = plan("dec", limbs, p, f, 17, scale, level)
                assert st == "ok" and tuple(map(int, rest.split()[:2])) == rr.plan("dec", p.bit_length(), qbits[level], Fraction(scale), f), (level, scale, f)
    # the widths the shipped parameters reach: encoder 3 / 5 words, decoder 2..7 words over levels 0..9
    assert [rr.plan("enc", p.bit_length(), 0, rc.SCALE, 30)[0] for p in (P2, P4)] == [3, 5]
    assert [rr.plan("dec", 0, qb, rc.SCALE, 30)[0] for qb in qbits] == [2, 3, 3, 4, 4, 5, 5, 6, 7, 7]
    for args, word in (((3, P2, 30, 8192, 2.0 ** 34, 9), "2 or 4"), ((2, P2 - 1, 30, 8192, 2.0 ** 34, 9), "odd"), ((2, P2, 30, 8193, 2.0 ** 34, 9), "element count"),
                       ((2, P2, 30, 0, 2.0 ** 34, 9), "element count"), ((2, P2, 63, 8192, 2.0 ** 34, 9), "frac_bits"), ((2, P2, -1, 8192, 2.0 ** 34, 9), "frac_bits"),
                       ((2, P2, 30, 8192, 0.5, 9), "scale"), ((2, P2, 30, 8192, float("nan"), 9), "scale"), ((2, P2, 30, 8192, float("inf"), 9), "scale"),
                       ((2, P2, 30, 8192, 2.0 ** 34, 10), "level"), ((2, P2, 30, 8192, 2.0 ** 34, -1), "level")):
        for direction in ("enc", "dec"):
            st, rest = plan(direction, *args)
            assert st == "refused" and word in rest, (direction, args, rest)


def _enc_host(exe, tmp_path, limbs, p, x, scale, level):
    lines = _run(exe, tmp_path, "encode " + _case(limbs, p, rc.F, len(x), scale, level) + " " + " ".join("%x" % v for v in x))
    assert lines[0].startswith("ok")
    coef = [int(v, 16) for v in lines[1:1 + rc.N]]
    rows = np.array([int(v) for v in lines[1 + rc.N:1 + rc.N + (level + 1) * rc.N]], dtype=np.uint64).reshape(level + 1, rc.N)
    return coef, rows


@pytest.mark.parametrize("limbs", [2, 4])
def test_host_arithmetic_encodes_word_for_word(host_exe, tmp_path, limbs):
    """the per-element functions of every encoder kernel, run over whole transforms in the kernels' order, against the reference: exact wherever the reference is
    further than 2^-32 (+ its own error) from a tie - and no input used here is that close"""
    from sfgwas_amd.params import Q_PN14
    p, level = rc.FIELDS[limbs], {2: 3, 4: 7}[limbs]
    for name, x in rc.encode_inputs(p).items():
        for scale in ((rc.SCALE, rc.SCALE_ODD) if name == "uniform" else (rc.SCALE,)):
            want, tie, err = rr.encode(x, p, rc.N, scale, rc.F)
            assert min(tie) > rc.TIE_BAND + err, name
            got, rows = _enc_host(host_exe, tmp_path, limbs, p, x, scale, level)
            assert got == want, name
            for i in range(level + 1):
                assert rows[i].tolist() == [v % Q_PN14[i] for v in want], (name, i)


@pytest.mark.parametrize("limbs", [2, 4])
def test_host_arithmetic_decodes_word_for_word(host_exe, tmp_path, limbs):
    """every directed row at level 9 (7 words), the uniform row and the two tie rows at levels 0 and 5 (2 and 5 words), the uniform row at levels 3 and 7 (4 and 6
    words) and at level 9 with f = 58 (8 words); limbs 4 (the field enters at the last step only): the uniform row and the all-tie row"""
    from sfgwas_amd.params import Q_PN14
    p = rc.FIELDS[limbs]
    some = ("uniform", "all_half_tie", "single_tie")
    for level, f, names in ((9, rc.F, None), (0, rc.F, some), (5, rc.F, some), (3, rc.F, some[:1]), (7, rc.F, some[:1]), (9, 58, some[:1])):
        Q = rr.q_product(Q_PN14, level)
        for name, res in rc.decode_inputs(Q).items():
            if (names is not None and name not in names) or (limbs == 4 and name not in some[:2]):
                continue
            coeffs = [rr.centred_crt(v, Q) for v in res]
            n_elem = rc.n - 5 if name == "uniform" else rc.n
            want, tie, err = rr.decode(coeffs, p, rc.N, rc.SCALE, f, n_elem)
            assert min(tie) > rc.TIE_BAND + err, (level, name)
            lines = _run(host_exe, tmp_path, "decode " + _case(limbs, p, f, n_elem, rc.SCALE, level) + " " +
                         " ".join(("-%x" % -v) if v < 0 else "%x" % v for v in coeffs))
            assert lines[0].split()[:2] == ["ok", str(rr.plan("dec", 0, Q.bit_length(), rc.SCALE, f)[0])]
            assert [int(v, 16) for v in lines[1:1 + n_elem]] == want, (level, name)


def test_host_arithmetic_rounds_an_exact_tie_to_a_neighbour(host_exe, tmp_path):
    """one slot holding 1, scale 2^32, f = 20: coefficient 0 is 2^32 * 2^-20 * 1 / 8192 = 1/2 exactly"""
    want, tie, _ = rr.encode([1], P2, rc.N, Fraction(2 ** 32), 20)
    assert tie[0] == 0
    got, _ = _enc_host_f(host_exe, tmp_path, 2, P2, [1], Fraction(2 ** 32), 9, 20)
    assert abs(Fraction(got[0]) - Fraction(1, 2)) == Fraction(1, 2)
    assert all(g == w for g, w, d in zip(got, want, tie) if d > rc.TIE_BAND)


def _enc_host_f(exe, tmp_path, limbs, p, x, scale, level, f):
    lines = _run(exe, tmp_path, "encode " + _case(limbs, p, f, len(x), scale, level) + " " + " ".join("%x" % v for v in x))
    assert lines[0].startswith("ok"), lines[0]
    return [int(v, 16) for v in lines[1:1 + rc.N]], None
