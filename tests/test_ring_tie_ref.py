"""The general ring's tie resolver (sfgwas_amd/csrc/gring_tie.hpp) on the CPU: the committed base roots, the cosine table its builder makes, the fold, the decision
function and whole coefficients, held against mpmath, Python integers (tests/ring_tie_ref.py) and tests/exactref.py.

tests/host/host_gring_tie_test.cpp includes the header alone and is built once with AddressSanitizer + UBSan as a plain executable (a plain build where the
runtimes are absent).  Nothing here needs a GPU."""
import os
import random
import re
import subprocess

import numpy as np
import pytest

import exactref
import ring_tie_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sfgwas_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "host", "host_gring_tie_test.cpp")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("tie") / "host_gring_tie_test")
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-I", CSRC, "-o", out, SRC]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    if subprocess.run(base + san, capture_output=True).returncode != 0:        # no sanitizer runtimes: the plain build must still succeed
        subprocess.check_call(base)
    return out


def run(exe, tmp_path, commands):
    script = tmp_path / "script.txt"
    script.write_text("\n".join(commands) + "\n")
    out = subprocess.run([exe, str(script)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("OK"), out.stdout[-2000:] + out.stderr[-4000:]
    return out.stdout.splitlines()[:-1]


def test_committed_base_roots_equal_mpmath_digit_for_digit():
    import mpmath as mp
    hdr = open(os.path.join(CSRC, "gring_tie_roots.hpp")).read()
    rows = re.findall(r"\{((?:0x[0-9A-F]{16}ULL(?:, )?){5})\}", hdr)
    assert len(rows) == 32
    vals = [sum(int(w[:-3], 16) << (64 * i) for i, w in enumerate(r.split(", "))) for r in rows]
    with mp.workdps(140):
        for k in range(1, 17):
            x = mp.mpf(1) / (1 << k)
            assert vals[k - 1] == int(mp.nint(mp.cospi(x) * mp.mpf(2) ** 256)), k
            assert vals[16 + k - 1] == int(mp.nint(mp.sinpi(x) * mp.mpf(2) ** 256)), k


@pytest.mark.parametrize("logN", [12, 16])
def test_every_table_entry_is_within_the_builders_bound_of_the_cosine(exe, tmp_path, logN):
    """the builder documents |entry - cos 2^F| <= kTabErr = 1 unit; mpmath's rounded entry is within half a unit of the cosine, so the two differ by at most one"""
    N = 1 << logN
    got = [int(x, 16) for x in run(exe, tmp_path, [f"T {logN}"])]
    want = tr.table(N)
    assert len(got) == N // 2 + 1 == len(want)
    worst = max(abs(g - w) for g, w in zip(got, want))
    print("largest difference from mpmath's rounded entries, units of 2^-191:", worst)
    assert worst <= tr.TAB_ERR
    assert got[0] == 1 << tr.FRAC and got[N // 2] == 0                     # k = 0 and k = N / 2 are exact
    assert all(got[k] > got[k + 1] for k in range(N // 2))                 # strictly falling on [0, pi / 2]


def test_fold_reaches_every_angle_by_symmetry(exe, tmp_path):
    N = 4096
    angles = [0, 1, N // 2 - 1, N // 2, N // 2 + 1, N - 1, N, N + 1, 3 * N // 2 - 1, 3 * N // 2, 3 * N // 2 + 1, 2 * N - 1] + random.Random(3).sample(range(2 * N), 200)
    lines = run(exe, tmp_path, [f"F {N} {a}" for a in angles])
    import mpmath as mp
    tab = tr.table(N)
    for a, ln in zip(angles, lines):
        k, neg = int(ln.split()[1]), bool(int(ln.split()[2]))
        assert (k, neg) == tr.fold(a, N) and 0 <= k <= N // 2
        with mp.workdps(70):                                               # the folded entry with its sign is the cosine of the unfolded angle
            assert abs((-tab[k] if neg else tab[k]) - mp.cospi(mp.mpf(a) / N) * mp.mpf(2) ** tr.FRAC) <= 0.5 + 1e-9, a


def decision_cases():
    """(X, m, e, logn, A): constructed sums around the margin"""
    rnd = random.Random(11)
    cases = []
    full = (1 << 53) - 1                                                   # a full 53-bit mantissa
    for m, e, logn, A in [(1 << 52, -7, 11, 1), (full, -7, 11, 1), (full, -52, 15, 1 << 22), (0x1F3A5B7C9D1E3F, 20, 11, 3), (0x1A2B3C4D5E6F71, 39, 15, 5), (full, -30, 15, 1 << 22),
                          (0x10000000000001, 0, 13, 200)]:
        sh = tr.FRAC + logn - e
        M = m * tr.TAB_ERR * A
        for K in (0, 1, 2, 12345, (1 << 61) + 12345):
            for dist in (0, 1, -1, M - 1, M, M + 1, -(M - 1), -M, -(M + 1), rnd.randrange(1 << (sh - 2)), -rnd.randrange(1 << (sh - 2))):
                # Y = (K + 1/2) 2^sh + dist must be a multiple of m: take the nearest X and keep what it gives
                Y = (2 * K + 1) * (1 << (sh - 1)) + dist
                X = Y // m
                for Xs in (X, X + 1, -X, -(X + 1)):
                    if abs(Xs) < 1 << 214:
                        cases.append((Xs, m, e, logn, A))
    # distances exactly at the margin need Y = m X on the grid: with m = 2^52 every multiple of 2^52 is reachable
    m, e, logn, A = 1 << 52, -10, 11, 7
    sh, M = tr.FRAC + logn - e, (1 << 52) * 7
    for K in (0, 5):
        for d in (0, M - m, M, M + m, -(M - m), -M, -(M + m)):
            Y = (2 * K + 1) * (1 << (sh - 1)) + d
            assert Y % m == 0
            cases += [(Y // m, m, e, logn, A), (-(Y // m), m, e, logn, A)]
    # the largest sums: A at its ceiling 2^7 n at logN 16 and every table entry at 2^F
    cases += [(s * (1 << 22) * (1 << tr.FRAC), full, e, 15, 1 << 22) for s in (1, -1) for e in (-52, -25, -20)]
    # sh <= 0 (the value is an integer) and the edges of the domain
    cases += [(1, 1 << 52, 300, 11, 1), (3, 1 << 52, 206, 11, 1), (-3, full, 202, 11, 1), (1 << 8, 1 << 52, 203, 11, 1), (1, 1 << 52, 211, 11, 1), (1, 1 << 52, 212, 11, 1),
              (0, full, 0, 11, 0), (0, full, 0, 11, 9)]
    cases += [(((1 << 62) - 1) << 150, 1 << 52, 0, 11, 1), ((1 << 62) << 150, 1 << 52, 0, 11, 1), ((((1 << 62) - 1) << 150) + (1 << 149), 1 << 52, 0, 11, 1)]
    return cases


def test_decision_function_equals_python_integers(exe, tmp_path):
    cases = decision_cases()
    cmds = []
    for X, m, e, logn, A in cases:
        w = X % (1 << 256)
        cmds.append("D %x %x %x %x %x %d %d %x" % (w >> 192, (w >> 128) & (2 ** 64 - 1), (w >> 64) & (2 ** 64 - 1), w & (2 ** 64 - 1), m, e, logn, A))
    lines = run(exe, tmp_path, cmds)
    seen = set()
    for (X, m, e, logn, A), ln in zip(cases, lines):
        st, p = int(ln.split()[1]), int(ln.split()[2])
        want_st, want_p = tr.decide(X, m, e, logn, A)
        assert st == want_st, (X, m, e, logn, A, st, want_st)
        if st == 0:
            assert p == want_p, (X, m, e, logn, A)
        seen.add((st, X < 0))
    assert seen >= {(0, False), (0, True), (1, False), (1, True), (2, False)}


def test_an_exact_tie_is_unproven_and_one_unit_either_side_of_the_margin_decides(exe, tmp_path):
    m, e, logn, A = 1 << 52, -10, 11, 7
    sh, M = tr.FRAC + logn - e, (1 << 52) * 7
    tie = 5 * (1 << (sh - 1))                                              # 2.5
    for d, want in [(0, (1, None)), (M, (1, None)), (-M, (1, None)), (M + m, (0, 3)), (-(M + m), (0, 2)), (M - m, (1, None)), (-(M - m), (1, None))]:
        for sign in (1, -1):
            X = sign * (tie + d) // m
            w = X % (1 << 256)
            (ln,) = run(exe, tmp_path, ["D %x %x %x %x %x %d %d %x" % (w >> 192, (w >> 128) & (2 ** 64 - 1), (w >> 64) & (2 ** 64 - 1), w & (2 ** 64 - 1), m, e, logn, A)])
            st, p = int(ln.split()[1]), int(ln.split()[2])
            assert st == want[0], (d, sign)
            if want[1] is not None:
                assert p == sign * want[1]


@pytest.fixture(scope="module")
def directed():
    """per (t0, j, K): the scales around the directed one and exactref's plaintexts at each, from ONE transform"""
    N = 4096
    out = []
    for t0, j, K in tr.DIRECTED_4096:
        s0 = tr.directed_scale(N, t0, j, K)
        scales = [tr.step(s0, u) for u in tr.ULPS]
        v = np.zeros(N // 2)
        v[t0] = 1.0
        out.append((t0, j, K, scales, exactref.encode_scaled(v, N, scales)))
    return out


def test_directed_near_ties_meet_the_conditions_on_the_reference_alone(directed):
    N = 4096
    for t0, j, K, scales, refs in directed:
        sides = set()
        for scale, (p, tie, err) in zip(scales, refs):
            flagged = {int(c) for c in np.nonzero(tie <= 2.0 ** -50)[0]}
            assert flagged == {j, N - j}, (t0, j, K, scale)
            assert tie[j] > err and tie[N - j] > err and err < 1e-50
            sides.add(abs(p[j]))
        assert sides == {K, K + 1}, (t0, j, K)                            # both roundings within one ulp either side


def test_host_coefficients_equal_exactref_on_both_sides_of_the_tie(exe, tmp_path, directed):
    N = 4096
    cmds, want = [], []
    for t0, j, K, scales, refs in directed:
        for scale, (p, tie, err) in zip(scales, refs):
            for jj in (j, N - j, 0, 1, 777, N // 2, N - 1):               # the flagged pair and coefficients far from any tie
                cmds.append(f"C 12 {jj} {tr.bits(scale):x} 1 {t0} 1")
                want.append(p[jj])
    lines = run(exe, tmp_path, cmds)
    for cmd, ln, w in zip(cmds, lines, want):
        assert ln.split()[1] == "0" and int(ln.split()[2]) == w, (cmd, ln, w)


def test_the_exact_tie_stays_unproven_and_one_ulp_either_side_resolves(exe, tmp_path):
    N, n = 4096, 2048
    v = np.zeros(n)
    v[0] = 1.0
    scales = [tr.step(n * 2.5, u) for u in (-1, 0, 1)]
    refs = exactref.encode_scaled(v, N, scales)
    assert refs[1][1][0] == 0.0                                            # the reference itself sees an exact tie at j = 0
    lines = run(exe, tmp_path, [f"C 12 0 {tr.bits(s):x} 1 0 1" for s in scales])
    assert [ln.split()[1] for ln in lines] == ["0", "1", "0"]
    assert int(lines[0].split()[2]) == refs[0][0][0] == 2 and int(lines[2].split()[2]) == refs[2][0][0] == 3
    for k in (0, 2):
        assert {int(c) for c in np.nonzero(refs[k][1] <= 2.0 ** -50)[0]} == {0} and refs[k][1][0] > refs[k][2]


def test_negative_values_dense_vectors_and_the_ceiling_of_the_sum(exe, tmp_path):
    """against Python integers on mpmath's table: the decision is the same wherever the two tables' one-unit difference cannot matter, i.e. where the Python sum is
    not within twice the margin of a tie, which is asserted"""
    cmds, want = [], []
    rnd = random.Random(5)
    for logN, scale in ((12, 2.0 ** 40 * 1.2345678901234567), (12, 3.0), (16, 2.0 ** 45), (16, float(2 ** 53 - 1) * 2.0 ** -20)):
        N = 1 << logN
        tab = tr.table(N)
        for val in (-128, 127, 1):                                         # every slot at the extreme: sum |v| = 2^7 n
            for j in (0, 1, N // 2 + 3, N - 1):
                cmds.append(f"U {logN} {j} {tr.bits(scale):x} {val}")
                want.append((tab, N, [val] * (N // 2), j, scale))
        for _ in range(3):                                                 # sparse signed vectors
            vs = {rnd.randrange(N // 2): rnd.randrange(-128, 128) for _ in range(40)}
            j = rnd.randrange(N)
            cmds.append(f"C {logN} {j} {tr.bits(scale):x} {len(vs)} " + " ".join(f"{t} {x}" for t, x in vs.items()))
            want.append((tab, N, vs, j, scale))
    lines = run(exe, tmp_path, cmds)
    for cmd, ln, (tab, N, v, j, scale) in zip(cmds, lines, want):
        X, A = tr.sum_terms(tab, N, v, j)
        m, e = tr.split_scale(scale)
        st, p = tr.decide(X, m, e, N.bit_length() - 2, 3 * A)              # three times the margin: room for the other table's unit
        if st == 1:
            continue
        assert ln.split()[1] == str(st) and (st != 0 or int(ln.split()[2]) == p), (cmd[:60], ln, st, p)
