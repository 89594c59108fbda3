"""The key switch's writer-side forward stage 1 (sfgwas_amd/csrc/fp64mod.hpp fwd_stage1_pair: r_x = v0 + W v1, r_(x + N/2) = v0 - W v1, both canonical) and
canon() underneath it, on the CPU (no GPU, nothing of the library linked) for every modulus of PN14QP438 and of the chains S1, S3 and S4 of tests/ksw_ref.py -
the moduli whose canon() fix-up fires (0x7fffb0001, 0x7fffffc48001, 0x7fffffda0001) among them.

tests/host/host_ksw_split_test.cpp includes the header - the functions the kernels run - compiled for the host with AddressSanitizer + UBSan as a plain
executable; it compares each result with 128-bit integers itself, and every word it prints is compared here with Python integers once more."""
import os
import subprocess

import numpy as np
import pytest

from sfgwas_amd.params import P_PN14, Q_PN14

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sfgwas_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "host", "host_ksw_split_test.cpp")

# the chains of tests/ksw_ref.py (that module loads the oracle, which this file does not need); test_the_chains_are_ksw_refs checks the copy where it can
S1 = ([0x7fffb0001, 0x7fff80001, 0x800280001, 0x7ffd80001, 0x7ffc80001, 0x7ff9c0001, 0x800008001, 0x8000f8001, 0x800250001], [0x80000050001])
S3 = ([0x7fffb0001] + Q_PN14[1:7], P_PN14 + [0x7ffffffc8001])
S4 = ([0x7fffffda0001, 0x7fffffc48001, 0x7ffffffc8001, 0x7ffffff00001, 0x7fffffe70001, 0x7fffffe48001, 0x7fffffe40001, 0x7fffffd08001],
      [0x7fffffc80001, 0x7fffffc18001, 0x7fffffbc0001, 0x7fffffbb8001])
MODULI = sorted(set(Q_PN14 + P_PN14 + S1[0] + S1[1] + S3[0] + S3[1] + S4[0] + S4[1]))
ARM_MODULI = [0x7fffb0001, 0x7fffffc48001, 0x7fffffda0001]


def ARM(q):
    """tests/ksw_ref.py ARM: canon()'s equality fix-up is reachable for q"""
    return float(q) * (1.0 / float(q)) < 1.0


def sqrt_minus_one(q):
    """psi^(N/2) for a primitive 2N-th root psi is a square root of -1: both of them, whichever root the tables hold"""
    a = 2
    while pow(a, (q - 1) // 2, q) != q - 1:
        a += 1
    w = pow(a, (q - 1) // 4, q)
    assert w * w % q == q - 1
    return [w, q - w]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("ksw_split") / "host_ksw_split_test")
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-I", CSRC, "-o", out, SRC]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    if subprocess.run(base + san, capture_output=True).returncode != 0:        # no sanitizer runtimes: the plain build must still succeed
        subprocess.check_call(base)
    return out


def run(exe, lines, tmp_path):
    script = tmp_path / "script.txt"
    script.write_text("\n".join(lines) + "\n")
    out = subprocess.run([exe, str(script)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    rows = out.stdout.split("\n")
    assert rows[-2] == "OK" and len(rows) == len(lines) + 2
    return [r.split() for r in rows[:-2]]


def test_the_moduli_and_their_fixup_predicate():
    assert all(q % (1 << 15) == 1 and q < 1 << 47 for q in MODULI)
    assert [q for q in MODULI if ARM(q)] == ARM_MODULI


def test_the_chains_are_ksw_refs():
    import ksw_ref as kr
    assert (kr.S1[0], kr.S1[1]) == S1 and (kr.S3[0], kr.S3[1]) == S3 and (kr.S4[0], kr.S4[1]) == S4


def pair_values(q, w, rnd):
    d = [0, 1, 2, q - 1, q - 2, q // 2, q // 2 + 1]
    pairs = [(a, b) for a in d for b in d]
    for b in d[1:] + [int(x) for x in rnd.integers(1, q, 40)]:
        pairs.append(((-w * b) % q, b))            # v0 + W v1 is a multiple of q: r0 = 0 through the fix-up where it is reachable
        pairs.append(((w * b) % q, b))             # v0 - W v1 is
    pairs += [(int(a), int(b)) for a, b in rnd.integers(0, q, (200, 2))]
    return pairs


@pytest.mark.parametrize("q", MODULI, ids=hex)
def test_forward_stage_one_by_the_writer(exe, tmp_path, q):
    rnd = np.random.default_rng(q % 1000003)
    lines, want = [], []
    for w in sqrt_minus_one(q) + [0, 1, q - 1, int(rnd.integers(2, q))]:
        for v0, v1 in pair_values(q, w, rnd):
            lines.append(f"S {q} {w} {v0} {v1}")
            want.append(((v0 + w * v1) % q, (v0 - w * v1) % q))
    rows = run(exe, lines, tmp_path)
    zeros = 0
    for r, (w0, w1) in zip(rows, want):
        assert (int(r[5]), int(r[6])) == (w0, w1) == (int(r[7]), int(r[8])), r
        zeros += (w0 == 0) + (w1 == 0)
    assert zeros >= 6 * 2 * 46                       # the directed multiples of q were there


@pytest.mark.parametrize("q", MODULI, ids=hex)
def test_canon_at_multiples_of_q(exe, tmp_path, q):
    """k q and its neighbours for the k the stage-1 sums and the summed finish reach (|x| < 2^51)"""
    ks = [k for k in (0, 1, 2, 3, 7, 10, 11, 15) if k * q + 1 < 1 << 51]
    xs = [s * (k * q + e) for k in ks for e in (-1, 0, 1) for s in (1, -1)]
    rows = run(exe, [f"C {q} {x}" for x in xs], tmp_path)
    for r, x in zip(rows, xs):
        assert int(r[3]) == x % q == int(r[4]), r
