"""The general ring's per-element arithmetic and host planner on the CPU (no GPU, nothing of the library linked).

tests/host/host_gring_test.cpp includes sfgwas_amd/csrc/gring_arith.hpp - the functions the kernels of gring.hip run - compiled for the host, built once with
AddressSanitizer + UBSan as a plain executable.  It runs them on directed operands at every modulus of tests/ring_cases.py; every word it prints is compared here
with Python integers, the basis extension's correction v with ksw_ref.ext_model.  Three planted mistakes must change the output of the directed operands alone.
"""
import os
import struct
import subprocess
from math import prod

import pytest

import ksw_ref
import ring_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sfgwas_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "host", "host_gring_test.cpp")


def _compile(exe, include_dir, sanitize):
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-I", include_dir, "-o", exe, SRC]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    if not sanitize or subprocess.run(base + san, capture_output=True).returncode != 0:        # no sanitizer runtimes: the plain build must still succeed
        subprocess.check_call(base)
    return exe


def ext_cases():
    """(qs, xs, qt) of the directed basis-extension elements: for every digit of every chain at its top level and for the ModDown digit P, the words X = k and
    X = D - k for small k (the float sum next to an integer, from either side), D // 2 and D // 2 + 1 (the fraction next to one half), and 0 and D - 1, each
    taken to one target inside and one outside the 50-bit range"""
    cases = []
    for name in rc.NAMES:
        _, q, p = rc.chain(name)
        groups = [[q[m] for m in dg] for dg in rc.digits(len(q) - 1, len(p))] + [list(p)]
        for qs in groups:
            others = [m for m in q + p if m not in qs]
            targets = [others[0], others[-1]] if len(others) > 1 else others
            D = prod(qs)
            ks = list(range(0, 40)) + [12345, 1 << 20]
            words = sorted({k for k in ks if k < D} | {D - k for k in ks if 0 < k <= D} | {D // 2, D // 2 + 1, D - 1})
            for X in words:
                for qt in targets:
                    cases.append((qs, [X % m for m in qs], qt))
    return cases


DOUBLES = [0, 1, (1 << 53) - 1, 1 << 53, (1 << 53) + 1, (1 << 53) + 2, (1 << 53) + 3, (1 << 54) + 2, (1 << 54) + 6, (1 << 60) + 127, (1 << 60) + 128, (1 << 60) + 129,
           (1 << 60) + 384, (1 << 61) - 1, (1 << 61) - 257, 0x1FFFFFFFFFFFFBFF, 0x1FFFFFFFFFFFFC00, 0x1FFFFFFFFFFFFC01, (1 << 64) - 1, (1 << 64) - 1024, (1 << 64) - 1025]


def write_script(path):
    with open(path, "w") as f:
        for q in rc.all_moduli():
            f.write(f"M {q}\n")
        for qs, xs, qt in ext_cases():
            f.write(f"E {len(qs)} {' '.join(map(str, qs))} {' '.join(map(str, xs))} {qt}\n")
        for y in DOUBLES + [m for m in rc.all_moduli() if m >= 1 << 53] + [m - 1 for m in rc.all_moduli() if m >= 1 << 53]:
            f.write(f"D {y}\n")
        for logN in range(10, 19):
            f.write(f"P {logN}\n")


def mismatches(lines):
    """every printed line against Python integers -> the list of lines that are wrong"""
    bad = []
    ext = iter(ext_cases())
    for ln in lines:
        t = ln.split()
        op, v = t[0], [int(x) for x in t[1:]]
        if op == "S":
            q, a, w, lazy, canon = v
            ok = lazy < 2 * q and lazy % q == a * w % q and canon == a * w % q
        elif op == "B":
            q, a, b, r = v
            ok = r == a * b % q
        elif op == "R":
            q, hi, lo, r = v
            ok = r == ((hi << 64) | lo) % q
        elif op == "F":
            q, X, Y, w, x, y = v
            ok = x < 4 * q and y < 4 * q and x % q == (X + w * Y) % q and y % q == (X - w * Y) % q
        elif op == "I":
            q, X, Y, w, x, y = v
            ok = x < 2 * q and y < 2 * q and x % q == (X + Y) % q and y % q == (X - Y) * w % q
        elif op == "C":
            q, x, r = v
            ok = r == x % q
        elif op == "A":
            q, a, b, s, d = v
            ok = s == (a + b) % q and d == (a - b) % q
        elif op == "E":
            qs, xs, qt = next(ext)
            k = len(qs)
            y, vf, _ = ksw_ref.ext_model(xs, qs)
            if k == 1:
                vf = 0                                       # a single-modulus digit is a raw copy
            ok = v[:k] == y and v[k] == vf and v[k + 1] == ksw_ref.ext_value(y, vf, qs, qt)
        elif op == "D":
            y, bits = v
            ok = bits == struct.unpack("<Q", struct.pack("<d", float(y)))[0]
        elif op == "P":
            logN, okf, a, b, col_run, chunks, tiles, stride, lds = v
            if 12 <= logN <= 16:
                ok = (okf == 1 and a + b == logN and 1 <= a <= 8 and 1 <= b <= 8 and col_run << a == 4096 and chunks << b == 4096 and stride == 1 << b
                      and tiles * 4096 == 1 << logN and tiles * col_run == 1 << b and tiles * chunks == 1 << a and col_run * 8 >= 128 and lds == 32768 and lds <= 65536)
            else:
                ok = okf == 0
        else:
            ok = op == "OK"
        if not ok:
            bad.append(ln)
    return bad


@pytest.fixture(scope="module")
def script(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("gring") / "script.txt")
    write_script(path)
    return path


def run(exe, script):
    out = subprocess.run([exe, script], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("OK"), out.stdout[-2000:] + out.stderr[-4000:]
    return out.stdout.splitlines()


def test_arithmetic_matches_python_integers_under_the_sanitizers(tmp_path, script):
    lines = run(_compile(str(tmp_path / "host_gring_test"), CSRC, sanitize=True), script)
    n_mod = len(rc.all_moduli())
    assert sum(ln[0] == "M" for ln in open(script)) == n_mod and len(lines) > 400 * n_mod
    assert sum(ln[0] == "E" for ln in lines) == len(ext_cases())
    bad = mismatches(lines)
    assert not bad, bad[:10]


def test_directed_extension_operands_reach_both_float_boundaries():
    """the directed words must contain elements whose float correction is off the exact one in both directions, elements where y * fl(1/q) would give another v
    than y / q, and elements whose sum has a fraction of at least one half - otherwise the mutants below could not be caught by them"""
    cls, recip, half = set(), 0, 0
    for qs, xs, _ in ext_cases():
        if len(qs) == 1:
            continue
        y, vf, ve = ksw_ref.ext_model(xs, qs)
        cls.add(vf - ve)
        recip += ksw_ref.ext_model(xs, qs, recip=True)[1] != vf
        half += int(sum(float(a) / float(b) for a, b in zip(y, qs)) + 0.5) != vf
    assert 1 in cls and 0 in cls and recip > 0 and half > 0, (cls, recip, half)


MUTANTS = {
    "the last conditional subtraction dropped": ("\n    return r >= q ? r - q : r;", "\n    return r;"),
    "y * fl(1/q) in place of y / q": ("double d = to_double(y) / to_double(q);", "double d = to_double(y) * (1.0 / to_double(q));"),
    "truncation replaced by rounding": ("GR_HD u64 ext_truncate(double vf) { return (u64)vf; }", "GR_HD u64 ext_truncate(double vf) { return (u64)(vf + 0.5); }"),
}


@pytest.mark.parametrize("name", list(MUTANTS))
def test_planted_mistake_is_caught_by_the_directed_operands(tmp_path, script, name):
    old, new = MUTANTS[name]
    text = open(os.path.join(CSRC, "gring_arith.hpp")).read()
    assert text.count(old) == 1, "the line this mutant replaces is gone from gring_arith.hpp"
    inc = tmp_path / "inc"
    inc.mkdir()
    (inc / "gring_arith.hpp").write_text(text.replace(old, new))
    (inc / "gring_plan.hpp").write_text(open(os.path.join(CSRC, "gring_plan.hpp")).read())
    lines = run(_compile(str(tmp_path / "mutant"), str(inc), sanitize=False), script)
    assert mismatches(lines), f"not caught: {name}"


def test_headers_are_host_only():
    """both headers compile as plain C++17 and pull in no HIP header"""
    for hdr in ("gring_arith.hpp", "gring_plan.hpp"):
        deps = subprocess.run(["g++", "-std=c++17", "-x", "c++", "-M", os.path.join(CSRC, hdr)], capture_output=True, text=True)
        assert deps.returncode == 0, deps.stderr
        assert "hip" not in deps.stdout.replace(ROOT, "").lower(), deps.stdout
