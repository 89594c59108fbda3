"""The general ring's per-element arithmetic and host planner on the CPU (no GPU, nothing of the library linked).

tests/host/host_gring_test.cpp includes sfgwas_amd/csrc/gring_arith.hpp - the functions the kernels of gring.hip run - compiled for the host, built once with
AddressSanitizer + UBSan as a plain executable.  It runs them on directed operands at every modulus of tests/ring_cases.py; every word it prints is compared here
with Python integers, the basis extension's correction v with ksw_ref.ext_model.  The planner's launch caps, and the layout and chunk plan of the key switch's and the
rescale's workspace, are held against the executors' former size formulas and pointer arithmetic, restated here, on every level of every chain.  Six planted
mistakes must change the output of the directed operands alone.
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
        for level, np_ in DIGIT_CASES:
            f.write(f"G {level} {np_}\n")
        for c in ks_cases():
            f.write("W " + " ".join(map(str, c)) + "\n")
        for c in rescale_cases():
            f.write("Z " + " ".join(map(str, c)) + "\n")
        for n, cap in SPLIT_CASES:
            f.write(f"X {n} {cap}\n")
        for nmod in range(1, 49):
            f.write(f"U {nmod}\n")


# ---------------------------------------------------------------- the evaluator's workspaces, restated from the executors as they stood before the plans existed
BUDGET = 768 << 20                       # struct sfg_ring's default
HUGE = 1 << 60                           # a budget under which only the launch cap bounds a chunk
JOB_BYTES, KS_CAP, EW_CAP, LAUNCH_CAP = 24, 32767, 16384, 32768
DIGIT_CASES = [(level, np_) for np_ in (1, 2, 3, 4, 47) for level in (0, 1, 2, 3, 4, 7, 8, 46) if level + 1 + np_ <= 48]
SPLIT_CASES = [(0, 5), (1, 5), (4, 5), (5, 5), (6, 5), (17, 5), (32767, 32768), (32768, 32768), (32769, 32768), (3 * 32768 + 2, 32768), (16385, 16384), (32770, 32767)]
# chunk sizes of the key switch at the default budget
PINNED_KS_CHUNKS = {("G12", 0): 1638, ("G12", 1): 983, ("G13", 5): 141, ("W15", 3): 57, ("W16", 2): 39, ("L19", 16): 85, ("X12", 2): 630}
PINNED_RESCALE_CHUNK = {("G12", 1): 6144}


def ks_parent(njobs, level, np_, N, budget):
    """-> (bytes of a job, chunk, bytes reserved, [(word offset, bytes)] of the regions in order): the size formula and the separate pointer arithmetic of the
    executor before the plan, each as it was written there"""
    nl = level + 1
    nt, beta = nl + np_, (nl + np_ - 1) // np_
    per = (nl * 2 + beta * nt + 2 * nl + 2 * np_ + 2 * np_ + 2 * nl + (beta + 2 + 1) // 2 + 1) * N * 8 + JOB_BYTES
    if njobs == 0:
        return per, 0, 0, []
    J = max(1, min(min(njobs, 32767), budget // per))
    regions, p = [], 0
    for words in (J * nl * N, J * nl * N, J * beta * nt * N, J * 2 * nl * N, J * 2 * np_ * N, J * 2 * np_ * N, J * 2 * nl * N):
        regions.append((p, words * 8))
        p += words
    regions += [(p, J * beta * N * 4), (p + J * beta * N // 2, J * 2 * N * 4)]                  # V, and V2 = V + J beta N 32-bit words
    p += (J * (beta + 2) * N + 1) // 2
    regions.append((p, J * JOB_BYTES))
    return per, J, J * per + 256, regions


def rescale_parent(nct, level, N, budget):
    per = 2 * (level + 1) * N * 8
    if nct == 0:
        return per, 0, 0, []
    J = max(1, min(min(nct, 16384), budget // per))
    return per, J, J * per, [(0, J * 2 * N * 8), (J * 2 * N, J * 2 * level * N * 8)]


def item_counts(chunk, cap):
    """1, chunk - 1, chunk, chunk + 1, 3 chunk + 2 of the chunk the default budget gives (the cap bounds it where the budget does not)"""
    return sorted({n for n in (1, chunk - 1, chunk, chunk + 1, 3 * chunk + 2) if n >= 1})


def ks_cases():
    """(njobs, level, np, N, budget) on every level of every chain: the item counts around the default budget's chunk, a count above the cap under a budget that
    does not bind, and budgets below one job"""
    cases = [(0, 0, 1, 4096, BUDGET)]
    for name in rc.NAMES:
        logN, q, p = rc.chain(name)
        N, np_ = 1 << logN, len(p)
        for level in range(len(q)):
            per, chunk = ks_parent(1 << 40, level, np_, N, BUDGET)[:2]
            cases += [(n, level, np_, N, BUDGET) for n in item_counts(chunk, KS_CAP)]
            cases += [(KS_CAP + 3, level, np_, N, HUGE), (3, level, np_, N, per - 1), (2, level, np_, N, 0)]
    return cases


def rescale_cases():
    cases = [(0, 1, 4096, BUDGET)]
    for name in rc.NAMES:
        logN, q, _ = rc.chain(name)
        N = 1 << logN
        for level in range(1, len(q)):
            per, chunk = rescale_parent(1 << 40, level, N, BUDGET)[:2]
            cases += [(n, level, N, BUDGET) for n in item_counts(chunk, EW_CAP)]
            cases += [(EW_CAP + 5, level, N, HUGE), (3, level, N, per - 1), (2, level, N, 0)]
    return cases


def workspace_ok(n, cap, want, got_plan, got_offsets, got_end, spans):
    """one printed plan and layout against the restated executor (want = per, chunk, bytes, regions) and the invariants: regions in order, 8-byte aligned (offsets
    are in 64-bit words) and disjoint, the last one's end inside the reserved bytes, the chunks' counts summing to n, no chunk above its cap, a chunk of at least 1"""
    per, chunk, nbytes, regions = want
    g_per, g_chunk, g_nchunks, g_bytes = got_plan
    ok = (g_per, g_chunk, g_bytes) == (per, chunk, nbytes) and len(spans) == g_nchunks
    if n == 0:
        return ok and g_nchunks == 0
    ok = ok and 1 <= g_chunk <= cap and got_offsets == [o for o, _ in regions]
    ends = [o * 8 + b for o, b in regions]
    ok = ok and all(e <= o * 8 for e, (o, _) in zip(ends, regions[1:])) and ends[-1] == got_end * 8 and got_end * 8 <= g_bytes
    return ok and [s for s, _ in spans] == [c * g_chunk for c in range(g_nchunks)] and sum(c for _, c in spans) == n and all(1 <= c <= g_chunk for _, c in spans)


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
        elif op == "G":
            level, np_, alpha, beta, nl = v
            ok = (alpha, beta, nl) == (np_, -(-(level + 1) // np_), level + 1) and len(rc.digits(level, np_)) == beta
        elif op == "W":
            njobs, level, np_, N, budget = v[:5]
            ok = workspace_ok(njobs, KS_CAP, ks_parent(njobs, level, np_, N, budget), v[5:9], v[9:19], v[19], list(zip(v[20::2], v[21::2])))
        elif op == "Z":
            nct, level, N, budget = v[:4]
            ok = workspace_ok(nct, EW_CAP, rescale_parent(nct, level, N, budget), v[4:8], v[8:10], v[10], list(zip(v[11::2], v[12::2])))
        elif op == "X":
            n, cap = v[:2]
            spans = list(zip(v[2::2], v[3::2]))
            ok = [s for s, _ in spans] == list(range(0, n, cap)) and sum(c for _, c in spans) == n and all(1 <= c <= cap for _, c in spans)
        elif op == "U":
            nmod, launch, ew, ks, mont = v
            ok = (launch, ew, ks) == (LAUNCH_CAP, EW_CAP, KS_CAP) and mont == 32768 // nmod * nmod and mont % nmod == 0 and 0 < mont <= launch
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
    assert sum(ln[0] == "W" for ln in lines) == len(ks_cases()) and sum(ln[0] == "Z" for ln in lines) == len(rescale_cases())
    bad = mismatches(lines)
    assert not bad, [b[:300] for b in bad[:10]]
    # the chunk sizes the GPU tests of the chunk boundaries rest on, as literals: read from the line of 3 chunk + 2 items at the default budget
    printed = {tuple(ln.split()[:6]): int(ln.split()[7]) for ln in lines if ln[0] == "W"}
    for (name, level), want in PINNED_KS_CHUNKS.items():
        logN, _, p = rc.chain(name)
        assert printed[tuple(map(str, ("W", 3 * want + 2, level, len(p), 1 << logN, BUDGET)))] == want, (name, level)
    for (name, level), want in PINNED_RESCALE_CHUNK.items():
        ln = next(ln.split() for ln in lines if ln.split()[:5] == list(map(str, ("Z", 3 * want + 2, level, 1 << rc.chain(name)[0], BUDGET))))
        assert int(ln[6]) == want, (name, level)


def test_restated_executor_gives_the_pinned_chunks():
    """the Python restatement itself against the literals, so that a slip in it cannot hide one in the header"""
    for (name, level), want in PINNED_KS_CHUNKS.items():
        logN, _, p = rc.chain(name)
        assert ks_parent(1 << 40, level, len(p), 1 << logN, BUDGET)[1] == want, (name, level)
    assert rescale_parent(1 << 40, 1, 4096, BUDGET)[1] == PINNED_RESCALE_CHUNK[("G12", 1)]
    assert any(c[0] > KS_CAP for c in ks_cases()) and any(c[0] > EW_CAP for c in rescale_cases()) and any(n > cap for n, cap in SPLIT_CASES)


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
    "the last conditional subtraction dropped": ("gring_arith.hpp", "\n    return r >= q ? r - q : r;", "\n    return r;"),
    "y * fl(1/q) in place of y / q": ("gring_arith.hpp", "double d = to_double(y) / to_double(q);", "double d = to_double(y) * (1.0 / to_double(q));"),
    "truncation replaced by rounding": ("gring_arith.hpp", "GR_HD u64 ext_truncate(double vf) { return (u64)vf; }", "GR_HD u64 ext_truncate(double vf) { return (u64)(vf + 0.5); }"),
    "a region left out of the key switch's layout": ("gring_plan.hpp", "l.Y2 = c.take(J * 2 * np * N);", "l.Y2 = c.at;"),
    "the job-count cap dropped": ("gring_plan.hpp", "kGrKsJobCap, budget_bytes, kGrKsSlackBytes);", "(size_t)-1, budget_bytes, kGrKsSlackBytes);"),
    "the first item of a chunk off by one": ("gring_plan.hpp", "size_t first(size_t c) const { return c * chunk; }", "size_t first(size_t c) const { return c * chunk + 1; }"),
}


@pytest.mark.parametrize("name", list(MUTANTS))
def test_planted_mistake_is_caught_by_the_directed_operands(tmp_path, script, name):
    which, old, new = MUTANTS[name]
    inc = tmp_path / "inc"
    inc.mkdir()
    for hdr in ("gring_arith.hpp", "gring_plan.hpp"):
        text = open(os.path.join(CSRC, hdr)).read()
        if hdr == which:
            assert text.count(old) == 1, f"the line this mutant replaces is gone from {hdr}"
            text = text.replace(old, new)
        (inc / hdr).write_text(text)
    lines = run(_compile(str(tmp_path / "mutant"), str(inc), sanitize=False), script)
    assert mismatches(lines), f"not caught: {name}"


def test_headers_are_host_only():
    """both headers compile as plain C++17 and pull in no HIP header"""
    for hdr in ("gring_arith.hpp", "gring_plan.hpp"):
        deps = subprocess.run(["g++", "-std=c++17", "-x", "c++", "-M", os.path.join(CSRC, hdr)], capture_output=True, text=True)
        assert deps.returncode == 0, deps.stderr
        assert "hip" not in deps.stdout.replace(ROOT, "").lower(), deps.stdout
