"""The key switch's job planning (sfgwas_amd/csrc/ksw_plan.hpp: tiles of jobs under one key and one automorphism table, and the segments of a summed finish)
on the CPU, no GPU and nothing of the library linked.

tests/host/host_ksw_plan_test.cpp includes the header - the functions rotate.hip calls - compiled for the host with AddressSanitizer + UBSan as a plain
executable; it checks the covering invariants itself on every call, and every line it prints is compared here with a literal restatement in Python.

Tiles of segments for the summed finish were measured and not kept (profiles/ksw_inner_finish_ab.txt): the planner has none.

The same executable runs fp64mod.hpp inv_last_pair - the last stage and the 1/N of the key switch's split inverse transform, done by the rows' readers - with
the constants formed as the kernels form them, for every PN14 modulus, the special primes and the three moduli whose canon() fix-up fires."""
import os
import subprocess

import numpy as np
import pytest

from sfgwas_amd.params import P_PN14, Q_PN14

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sfgwas_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "host", "host_ksw_plan_test.cpp")
TS = [1, 2, 3, 5]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("ksw_plan") / "host_ksw_plan_test")
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
    return rows[:-2]


# ---------------------------------------------------------------------------------------------------- the literal restatement
def job_tiles(jobs, T):
    """jobs: [(key, table)]; maximal runs of equal consecutive pairs, each cut into pieces of at most T"""
    runs, k = [], 0
    while k < len(jobs):
        e = k
        while e < len(jobs) and jobs[e] == jobs[k]:
            e += 1
        runs.append((k, e))
        k = e
    return [(a, min(T, e - a)) for k, e in runs for a in range(k, e, T)]


def segments(groups, nout, seen):
    """one segment per output with a job in the chunk (no job at all: per output nobody has written), its jobs in chunk order"""
    segs, segjobs = [], []
    for i in range(nout):
        mine = [k for k, g in enumerate(groups) if g == i]
        if (not mine) if groups else seen[i]:
            continue
        segs.append((i, len(segjobs), len(mine), 0 if seen[i] else 1))
        segjobs += mine
        seen[i] = True
    return segs, segjobs


def fmt_j(T, jobs):
    return f"J {T} {len(jobs)} " + " ".join(f"{k} {t}" for k, t in jobs)


def want_j(jobs, T):
    tl = job_tiles(jobs, T)
    return " ".join([f"J {len(tl)}"] + [f"{a} {c}" for a, c in tl])


def fmt_c(groups):
    return f"C {len(groups)} " + " ".join(str(g) for g in groups)


def want_c(groups, nout, seen):
    segs, segjobs = segments(groups, nout, seen)
    return " ".join([f"C {len(segs)}"] + [f"{o} {s} {c} {f}" for o, s, c, f in segs]) + " |" + "".join(f" {j}" for j in segjobs)


# ---------------------------------------------------------------------------------------------------- tiles of jobs
def job_lists(T):
    a, b, c = (10, 100), (20, 200), (30, 300)
    lists = {"empty": [],
             "runs of 1, 2, T, T + 1, 2T + 1": [a] + [b] * 2 + [c] * T + [a] * (T + 1) + [b] * (2 * T + 1),
             "interleaved keys": [a, b, a, b, a],
             "one key, another table": [a, a, (10, 101), (10, 101), a],
             "one table, another key": [a, (11, 100), a],
             "every job its own key": [(k, k) for k in range(7)]}
    return lists


@pytest.mark.parametrize("T", TS)
def test_job_tiles_against_the_restatement(exe, tmp_path, T):
    lists = job_lists(T)
    rows = run(exe, [fmt_j(T, jobs) for jobs in lists.values()], tmp_path)
    for (name, jobs), row in zip(lists.items(), rows):
        assert row == want_j(jobs, T), name
    # and what the restatement says about the named cases, spelled out once
    assert job_tiles(lists["interleaved keys"], T) == [(k, 1) for k in range(5)]
    assert job_tiles(lists["every job its own key"], T) == [(k, 1) for k in range(7)]
    assert job_tiles([(1, 1)] * (2 * T + 1), T) == [(0, T), (T, T), (2 * T, 1)]
    if T > 1:
        assert job_tiles(lists["one key, another table"], T) == [(0, 2), (2, 2), (4, 1)]


@pytest.mark.parametrize("T", TS)
def test_a_run_cut_by_a_chunk_boundary(exe, tmp_path, T):
    """the planner sees one chunk at a time: a run of 2T + 1 jobs that a chunk boundary cuts after T + 1 gives the tiles of T + 1 and of T jobs"""
    run_ = [(5, 50)] * (2 * T + 1)
    rows = run(exe, [fmt_j(T, run_[:T + 1]), fmt_j(T, run_[T + 1:])], tmp_path)
    assert rows == [want_j(run_[:T + 1], T), want_j(run_[T + 1:], T)]
    assert job_tiles(run_[:T + 1], T) == [(0, T)] + [(T, 1)] and sum(c for _, c in job_tiles(run_[T + 1:], T)) == T


def test_random_job_lists(exe, tmp_path):
    rnd = np.random.default_rng(5)
    cases = []
    for _ in range(200):
        T = int(rnd.integers(1, 7)); nb = int(rnd.integers(0, 40)); nk = int(rnd.integers(1, 4))
        cases.append((T, [(int(rnd.integers(0, nk)), int(rnd.integers(0, 2))) for _ in range(nb)]))
    rows = run(exe, [fmt_j(T, jobs) for T, jobs in cases], tmp_path)
    assert rows == [want_j(jobs, T) for T, jobs in cases]


# ---------------------------------------------------------------------------------------------------- segments of a summed finish
def alignment_groups(s, ngiants):
    """the giant-step alignment's list: key-major, the s jobs of one giant go to outputs 0 .. s - 1"""
    return [i for _ in range(ngiants) for i in range(s)]


@pytest.mark.parametrize("s", [1, 2, 3, 4, 7])
def test_alignment_chunks_against_the_restatement(exe, tmp_path, s):
    """three giants of s outputs each, cut into chunks of 1, 2, s, s + 1, 5 and all jobs (an output's jobs straddle chunk boundaries), then the closing call"""
    groups = alignment_groups(s, 3)
    lines, want = [], []
    for chunk in sorted({1, 2, s, s + 1, 5, len(groups)}):
        lines.append(f"R {s + 1}"); want.append("R")                           # output s has no job: only the closing call makes its segment
        seen = [False] * (s + 1)
        for c0 in range(0, len(groups), chunk):
            lines.append(fmt_c(groups[c0:c0 + chunk])); want.append(want_c(groups[c0:c0 + chunk], s + 1, seen))
        lines.append(fmt_c([])); want.append(want_c([], s + 1, seen))
        assert want[-1] == f"C 1 {s} 0 0 1 |"                                  # the output without a job, once, as a first write
        lines.append(fmt_c([])); want.append(want_c([], s + 1, seen))
        assert want[-1] == "C 0 |"
    assert run(exe, lines, tmp_path) == want


def test_first_and_later_segments_of_an_output():
    """an output's first segment is marked first (it takes the plain member and obeys the caller's accumulate flag), the later ones are not"""
    seen = [False] * 2
    assert segments([0, 1, 0], 2, seen) == ([(0, 0, 2, 1), (1, 2, 1, 1)], [0, 2, 1])
    assert segments([1], 2, seen) == ([(1, 0, 1, 0)], [0])
    assert segments([], 2, seen) == ([], [])


def test_random_sums(exe, tmp_path):
    rnd = np.random.default_rng(6)
    lines, want = [], []
    for _ in range(100):
        nout = int(rnd.integers(1, 6))
        lines.append(f"R {nout}"); want.append("R")
        seen = [False] * nout
        for _ in range(int(rnd.integers(0, 4))):
            nb = int(rnd.integers(1, 12))                                       # (an empty chunk is the closing call: last)
            groups = [int(rnd.integers(0, nout)) for _ in range(nb)]
            lines.append(fmt_c(groups)); want.append(want_c(groups, nout, seen))
        lines.append(fmt_c([])); want.append(want_c([], nout, seen))
    assert run(exe, lines, tmp_path) == want


# ---------------------------------------------------------------------------------------------------- the last inverse stage by the reader
PAIR_MODULI = sorted(set(Q_PN14 + P_PN14 + [0x7fffb0001, 0x7fffffda0001, 0x7fffffc48001]))


def sqrt_minus_one(q):
    """psi^-(N/2) for a primitive 2N-th root psi is a square root of -1: both of them, whichever root the tables hold"""
    a = 2
    while pow(a, (q - 1) // 2, q) != q - 1:
        a += 1
    w = pow(a, (q - 1) // 4, q)
    assert w * w % q == q - 1
    return [w, q - w]


@pytest.mark.parametrize("q", PAIR_MODULI, ids=hex)
def test_inv_last_pair_is_the_last_stage_and_the_scaling(exe, tmp_path, q):
    """(U, V) -> ((U + V) / N, (U - V) w / N) mod q in Python integers: the one-workgroup transform's last Gentleman-Sande stage followed by its 1/N"""
    rnd = np.random.default_rng(q % 1000003)
    ninv = pow(1 << 14, -1, q)
    a = int(rnd.integers(1, q))
    pairs = [(0, 0), (q - 1, q - 1), (a, a), (a, q - a), (0, a), (a, 0)] + [(int(u), int(v)) for u, v in rnd.integers(0, q, (10000, 2))]
    lines, want = [], []
    for w in sqrt_minus_one(q):
        for u, v in pairs:
            lines.append(f"P {q} {w} {u} {v}")
            want.append(((u + v) * ninv % q, (u - v) * w * ninv % q))
    rows = [r.split() for r in run(exe, lines, tmp_path)]
    for r, (w0, w1) in zip(rows, want):
        assert (int(r[1]), int(r[2])) == (w0, w1) == (int(r[3]), int(r[4])), r
