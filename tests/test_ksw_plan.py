"""The key switch's job planning (sfgwas_amd/csrc/ksw_plan.hpp: how many inputs a group and how many jobs a chunk holds under a scratch budget, where the
regions of the workspace lie, which jobs fall into which input group, chunk and tile, tiles of jobs under one key and one automorphism table, and the segments of a
summed finish) on the CPU, no GPU and nothing of the library linked.

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


# ---------------------------------------------------------------------------------------------------- sizes and the workspace layout
N14 = 16384
MIB, GIB = 1 << 20, 1 << 30
LEVEL5, LEVEL4 = (6, 2, 8, 3), (5, 2, 7, 3)                  # nl, np, nt, beta on PN14


def sizes(shape, nin, nr, nout, budget, N=N14):
    """in_grp, chunk, the row counts, the six row regions in words, the seven tables in bytes, the total"""
    nl, np_, nt, beta = shape
    in_grp = min(max(budget // ((nl + beta * nt) * N * 8), 1), nin)
    chunk = min(max(budget // ((2 * nt + 2 * nl) * N * 8), 1), nr)      # cut as when a job's accumulator held all 2 nt rows
    ext_rows, ext2_rows, acc_rows = in_grp * beta * nt, chunk * 2 * nl, chunk * 2 * np_
    words, at = [], 0
    for rows in [in_grp * nl, ext_rows, acc_rows, ext2_rows, ext_rows, ext2_rows]:          # c2 ext acc ext2 extT ext2T
        words.append(at)
        at += rows * N
    tables, at = [], at * 8
    for size in [nr * 8, nr * 8, nr * 8, nout * 32, nr * 4, nr * 4, nr * 8]:                # keys idx out segs inidx segjobs tiles
        tables.append(at)
        at += size
    return (in_grp, chunk, ext_rows, ext2_rows, acc_rows), words, tables, at + 256


def closed_form(shape, in_grp, chunk, nr, nout, N=N14):
    """the bytes the launcher reserved before it had a plan"""
    nl, np_, nt, beta = shape
    in_rows, ext_rows, ext2_rows, acc_rows = nl + beta * nt, in_grp * beta * nt, chunk * 2 * nl, chunk * 2 * np_
    return (in_rows * in_grp + acc_rows + 2 * ext2_rows + ext_rows) * N * 8 + nr * (3 * 8 + 2 * 4 + 8) + nout * 32 + 256


def fmt_s(shape, nin, nr, nout, budget, N=N14):
    return f"S {shape[0]} {shape[1]} {shape[2]} {shape[3]} {nin} {nr} {nout} {budget} {N}"


def want_s(shape, nin, nr, nout, budget, N=N14):
    head, words, tables, total = sizes(shape, nin, nr, nout, budget, N)
    return " | ".join([" ".join(map(str, ("S",) + head)), " ".join(map(str, words)), " ".join(map(str, tables)), str(total)])


# (shape, budget, nin, nr, nout) -> (in_grp, chunk)
SIZE_CASES = [((LEVEL5, 16 * MIB, 1000, 1000, 0), (4, 4)),                # 128 rows over 30 and 28
              ((LEVEL4, 16 * MIB, 1000, 1000, 0), (4, 5)),                # 128 rows over 26 and 24
              ((LEVEL5, 4 * GIB, 6, 546, 0), (6, 546)),                   # clamped by the counts
              ((LEVEL5, 4 * GIB, 2000, 2000, 15), (1092, 1170)),          # clamped by the budget
              ((LEVEL5, 30 * N14 * 8 - 1, 7, 9, 0), (1, 1)),              # less than one input's rows
              ((LEVEL4, 0, 1, 1, 3), (1, 1)),
              ((LEVEL5, 4 * GIB, 3, 0, 2), (3, 0)),                       # a sum with outputs and no job
              ((LEVEL4, 16 * MIB, 3, 0, 2), (3, 0)),
              ((LEVEL5, 4 * GIB, 0, 0, 0), (0, 0)),
              ((LEVEL4, 16 * MIB, 0, 0, 1), (0, 0))]


def test_sizes_and_layout_at_the_named_budgets(exe, tmp_path):
    rows = run(exe, [fmt_s(sh, nin, nr, nout, budget) for (sh, budget, nin, nr, nout), _ in SIZE_CASES], tmp_path)
    for row, ((sh, budget, nin, nr, nout), (in_grp, chunk)) in zip(rows, SIZE_CASES):
        assert row == want_s(sh, nin, nr, nout, budget)
        assert row.split()[1:3] == [str(in_grp), str(chunk)], row
        assert int(row.split()[-1]) == closed_form(sh, in_grp, chunk, nr, nout)


def test_random_sizes_and_layouts(exe, tmp_path):
    """any shape the key switch accepts (np <= 4 primes per digit, beta <= 8 digits), any row length, budgets around the sizes of one input and one job"""
    rnd = np.random.default_rng(7)
    cases = []
    for _ in range(300):
        np_ = int(rnd.integers(1, 5)); nl = int(rnd.integers(1, 8 * np_ + 1)); shape = (nl, np_, nl + np_, -(-nl // np_))
        N = 1 << int(rnd.integers(4, 17))
        nin, nr, nout = int(rnd.integers(0, 40)), int(rnd.integers(0, 200)), int(rnd.integers(0, 16))
        budget = int(rnd.integers(0, 50)) * (nl + shape[3] * shape[2]) * N * 8 // int(rnd.integers(1, 5)) + int(rnd.integers(0, 3))
        cases.append((shape, nin, nr, nout, budget, N))
    rows = run(exe, [fmt_s(*c) for c in cases], tmp_path)
    for row, c in zip(rows, cases):
        assert row == want_s(*c)
        assert int(row.split()[-1]) == closed_form(c[0], int(row.split()[1]), int(row.split()[2]), c[2], c[3], c[5])


# ---------------------------------------------------------------------------------------------------- jobs -> input groups, chunks, tiles
def groups_of(jobs, nin, in_grp, chunk, T):
    """jobs: [(input, key, table)].  Per run of in_grp inputs with a job: its jobs in list order, cut into chunks, each chunk into tiles of its own numbering"""
    out = []
    for i0 in range(0, nin, in_grp) if in_grp > 0 and chunk > 0 else []:
        ni = min(in_grp, nin - i0)
        mine = [k for k, (i, _, _) in enumerate(jobs) if i0 <= i < i0 + ni]
        if mine:
            out.append((i0, ni, mine, [(c0, len(mine[c0:c0 + chunk]), job_tiles([jobs[k][1:] for k in mine[c0:c0 + chunk]], T)) for c0 in range(0, len(mine), chunk)]))
    return out


def fmt_g(jobs, nin, in_grp, chunk, T):
    return f"G {T} {in_grp} {chunk} {nin} {len(jobs)}" + "".join(f" {i} {k} {t}" for i, k, t in jobs)


def want_g(jobs, nin, in_grp, chunk, T):
    gs = groups_of(jobs, nin, in_grp, chunk, T)
    out = f"G {len(gs)}"
    for i0, ni, mine, chunks in gs:
        out += f" | {i0} {ni} {len(mine)}" + "".join(f" {k}" for k in mine) + f" ; {len(chunks)}"
        for c0, nb, tl in chunks:
            out += f" , {c0} {nb} {len(tl)}" + "".join(f" {a} {c}" for a, c in tl)
    return out


def runs_39():
    """the 39-job list of tests/test_gpu_ksw_inner_finish.py: key a x 1, b x 2, a x 3, b x 4, a x 5, b x 6, a x 7, b x 11"""
    a, b = (10, 100), (20, 200)
    return [(b if k & 1 else a) for k, n in enumerate([1, 2, 3, 4, 5, 6, 7, 11]) for _ in range(n)]


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("in_grp,chunk", [(4, 4), (4, 5), (39, 39), (1, 1)])
def test_the_runs_list_in_groups_and_chunks(exe, tmp_path, T, in_grp, chunk):
    """job j over 4 and 5 inputs (j mod nin: every group's list is a sieve of the runs) and over 39 (its own input: list order is input order)"""
    keys = runs_39()
    lines, want = [], []
    for nin in (4, 5, 39):
        g = min(in_grp, nin)                                            # as the sizes clamp it
        jobs = [(j % nin,) + keys[j] for j in range(39)]
        lines.append(fmt_g(jobs, nin, g, chunk, T)); want.append(want_g(jobs, nin, g, chunk, T))
    assert run(exe, lines, tmp_path) == want
    # spelled out once: 39 inputs in groups of 4 at chunks of 4 - ten groups, the last of 3; group 0 holds jobs 0 .. 3 = a, b, b, a
    if (in_grp, chunk, T) == (4, 4, 3):
        assert want[2].startswith("G 10 | 0 4 4 0 1 2 3 ; 1 , 0 4 3 0 1 1 2 3 1 | 4 4 4 4 5 6 7 ; 1 , 0 4 2 0 2 2 2 |")
        assert want[2].endswith("| 36 3 3 36 37 38 ; 1 , 0 3 1 0 3")
    if (in_grp, chunk, T) == (1, 1, 3):
        assert want[0].count("|") == 4 and all(f" , {c} 1 1 0 1" in want[0] for c in range(9))


def test_descending_inputs_and_inputs_without_a_job(exe, tmp_path):
    a, b = (10, 100), (20, 200)
    desc = [(i,) + (a if i & 2 else b) for i in range(11, -1, -1)]      # inputs 11 .. 0: the groups come in input order, each with its jobs in list order
    gaps = [(i,) + a for i in (9, 9, 0, 9, 1, 0)]                       # inputs 2 .. 8 and 10, 11 have no job: at groups of 2, only groups 0 and 8 exist
    lines = [fmt_g(desc, 12, 5, 3, 3), fmt_g(gaps, 12, 2, 2, 3), fmt_g(gaps, 12, 12, 6, 2), fmt_g([], 3, 3, 0, 3), fmt_g([], 0, 0, 0, 3)]
    want = [want_g(desc, 12, 5, 3, 3), want_g(gaps, 12, 2, 2, 3), want_g(gaps, 12, 12, 6, 2), "G 0", "G 0"]
    assert run(exe, lines, tmp_path) == want
    assert want[0] == "G 3 | 0 5 5 7 8 9 10 11 ; 2 , 0 3 2 0 1 1 2 , 3 2 1 0 2 | 5 5 5 2 3 4 5 6 ; 2 , 0 3 2 0 2 2 1 , 3 2 2 0 1 1 1 | 10 2 2 0 1 ; 1 , 0 2 1 0 2"
    assert want[1] == "G 2 | 0 2 3 2 4 5 ; 2 , 0 2 1 0 2 , 2 1 1 0 1 | 8 2 3 0 1 3 ; 2 , 0 2 1 0 2 , 2 1 1 0 1"


def test_random_groupings(exe, tmp_path):
    rnd = np.random.default_rng(8)
    lines, want = [], []
    for _ in range(300):
        nin, nr, T = int(rnd.integers(1, 13)), int(rnd.integers(0, 61)), int(rnd.choice(TS))
        nk = int(rnd.integers(1, 4))
        jobs = sorted([(int(rnd.integers(0, nin)), int(rnd.integers(0, nk)), int(rnd.integers(0, 2))) for _ in range(nr)], key=lambda j: j[1]) if rnd.integers(0, 2) else \
            [(int(rnd.integers(0, nin)), int(rnd.integers(0, nk)), int(rnd.integers(0, 2))) for _ in range(nr)]
        in_grp, chunk = int(rnd.integers(1, nin + 1)), (int(rnd.integers(1, nr + 1)) if nr else 0)
        lines.append(fmt_g(jobs, nin, in_grp, chunk, T)); want.append(want_g(jobs, nin, in_grp, chunk, T))
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
