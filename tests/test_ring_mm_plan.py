"""The host-only plan of the general ring's matrix products (sfgwas_amd/csrc/gring_matmul_plan.hpp) on the CPU, and the expectation the GPU tests use.

tests/host/host_gring_mm_test.cpp includes the plan header alone, built once with AddressSanitizer + UBSan as a plain executable (a plain build where the
runtimes are absent), and prints what its functions give; every figure is compared here with a literal Python restatement: the shift tables with the oracle's loop
through orc_get_diag_bool, fold_terms and the folded sum with Python integers, the layout as a partition of the reserve, the chunk plans as exact partitions.
The last test holds the range-sum expectation of tests/ring_mm_cases.py against the oracle's whole product where the oracle's 128-bit sum wraps."""
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as ol
import ring_cases as rc
import ring_mm_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sfgwas_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "host", "host_gring_mm_test.cpp")
SLOTS = 2048


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("mm") / "host_gring_mm_test")
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


def shape_pairs():
    """(rows, cols) of the operand: an exhaustive small range, the directed sums around `slots`, single rows and columns, several blocks either way"""
    pairs = [(r, c) for r in range(1, 7) for c in range(1, 7)]
    pairs += [(r, SLOTS - r) for r in (1, 2, 45, 46, 47, 1024, 2047)] + [(r, SLOTS + 1 - r) for r in (1, 2, 46, 1024, 2047, 2048)]
    pairs += [(1, 300), (300, 1), (1, 2048), (2048, 1), (2048, 2048), (100, 100), (2078, 2065), (4097, 3), (3, 4097), (2049, 2047)]
    return pairs


def test_shift_tables_equal_the_oracles_loop_in_both_orientations(exe, tmp_path):
    cmds, want = [], []
    for rows, cols in shape_pairs():
        for r_, c_ in ((rows, cols), (cols, rows)):                       # the transposed view swaps the operand's rows and columns
            for bi in range(mc.blocks(r_, SLOTS)):
                cmds.append(f"S {r_} {c_} {SLOTS} {bi}")
                want.append(mc.shift_tables(r_, c_, SLOTS, bi))
    lines = run(exe, tmp_path, cmds)
    assert len(lines) == len(cmds)
    for cmd, ln, (baby, giant, shift) in zip(cmds, lines, want):
        f = ln.split()
        assert f[0] == "S" and int(f[5]) == 46
        assert f[1] == "".join(map(str, baby)) and f[2] == "".join(map(str, giant)) and f[3] == "".join(map(str, shift)), cmd


def test_the_full_block_has_45_giants_and_the_last_holds_24_babies(exe, tmp_path):
    baby, giant, shift = mc.shift_tables(2048, 2048, SLOTS, 0)
    assert shift.all() and baby.all() and giant[:45].all() and not giant[45] and 46 * 46 > 2048 and 2048 - 44 * 46 == 24
    (ln,) = run(exe, tmp_path, [f"S 2048 2048 {SLOTS} 0"])
    assert ln.split()[2] == "1" * 45 + "0"


def test_d_is_the_ceiling_of_the_square_root_at_every_ring_size(exe, tmp_path):
    lines = run(exe, tmp_path, [f"D {1 << k}" for k in range(11, 16)])
    assert [int(ln.split()[1]) for ln in lines] == [46, 64, 91, 128, 182] == [mc.d_of(1 << k) for k in range(11, 16)]


def test_rotation_list_is_the_active_babies_then_the_active_giants(exe, tmp_path):
    shapes = [(100, 100), (2078, 2065), (1, 300), (300, 1), (2048, 2048), (20, 30)]
    lines = run(exe, tmp_path, [f"R {r} {c} {SLOTS} 0 {mc.blocks(r, SLOTS)} 1 1" for r, c in shapes])
    for (r, c), ln in zip(shapes, lines):
        assert [int(x) for x in ln.split()[1:]] == mc.rotations(r, c, SLOTS), (r, c)
    full, _ = ol.needed_rotations(SLOTS, 2048, 2048)
    assert sorted(mc.rotations(2048, 2048, SLOTS)) == full                 # on a full block: what oracle_lib.needed_rotations lists
    (b_only,), (g_only,) = run(exe, tmp_path, [f"R 100 100 {SLOTS} 0 1 1 0"]), run(exe, tmp_path, [f"R 100 100 {SLOTS} 0 1 0 1"])
    both = mc.rotations(100, 100, SLOTS)
    assert [int(x) for x in b_only.split()[1:]] == [k for k in both if k < 46] and [int(x) for x in g_only.split()[1:]] == [k for k in both if k >= 46]


def fold_moduli():
    return rc.all_moduli() + [(1 << 61) - 1, ol.small_primes(12, 30, 1)[0]]


def test_fold_terms_equals_python_integers(exe, tmp_path):
    qs = fold_moduli()
    lines = run(exe, tmp_path, [f"F {q}" for q in qs])
    for q, ln in zip(qs, lines):
        assert int(ln.split()[1]) == min(mc.fold_terms(q), 0xFFFFFFFF), q
        assert (q - 1) + mc.fold_terms(q) * (q - 1) ** 2 < 1 << 128 <= (q - 1) + (mc.fold_terms(q) + 1) * (q - 1) ** 2 + 1
    assert mc.fold_terms(rc.chain("X12")[1][0]) == 64 and mc.fold_terms(rc.chain("W16")[1][0]) >= 1 << 18


def test_folded_sum_is_the_exact_sum_and_a_late_or_missing_fold_is_not(exe, tmp_path):
    """the kernel's walk (MmSum, mm_sum_terms) on near-maximal words: exact with the plan's bound for up to three folds; one term late, or no fold, wraps"""
    wide = [q for q in fold_moduli() if q.bit_length() == 61]
    cmds, want = [], []
    for q in wide:
        f = mc.fold_terms(q)
        for n in (1, f, f + 1, 2 * f, 2 * f + 1, 3 * f + 5, 182 * 3):
            cmds.append(f"A {q} {f} {n}")
            want.append(sum((q - 1 - k % 5) * (q - 1 - k % 3) for k in range(n)) % q)
    lines = run(exe, tmp_path, cmds)
    assert [int(ln.split()[1]) for ln in lines] == want
    for q in wide:
        f = mc.fold_terms(q)
        n = 3 * f + 5
        exact = sum((q - 1 - k % 5) * (q - 1 - k % 3) for k in range(n)) % q
        late, never = run(exe, tmp_path, [f"A {q} {f + 1} {n}", f"A {q} {1 << 40} {n}"])
        assert int(late.split()[1]) != exact and int(never.split()[1]) != exact, q


def plan_cases():
    """(s, d, nl, L, m_ct, N, with_acc) at the tests' shapes and at W16's and PN16's"""
    return [(2, 46, 2, 1, 1, 4096, True), (1, 46, 3, 2, 2, 4096, True), (3, 64, 4, 3, 1, 8192, False), (15, 182, 3, 3, 1, 65536, True), (8, 182, 35, 34, 2, 65536, True),
            (5, 128, 4, 3, 1, 32768, False)]


REGIONS = ["rot", "acc", "dft", "pt", "vecs", "first", "jobs", "glist", "sums", "band", "flags"]


def region_words(d, nl, L, m_ct, N, sc, vc, with_acc):
    return [sc * d * 2 * nl * N, m_ct * d * sc * 2 * L * N if with_acc else 0, vc * (N // 2) * 4, vc * L * N, vc * 2, (m_ct + 2) // 2, sc * d * 3, (d + 1) // 2,
            (vc + 1) // 2, vc, 1]


def test_layout_is_a_partition_and_its_end_is_the_reserve(exe, tmp_path):
    for s, d, nl, L, m_ct, N, with_acc in plan_cases():
        for budget in (1, 64 << 20, 768 << 20, 1 << 40):
            head, *_ = run(exe, tmp_path, [f"P {s} {d} {nl} {L} {m_ct} {N} {int(with_acc)} {budget} {d * m_ct}"])
            sc, nsc, vc, nbytes = (int(x) for x in head.split()[1:])
            (lay,) = run(exe, tmp_path, [f"L {d} {nl} {L} {m_ct} {N} {sc} {vc} {int(with_acc)}"])
            off = [int(x) for x in lay.split()[1:]]
            sizes = region_words(d, nl, L, m_ct, N, sc, vc, with_acc)
            assert off[0] == 0
            for k in range(len(REGIONS)):
                assert off[k] + sizes[k] == off[k + 1], (REGIONS[k], s, d, budget)   # each region ends where the next begins: no overlap, no hole
            assert nbytes == off[-1] * 8 + 256
            # what each region must hold: 32-bit tables fit their words
            assert sizes[5] * 2 >= m_ct + 1 and sizes[7] * 2 >= d and sizes[8] * 2 >= vc and sizes[4] * 8 == vc * 16 and sizes[6] * 8 == sc * d * 24


def test_chunk_plans_are_exact_partitions_under_the_budget(exe, tmp_path):
    seen = set()
    for s, d, nl, L, m_ct, N, with_acc in plan_cases():
        per_ct = (d * 2 * nl * N + (m_ct * d * 2 * L * N if with_acc else 0) + 3 * d) * 8
        per_vec = ((N // 2) * 4 + L * N + 4) * 8
        nd = d * m_ct
        for budget in (1, 6 * per_vec, 2 * -(-nd // 2) * per_vec, nd * per_vec + 2 * per_ct, nd * per_vec + 4 * per_ct + per_ct // 2, nd * per_vec + s * per_ct, 1 << 44):
            lines = run(exe, tmp_path, [f"P {s} {d} {nl} {L} {m_ct} {N} {int(with_acc)} {budget} {nd}"])
            sc, nsc, vc, nbytes = (int(x) for x in lines[0].split()[1:])
            want_vc = min(nd, 4096)
            if want_vc * per_vec > budget // 2:
                want_vc = max(1, budget // 2 // per_vec)
            want_sc = max(1, min(s, max(0, budget - want_vc * per_vec) // per_ct))
            assert (sc, nsc, vc) == (want_sc, -(-s // want_sc), want_vc), (s, d, budget)
            chunks = [tuple(int(x) for x in ln.split()[1:]) for ln in lines if ln[0] == "c"]
            batches = [tuple(int(x) for x in ln.split()[1:]) for ln in lines if ln[0] == "b"]
            for parts, total, size in ((chunks, s, sc), (batches, nd, vc)):
                at = 0
                for first, count in parts:
                    assert first == at and 1 <= count <= size
                    at += count
                assert at == total
            if sc * per_ct + vc * per_vec <= budget:
                assert nbytes <= budget + (m_ct + d + 64) * 8 + 256            # the small tables ride on top of the budget
            seen.add((min(nsc, 3), min(len(batches), 3)))
    assert {(1, 1), (2, 1), (3, 1), (3, 3)} <= seen and any(b == 2 for _, b in seen)  # one, two and many chunks either way


def test_header_is_host_only():
    deps = subprocess.run(["g++", "-std=c++17", "-x", "c++", "-M", os.path.join(CSRC, "gring_matmul_plan.hpp")], capture_output=True, text=True)
    assert deps.returncode == 0, deps.stderr
    assert "hip" not in deps.stdout.replace(ROOT, "").lower(), deps.stdout


def test_range_sum_expectation_differs_from_the_oracles_wrapped_sum_on_eight_block_rows():
    """X12, eight block rows x 8 columns: 8 * 46 terms a sum, fold_terms = 64.  The oracle's own whole-matrix sum wraps; the range sum does not.  The GPU
    test of the fold discriminates on exactly this."""
    p = mc.Party("X12")
    nrow, ncol = 8 * p.slots, 8
    assert all(mc.fold_terms(q) < 8 * 46 for q in p.q[:2])
    p.need(mc.rotations(nrow, ncol, p.slots))
    geno = mc.geno_matrix(nrow, ncol, 5)
    A = mc.inputs(p.ring, 1, 8, 2, 900)
    whole = mc.orc_product(p.ring, p.keys, A, 2, 2, geno)
    exact = mc.range_sum_product(p.ring, p.keys, A, 2, 2, geno)
    assert whole.shape == exact.shape == (1, 1, 2, 2, p.N) and whole.size == 16384
    assert int(np.count_nonzero(whole != exact)) == 16384
