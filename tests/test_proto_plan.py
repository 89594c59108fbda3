"""The chunk rule of the fixed-ring protocol ends (sfgwas_amd/csrc/batch_plan.hpp: how many ciphertexts, plaintexts or rows one pass of encrypt.hip, decrypt.hip,
refresh.hip, rvec.hip and keygen.hip takes, and the bytes of every named scratch buffer of a chunk) on the CPU, no GPU and nothing of the library linked.

tests/host/host_proto_plan_test.cpp includes the header - the functions the executors call - compiled for the host with AddressSanitizer + UBSan as a plain
executable; it checks on every call that the chunks cover [0, n) exactly once and in order, and every line it prints is compared here with a literal restatement in
Python.

The second chunk of a refresh entry point has no GPU test: its smallest shape is 32769 ciphertexts, more than 8 GB of input at level 0.  This file carries that
rule (test_grid_bound_of_every_plan, test_refresh_plans_split_at_the_grid_bound); the second chunks of the other families run in tests/test_gpu_encrypt.py,
test_gpu_decrypt.py and test_gpu_rvec.py."""
import os
import re
import subprocess

import numpy as np
import pytest

from sfgwas_amd.params import P_PN14, Q_PN14

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sfgwas_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "host", "host_proto_plan_test.cpp")
N14, NQ, NP = 16384, len(Q_PN14), len(P_PN14)
GIB = 1 << 30
NO_BUDGET = (1 << 64) - 1
ENC_BUDGET, PCKS_CAP, DECODE_CAP, RVEC_CAP, GRID_CAP, GRID_DIM_MAX = GIB, 256, 512, 64, 32768, 65535
# items of a chunk that one launch puts into grid.y or grid.z, per family (0: its launches are grid.x only)
GRID_ROWS_PER_ITEM = {"E": 0, "P": 1, "D": 1, "V": 1, "G": 1, "F": 1, "S": 1}


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("proto_plan") / "host_proto_plan_test")
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-o", out, SRC]
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
def plan(n, words, budget, cap):
    """(chunk, nchunks, bytes, [(first, count)]): budget // (words * 8) items, clamped to [1, cap] and to n; the empty call has no chunk"""
    if n <= 0:
        return 0, 0, 0, []
    fit = budget // (words * 8) if words else n
    fit = max(fit, 1)
    if cap > 0:
        fit = min(fit, cap)
    chunk = min(fit, n)
    chunks = [(c0, min(chunk, n - c0)) for c0 in range(0, n, chunk)]
    return chunk, len(chunks), chunk * words * 8, chunks


def tail(n, words, budget, cap):
    chunk, nchunks, nbytes, chunks = plan(n, words, budget, cap)
    return f" | {chunk} {nchunks} {nbytes}" + "".join(f" {a} {c}" for a, c in chunks)


def want(line):
    op, *a = line.split()
    a = [int(v) for v in a]
    if op == "B":
        n, words, budget, cap = a
        return "B" + tail(n, words, budget, cap)
    if op == "E":
        nct, nl, np_, N = a
        words = 2 * (nl + np_) * N
        return f"E {words}" + tail(nct, words, ENC_BUDGET, 0)
    if op == "P":
        nct, nl, N = a
        return f"P {2 * nl * N}" + tail(nct, 2 * nl * N, NO_BUDGET, PCKS_CAP)
    if op == "D":
        nvec, nl, N, coeff, host, parts = a
        x, w, out = nl * N, 0 if coeff else 2 * N, 0 if not host else N if coeff else (N // 2) * parts
        chunk = plan(nvec, x + w + out, NO_BUDGET, DECODE_CAP)[0]
        return f"D {x} {w} {out} {chunk * x * 8} {chunk * w * 8} {chunk * out * 8}" + tail(nvec, x + w + out, NO_BUDGET, DECODE_CAP)
    if op == "V":
        nct, W, nl, N = a
        fft, coef = 2 * W * (N // 2), nl * N
        chunk = plan(nct, fft + coef, NO_BUDGET, RVEC_CAP)[0]
        return f"V {fft} {coef} {chunk * fft * 8} {chunk * coef * 8}" + tail(nct, fft + coef, NO_BUDGET, RVEC_CAP)
    if op == "G":
        return "G" + tail(a[0], 0, NO_BUDGET, GRID_CAP)
    if op in "FS":
        nct, nl, N = a
        words = nl * N if op == "F" else N // 2                  # x: nl rows; zero_e: N 32-bit zeros
        return f"{op} {words}" + tail(nct, words, NO_BUDGET, GRID_CAP)
    raise AssertionError(line)


def chunk_of(row):
    return int(row.split("|")[1].split()[0])


def around(cap):
    return [0, 1, cap - 1, cap, cap + 1, 2 * cap, 2 * cap + 1]


# ---------------------------------------------------------------------------------------------------- the constants and the rule itself
def test_named_constants(exe, tmp_path):
    assert run(exe, ["K"], tmp_path) == [f"K {ENC_BUDGET} {PCKS_CAP} {DECODE_CAP} {RVEC_CAP} {GRID_CAP} {GRID_DIM_MAX}"]


def test_the_rule_at_its_edges(exe, tmp_path):
    """the empty and the negative call; a budget below one item (the chunk is 1, however many items); a budget of exactly one and exactly two items; no cap; no
    scratch at all; the cap and the budget each being the smaller"""
    item = 3 * N14 * 8
    lines = [f"B 0 {3 * N14} {GIB} 256", f"B -5 {3 * N14} {GIB} 256", f"B 7 {3 * N14} {item - 1} 256", f"B 7 {3 * N14} 0 0", f"B 7 {3 * N14} {item} 256",
             f"B 7 {3 * N14} {2 * item} 256", f"B 7 {3 * N14} {2 * item + item - 1} 256", f"B 100000 {3 * N14} {NO_BUDGET} 0", "B 100000 0 0 0", "B 100000 0 0 32768",
             f"B 1000 {3 * N14} {300 * item} 256", f"B 1000 {3 * N14} {200 * item} 256", "B 700 1 8 0"]
    rows = run(exe, lines, tmp_path)
    assert rows == [want(ln) for ln in lines]
    assert [chunk_of(r) for r in rows] == [0, 0, 1, 1, 1, 2, 2, 100000, 100000, 32768, 256, 200, 1]
    assert rows[2].endswith(" 0 1 1 1 2 1 3 1 4 1 5 1 6 1") and rows[0] == "B | 0 0 0"


def test_random_plans(exe, tmp_path):
    rnd = np.random.default_rng(11)
    lines = []
    for _ in range(400):
        words = int(rnd.integers(0, 5)) * (1 << int(rnd.integers(0, 18)))
        n, cap = int(rnd.integers(-2, 3000)), int(rnd.choice([0, 1, 7, 64, 256, 512, 32768]))
        budget = int(rnd.integers(0, 700)) * max(words, 1) * 8 // int(rnd.integers(1, 4)) + int(rnd.integers(0, 3))
        lines.append(f"B {n} {words} {budget} {cap}")
    assert run(exe, lines, tmp_path) == [want(ln) for ln in lines]


# ---------------------------------------------------------------------------------------------------- the families on the PN14 chain
def test_encryption_chunk_at_every_level(exe, tmp_path):
    """2^30 // (2 (level + 1 + 2) 16384 8) ciphertexts: what encrypt_run computed inline"""
    assert (NQ, NP) == (10, 2)
    chunks = [GIB // (2 * (level + 1 + NP) * N14 * 8) for level in range(NQ)]
    assert (chunks[0], chunks[5], chunks[9]) == (1365, 512, 341)
    lines = [f"E {n} {level + 1} {NP} {N14}" for level in range(NQ) for n in around(chunks[level])]
    rows = run(exe, lines, tmp_path)
    assert rows == [want(ln) for ln in lines]
    for level in range(NQ):
        got = [chunk_of(r) for r in rows[7 * level:7 * level + 7]]
        c = chunks[level]
        assert got == [0, 1, c - 1, c, c, c, c]
    assert rows[3].endswith(f"| 1365 1 {1365 * 2 * 3 * N14 * 8} 0 1365") and rows[4].endswith("0 1365 1365 1") and rows[6].endswith("0 1365 1365 1365 2730 1")
    # a ring whose one ciphertext exceeds the budget still runs, one at a time
    big = run(exe, [f"E 3 40 8 {1 << 22}"], tmp_path)
    assert big == [want(f"E 3 40 8 {1 << 22}")] and chunk_of(big[0]) == 1


def family_lines():
    lines = []
    for level in (0, 5, 9):
        nl = level + 1
        lines += [f"P {n} {nl} {N14}" for n in around(PCKS_CAP)]
        for coeff, host, parts in [(1, 1, 1), (0, 1, 1), (0, 1, 2), (0, 0, 1), (0, 0, 2)]:       # decode_coeffs, decode_vectors real / complex, decode_vectors_dev
            lines += [f"D {n} {nl} {N14} {coeff} {host} {parts}" for n in around(DECODE_CAP)]
        for W in (2, 3, 5, 8):
            lines += [f"V {n} {W} {nl} {N14}" for n in around(RVEC_CAP)]
        for op in "FS":
            lines += [f"{op} {n} {nl} {N14}" for n in around(GRID_CAP) + [65535, 65536, 200000]]
    lines += [f"G {n}" for n in around(GRID_CAP) + [65535, 65536, 200000]]
    return lines


def test_every_cap_at_its_edges(exe, tmp_path):
    """n in {0, 1, cap - 1, cap, cap + 1, 2 cap, 2 cap + 1} for every family at levels 0, 5 and 9, with the bytes of every named buffer"""
    lines = family_lines()
    rows = run(exe, lines, tmp_path)
    assert rows == [want(ln) for ln in lines]
    caps = {"P": PCKS_CAP, "D": DECODE_CAP, "V": RVEC_CAP, "F": GRID_CAP, "S": GRID_CAP, "G": GRID_CAP}
    for ln, row in zip(lines, rows):
        n = int(ln.split()[1])
        assert chunk_of(row) == min(n, caps[ln[0]]), ln
    # spelled out once: the decoder's buffers for 513 complex host vectors at level 0 - x 1 row, w N pairs, out 2 n doubles a plaintext; chunks 512 + 1
    i = lines.index(f"D 513 1 {N14} 0 1 2")
    assert rows[i] == f"D {N14} {2 * N14} {N14} {512 * N14 * 8} {512 * 2 * N14 * 8} {512 * N14 * 8} | 512 2 {512 * 4 * N14 * 8} 0 512 512 1"
    # and the ring-vector scratch the file header of rvec.hip states: 2 W 65,536 B + (level + 1) 131,072 B a ciphertext
    i = lines.index(f"V 1 5 10 {N14}")
    assert rows[i].split()[3:5] == [str(2 * 5 * 65536), str(10 * 131072)]


def test_grid_bound_of_every_plan(exe, tmp_path):
    """chunk * (grid rows an item takes in grid.y or grid.z) <= 65535 for every plan the executors use"""
    lines = family_lines() + [f"E {n} {nl} {NP} {N14}" for nl in (1, 10) for n in (1, 1365, 1366, 200000)]
    rows = run(exe, lines, tmp_path)
    for ln, row in zip(lines, rows):
        assert chunk_of(row) * GRID_ROWS_PER_ITEM[ln[0]] <= GRID_DIM_MAX, ln
    assert 2 * GRID_CAP > GRID_DIM_MAX >= GRID_CAP                              # the cap is the largest power of two the grid holds


def test_refresh_plans_split_at_the_grid_bound(exe, tmp_path):
    """sfg_refresh_gen_shares_dev (no scratch), sfg_refresh_finish_dev (x) and sfg_ckks_to_ss_share_dev (zero_e): one chunk up to 32768 ciphertexts - the launches
    they made before they had a plan - two from 32769 to 65535, and a call above 65535, which used to fail at launch, in chunks of 32768"""
    cases = {32768: [(0, 32768)], 32769: [(0, 32768), (32768, 1)], 65535: [(0, 32768), (32768, 32767)], 65536: [(0, 32768), (32768, 32768)],
             200000: [(c0, min(32768, 200000 - c0)) for c0 in range(0, 200000, 32768)]}
    for n, chunks in cases.items():
        lines = [f"G {n}", f"F {n} 1 {N14}", f"S {n} 1 {N14}", f"F {n} 10 {N14}"]
        rows = run(exe, lines, tmp_path)
        assert rows == [want(ln) for ln in lines]
        listing = "".join(f" {a} {c}" for a, c in chunks)
        assert rows[0] == f"G | 32768 {len(chunks)} 0" + listing
        assert rows[1] == f"F {N14} | 32768 {len(chunks)} {32768 * N14 * 8}" + listing           # refresh.x: one row a ciphertext at level 0
        assert rows[2] == f"S {N14 // 2} | 32768 {len(chunks)} {32768 * N14 * 4}" + listing       # refresh.zero_e: N 32-bit zeros a ciphertext
        assert rows[3] == f"F {10 * N14} | 32768 {len(chunks)} {32768 * 10 * N14 * 8}" + listing


# ---------------------------------------------------------------------------------------------------- the header and its users
def test_header_is_host_only():
    deps = subprocess.run(["g++", "-std=c++17", "-x", "c++", "-M", os.path.join(CSRC, "batch_plan.hpp")], capture_output=True, text=True)
    assert deps.returncode == 0, deps.stderr
    assert "hip" not in deps.stdout.replace(ROOT, "").lower(), deps.stdout


def test_the_executors_hold_no_chunk_rule_of_their_own():
    """the five files take every chunk from the plan: no size literal, no inline remainder arithmetic, no hand-written row pattern, one decryption front end"""
    text = {f: open(os.path.join(CSRC, f)).read() for f in ("encrypt.hip", "decrypt.hip", "refresh.hip", "rvec.hip", "keygen.hip")}
    for name, t in text.items():
        for literal in ("32768", "1ULL << 30", "RVEC_CHUNK", "enum RvecSrc", "< chunk ?"):
            assert literal not in t, (name, literal)
        assert not re.search(r"(?<![\w.])(256|512)\)? \? ", t) and not re.search(r"<\s*(256|512)\s*\?", t), name       # nct < 256 ? nct : 256
        if name != "keygen.hip":
            assert ".period = " not in t, name
    body = text["refresh.hip"].split("// ---- launch interface")[0]
    assert "hipLaunchKernelGGL(k_share" not in body and "hipLaunchKernelGGL(k_add_rows" not in body
    for name in ("decrypt.hip", "refresh.hip", "rvec.hip"):
        assert "launch_dec_front(" in text[name], name
