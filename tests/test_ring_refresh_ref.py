"""CPU tests of the general ring's collective bootstrap (sfgwas_amd/csrc/gring_refresh_arith.hpp, gring_refresh_plan.hpp, gring_refresh.hip).

The Python-integer statement (tests/ring_refresh_ref.py) is held against the CPU oracle's orc_refresh_* on every chain whose big integer fits the oracle's 1024
bits.  tests/host/host_gring_refresh_test.cpp includes the two headers - the functions the kernels run - compiled for the host, built once with AddressSanitizer +
UBSan as a plain executable and run as a child process; every word it prints is compared here with Python integers, at 1, 2, 45, 46 and 48 limbs (one limb is
reachable by the unscaled mask functions alone: a rescale adds 54 bits to at least 64).  The limb-level model of the header takes every branch class on the
directed inputs, and seven planted mistakes each change its output there.
"""
import os
import struct
import subprocess
from math import prod

import numpy as np
import pytest

import oracle_lib as ol
import ring_refresh_ref as rf
import refresh_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sfgwas_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "host", "host_gring_refresh_test.cpp")
M64 = rf.M64


# ---------------------------------------------------------------- the statement against the oracle
ORACLE_CASES = [(n, lv, p) for n in ("G12", "G13", "X12", "P14", "W15") for lv in rf.levels(n) for p in [None] + rf.pairs_of(n, lv)[:3]
                if rf.q_bits(n, lv) + 54 + 80 <= 1024]


@pytest.mark.parametrize("name,level,pair", ORACLE_CASES, ids=lambda v: str(v))
def test_statement_matches_the_oracle(name, level, pair):
    logN, q, p = rf.chain(name)
    oring = ol.Ring(logN, q, p)
    inp = rf.case_inputs(name, level, pair, nct=1, wide_errors=False)
    h0, h1, out = rf.expected_of(inp)
    if rf.unscaled(inp.scales):
        g0, g1 = ol.refresh_gen_shares(oring, level, inp.cts[0], inp.sk, inp.crs[0], inp.mask_limbs[0], inp.e0[0], inp.e1[0])
        go = ol.refresh_finish(oring, level, inp.cts[0], inp.h0agg[0], inp.h1agg[0], inp.crs[0])
    else:
        s = inp.scales
        g0, g1 = ol.refresh_gen_shares_scaled(oring, level, inp.cts[0], s[0], s[1], inp.sk, inp.crs[0], inp.mask_limbs[0], inp.e0[0], inp.e1[0])
        go = ol.refresh_finish_scaled(oring, level, inp.cts[0], s[0], s[1], inp.h0agg[0], inp.h1agg[0], inp.crs[0])
    assert np.array_equal(g0, h0[0]) and np.array_equal(g1, h1[0]) and np.array_equal(go, out[0])
    # and the general path of the statement (INTT + CRT) sees the integers the inputs were made from
    assert rf.plaintext_of(inp.ring, level, inp.cts[0], inp.h0agg[0]) == inp.xs[0]


def test_wide_ring_serves_every_modulus_of_m48():
    ring = rf.ring_of("M48")
    assert len(ring.moduli) == 48 and rf.q_bits("M48", 46) == 2867 and rf.limbs_for(2867, 0) == 46
    rnd = np.random.default_rng(3)
    for m in (0, 15, 16, 31, 32, 46, 47):
        a = rnd.integers(0, ring.moduli[m], ring.N, dtype=np.uint64)
        assert np.array_equal(ring.intt(m, ring.ntt(m, a)), a)
        one = np.zeros(ring.N, dtype=np.uint64)
        one[0] = 5
        assert np.all(ring.ntt(m, one) == 5)


# ---------------------------------------------------------------- the stand-alone program
def _compile(exe, sanitize=True):
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-I", CSRC, "-o", exe, SRC]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    if not sanitize or subprocess.run(base + san, capture_output=True).returncode != 0:        # no sanitizer runtimes: the plain build must still succeed
        subprocess.check_call(base)
    return exe


def words(v, n):
    return [(v >> (64 * i)) & M64 for i in range(n)]


def share_lines():
    """(script line, expected output line) for masks at W = 1, 2, 45, 46, 48 limbs"""
    _, q, _ = rf.chain("M48")
    mods = [q[0], q[20], q[46], 12289]           # 12289: a modulus far below |e| = 2^31 and below a limb
    out = []
    for W in (1, 2, 45, 46, 48):
        level = min(max((64 * W - 70) // 61, 0), 46)
        for pair in [None, "ref", "ref_np2", "r64", "r70", "l64", "l75", "d1", "np2_l48", "m1"]:
            scales = None if pair is None else rf.PAIRS[pair]
            r = None if rf.unscaled(scales) else rf.ratio(scales)
            if r is not None and not rf.fits_mask(W, r[2]):
                continue
            n = 0 if r is None else rf.limbs_for(64 * W, r[2])
            mo, mi, sh = r or (1, 1, 0)
            for k, m in enumerate(rf.directed_masks(q, level, W, scales)):
                e = [0, 19, -19, (1 << 31) - 1, -(1 << 31)][k % 5]
                limbs = words(m % (1 << (64 * W)), W)
                exp = [1 if m < 0 else 0] + words(abs(m), W) + [(m + e) % qj for qj in mods]
                if n:
                    m2 = rf.rescaled(m, scales)
                    exp += words(abs(m2), n) + [(m2 + e) % qj for qj in mods]
                out.append((f"R {W} {n} {mo} {mi} {sh} {e} {len(mods)} " + " ".join(map(str, mods + limbs)), "R " + " ".join(map(str, exp))))
    return out


def recode_cases():
    """(chain, level, pair): limb counts 2 (level 0), 45 and 46 (M48's levels 45 and 46), 48 (the pair that just fits), and the widths between"""
    cs = [("G12", 0, "ref"), ("G12", 1, None), ("G12", 1, "l75"), ("X12", 2, "r70"), ("X12", 1, "d1"), ("P14", 4, "ref"), ("P14", 4, "ref_np2"), ("L19", 16, "np2_l48"),
          ("L19", 8, None), ("M33", 31, "r64"), ("M33", 16, "l64"), ("M33", 16, None), ("M48", 45, "ref"), ("M48", 45, "np2_up"), ("M48", 46, "ref_np2"), ("M48", 46, "fit"),
          ("M48", 46, None), ("M48", 0, "ref"), ("M48", 23, "l75"), ("M48", 0, None)]
    return cs


def recode_lines():
    out, seen = [], set()
    for name, level, pair in recode_cases():
        _, q, _ = rf.chain(name)
        nl, nq = level + 1, len(q)
        Q = prod(q[:nl])
        scales = None if pair is None else rf.PAIRS[pair]
        r = None if rf.unscaled(scales) else rf.ratio(scales)
        n = 0 if r is None else rf.limbs_for(Q.bit_length(), r[2])
        assert r is None or rf.fits_q(Q.bit_length(), r[2])
        seen.add(n)
        mo, mi, sh = r or (1, 1, 0)
        for x in rf.directed_x(q, level, scales):
            d = rr.to_digits(x, q[:nl])
            neg = x >= Q // 2
            v = x - Q if neg else x
            exp = [1 if neg else 0] + [v % qj for qj in q[nl:]]
            if n:
                v2 = rf.rescaled(v, scales)
                exp += words(x, n) + words(abs(v2), n) + [v2 % qj for qj in q]
            out.append((f"X {nl} {nq} {n} {mo} {mi} {sh} " + " ".join(map(str, q + d)), "X " + " ".join(map(str, exp))))
    assert {2, 45, 46, 48} <= seen
    return out


def scale_lines():
    out = []
    fs = [1.0, 1.5, 2.0 ** 34, 2.0 ** 52, 2.0 ** 53 - 1, 2.0 ** 53, 2.0 ** 53 + 2.0, 2.0 ** 400, 2.0 ** 401, 0.5, 0.0, -4.0, float("inf"), float("nan"), 1234567.0 * 2.0 ** 20]
    fs += [s for p in rf.PAIRS.values() for s in p]
    for f in fs:
        bits = struct.unpack("<Q", struct.pack("<d", f))[0]
        ok = f == f and 1.0 <= f <= 2.0 ** 400
        m, e = rf.scale_parts(f) if ok else (0, 0)
        out.append((f"S {bits}", f"S {bits} {1 if ok else 0} {m} {e}"))
    for bits, W, sh in [(2867, 46, 149), (2867, 44, 149), (2867, 44, 150), (2867, 45, 74), (2867, 46, 74), (2867, 46, 75), (61, 1, 0), (61, 2, -70), (3016, 47, 0), (3017, 48, 0),
                        (438, 7, -16), (10, 1, -300)]:
        out.append((f"F {bits} {W} {sh}", f"F {bits} {W} {sh} {int(rf.fits_q(bits, sh))} {int(rf.fits_mask(W, sh))} {rf.limbs_for(bits, sh)} {rf.limbs_for(64 * W, sh)}"))
    return out


def plan_of(nct, words_, budget):
    """gring_refresh_plan.hpp's grf_plan_words restated"""
    if nct == 0 or words_ == 0:
        return words_, 0, 0, 0
    fit = max(1, min(budget // (words_ * 8), rf.CHUNK_CAP, nct))
    return words_, fit, -(-nct // fit), fit * words_ * 8


def plan_text(p, nct):
    w, chunk, nchunks, nbytes = p
    s = f" {w} {chunk} {nchunks} {nbytes} {nbytes + 64 if nbytes else 0}"
    return s + "".join(f" {c * chunk} {min(chunk, nct - c * chunk)}" for c in range(nchunks))


def plan_lines():
    out = []
    for N, nl, nq in [(4096, 1, 2), (4096, 2, 2), (65536, 3, 38), (4096, 47, 47), (16384, 5, 10)]:
        for nct in (0, 1, 2, 1023, 1024, 1025, 2048, 2049):
            sw = (nl + nq) * N
            for budget in (512 << 20, sw * 8, sw * 8 - 1, 2 * sw * 8 + 1, 0, 1 << 62):            # the default; exactly one item; less than one; two; none; no limit: the cap decides
                p = plan_of(nct, sw, budget)
                out.append((f"PS {nct} {nl} {nq} {N} {budget}", f"PS {nct} {nl} {nq} {N} {budget}" + plan_text(p, nct) + f" | 0 {p[1] * nl * N} {p[1] * sw}"))
                for scaled in (0, 1):
                    ny = nq if scaled else nq - nl
                    fw = (nl + ny) * N + (0 if scaled else N // 8) if ny else 0
                    if fw:
                        p = plan_of(nct, fw, budget)
                    else:
                        ch = min(nct, rf.CHUNK_CAP)
                        p = (0, ch, -(-nct // ch) if ch else 0, 0)
                    J = p[1]
                    X, Y, S = 0, (J * nl * N if ny else 0), (J * nl * N if ny else 0) + J * ny * N
                    end = S + (J * (N // 8) if ny and not scaled else 0)
                    out.append((f"PF {nct} {nl} {nq} {scaled} {N} {budget}", f"PF {nct} {nl} {nq} {scaled} {N} {budget}" + plan_text(p, nct) + f" | {ny} {X} {Y} {S} {end}"))
    return out


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _compile(str(tmp_path_factory.mktemp("gring_refresh") / "host_gring_refresh_test"))


def run_lines(exe, tmp_path, pairs):
    path = str(tmp_path / "script.txt")
    with open(path, "w") as f:
        f.write("\n".join(p[0] for p in pairs) + "\n")
    out = subprocess.run([exe, path], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("OK"), out.stdout[-2000:] + out.stderr[-4000:]
    got = out.stdout.splitlines()
    assert len(got) == len(pairs) + 1
    bad = [(p[0][:120], g[:200], p[1][:200]) for p, g in zip(pairs, got) if g.split() != p[1].split()]
    assert not bad, bad[:3]


def test_share_arithmetic_matches_python_integers_under_the_sanitizers(exe, tmp_path):
    lines = share_lines()
    assert len(lines) > 500
    run_lines(exe, tmp_path, lines)


def test_recode_arithmetic_matches_python_integers_under_the_sanitizers(exe, tmp_path):
    lines = recode_lines()
    assert len(lines) > 150
    run_lines(exe, tmp_path, lines)


def test_scales_and_fit_checks(exe, tmp_path):
    run_lines(exe, tmp_path, scale_lines())


def test_plans_and_layouts_at_their_edges(exe, tmp_path):
    """one item, exactly the chunk cap, cap + 1, a budget that holds a single item (and one that holds none): chunks tile the call, regions tile the chunk"""
    lines = plan_lines()
    assert any(" 1025 " in a and " 1024 2 " in b for a, b in lines)
    run_lines(exe, tmp_path, lines)


def test_headers_are_host_only():
    for hdr in ("gring_refresh_arith.hpp", "gring_refresh_plan.hpp"):
        deps = subprocess.run(["g++", "-std=c++17", "-x", "c++", "-M", os.path.join(CSRC, hdr)], capture_output=True, text=True)
        assert deps.returncode == 0, deps.stderr
        assert "hip" not in deps.stdout.replace(ROOT, "").lower(), deps.stdout


# ---------------------------------------------------------------- the limb model: branch classes and planted mistakes
MODEL_CASES = [("G12", 0, None), ("G12", 0, "ref"), ("G12", 1, "l75"), ("X12", 1, "d1"), ("X12", 1, "r70"), ("P14", 4, "ref"), ("P14", 4, "ref_np2"), ("P14", 9, None),
               ("L19", 8, "np2_l48"), ("M33", 16, "r64"), ("M33", 8, "l64"), ("M48", 46, "fit"), ("M48", 45, "ref")]


def model_outputs(mutant=None, cls=None):
    cls = set() if cls is None else cls
    out = []
    for name, level, pair in MODEL_CASES:
        _, q, _ = rf.chain(name)
        scales = None if pair is None else rf.PAIRS[pair]
        W = rf.mask_limbs_of(name, level, scales)
        for k, m in enumerate(rf.directed_masks(q, level, W, scales)):
            e = [0, 19, -19][k % 3]
            out.append(rf.model_share_rows(words(m % (1 << (64 * W)), W), e, q, scales, cls, mutant))
        for x in rf.directed_x(q, level, scales):
            out.append(rf.model_recode(x, level, q, scales, cls, mutant))
    return out


def statement_outputs(mutant=None):
    out = []
    for name, level, pair in MODEL_CASES:
        _, q, _ = rf.chain(name)
        scales = None if pair is None else rf.PAIRS[pair]
        W = rf.mask_limbs_of(name, level, scales)
        Q = prod(q[:level + 1])
        for k, m in enumerate(rf.directed_masks(q, level, W, scales)):
            e = [0, 19, -19][k % 3]
            out.append([(rf.rescaled(m, scales, mutant) + e) % qj for qj in q])
        for x in rf.directed_x(q, level, scales):
            out.append([rf.rescaled(rf.recentred(x, Q, mutant), scales, mutant) % qj for qj in q])
    return out


def test_limb_model_is_the_statement_and_takes_every_branch_class():
    cls = set()
    assert model_outputs(None, cls) == statement_outputs()
    missing = [c for c in rf.CLASSES if c not in cls]
    assert not missing, missing
    shifts = {c for c in cls if c.startswith("shift_")}
    assert {"shift_none", "shift_right_ws0_bs", "shift_right_ws1_bs0", "shift_right_ws1_bs", "shift_left_ws1_bs", "shift_left_ws0_bs", "shift_left_ws1_bs0"} <= shifts
    assert len(rf.UNREACHABLE) == 4              # listed with their reasons in ring_refresh_ref.py


@pytest.mark.parametrize("mutant", rf.MUTANTS)
def test_planted_mistake_is_caught_by_the_directed_inputs(mutant):
    assert model_outputs(mutant) != statement_outputs(), f"not caught: {mutant}"


@pytest.mark.parametrize("mutant", ["sign_gt", "floor"])
def test_statement_mutants_differ_from_the_statement(mutant):
    """the two mistakes that exist at the level of the integers themselves"""
    assert statement_outputs(mutant) != statement_outputs()
