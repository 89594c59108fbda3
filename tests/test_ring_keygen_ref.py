"""CPU checks of the general ring's key generation (sfgwas_amd/csrc/gring_keygen_arith.hpp, gring_keygen_plan.hpp).

tests/host/host_gring_keygen_test.cpp runs the kernels' own per-element epilogues and the host planner under AddressSanitizer and UBSan on directed operands at
every modulus of tests/ring_cases.py (0, 1, q - 1 and words on both sides of every conditional subtraction of the epilogues; g_i for every (digit, modulus) of
every chain), and this file holds each printed word against Python integers and the plan against its restatement.  keygen_ref itself is held on ring_ref.SplitRing
(G12 and L19): the three key equations of section 11 hold exactly for two parties.  Three planted mistakes of the epilogue must change the output."""
import os
import subprocess
from math import prod

import numpy as np
import pytest

import keygen_ref as kr
import ring_cases as rc
import ring_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sfgwas_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "host", "host_gring_keygen_test.cpp")
HDRS = ("gring_arith.hpp", "gring_io_arith.hpp", "gring_keygen_arith.hpp", "gring_keygen_plan.hpp")
I32 = (2 ** 31 - 1, -(2 ** 31 - 1), -2 ** 31, 0, 1, -1, 19, -19)


def _compile(exe, include_dir, sanitize):
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-I", include_dir, "-o", exe, SRC]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    if not sanitize or subprocess.run(base + san, capture_output=True).returncode != 0:        # no sanitizer runtimes: the plain build must still succeed
        subprocess.check_call(base)
    return exe


def words(q):
    """0, 1, q - 1 and neighbours, both sides of q / 2 (a sum of two of them is just below or just above q), and a word in the middle of nowhere"""
    return [0, 1, 2, q - 1, q - 2, q // 2, q // 2 + 1, (q * 5) // 7]


def chain_g_terms():
    """(chain, digit, m, nq, np, P mod q_m or 0) for every digit and modulus of every chain"""
    out = []
    for name in rc.NAMES:
        _, q, p = rc.chain(name)
        nq, np_, P = len(q), len(p), prod(p)
        for i in range((nq + np_ - 1) // np_):
            for m, mod in enumerate(q + p):
                out.append((name, i, m, nq, np_, P % mod if m < nq and m // np_ == i else 0))
    return out


PLAN_CASES = ([(nk, 2, 3, 4096, 256 << 20, w) for nk in (0, 1, 1024, 1025, 5000) for w in (0, 1)]
              + [(nk, 2, 3, 4096, 4 * 4096, 0) for nk in (1, 7)]                                        # a budget that holds one table: chunks of 1
              + [(nk, 2, 3, 4096, 100, 0) for nk in (3,)]                                               # a budget below one table: still chunks of 1
              + [(3000, 2, 3, 1 << logN, 256 << 20, 1) for logN in range(12, 17)]
              + [(nk, 47, 48, 1 << logN, 256 << 20, 1) for nk in (1, 14, 15, 1025) for logN in (12, 16)]   # beta * nmod at its largest: nq + np = 48, np = 1
              + [(40000, 6, 7, 65536, 256 << 20, 0), (70000, 1, 2, 4096, 1 << 40, 0)])                  # the index budget binds; only the cap of 1024 binds
GALOIS = [(5, 12), (pow(5, 1024, 8192), 12), (8191, 12), (1, 12), (3, 12), (5, 13), (pow(5, 100, 1 << 17), 16), ((1 << 17) - 1, 16)]


def write_script(path):
    with open(path, "w") as f:
        for q in rc.all_moduli():
            W = words(q)
            for eh in W:
                for a in W:
                    for b in W:
                        for s, wg, pg in ((0, 0, 0), (q - 1, 1, q - 1), (1, 1, 1), (q // 2 + 1, 1, q // 2 + 1), (q - 1, 0, q - 1)):
                            f.write(f"S {eh} {a} {b} {s} {wg} {pg} {q}\n")
                        f.write(f"H {eh} {a} {b} {q}\n")
                        for s, uh in ((0, 0), (q - 1, 0), (0, q - 1), (q - 1, q - 1), (q // 2, q // 2 + 1), (1, 0)):
                            f.write(f"R {eh} {a} {b} {s} {uh} {q}\n")
            for a in I32:
                for b in I32:
                    f.write(f"LS {a} {b} {q}\n")
            f.write(f"M {q}\n")
            f.write(f"K {q} " + " ".join(["4294967295"] * 14 + [str(q & 0xFFFFFFFF), str(q >> 32)]) + "\n")                # seven masked candidates above q, the last equal to q: none
            f.write(f"K {q} " + " ".join(["4294967295"] * 12 + [str((q - 1) & 0xFFFFFFFF), str((q - 1) >> 32), "0", "0"]) + "\n")   # candidates 6 and 7 pass: the first is taken
            f.write(f"K {q} " + " ".join(["7", "4294967295"] * 8) + "\n")        # high bits beyond bitlen(q) are masked away before the comparison
        for name, i, m, nq, np_, pg in chain_g_terms():
            q = rc.chain(name)[1][m] if m < nq else rc.chain(name)[2][m - nq]
            f.write(f"G {i} {m} {nq} {np_}\n")
            if pg:
                for eh, s in ((0, q - 1), (q - 1, q - 1), (q // 2, 1)):
                    f.write(f"S {eh} {q - 1} {q - 1} {s} 1 {pg} {q}\n")
        for g, logN in GALOIS:
            f.write(f"I {g} {logN}\nJ {g} {logN}\n")
        for c in PLAN_CASES:
            f.write("P " + " ".join(map(str, c)) + "\n")


def plan_restated(nkeys, beta, nmod, N, budget, with_u):
    """-> chunk, nchunks, index_bytes, galois_at, u_bytes: the least of the cap of 1024 keys, the rows of one transform launch (32768) and of a grid dimension
    (below 65536) over beta * nmod rows a key, and the tables the budget holds; at least 1"""
    u_bytes = nmod * N * 8 if with_u else 0
    if nkeys == 0:
        return 0, 0, 0, 0, u_bytes
    rows = beta * nmod
    k = max(1, min(1024, 32768 // rows, 65535 // rows, budget // (4 * N)))
    chunk = min(k, nkeys)
    return chunk, -(-nkeys // chunk), chunk * 4 * N + chunk * 8, chunk * 4 * N, u_bytes


def lift(v, q):
    return v % q


def check_line(t):
    """-> None when the printed line holds, else a description"""
    op, v = t[0], [int(x) for x in t[1:]]
    if op == "S":
        eh, a, b, s, wg, pg, q, got = v
        return None if got == (eh - a * b + (pg * s if wg else 0)) % q else "share"
    if op == "H":
        eh, a, s, q, got = v
        return None if got == (eh + s * a) % q else "h1"
    if op == "R":
        eh, h0, h1, s, uh, q, got = v
        return None if got == (eh + s * h0 + (uh - s) * h1) % q else "round2"
    if op == "LS":
        a, b, q, got = v
        return None if got == (a + b) % q else "lift_sum"
    if op == "G":
        d, m, nq, np_, got = v

        class R:
            pass
        R.nq, R.np_, R.moduli = nq, np_, [3] * nq + [5] * np_
        return None if bool(got) == (kr.g_term(R, d, m) != 0) else "g_applies"
    if op in ("I", "J"):
        g, logN = v[0], v[1]
        ge = kr.galois_inverse(g, 1 << logN) if op == "I" else g
        return None if v[2:] == [int(x) for x in ring_ref.automorphism_index(logN, ge)] else "index"
    if op == "M":
        return None if v[1] == (1 << v[0].bit_length()) - 1 else "mask"
    if op == "P":
        nkeys, beta, nmod, N, budget, with_u = v[:6]
        want = plan_restated(nkeys, beta, nmod, N, budget, with_u)
        if tuple(v[6:11]) != want:
            return f"plan {v[6:11]} != {want}"
        pieces = list(zip(v[11::2], v[12::2]))
        covered = [k for f0, n in pieces for k in range(f0, f0 + n)]
        ok = covered == list(range(nkeys)) and all(1 <= n <= want[0] for _, n in pieces) and len(pieces) == want[1]
        ok = ok and (nkeys == 0 or (want[0] * beta * nmod <= 32768 or want[0] == 1) and want[0] * beta < 65536 and want[0] <= 1024)
        return None if ok else "plan coverage"
    return "unknown line"


def mismatches(lines, script):
    bad, k_lines = [], [ln.split() for ln in open(script) if ln.startswith("K ")]
    ki = 0
    for ln in lines[:-1]:
        t = ln.split()
        if t[0] == "K":
            q, w = int(k_lines[ki][1]), [int(x) for x in k_lines[ki][2:]]
            ki += 1
            mask = (1 << q.bit_length()) - 1
            cands = [c for c in ((w[2 * k] | (w[2 * k + 1] << 32)) & mask for k in range(8)) if c < q]
            want = (1, cands[0]) if cands else (0, 0)
            if (int(t[2]), int(t[3])) != want:
                bad.append(ln)
        elif check_line(t):
            bad.append(check_line(t) + ": " + ln[:200])
    return bad


@pytest.fixture(scope="module")
def script(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("gring_keygen") / "script.txt")
    write_script(path)
    return path


def run(exe, script):
    out = subprocess.run([exe, script], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("OK"), out.stdout[-2000:] + out.stderr[-4000:]
    return out.stdout.splitlines()


def test_epilogues_and_plan_match_python_integers_under_the_sanitizers(tmp_path, script):
    lines = run(_compile(str(tmp_path / "host_gring_keygen_test"), CSRC, sanitize=True), script)
    assert len(lines) == sum(1 for _ in open(script)) + 1
    bad = mismatches(lines, script)
    assert not bad, bad[:10]
    assert sum(ln.startswith("G ") for ln in lines) == len(chain_g_terms()) and sum(ln.startswith("P ") for ln in lines) == len(PLAN_CASES)
    assert any(int(ln.split()[2]) == 0 for ln in lines if ln.startswith("K ")) and any(int(ln.split()[2]) == 1 for ln in lines if ln.startswith("K "))


def test_directed_operands_take_both_sides_of_every_conditional_subtraction():
    """of the epilogues' own: the share's eh - ab borrows or not, its + g s wraps or not; h1's and round 2's sums wrap or not; u - s borrows or not; the lifted
    sum of two errors wraps or not.  (The subtractions inside mulmod, barrett128 and shoup are gring_arith.hpp's, held by tests/test_ring_ref.py.)"""
    for q in rc.all_moduli():
        W = words(q)
        borrow = {eh >= (a * b) % q for eh in W for a in W for b in W}
        wrap_g = {((eh - a * b) % q) + ((q - 1) * (q - 1)) % q >= q for eh in W for a in W for b in W}
        wrap_h = {eh + (a * b) % q >= q for eh in W for a in W for b in W}
        wrap_r = {eh + ((q - 1) * a + (0 - (q - 1)) % q * b) % q >= q for eh in W for a in W for b in W}
        wrap_l = {lift(a, q) + lift(b, q) >= q for a in I32 for b in I32}
        assert borrow == wrap_g == wrap_h == wrap_r == wrap_l == {True, False}, q


def test_plan_cases_reach_every_limit():
    got = {c: plan_restated(*c) for c in PLAN_CASES}
    chunks = {c: v[0] for c, v in got.items()}
    assert chunks[(1025, 2, 3, 4096, 256 << 20, 0)] == 1024 and got[(1025, 2, 3, 4096, 256 << 20, 0)][1] == 2           # the cap of 1024 keys
    assert chunks[(7, 2, 3, 4096, 4 * 4096, 0)] == 1 and chunks[(3, 2, 3, 4096, 100, 0)] == 1                          # the budget, and "at least 1"
    assert chunks[(1025, 47, 48, 4096, 256 << 20, 1)] == 32768 // (47 * 48) == 14                                      # the transform launch cap
    assert chunks[(40000, 6, 7, 65536, 256 << 20, 0)] == min(32768 // 42, (256 << 20) // (4 * 65536)) == 780
    assert chunks[(3000, 2, 3, 65536, 256 << 20, 1)] == 1024 and got[(3000, 2, 3, 65536, 256 << 20, 1)][4] == 3 * 65536 * 8


# ---------------------------------------------------------------- keygen_ref on SplitRing: the three key equations, two parties
def _ntt_rows(ring, poly):
    return [np.array([int(x) for x in r], dtype=object) for r in kr.rows_of(ring, poly)]


@pytest.mark.parametrize("name", ["G12", "L19"])
def test_key_equations_hold_exactly_on_a_split_ring(name):
    logN, q, p = rc.chain(name)
    ring = ring_ref.SplitRing(logN, q, p)
    N, beta, nmod = ring.N, kr.beta_of(ring), len(ring.moduli)
    rnd = np.random.default_rng(500)
    parties = [dict(s=rnd.integers(-1, 2, N), u=rnd.integers(-1, 2, N), e=rnd.integers(-19, 20, N), **{k: rnd.integers(-19, 20, (beta, N)) for k in ("ert", "e0", "e1", "e2", "e3")})
               for _ in range(2)]
    uni = lambda *lead: np.stack([rnd.integers(0, m, lead + (N,), dtype=np.uint64) for m in ring.moduli], axis=len(lead))      # noqa: E731
    tot = lambda k, *i: sum(pt[k][i] if i else pt[k] for pt in parties)                                                          # noqa: E731
    S, U = tot("s"), tot("u")
    Sh, Uh = _ntt_rows(ring, S), _ntt_rows(ring, U)
    # public key: H + crp S = NTT(E)
    crp = uni()
    H = kr.aggregate(ring, [kr.ckg_share(ring, pt["s"], crp, pt["e"]) for pt in parties])
    Eh = _ntt_rows(ring, tot("e"))
    for m, mod in enumerate(ring.moduli):
        assert np.array_equal((H[m] + kr._obj(crp[m]) * Sh[m]) % mod, Eh[m]), m
    # rotation key: b_i + a_i phi_{g^-1}(S) - g_i S = NTT(E_i)
    g = ring.galois(1)
    crp = uni(beta)
    b = kr.aggregate(ring, [kr.rtg_share(ring, pt["s"], g, crp, pt["ert"]) for pt in parties])
    Sg = _ntt_rows(ring, kr.automorphism(S, kr.galois_inverse(g, N), N))
    for i in range(beta):
        Eh = _ntt_rows(ring, tot("ert", i))
        for m, mod in enumerate(ring.moduli):
            assert np.array_equal((b[i][m] + kr._obj(crp[i][m]) * Sg[m] - kr.g_term(ring, i, m) * Sh[m]) % mod, Eh[m]), (i, m)
    # relinearisation key: b_i + a_i S - g_i S^2 = NTT(S E0_i + U E1_i + E2_i + E3_i), the products of polynomials taken in the NTT domain
    r1 = [kr.rkg_round1(ring, pt["s"], crp, pt["u"], pt["e0"], pt["e1"]) for pt in parties]
    H0, H1 = kr.aggregate(ring, [x[0] for x in r1]), kr.aggregate(ring, [x[1] for x in r1])
    b = kr.aggregate(ring, [kr.rkg_round2(ring, pt["s"], H0, H1, pt["u"], pt["e2"], pt["e3"]) for pt in parties])
    for i in range(beta):
        E = [_ntt_rows(ring, tot(k, i)) for k in ("e0", "e1", "e2", "e3")]
        for m, mod in enumerate(ring.moduli):
            noise = (Sh[m] * E[0][m] + Uh[m] * E[1][m] + E[2][m] + E[3][m]) % mod
            assert np.array_equal((b[i][m] + H1[i][m] * Sh[m] - kr.g_term(ring, i, m) * Sh[m] * Sh[m]) % mod, noise), (i, m)
    assert nmod == len(q) + len(p) and sum(kr.g_term(ring, i, m) != 0 for i in range(beta) for m in range(nmod)) == len(q)


# ---------------------------------------------------------------- planted mistakes (profiles/EXPERIMENTS.md lists them)
MUTANTS = {
    "the sign of the crp term": ("gring_keygen_arith.hpp", "u64 r = gr::submod(eh, gr::mulmod(a, b, q, uhi, ulo), q);", "u64 r = gr::addmod(eh, gr::mulmod(a, b, q, uhi, ulo), q);"),
    "g_i applied at the wrong digit": ("gring_keygen_arith.hpp", "return m < nq && m / np == digit;", "return m < nq && (m + 1) / np == digit;"),
    "the index table of g instead of g^-1": ("gring_keygen_arith.hpp", "GR_HD u64 share_galois(u64 g, int logN) { return galois_inverse(g, logN); }",
                                             "GR_HD u64 share_galois(u64 g, int logN) { (void)logN; return g; }"),
}


@pytest.mark.parametrize("name", list(MUTANTS))
def test_planted_mistake_is_caught(tmp_path, script, name):
    which, old, new = MUTANTS[name]
    inc = tmp_path / "inc"
    inc.mkdir()
    for hdr in HDRS:
        text = open(os.path.join(CSRC, hdr)).read()
        if hdr == which:
            assert text.count(old) == 1, f"the line this mutant replaces is gone from {hdr}"
            text = text.replace(old, new)
        (inc / hdr).write_text(text)
    lines = run(_compile(str(tmp_path / "mutant"), str(inc), sanitize=False), script)
    assert mismatches(lines, script), f"not caught: {name}"


def test_headers_are_host_only():
    """both headers compile as plain C++17 and pull in no HIP header"""
    for hdr in ("gring_keygen_arith.hpp", "gring_keygen_plan.hpp"):
        deps = subprocess.run(["g++", "-std=c++17", "-x", "c++", "-M", os.path.join(CSRC, hdr)], capture_output=True, text=True)
        assert deps.returncode == 0, deps.stderr
        assert "hip" not in deps.stdout.replace(ROOT, "").lower(), deps.stdout
