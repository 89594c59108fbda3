"""The general ring's two ends on the CPU (no GPU, nothing of the library linked): the test-side statements of tests/ring_io_ref.py against literal loops and
against the PN14 statements they generalise, and the per-element arithmetic and host planner of sfgwas_amd/csrc/gring_io_arith.hpp / gring_io_plan.hpp.

tests/host/host_gring_io_test.cpp includes the two headers - the functions the kernels of gring_io.hip run - compiled for the host, built once with
AddressSanitizer + UBSan as a plain executable and run as a child process.  Every word it prints is compared here with Python integers.  Twelve planted mistakes
must change the output of the directed operands alone.
"""
import functools
import os
import struct
import subprocess
from fractions import Fraction
from math import prod

import numpy as np
import pytest

import decode_ref
import encrypt_ref as er
import exactref
import ring_cases as rc
import ring_io_ref as rio
import oracle_lib as ol
import ring_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sfgwas_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "host", "host_gring_io_test.cpp")
HEADERS = ("gring_io_arith.hpp", "gring_io_plan.hpp", "gring_arith.hpp")
KEY = er.TEST_KEY


# ---------------------------------------------------------------- the sampler's map
@pytest.mark.parametrize("index", [0, 1, (1 << 32) + 5])
def test_general_map_is_the_pn14_map_at_16384(index):
    assert np.array_equal(rio.sample_u(KEY, index, 1 << 14), er.sample_u(KEY, index))
    for poly in (1, 2):
        assert np.array_equal(rio.sample_e(KEY, index, poly, 1 << 14), er.sample_e(KEY, index, poly))


@pytest.mark.parametrize("logN", [12, 13, 14, 15, 16])
def test_general_map_against_a_literal_walk(logN):
    N = 1 << logN
    u, e1, e2 = rio.sample_u(KEY, 3, N), rio.sample_e(KEY, 3, 1, N), rio.sample_e(KEY, 3, 2, N)
    assert set(np.unique(u)) <= {-1, 0, 1} and np.abs(e1).max() <= er.BOUND
    rnd = np.random.default_rng(logN)
    js = sorted({0, 1, 7, 8, 511, 512, 4095, N - 512, N - 1, N // 2, N // 2 - 1} | {int(x) for x in rnd.integers(0, N, 40)})
    for j in js:
        assert u[j] == rio.sample_one_literal(KEY, 3, 0, j), (logN, j)
        assert e1[j] == rio.sample_one_literal(KEY, 3, 1, j) and e2[j] == rio.sample_one_literal(KEY, 3, 2, j), (logN, j)
    # a smaller ring's samples are the first coefficients' of a larger one only where the map says so: e (blocks t + 512 (a >> 3)) is a prefix, u is too (a < 32 shares block rows)
    if logN > 12:
        assert np.array_equal(rio.sample_e(KEY, 3, 1, N // 2), e1[:N // 2]) and np.array_equal(rio.sample_u(KEY, 3, N // 2), u[:N // 2])


def test_sampler_statistics_at_65536():
    """one polynomial each at the largest N: the ternary thirds and the Gaussian's variance, within five standard errors"""
    N = 1 << 16
    u, e = rio.sample_u(KEY, 9, N), rio.sample_e(KEY, 9, 1, N)
    p_nonzero = np.mean(u != 0)                      # b0 set: 1/2; the sign splits it evenly
    assert abs(p_nonzero - 0.5) < 5 * np.sqrt(0.25 / N) and abs(np.mean(u)) < 5 * np.sqrt(0.5 / N)
    probs = np.array(er.magnitude_probabilities(), dtype=np.float64) / 2.0 ** 63
    var = float(np.sum(probs * np.arange(20) ** 2))
    m4 = float(np.sum(probs * np.arange(20) ** 4))
    assert abs(np.mean(e.astype(np.float64) ** 2) - var) < 5 * np.sqrt((m4 - var * var) / N)


# ---------------------------------------------------------------- keys and shares
class _Tiny(er.TinyRing):
    def gen_secret(self, seed):
        return np.random.default_rng(seed).integers(-1, 2, self.N).astype(np.int8)


def _centred(x, q):
    return [int(v) - q if int(v) > q // 2 else int(v) for v in x]


def test_keypair_of_a_split_ring_decrypts_to_its_small_error():
    logN, q, p = rc.chain("L19")
    ring = ring_ref.SplitRing(logN, q, p)
    s, pk = rio.keypair(ring, 5)
    assert set(np.unique(s)) <= {-1, 0, 1} and pk.shape == (2, 19, ring.N)
    for m in (0, 8, 9, 18):                          # both parts of the split ring, their first and last modulus
        qm = ring.moduli[m]
        sh = ring.ntt(m, np.array([int(x) % qm for x in s], dtype=np.uint64))
        e = ring.intt(m, np.array([(int(a) + int(b) * int(c)) % qm for a, b, c in zip(pk[0, m], pk[1, m], sh)], dtype=np.uint64))
        assert max(abs(v) for v in _centred(e, qm)) <= 19, m


def test_encryption_and_two_shares_decrypt_on_a_tiny_ring():
    """encrypt_bigint, then pcks_share_bigint from two additive key shares, summed, then c0 + h0agg: the message plus the ModDowns' rounding.
    Bound: t0 + t1 s = e_pk u + e0 + e1 s lives in R_QP and is divided by P (below 1 in magnitude here); every ModDown coefficient is off its exact quotient by at most 2
    (rounding, and the float correction's possible miss of one P); c0 + c1 s carries 1 + N of them, each share one more."""
    ring = _Tiny(4, [1153, 1217], [1249, 1409])
    N, level = ring.N, 1
    s, pk = er.make_keypair(ring, 3)
    rnd = np.random.default_rng(8)
    m = rnd.integers(-200, 201, N)
    pt = [ring.ntt(t, [int(x) % ring.moduli[t] for x in m]) for t in range(level + 1)]
    u, e0, e1 = rnd.integers(-1, 2, N), rnd.integers(-19, 20, N), rnd.integers(-19, 20, N)
    ct = np.stack([np.stack([np.array([int(x) for x in er.encrypt_bigint(ring, level, pk, u, e0, e1, pt)[t][pl]], dtype=object) for t in range(level + 1)]) for pl in range(2)])
    s1, s2 = rio.split_secret(s, 4)
    assert np.array_equal(s1 + s2, s)
    agg = None
    for k, sk in enumerate((s1, s2)):
        rows = [ring.ntt(t, [int(x) % ring.moduli[t] for x in sk]) for t in range(level + 1)]
        h0, h1 = rio.pcks_share_bigint(ring, level, rows, ct, rnd.integers(-38, 39, N), rnd.integers(-38, 39, N))
        assert max(abs(v) for t in range(level + 1) for v in _centred(ring.intt(t, h1[t]), ring.moduli[t])) <= 2
        agg = h0.astype(object) if agg is None else agg + h0.astype(object)
    for t in range(level + 1):
        q = ring.moduli[t]
        got = _centred(ring.intt(t, [(int(a) + int(b)) % q for a, b in zip(ct[0, t], agg[t])]), q)
        assert max(abs(g - int(w)) for g, w in zip(got, m)) <= 2 * (1 + N) + 2 * 2 + 1


# ---------------------------------------------------------------- the stand-alone program
def _compile(exe, include_dir, sanitize):
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-I", include_dir, "-o", exe, SRC]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    if not sanitize or subprocess.run(base + san, capture_output=True).returncode != 0:        # no sanitizer runtimes: the plain build must still succeed
        subprocess.check_call(base)
    return exe


LIFT_MODULI = [3, 8193, 12289, 65537, (1 << 31) - 1, (1 << 31) + 11] + rc.all_moduli()
PLAN_CASES = [(1, 1, 1, 2, 1, 4096, 512 << 20), (3, 4, 3, 2, 1, 32768, 512 << 20), (257, 1, 1, 2, 1, 4096, 512 << 20), (256, 2, 1, 1, 0, 4096, 512 << 20),
              (513, 2, 1, 2, 1, 4096, 512 << 20), (8, 34, 4, 2, 1, 65536, 512 << 20), (8, 34, 4, 2, 1, 65536, 1 << 20), (7, 3, 2, 1, 0, 65536, 40 << 20), (0, 3, 2, 2, 1, 4096, 1 << 20)]

DECODE_PLAN_CASES = [(1, 1, 4096, 512 << 20), (3, 47, 65536, 512 << 20), (300, 2, 4096, 512 << 20), (40, 17, 4096, 1 << 20), (0, 3, 4096, 1 << 20)]

# ---------------------------------------------------------------- the four workspaces, restated from the executors as they stood before the layouts existed
IO_BUDGET = 512 << 20                    # struct GrIo's default
HUGE = 1 << 60                           # a budget under which only the chunk cap binds
MAX_CHUNK, SLACK = 256, 64


def ws_parent(kind, nl, np_, npoly, with_u, N):
    """-> (words that size one item, [bytes of one item's share of each region, in order; None = a region of one word a call])"""
    n, nt = N // 2, nl + np_
    if kind == "CL":
        words = ((nt if with_u else 0) + npoly * nt + npoly * np_ + npoly * nl) * N + (npoly * N + 1) // 2
        return words, [nl * N * 8 * with_u, np_ * N * 8 * with_u, npoly * nl * N * 8, npoly * np_ * N * 8, npoly * np_ * N * 8, npoly * nl * N * 8, npoly * N * 4]
    if kind == "KL":
        return (nl + 1) * N, [nl * N * 8, N * 8]
    if kind == "EL":
        return n + 4 * n + nl * N + 8, [n * 32, n * 8, nl * N * 8, 8, None]           # A, values, R; the tail: a band a vector, two counters
    return nl * N + 2 * N + 4 * n + N, [n * 32, N * 16, nl * N * 8, n * 8, n * 8]     # A, Wd, X, re, im


def ws_cases():
    """(kind, nct, nl, np, npoly, with_u, N, budget) on every level of every chain: 1, chunk - 1, chunk, chunk + 1 and 3 chunk + 2 items of the default budget's
    chunk, a count above the cap under a budget that does not bind, and budgets below one item"""
    cases = []
    for name in rc.NAMES:
        logN, q, p = rc.chain(name)
        N = 1 << logN
        for nl in range(1, len(q) + 1):
            for kind, np_, npoly, with_u in [("CL", len(p), 2, 1), ("CL", len(p), 1, 0), ("CL", len(p), 2, 0), ("KL", 0, 0, 0), ("EL", 0, 0, 0), ("VL", 0, 0, 0)]:
                words = ws_parent(kind, nl, np_, npoly, with_u, N)[0]
                chunk = max(1, min(MAX_CHUNK, IO_BUDGET // (words * 8)))
                counts = sorted({c for c in (1, chunk - 1, chunk, chunk + 1, 3 * chunk + 2) if c >= 1})
                cases += [(kind, c, nl, np_, npoly, with_u, N, IO_BUDGET) for c in counts]
                cases += [(kind, 3 * MAX_CHUNK + 2, nl, np_, npoly, with_u, N, HUGE), (kind, 3, nl, np_, npoly, with_u, N, words * 8 - 1), (kind, 2, nl, np_, npoly, with_u, N, 0)]
    return cases


def ws_line_ok(kind, v):
    nct, nl, np_, npoly, with_u, N, budget, words, chunk, nchunks, nbytes, reserve, nat = v[:13]
    at, spans = v[13:13 + nat], list(zip(v[13 + nat::2], v[14 + nat::2]))
    want_words, shares = ws_parent(kind, nl, np_, npoly, with_u, N)
    J = min(nct, MAX_CHUNK, max(1, budget // (want_words * 8)))
    ok = (words, chunk, nbytes, reserve) == (want_words, J, J * want_words * 8, J * want_words * 8 + SLACK) and len(at) == len(shares) + 1 and len(spans) == nchunks
    sizes = [8 if b is None else J * b for b in shares]
    if kind == "CL":
        sizes[-1] = (sizes[-1] + 7) // 8 * 8                # the 32-bit region ends the layout on a whole word
    p = 0
    for off, size in zip(at, sizes):                        # each region where the executor's pointer arithmetic put it: behind the one before, on a word
        ok = ok and off * 8 == p and p % 8 == 0
        p += size
    ok = ok and at[-1] * 8 == p and p <= reserve
    return ok and [s for s, _ in spans] == [c * J for c in range(nchunks)] and sum(c for _, c in spans) == nct and all(1 <= c <= J <= MAX_CHUNK for _, c in spans)


def lift_values(q):
    vals = {0, 1, -1, 2, -2, 19, -19, 38, -38, (1 << 31) - 1, -(1 << 31), -(1 << 31) + 1}
    for k in (1, 2, 3):
        vals |= {k * q - 1, k * q, k * q + 1, -(k * q) - 1, -(k * q), -(k * q) + 1}
    return sorted(v for v in vals if -(1 << 31) <= v < (1 << 31))


def directed_js():
    js = {0, 1, 7, 8, 9, 63, 64, 511, 512, 513, 4095, 4096, 8191, 16383, 16384, 16384 + 511, 32767, 32768, 65535}
    for a in (7, 8, 15, 16, 17, 31, 32, 33, 63, 64, 95, 96, 127):
        for t in (0, 7, 8, 255, 511):
            js.add(512 * a + t)
    return sorted(js)


DECODE_SCALES = [1.0, 2.0 ** 40, 1.2345678e12, 2.0 ** 45 * 2.0 ** 45 / 35184372088891.0]      # powers of two, and what a rescale leaves


@functools.lru_cache(maxsize=None)
def decode_cases():
    """(moduli, residues, scale, p): the directed coefficients of ring_io_ref at one modulus, two, three 61-bit ones, 17 and 48 digits (the most a ring holds: 61-bit
    primes, values up to 2^2927, where the walk must end in an infinity and never a NaN), and random values of every size"""
    chains = [rc.chain("G12")[1][:1], rc.chain("G12")[1], rc.chain("X12")[1], rc.chain("W15")[1], rc.chain("L19")[1], ol.small_primes(12, 61, 48)]
    rnd = np.random.default_rng(96)
    out = []
    for qs in chains:
        Q = prod(qs)
        vals = rio.directed_coefficients(qs)
        for bits in (20, 53, 54, 107, 200, 800, Q.bit_length() - 2):
            if bits <= Q.bit_length() - 2:
                for _ in range(3):
                    v = int.from_bytes(rnd.bytes(bits // 8 + 1), "little") >> (8 - bits % 8)
                    vals += [v, -v]
        for i, p in enumerate(vals):
            scale = DECODE_SCALES[i % len(DECODE_SCALES)]
            x = rio.quotient(p, scale)
            if p and abs(rio.rounded(x)) != float("inf") and rio.boundary_distance(x) <= rio.DECODE_REL:
                continue                    # (an odd 54-bit integer over a power of two is an exact tie: the contract promises nothing there)
            out.append((tuple(qs), tuple(p % q for q in qs), scale, p))
    return out


def _bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


# (hi, lo, band): pairs at exact ties of both signs and sizes, next to them, at the edges of the domain, beyond it, and inside / outside a band
ROUND_CASES = [(2.5, 0.0, 0.0), (-2.5, 0.0, 0.0), (0.5, 0.0, 0.0), (-0.5, 0.0, 0.0), (0.49999999999999994, 0.0, 0.0), (2.5, -2.0 ** -60, 0.0), (2.5, 2.0 ** -60, 0.0),
               (-2.5, 2.0 ** -60, 2.0 ** -70), (2.0 ** 53 + 2, 0.5, 0.0), (-(2.0 ** 53 + 2), -0.5, 0.0), (2.0 ** 61, -0.5, 0.0), (2.0 ** 61, 255.5, 0.0), (2.0 ** 61, -255.75, 0.0),
               (2.0 ** 62, -1.0, 0.0), (-(2.0 ** 62), 1.0, 0.0), (2.0 ** 62, -0.5, 0.0), (2.0 ** 62, 0.0, 0.0), (2.0 ** 63, 0.0, 0.0), (float("nan"), 0.0, 0.0), (float("inf"), 0.0, 0.0),
               (7.25, 0.0, 0.3), (7.25, 0.0, 0.2), (-7.75, 0.0, 0.3), (3.0, -1e-20, 2.0 ** -50), (3.0, 1e-20, 2.0 ** -50), (0.0, 0.0, 2.0 ** -50), (1e-300, 0.0, 2.0 ** -50),
               (123456789.5, 2.0 ** -40, 2.0 ** -50), (123456789.5, 2.0 ** -40, 2.0 ** -30), (-4611686018427387903.0 + 0, 0.0, 0.0)]
REDUCE_MODULI = rc.chain("X12")[1] + rc.chain("X12")[2] + [12289, rc.chain("G12")[1][0]]
BAND_CASES = [0.0, 1.0, 2.0 ** 43, 2.0 ** 43 * (1 + 2.0 ** -52), 2.0 ** 50, 2.0 ** 61.9]


def reduce_values(q):
    return [0, 1, -1, (1 << 62) - 1, -((1 << 62) - 1), q, -q, q - 1, -(q - 1), q + 1, -(q + 1), 2 * q, -2 * q, (1 << 61), -(1 << 61)]


def write_script(path):
    with open(path, "w") as f:
        for q in LIFT_MODULI:
            for v in lift_values(q):
                f.write(f"L {v} {q}\n")
        for r in (0, 0x5555555555555555, 0xAAAAAAAAAAAAAAAA, 0xFFFFFFFFFFFFFFFF, 0x0123456789ABCDEF, 1, 2, 3, 1 << 62, 3 << 62):
            for sh in (0, 2, 30, 32, 60, 62):
                f.write(f"T {r} {sh}\n")
        for j in directed_js():
            f.write(f"J {j}\n")
        for logN in range(12, 17):
            f.write(f"N {logN}\n")
        for c in PLAN_CASES:
            f.write("C " + " ".join(map(str, c)) + "\n")
        for qs, xs, scale, _ in decode_cases():
            f.write(f"G {len(qs)} {' '.join(map(str, qs))} {' '.join(map(str, xs))} {struct.unpack('<Q', struct.pack('<d', scale))[0]}\n")
        for c in DECODE_PLAN_CASES:
            f.write("K " + " ".join(map(str, c)) + "\n")
        for kind, nct, nl, np_, npoly, with_u, N, budget in ws_cases():
            f.write(f"{kind} {nct} {nl} " + (f"{np_} {npoly} {with_u} " if kind == "CL" else "") + f"{N} {budget}\n")
        for hi, lo, band in ROUND_CASES:
            f.write(f"R {_bits(hi)} {_bits(lo)} {_bits(band)}\n")
        for q in REDUCE_MODULI:
            for v in reduce_values(q):
                f.write(f"Q {v} {q}\n")
        for S in BAND_CASES:
            f.write(f"B {_bits(S)}\n")


def mismatches(lines):
    bad = []
    dec = iter(decode_cases())
    for ln in lines:
        t = ln.split()
        op, v = t[0], [int(x) for x in t[1:]]
        if op == "L":
            x, q, r = v
            ok = 0 <= r < q and r == x % q
        elif op == "T":
            r, sh, s = v
            b0, b1 = (r >> sh) & 1, (r >> (sh + 1)) & 1
            ok = s == ((-1 if b1 else 1) if b0 else 0)
        elif op == "J":
            j, tt, a, ub, uw, us, eb, ew = v
            ok = (tt, a) == (j & 511, j >> 9) and j == 512 * a + tt and ub == (tt >> 3) + 64 * (a >> 5) and uw == 2 * (tt & 7) and us == 2 * (a & 31) \
                and eb == tt + 512 * (a >> 3) and ew == 2 * (a & 7)
        elif op == "N":
            logN, nu, ne, mu, me = v
            N = 1 << logN
            ok = nu == 64 * -(-(N // 512) // 32) and ne == 512 * (N // 4096) and mu == nu - 1 and me == ne - 1 and ne * 8 == N and nu * 256 >= N
        elif op == "C":
            nct, nl, np_, npoly, with_u, N, budget, words, chunk, nchunks, nbytes = v[:11]
            spans = list(zip(v[11::2], v[12::2]))
            nt = nl + np_
            want_words = ((nt if with_u else 0) + npoly * nt + npoly * np_ + npoly * nl) * N + (npoly * N + 1) // 2
            ok = words == want_words and len(spans) == nchunks
            if nct == 0:
                ok = ok and chunk == 0 and nchunks == 0
            else:
                ok = ok and 1 <= chunk <= min(nct, 256) and nbytes == chunk * words * 8 and (nbytes <= budget or chunk == 1)
                ok = ok and (chunk == min(nct, 256) or (chunk + 1) * words * 8 > budget)                 # as large as the budget allows
                ok = ok and [s for s, _ in spans] == list(range(0, nct, chunk)) and sum(n for _, n in spans) == nct and all(1 <= n <= chunk for _, n in spans)
        elif op == "G":
            qs, xs, scale, p = next(dec)
            k = v[0]
            digits, mag, bits = v[1:1 + k], v[1 + k:1 + 2 * k], v[1 + 2 * k]
            assert rio.crt_centred(xs, qs) == p
            want = rio.rounded(rio.quotient(p, scale))
            ok = k == len(qs) and digits == rio.mixed_radix(p % prod(qs), qs) and mag == rio.mixed_radix(abs(p), qs) and bits == struct.unpack("<Q", struct.pack("<d", want))[0]
        elif op == "K":
            nct, nl, N, budget, words, chunk, nchunks, nbytes = v
            ok = words == (nl + 1) * N and nbytes == chunk * words * 8
            ok = ok and ((nct == 0 and chunk == 0 and nchunks == 0) or (1 <= chunk <= min(nct, 256) and nchunks == -(-nct // chunk) and (nbytes <= budget or chunk == 1)))
        elif op in ("CL", "KL", "EL", "VL"):
            ok = ws_line_ok(op, v)
        elif op == "R":
            hi, lo, band = (struct.unpack("<d", struct.pack("<Q", b))[0] for b in v[:3])
            st, pp = v[3], v[4]
            if hi != hi or abs(hi) > 2.0 ** 62:
                ok = st == 2
            else:
                x = Fraction(hi) + Fraction(lo)
                a = abs(x)
                m = int(a + Fraction(1, 2))                       # floor(|x| + 1/2): half away from zero
                if m >= 1 << 62:
                    ok = st == 2
                else:
                    dist = abs(a - int(a) - Fraction(1, 2))
                    ok = pp == (-m if x < 0 else m) and st == (1 if dist <= Fraction(band) else 0)
        elif op == "Q":
            pp, q, r_ = v
            ok = r_ == pp % q
        elif op == "B":
            S = struct.unpack("<d", struct.pack("<Q", v[0]))[0]
            ok = v[1] == _bits(max(2.0 ** -50, 2.0 ** -93 * S))
        else:
            ok = op == "OK"
        if not ok:
            bad.append(ln[:300])
    return bad


@pytest.fixture(scope="module")
def script(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("gring_io") / "script.txt")
    write_script(path)
    return path


def run(exe, script):
    out = subprocess.run([exe, script], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("OK"), out.stdout[-2000:] + out.stderr[-4000:]
    return out.stdout.splitlines()


def test_arithmetic_matches_python_integers_under_the_sanitizers(tmp_path, script):
    lines = run(_compile(str(tmp_path / "host_gring_io_test"), CSRC, sanitize=True), script)
    assert len(lines) == sum(1 for _ in open(script)) + 1
    assert sum(ln[0] == "G" for ln in lines) == len(decode_cases()) and sum(ln.split()[0] == "K" for ln in lines) == len(DECODE_PLAN_CASES)
    assert sum(ln[:2] in ("CL", "KL", "EL", "VL") for ln in lines) == len(ws_cases()) > 1000
    assert sum(ln.split()[0] == "L" for ln in lines) >= 12 * len(LIFT_MODULI) and sum(ln.split()[0] == "C" for ln in lines) == len(PLAN_CASES)
    bad = mismatches(lines)
    assert not bad, bad[:10]


def test_directed_operands_reach_the_edges_the_mutants_need():
    """a negative multiple of a modulus (the lift's -0), a coefficient with a >= 16 whose low four bits differ from its low five, one whose a + 1 crosses a multiple
    of 8, and a call that the chunk cap - not the budget - splits"""
    assert any(v < 0 and v % q == 0 for q in LIFT_MODULI for v in lift_values(q))
    assert any((j >> 9) & 31 != (j >> 9) & 15 for j in directed_js()) and any(((j >> 9) + 1) >> 3 != (j >> 9) >> 3 for j in directed_js())
    assert any(c[0] > 256 for c in PLAN_CASES)


def test_decode_operands_are_outside_the_stated_distance_and_reach_the_edges():
    """the contract is conditional: no finite non-zero quotient of the cases lies within 2^-96 relative of a rounding boundary.  And the cases hold Q/2 and the value
    one past it, a negative value whose carry runs through every digit, 48 digits, a result beyond the double range, and a scale that is no power of two"""
    finite = 0
    for qs, xs, scale, p in decode_cases():
        x = rio.quotient(p, scale)
        if p and abs(rio.rounded(x)) != float("inf"):
            assert rio.boundary_distance(x) > rio.DECODE_REL, (len(qs), p, scale)
            finite += 1
    assert finite > 200
    cases = decode_cases()
    assert any(p == prod(qs) // 2 for qs, _, _, p in cases) and any(p == -(prod(qs) // 2) for qs, _, _, p in cases)
    assert any(p < 0 and len(qs) > 2 and all(d == 0 for d in rio.mixed_radix(p % prod(qs), qs)[:-1]) for qs, _, _, p in cases)
    assert any(len(qs) == 48 and rio.rounded(rio.quotient(p, s)) == float("-inf") for qs, _, s, p in cases)
    assert any(len(qs) == 48 and 0 < abs(p) < 1 << 900 and s != 1.0 for qs, _, s, p in cases)


@pytest.mark.parametrize("logN", [12, 13, 16])
def test_exact_encoder_and_exact_decoder_round_trip(logN):
    """exactref.encode -> decode_ref.decode gives the slots back: every coefficient moved by at most 1/2 in rounding, so a slot moves by at most N / 2 / scale (plus
    the decoder's own error bound); the imaginary parts are that small too"""
    N, scale = 1 << logN, 2.0 ** 40
    v = np.random.default_rng(logN).uniform(-4, 4, N // 2)
    p, tie, err = exactref.encode(v, N, scale)
    assert float(np.min(tie)) > err
    re, im, derr = decode_ref.decode(p, N, scale)
    bound = Fraction(N, 2) / Fraction(scale) + derr
    assert max(abs(a - Fraction(float(b))) for a, b in zip(re, v)) <= bound and max(abs(a) for a in im) <= bound


MUTANTS = {
    "a tie rounded towards zero": ("gring_io_arith.hpp", "m += d >= 0.0 ? 1 : 0;", "m += d > 0.0 ? 1 : 0;"),
    "the sign of the 62-bit reduction dropped": ("gring_io_arith.hpp", "return (p < 0 && m) ? q - m : m;", "return m;"),
    "the band test without its floor": ("gring_io_arith.hpp", "return b > kEncBandFloor ? b : kEncBandFloor; }", "return b; }"),
    "the carry of the complement dropped": ("gring_io_arith.hpp", "if (m == q) { m = 0; carry = 1; } else carry = 0;", "if (m == q) { m = 0; carry = 0; } else carry = 0;"),
    "Q/2 itself taken as negative": ("gring_io_arith.hpp", "return state ? state : (d > h ? 1 : (d < h ? -1 : 0));", "return state ? state : (d >= h ? 1 : -1);"),
    "the product's cross term with the low part dropped": ("gring_io_arith.hpp", "e = __builtin_fma(a.hi, b.lo, e); e = __builtin_fma(a.lo, b.hi, e);", "e = __builtin_fma(a.hi, b.lo, e);"),
    "the lift of a negative multiple of q left at q": ("gring_io_arith.hpp", "return (w < 0 && m) ? q - m : m;", "return (w < 0) ? q - m : m;"),
    "the u shift taken modulo 16 coefficients": ("gring_io_arith.hpp", "GR_HD int samp_u_shift(int a) { return 2 * (a & 31); }", "GR_HD int samp_u_shift(int a) { return 2 * (a & 15); }"),
    "an off-by-one in the Gaussian block index": ("gring_io_arith.hpp", "return (unsigned)(t + kSampT * (a >> 3));", "return (unsigned)(t + kSampT * ((a + 1) >> 3));"),
    "a region left out of the encryption core's layout": ("gring_io_plan.hpp", "l.Y2 = c.take(J * npoly * np * N);", "l.Y2 = c.at;"),
    "the encoder's tail carved from the slack": ("gring_io_plan.hpp", "(size_t)nl * N + 8, budget_bytes); }", "(size_t)nl * N, budget_bytes); }"),
    "the chunk cap dropped": ("gring_io_plan.hpp", "if (fit > (size_t)GriPlan::kMaxChunk) fit = GriPlan::kMaxChunk;", ""),
}


@pytest.mark.parametrize("name", list(MUTANTS))
def test_planted_mistake_is_caught_by_the_directed_operands(tmp_path, script, name):
    which, old, new = MUTANTS[name]
    inc = tmp_path / "inc"
    inc.mkdir()
    for hdr in HEADERS:
        text = open(os.path.join(CSRC, hdr)).read()
        if hdr == which:
            assert text.count(old) == 1, f"the line this mutant replaces is gone from {hdr}"
            text = text.replace(old, new)
        (inc / hdr).write_text(text)
    lines = run(_compile(str(tmp_path / "mutant"), str(inc), sanitize=False), script)
    assert mismatches(lines), f"not caught: {name}"


def test_headers_are_host_only():
    """the new headers compile as plain C++17 and pull in no HIP header"""
    for hdr in ("gring_io_arith.hpp", "gring_io_plan.hpp"):
        deps = subprocess.run(["g++", "-std=c++17", "-x", "c++", "-M", os.path.join(CSRC, hdr)], capture_output=True, text=True)
        assert deps.returncode == 0, deps.stderr
        assert "hip" not in deps.stdout.replace(ROOT, "").lower(), deps.stdout
