"""The general ring's collective bootstrap (sfgwas_amd/csrc/gring_refresh.hip) stated in Python integers - the only source of expected values of
tests/test_ring_refresh_ref.py and tests/test_gpu_ring_refresh.py, as tests/refresh_ref.py is for the PN14 path.

  * the statement: int(f) for the scales, the truncating quo, the tie x == floor(Q / 2) counted as negative (expected_shares, expected_finish);
  * WideRing: a ring of any modulus count, its transforms served by as many 16-modulus oracle rings as it takes;
  * the chains: G12, G13, W15, W16, X12, L19, P14 of ring_cases, M48 of ring_cases' edge chains (47 + 1 moduli of 61 bits: Q_46 has 2867 bits, the widest integer the
    ring admits) and M33 (32 + 1 moduli: a middle width) defined here;
  * directed plaintext integers, masks and scale pairs, placed at coefficients 0, 63, 64, 255, 256, N - 1 and a seeded spread, the rest a seeded random fill;
  * a limb-level model of gring_refresh_arith.hpp (lists of 64-bit words) with planted mistakes and a record of the branch classes its inputs take.
PARITY UNPINNED like the PN14 path: the semantics are lattigo v2.1.0 / v2.2.0 dckks/refresh.go as oracle/sfgwas_oracle.c restates them.
"""
import functools
import random
from math import prod

import numpy as np

import oracle_lib as ol
import refresh_ref as rr
import ring_cases as rc

BIG_LIMBS = 48                               # grf::kBigLimbs
BIG_BITS = 64 * BIG_LIMBS
M64 = (1 << 64) - 1
CHUNK_CAP = 1024                             # kGrfMaxChunk
FIXED_PLACES = (0, 63, 64, 255, 256)         # and N - 1: both tile widths (64 coefficients a wave of the multi-word kernels, 256 a block of the others)
NAMES = ["G12", "G13", "W15", "W16", "X12", "L19", "P14", "M48", "M33"]


@functools.lru_cache(maxsize=None)
def chain(name):
    """-> (logN, q, p)"""
    if name == "M33":
        m = ol.small_primes(12, 61, 33)
        return 12, m[:32], m[32:]
    return rc.chain(name)


def levels(name):
    """top (= nq - 1: no new modulus), one in the middle, 0"""
    top = len(chain(name)[1]) - 1
    return sorted({top, top // 2, 0}, reverse=True)


class WideRing:
    """transforms at any number of moduli: groups of at most 16, each an oracle ring (its last modulus stands as that ring's P)"""
    GROUP = 16

    def __init__(self, logN, q, p):
        self.logN, self.N, self.nq, self.np_ = logN, 1 << logN, len(q), len(p)
        self.moduli = list(q) + list(p)
        cuts, n = [], len(self.moduli)
        i = 0
        while i < n:
            size = min(self.GROUP, n - i)
            if n - i - size == 1:                # never leave a group of one behind
                size -= 1
            cuts.append((i, i + size))
            i += size
        self.parts = [(a, ol.Ring(logN, self.moduli[a:b - 1], self.moduli[b - 1:b])) for a, b in cuts]

    def _at(self, mod):
        for off, r in reversed(self.parts):
            if mod >= off:
                return r, mod - off
        raise IndexError(mod)

    def ntt(self, mod, a):
        r, m = self._at(mod)
        return r.ntt(m, a)

    def intt(self, mod, a):
        r, m = self._at(mod)
        return r.intt(m, a)


@functools.lru_cache(maxsize=None)
def ring_of(name):
    return WideRing(*chain(name))


# ---------------------------------------------------------------- the statement in Python integers
quo = rr.quo                                  # big.Int.Quo: truncated towards zero


def unscaled(scales):
    return scales is None or scales[0] == scales[1]


def rescaled(v, scales, mutant=None):
    if unscaled(scales):
        return v
    num, den = v * int(scales[1]), int(scales[0])
    return num // den if mutant == "floor" else quo(num, den)


def recentred(x, Q, mutant=None):
    """x in [0, Q): lattigo's refresh takes x >= floor(Q / 2) as negative"""
    neg = x > Q // 2 if mutant == "sign_gt" else x >= Q // 2
    return x - Q if neg else x


def _obj(a):
    a = np.asarray(a)
    return a.astype(object) if a.dtype != object else a       # numpy integers become Python integers


def rows_of(vals, moduli):
    """[len(moduli)][N] canonical residues of signed Python integers"""
    v = _obj(vals)
    return np.stack([(v % q).astype(np.uint64) for q in moduli])


def expected_shares(ring, level, ct, sk, crs, masks, e0, e1, scales=None):
    """one ciphertext: ct [2][nl][N], sk, crs [nq][N], masks N signed integers, e0, e1 [N] -> (h0 [nl][N], h1 [nq][N])"""
    nl, nq, q = level + 1, ring.nq, ring.moduli
    r0 = rows_of([m + int(e) for m, e in zip(masks, e0)], q[:nl])
    r1 = rows_of([rescaled(m, scales) + int(e) for m, e in zip(masks, e1)], q[:nq])
    h0 = np.stack([((_obj(ring.ntt(j, r0[j])) + _obj(sk[j]) * _obj(ct[1, j])) % q[j]).astype(np.uint64) for j in range(nl)])
    h1 = np.stack([((-(_obj(ring.ntt(j, r1[j])) + _obj(sk[j]) * _obj(crs[j]))) % q[j]).astype(np.uint64) for j in range(nq)])
    return h0, h1


def plaintext_of(ring, level, ct, h0agg):
    """x in [0, Q_level) of every coefficient: INTT_level(c0 + h0agg), then the CRT"""
    nl, q = level + 1, ring.moduli
    Q = prod(q[:nl])
    x = np.zeros(ring.N, dtype=object)
    for j in range(nl):
        r = ring.intt(j, ((_obj(ct[0, j]) + _obj(h0agg[j])) % q[j]).astype(np.uint64))
        x = x + _obj(r) * ((Q // q[j]) * pow(Q // q[j], -1, q[j]))
    return [int(v) for v in x % Q]


def expected_finish_of_x(ring, level, xs, h1agg, crs, scales=None, mutant=None):
    """the refreshed ciphertext [2][nq][N] of one ciphertext whose plaintext integers are xs (in [0, Q_level))"""
    nq, q = ring.nq, ring.moduli
    Q = prod(q[:level + 1])
    rows = rows_of([rescaled(recentred(x, Q, mutant), scales, mutant) for x in xs], q[:nq])
    out = np.zeros((2, nq, ring.N), dtype=np.uint64)
    for j in range(nq):
        out[0, j] = ((_obj(ring.ntt(j, rows[j])) + _obj(h1agg[j])) % q[j]).astype(np.uint64)
        out[1, j] = crs[j]
    return out


def expected_finish(ring, level, ct, h0agg, h1agg, crs, scales=None):
    return expected_finish_of_x(ring, level, plaintext_of(ring, level, ct, h0agg), h1agg, crs, scales)


def ct_of_x(ring, level, xs, h0agg, c1):
    """a ciphertext [2][nl][N] with c0 + h0agg = NTT(x): the finish then sees exactly the integers xs"""
    nl, q = level + 1, ring.moduli
    xr = rows_of(xs, q[:nl])
    c0 = np.stack([((_obj(ring.ntt(j, xr[j])) - _obj(h0agg[j])) % q[j]).astype(np.uint64) for j in range(nl)])
    return np.stack([c0, np.ascontiguousarray(c1, dtype=np.uint64)])


# ---------------------------------------------------------------- scale pairs
PAIRS = dict(rr.PAIRS)
REFERENCE_PAIRS = rr.REFERENCE_PAIRS
# the capacity at M48's top level: bits(Q_46) = 2867, so sh = 3070 - 54 - 2867 = 149 just fits and 150 misses by one bit (Int(2^52) = 2^52 2^0, Int(2^201) = 2^52 2^149)
PAIRS["fit"] = (2.0 ** 52, 2.0 ** 201)
PAIRS["miss"] = (2.0 ** 52, 2.0 ** 202)
ALL_PAIRS = ["ref", "ref_np2", "one", "r64", "r70", "l64", "l75", "d1", "np2_l48", "np2_up"]
# what each of the issue's classes is served by: the reference's two; ratio 1; right and left shifts across a word boundary with bs == 0 and bs != 0;
# Int(ct scale) = 1; non-powers of two with an inexact division; fit / miss (M48's top level only: no other chain reaches the capacity below the scale limit 2^400)
TWO_PAIRS = {"G12": ["ref", "l75"], "G13": ["ref_np2", "r64"], "W15": ["ref", "np2_l48"], "W16": ["ref_np2", "l64"], "X12": ["r70", "d1"], "L19": ["ref", "np2_up"],
             "M33": ["ref_np2", "l75"]}


def pairs_of(name, level):
    if name == "P14":
        return list(ALL_PAIRS)
    if name == "M48":
        return ALL_PAIRS + (["fit"] if level == len(chain(name)[1]) - 1 else [])
    return TWO_PAIRS[name]


def scale_parts(f):
    return rr.scale_parts(f)


def ratio(scales):
    return rr.ratio(scales)


def q_bits(name, level):
    return prod(chain(name)[1][:level + 1]).bit_length()


def fits_q(bits, sh):
    return bits + 54 + max(sh, 0) <= BIG_BITS - 2


def fits_mask(W, sh):
    return 64 * W + 54 + max(sh, 0) <= BIG_BITS


def limbs_for(bits, sh):
    return (bits + 54 + max(sh, 0) + 63) // 64


def mask_limbs_of(name, level, scales):
    """one limb more than Q_level needs (a mask wider than Q_level), as far as the share form's fit check lets it"""
    W = (q_bits(name, level) + 63) // 64 + 1
    r = None if unscaled(scales) else ratio(scales)
    cap = BIG_LIMBS if r is None else (BIG_BITS - 54 - max(r[2], 0)) // 64
    return max(1, min(W, cap))


# ---------------------------------------------------------------- directed inputs
def directed_x(q_all, level, scales=None):
    nl = level + 1
    mods = q_all[:nl]
    Q = prod(mods)
    half = Q // 2
    xs = [0, 1, half - 1, half, half + 1, Q - 1]
    hd = rr.to_digits(half, mods)
    if nl > 1:                                   # every digit but the top equal to the half's
        for top in {0, max(hd[-1] - 1, 0), min(hd[-1] + 1, mods[-1] - 1), mods[-1] - 1}:
            xs.append(rr.from_digits(hd[:-1] + [top], mods))
    for qj in q_all[nl:nl + 2]:                  # == 0 modulo a new modulus, on both sides of the sign (unscaled: x - Q == 0; scaled: the rescaled magnitude == 0)
        xs += [qj % Q if qj < half else 0, 3 * qj if 3 * qj < half else 0]
        if not unscaled(scales):
            it, ic = int(scales[1]), int(scales[0])
            for k in (1, 5):
                t = -(-(k * qj * ic) // it)      # the least t with floor(t it / ic) >= k qj
                if quo(t * it, ic) == k * qj and 0 < t <= Q - half:
                    xs += [Q - t, t if t < half else 0]
        else:
            for k in (1, 7):
                if k * qj <= Q - half:
                    xs.append(Q - k * qj)
    return [x for x in xs if 0 <= x < Q]


def directed_masks(q_all, level, W, scales=None):
    nl = level + 1
    Q = prod(q_all[:nl])
    top = 1 << (64 * W - 1)
    ms = [0, 1, -1, -top, top - 1, -(top - 1), top >> 1, -(top >> 1)]
    if W >= 2:
        ms += [(1 << (64 * (W - 1))) - 1, -((1 << (64 * (W - 1))) - 1), 1 << (64 * (W - 1)), -(1 << (64 * (W - 1)))]      # all-ones limbs under a zero top limb; a lone top limb
    for qj in (q_all[0], q_all[-1]):
        for k in (1, 12345):
            ms += [k * qj, -k * qj]
            if not unscaled(scales):
                it, ic = int(scales[1]), int(scales[0])
                t = -(-(k * qj * ic) // it)
                if quo(t * it, ic) == k * qj:
                    ms += [t, -t]
    ms += [Q + 12345, -(Q + 12345), Q, -Q]      # wider than Q_level (kept only where W holds them)
    if not unscaled(scales):
        ic = int(scales[0])
        ms += [ic - 1, -(ic - 1), ic, -ic]      # magnitudes around one unit of the quotient: a negative one that rescales to 0
    return [m for m in ms if -top <= m < top]


def places(N, count, seed):
    """count distinct coefficients: 0, 63, 64, 255, 256, N - 1 first, then a seeded spread"""
    fixed = list(FIXED_PLACES) + [N - 1]
    rnd = random.Random(seed)
    rest = rnd.sample([i for i in range(N) if i not in fixed], max(count - len(fixed), 0))
    return (fixed + rest)[:max(count, len(fixed))]


def placed(directed, fill, N, seed):
    """fill(rnd) everywhere, the directed values at places(): every one at least once, the six fixed places cycling through the first"""
    rnd = random.Random(seed)
    out = [fill(rnd) for _ in range(N)]
    at = places(N, len(directed), seed + 1)
    for i, pos in enumerate(at):
        out[pos] = directed[i % len(directed)]
    return out


def limbs_of(vals, W):
    """signed integers -> two's-complement limbs uint64 [len][W]"""
    out = np.zeros((len(vals), W), dtype=np.uint64)
    for c, v in enumerate(vals):
        u = v % (1 << (64 * W))
        for i in range(W):
            out[c, i] = (u >> (64 * i)) & M64
    return out


class Inputs:
    pass


@functools.lru_cache(maxsize=None)
def secret_of(name, seed=7):
    ring = ring_of(name)
    rnd = np.random.default_rng(seed)
    s = rnd.integers(-1, 2, ring.N)
    return np.stack([ring.ntt(j, np.where(s < 0, q - 1, s).astype(np.uint64)) for j, q in enumerate(ring.moduli[:ring.nq])])


def uniform_rows(rnd, moduli, N):
    return np.stack([rnd.integers(0, q, N, dtype=np.uint64) for q in moduli])


def _narrowed(rnd, v, bound):
    """the seeded fill: a quarter of the values at full width, the rest shifted down to a random width, so that every limb count below the widest occurs (and the
    Python integers of the expected values stay affordable); a narrowed value keeps its sign, and for a plaintext integer x the negative side is Q - |v|"""
    if rnd.randrange(4) == 0:
        return v
    w = v >> rnd.randrange(bound.bit_length())
    return -w if rnd.randrange(2) else w


def case_inputs(name, level, pair, nct=3, seed=1, wide_errors=True, W=None):
    """everything one word-for-word case needs; ciphertext 0 carries the directed values, the others more of the seeded fill.  wide_errors: errors up to
    2^31 in magnitude, above the smallest moduli (the oracle lifts an error without reducing it, so its comparison keeps them at 19)"""
    ring = ring_of(name)
    scales = None if pair is None else PAIRS[pair]
    q, nl, N = ring.moduli[:ring.nq], level + 1, ring.N
    Q = prod(q[:nl])
    W = mask_limbs_of(name, level, scales) if W is None else W
    rnd = np.random.default_rng(seed)
    inp = Inputs()
    inp.name, inp.level, inp.scales, inp.W, inp.ring = name, level, scales, W, ring
    bound = min(1 << (64 * W - 1), max(Q >> 3, 2))
    inp.masks, inp.xs = [], []
    for c in range(nct):
        dm = directed_masks(q, level, W, scales) if c == 0 else [0]
        dx = directed_x(q, level, scales) if c == 0 else [0]
        inp.masks.append(placed(dm, lambda r: _narrowed(r, r.randrange(-bound, bound), bound), N, seed + 10 * c))
        inp.xs.append(placed(dx, lambda r: _narrowed(r, r.randrange(Q), Q) % Q, N, seed + 10 * c + 5))
    inp.mask_limbs = np.stack([limbs_of(m, W) for m in inp.masks])
    e_edges = [0, 19, -19, (1 << 31) - 1, -(1 << 31)] if wide_errors else [0, 19, -19]
    inp.e0 = rnd.integers(-19, 20, (nct, N)).astype(np.int32)
    inp.e1 = rnd.integers(-19, 20, (nct, N)).astype(np.int32)
    inp.e0[0, :len(e_edges)] = e_edges
    inp.e1[0, 64:64 + len(e_edges)] = e_edges
    inp.sk = secret_of(name)
    inp.crs = np.stack([uniform_rows(rnd, q, N) for _ in range(nct)])
    inp.h0agg = np.stack([uniform_rows(rnd, q[:nl], N) for _ in range(nct)])
    inp.h1agg = np.stack([uniform_rows(rnd, q, N) for _ in range(nct)])
    inp.cts = np.stack([ct_of_x(ring, level, inp.xs[c], inp.h0agg[c], uniform_rows(rnd, q[:nl], N)) for c in range(nct)])
    return inp


def expected_of(inp):
    """-> (h0 [nct][nl][N], h1 [nct][nq][N], out [nct][2][nq][N])"""
    nct = len(inp.xs)
    sh = [expected_shares(inp.ring, inp.level, inp.cts[c], inp.sk, inp.crs[c], inp.masks[c], inp.e0[c], inp.e1[c], inp.scales) for c in range(nct)]
    out = [expected_finish_of_x(inp.ring, inp.level, inp.xs[c], inp.h1agg[c], inp.crs[c], inp.scales) for c in range(nct)]
    return np.stack([s[0] for s in sh]), np.stack([s[1] for s in sh]), np.stack(out)


# ---------------------------------------------------------------- the limb-level model of gring_refresh_arith.hpp, with planted mistakes
MUTANTS = ["sign_gt",            # > for >= in the sign rule
           "floor",              # floor for truncation (the sign applied before the division)
           "drop_carry_mul",     # mul_add loses the carry between limbs
           "drop_carry_neg",     # to_magnitude's + 1 stops at limb 0
           "neg_zero",           # a negative magnitude == 0 mod q gives q
           "drop_borrow",        # rsub loses the borrow
           "shift_word_only"]    # the shift ignores its bit part
# classes unreachable by construction: a carry out of limb n - 1 of mul_add, a bit shifted out of the top by a left shift, a borrow out of rsub's top limb (the two
# fit checks and x < Q_level exclude them); to_magnitude's carry out of limb W - 1 (only -0 would produce it)
UNREACHABLE = ["mul_carry_out_of_top", "shift_left_loses_bits", "rsub_borrow_out_of_top", "negate_carry_out_of_top"]
CLASSES = ["sign_neg", "sign_pos", "negate_carry", "negate_no_carry", "mul_carry", "mul_no_carry", "d_is_1", "d_above_1", "res0_of_negative", "res_of_negative",
           "rsub_borrow", "rsub_no_borrow", "sign_tie", "sign_decided_at_top", "sign_decided_below_top", "rescale_to_zero_neg", "digits_carry_opens_limb"]


def m_to_magnitude(limbs, cls, mutant=None):
    W = len(limbs)
    neg = limbs[W - 1] >> 63 != 0
    if neg:
        cy, out = 1, []
        for i, w in enumerate(limbs):
            v = ((w ^ M64) + cy) & M64
            nxt = 1 if (cy and v == 0) else 0
            if mutant == "drop_carry_neg" and i == 0:
                nxt = 0
            cls.add("negate_carry" if nxt else "negate_no_carry")
            cy = nxt
            out.append(v)
        limbs = out
    cls.add("sign_neg" if neg else "sign_pos")
    return neg, list(limbs)


def m_mul_add(a, m, add, cls, mutant=None):
    c, out = add, []
    for w in a:
        t = w * m + c
        out.append(t & M64)
        c = 0 if mutant == "drop_carry_mul" else t >> 64
        cls.add("mul_carry" if t >> 64 else "mul_no_carry")
    return out, c


def m_shift(a, sh, cls, mutant=None):
    n = len(a)
    if sh == 0:
        cls.add("shift_none")
        return list(a)
    k = abs(sh)
    ws, bs = k >> 6, (0 if mutant == "shift_word_only" else k & 63)
    cls.add(rr.shift_class(sh))
    g = lambda i: a[i] if 0 <= i < n else 0
    if sh > 0:
        return [((g(i - ws) << bs) | (g(i - ws - 1) >> (64 - bs))) & M64 if bs else g(i - ws) for i in range(n)]
    return [((g(i + ws) >> bs) | (g(i + ws + 1) << (64 - bs))) & M64 if bs else g(i + ws) for i in range(n)]


def m_div_small(a, d, cls):
    if d == 1:
        cls.add("d_is_1")
        return list(a)
    cls.add("d_above_1")
    r, out = 0, [0] * len(a)
    for i in range(len(a) - 1, -1, -1):
        qw = 0
        for b in range(7, -1, -1):
            r = (r << 8) | ((a[i] >> (8 * b)) & 0xFF)
            assert r < 1 << 61
            qb = r // d
            r -= qb * d
            qw = (qw << 8) | qb
        out[i] = qw
    return out


def m_rescale(a, r, cls, mutant=None):
    mo, mi, sh = r
    a, _ = m_mul_add(a, mo, 0, cls, mutant)
    return m_div_small(m_shift(a, sh, cls, mutant), mi, cls)


def m_rsub(a, b, cls, mutant=None):
    br, out = 0, []
    for ai, bi in zip(a, b):
        d = bi - ai - br
        out.append(d & M64)
        br = 0 if mutant == "drop_borrow" else (1 if d < 0 else 0)
        cls.add("rsub_borrow" if d < 0 else "rsub_no_borrow")
    return out


def m_int(a):
    return sum(w << (64 * i) for i, w in enumerate(a))


def m_residue(a, neg, q, cls, mutant=None):
    m = m_int(a) % q                             # the Horner through barrett128 is exact: the host program pins it word by word
    if neg:
        cls.add("res0_of_negative" if m == 0 else "res_of_negative")
        return q - m if (m or mutant == "neg_zero") else 0
    return m


def model_share_rows(limbs, e, moduli, scales, cls, mutant=None):
    """one coefficient: its W two's-complement limbs -> (mask' + e) mod q_j for every modulus, through the limb functions"""
    W = len(limbs)
    neg, a = m_to_magnitude(limbs, cls, mutant)
    if not unscaled(scales):
        r = ratio(scales)
        a = m_rescale(a + [0] * (limbs_for(64 * W, r[2]) - W), r, cls, mutant)
        if mutant == "floor" and neg and m_int(a) * int(scales[0]) != m_int(m_to_magnitude(limbs, set())[1]) * int(scales[1]):
            a = m_mul_add(a, 1, 1, set())[0]     # floor of a negative quotient: one more in magnitude when the division is inexact
        if neg and m_int(a) == 0:
            cls.add("rescale_to_zero_neg")
    return [(m_residue(a, neg, q, cls, mutant) + e) % q for q in moduli]


def model_recode(x, level, q_all, scales, cls, mutant=None):
    """one coefficient of the finish: x in [0, Q_level) -> its residue at every modulus of Q, through digits, sign, limbs"""
    nl, nq = level + 1, len(q_all)
    mods = q_all[:nl]
    Q = prod(mods)
    d, h = rr.to_digits(x, mods), rr.to_digits(Q // 2, mods)
    st = 0
    for i in range(nl - 1, -1, -1):
        if st == 0 and d[i] != h[i]:
            st = 1 if d[i] > h[i] else -1
            cls.add("sign_decided_at_top" if i == nl - 1 else "sign_decided_below_top")
    if st == 0:
        cls.add("sign_tie")
    neg = st > 0 if mutant == "sign_gt" else st >= 0
    cls.add("sign_neg" if neg else "sign_pos")
    if unscaled(scales):
        out = [x % q for q in mods]
        for qj in q_all[nl:nq]:
            v = rr.from_digits(d, mods) % qj
            out.append((v - Q % qj) % qj if neg else v)
        return out
    r = ratio(scales)
    n = limbs_for(Q.bit_length(), r[2])
    a, ln = [d[nl - 1]], 1
    for i in range(nl - 2, -1, -1):
        a, c = m_mul_add(a, mods[i], d[i], cls, mutant)
        if ln < n:
            a.append(c)
            ln += 1
            if c:
                cls.add("digits_carry_opens_limb")
    a += [0] * (n - ln)
    if neg:
        a = m_rsub(a, [(Q >> (64 * i)) & M64 for i in range(n)], cls, mutant)
    before = m_int(a)
    a = m_rescale(a, r, cls, mutant)
    if mutant == "floor" and neg and m_int(a) * int(scales[0]) != before * int(scales[1]):
        a = m_mul_add(a, 1, 1, set())[0]
    if neg and m_int(a) == 0:
        cls.add("rescale_to_zero_neg")
    return [m_residue(a, neg, q, cls, mutant) for q in q_all[:nq]]
