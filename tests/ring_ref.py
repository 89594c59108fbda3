"""Test-side references of the general ring beyond what one oracle ring holds.

  * SplitRing: a ring of up to 48 moduli, its transforms served by ceil(nmod / 15) oracle rings that together hold every modulus (the oracle's stack arrays and
    sums were written for ORC_MAXMOD = 16 moduli, so that limit stays);
  * extend_rows(): the float-corrected basis extension on whole rows.  A digit's constants - (D / q_m)^-1 mod q_m, D / q_m mod q_t, D mod q_t - are computed once
    per digit, not per word; the float sum is float64 numpy, one IEEE division per term, added in modulus order, truncated.  On request it returns the class
    v_float - v_exact of every word, and it can make one of three MISTAKES on purpose (the discrimination tests of tests/test_ring_edges_ref.py);
  * keyswitch(): orc_keyswitch restated in Python integers, vectorised over the coefficients (numpy object arrays); the transforms are the oracle's.
    trace=True also returns the classes per digit and per ModDown plane;
  * directed_ct(), identity_key(): the inputs that put the key switch's and ModDown's float sums on both integer boundaries;
  * rescale_model(): orc_rescale in Python integers;
  * decode(): slot values of a coefficient vector (plain complex FFT - the end-to-end tests compare within the scheme's noise, far above fp64's);
  * crt_centered(): residue rows -> signed Python integers.
"""
import functools
from math import prod

import numpy as np

import ksw_ref
import oracle_lib as ol

GROUP = 15                                   # moduli per oracle ring: one below ORC_MAXMOD
MISTAKES = ("recip", "round", "exact")       # y * fl(1/q) in place of y / q; v rounded, not truncated; v exact, not float
KEY_SEED, CT_SEED = 19, 3                    # the uniform key and the ciphertexts the CPU file judges and the GPU file runs


class SplitRing:
    def __init__(self, logN, q, p):
        self.logN, self.N, self.nq, self.np_ = logN, 1 << logN, len(q), len(p)
        self.moduli = list(q) + list(p)
        self.slots, self.beta = self.N // 2, (len(q) + len(p) - 1) // len(p)
        n = len(self.moduli)
        k = -(-n // GROUP)                                                           # groups as even as they come: 19 -> 10 + 9, 38 -> 13 + 13 + 12, 48 -> 4 x 12
        cuts = [n * i // k + (n * i % k > 0) for i in range(k + 1)]
        assert n >= 2 and all(b - a >= 2 for a, b in zip(cuts, cuts[1:]))            # an oracle ring needs a q and a p
        self.parts = [(a, ol.Ring(logN, self.moduli[a:b - 1], self.moduli[b - 1:b])) for a, b in zip(cuts, cuts[1:])]

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

    def galois(self, k):
        return self.parts[0][1].galois(k)


def ring_of(logN, q, p):
    """one oracle ring where it holds the chain (its own key switch and rescale are then at hand), a SplitRing beyond"""
    return ol.Ring(logN, q, p) if len(q) + len(p) <= 16 else SplitRing(logN, q, p)


@functools.lru_cache(maxsize=None)
def chain_ring(name):
    """the reference ring of a chain of tests/ring_cases.py, made once"""
    import ring_cases
    return ring_of(*ring_cases.chain(name))


def uniform_key(ring, seed):
    """uniform key words [beta][2][nmod][N]: parity needs no valid key"""
    from sfgwas_amd import capi
    return capi.random_rotkey(ring.moduli, (ring.nq + ring.np_ - 1) // ring.np_, ring.N, seed)


def _obj(a):
    """-> an object array of Python integers"""
    a = np.asarray(a)
    return a.astype(object) if a.dtype.kind in "iu" else np.array([int(v) for v in a], dtype=object)


# ---------------------------------------------------------------- the basis extension on rows
@functools.lru_cache(maxsize=None)
def _digit_consts(qs):
    """(D, [(D / q_m)^-1 mod q_m], [D / q_m]) of the digit with moduli qs (a tuple)"""
    D = prod(qs)
    return D, [pow(D // q, -1, q) for q in qs], [D // q for q in qs]


def extend_rows(rows, qs, targets, mistake=None, classes=False):
    """coefficient-domain rows of one digit -> {qt: row} (uint64), as the oracle's basis_extend defines it.  classes=True: -> ({qt: row}, v_float - v_exact per word,
    an int64 array; None for a single-modulus digit, which is a raw copy with no correction).  mistake: one of MISTAKES, made in v."""
    if len(qs) == 1:
        x = _obj(rows[0])
        out = {qt: (x % qt).astype(np.uint64) for qt in targets}
        return (out, None) if classes else out
    D, inv, Dq = _digit_consts(tuple(qs))
    ys = [_obj(r) * i % q for r, i, q in zip(rows, inv, qs)]
    vf = np.zeros(len(ys[0]), dtype=np.float64)
    for y, q in zip(ys, qs):                                                         # in modulus order, one rounding per division and one per addition
        yf = y.astype(np.float64)                                                    # float(int): round to nearest even, as the C conversion
        vf = vf + (yf * (1.0 / float(q)) if mistake == "recip" else yf / float(q))
    v = _obj(np.floor(vf + 0.5) if mistake == "round" else np.floor(vf))             # vf >= 0: floor is the truncation; at most alpha <= 47
    if classes or mistake == "exact":
        ve = sum(y * d for y, d in zip(ys, Dq)) // D                                 # floor of the exact sum: sum y_m / q_m = sum y_m (D / q_m) / D
        cls = np.array([int(a) - int(b) for a, b in zip(v, ve)], dtype=np.int64)
        if mistake == "exact":
            v = ve
    out = {}
    for qt in targets:
        out[qt] = ((sum(y * (d % qt) for y, d in zip(ys, Dq)) - v * (D % qt)) % qt).astype(np.uint64)
    return (out, cls) if classes else out


def word_classes(values, qs, mistake=None):
    """v_float - v_exact of the signed integers `values` taken as words of the digit qs"""
    return extend_rows([[c % q for c in values] for q in qs], qs, [], mistake, classes=True)[1]


# ---------------------------------------------------------------- the key switch
def key_sums(ring, level, cx, key, mistake=None, trace=None):
    """the key switch up to its inner product: -> [2][level + 1 + np] object rows, the UNREDUCED sums over the digits of ext * key (what k_gr_keyip holds in 128
    bits before its one reduction).  A digit whose key words are all zero adds nothing and is skipped, unless its classes are asked for (trace, a list)."""
    nq, np_, mods, nl = ring.nq, ring.np_, ring.moduli, level + 1
    c2 = [ring.intt(m, cx[m]) for m in range(nl)]
    tmod = list(range(nl)) + [nq + p for p in range(np_)]
    acc = [[np.zeros(ring.N, dtype=object) for _ in tmod] for _ in range(2)]
    for i, dg in enumerate(ksw_ref.digits(level, np_)):
        if trace is None and not key[i].any():
            continue
        qs = [mods[m] for m in dg]
        ext, cls = extend_rows([c2[m] for m in dg], qs, [mods[m] for m in tmod if m not in dg], mistake, classes=True)
        if trace is not None:
            trace.append(cls)
        for t, mod in enumerate(tmod):
            e = _obj(cx[mod] if mod in dg else ring.ntt(mod, ext[mods[mod]]))
            for pl in range(2):
                acc[pl][t] = acc[pl][t] + e * _obj(key[i, pl, mod])
    return acc


def keyswitch(ring, level, cx, key, trace=False, mistake=None, where="all"):
    """cx [level+1][N] NTT rows, key [beta][2][nmod][N] -> (d0, d1) [level+1][N]; trace=True: -> (d0, d1, {"digits": [classes or None per digit],
    "moddown": [classes of plane 0, of plane 1]}) with the classes of extend_rows (None where np = 1).  mistake: made in every extension (where="all"), in the digits' alone
    ("digits") or in ModDown's alone ("moddown")"""
    assert where in ("all", "digits", "moddown")
    nq, np_, mods, nl = ring.nq, ring.np_, ring.moduli, level + 1
    tr = {"digits": [], "moddown": []}
    sums = key_sums(ring, level, cx, key, None if where == "moddown" else mistake, tr["digits"] if trace else None)
    acc = [[s % mods[t if t < nl else nq + t - nl] for t, s in enumerate(plane)] for plane in sums]
    ps = [mods[nq + p] for p in range(np_)]
    pinv = [pow(prod(ps) % mods[t], -1, mods[t]) for t in range(nl)]
    out = []
    for pl in range(2):
        rows = [ring.intt(nq + p, acc[pl][nl + p].astype(np.uint64)) for p in range(np_)]
        ext, cls = extend_rows(rows, ps, [mods[t] for t in range(nl)], None if where == "digits" else mistake, classes=True)
        tr["moddown"].append(cls)
        d = []
        for t in range(nl):
            qt = mods[t]
            e = _obj(ring.ntt(t, ext[qt]))
            d.append(((acc[pl][t] - e) * pinv[t] % qt).astype(np.uint64))
        out.append(np.stack(d))
    return (out[0], out[1], tr) if trace else (out[0], out[1])


def automorphism_index(logN, g):
    """lattigo ring.PermuteNTTIndex: out[i] = in[index[i]]"""
    N = 1 << logN

    def brev(x):
        return int(format(x, f"0{logN}b")[::-1], 2)
    return np.array([brev((((g * (2 * brev(i) + 1)) & (2 * N - 1)) - 1) >> 1) for i in range(N)], dtype=np.int64)


def galois_from_switch(ring, level, ct, d0, d1, g):
    """orc_apply_galois after its key switch: (c0 + d0, d1) read through the automorphism index of g"""
    idx = automorphism_index(ring.logN, g)
    out = np.zeros_like(ct)
    for m in range(level + 1):
        q = ring.moduli[m]
        out[0, m] = ((_obj(d0[m]) + _obj(ct[0, m])) % q).astype(np.uint64)[idx]
        out[1, m] = d1[m][idx]
    return out


def rotate_model(ring, level, ct, g, key):
    """orc_apply_galois around keyswitch(): ct [2][level+1][N]"""
    d0, d1 = keyswitch(ring, level, ct[1], key)
    return galois_from_switch(ring, level, ct, d0, d1, g)


def mulrelin_model(ring, level, a, b, rlk):
    """orc_mulrelin around keyswitch()"""
    out, c2 = np.zeros_like(a), np.zeros_like(a[0])
    for m in range(level + 1):
        q = ring.moduli[m]
        a0, a1, b0, b1 = _obj(a[0, m]), _obj(a[1, m]), _obj(b[0, m]), _obj(b[1, m])
        out[0, m], out[1, m], c2[m] = (a0 * b0 % q).astype(np.uint64), ((a0 * b1 + a1 * b0) % q).astype(np.uint64), (a1 * b1 % q).astype(np.uint64)
    d0, d1 = keyswitch(ring, level, c2, rlk)
    for m in range(level + 1):
        q = ring.moduli[m]
        out[0, m] = ((_obj(out[0, m]) + _obj(d0[m])) % q).astype(np.uint64)
        out[1, m] = ((_obj(out[1, m]) + _obj(d1[m])) % q).astype(np.uint64)
    return out


def rotation_and_product_model(ring, level, a, b0, g, key):
    """the rotation of a by the galois element g and the product of a with the partner (b0, all ones), both under `key`: all ones are the NTT of the constant 1,
    so a1 b1 = a1 and both operations switch the same polynomial - the key switch, the slow part, is computed once.  -> (rotated, product), [2][level+1][N]"""
    d0, d1 = keyswitch(ring, level, a[1], key)
    rot, mul = galois_from_switch(ring, level, a, d0, d1, g), np.zeros_like(a)
    for m in range(level + 1):
        q = ring.moduli[m]
        a0, a1, B0 = _obj(a[0, m]), _obj(a[1, m]), _obj(b0[m])
        mul[0, m] = ((a0 * B0 + _obj(d0[m])) % q).astype(np.uint64)
        mul[1, m] = ((a0 + a1 * B0 + _obj(d1[m])) % q).astype(np.uint64)
    return rot, mul


def rescale_model(ring, level, ct):
    """orc_rescale (lattigo ring.DivRoundByLastModulusNTT) in Python integers: ct [2][level+1][N] -> [2][level][N].  With t the last row in the coefficient
    domain and h = (q_L - 1) / 2: out_m = (ct_m - NTT_m(((t + h) mod q_L) - h mod q_m)) q_L^-1 mod q_m"""
    qL = ring.moduli[level]
    half = (qL - 1) >> 1
    out = np.zeros((2, level, ring.N), dtype=np.uint64)
    for p in range(2):
        t = (_obj(ring.intt(level, ct[p, level])) + half) % qL
        for m in range(level):
            q = ring.moduli[m]
            tmp = _obj(ring.ntt(m, ((t - half) % q).astype(np.uint64)))
            out[p, m] = ((_obj(ct[p, m]) - tmp) * pow(qL % q, -1, q) % q).astype(np.uint64)
    return out


# ---------------------------------------------------------------- directed inputs
def directed_values(q, alpha, level):
    """the cycle of signed integers that puts every digit's float sum on its integer boundaries: ksw_ref.SMALL (X = D - k rounds the sum up: class +1; X = k can
    round it down: class -1), every digit's D // 2 and D // 2 + 1 (the generic class 0), and, per multi-modulus digit and per sign, the smallest |k| < 200 in each
    class that none of the former reaches on that digit (searched as tests/test_ksw_ref.py searches; on most digits the search adds nothing), and the smallest
    |k| < 200 of each sign on which y * fl(1/q) in place of y / q gives another v, where none of the former is such a word (no 61-bit digit has one)"""
    digs = ksw_ref.digits(level, alpha)
    vals = list(ksw_ref.SMALL)
    for dg in digs:
        D = prod(q[m] for m in dg)
        vals += [D // 2, D // 2 + 1]
    base = list(vals)
    for dg in digs:
        if len(dg) == 1:
            continue
        qs = [q[m] for m in dg]
        reached = set(word_classes(base, qs).tolist())
        for sign in (1, -1):
            cand = [sign * k for k in range(1, 200)]
            found = {}
            for c, cls in zip(cand, word_classes(cand, qs).tolist()):
                if cls not in reached and cls not in found:
                    found[cls] = c
            vals += [c for c in found.values() if c not in vals]
        if (word_classes(base, qs) != word_classes(base, qs, "recip")).any():
            continue
        for sign in (1, -1):                                                         # no word yet on which y * fl(1/q) gives another v than y / q: the smallest one
            cand = [sign * k for k in range(1, 200)]
            moved = [c for c, a, b in zip(cand, word_classes(cand, qs), word_classes(cand, qs, "recip")) if a != b]
            vals += [c for c in moved[:1] if c not in vals]
    return vals


def uniform_ct(ring, level, seed):
    rnd = np.random.default_rng(seed)
    return np.stack([np.stack([rnd.integers(0, q, ring.N, dtype=np.uint64) for q in ring.moduli[:level + 1]]) for _ in range(2)])


def directed_ct(ring, level, seed):
    """a ciphertext [2][level+1][N]: polynomial 0 uniform, polynomial 1 the NTT of the cycle directed_values (shifted by seed), reduced modulo every q of the level"""
    ct = uniform_ct(ring, level, seed)
    rows = ksw_ref.directed_rows(ring.moduli[:level + 1], directed_values(ring.moduli[:ring.nq], ring.np_, level), ring.N, shift=seed)
    for m in range(level + 1):
        ct[1, m] = ring.ntt(m, rows[m])
    return ct


def boundary_last_row(ring, level, ct):
    """both polynomials' last rows <- the NTT of the cycle 0, 1, h - 1, h, h + 1, q_L - 2, q_L - 1 with h = (q_L - 1) / 2: the words at which the rescale's t + h
    wraps around q_L, and the ends of the range"""
    qL = ring.moduli[level]
    h = (qL - 1) >> 1
    for p in range(2):
        ct[p, level] = ring.ntt(level, ksw_ref.directed_rows([qL], [0, 1, h - 1, h, h + 1, qL - 2, qL - 1], ring.N, shift=p)[0])
    return ct


def identity_key(ring):
    """digit 0, plane 0: the constant 1 (all-ones rows); digit 0, plane 1: the constant -1 (rows of q - 1); every other digit zero.  The accumulators' P rows are
    then +-X0 extended to P in the coefficient domain, X0 the first digit's word: X0 = k and X0 = D0 - k (which the float correction takes to -k) give P-row words
    k and P - k, so ModDown's own float sum sits on both boundaries - without a valid key"""
    nmod = len(ring.moduli)
    beta = (ring.nq + ring.np_ - 1) // ring.np_
    key = np.zeros((beta, 2, nmod, ring.N), dtype=np.uint64)
    key[0, 0] = 1
    for m, q in enumerate(ring.moduli):
        key[0, 1, m] = q - 1
    return key


def planted_maximum(ring, level):
    """(cx, key): every input row and every key row all q - 1, which drives the key switch's unreduced inner sums as high as they go"""
    mods = ring.moduli
    cx = np.stack([np.full(ring.N, q - 1, dtype=np.uint64) for q in mods[:level + 1]])
    key = np.zeros(((ring.nq + ring.np_ - 1) // ring.np_, 2, len(mods), ring.N), dtype=np.uint64)
    for m, q in enumerate(mods):
        key[:, :, m] = q - 1
    return cx, key


def crt_centered(rows, moduli):
    """[len(moduli)][N] residues -> list of N signed Python integers in (-Q/2, Q/2]"""
    Q = prod(moduli)
    x = np.zeros(rows.shape[1], dtype=object)
    for r, q in zip(rows, moduli):
        x = x + _obj(r) * ((Q // q) * pow(Q // q, -1, q))
    x = x % Q
    return [int(v) - Q if int(v) > Q // 2 else int(v) for v in x]


def decode(coeffs, N, scale):
    """slot t of the plaintext with integer coefficients p: sum_c w_c zeta^(5^t c), w_c = (p_c + i p_{c+n}) / scale, zeta = exp(2 pi i / 2N)"""
    n = N // 2
    w = (np.array([float(c) for c in coeffs[:n]]) + 1j * np.array([float(c) for c in coeffs[n:]])) / float(scale)
    a = w * np.exp(1j * np.pi * np.arange(n) / N)                  # w_c zeta^c; 5^t = 4 m_t + 1 turns the sum into a length-n transform at m_t
    V = np.fft.ifft(a) * n
    m_t, g = np.empty(n, dtype=np.int64), 1
    for t in range(n):
        m_t[t] = ((g - 1) // 4) % n
        g = g * 5 % (2 * N)
    return V[m_t]
