"""Independent Python statement of the device encryption (sfgwas_amd/csrc/encrypt.hip, DESIGN.md "Encryption on the device"): ChaCha20 (RFC 8439), the map from
stream bytes to ternary / Gaussian samples, the Gaussian table's derivation, and the big-integer public-key encryption with the key switch's ModDown.
tests/test_encrypt_ref.py pins this file; tests/test_gpu_encrypt.py compares the library against it."""
import numpy as np

N14 = 1 << 14
SIGMA, BOUND = 3.2, 19

TEST_KEY = bytes(range(100, 132))              # the sampler key of the tests: tests/test_encrypt_ref.py checks the Python sampler's statistics under it first

# the table the library documents (encrypt.hip ENC_GAUSS_CUM): cumulative distribution of the magnitude in units of 2^-63
GAUSS_CUM = [
    0x0fe49b6827cb0a22, 0x2e2d1c3d2d673909, 0x485d35a4168455fb, 0x5ceb732fcf500f03, 0x6b909790cec541bc,
    0x750918a85086780a, 0x7a98381b8b05d44b, 0x7d8e6d674ccde58a, 0x7efd1569779956ed, 0x7f9e04eac7bbada7,
    0x7fde228ae318bb83, 0x7ff551b87c6c82e1, 0x7ffcedaa42aca3e8, 0x7fff31ef2eb41935, 0x7fffced272bc4241,
    0x7ffff5523bb74b16, 0x7ffffde5526b5ceb, 0x7fffffa10a4c8db3, 0x7ffffff2720cd7c6, 0x8000000000000000]


def gauss_table_mpmath():
    """C[k] = round(2^63 (p_0 + 2 p_1 + ... + 2 p_k)), p_k = (Phi((k + 1/2) / sigma) - Phi((k - 1/2) / sigma)) / Z over |k| <= 19; also (p list, mass removed by the cut)"""
    import mpmath as mp
    with mp.workprec(400):
        s = mp.mpf("3.2")
        w = [mp.ncdf((k + mp.mpf(1) / 2) / s) - mp.ncdf((k - mp.mpf(1) / 2) / s) for k in range(BOUND + 1)]
        Z = w[0] + 2 * sum(w[1:])
        p = [x / Z for x in w]
        cum, acc = [], mp.mpf(0)
        for k in range(BOUND + 1):
            acc += p[k] if k == 0 else 2 * p[k]
            cum.append(int(mp.nint(acc * mp.mpf(2) ** 63)))
        return cum, [float(x) for x in p], float(1 - Z)


def magnitude_probabilities():
    """exact P(|e| = k) as integers over 2^63"""
    return [GAUSS_CUM[0]] + [GAUSS_CUM[k] - GAUSS_CUM[k - 1] for k in range(1, BOUND + 1)]


# ---------------------------------------------------------------- ChaCha20, vectorised over blocks (uint32 arithmetic wraps)
def _rotl(x, n):
    return (x << np.uint32(n)) | (x >> np.uint32(32 - n))


def quarter_round(a, b, c, d):
    a = a + b; d = _rotl(d ^ a, 16)
    c = c + d; b = _rotl(b ^ c, 12)
    a = a + b; d = _rotl(d ^ a, 8)
    c = c + d; b = _rotl(b ^ c, 7)
    return a, b, c, d


def chacha20_blocks(key32, counters, nonce_words):
    """key32: 32 bytes; counters: array of 32-bit block counters; nonce_words: three 32-bit words (state words 13, 14, 15) -> uint32 [len(counters)][16]"""
    key = np.frombuffer(bytes(key32), dtype="<u4")
    counters = np.asarray(counters, dtype=np.uint32)
    n = counters.shape[0]
    init = [np.full(n, v, dtype=np.uint32) for v in (0x61707865, 0x3320646e, 0x79622d32, 0x6b206574)]
    init += [np.full(n, int(k), dtype=np.uint32) for k in key]
    init += [counters.copy()] + [np.full(n, int(w) & 0xFFFFFFFF, dtype=np.uint32) for w in nonce_words]
    x = [v.copy() for v in init]
    old = np.seterr(over="ignore")
    try:
        for _ in range(10):
            for (i, j, k, l) in ((0, 4, 8, 12), (1, 5, 9, 13), (2, 6, 10, 14), (3, 7, 11, 15), (0, 5, 10, 15), (1, 6, 11, 12), (2, 7, 8, 13), (3, 4, 9, 14)):
                x[i], x[j], x[k], x[l] = quarter_round(x[i], x[j], x[k], x[l])
        out = np.stack([x[i] + init[i] for i in range(16)], axis=1)
    finally:
        np.seterr(**old)
    return out


def nonce_of(index, poly):
    """nonce = the 64-bit encryption index (little endian: low word first), then the polynomial id"""
    return (index & 0xFFFFFFFF, (index >> 32) & 0xFFFFFFFF, poly)


# ---------------------------------------------------------------- stream bytes -> samples (N = 16384; coefficient j = a * 512 + t, a < 32, t < 512)
def sample_u(key32, index):
    W = chacha20_blocks(key32, np.arange(64), nonce_of(index, 0)).astype(np.uint64)
    j = np.arange(N14); a, t = j >> 9, j & 511
    r = W[t >> 3, 2 * (t & 7)] | (W[t >> 3, 2 * (t & 7) + 1] << np.uint64(32))
    two = (r >> (2 * a).astype(np.uint64)) & np.uint64(3)
    return np.where(two & np.uint64(1), np.where(two & np.uint64(2), -1, 1), 0).astype(np.int8)


def sample_e(key32, index, poly):
    W = chacha20_blocks(key32, np.arange(2048), nonce_of(index, poly)).astype(np.uint64)
    j = np.arange(N14); a, t = j >> 9, j & 511
    blk, k = t + 512 * (a >> 3), a & 7
    r = W[blk, 2 * k] | (W[blk, 2 * k + 1] << np.uint64(32))
    mag = np.searchsorted(np.array(GAUSS_CUM, dtype=np.uint64), r >> np.uint64(1), side="right").astype(np.int32)      # number of thresholds <= the 63 bits
    return np.where(r & np.uint64(1), -mag, mag).astype(np.int32)


def transcript(key32, first_index, nct):
    idx = [first_index + i for i in range(nct)]
    return (np.stack([sample_u(key32, i) for i in idx]), np.stack([sample_e(key32, i, 1) for i in idx]), np.stack([sample_e(key32, i, 2) for i in idx]))


# ---------------------------------------------------------------- the encryption, big integers
class TinyRing:
    """negacyclic ring of degree 2^logN over invented primes with the interface of oracle_lib.Ring that encrypt_bigint uses: ntt / intt by direct evaluation at
    the odd powers of a primitive 2N-th root (any fixed order: the encryption is element-wise in that domain)"""

    def __init__(self, logN, q, p):
        self.N, self.nq, self.np_, self.moduli = 1 << logN, len(q), len(p), list(q) + list(p)
        self.psi = []
        for m in self.moduli:
            assert (m - 1) % (2 * self.N) == 0
            g = next(g for g in range(2, m) if pow(pow(g, (m - 1) // (2 * self.N), m), self.N, m) == m - 1)
            self.psi.append(pow(g, (m - 1) // (2 * self.N), m))

    def ntt(self, mod, a):
        m, w = self.moduli[mod], self.psi[mod]
        return np.array([sum(int(a[j]) * pow(w, (2 * i + 1) * j, m) for j in range(self.N)) % m for i in range(self.N)], dtype=object)

    def intt(self, mod, a):
        m, wi, ninv = self.moduli[mod], pow(self.psi[mod], -1, self.moduli[mod]), pow(self.N, -1, self.moduli[mod])
        return np.array([sum(int(a[i]) * pow(wi, (2 * i + 1) * j, m) for i in range(self.N)) * ninv % m for j in range(self.N)], dtype=object)


def _obj(a):
    return np.array([int(x) for x in a], dtype=object)


def moddown_rows(ring, level, tq_rows, tp_rows, rows=None):
    """(t_Q - NTT(ext_{P->Q}(INTT(t_P)))) * P^-1 for Q rows `rows` (default all of 0..level): the key switch's ModDown with lattigo's float-corrected basis
    extension: y_p = x_p (P/p)^-1 mod p, v = uint64(sum float64(y_p) / float64(p)) accumulated in modulus order, ext = sum y_p (P/p) - v P."""
    nq, np_ = ring.nq, ring.np_
    ps = ring.moduli[nq:nq + np_]
    P = 1
    for p in ps:
        P *= p
    x = [_obj(ring.intt(nq + i, tp_rows[i])) for i in range(np_)]
    out = {}
    if np_ == 1:
        y, v = None, None
    else:
        y = [x[i] * pow(P // ps[i], -1, ps[i]) % ps[i] for i in range(np_)]
        vf = np.zeros(ring.N, dtype=np.float64)
        for i in range(np_):
            vf = vf + np.array([float(int(t)) for t in y[i]], dtype=np.float64) / np.float64(float(ps[i]))
        v = _obj(vf.astype(np.uint64))
    for t in (range(level + 1) if rows is None else rows):
        q = ring.moduli[t]
        ext = x[0] % q if np_ == 1 else (sum(y[i] * ((P // ps[i]) % q) for i in range(np_)) - v * (P % q)) % q
        exth = _obj(ring.ntt(t, np.array(ext, dtype=np.uint64) if ring.N > 64 else ext))
        out[t] = (_obj(tq_rows[t]) - exth) * pow(P % q, -1, q) % q
    return out


def encrypt_bigint(ring, level, pk, u, e0, e1, pt=None, rows=None):
    """pk [2][nq+np][N] NTT-domain words; u, e0, e1 signed integer polynomials; pt None or [level+1][N] NTT-domain rows -> {row: (c0 row, c1 row)} as object arrays"""
    nq, np_ = ring.nq, ring.np_
    big = ring.N > 64                                 # oracle_lib.Ring takes uint64 arrays
    targets = list(range(level + 1) if rows is None else rows) + [nq + i for i in range(np_)]
    t = [{}, {}]
    for m in targets:
        q = ring.moduli[m]
        red = lambda a: np.array([int(z) % q for z in a], dtype=np.uint64 if big else object)
        uh = _obj(ring.ntt(m, red(u)))
        for i, e in enumerate((e0, e1)):
            t[i][m] = (_obj(pk[i][m]) * uh + _obj(ring.ntt(m, red(e)))) % q
    out = {}
    c = [moddown_rows(ring, level, t[i], [t[i][nq + k] for k in range(np_)], rows) for i in range(2)]
    for r in c[0]:
        c0 = c[0][r] if pt is None else (c[0][r] + _obj(pt[r])) % ring.moduli[r]
        out[r] = (c0, c[1][r])
    return out


def negacyclic(a, b):
    """exact integer product in Z[X] / (X^N + 1)"""
    n = len(a); out = [0] * n
    for i in range(n):
        if a[i]:
            for j in range(n):
                k = i + j
                if k < n:
                    out[k] += int(a[i]) * int(b[j])
                else:
                    out[k - n] -= int(a[i]) * int(b[j])
    return out


def make_keypair(ring, seed):
    """pk = (-a s + e, a) over all of Q and P, NTT domain; s ternary (the oracle's), |e| <= 19"""
    rnd = np.random.default_rng(seed)
    s = ring.gen_secret(seed)
    e = rnd.integers(-19, 20, ring.N)
    N = ring.N
    pk = np.zeros((2, len(ring.moduli), N), dtype=np.uint64)
    for m, q in enumerate(ring.moduli):
        a = rnd.integers(0, q, N, dtype=np.uint64)
        sh = ring.ntt(m, np.array([int(x) % q for x in s], dtype=np.uint64))
        eh = ring.ntt(m, np.array([int(x) % q for x in e], dtype=np.uint64))
        pk[0, m] = np.array([(-(int(x) * int(y)) + int(z)) % q for x, y, z in zip(a, sh, eh)], dtype=np.uint64)
        pk[1, m] = a
    return s, pk
