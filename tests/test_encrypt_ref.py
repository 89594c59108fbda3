"""The Python restatement the GPU encryption tests compare against (tests/encrypt_ref.py) is itself pinned: ChaCha20 against RFC 8439, the Gaussian table
against its derivation, and the big-integer encryption by decrypting it on a tiny ring."""
import math
import os
import random
import re

import numpy as np

import encrypt_ref as er
from pyref import crt_centered

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_chacha20_quarter_round_rfc8439_2_1_1():
    a, b, c, d = (np.array([v], dtype=np.uint32) for v in (0x11111111, 0x01020304, 0x9b8d6f43, 0x01234567))
    old = np.seterr(over="ignore")
    try:
        out = er.quarter_round(a, b, c, d)
    finally:
        np.seterr(**old)
    assert [int(x[0]) for x in out] == [0xea2a92f4, 0xcb1cf8ce, 0x4581472e, 0x5881c4bb]


def test_chacha20_block_rfc8439_2_3_2():
    key = bytes(range(32))
    nonce = bytes.fromhex("000000090000004a00000000")
    words = [int.from_bytes(nonce[4 * i:4 * i + 4], "little") for i in range(3)]
    blk = er.chacha20_blocks(key, [1], words)[0]
    want = [0xe4e7f110, 0x15593bd1, 0x1fdd0f50, 0xc47120a3, 0xc7f4d1c7, 0x0368c033, 0x9aaa2204, 0x4e6cd4c3,
            0x466482d2, 0x09aa9f07, 0x05d7c214, 0xa2028bd9, 0xd19c12b5, 0xb94e16de, 0xe883d0cb, 0x4e3c50a2]
    assert [int(x) for x in blk] == want
    ser = b"".join(int(x).to_bytes(4, "little") for x in blk)
    assert ser[:16].hex() == "10f1e7e4d13b5915500fdd1fa32071c4" and ser[-4:].hex() == "a2503c4e"
    # vectorised over counters = block by block
    two = er.chacha20_blocks(key, [0, 1], words)
    assert (two[1] == blk).all() and (two[0] != blk).any()


def test_gaussian_table_is_its_derivation_and_what_the_library_documents():
    cum, p, cut = er.gauss_table_mpmath()
    assert cum == er.GAUSS_CUM                                   # entry by entry
    probs = er.magnitude_probabilities()
    assert len(probs) == 20 and all(0 < x < 1 << 63 for x in probs) and sum(probs) == 1 << 63
    assert abs(p[0] - 0.124164) < 1e-6 and abs(probs[0] / 2.0 ** 63 - p[0]) < 1e-18
    var = sum(k * k * probs[k] for k in range(20)) / 2.0 ** 63
    assert abs(var - 10.32333) < 1e-5 and abs(cut - 1.1e-9) < 1e-10
    # the same twenty words in the kernel source and in DESIGN.md
    for rel in (os.path.join("sfgwas_amd", "csrc", "encrypt.hip"), "DESIGN.md"):
        txt = open(os.path.join(ROOT, rel)).read().lower()
        found = [int(h, 16) for h in re.findall(r"0x([0-9a-f]{16})", txt)]
        assert all(c in found for c in er.GAUSS_CUM), rel


def test_sampler_map_support_and_moments_on_the_cpu():
    """the statistics test_gpu_encrypt.py asks of the device, asked of this file first (same key, same indices): deterministic"""
    key = er.TEST_KEY
    u, e0, e1 = er.transcript(key, 0, 32)
    e = np.concatenate([e0.ravel(), e1.ravel()]).astype(np.int64); u = u.ravel().astype(np.int64)
    assert set(np.unique(u)) == {-1, 0, 1} and e.min() >= -19 and e.max() <= 19
    n = u.size
    for val, pr in ((-1, 0.25), (0, 0.5), (1, 0.25)):
        assert abs((u == val).mean() - pr) <= 5 * math.sqrt(pr * (1 - pr) / n)
    probs = [x / 2.0 ** 63 for x in er.magnitude_probabilities()]
    m2 = sum(k * k * probs[k] for k in range(20)); m4 = sum(k ** 4 * probs[k] for k in range(20))
    assert abs(e.mean()) <= 5 * math.sqrt(m2 / e.size)
    assert abs((e * e).mean() - m2) <= 5 * math.sqrt((m4 - m2 * m2) / e.size)
    # distinct (index, polynomial) pairs give distinct streams; the index is 64 bits wide
    assert (er.sample_e(key, 5, 1) != er.sample_e(key, 5, 2)).any() and (er.sample_u(key, 1) != er.sample_u(key, 1 + (1 << 32))).any()


def _primes(N2, bits, count):
    out, x = [], (1 << bits) + 1
    while len(out) < count:
        if all(x % d for d in range(3, int(x ** 0.5) + 1, 2)):
            out.append(x)
        x += N2
    return out


def _tiny_setup(seed):
    rnd = random.Random(seed)
    logN, N = 4, 16
    q, p = _primes(2 * N, 20, 3), _primes(2 * N, 12, 2)
    ring = er.TinyRing(logN, q, p)
    s = [rnd.choice((-1, 0, 1)) for _ in range(N)]
    e_pk = [rnd.randint(-19, 19) for _ in range(N)]
    pk = [[None] * 5, [None] * 5]
    for m, mod in enumerate(ring.moduli):
        a = np.array([rnd.randrange(mod) for _ in range(N)], dtype=object)
        sh, eh = ring.ntt(m, [x % mod for x in s]), ring.ntt(m, [x % mod for x in e_pk])
        pk[0][m] = (-(a * sh) + eh) % mod
        pk[1][m] = a
    return rnd, ring, q, p, s, e_pk, pk


def _decrypt(ring, q, s, ct):
    res = []
    for m in range(len(q)):
        sh = ring.ntt(m, [x % q[m] for x in s])
        res.append(ring.intt(m, (ct[m][0] + ct[m][1] * sh) % q[m]))
    return crt_centered(res, q)


def test_bigint_encryption_decrypts_to_message_plus_noise_over_P():
    """c0 + c1 s = m + (u e_pk + e0 + e1 s) / P up to the ModDown rounding 2 (N + 1): the division by P is the point of this form, so the errors are chosen
    LARGE (2^28) - a noise of about 2^32 that an encryption without the ModDown would carry whole - and what is left must be that noise over P = 2^24"""
    rnd, ring, q, p, s, e_pk, pk = _tiny_setup(7)
    N, P = ring.N, p[0] * p[1]
    for trial in range(4):
        big = 1 << 28
        u = [rnd.choice((-1, 0, 1)) for _ in range(N)]
        e0 = [rnd.randint(-big, big) for _ in range(N)]; e1 = [rnd.randint(-big, big) for _ in range(N)]
        msg = [rnd.randint(-(1 << 40), 1 << 40) for _ in range(N)]
        pt = [ring.ntt(m, [x % q[m] for x in msg]) for m in range(3)]
        ct = er.encrypt_bigint(ring, 2, pk, u, e0, e1, pt if trial % 2 == 0 else None)
        dec = _decrypt(ring, q, s, ct)
        w = [a + b + c for a, b, c in zip(er.negacyclic(u, e_pk), e0, er.negacyclic(e1, s))]
        want = msg if trial % 2 == 0 else [0] * N
        resid = [dec[j] - want[j] for j in range(N)]
        assert max(abs(x) for x in w) > (1 << 28) > 1000 * 2 * (N + 1)     # the undivided noise is huge ...
        assert max(abs(resid[j] - w[j] / P) for j in range(N)) <= 2 * (N + 1)                                  # ... and what remains is w / P, to the rounding
        assert max(abs(x) for x in resid) < max(abs(x) for x in w) / (P / 4)                                   # shrunk by (about) P
        assert max(abs(w[j] / P) for j in range(N)) > 4                                                        # (and w / P itself is visible: the quotient is checked, not only the bound)


def test_bigint_encryption_level_rows_do_not_depend_on_the_level():
    rnd, ring, q, p, s, e_pk, pk = _tiny_setup(11)
    N = ring.N
    u = [rnd.choice((-1, 0, 1)) for _ in range(N)]; e0 = [rnd.randint(-19, 19) for _ in range(N)]; e1 = [rnd.randint(-19, 19) for _ in range(N)]
    full, low = er.encrypt_bigint(ring, 2, pk, u, e0, e1), er.encrypt_bigint(ring, 0, pk, u, e0, e1)
    assert list(low) == [0] and all((low[0][i] == full[0][i]).all() for i in range(2))
