"""Public-key encryption on the device (sfgwas_amd/csrc/encrypt.hip): the deterministic core against the Python big-integer statement (tests/encrypt_ref.py,
itself pinned by tests/test_encrypt_ref.py), the keyed sampler against the independent Python ChaCha20 + table inversion, the fused calls against
transcript + core, decryption within the derived worst-case noise, and the refusals.  PN14 moduli; the oracle's Ring supplies NTTs, secrets and decryption.

PARITY UNPINNED against lattigo's pkEncryptor.EncryptNew (no Go toolchain; fresh randomness excludes bit parity anyway): what is pinned is the arithmetic."""
import math
import os

import numpy as np
import pytest

import encrypt_ref as er
import oracle_lib as ol
from pyref import crt_centered

pytestmark = pytest.mark.gpu
N, NQ, NP = 1 << 14, len(ol.Q_PN14), len(ol.P_PN14)
KEY = er.TEST_KEY
P_PROD = ol.P_PN14[0] * ol.P_PN14[1]
NOISE_BOUND = -(-19 * (2 * N + 1) // P_PROD) + 2 * (N + 1)       # ceil(19 (2N + 1) / P) + ModDown rounding 2 (N + 1): derived in the issue, not measured


@pytest.fixture(scope="module")
def env():
    from sfgwas_amd import capi
    ring = ol.Ring(14, ol.Q_PN14, ol.P_PN14)
    ctx = capi.Context(ol.Q_PN14, ol.P_PN14)
    s, pk = er.make_keypair(ring, 31)
    ctx.load_public_key(pk)
    ctx.seed_encryptor(KEY)
    yield ctx, ring, s, pk
    ctx.close()


def samples_for_core(seed):
    """three ciphertexts: random u, e; all u = +1 with every e = +19; all u = -1 with e = -19 / alternating +-19"""
    rnd = np.random.default_rng(seed)
    u = np.stack([rnd.integers(-1, 2, N), np.ones(N, dtype=np.int64), -np.ones(N, dtype=np.int64)]).astype(np.int8)
    alt = np.where(np.arange(N) % 2 == 0, 19, -19)
    e0 = np.stack([rnd.integers(-19, 20, N), np.full(N, 19), np.full(N, -19)]).astype(np.int32)
    e1 = np.stack([rnd.integers(-19, 20, N), np.full(N, 19), alt]).astype(np.int32)
    return u, e0, e1


def test_core_every_word_against_big_integers_and_level_consistency(env):
    """levels 0, 4 and 9, nct = 3 (random / all-plus / all-minus extremes), without and with a plaintext: EVERY output word of every level (level 9 included -
    nothing is sampled) equals the Python statement; and level 4 is rows 0..4 of level 9 for the same randomness"""
    ctx, ring, s, pk = env
    u, e0, e1 = samples_for_core(5)
    rnd = np.random.default_rng(9)
    ref9 = [er.encrypt_bigint(ring, 9, pk, u[i], e0[i], e1[i]) for i in range(3)]          # rows of lower levels are rows of this one - which the device must show, not assume
    got = {}
    for level in (0, 4, 9):
        nl = level + 1
        pt = np.stack([np.stack([rnd.integers(0, ring.moduli[m], N, dtype=np.uint64) for m in range(nl)]) for _ in range(3)])
        got[level] = ctx.encrypt_explicit(None, level, u, e0, e1)
        with_pt = ctx.encrypt_explicit(pt, level, u, e0, e1)
        assert got[level].shape == (3, 2, nl, N)
        ref = ref9 if level == 9 else [er.encrypt_bigint(ring, level, pk, u[i], e0[i], e1[i]) for i in range(3)]
        for i in range(3):
            for m in range(nl):
                q = ring.moduli[m]
                c0, c1 = (np.array(x, dtype=np.uint64) for x in ref[i][m])
                assert np.array_equal(got[level][i, 0, m], c0) and np.array_equal(got[level][i, 1, m], c1), (level, i, m)
                assert np.array_equal(with_pt[i, 0, m], (c0 + pt[i, m]) % np.uint64(q)) and np.array_equal(with_pt[i, 1, m], c1), (level, i, m, "pt")
                assert got[level][i, :, m].max() < q
    assert np.array_equal(got[4], got[9][:, :, :5]) and np.array_equal(got[0], got[9][:, :, :1])


def test_transcript_is_the_python_sampler_and_has_the_tables_statistics(env):
    ctx, ring, s, pk = env
    before = ctx.encryptor_next_index()
    for idx in (0, 1, (1 << 32) - 1, 1 << 32, 1 << 63):               # the index is 64 bits wide everywhere
        u, e0, e1 = ctx.encrypt_transcript(idx, 1)
        wu, w0, w1 = er.transcript(KEY, idx, 1)
        assert np.array_equal(u, wu) and np.array_equal(e0, w0) and np.array_equal(e1, w1), idx
    u, e0, e1 = ctx.encrypt_transcript(0, 64)                          # 2^20 coefficients of each polynomial
    assert ctx.encryptor_next_index() == before                        # the hook does not advance the counter
    wu, w0, w1 = er.transcript(KEY, 0, 64)
    assert np.array_equal(u, wu) and np.array_equal(e0, w0) and np.array_equal(e1, w1)
    u = u.ravel().astype(np.int64); n = u.size
    assert n >= 1 << 20 and set(np.unique(u)) == {-1, 0, 1}
    for val, pr in ((-1, 0.25), (0, 0.5), (1, 0.25)):
        assert abs((u == val).mean() - pr) <= 5 * math.sqrt(pr * (1 - pr) / n), val
    probs = [x / 2.0 ** 63 for x in er.magnitude_probabilities()]
    m2 = sum(k * k * probs[k] for k in range(20)); m4 = sum(k ** 4 * probs[k] for k in range(20))
    for e in (e0, e1):
        e = e.ravel().astype(np.int64)
        assert e.size >= 1 << 20 and e.min() >= -19 and e.max() <= 19 and set(np.unique(e)) <= set(range(-19, 20))
        assert abs(e.mean()) <= 5 * math.sqrt(m2 / e.size)
        assert abs((e * e).mean() - m2) <= 5 * math.sqrt((m4 - m2 * m2) / e.size)


def test_fused_calls_are_transcript_plus_core(env):
    from sfgwas_amd import capi
    ctx, ring, s, pk = env
    ctx.seed_encryptor(KEY)
    assert ctx.encryptor_next_index() == 0
    level, nct = 4, 3
    qs = np.array(ring.moduli[:level + 1], dtype=np.uint64).reshape(1, 1, level + 1, 1)

    def fresh_zero_call(c):
        d = c.fill_uniform_cts(nct, level, 0xE11C)
        base = d.host()
        c.add_fresh_zero(d, level)
        out = d.host(); d.free()
        return base, out

    base, out1 = fresh_zero_call(ctx)
    assert ctx.encryptor_next_index() == nct                           # exactly nct indices
    u, e0, e1 = ctx.encrypt_transcript(0, nct)
    want = (base + ctx.encrypt_explicit(None, level, u, e0, e1)) % qs
    assert np.array_equal(out1, want)                                  # all words
    _, out2 = fresh_zero_call(ctx)                                     # a second call: other indices, other words
    assert ctx.encryptor_next_index() == 2 * nct and (out2 != out1).mean() > 0.99
    u, e0, e1 = ctx.encrypt_transcript(nct, nct)
    assert np.array_equal(out2, (base + ctx.encrypt_explicit(None, level, u, e0, e1)) % qs)
    # a fork draws from the same counter: its indices are disjoint from the root's
    fork = ctx.fork()
    try:
        assert fork.has_public_key()
        _, outf = fresh_zero_call(fork)
        assert ctx.encryptor_next_index() == 3 * nct == fork.encryptor_next_index()
        u, e0, e1 = ctx.encrypt_transcript(2 * nct, nct)
        assert np.array_equal(outf, (base + ctx.encrypt_explicit(None, level, u, e0, e1)) % qs)
    finally:
        fork.close()
    # EncryptFloatVector = the encoder's rows + the encryption
    rnd = np.random.default_rng(3)
    vals = rnd.uniform(-50, 50, (2, ring.slots))
    d = ctx.encrypt_vectors(vals, 9)
    got = d.host(); d.free()
    assert ctx.encryptor_next_index() == 3 * nct + 2
    u, e0, e1 = ctx.encrypt_transcript(3 * nct, 2)
    assert np.array_equal(got, ctx.encrypt_explicit(ctx.encode_vectors(vals, 9), 9, u, e0, e1))
    # re-seeding with the same key reproduces the first call
    ctx.seed_encryptor(KEY)
    assert ctx.encryptor_next_index() == 0
    _, again = fresh_zero_call(ctx)
    assert np.array_equal(again, out1)


def centred_diff(ring, level, a, b):
    mods = ring.moduli[:level + 1]
    return crt_centered([[(int(x) - int(y)) % q for x, y in zip(a[m], b[m])] for m, q in enumerate(mods)], mods)


def test_it_is_an_encryption_within_the_worst_case_noise(env):
    """decrypt(encrypt_vectors(v)) - encoder coefficients of v, and decrypt(product + Enc(0)) - decrypt(product), are at most
    ceil(19 (2N + 1) / P) + 2 (N + 1) in every coefficient (|u|, |s| <= 1, |e| <= 19; each of c0, c1 off by < 2 from the ModDown, c1 meeting |s|_1 <= N)"""
    from sfgwas_amd import capi
    import ctypes as C
    from sfgwas_amd.params import rotations_for_matmul
    ctx, ring, s, pk = env
    assert NOISE_BOUND == 1 + 2 * (N + 1)
    level = 1
    rnd = np.random.default_rng(17)
    vals = rnd.uniform(-100, 100, (2, ring.slots))
    d = ctx.encrypt_vectors(vals, level)
    cts = d.host(); d.free()
    mods = ring.moduli[:level + 1]
    for i in range(2):
        res = ring.decrypt_residues(s, level, cts[i])
        dec = crt_centered([[int(x) for x in res[m]] for m in range(level + 1)], mods)
        coeffs = ring.encode_coeffs(vals[i], 2.0 ** 34)
        pt_rows = ctx.encode_vectors(vals[i:i + 1], level)[0]            # the device encoder's own coefficients, read back from its rows
        for m in range(level + 1):
            assert np.array_equal(ring.intt(m, pt_rows[m]), np.array([int(c) % mods[m] for c in coeffs], dtype=np.uint64))
        worst = max(abs(a - int(b)) for a, b in zip(dec, coeffs))
        print(f"encrypt_vectors noise: max |dec - coeff| = {worst}, bound {NOISE_BOUND}")
        assert worst <= NOISE_BOUND
    # a product (60 x 40 genotypes, uniform input ciphertexts, synthetic rotation keys: decryption is linear, validity of the keys is not needed) finished on the device
    rots = rotations_for_matmul()
    ctx.check(capi.lib().sfg_fill_rotkeys_synthetic(ctx.h, (C.c_int * len(rots))(*rots), len(rots), 77), "rotkeys")
    gd, g = ctx.fill_geno(60, 40, 12)
    A = ctx.fill_uniform_cts(1, 5, 0xA11)
    out = ctx.matmul_resident(A, 1, 5, 5, g)
    unfinished = out.host()
    ctx.add_fresh_zero(out, 4)
    finished = out.host()
    for a in (out, A, gd):
        a.free()
    ctx.geno_free(g)
    assert unfinished.shape == (1, 1, 2, 5, N) and (finished != unfinished).mean() > 0.99
    r0, r1 = ring.decrypt_residues(s, 4, unfinished[0, 0]), ring.decrypt_residues(s, 4, finished[0, 0])
    worst = max(abs(x) for x in centred_diff(ring, 4, r1, r0))
    print(f"finished product: max |dec(finished) - dec(unfinished)| = {worst}, bound {NOISE_BOUND}")
    assert worst <= NOISE_BOUND


def test_refusals_are_clean_errors(env):
    from sfgwas_amd import capi
    ctx, ring, s, pk = env
    L = capi.lib()
    d = ctx.fill_uniform_cts(1, 4, 1)
    keep = d.host()
    bare = capi.Context(ol.Q_PN14, ol.P_PN14)
    try:
        assert not bare.has_public_key()
        db = bare.fill_uniform_cts(1, 4, 1)
        with pytest.raises(capi.SfgError, match="no public key"):
            bare.add_fresh_zero(db, 4)
        with pytest.raises(capi.SfgError, match="no public key"):
            bare.encrypt_vectors(np.zeros((1, ring.slots)), 4)
        with pytest.raises(capi.SfgError, match="no public key"):
            bare.encrypt_explicit(None, 4, np.zeros((1, N), np.int8), np.zeros((1, N), np.int32), np.zeros((1, N), np.int32))
        bare.load_public_key(pk)
        with pytest.raises(capi.SfgError, match="no key"):              # no seed, no default
            bare.add_fresh_zero(db, 4)
        with pytest.raises(capi.SfgError, match="no key"):
            bare.encrypt_vectors(np.zeros((1, ring.slots)), 4)
        with pytest.raises(capi.SfgError, match="no key"):
            bare.encrypt_transcript(0, 1)
        assert np.array_equal(db.host(), keep)                          # nothing was launched on the ciphertext
        bare.seed_encryptor(KEY)
        msg = L.sfg_last_error(bare.h).decode()
        assert KEY.hex() not in msg
        db.free()
    finally:
        bare.close()
    with pytest.raises(capi.SfgError, match="level"):
        ctx.add_fresh_zero(capi.DevArray(ctx, (1, 2, NQ + 1, N)), NQ)   # level > nq - 1
    assert L.sfg_ct_add_fresh_zero_dev(ctx.h, d.p, 0, 4) != 0 and b"count" in L.sfg_last_error(ctx.h)      # nct = 0
    assert L.sfg_encrypt_vectors_dev(ctx.h, None, 0, 4, d.p) != 0
    assert L.sfg_encrypt_explicit_dev(ctx.h, None, 0, 4, d.p, d.p, d.p, d.p) != 0
    assert L.sfg_ct_add_fresh_zero_dev(ctx.h, d.p, 1, -1) != 0
    before = ctx.encryptor_next_index()
    assert np.array_equal(d.host(), keep) and ctx.encryptor_next_index() == before
    d.free()
    # the hook without the switch
    saved = os.environ.pop("SFG_ENABLE_TEST_HOOKS", None)
    try:
        other = capi.Context(ol.Q_PN14, ol.P_PN14)
    finally:
        if saved is not None:
            os.environ["SFG_ENABLE_TEST_HOOKS"] = saved
    try:
        other.load_public_key(pk); other.seed_encryptor(KEY)
        with pytest.raises(capi.SfgError, match="test hook, enabled only"):
            other.encrypt_transcript(0, 1)
    finally:
        other.close()


def test_core_second_chunk_at_1366_ciphertexts(env):
    """level 0: the core's chunk is 2^30 // (2 * 3 * N * 8) = 1365 ciphertexts (batch_plan.hpp enc_core_plan), so 1366 is the smallest call with a second chunk.
    Every item has its own u, e0, e1 and plaintext.  Items 1364 and 1365, either side of the boundary, word for word against the big-integer statement; every
    item against the same inputs submitted as two calls split at the boundary (one chunk each)."""
    ctx, ring, s, pk = env
    level, nct, cut = 0, 1366, 1365
    assert cut == (1 << 30) // (2 * (level + 1 + NP) * N * 8)
    rnd = np.random.default_rng(1366)
    q = ring.moduli[0]
    u = rnd.integers(-1, 2, (nct, N)).astype(np.int8)
    e0 = rnd.integers(-19, 20, (nct, N)).astype(np.int32)
    e1 = rnd.integers(-19, 20, (nct, N)).astype(np.int32)
    pt = rnd.integers(0, q, (nct, 1, N), dtype=np.uint64)
    got = ctx.encrypt_explicit(pt, level, u, e0, e1)
    assert got.shape == (nct, 2, 1, N) and got.max() < q
    for i in (cut - 1, cut):
        c0, c1 = er.encrypt_bigint(ring, level, pk, u[i], e0[i], e1[i])[0]             # {row: (c0 row, c1 row)}
        assert np.array_equal(got[i, 0, 0], (np.array(c0, dtype=np.uint64) + pt[i, 0]) % np.uint64(q)), i
        assert np.array_equal(got[i, 1, 0], np.array(c1, dtype=np.uint64)), i
    assert np.array_equal(got[:cut], ctx.encrypt_explicit(pt[:cut], level, u[:cut], e0[:cut], e1[:cut]))
    assert np.array_equal(got[cut:], ctx.encrypt_explicit(pt[cut:], level, u[cut:], e0[cut:], e1[cut:]))
