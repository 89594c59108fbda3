"""Collective decryption and decoding on the device (sfgwas_amd/csrc/decrypt.hip): the shares word for word against the big-integer statement
(tests/encrypt_ref.py), the decoded coefficients bit for bit against Python's correctly rounded rational division, the slots against the exact decoder
(tests/decode_ref.py, pinned by tests/test_decode_ref.py) and against the complex128 pipeline they replace, a two-party decryption end to end, a product read on
the device, and the refusals.  PN14 moduli; the oracle's Ring supplies NTTs, secrets and decryption.

PARITY UNPINNED against lattigo's PCKSProtocol and encoder.Decode (no Go toolchain): what is pinned is the arithmetic."""
import ctypes as C
import math
from fractions import Fraction

import numpy as np
import pytest

import decode_ref
import encrypt_ref as er
import exactref
import oracle_lib as ol
import pyref

pytestmark = pytest.mark.gpu
N, NQ, NP = 1 << 14, len(ol.Q_PN14), len(ol.P_PN14)
n = N // 2
P_PROD = ol.P_PN14[0] * ol.P_PN14[1]
NOISE_BOUND = -(-19 * (2 * N + 1) // P_PROD) + 2 * (N + 1)       # tests/test_gpu_encrypt.py: a fresh encryption under a ternary secret, |e| <= 19
B = 2.0 ** -53 + 2.0 ** -82                                       # include/sfgwas_hip.h: |d_t - v_t| <= B max_t |v_t| (derived in decrypt.hip / DESIGN.md)


@pytest.fixture(scope="module")
def env():
    from sfgwas_amd import capi
    ring = ol.Ring(14, ol.Q_PN14, ol.P_PN14)
    ctx = capi.Context(ol.Q_PN14, ol.P_PN14)
    s = ring.gen_secret(31)
    ctx.load_secret_key(ol.secret_ntt(ring, s))
    yield ctx, ring, s
    ctx.close()


def rows_of(ring, level, p):
    """NTT-domain rows [level+1][N] of the integer polynomial p"""
    return np.stack([ring.ntt(m, np.array([int(x) % ring.moduli[m] for x in p], dtype=np.uint64)) for m in range(level + 1)])


def q_level(ring, level):
    Q = 1
    for m in range(level + 1):
        Q *= ring.moduli[m]
    return Q


def test_shares_every_word_against_big_integers(env):
    """levels 0, 4, 9, three ciphertexts (errors random in [-38, 38] / all +38 / alternating +-38): h0 = ModDown_P(NTT_QP(e0)) + sk (.) c1 and h1 = ModDown_P(NTT_QP(e1)),
    the ModDown being encrypt_bigint's for the zero public key and u = 0; level 4 is rows 0..4 of level 9; h1 = NULL gives the same h0"""
    ctx, ring, s = env
    rnd = np.random.default_rng(41)
    alt = np.where(np.arange(N) % 2 == 0, 38, -38)
    e0 = np.stack([rnd.integers(-38, 39, N), np.full(N, 38), alt]).astype(np.int32)
    e1 = np.stack([rnd.integers(-38, 39, N), np.full(N, 38), -alt]).astype(np.int32)
    zero_pk = np.zeros((2, NQ + NP, N), dtype=np.uint64)
    zero_u = np.zeros(N, dtype=np.int64)
    sk = ol.secret_ntt(ring, s)
    ct9 = np.stack([ring.fill_uniform(9, 100 + i) for i in range(3)])
    got = {}
    for level in (0, 4, 9):
        nl = level + 1
        cts = np.ascontiguousarray(ct9[:, :, :nl])
        h0, h1 = ctx.pcks_gen_share(cts, level, e0, e1)
        h0_only, none = ctx.pcks_gen_share(cts, level, e0)
        assert none is None and np.array_equal(h0_only, h0)
        assert h0.shape == h1.shape == (3, nl, N)
        for i in range(3):
            ref = er.encrypt_bigint(ring, level, zero_pk, zero_u, e0[i], e1[i])
            for m in range(nl):
                q = ring.moduli[m]
                w0 = np.array([(int(a) + int(b) * int(c)) % q for a, b, c in zip(ref[m][0], sk[m], cts[i, 1, m])], dtype=np.uint64)
                assert np.array_equal(h0[i, m], w0), (level, i, m, "h0")
                assert np.array_equal(h1[i, m], np.array(ref[m][1], dtype=np.uint64)), (level, i, m, "h1")
        got[level] = (h0, h1)
    for k in range(2):
        assert np.array_equal(got[4][k], got[9][k][:, :5]) and np.array_equal(got[0][k], got[9][k][:, :1])


def test_coefficients_bit_for_bit(env):
    """sfg_decode_coeffs on planted centred integers: every output is float(Fraction(p) / Fraction(scale)), which Python rounds correctly.  No tolerance."""
    ctx, ring, s = env
    rnd = np.random.default_rng(43)
    pyr = __import__("random").Random(47)
    for level in (0, 4, 9):
        Q = q_level(ring, level)
        half = Q // 2
        # x == floor(Q/2) is negative by the Cmp rule: the planted values are the REPRESENTED ones
        p = [0, 1, -1, half - Q, half - 1, half + 1 - Q] + [pyr.randrange(half - Q, half) for _ in range(N - 6)]
        p[100:108] = [3, -3, (1 << 40) + 1, -((1 << 40) + 1), min(half - 1, (1 << 53) + 1), -min(half - 1, (1 << 53) + 1), 2, -2]
        rows = rows_of(ring, level, p)[None]
        for scale in (2.0 ** 34, 2.0 ** 68, 2.0 ** 68 / float(ring.moduli[4])):
            got = ctx.decode_coeffs(rows, level, scale)[0]
            fs = Fraction(scale)
            want = np.array([float(Fraction(x) / fs) for x in p])
            bad = np.nonzero(got != want)[0]
            assert bad.size == 0, (level, scale, bad[:5], [(p[i], got[i], want[i]) for i in bad[:3]])


def slot_errors(d_re, d_im, E_re, E_im):
    err = 0.0
    for t in range(n):
        err = max(err, abs(float(Fraction(float(d_re[t])) - E_re[t])))
        if d_im is not None:
            err = max(err, abs(float(Fraction(float(d_im[t])) - E_im[t])))
    return err


def test_slots_against_the_exact_decoder_and_the_complex128_pipeline(env):
    """err_dev = max_t |d_t - E_t| against decode_ref; (1) err_dev <= err_c128, the error of pyref.decode(float(p_c) / scale) - the complex128 arithmetic that stands in
    for lattigo's decoder - on the same input against the same exact values; (2) err_dev <= B max_t |E_t|, B = 2^-53 + 2^-82 from the header.  Real-only and
    real-and-imaginary calls return the same real parts bit for bit."""
    ctx, ring, s = env
    rnd = np.random.default_rng(53)
    pyr = __import__("random").Random(59)
    Q9 = q_level(ring, 9)
    cases = [
        ("a: encode(uniform(-100, 100)), level 4, scale 2^34", 4, 2.0 ** 34, exactref.encode(rnd.uniform(-100, 100, n), N, 2.0 ** 34)[0], False),
        ("b: the same at level 0", 0, 2.0 ** 34, exactref.encode(rnd.uniform(-100, 100, n), N, 2.0 ** 34)[0], False),
        ("c: product-like, level 4, scale 2^68", 4, 2.0 ** 68, [pyr.randrange(-(1 << 72), 1 << 72) for _ in range(N)], False),
        ("d: full range, level 9, real and imaginary", 9, 2.0 ** 34, [pyr.randrange(Q9 // 2 - Q9 + 1, Q9 // 2) for _ in range(N)], True),
    ]
    for name, level, scale, p, both in cases:
        rows = rows_of(ring, level, p)[None]
        E_re, E_im, ref_err = decode_ref.decode(p, N, Fraction(scale))
        emax = max(math.hypot(float(a), float(b)) for a, b in zip(E_re, E_im))
        assert float(ref_err) <= emax * 2.0 ** -120
        d_re = ctx.decode_vectors(rows, level, scale)[0]
        d_re2, d_im = ctx.decode_vectors(rows, level, scale, want_imag=True)
        assert np.array_equal(d_re, d_re2[0]), name
        c128 = pyref.decode(np.array([float(x) for x in p]) / scale, N)
        err_dev = slot_errors(d_re, d_im[0] if both else None, E_re, E_im)
        err_c128 = slot_errors(c128.real, c128.imag if both else None, E_re, E_im)
        print(f"{name}: err_dev = {err_dev:.3e}, err_c128 = {err_c128:.3e}, B max|E| = {B * emax:.3e} (max|E| = {emax:.3e})")
        assert err_dev <= err_c128, name
        assert err_dev <= B * emax, name


def keypair_for(ring, s, seed):
    """pk = (-a s + e, a) over all of Q and P, NTT domain, for the GIVEN secret; |e| <= 19"""
    rnd = np.random.default_rng(seed)
    e = rnd.integers(-19, 20, N)
    pk = np.zeros((2, len(ring.moduli), N), dtype=np.uint64)
    for m, q in enumerate(ring.moduli):
        a = rnd.integers(0, q, N, dtype=np.uint64)
        sh = ring.ntt(m, np.array([int(x) % q for x in s], dtype=np.uint64))
        eh = ring.ntt(m, np.array([int(x) % q for x in e], dtype=np.uint64))
        pk[0, m] = np.array([(-(int(x) * int(y)) + int(z)) % q for x, y, z in zip(a, sh, eh)], dtype=np.uint64)
        pk[1, m] = a
    return pk


def test_two_party_collective_decryption_end_to_end(env):
    """s = s1 + s2 with the two shards on disjoint supports (even / odd coefficients of two ternary secrets), so s is ternary with |s|_1 <= N and the noise of a fresh
    encryption under its public key is test_gpu_encrypt.py's: c0 + c1 s = m + (u e_pk + e0 + e1 s) / P + rounding, |u|, |s| <= 1, |e| <= 19:
    |.| <= ceil(19 (2N + 1) / P) + 2 (N + 1) = NOISE_BOUND (each of c0, c1 off by < 2 from the ModDown, c1 meeting |s|_1 <= N).  Every party adds ModDown_P(e0_i) with
    |e0_i| <= 38: at most ceil(38 / P) + 2 in a coefficient (the quotient, and the ModDown's rounding < 2).  The encoder rounds each coefficient by at most 1/2.
    Each of the N real coefficients moves a slot by at most its own error (|zeta| = 1):  |out - v| <= (NOISE_BOUND + 2 (ceil(38 / P) + 2) + 1/2) N / scale.
    Derived, not measured."""
    from sfgwas_amd import capi
    ctx, ring, _ = env
    level, scale = 4, 2.0 ** 34
    mask = (np.arange(N) % 2 == 0)
    s1 = np.where(mask, ring.gen_secret(71), 0).astype(np.int8)
    s2 = np.where(~mask, ring.gen_secret(73), 0).astype(np.int8)
    s = (s1 + s2).astype(np.int8)
    assert np.abs(s).max() <= 1
    rnd = np.random.default_rng(61)
    v = rnd.uniform(-100, 100, (2, n))
    e0 = rnd.integers(-38, 39, (2, 2, N)).astype(np.int32)
    parties = [capi.Context(ol.Q_PN14, ol.P_PN14) for _ in range(2)]
    try:
        parties[0].load_public_key(keypair_for(ring, s, 67))
        parties[0].seed_encryptor(er.TEST_KEY)
        ct = parties[0].encrypt_vectors(v, level)
        cts = ct.host(); ct.free()
        qs = np.array(ring.moduli[:level + 1], dtype=np.uint64).reshape(1, level + 1, 1)
        agg = np.zeros((2, level + 1, N), dtype=np.uint64)
        for i, (c, si) in enumerate(zip(parties, (s1, s2))):
            c.load_secret_key(ol.secret_ntt(ring, si))
            h0, _ = c.pcks_gen_share(cts, level, e0[i])
            agg = (agg + h0) % qs
        out = parties[1].pcks_finish(cts, level, agg, scale=scale)
        per_party = -(-38 // P_PROD) + 2
        bound = (NOISE_BOUND + 2 * per_party + 0.5) * N / scale
        worst = np.abs(out - v).max()
        print(f"two-party decryption: max |out - v| = {worst:.3e}, bound {bound:.3e}")
        assert worst <= bound
        pt = parties[1].pcks_finish(cts, level, agg)
        assert np.array_equal(parties[1].decode_vectors(pt, level, scale), out)          # finish + decode = the fused call, bit for bit
        # the plaintext rows ARE c0 + h0agg
        assert np.array_equal(pt, (cts[:, 0] + agg) % qs)
    finally:
        for c in parties:
            c.close()


def test_a_product_read_on_the_device(env):
    """the 60 x 40 product of test_gpu_encrypt.py's last test under the loaded key: sfg_decrypt_vectors of the output words = decode_ref of the oracle's decryption of
    the same words, within the decoder's bound"""
    from sfgwas_amd import capi
    from sfgwas_amd.params import rotations_for_matmul
    ctx, ring, s = env
    rots = rotations_for_matmul()
    ctx.check(capi.lib().sfg_fill_rotkeys_synthetic(ctx.h, (C.c_int * len(rots))(*rots), len(rots), 77), "rotkeys")
    gd, g = ctx.fill_geno(60, 40, 12)
    A = ctx.fill_uniform_cts(1, 5, 0xA11)
    out = ctx.matmul_resident(A, 1, 5, 5, g)
    words = out.host()
    scale = 2.0 ** 68
    got = ctx.decrypt_vectors(out, 4, scale)
    for a in (out, A, gd):
        a.free()
    ctx.geno_free(g)
    assert words.shape == (1, 1, 2, 5, N) and got.shape == (1, n)
    res = ring.decrypt_residues(s, 4, words[0, 0])
    p = pyref.crt_centered([[int(x) for x in res[m]] for m in range(5)], ring.moduli[:5])
    E_re, E_im, _ = decode_ref.decode(p, N, Fraction(scale))
    emax = max(math.hypot(float(a), float(b)) for a, b in zip(E_re, E_im))
    err = slot_errors(got[0], None, E_re, E_im)
    print(f"product: err_dev = {err:.3e}, B max|E| = {B * emax:.3e}")
    assert emax > 0 and err <= B * emax


def test_refusals_are_clean_errors(env):
    from sfgwas_amd import capi
    ctx, ring, s = env
    L = capi.lib()
    d = ctx.fill_uniform_cts(1, 4, 1)
    sentinel = np.full((1, n), 7.25)
    out = sentinel.copy()
    po = out.ctypes.data_as(C.c_void_p)
    bare = capi.Context(ol.Q_PN14, ol.P_PN14)
    try:
        db = bare.fill_uniform_cts(1, 4, 1)
        with pytest.raises(capi.SfgError, match="no secret"):
            bare.decrypt_vectors(db, 4, 2.0 ** 34)
        with pytest.raises(capi.SfgError, match="no secret"):
            bare.pcks_gen_share(db, 4, np.zeros((1, N), np.int32))
        db.free()
    finally:
        bare.close()
    stride = 2 * 5 * N
    for level in (-1, NQ):
        assert L.sfg_decode_vectors(ctx.h, d.p, stride, 1, level, 2.0 ** 34, po, None) != 0 and b"level" in L.sfg_last_error(ctx.h)
        assert L.sfg_decrypt_vectors(ctx.h, d.p, 1, level, 2.0 ** 34, po, None) != 0
        assert L.sfg_pcks_gen_share_dev(ctx.h, d.p, 1, level, d.p, None, d.p, None) != 0
        assert L.sfg_pcks_finish_dev(ctx.h, d.p, 1, level, d.p, d.p) != 0
    for scale in (0.5, 0.0, -4.0, float("nan"), float("inf")):
        assert L.sfg_decode_vectors(ctx.h, d.p, stride, 1, 4, scale, po, None) != 0 and b"scale" in L.sfg_last_error(ctx.h)
        assert L.sfg_decode_coeffs(ctx.h, d.p, stride, 1, 4, scale, po) != 0
        assert L.sfg_pcks_finish_decode(ctx.h, d.p, 1, 4, scale, d.p, po, None) != 0
    assert L.sfg_decode_vectors(ctx.h, d.p, stride, -1, 4, 2.0 ** 34, po, None) != 0 and b"count" in L.sfg_last_error(ctx.h)
    assert L.sfg_decode_vectors(ctx.h, d.p, N, 1, 4, 2.0 ** 34, po, None) != 0 and b"stride" in L.sfg_last_error(ctx.h)
    for fn_rc in (L.sfg_decode_vectors(ctx.h, d.p, stride, 0, 4, 2.0 ** 34, po, None), L.sfg_decrypt_vectors(ctx.h, d.p, 0, 4, 2.0 ** 34, po, None),
                  L.sfg_decode_coeffs(ctx.h, d.p, stride, 0, 4, 2.0 ** 34, po), L.sfg_pcks_finish_decode(ctx.h, d.p, 0, 4, 2.0 ** 34, d.p, po, None),
                  L.sfg_pcks_gen_share_dev(ctx.h, d.p, 0, 4, d.p, None, d.p, None), L.sfg_pcks_finish_dev(ctx.h, d.p, 0, 4, d.p, d.p)):
        assert fn_rc == 0                                                # nct == 0
    # an outstanding near-tie condition: the decode calls fail like sfg_memcpy_d2h, until the reset
    ctx.encoder_near_ties(reset=True)
    ctx.check(L.sfg_ctx_encoder_inject_unsafe_for_test(ctx.h, 2), "inject")
    try:
        assert L.sfg_decode_vectors(ctx.h, d.p, stride, 1, 4, 2.0 ** 34, po, None) != 0 and b"rounding tie" in L.sfg_last_error(ctx.h)
        assert L.sfg_decrypt_vectors(ctx.h, d.p, 1, 4, 2.0 ** 34, po, None) != 0 and b"rounding tie" in L.sfg_last_error(ctx.h)
        assert L.sfg_decode_coeffs(ctx.h, d.p, stride, 1, 4, 2.0 ** 34, po) != 0
    finally:
        ctx.encoder_near_ties(reset=True)
    assert np.array_equal(out, sentinel)                                 # nothing was written by any refused call
    assert L.sfg_decrypt_vectors(ctx.h, d.p, 1, 4, 2.0 ** 34, po, None) == 0 and not np.array_equal(out, sentinel)
    d.free()


# ---------------------------------------------------------------- a second chunk at the smallest shapes that reach one (level 0; batch_plan.hpp holds the chunk rules)
# The refresh entry points (sfg_refresh_gen_shares_dev, sfg_refresh_finish_dev, sfg_ckks_to_ss_share_dev) chunk at 32768 ciphertexts: their second chunk needs
# more than 8 GB of input and has no GPU test; tests/test_proto_plan.py holds that rule on the CPU.
def test_shares_second_chunk_at_257_ciphertexts(env):
    """sfg_pcks_gen_share_dev takes 256 ciphertexts a chunk.  Every item has its own ciphertext and errors; items 255 and 256 against the big-integer statement
    as in test_shares_every_word_against_big_integers, every item against two calls split at the boundary; h1 = NULL gives the same h0"""
    ctx, ring, s = env
    level, nct, cut = 0, 257, 256
    rnd = np.random.default_rng(257)
    q = ring.moduli[0]
    cts = rnd.integers(0, q, (nct, 2, 1, N), dtype=np.uint64)
    e0 = rnd.integers(-38, 39, (nct, N)).astype(np.int32)
    e1 = rnd.integers(-38, 39, (nct, N)).astype(np.int32)
    h0, h1 = ctx.pcks_gen_share(cts, level, e0, e1)
    assert h0.shape == h1.shape == (nct, 1, N)
    zero_pk = np.zeros((2, NQ + NP, N), dtype=np.uint64)
    zero_u = np.zeros(N, dtype=np.int64)
    sk = ol.secret_ntt(ring, s)
    for i in (cut - 1, cut):
        ref = er.encrypt_bigint(ring, level, zero_pk, zero_u, e0[i], e1[i])
        w0 = np.array([(int(a) + int(b) * int(c)) % q for a, b, c in zip(ref[0][0], sk[0], cts[i, 1, 0])], dtype=np.uint64)
        assert np.array_equal(h0[i, 0], w0), (i, "h0")
        assert np.array_equal(h1[i, 0], np.array(ref[0][1], dtype=np.uint64)), (i, "h1")
    for a, b in ((0, cut), (cut, nct)):
        p0, p1 = ctx.pcks_gen_share(cts[a:b], level, e0[a:b], e1[a:b])
        assert np.array_equal(h0[a:b], p0) and np.array_equal(h1[a:b], p1), a
    h0_only, none = ctx.pcks_gen_share(cts, level, e0)
    assert none is None and np.array_equal(h0_only, h0)


def test_decoder_second_chunk_at_513_plaintexts(env):
    """the decoder takes 512 plaintexts a chunk.  513 plaintexts of planted centred integers, every one different: sfg_decode_coeffs of items 511 and 512 bit for
    bit against Python's correctly rounded division (no tolerance), every item against two calls split at the boundary; sfg_decode_vectors, real and complex, of
    items 511 and 512 against the exact decoder within the header's bound B max|E|, and every item against the split calls"""
    ctx, ring, s = env
    level, nct, cut, scale = 0, 513, 512, 2.0 ** 34
    q = ring.moduli[0]
    half = q // 2
    rnd = np.random.default_rng(513)
    p = rnd.integers(half - q, half, (nct, N))                              # the represented values: floor(Q/2) itself is negative by the Cmp rule
    p[cut - 1, :4] = [half - q, half - 1, 0, -1]
    p[cut, :4] = [half - 1, half - q, 1, -2]
    assert len({row.tobytes() for row in p}) == nct
    rows = np.stack([ring.ntt(0, (pi % q).astype(np.uint64)) for pi in p])[:, None]          # rows_of, without a Python integer per word
    assert np.array_equal(rows[cut], rows_of(ring, level, p[cut]))
    coeffs = ctx.decode_coeffs(rows, level, scale)
    fs = Fraction(scale)
    for i in (cut - 1, cut):
        want = np.array([float(Fraction(int(x)) / fs) for x in p[i]])
        assert np.array_equal(coeffs[i], want), i
    assert np.array_equal(coeffs[:cut], ctx.decode_coeffs(rows[:cut], level, scale)) and np.array_equal(coeffs[cut:], ctx.decode_coeffs(rows[cut:], level, scale))
    re = ctx.decode_vectors(rows, level, scale)
    re2, im = ctx.decode_vectors(rows, level, scale, want_imag=True)
    assert np.array_equal(re, re2)
    for i in (cut - 1, cut):
        E_re, E_im, _ = decode_ref.decode([int(x) for x in p[i]], N, fs)
        emax = max(math.hypot(float(a), float(b)) for a, b in zip(E_re, E_im))
        err = slot_errors(re[i], im[i], E_re, E_im)
        print(f"item {i}: err_dev = {err:.3e}, B max|E| = {B * emax:.3e}")
        assert emax > 0 and err <= B * emax, i
    for a, b in ((0, cut), (cut, nct)):
        pr, pi_ = ctx.decode_vectors(rows[a:b], level, scale, want_imag=True)
        assert np.array_equal(re[a:b], pr) and np.array_equal(im[a:b], pi_), a
