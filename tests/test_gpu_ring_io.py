"""The general ring's two ends on the GPU (sfgwas_amd/csrc/gring_io.hip, capi.Ring): the encoder word for word against tests/exactref.py and the oracle, the sampler
against the Python map of tests/ring_io_ref.py at every logN, public-key encryption word for word against encrypt_ref.encrypt_bigint on the chains of
tests/ring_cases.py, the sampled forms against transcript + explicit with their index accounting, the collective decryption's shares against their big-integer
statement, the decoder's coefficients against the exact quotient and its slots against tests/decode_ref.py within the derived bound, the PN14 chain against the
specialised Context, an end-to-end encrypt / rotate / square / rescale / two-party decryption on two wide chains wholly on the device, a call that crosses a chunk
boundary, and every refusal with its message.  One device ring, one reference ring and one key pair per chain for the module."""
import atexit
import ctypes as C
import os

import numpy as np
import pytest

import decode_ref
import encrypt_ref as er
import exactref
import oracle_lib as ol
import ring_cases as rc
import ring_io_ref as rio
import ring_ref
from sfgwas_amd import capi

pytestmark = pytest.mark.gpu

KEY = er.TEST_KEY
_ENV = {}


class Env:
    def __init__(self, name):
        self.name = name
        self.logN, self.q, self.p = rc.chain(name)
        self.dev = capi.Ring(self.logN, self.q, self.p)
        self.ring = ring_ref.SplitRing(self.logN, self.q, self.p) if name == "L19" else ol.Ring(self.logN, self.q, self.p)
        self.N, self.slots, self.moduli, self.top = self.ring.N, self.ring.N // 2, self.ring.moduli, len(self.q) - 1
        self.s, self.pk = rio.keypair(self.ring, 31)
        self.dev.load_public_key(self.pk)
        self.dev.seed_encryptor(KEY)

    def rows(self, rnd, n, level):
        """n sets of uniform canonical rows [n][level+1][N]"""
        return np.stack([np.stack([rnd.integers(0, self.moduli[m], self.N, dtype=np.uint64) for m in range(level + 1)]) for _ in range(n)])

    def add_rows(self, a, b, level):
        """a + b mod q_m on [level+1][N] rows (sums below 2^62)"""
        return np.stack([(a[m] + b[m]) % np.uint64(self.moduli[m]) for m in range(level + 1)])

    def ref_encrypt(self, level, u, e0, e1):
        return rio.ct_rows(er.encrypt_bigint(self.ring, level, self.pk, u, e0, e1), level)


def env(name):
    if name not in _ENV:
        _ENV[name] = Env(name)
    return _ENV[name]


@atexit.register
def _close_all():
    for e in _ENV.values():
        e.dev.close()
    _ENV.clear()


def encrypt_sampled(dev, pt, level, nct=None):
    """encryptor.EncryptNew with samples drawn on the device: ct += Enc(0) on (pt, 0) - c_0 += pt is the core's last step; pt None: nct encryptions of zero"""
    nct = pt.shape[0] if pt is not None else nct
    base = np.zeros((nct, 2, level + 1, dev.N), dtype=np.uint64)
    if pt is not None:
        base[:, 0] = pt
    return dev.add_fresh_zero(base, level)


def small(rnd, n, N, bound):
    return rnd.integers(-bound, bound + 1, (n, N)).astype(np.int32)


# ---------------------------------------------------------------- the sampler
@pytest.mark.parametrize("name", ["G12", "G13", "P14", "W15", "W16"])
def test_transcript_equals_the_python_map_at_every_logN(name):
    e = env(name)
    for first, n in ((0, 2), ((1 << 32) + 5, 1)):
        u, e0, e1 = e.dev.encrypt_transcript(first, n)
        wu, w0, w1 = rio.transcript(KEY, first, n, e.N)
        assert np.array_equal(u, wu) and np.array_equal(e0, w0) and np.array_equal(e1, w1), (name, first)


# ---------------------------------------------------------------- the explicit form, word for word
EXPLICIT = [("G12", 1), ("G12", 0), ("W15", 3), ("W15", 1), ("W15", 0), ("W16", 2), ("W16", 0), ("X12", 2), ("X12", 0), ("L19", 16), ("L19", 0)]


@pytest.mark.parametrize("name,level", EXPLICIT)
def test_encrypt_explicit_equals_the_big_integer_statement(name, level):
    """three ciphertexts in one batch with plaintexts (the all-zero transcript, u = 1 with e = +19 / -19, a random transcript), then the random one alone without a
    plaintext.  c_0 += pt is the statement's last step: the reference is computed once per transcript without it and the rows are added here."""
    e = env(name)
    rnd = np.random.default_rng(100 + level)
    N = e.N
    U = np.stack([np.zeros(N, np.int8), np.ones(N, np.int8), rnd.integers(-1, 2, N).astype(np.int8)])
    E0 = np.stack([np.zeros(N, np.int32), np.full(N, 19, np.int32), small(rnd, 1, N, 19)[0]])
    E1 = np.stack([np.zeros(N, np.int32), np.full(N, -19, np.int32), small(rnd, 1, N, 19)[0]])
    pt = e.rows(rnd, 3, level)
    got = e.dev.encrypt_explicit(pt, level, U, E0, E1)
    assert np.array_equal(got[0, 0], pt[0]) and not got[0, 1].any(), (name, level, "zero transcript")
    for j in (1, 2):
        want = e.ref_encrypt(level, U[j], E0[j], E1[j])
        assert np.array_equal(got[j, 1], want[1]), (name, level, j)
        assert np.array_equal(got[j, 0], e.add_rows(want[0], pt[j], level)), (name, level, j)
    alone = e.dev.encrypt_explicit(None, level, U[2:], E0[2:], E1[2:])
    assert np.array_equal(alone[0], want), (name, level, "no plaintext")
    for m in range(level + 1):
        assert got[:, :, m].max() < e.moduli[m]


def test_keys_in_montgomery_form_load_to_the_same_words():
    e = env("G12")
    rnd = np.random.default_rng(3)
    mont = np.stack([np.stack([np.array([(int(x) << 64) % q for x in e.pk[p_, m]], dtype=np.uint64) for m, q in enumerate(e.moduli)]) for p_ in range(2)])
    args = (None, 1, rnd.integers(-1, 2, (1, e.N)).astype(np.int8), small(rnd, 1, e.N, 19), small(rnd, 1, e.N, 19))
    want = e.dev.encrypt_explicit(*args)
    other = capi.Ring(e.logN, e.q, e.p)
    try:
        assert not other.has_public_key()
        other.load_public_key(mont, montgomery=True)
        assert other.has_public_key() and np.array_equal(other.encrypt_explicit(*args), want)
        sk = rio.sk_rows(e.ring, e.s)
        sk_m = np.stack([np.array([(int(x) << 64) % q for x in sk[m]], dtype=np.uint64) for m, q in enumerate(e.q)])
        cts, e0 = e.rows(rnd, 2, 1).reshape(1, 2, 2, e.N), small(rnd, 1, e.N, 38)
        other.load_secret_key(sk_m, montgomery=True)
        e.dev.load_secret_key(sk)
        assert np.array_equal(other.pcks_gen_share(cts, 1, e0)[0], e.dev.pcks_gen_share(cts, 1, e0)[0])
    finally:
        other.close()


# ---------------------------------------------------------------- the sampled forms and the index
@pytest.mark.parametrize("name,level", [("G13", 5), ("W15", 1), ("L19", 16)])
def test_sampled_forms_equal_transcript_plus_explicit_and_count_their_indices(name, level):
    e = env(name)
    rnd = np.random.default_rng(7)
    e.dev.seed_encryptor(KEY)
    assert e.dev.encryptor_next_index() == 0
    pt = e.rows(rnd, 3, level)
    got = encrypt_sampled(e.dev, pt, level)
    assert e.dev.encryptor_next_index() == 3
    assert np.array_equal(got, e.dev.encrypt_explicit(pt, level, *e.dev.encrypt_transcript(0, 3)))
    one = encrypt_sampled(e.dev, None, level, nct=1)                                  # index 3, no plaintext
    assert e.dev.encryptor_next_index() == 4
    assert np.array_equal(one, e.dev.encrypt_explicit(None, level, *e.dev.encrypt_transcript(3, 1)))
    base = e.rows(rnd, 6, level).reshape(3, 2, level + 1, e.N)
    added = e.dev.add_fresh_zero(base, level)                                      # indices 4, 5, 6
    assert e.dev.encryptor_next_index() == 7
    assert np.array_equal(added, e.dev.add(base, e.dev.encrypt_explicit(None, level, *e.dev.encrypt_transcript(4, 3)), level))
    e.dev.seed_encryptor(KEY)                                                      # seeding resets the index: the same ciphertexts again
    assert e.dev.encryptor_next_index() == 0 and np.array_equal(encrypt_sampled(e.dev, pt, level), got)
    e.dev.seed_encryptor(bytes(range(32)))                                         # another key, other samples
    assert not np.array_equal(encrypt_sampled(e.dev, pt[:1], level), got[:1])
    e.dev.seed_encryptor(KEY)


def test_a_call_that_crosses_a_chunk_boundary():
    """gring_io_plan.hpp caps a chunk at 256 ciphertexts: 257 fresh encryptions of zero at logN 12, level 0; the last of the first chunk and the first of the second
    must carry the samples of their own indices"""
    e = env("G12")
    e.dev.seed_encryptor(KEY)
    got = encrypt_sampled(e.dev, None, 0, nct=257)
    assert e.dev.encryptor_next_index() == 257
    assert np.array_equal(got[255:], e.dev.encrypt_explicit(None, 0, *e.dev.encrypt_transcript(255, 2)))
    assert np.array_equal(got[:1], e.dev.encrypt_explicit(None, 0, *e.dev.encrypt_transcript(0, 1)))
    e.dev.seed_encryptor(KEY)


# ---------------------------------------------------------------- the collective decryption's local halves
@pytest.mark.parametrize("name,level,nct", [("G12", 1, 3), ("W15", 1, 1), ("W16", 0, 1), ("X12", 2, 3), ("L19", 16, 1)])
def test_pcks_share_and_finish_equal_the_big_integer_statement(name, level, nct):
    e = env(name)
    rnd = np.random.default_rng(40 + level)
    share, _ = rio.split_secret(e.s, 9)                                            # one party's additive share of the key
    sk = rio.sk_rows(e.ring, share)
    e.dev.load_secret_key(sk)
    cts = e.rows(rnd, 2 * nct, level).reshape(nct, 2, level + 1, e.N)              # parity needs no valid ciphertext
    e0, e1 = small(rnd, nct, e.N, 38), small(rnd, nct, e.N, 38)
    h0, h1 = e.dev.pcks_gen_share(cts, level, e0, e1)
    for j in range(nct):
        w0, w1 = rio.pcks_share_bigint(e.ring, level, sk, cts[j], e0[j], e1[j])
        assert np.array_equal(h0[j], w0) and np.array_equal(h1[j], w1), (name, level, j)
    only0, none = e.dev.pcks_gen_share(cts, level, e0)
    assert none is None and np.array_equal(only0, h0)
    pt = e.dev.pcks_finish(cts, level, h0)
    for j in range(nct):
        assert np.array_equal(pt[j], e.add_rows(cts[j, 0], h0[j], level))


# ---------------------------------------------------------------- the encoder
ENC_SCALES = [2.0 ** 30, 2.0 ** 40, 2.0 ** 45, 2.0 ** 55]
_ENC = {}


def b_enc(p, n):
    """gring_io_arith.hpp: B_enc(Sp, n) = max(2^-50, 2^-93 (Sp + n))"""
    return max(2.0 ** -50, 2.0 ** -93 * (sum(abs(x) for x in p) + n))


def encoder_inputs(name):
    """(vectors [k][slots], scales [k], exact coefficients [k][N]) of a chain, computed once: random slots at four scales, |p| up to 2^61.9 (a constant vector at 2^59),
    a one-hot slot, an alternating vector, the zero vector, one tiny and one huge slot.  The wide chains take the first, the one-hot and the large one only (the exact
    reference costs a second a vector there).  The condition - no coefficient within B_enc of a tie - is asserted here, on the reference's own tie distance."""
    if name not in _ENC:
        e = env(name)
        n = e.slots
        rnd = np.random.default_rng(e.logN)
        vs, scs = [], []
        for sc in (ENC_SCALES if e.logN < 15 else ENC_SCALES[1 + (e.logN & 1):][:1]):
            vs.append(rnd.uniform(-8, 8, n)); scs.append(sc)
        hot = np.zeros(n); hot[n // 3] = -3.75
        vs.append(hot); scs.append(2.0 ** 40)
        vs.append(np.full(n, 2.0 ** 2.9)); scs.append(2.0 ** 59)
        if e.logN < 15:
            vs.append(np.where(np.arange(n) & 1, -1.5, 1.5)); scs.append(2.0 ** 45)
            vs.append(np.zeros(n)); scs.append(2.0 ** 30)
            mix = np.zeros(n); mix[1], mix[n - 2] = 2.0 ** -20, 1000.0
            vs.append(mix); scs.append(2.0 ** 45)
        ps = []
        for v, sc in zip(vs, scs):
            p, tie, err = exactref.encode(v, e.N, sc)
            assert float(np.min(tie)) - err > b_enc(p, n), (name, sc)
            ps.append(p)
        assert max(abs(x) for x in ps[len(ps) - 1 if e.logN >= 15 else len(ENC_SCALES) + 1]) > 2.0 ** 61.8
        _ENC[name] = (np.array(vs), scs, ps)
    return _ENC[name]


@pytest.mark.parametrize("name", ["G12", "G13", "W15", "W16", "X12", "L19"])
def test_encode_vectors_equals_the_exact_encoder_word_for_word(name):
    """every word of encode_vectors, through the device's inverse transform, equals p_c mod q_i of exactref.encode at the top level and at level 0; on the chains one
    oracle ring holds the rows also equal orc_encode_ntt (prec 0) directly"""
    e = env(name)
    vs, scs, ps = encoder_inputs(name)
    for level in (e.top, 0):
        for k, (v, sc, p) in enumerate(zip(vs, scs, ps)):
            got = e.dev.encode_vectors(v[None], level, sc)[0]
            for m in range(level + 1):
                assert got[m].max() < e.moduli[m]
            coef = e.dev.ntt_rows(got, list(range(level + 1)), inverse=True)
            want = np.array([[x % e.moduli[m] for x in p] for m in range(level + 1)], dtype=np.uint64)
            assert np.array_equal(coef, want), (name, level, k, np.argwhere(coef != want)[:4])
            if name != "L19" and k == 0:
                assert np.array_equal(got, e.ring.encode_ntt(v, sc, level + 1)), (name, level, "oracle")
    if e.logN < 15:                                                                  # one batch of all vectors of one scale
        idx = [k for k, sc in enumerate(scs) if sc == 2.0 ** 45]
        batch = e.dev.encode_vectors(vs[idx], e.top, 2.0 ** 45)
        for j, k in enumerate(idx):
            assert np.array_equal(batch[j], e.dev.encode_vectors(vs[k][None], e.top, 2.0 ** 45)[0])


def test_encoder_refuses_ties_and_inputs_outside_its_domain():
    e = env("G12")
    n = e.slots
    keep = e.dev.to_device(np.full((1, 2, e.N), 7, dtype=np.uint64))
    L = capi.lib()
    try:
        def call(v, scale):
            v = np.ascontiguousarray(v, dtype=np.float64)
            rc = L.sfg_ring_encode_vectors_dev(e.dev.h, v.ctypes.data_as(C.POINTER(C.c_double)), 1, 1, scale, keep)
            return rc, L.sfg_ring_last_error(e.dev.h).decode()
        rc, msg = call(np.full(n, 5.5 / 2.0 ** 30), 2.0 ** 30)                       # p_0 = 5 + 1/2 exactly: a tie
        assert rc == 1 and "1 coefficients lie within the proven band of a rounding tie" in msg, msg
        bad = np.zeros(n); bad[5] = float("nan")
        rc, msg = call(bad, 2.0 ** 30)
        assert rc == 1 and "value 5 of vector 0 is not finite" in msg
        bad[5] = float("-inf")
        assert call(bad, 2.0 ** 30)[0] == 1
        rc, msg = call(np.full(n, 8.0), 2.0 ** 60)                                   # p_0 = 2^63
        assert rc == 1 and "outside the domain |p| < 2^62" in msg, msg
        for scale in (0.5, float("nan"), float("inf")):
            rc, msg = call(np.zeros(n), scale)
            assert rc == 1 and "must be finite and at least 1" in msg
        assert (e.dev.to_host(keep, (1, 2, e.N)) == 7).all()                         # no refusal wrote a word
        with pytest.raises(capi.SfgError, match="level 2 out of range"):
            e.dev.encode_vectors(np.zeros((1, n)), 2, 2.0 ** 30)
        assert L.sfg_ring_encode_vectors_dev(e.dev.h, None, 0, 1, 2.0 ** 30, None) == 0
    finally:
        e.dev.free(keep)


@pytest.mark.parametrize("name,level", [("G13", 5), ("W15", 3), ("L19", 0)])
def test_encrypt_vectors_equals_encode_plus_transcript_plus_explicit(name, level):
    e = env(name)
    v = np.random.default_rng(23).uniform(-4, 4, (3, e.slots))
    e.dev.seed_encryptor(KEY)
    got = e.dev.encrypt_vectors(v, level, 2.0 ** 40)
    assert e.dev.encryptor_next_index() == 3
    assert np.array_equal(got, e.dev.encrypt_explicit(e.dev.encode_vectors(v, level, 2.0 ** 40), level, *e.dev.encrypt_transcript(0, 3)))
    with pytest.raises(capi.SfgError, match="outside the domain"):                  # the encoder's refusal comes first and spends no index
        e.dev.encrypt_vectors(np.full((1, e.slots), 8.0), level, 2.0 ** 60)
    assert e.dev.encryptor_next_index() == 3
    e.dev.seed_encryptor(KEY)


# ---------------------------------------------------------------- the decoder's slots
B_SLOT = 2.0 ** -53 + 2.0 ** -86            # gring_io_arith.hpp: kSlotBound, derived there


@pytest.mark.parametrize("name,level,scale", [("G12", 1, 2.0 ** 30), ("G13", 5, 2.0 ** 40 * 2.0 ** 40 / 1073692673.0), ("W15", 3, 2.0 ** 40), ("W16", 2, 2.0 ** 45 * 2.0 ** 45 / 35184372088891.0),
                                              ("L19", 16, 2.0 ** 34)])
def test_decode_vectors_is_within_the_derived_bound_of_the_exact_decoder(name, level, scale):
    """coefficients of a message-sized plaintext with noise (46-bit integers, all N of them: complex slots): both parts of every slot within B max|v| of
    decode_ref.decode (plus that reference's own error bound); the real parts are the same bits with and without im, from polynomial 0 of a ciphertext in place, and
    through the device-output form"""
    from fractions import Fraction
    e = env(name)
    rnd = np.random.default_rng(70 + level)
    p = [int(x) for x in rnd.integers(-(1 << 46), 1 << 46, e.N)]
    pt = coefficient_rows(e, level, [p])
    re, im = e.dev.decode_vectors(pt, level, scale, want_imag=True)
    wr, wi, err = decode_ref.decode(p, e.N, scale)
    vmax = max(float(a * a + b * b) for a, b in zip(wr, wi)) ** 0.5
    bound = Fraction(B_SLOT) * Fraction(vmax * (1 + 2.0 ** -40)) + err
    worst = max(max(abs(Fraction(float(g)) - w) for g, w in zip(re[0], wr)), max(abs(Fraction(float(g)) - w) for g, w in zip(im[0], wi)))
    print(f"{name}: worst slot error {float(worst):.3e}, bound {float(bound):.3e}, max|v| {vmax:.3e}")
    assert worst <= bound
    assert np.array_equal(e.dev.decode_vectors(pt, level, scale), re)
    cts = np.zeros((1, 2, level + 1, e.N), dtype=np.uint64)
    cts[0, 0], cts[0, 1] = pt[0], pt[0][::-1]
    assert np.array_equal(e.dev.decode_vectors(cts, level, scale, poly0_of_cts=True), re)
    r2, i2 = e.dev.decode_vectors(pt, level, scale, want_imag=True, on_device=True)
    assert np.array_equal(r2, re) and np.array_equal(i2, im)


# ---------------------------------------------------------------- the decoder's coefficients
def coefficient_rows(e, level, coeffs):
    """signed Python integers [n][N] -> NTT-domain plaintext rows [n][level+1][N] through the device's own forward transform (held to the oracle in test_gpu_ring.py)"""
    rows = np.array([[[int(p) % e.moduli[m] for p in c] for m in range(level + 1)] for c in coeffs], dtype=np.uint64)
    flat = e.dev.ntt_rows(rows.reshape(-1, e.N), [m for _ in coeffs for m in range(level + 1)])
    return flat.reshape(len(coeffs), level + 1, e.N)


@pytest.mark.parametrize("name,level,scale", [("X12", 2, 2.0 ** 55), ("X12", 0, 1.0), ("L19", 16, 1.2345678e12), ("G12", 1, 2.0 ** 30), ("W16", 2, 2.0 ** 45 * 2.0 ** 45 / 35184372088891.0)])
def test_decode_coeffs_is_the_correctly_rounded_exact_quotient(name, level, scale):
    """three plaintexts: the directed coefficients of ring_io_ref (0, +-1, Q/2 and one past it, carries through every digit) padded with small values, values of every
    size up to Q/2, and message-sized values.  Every coefficient equals the Fraction quotient correctly rounded; the condition of the contract - no quotient within
    2^-96 relative of a rounding boundary - is asserted on the inputs."""
    e = env(name)
    rnd = np.random.default_rng(60 + level)
    qs = e.moduli[:level + 1]
    Q = int(np.prod(np.array(qs, dtype=object)))
    h = Q // 2

    def rand_bits(bits):
        v = int.from_bytes(rnd.bytes(bits // 8 + 1), "little") >> (8 - bits % 8)
        return min(v, h) * (1 if rnd.integers(0, 2) else -1)
    directed = rio.directed_coefficients(qs)
    n = min(e.N, 8192)                                                             # non-zero coefficients per plaintext (the exact reference costs per coefficient)
    c0 = directed + [rand_bits(20) for _ in range(n - len(directed))] + [0] * (e.N - n)
    c1 = [0] * (e.N - n) + [rand_bits(int(rnd.integers(1, Q.bit_length() - 1))) for _ in range(n)]
    c2 = [rand_bits(min(50, Q.bit_length() - 2)) for _ in range(n)] + [0] * (e.N - n)
    coeffs = [c0, c1, c2]
    for c in coeffs:                                                               # keep exact ties and their neighbourhood out: the contract promises nothing there
        for i, p in enumerate(c):
            if p and rio.boundary_distance(rio.quotient(p, scale)) <= rio.DECODE_REL:
                c[i] = p + 1 if p < h else p - 1
                assert rio.boundary_distance(rio.quotient(c[i], scale)) > rio.DECODE_REL
    pt = coefficient_rows(e, level, coeffs)
    got = e.dev.decode_coeffs(pt, level, scale)
    want = np.array([[rio.rounded(rio.quotient(p, scale)) for p in c] for c in coeffs])
    assert np.array_equal(got, want), (name, level, np.argwhere(got != want)[:5])
    assert not np.signbit(got[0][0])                                               # the zero coefficient is +0
    # polynomial 0 of resident ciphertexts read in place, and one plaintext alone
    cts = np.zeros((3, 2, level + 1, e.N), dtype=np.uint64)
    cts[:, 0], cts[:, 1] = pt, pt[::-1]
    assert np.array_equal(e.dev.decode_coeffs(cts, level, scale, poly0_of_cts=True), want)
    assert np.array_equal(e.dev.decode_coeffs(pt[1:2], level, scale), want[1:2])


def test_decode_coeffs_after_encryption_and_decryption_returns_the_message_coefficients():
    """encrypt_explicit with zero errors, one-party share with zero error, finish, decode_coeffs: the message's coefficients over the scale, off by the two ModDowns'
    rounding only (|delta_0 + delta_1 s| <= 2 (1 + N) coefficient units, the bound of the tiny-ring test in test_ring_io_ref.py, plus 2 for the share's)"""
    e = env("G13")
    level, scale = e.top, 2.0 ** 30
    rnd = np.random.default_rng(17)
    msg = rnd.integers(-(1 << 40), 1 << 40, e.N)
    pt = coefficient_rows(e, level, [[int(x) for x in msg]])
    ct = e.dev.encrypt_explicit(pt, level, rnd.integers(-1, 2, (1, e.N)).astype(np.int8), small(rnd, 1, e.N, 19), small(rnd, 1, e.N, 19))
    e.dev.load_secret_key(rio.sk_rows(e.ring, e.s))
    h0, _ = e.dev.pcks_gen_share(ct, level, np.zeros((1, e.N), np.int32))
    got = e.dev.decode_coeffs(e.dev.pcks_finish(ct, level, h0), level, scale)[0]
    assert np.max(np.abs(got * scale - msg)) <= 2 * (1 + e.N) + 2


# ---------------------------------------------------------------- P14 against the specialised context
def test_p14_equals_the_specialised_context_word_for_word():
    """same parameters, same public key, same sampler key: the samples, the explicit encryption at three levels and the shares of both paths"""
    e = env("P14")
    ctx = capi.Context(e.q, e.p)
    try:
        ctx.load_public_key(e.pk)
        ctx.seed_encryptor(KEY)
        tr_c, tr_r = ctx.encrypt_transcript(0, 3), e.dev.encrypt_transcript(0, 3)
        assert all(np.array_equal(a, b) for a, b in zip(tr_c, tr_r))
        rnd = np.random.default_rng(14)
        for level in (e.top, 4, 0):
            pt = e.rows(rnd, 3, level)
            assert np.array_equal(e.dev.encrypt_explicit(pt, level, *tr_r), ctx.encrypt_explicit(pt, level, *tr_c)), level
        # the sampled forms from index 0 under one key: EncryptFloatVector of the context = its own encoder's rows through the ring's ct += Enc(0)
        v = rnd.uniform(-4, 4, (3, e.slots))
        for level in (e.top, 0):
            ctx.seed_encryptor(KEY)
            e.dev.seed_encryptor(KEY)
            want = ctx.encrypt_vectors(v, level)
            try:
                assert np.array_equal(encrypt_sampled(e.dev, ctx.encode_vectors(v, level), level), want.host()), level
            finally:
                want.free()
            assert ctx.encryptor_next_index() == e.dev.encryptor_next_index() == 3
        for level in (e.top, 0):                                                       # the encoder and EncryptFloatVector against their PN14 twins
            assert np.array_equal(e.dev.encode_vectors(v, level, 2.0 ** 34), ctx.encode_vectors(v, level)), level
            ctx.seed_encryptor(KEY)
            e.dev.seed_encryptor(KEY)
            want = ctx.encrypt_vectors(v, level)
            try:
                assert np.array_equal(e.dev.encrypt_vectors(v, level, 2.0 ** 34), want.host()), level
            finally:
                want.free()
        sk = rio.sk_rows(e.ring, e.s)
        ctx.load_secret_key(sk)
        e.dev.load_secret_key(sk)
        for level in (e.top, 0):
            cts = e.rows(rnd, 4, level).reshape(2, 2, level + 1, e.N)
            e0, e1 = small(rnd, 2, e.N, 38), small(rnd, 2, e.N, 38)
            g0, g1 = e.dev.pcks_gen_share(cts, level, e0, e1)
            c0, c1 = ctx.pcks_gen_share(cts, level, e0, e1)
            assert np.array_equal(g0, c0) and np.array_equal(g1, c1), level
            assert np.array_equal(e.dev.pcks_finish(cts, level, g0), ctx.pcks_finish(cts, level, c0)), level
    finally:
        ctx.close()


# ---------------------------------------------------------------- end to end
@pytest.mark.parametrize("name,scale", [("W15", 2.0 ** 40), ("W16", 2.0 ** 45)])
def test_end_to_end_encrypt_evaluate_and_decrypt_between_two_parties(name, scale):
    """encryption with samples drawn on the device, rotate right by 1, square, rescale, one share per party from additive key shares, summed on the host, finish; all of it
    on the device, from encrypt_vectors to decode_vectors.  Slots uniform in (-1, 1), bound 2^-16 of a unit slot.
    Where it comes from (W15, the tighter case: scale 2^40, q_top about 2^40, N = 2^15): the fresh encryption leaves the two ModDowns' rounding, delta_0 + delta_1 s
    with |delta| <= 2 and N / 3 non-zero terms of s: about 2^8.5 for independent terms (80 .. 388 measured on the reference statement); the rotation's key switch
    about 2^10 (the oracle's measurement, 354 .. 1232): 2^10.5 together.  Squaring multiplies it by twice the message polynomial, N coefficients of about
    2^40 / sqrt(N / 2): sqrt(N) 2^33.5 2^10.5 2 = 2^52.5 per coefficient, 2^12.5 after the division by q_top (the relinearisation adds its own 2^10 below that).  A
    slot sums N coefficients: sqrt(N) 2^12.5 = 2^20, four deviations 2^22, over the output scale 2^40: 2^-18.  The two shares add ModDown_P(e) <= 2 per coefficient and
    party, N 4 / 2^40 = 2^-23 at the worst.  2^-16 leaves a factor of four.  W16 (2^45, q_top about 2^45, N = 2^16) ends at 2^-23 by the same steps."""
    e = env(name)
    r, top = e.ring, e.top
    g = r.galois(e.slots - 1)
    key = r.gen_rotkey(e.s, g, 77 + g)
    e.dev.load_rotkey(g, key)
    rlk = np.zeros((r.beta, 2, len(e.moduli), e.N), dtype=np.uint64)
    ol.lib().orc_gen_rlk(r.h, ol.pi8(e.s), 4242, ol.p64(rlk))
    e.dev.load_relinkey(rlk)
    rnd = np.random.default_rng(5)
    v = rnd.uniform(-1, 1, e.slots)
    e.dev.seed_encryptor(KEY)
    ct = e.dev.encrypt_vectors(v[None], top, scale)
    rot = e.dev.rotate_right(ct, top, [1])
    out = e.dev.rescale(e.dev.mulrelin(rot, rot, top), top)
    lvl, out_scale = top - 1, scale * scale / e.q[top]
    agg = None
    for share in rio.split_secret(e.s, 11):
        e.dev.load_secret_key(rio.sk_rows(r, share))
        h0, _ = e.dev.pcks_gen_share(out, lvl, small(rnd, 1, e.N, 38))
        agg = h0 if agg is None else np.stack([e.add_rows(agg[0], h0[0], lvl)])
    re, im = e.dev.decode_vectors(e.dev.pcks_finish(out, lvl, agg), lvl, out_scale, want_imag=True)
    err = max(np.max(np.abs(re[0] - np.roll(v, 1) ** 2)), np.max(np.abs(im[0])))
    print(f"{name}: slot error {err:.3e}")
    assert err < 2.0 ** -16
    # the same ciphertext under the whole key: decrypt_vectors
    e.dev.load_secret_key(rio.sk_rows(r, e.s))
    re = e.dev.decrypt_vectors(out, lvl, out_scale)
    assert np.max(np.abs(re[0] - np.roll(v, 1) ** 2)) < 2.0 ** -16
    e.dev.seed_encryptor(KEY)


# ---------------------------------------------------------------- refusals
def test_calls_refuse_with_the_cause_and_launch_nothing():
    logN, q, p = rc.chain("G12")
    N = 1 << logN
    L = capi.lib()
    dev = capi.Ring(logN, q, p)
    e = env("G12")
    try:
        z8, z32, ct = np.zeros((1, N), np.int8), np.zeros((1, N), np.int32), np.zeros((1, 2, 2, N), np.uint64)
        with pytest.raises(capi.SfgError, match="no public key loaded"):
            dev.encrypt_explicit(None, 1, z8, z32, z32)
        with pytest.raises(capi.SfgError, match="no public key loaded"):
            dev.add_fresh_zero(ct, 1)
        with pytest.raises(capi.SfgError, match="no secret-key shard loaded"):
            dev.pcks_gen_share(ct, 1, z32)
        with pytest.raises(capi.SfgError, match="the encryptor has no key"):
            dev.encrypt_transcript(0, 1)
        with pytest.raises(capi.SfgError, match="no public key loaded"):
            dev.encrypt_vectors(np.zeros((1, N // 2)), 1, 2.0 ** 30)
        with pytest.raises(capi.SfgError, match="no secret key loaded"):
            dev.decrypt_vectors(ct, 1, 2.0 ** 30)
        dev.load_public_key(e.pk)
        with pytest.raises(capi.SfgError, match="the encryptor has no key .*there is no default"):
            dev.encrypt_vectors(np.zeros((1, N // 2)), 1, 2.0 ** 30)
        with pytest.raises(capi.SfgError, match="the encryptor has no key .*there is no default"):
            dev.add_fresh_zero(ct, 1)
        assert dev.encryptor_next_index() == 0
        dev.seed_encryptor(KEY)
        dev.load_secret_key(rio.sk_rows(e.ring, e.s))
        for level in (2, -1):
            with pytest.raises(capi.SfgError, match=f"level {level} out of range 0..1"):
                dev.encrypt_explicit(None, level, z8, z32, z32)
            with pytest.raises(capi.SfgError, match=f"level {level} out of range 0..1"):
                dev.pcks_finish(ct, level, ct[:, 0])
        buf = dev.to_device(ct)
        try:
            for call in (lambda n: L.sfg_ring_encrypt_explicit_dev(dev.h, None, n, 1, buf, buf, buf, buf),
                         lambda n: L.sfg_ring_ct_add_fresh_zero_dev(dev.h, buf, n, 1), lambda n: L.sfg_ring_pcks_gen_share_dev(dev.h, buf, n, 1, buf, buf, buf, buf),
                         lambda n: L.sfg_ring_pcks_finish_dev(dev.h, buf, n, 1, buf, buf)):
                assert call(-1) == 1 and "negative ciphertext count -1" in L.sfg_ring_last_error(dev.h).decode()
                assert call(0) == 0
            assert L.sfg_ring_encrypt_transcript_for_test(dev.h, 0, 0, buf, buf, buf) == 0
            assert L.sfg_ring_encrypt_transcript_for_test(dev.h, 0, -1, buf, buf, buf) == 1 and "negative ciphertext count" in L.sfg_ring_last_error(dev.h).decode()
            assert L.sfg_ring_encrypt_explicit_dev(dev.h, None, 1, 1, None, buf, buf, buf) == 1 and "null polynomial or output" in L.sfg_ring_last_error(dev.h).decode()
            assert L.sfg_ring_pcks_gen_share_dev(dev.h, buf, 1, 1, buf, None, buf, buf) == 1 and "null ciphertexts, errors or output" in L.sfg_ring_last_error(dev.h).decode()
            assert L.sfg_ring_encrypt_transcript_for_test(dev.h, (1 << 64) - 1, 2, buf, buf, buf) == 1 and "beyond 2^64" in L.sfg_ring_last_error(dev.h).decode()
            assert dev.encryptor_next_index() == 0 and not dev.to_host(buf, ct.shape).any()              # no refusal spent an index or wrote a word
        finally:
            dev.free(buf)
        assert L.sfg_ring_load_public_key(dev.h, None, 0) == 1 and L.sfg_ring_load_secret_key(dev.h, None, 0) == 1 and L.sfg_ring_seed_encryptor(dev.h, None) == 1
        for bad in (0.5, 0.0, -4.0, float("nan"), float("inf")):
            with pytest.raises(capi.SfgError, match="must be finite and at least 1"):
                dev.decode_coeffs(ct[:, 0], 1, bad)
        with pytest.raises(capi.SfgError, match="level 2 out of range 0..1"):
            dev.decode_coeffs(ct[:, 0], 2, 1.0)
        buf = dev.to_device(ct)
        out = (C.c_double * (2 * N))()
        try:
            assert L.sfg_ring_decode_coeffs(dev.h, buf, 2 * N - 1, 1, 1, 1.0, out) == 1 and "pt_stride 8191 is below" in L.sfg_ring_last_error(dev.h).decode()
            assert L.sfg_ring_decode_coeffs(dev.h, buf, 0, 1, 1, 1.0, out) == 1 and "pt_stride 0 is below" in L.sfg_ring_last_error(dev.h).decode()
            assert L.sfg_ring_decode_coeffs(dev.h, buf, 2 * N, -1, 1, 1.0, out) == 1 and "negative ciphertext count" in L.sfg_ring_last_error(dev.h).decode()
            assert L.sfg_ring_decode_coeffs(dev.h, None, 2 * N, 1, 1, 1.0, out) == 1 and "null plaintexts or output" in L.sfg_ring_last_error(dev.h).decode()
            assert L.sfg_ring_decode_coeffs(dev.h, buf, 2 * N, 0, 1, 1.0, out) == 0
        finally:
            dev.free(buf)
        vals = np.zeros((1, N // 2))
        with pytest.raises(capi.SfgError, match="must be finite and at least 1"):
            dev.decode_vectors(ct[:, 0], 1, 0.25)
        with pytest.raises(capi.SfgError, match="must be finite and at least 1"):
            dev.decrypt_vectors(ct, 1, float("nan"))
        with pytest.raises(capi.SfgError, match="must be finite and at least 1"):
            dev.encrypt_vectors(vals, 1, 0.0)
        assert dev.encryptor_next_index() == 0
        assert dev.decode_vectors(ct[:, 0], 1, 1.0).shape == (1, N // 2) and not dev.decrypt_vectors(ct, 1, 4.0).any()
        assert L.sfg_ring_encryptor_next_index(dev.h, None) == 1 and "null result pointer" in L.sfg_ring_last_error(dev.h).decode()
        assert KEY.hex() not in L.sfg_ring_last_error(dev.h).decode()
    finally:
        dev.close()
    # the hook without the switch
    saved = os.environ.pop("SFG_ENABLE_TEST_HOOKS", None)
    try:
        other = capi.Ring(logN, q, p)
    finally:
        if saved is not None:
            os.environ["SFG_ENABLE_TEST_HOOKS"] = saved
    try:
        other.seed_encryptor(KEY)
        with pytest.raises(capi.SfgError, match="test hook, enabled only"):
            other.encrypt_transcript(0, 1)
    finally:
        other.close()
