"""The general ring's collective key generation on the GPU (sfgwas_amd/csrc/gring_keygen.hip, capi.Ring): every share word of the four explicit cores against the
Python-integer statement tests/keygen_ref.py on the chains of tests/ring_cases.py, the PN14 parameters against the specialised Context, the sampled forms against
transcript + explicit core with their index accounting, the common reference polynomials against the Python map, installation against the key storage the key switch
reads, a call across the 1024-key chunk boundary, two parties end to end on two wide chains within DESIGN.md section 11's bound, and every refusal.

chain  why it is here
G12    np = 1, beta = 2                         G13   beta = 6, single-modulus digits, odd logN
W15    np = 3, ragged last digit, row > tile    W16   the largest row, ragged digit
X12    61-bit words                             L19   beta = 9, 19 moduli, beyond the oracle ring
P14    against the specialised Context

PARITY UNPINNED against lattigo's dckks / drlwe protocols, as for keygen.hip: what is pinned is the arithmetic.  One device ring and one reference ring per chain."""
import atexit
import ctypes as C
import math
from fractions import Fraction

import numpy as np
import pytest

import encrypt_ref as er
import keygen_ref as kr
import oracle_lib as ol
import ring_cases as rc
import ring_io_ref as rio
import ring_ref
from sfgwas_amd import capi

pytestmark = pytest.mark.gpu

KEY = er.TEST_KEY
CHAINS = ["G12", "G13", "W15", "W16", "X12", "L19"]
_ENV = {}


class Env:
    def __init__(self, name):
        self.name = name
        self.logN, self.q, self.p = rc.chain(name)
        self.dev = capi.Ring(self.logN, self.q, self.p)
        self.ring = ring_ref.SplitRing(self.logN, self.q, self.p) if name == "L19" else ol.Ring(self.logN, self.q, self.p)
        self.N, self.slots, self.moduli, self.top = self.ring.N, self.ring.N // 2, self.ring.moduli, len(self.q) - 1
        self.nmod, self.beta = len(self.moduli), self.dev.beta
        assert self.beta == kr.beta_of(self.ring)
        rnd = np.random.default_rng(41)
        self.s = rnd.integers(-1, 2, self.N).astype(np.int8)
        self.s2 = rnd.integers(-1, 2, self.N).astype(np.int8)                # a second party
        self.sk, self.sk2 = kr.to_u64(kr.rows_of(self.ring, self.s)), kr.to_u64(kr.rows_of(self.ring, self.s2))
        self.dev.load_secret_key_qp(self.sk)
        self.dev.seed_encryptor(KEY)

    def uniform(self, rnd, *lead):
        out = np.empty(lead + (self.nmod, self.N), dtype=np.uint64)
        for m, q in enumerate(self.moduli):
            out[..., m, :] = rnd.integers(0, q, lead + (self.N,), dtype=np.uint64)
        return out

    def errors(self, rnd, *lead):
        """error polynomials in [-19, 19]: the first has +19 at coefficient 0 and -19 at N - 1, the last is all zero (when there is more than one)"""
        e = rnd.integers(-19, 20, lead + (self.N,)).astype(np.int32)
        flat = e.reshape(-1, self.N)
        flat[0, 0], flat[0, -1] = 19, -19
        if flat.shape[0] > 1:
            flat[-1] = 0
        return e

    def galois_set(self):
        N = self.N
        g = [self.ring.galois(1), self.ring.galois(self.slots // 2), 2 * N - 1, 1]      # g^-1 != g; g^-1 = g twice; the identity
        assert kr.galois_inverse(g[0], N) != g[0] and kr.galois_inverse(g[1], N) == g[1] and kr.galois_inverse(g[2], N) == g[2]
        return g

    def agg(self, *shares):
        mods = np.array(self.moduli, dtype=np.uint64).reshape(self.nmod, 1)
        acc = shares[0]
        for s in shares[1:]:
            acc = (acc + s) % mods                                         # words below 2^61: the sum fits 64 bits
        return acc


def env(name):
    if name not in _ENV:
        _ENV[name] = Env(name)
    return _ENV[name]


@atexit.register
def _close_all():
    for e in _ENV.values():
        e.dev.close()
    _ENV.clear()


def canonical(e, rows):
    return all(int(rows[..., m, :].max()) < q for m, q in enumerate(e.moduli))


# ---------------------------------------------------------------- explicit cores, word for word
@pytest.mark.parametrize("name", CHAINS)
def test_public_key_share_every_word(name):
    e = env(name)
    rnd = np.random.default_rng(1)
    crp = e.uniform(rnd)
    directed = np.zeros(e.N, np.int32)
    directed[0::4], directed[1::4], directed[2::4] = 2 ** 31 - 1, -(2 ** 31 - 1), -2 ** 31      # and 0 at 3 mod 4
    for err in (e.errors(rnd), directed):
        got = e.dev.ckg_gen_share(crp, err)
        assert np.array_equal(got, kr.to_u64(kr.ckg_share(e.ring, e.s, crp, err))), name
        assert canonical(e, got)


@pytest.mark.parametrize("name", CHAINS)
def test_rotation_key_shares_every_word(name):
    """four Galois elements in one call (rotation by 1, by slots / 2, the conjugate, g = 1); one element on the two wide chains, whose references are slow"""
    e = env(name)
    rnd = np.random.default_rng(2)
    gs = e.galois_set() if name not in ("W15", "W16") else [e.ring.galois(1)]
    crp = e.uniform(rnd, len(gs), e.beta)
    err = e.errors(rnd, len(gs), e.beta)
    got = e.dev.rtg_gen_shares(gs, crp, err)
    assert got.shape == (len(gs), e.beta, e.nmod, e.N) and canonical(e, got)
    for k, g in enumerate(gs):
        assert np.array_equal(got[k], kr.to_u64(kr.rtg_share(e.ring, e.s, g, crp[k], err[k]))), (name, k, g)


@pytest.mark.parametrize("name", CHAINS)
def test_relinearisation_rounds_every_word(name):
    """round 1 word for word; round 2 on the aggregates of two parties (the second party's round-1 shares are made by the same ring under its own key); on G12 a
    second round-2 case with e2 = e3 = 2^31 - 1 everywhere: their sum leaves int32"""
    e = env(name)
    rnd = np.random.default_rng(3)
    crp = e.uniform(rnd, e.beta)
    u = rnd.integers(-1, 2, e.N).astype(np.int8)
    e0, e1, e2, e3 = (e.errors(rnd, e.beta) for _ in range(4))
    h0, h1 = e.dev.rkg_round1(crp, u, e0, e1)
    w0, w1 = kr.rkg_round1(e.ring, e.s, crp, u, e0, e1)
    assert np.array_equal(h0, kr.to_u64(w0)) and np.array_equal(h1, kr.to_u64(w1)), name
    try:
        e.dev.load_secret_key_qp(e.sk2)
        o0, o1 = e.dev.rkg_round1(crp, rnd.integers(-1, 2, e.N).astype(np.int8), e1, e0)
    finally:
        e.dev.load_secret_key_qp(e.sk)
    H0, H1 = e.agg(h0, o0), e.agg(h1, o1)
    cases = [(e2, e3)] + ([(np.full((e.beta, e.N), 2 ** 31 - 1, np.int32),) * 2] if name == "G12" else [])
    for a, b in cases:
        got = e.dev.rkg_round2(H0, H1, u, a, b)
        assert np.array_equal(got, kr.to_u64(kr.rkg_round2(e.ring, e.s, H0, H1, u, a, b))), name
        assert canonical(e, got)


# ---------------------------------------------------------------- P14 against the specialised context
def take(d):
    out = d.host(); d.free()
    return out


def test_p14_equals_the_specialised_context_word_for_word():
    e = env("P14")
    ctx = capi.Context(e.q, e.p)
    try:
        ctx.load_secret_key_qp(e.sk)
        rnd = np.random.default_rng(14)
        crp, err = e.uniform(rnd), e.errors(rnd)
        assert np.array_equal(e.dev.ckg_gen_share(crp, err), take(ctx.ckg_gen_share(crp, err)))
        gs = e.galois_set()
        crp, err = e.uniform(rnd, len(gs), e.beta), e.errors(rnd, len(gs), e.beta)
        assert np.array_equal(e.dev.rtg_gen_shares(gs, crp, err), take(ctx.rtg_gen_shares(gs, crp, err)))
        crp, u = e.uniform(rnd, e.beta), rnd.integers(-1, 2, e.N).astype(np.int8)
        e0, e1 = e.errors(rnd, e.beta), e.errors(rnd, e.beta)
        h0, h1 = e.dev.rkg_round1(crp, u, e0, e1)
        c0, c1 = (take(d) for d in ctx.rkg_round1(crp, u, e0, e1))
        assert np.array_equal(h0, c0) and np.array_equal(h1, c1)
        H0, H1 = e.uniform(rnd, e.beta), e.uniform(rnd, e.beta)
        assert np.array_equal(e.dev.rkg_round2(H0, H1, u, e0, e1), take(ctx.rkg_round2(H0, H1, u, e0, e1)))
        # the common reference polynomials: the same words, an offset row range included
        idx = list(range(e.nmod)) + [0, e.nmod - 1]
        for first in (0, (1 << 32) + 5):
            assert np.array_equal(e.dev.crp_fill(CRP_SEED, first, idx), take(ctx.crp_fill(CRP_SEED, first, idx)))
        # the sampled forms under the same sampler key from the same indices
        ctx.seed_encryptor(KEY); e.dev.seed_encryptor(KEY)
        crp1, crpk, crpb = e.uniform(rnd), e.uniform(rnd, 2, e.beta), e.uniform(rnd, e.beta)
        d, f = ctx.ckg_gen_share(crp1)
        got, gf = e.dev.ckg_gen_share(crp1, sampled=True)
        assert f == gf == 0 and np.array_equal(got, take(d))
        d, f = ctx.rtg_gen_shares(gs[:2], crpk)
        got, gf = e.dev.rtg_gen_shares(gs[:2], crpk, sampled=True)
        assert f == gf == 1 and np.array_equal(got, take(d))
        c0, c1, f, cu = ctx.rkg_round1(crpb)
        h0, h1, gf, gu = e.dev.rkg_round1(crpb, sampled=True)
        assert (f, cu) == (gf, gu) == (1 + 2 * e.beta, 1 + 3 * e.beta) and np.array_equal(h0, take(c0)) and np.array_equal(h1, take(c1))
        d, f = ctx.rkg_round2(H0, H1, u_index=cu)
        got, gf = e.dev.rkg_round2(H0, H1, u_index=gu, sampled=True)
        assert f == gf == 2 + 3 * e.beta and np.array_equal(got, take(d))
        assert ctx.encryptor_next_index() == e.dev.encryptor_next_index() == 2 + 4 * e.beta
    finally:
        ctx.close()
        e.dev.seed_encryptor(KEY)


# ---------------------------------------------------------------- sampled forms
@pytest.mark.parametrize("name", ["G12", "W16"])
def test_sampled_forms_are_transcript_plus_core_and_count_their_indices(name):
    e = env(name)
    dev, beta, N = e.dev, e.beta, e.N
    dev.seed_encryptor(KEY)
    assert dev.encryptor_next_index() == 0
    rnd = np.random.default_rng(4)
    nxt = 0
    crp = e.uniform(rnd)                                                    # public key share: 1 index, e = polynomial id 1
    got, first = dev.ckg_gen_share(crp, sampled=True)
    assert first == nxt and dev.encryptor_next_index() == nxt + 1
    _, err, _ = dev.encrypt_transcript(first, 1)
    assert np.array_equal(got, dev.ckg_gen_share(crp, err[0]))
    nxt += 1
    gs = e.galois_set()[:2]                                                  # rotation shares: nkeys * beta indices, (k, i) takes first + k beta + i
    crp = e.uniform(rnd, 2, beta)
    got, first = dev.rtg_gen_shares(gs, crp, sampled=True)
    assert first == nxt and dev.encryptor_next_index() == nxt + 2 * beta
    _, err, _ = dev.encrypt_transcript(first, 2 * beta)
    assert np.array_equal(got, dev.rtg_gen_shares(gs, crp, err.reshape(2, beta, N)))
    nxt += 2 * beta
    crp = e.uniform(rnd, beta)                                              # round 1: beta + 1 indices, the last one is u's
    h0, h1, first, ui = dev.rkg_round1(crp, sampled=True)
    assert first == nxt and ui == nxt + beta and dev.encryptor_next_index() == nxt + beta + 1
    _, e0, e1 = dev.encrypt_transcript(first, beta)
    u, _, _ = dev.encrypt_transcript(ui, 1)
    x0, x1 = dev.rkg_round1(crp, u[0], e0, e1)
    assert np.array_equal(h0, x0) and np.array_equal(h1, x1)
    nxt += beta + 1
    H0, H1 = e.uniform(rnd, beta), e.uniform(rnd, beta)                     # round 2: beta fresh indices; u redrawn from its index
    got, first = dev.rkg_round2(H0, H1, u_index=ui, sampled=True)
    assert first == nxt and dev.encryptor_next_index() == nxt + beta
    _, e2, e3 = dev.encrypt_transcript(first, beta)
    assert np.array_equal(got, dev.rkg_round2(H0, H1, u[0], e2, e3))
    nxt += beta
    with pytest.raises(capi.SfgError, match="not an odd number below 2N"):  # a refused call leaves the counter where it was
        dev.rtg_gen_shares([4], crp[None], sampled=True)
    assert dev.encryptor_next_index() == nxt


# ---------------------------------------------------------------- common reference polynomials
def _pick_crp_seed():
    """a seed under which the REFERENCE needs a second try for some coefficient of the PN14 rows below (its moduli sit just above a power of two; the other chains'
    sit just below one and practically never retry).  Decided here on the CPU from keygen_ref alone."""
    _, q, p = rc.chain("P14")
    for c in range(7, 40):
        seed = bytes(range(c, c + 32))
        if any(int((kr.crp_row(seed, m, mod, 1 << 14, want_tries=True)[1] > 0).sum()) for m, mod in enumerate(q + p)):
            return seed
    raise AssertionError("no seed with a retry")


CRP_SEED = bytes(range(7, 39))


@pytest.mark.parametrize("name", ["G12", "W16", "X12", "P14"])
def test_crp_fill_every_modulus_and_an_offset_row_range(name):
    e = env(name)
    seed = _pick_crp_seed() if name == "P14" else CRP_SEED
    idx = list(range(e.nmod))
    got = e.dev.crp_fill(seed, 0, idx)
    retried = 0
    for m in idx:
        want, tries = kr.crp_row(seed, m, e.moduli[m], e.N, want_tries=True)
        assert np.array_equal(got[m], want), (name, m)
        assert int(got[m].max()) < e.moduli[m]
        retried += int((tries > 0).sum())
    if name == "P14":
        assert retried > 0                                                  # the t + 1 path ran on the device, on coefficients the reference names
    first = (1 << 32) + 5
    idx2 = idx[::-1] + [0]
    assert np.array_equal(e.dev.crp_fill(seed, first, idx2), kr.crp_rows(seed, first, idx2, e.moduli, e.N)), name
    assert np.array_equal(e.dev.crp_fill(seed, 2, idx[2:]), got[2:])          # a row is a function of (seed, global row number, modulus) alone


# ---------------------------------------------------------------- installation
def orc_mulrelin(ring, level, a, b, rlk):
    want = np.zeros_like(a)
    ol.lib().orc_mulrelin(ring.h, level, ol.p64(np.ascontiguousarray(a)), ol.p64(np.ascontiguousarray(b)), ol.p64(np.ascontiguousarray(rlk)), ol.p64(want))
    return want


@pytest.mark.parametrize("name", ["G12", "W15", "L19"])
def test_installed_keys_are_exported_exactly_and_switch_as_the_reference_does(name):
    e = env(name)
    dev, ring, beta, N = e.dev, e.ring, e.beta, e.N
    rnd = np.random.default_rng(6)
    k, level = 3, e.top
    gs = [ring.galois(e.slots - k), 2 * N - 1]
    agg = e.uniform(rnd, 2, beta)
    crp_dev = dev.crp_fill(CRP_SEED, 100, [m for _ in range(2 * beta) for m in range(e.nmod)], keep=True)
    try:
        crp = dev.to_host(crp_dev, (2, beta, e.nmod, N))
        assert not dev.has_rotkey(gs[0]) and not dev.has_rotkey(gs[1])
        with pytest.raises(capi.SfgError, match="not an odd number below 2N"):
            dev.install_rotkeys([gs[0], 6], agg, crp_dev)
        assert not dev.has_rotkey(gs[0]) and not dev.has_rotkey(6)             # nothing of a refused call is installed
        with pytest.raises(capi.SfgError, match="no key for galois element"):
            dev.export_rotkey(gs[0])
        dev.install_rotkeys(gs, agg, crp_dev)                                 # crp straight from device memory
        assert dev.has_rotkey(gs[0]) and dev.has_rotkey(gs[1])
    finally:
        dev.free(crp_dev)
    for i, g in enumerate(gs):
        key = dev.export_rotkey(g)
        assert np.array_equal(key[:, 0], agg[i]) and np.array_equal(key[:, 1], crp[i]), (name, g)
    key = dev.export_rotkey(gs[0])
    ct = np.stack([e.uniform(rnd)[:level + 1] for _ in range(2)])
    got = dev.rotate_right(ct[None], level, [k])[0]
    if name == "L19":
        want = ring_ref.rotate_model(ring, level, ct, gs[0], key)
    else:
        keys = ol.RotKeys(ring)
        keys.add(gs[0], key)
        want = ol.rotate_left(ring, keys, level, ct, e.slots - k)
    assert np.array_equal(got, want), name
    # the relinearisation key lives under Galois element 1
    dev.install_relinkey(agg[1], crp[1])
    rlk = dev.export_rotkey(1)
    assert np.array_equal(rlk[:, 0], agg[1]) and np.array_equal(rlk[:, 1], crp[1])
    lvl = 2 if name == "L19" else level
    a, b = (np.stack([e.uniform(rnd)[:lvl + 1] for _ in range(2)]) for _ in range(2))
    got = dev.mulrelin(a[None], b[None], lvl)[0]
    if name != "W15":                                                       # the Python-integer model walks every coefficient: too slow at N = 32768, where the oracle stands in
        assert np.array_equal(got, ring_ref.mulrelin_model(ring, lvl, a, b, rlk)), name
    if name != "L19":
        assert np.array_equal(got, orc_mulrelin(ring, lvl, a, b, rlk)), name
    # the public key is (agg, crp): it encrypts as the big-integer statement does under that pair
    dev.install_public_key(agg[0, 0], crp[0, 0])
    assert dev.has_public_key()
    u, e0, e1 = rnd.integers(-1, 2, (1, N)).astype(np.int8), e.errors(rnd, 1), e.errors(rnd, 1)
    lvl = min(level, 1)
    want = rio.ct_rows(er.encrypt_bigint(ring, lvl, np.stack([agg[0, 0], crp[0, 0]]), u[0], e0[0], e1[0]), lvl)
    assert np.array_equal(dev.encrypt_explicit(None, lvl, u, e0, e1)[0], want), name


def test_secret_key_qp_alone_serves_the_shares_and_the_decryption():
    logN, q, p = rc.chain("G12")
    e = env("G12")
    rnd = np.random.default_rng(9)
    a, b = capi.Ring(logN, q, p), capi.Ring(logN, q, p)
    try:
        a.load_secret_key(e.sk[:len(q)])
        b.load_secret_key_qp(e.sk)
        cts = np.stack([e.uniform(rnd)[:2] for _ in range(2)])[None]
        e0 = e.errors(rnd, 1)
        assert np.array_equal(a.pcks_gen_share(cts, 1, e0)[0], b.pcks_gen_share(cts, 1, e0)[0])
        assert np.array_equal(a.decrypt_vectors(cts, 1, 2.0 ** 30), b.decrypt_vectors(cts, 1, 2.0 ** 30))
        mont = np.stack([np.array([(int(x) << 64) % m for x in e.sk[i]], dtype=np.uint64) for i, m in enumerate(e.moduli)])
        b.load_secret_key_qp(mont, montgomery=True)
        crp, err = e.uniform(rnd), e.errors(rnd)
        assert np.array_equal(b.ckg_gen_share(crp, err), e.dev.ckg_gen_share(crp, err))
    finally:
        a.close(); b.close()


# ---------------------------------------------------------------- the chunk boundary
def test_1025_rotation_keys_cross_the_chunk_boundary():
    """1025 keys on G12 (197 MiB of shares and as much crp, filled on the device), Galois elements repeating: the one call equals the concatenation of calls of at
    most 256 keys drawing the same indices, and keys 0, 1023 and 1024 equal the reference on the transcript's errors"""
    e = env("G12")
    dev, beta, N, nk = e.dev, e.beta, e.N, 1025
    gs = (e.galois_set() * 257)[:nk]
    per = beta * e.nmod * N
    crp = dev.crp_fill(CRP_SEED, 0, [m for _ in range(nk * beta) for m in range(e.nmod)], keep=True)
    one, parts = dev.malloc(nk * per * 8), dev.malloc(nk * per * 8)
    try:
        dev.seed_encryptor(KEY)
        _, first = dev.rtg_gen_shares(gs, crp, sampled=True, out=[one])
        assert first == 0 and dev.encryptor_next_index() == nk * beta
        dev.seed_encryptor(KEY)
        for k0 in range(0, nk, 256):
            n = min(256, nk - k0)
            _, first = dev.rtg_gen_shares(gs[k0:k0 + n], C.c_void_p(crp.value + k0 * per * 8), sampled=True, out=[C.c_void_p(parts.value + k0 * per * 8)])
            assert first == k0 * beta
        got = dev.to_host(one, (nk, beta, e.nmod, N))
        assert np.array_equal(got, dev.to_host(parts, (nk, beta, e.nmod, N)))
        for k in (0, 1023, 1024):
            c = dev.to_host(C.c_void_p(crp.value + k * per * 8), (beta, e.nmod, N))
            _, err, _ = dev.encrypt_transcript(k * beta, beta)
            assert np.array_equal(got[k], kr.to_u64(kr.rtg_share(e.ring, e.s, gs[k], c, err))), k
    finally:
        for d in (crp, one, parts):
            dev.free(d)
        dev.seed_encryptor(KEY)


# ---------------------------------------------------------------- two parties end to end, wholly on the device
NPARTY, EB, EB_PCKS = 2, 19, 38


def derived_bound(q, p, level, scale, vmax, N):
    """DESIGN.md section 11 in slot units, exactly, for this chain's digits D_i, P, N, n = 2 parties, the scale and v_max, along encrypt -> rotate -> square ->
    rescale -> two-party decryption.  |S| <= n per coefficient, ||S||_1 <= n N, aggregated errors <= 19 n; a key-switch digit |d_i| < 2 D_i; every ModDown leaves a
    polynomial off by < 2 (together 2 + 2 ||S||_1), a rescale by <= 1; a coefficient error c moves a slot by at most N c / scale.
      eps_enc = N ((19 n N + 19 + 19 n N) / P + 2 + 2 n N + 1) / scale
      eps_rot = eps_enc + N (sum_i N 2 D_i 19 n / P + 2 + 2 n N) / scale
      eps_sq  = 2 v_max eps_rot + eps_rot^2 + N (sum_i N 2 D_i F / P + 2 + 2 n N) / scale^2 + N (1 + n N) q_l / scale^2,   F = 2 N n^2 19 + 2 19 n
      the decryption's shares: each party adds ModDown_P(e), |e| <= 38: (38 / P + 2) per coefficient and party, at the output scale scale^2 / q_l"""
    n, P, nl = NPARTY, math.prod(p), level + 1
    s1 = n * N
    digits = [math.prod(q[i:min(i + len(p), nl)]) for i in range(0, nl, len(p))]
    md = 2 + 2 * s1
    sc = Fraction(scale)
    eps_enc = N * (Fraction(n * EB * N + EB + EB * s1, P) + md + 1) / sc
    eps_rot = eps_enc + N * (Fraction(sum(N * 2 * d * n * EB for d in digits), P) + md) / sc
    F = 2 * N * n * n * EB + 2 * n * EB
    eps_sq = 2 * Fraction(vmax) * eps_rot + eps_rot ** 2 + N * (Fraction(sum(N * 2 * d * F for d in digits), P) + md) / sc ** 2 + N * (1 + s1) * q[level] / sc ** 2
    return eps_sq + N * n * (Fraction(EB_PCKS, P) + 2) / (sc ** 2 / q[level])


@pytest.mark.parametrize("name,scale", [("W15", 2.0 ** 40), ("W16", 2.0 ** 45)])
def test_end_to_end_two_parties_keys_made_on_the_device(name, scale):
    e = env(name)
    dev, ring, beta, N, nmod, top, vmax = e.dev, e.ring, e.beta, e.N, e.nmod, e.top, 1.0
    rnd = np.random.default_rng(2024)
    shares = rio.split_secret(e.s, 11)
    sks = [kr.to_u64(kr.rows_of(ring, sh)) for sh in shares]
    g = ring.galois(e.slots - 1)
    key_rows = [m for _ in range(beta) for m in range(nmod)]
    spans = ((0, list(range(nmod))), (nmod, key_rows), (nmod * (1 + beta), key_rows))
    parties = [capi.Ring(e.logN, e.q, e.p) for _ in sks]                      # each party: its key shard, its own sampler key, its own expansion of the seed
    crp_pk, crp_rl, crp_rt = (dev.crp_fill(CRP_SEED, f, rows, keep=True) for f, rows in spans)
    crp_bad = dev.crp_fill(CRP_SEED, nmod * (1 + beta), key_rows, keep=True)
    try:
        dev.check(capi.lib().sfg_ring_crp_fill_dev(dev.h, CRP_SEED, 1 << 40, 1, (C.c_int * 1)(0), crp_bad), "crp_fill")      # ONE wrong row: digit 0, modulus 0
        pk, rt, r1, r2 = [], [], [], []
        for i, (party, sk) in enumerate(zip(parties, sks)):
            party.load_secret_key_qp(sk)
            party.seed_encryptor(bytes([i + 1]) * 32)
            c_pk, c_rl, c_rt = (party.crp_fill(CRP_SEED, f, rows, keep=True) for f, rows in spans)      # stays in device memory
            pk.append(party.ckg_gen_share(c_pk, sampled=True)[0])
            rt.append(party.rtg_gen_shares([g], c_rt, sampled=True)[0][0])
            r1.append(party.rkg_round1(c_rl, sampled=True))
            for d in (c_pk, c_rl, c_rt):
                party.free(d)
        H0, H1 = e.agg(*[x[0] for x in r1]), e.agg(*[x[1] for x in r1])
        for i, party in enumerate(parties):
            r2.append(party.rkg_round2(H0, H1, u_index=r1[i][3], sampled=True)[0])
        dev.install_public_key(e.agg(*pk), crp_pk)
        dev.install_rotkeys([g], e.agg(*rt)[None], crp_rt)
        dev.install_relinkey(e.agg(*r2), H1)
        dev.seed_encryptor(bytes([9]) * 32)
        v = rnd.uniform(-vmax, vmax, e.slots)
        ct = dev.encrypt_vectors(v[None], top, scale)
        lvl, out_scale = top - 1, scale * scale / e.q[top]

        def decrypt(ct_in):
            rot = dev.rotate_right(ct_in, top, [1])
            out = dev.rescale(dev.mulrelin(rot, rot, top), top)
            acc = None
            for party in parties:
                h0, _ = party.pcks_gen_share(out, lvl, rnd.integers(-EB_PCKS, EB_PCKS + 1, (1, N)).astype(np.int32))
                acc = h0 if acc is None else (acc + h0) % np.array(e.q[:lvl + 1], dtype=np.uint64).reshape(1, lvl + 1, 1)
            re, im = dev.decode_vectors(dev.pcks_finish(out, lvl, acc), lvl, out_scale, want_imag=True)
            return max(np.max(np.abs(re[0] - np.roll(v, 1) ** 2)), np.max(np.abs(im[0])))

        bound = derived_bound(e.q, e.p, top, scale, vmax, N)
        err = decrypt(ct)
        print(f"{name}: rotate, square, rescale under collectively generated keys: max slot error {err:.3e}, derived bound {float(bound):.3e}")
        dev.install_rotkeys([g], e.agg(*rt)[None], crp_bad)
        err_bad = decrypt(ct)
        print(f"{name}: the same under a rotation key installed with one wrong crp row: {err_bad:.3e}")
        assert float(bound) < 0.25                                          # it means something against squares up to 1
        assert Fraction(err) <= bound
        assert Fraction(err_bad) > bound
    finally:
        for d in (crp_pk, crp_rl, crp_rt, crp_bad):
            dev.free(d)
        for party in parties:
            party.close()
        dev.seed_encryptor(KEY)


# ---------------------------------------------------------------- refusals
def test_refusals_give_their_message_and_launch_nothing():
    logN, q, p = rc.chain("G12")
    N, nmod, beta = 1 << logN, 3, 2
    L = capi.lib()
    dev = capi.Ring(logN, q, p)
    err = lambda: L.sfg_ring_last_error(dev.h).decode()                       # noqa: E731
    try:
        sentinel = np.full((2 * beta * nmod, N), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
        out = dev.to_device(sentinel)
        z, zi, zu = dev.to_device(np.zeros((2 * beta * nmod, N), np.uint64)), dev.to_device(np.zeros((2 * beta, N), np.int32)), dev.to_device(np.zeros(N, np.int8))
        g1 = (C.c_uint64 * 1)(5)
        first, ui = C.c_uint64(), C.c_uint64()
        calls = [lambda: L.sfg_ring_ckg_gen_share_dev(dev.h, z, zi, out),
                 lambda: L.sfg_ring_rtg_gen_shares_dev(dev.h, g1, 1, z, zi, out),
                 lambda: L.sfg_ring_rkg_round1_dev(dev.h, z, zu, zi, zi, out, out),
                 lambda: L.sfg_ring_rkg_round2_dev(dev.h, z, z, zu, zi, zi, out)]
        sampled = [lambda: L.sfg_ring_ckg_gen_share_sampled_dev(dev.h, z, out, C.byref(first)),
                   lambda: L.sfg_ring_rtg_gen_shares_sampled_dev(dev.h, g1, 1, z, out, C.byref(first)),
                   lambda: L.sfg_ring_rkg_round1_sampled_dev(dev.h, z, out, out, C.byref(first), C.byref(ui)),
                   lambda: L.sfg_ring_rkg_round2_sampled_dev(dev.h, z, z, 0, out, C.byref(first))]
        dev.seed_encryptor(KEY)
        for f in calls + sampled:                                            # no secret key over QP
            assert f() == 1 and "no secret key over QP loaded" in err()
        assert dev.encryptor_next_index() == 0
        rnd = np.random.default_rng(8)
        dev.load_secret_key_qp(np.stack([rnd.integers(0, m, N, dtype=np.uint64) for m in q + p]))
        bare = capi.Ring(logN, q, p)                                          # a secret key but no sampler key
        try:
            bare.load_secret_key_qp(np.zeros((nmod, N), np.uint64))
            for fn in (lambda: L.sfg_ring_ckg_gen_share_sampled_dev(bare.h, z, out, None), lambda: L.sfg_ring_rtg_gen_shares_sampled_dev(bare.h, g1, 1, z, out, None),
                       lambda: L.sfg_ring_rkg_round1_sampled_dev(bare.h, z, out, out, None, C.byref(ui)), lambda: L.sfg_ring_rkg_round2_sampled_dev(bare.h, z, z, 0, out, None)):
                assert fn() == 1 and "the encryptor has no key" in L.sfg_ring_last_error(bare.h).decode()
        finally:
            bare.close()
        # null arguments
        assert L.sfg_ring_load_secret_key_qp(dev.h, None, 0) == 1 and "null key" in err()
        assert L.sfg_ring_ckg_gen_share_dev(dev.h, z, None, out) == 1 and "null polynomial or output" in err()
        assert L.sfg_ring_ckg_gen_share_sampled_dev(dev.h, None, out, None) == 1 and "null polynomial or output" in err()
        assert L.sfg_ring_rtg_gen_shares_dev(dev.h, g1, 1, None, zi, out) == 1 and "null polynomial or output" in err()
        assert L.sfg_ring_rtg_gen_shares_dev(dev.h, None, 1, z, zi, out) == 1 and "null Galois elements" in err()
        assert L.sfg_ring_rkg_round1_dev(dev.h, z, None, zi, zi, out, out) == 1 and "null polynomial or output" in err()
        assert L.sfg_ring_rkg_round1_sampled_dev(dev.h, z, out, out, C.byref(first), None) == 1 and "u_index" in err()
        assert L.sfg_ring_rkg_round2_dev(dev.h, z, None, zu, zi, zi, out) == 1 and "null polynomial or output" in err()
        assert L.sfg_ring_install_public_key_dev(dev.h, None, z) == 1 and "null polynomial" in err()
        assert L.sfg_ring_install_rotkeys_dev(dev.h, g1, 1, z, None) == 1 and "null polynomial" in err()
        assert L.sfg_ring_install_relinkey_dev(dev.h, z, None) == 1 and "null polynomial" in err()
        assert L.sfg_ring_export_rotkey(dev.h, 5, None) == 1 and "null output" in err()
        assert L.sfg_ring_crp_fill_dev(dev.h, None, 0, 1, (C.c_int * 1)(0), out) == 1 and "null key, modulus indices or output" in err()
        # Galois elements and key counts
        even, big = (C.c_uint64 * 2)(5, 6), (C.c_uint64 * 1)(2 * N + 1)
        for gal, n in ((even, 2), (big, 1)):
            assert L.sfg_ring_rtg_gen_shares_dev(dev.h, gal, n, z, zi, out) == 1 and "not an odd number below 2N" in err()
            assert L.sfg_ring_rtg_gen_shares_sampled_dev(dev.h, gal, n, z, out, C.byref(first)) == 1 and "not an odd number below 2N" in err()
            assert L.sfg_ring_install_rotkeys_dev(dev.h, gal, n, z, z) == 1 and "not an odd number below 2N" in err()
        assert not dev.has_rotkey(5) and not dev.has_rotkey(6)
        for fn in (lambda n: L.sfg_ring_rtg_gen_shares_dev(dev.h, g1, n, z, zi, out), lambda n: L.sfg_ring_rtg_gen_shares_sampled_dev(dev.h, g1, n, z, out, C.byref(first)),
                   lambda n: L.sfg_ring_install_rotkeys_dev(dev.h, g1, n, z, z)):
            assert fn(-1) == 1 and "negative key count -1" in err()
            assert fn(0) == 0
        # modulus indices, empty calls, exports
        for bad in (nmod, -1):
            assert L.sfg_ring_crp_fill_dev(dev.h, CRP_SEED, 0, 1, (C.c_int * 1)(bad), out) == 1 and "out of range 0..2" in err()
        assert L.sfg_ring_crp_fill_dev(dev.h, CRP_SEED, 0, 0, None, None) == 0
        host = np.zeros((beta, 2, nmod, N), np.uint64)
        for g in (1, 5):
            assert L.sfg_ring_export_rotkey(dev.h, g, capi.p64(host)) == 1 and f"no key for galois element {g}" in err()
        assert dev.encryptor_next_index() == 0 and not dev.has_rotkey(5) and not dev.has_public_key()
        dev.sync()
        assert np.array_equal(dev.to_host(out, sentinel.shape), sentinel)      # nothing was launched on the outputs
        assert KEY.hex() not in err()
        for d in (out, z, zi, zu):
            dev.free(d)
    finally:
        dev.close()
