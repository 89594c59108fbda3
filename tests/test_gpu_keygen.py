"""Collective key generation on the device (sfgwas_amd/csrc/keygen.hip): every word of the explicit cores against the Python-integer statement tests/keygen_ref.py
(itself pinned by tests/test_keygen_ref.py), the sampled forms against the explicit cores on the sampler's transcript, the common reference polynomials against the
Python map, installation against the key storage the key switch reads, keys made here carrying a ciphertext through a rotation and a squaring within the noise
bound DESIGN.md section 11 derives, and the refusals.  Two contexts: the PN14 chain (beta = 5) and nq = 3, np = 2 (beta = 2, the last digit holds ONE modulus).

PARITY UNPINNED against lattigo's dckks / drlwe protocols (no Go toolchain; fresh randomness excludes bit parity anyway): what is pinned is the arithmetic."""
import ctypes as C
import math
from fractions import Fraction

import numpy as np
import pytest

import encrypt_ref as er
import keygen_ref as kr
import oracle_lib as ol

pytestmark = pytest.mark.gpu
N, SLOTS = 1 << 14, 1 << 13
KEY = er.TEST_KEY
CRP_SEED = bytes(range(7, 39))
SHAPES = {"pn14": (ol.Q_PN14, ol.P_PN14), "q3p2": (ol.Q_PN14[1:4], ol.P_PN14)}        # q3p2: digits {q0, q1}, {q2}


class Env:
    def __init__(self, name):
        from sfgwas_amd import capi
        q, p = SHAPES[name]
        self.ring = ol.Ring(14, q, p)
        self.ctx = capi.Context(q, p)
        self.nmod, self.beta = len(q) + len(p), self.ctx.beta
        assert self.beta == kr.beta_of(self.ring) == self.ring.beta
        rnd = np.random.default_rng(41)
        self.s = rnd.integers(-1, 2, N).astype(np.int8)
        self.sk = kr.to_u64(kr.rows_of(self.ring, self.s))
        self.ctx.load_secret_key_qp(self.sk)
        self.ctx.seed_encryptor(KEY)

    def uniform(self, rnd, *lead):
        out = np.empty(lead + (self.nmod, N), dtype=np.uint64)
        for m, q in enumerate(self.ring.moduli):
            out[..., m, :] = rnd.integers(0, q, lead + (N,), dtype=np.uint64)
        return out


@pytest.fixture(scope="module", params=["pn14", "q3p2"])
def env(request):
    e = Env(request.param)
    yield e
    e.ctx.close()


def errors(rnd, *lead):
    """error polynomials in [-19, 19]: the first has +19 at coefficient 0 and -19 at N - 1, the last is all zero (when there is more than one)"""
    e = rnd.integers(-19, 20, lead + (N,)).astype(np.int32)
    flat = e.reshape(-1, N)
    flat[0, 0], flat[0, N - 1] = 19, -19
    if flat.shape[0] > 1:
        flat[-1] = 0
    if flat.shape[0] > 2:
        flat[1, 0], flat[1, N - 1] = -19, 19
    return e


def take(d):
    out = d.host(); d.free()
    return out


def galois_set(ring):
    g = [ring.galois(1), ring.galois(SLOTS // 2), 2 * N - 1]          # g^-1 != g;  rotation by slots / 2 and the conjugate: g^-1 = g
    assert kr.galois_inverse(g[0], N) != g[0] and kr.galois_inverse(g[1], N) == g[1] and kr.galois_inverse(g[2], N) == g[2]
    return g


# ---------------------------------------------------------------- explicit cores
def test_secret_key_qp_also_provides_the_q_rows(env):
    """a ciphertext (0, 1) decrypts to sk itself: the Q rows sfg_ctx_load_secret_key would have stored"""
    lvl = env.ring.nq - 1
    ct = np.zeros((1, 2, lvl + 1, N), dtype=np.uint64); ct[0, 1] = 1
    h0, _ = env.ctx.pcks_gen_share(ct, lvl, np.zeros((1, N), np.int32))
    assert np.array_equal(h0[0], env.sk[:lvl + 1])


def test_public_key_share_every_word(env):
    rnd = np.random.default_rng(1)
    crp = env.uniform(rnd)
    for e in (errors(rnd), np.zeros(N, np.int32)):
        got = take(env.ctx.ckg_gen_share(crp, e))
        assert np.array_equal(got, kr.to_u64(kr.ckg_share(env.ring, env.s, crp, e)))
        assert all(got[m].max() < q for m, q in enumerate(env.ring.moduli))


def test_rotation_key_shares_every_word(env):
    rnd = np.random.default_rng(2)
    gs = galois_set(env.ring)
    crp = env.uniform(rnd, len(gs), env.beta)
    e = errors(rnd, len(gs), env.beta)
    got = take(env.ctx.rtg_gen_shares(gs, crp, e))
    assert got.shape == (len(gs), env.beta, env.nmod, N)
    for k, g in enumerate(gs):
        want = kr.to_u64(kr.rtg_share(env.ring, env.s, g, crp[k], e[k]))
        assert np.array_equal(got[k], want), (k, g)
    if env.ring.np_ == 2 and env.ring.nq == 3:                         # the ragged shape: digit 1 holds modulus 2 alone, and the reference says so
        assert [[kr.g_term(env.ring, i, m) != 0 for m in range(5)] for i in range(2)] == [[True, True, False, False, False], [False, False, True, False, False]]


def test_relinearisation_rounds_every_word(env):
    rnd = np.random.default_rng(3)
    crp = env.uniform(rnd, env.beta)
    for u in (rnd.integers(-1, 2, N).astype(np.int8), np.zeros(N, np.int8)):
        e0, e1, e2, e3 = (errors(rnd, env.beta) for _ in range(4))
        h0, h1 = (take(d) for d in env.ctx.rkg_round1(crp, u, e0, e1))
        w0, w1 = kr.rkg_round1(env.ring, env.s, crp, u, e0, e1)
        assert np.array_equal(h0, kr.to_u64(w0)) and np.array_equal(h1, kr.to_u64(w1))
        H0, H1 = env.uniform(rnd, env.beta), env.uniform(rnd, env.beta)            # any rows serve as the aggregates
        got = take(env.ctx.rkg_round2(H0, H1, u, e2, e3))
        assert np.array_equal(got, kr.to_u64(kr.rkg_round2(env.ring, env.s, H0, H1, u, e2, e3)))


# ---------------------------------------------------------------- sampled forms
def test_sampled_forms_are_transcript_plus_core_and_count_their_indices(env):
    ctx, beta = env.ctx, env.beta
    ctx.seed_encryptor(KEY)
    assert ctx.encryptor_next_index() == 0
    rnd = np.random.default_rng(4)
    nxt = 0
    # public key share: 1 index, e = polynomial id 1
    crp = env.uniform(rnd)
    d, first = ctx.ckg_gen_share(crp)
    assert first == nxt and ctx.encryptor_next_index() == nxt + 1
    _, e, _ = ctx.encrypt_transcript(first, 1)
    assert np.array_equal(take(d), take(ctx.ckg_gen_share(crp, e[0])))
    nxt += 1
    # rotation shares: nkeys * beta indices, (k, i) takes first + k beta + i
    gs = galois_set(env.ring)[:2]
    crp = env.uniform(rnd, 2, beta)
    d, first = ctx.rtg_gen_shares(gs, crp)
    assert first == nxt and ctx.encryptor_next_index() == nxt + 2 * beta
    _, e, _ = ctx.encrypt_transcript(first, 2 * beta)
    assert np.array_equal(take(d), take(ctx.rtg_gen_shares(gs, crp, e.reshape(2, beta, N))))
    nxt += 2 * beta
    # round 1: beta + 1 indices, the last one is u's
    crp = env.uniform(rnd, beta)
    h0, h1, first, ui = ctx.rkg_round1(crp)
    assert first == nxt and ui == nxt + beta and ctx.encryptor_next_index() == nxt + beta + 1
    _, e0, e1 = ctx.encrypt_transcript(first, beta)
    u, _, _ = ctx.encrypt_transcript(ui, 1)
    x0, x1 = ctx.rkg_round1(crp, u[0], e0, e1)
    assert np.array_equal(take(h0), take(x0)) and np.array_equal(take(h1), take(x1))
    nxt += beta + 1
    # round 2: beta fresh indices; u redrawn from its index.  A fork draws from the same counter: disjoint indices
    H0, H1 = env.uniform(rnd, beta), env.uniform(rnd, beta)
    fork, fork2 = ctx.fork(), ctx.fork()
    try:
        d, first = fork.rkg_round2(H0, H1, u_index=ui)
        assert first == nxt and ctx.encryptor_next_index() == nxt + beta == fork.encryptor_next_index()
        _, e2, e3 = ctx.encrypt_transcript(first, beta)
        assert np.array_equal(take(d), take(ctx.rkg_round2(H0, H1, u[0], e2, e3)))
        nxt += beta
        d1, f1 = fork.ckg_gen_share(crp[0])                              # two forks: disjoint indices, different shares
        d2, f2 = fork2.ckg_gen_share(crp[0])
        assert (f1, f2) == (nxt, nxt + 1) and not np.array_equal(take(d1), take(d2))
    finally:
        fork.close(); fork2.close()
    assert ctx.encryptor_next_index() == nxt + 2


# ---------------------------------------------------------------- common reference polynomials
def test_crp_fill_every_modulus_and_an_offset_row_range(env):
    mods = env.ring.moduli
    idx = list(range(env.nmod))
    got = take(env.ctx.crp_fill(CRP_SEED, 0, idx))
    retried = 0
    for m in idx:
        want, tries = kr.crp_row(CRP_SEED, m, mods[m], N, want_tries=True)
        assert np.array_equal(got[m], want), m
        assert got[m].max() < mods[m]
        retried += int((tries > 0).sum())
    assert retried > 0                                                  # moduli just above a power of two: the t + 1 path ran on the device
    first = (1 << 32) + 5
    idx2 = idx[::-1] + [0]
    got2 = take(env.ctx.crp_fill(CRP_SEED, first, idx2))
    assert np.array_equal(got2, kr.crp_rows(CRP_SEED, first, idx2, mods, N))
    # a row is a function of (seed, global row number, modulus) alone: the same rows asked for from row 2 on
    part = take(env.ctx.crp_fill(CRP_SEED, 2, idx[2:]))
    assert np.array_equal(part, got[2:])


# ---------------------------------------------------------------- installation
def test_installed_keys_are_exported_exactly_and_rotate_as_the_oracle_does(env):
    ctx, ring, beta = env.ctx, env.ring, env.beta
    rnd = np.random.default_rng(6)
    k, level = 3, ring.nq - 1
    gs = [ring.galois(SLOTS - k), 2 * N - 1]
    agg = env.uniform(rnd, 2, beta)
    crp_dev = ctx.crp_fill(CRP_SEED, 100, [m for _ in range(2 * beta) for m in range(env.nmod)])
    crp = crp_dev.host().reshape(2, beta, env.nmod, N)
    ctx.install_rotkeys(gs, agg, crp_dev)                                 # crp straight from device memory
    crp_dev.free()
    fork = ctx.fork()
    try:
        for i, g in enumerate(gs):
            key = fork.export_rotkey(g)
            assert np.array_equal(key[:, 0], agg[i]) and np.array_equal(key[:, 1], crp[i]), g
    finally:
        fork.close()
    keys = ol.RotKeys(ring)
    keys.add(gs[0], ctx.export_rotkey(gs[0]))
    ct = ring.fill_uniform(level, 77)
    got = ctx.rotate_right(ct[None], level, [k])[0]
    assert np.array_equal(got, ol.rotate_left(ring, keys, level, ct, SLOTS - k))
    # the relinearisation key lives under Galois element 1; the public key is (agg, crp)
    ctx.install_relinkey(agg[0], crp[0])
    key = ctx.export_rotkey(1)
    assert np.array_equal(key[:, 0], agg[0]) and np.array_equal(key[:, 1], crp[0])
    ctx.install_public_key(agg[0, 0], crp[0, 0])
    assert ctx.has_public_key()


# ---------------------------------------------------------------- end to end: no oracle-made key anywhere
NPARTY, EB = 2, 19


def derived_bounds(q, p, level, scale, vmax):
    """DESIGN.md section 11, slot domain (a slot is a sum of N coefficients of modulus-1 weights over the scale: |slot error| <= N |coefficient error| / scale).
    |S| <= NPARTY per coefficient, ||S||_1 <= NPARTY N; aggregated errors <= NPARTY * EB; key-switch digits |d_i| < 2 D_i; every ModDown leaves each polynomial
    off by < 2, every rescale by <= 1."""
    P = p[0] * p[1]
    s1 = NPARTY * N
    nl = level + 1
    digits = [math.prod(q[i:min(i + len(p), nl)]) for i in range(0, nl, len(p))]
    md = 2 + 2 * s1
    enc = Fraction(NPARTY * EB * N + EB + EB * s1, P) + md + 1            # (E u + e0 + e1 S) / P, the ModDown, the encoder's rounding (1/2 <= 1)
    eps_enc = N * enc / Fraction(scale)
    ks_rot = Fraction(sum(N * 2 * d * NPARTY * EB for d in digits), P) + md
    rot = eps_enc + N * ks_rot / Fraction(scale)
    f = 2 * N * NPARTY * NPARTY * EB + 2 * NPARTY * EB                      # |S E0 + U E1 + E2 + E3|
    ks_rl = Fraction(sum(N * 2 * d * f for d in digits), P) + md
    scale2 = Fraction(scale) ** 2
    sq = 2 * vmax * eps_enc + eps_enc ** 2 + N * ks_rl / scale2 + N * (1 + s1) * q[level] / scale2
    return float(rot), float(sq)


def test_end_to_end_two_parties_keys_made_on_the_device():
    from sfgwas_amd import capi
    L = capi.lib()
    q, p = ol.Q_PN14, ol.P_PN14
    ring = ol.Ring(14, q, p)
    nmod, beta, level, scale, vmax = len(q) + len(p), ring.beta, 2, 2.0 ** 34, 4.0
    rnd = np.random.default_rng(2024)
    secrets = [rnd.integers(-1, 2, N).astype(np.int8) for _ in range(NPARTY)]
    S = (secrets[0].astype(np.int64) + secrets[1]).astype(np.int8)
    parties = [capi.Context(q, p) for _ in range(NPARTY)]
    third = capi.Context(q, p)
    mods = np.array(ring.moduli, dtype=np.uint64).reshape(nmod, 1)
    agg = lambda shares: sum(shares[1:], shares[0]) % mods                   # plain modular adds (words < 2^47)
    k = 5
    g = ring.galois(SLOTS - k)
    pk_rows, rl_rows, rt_rows = list(range(nmod)), [m for _ in range(beta) for m in range(nmod)], [m for _ in range(beta) for m in range(nmod)]
    try:
        for i, c in enumerate(parties):
            c.load_secret_key_qp(kr.to_u64(kr.rows_of(ring, secrets[i])))
            c.seed_encryptor(bytes([i + 1]) * 32)
        third.load_secret_key_qp(kr.to_u64(kr.rows_of(ring, S)))
        third.seed_encryptor(bytes([9]) * 32)
        # every party expands the same seed; the third context keeps its own copy on the device for the installation
        crp = [[c.crp_fill(CRP_SEED, 0, pk_rows), c.crp_fill(CRP_SEED, nmod, rl_rows), c.crp_fill(CRP_SEED, nmod * (1 + beta), rt_rows)] for c in parties + [third]]
        assert np.array_equal(crp[0][2].host(), crp[1][2].host())
        pk = agg([take(c.ckg_gen_share(crp[i][0])[0]) for i, c in enumerate(parties)])
        third.install_public_key(pk, crp[2][0])
        rt = agg([take(c.rtg_gen_shares([g], crp[i][2])[0]) for i, c in enumerate(parties)])
        third.install_rotkeys([g], rt, crp[2][2])
        r1 = [c.rkg_round1(crp[i][1]) for i, c in enumerate(parties)]
        H0, H1 = agg([take(x[0]) for x in r1]), agg([take(x[1]) for x in r1])
        r2 = agg([take(c.rkg_round2(H0, H1, u_index=r1[i][3])[0]) for i, c in enumerate(parties)])
        third.install_relinkey(r2, H1)
        for row in crp:
            for d in row:
                d.free()
        vals = rnd.uniform(-vmax, vmax, (1, SLOTS))
        ct = third.encrypt_vectors(vals, level)
        rot = capi.DevArray(third, (1, 2, level + 1, N))
        third.check(L.sfg_rotate_right_dev(third.h, ct.p, rot.p, 1, level, (C.c_int * 1)(k)), "rotate")
        bound_rot, bound_sq = derived_bounds(q, p, level, scale, vmax)
        err_rot = np.abs(third.decrypt_vectors(rot, level, scale)[0] - np.roll(vals[0], k)).max()
        print(f"rotation by {k} under the collectively generated key: max slot error {err_rot:.3e}, derived bound {bound_rot:.3e}")
        prod, res = capi.DevArray(third, (1, 2, level + 1, N)), capi.DevArray(third, (1, 2, level, N))
        third.check(L.sfg_ct_mulrelin_dev(third.h, ct.p, ct.p, prod.p, 1, level), "mulrelin")
        third.check(L.sfg_ct_rescale_dev(third.h, prod.p, res.p, 1, level), "rescale")
        err_sq = np.abs(third.decrypt_vectors(res, level - 1, scale * scale / q[level])[0] - vals[0] ** 2).max()
        print(f"square + rescale under the collectively generated relinearisation key: max slot error {err_sq:.3e}, derived bound {bound_sq:.3e}")
        # orientation only: the same rotation under a single-party oracle key of S (errors in [-3, 3])
        third.load_rotkey(g, ring.gen_rotkey(S, g, 123))
        third.check(L.sfg_rotate_right_dev(third.h, ct.p, rot.p, 1, level, (C.c_int * 1)(k)), "rotate")
        err_orc = np.abs(third.decrypt_vectors(rot, level, scale)[0] - np.roll(vals[0], k)).max()
        print(f"(orientation) the same rotation under an orc_gen_rotkey key of S: max slot error {err_orc:.3e}")
        for d in (ct, rot, prod, res):
            d.free()
        assert bound_rot < 0.2 and bound_sq < 1.0                       # the bounds mean something against values up to 4 and squares up to 16
        assert err_rot <= bound_rot
        assert err_sq <= bound_sq
    finally:
        for c in parties + [third]:
            c.close()


# ---------------------------------------------------------------- refusals
def test_refusals_launch_nothing():
    from sfgwas_amd import capi
    L = capi.lib()
    q, p = SHAPES["q3p2"]
    ctx = capi.Context(q, p)
    nmod, beta = 5, 2
    try:
        out = ctx.fill_uniform_cts(4, 2, 5)                             # 24 rows of recognisable words: room for every output below (at most 2 beta nmod = 20 rows)
        keep = out.host()
        z = capi.DevArray(ctx, (2 * beta * nmod, N)); zi = capi.DevArray(ctx, (2 * beta, N), np.int32); zu = capi.DevArray(ctx, (N,), np.int8)
        g1 = (C.c_uint64 * 1)(5)
        first, ui = C.c_uint64(), C.c_uint64()
        calls = [lambda: L.sfg_ckg_gen_share_dev(ctx.h, z.p, zi.p, out.p),
                 lambda: L.sfg_rtg_gen_shares_dev(ctx.h, g1, 1, z.p, zi.p, out.p),
                 lambda: L.sfg_rkg_round1_dev(ctx.h, z.p, zu.p, zi.p, zi.p, out.p, out.p),
                 lambda: L.sfg_rkg_round2_dev(ctx.h, z.p, z.p, zu.p, zi.p, zi.p, out.p)]
        sampled = [lambda: L.sfg_ckg_gen_share_sampled_dev(ctx.h, z.p, out.p, C.byref(first)),
                   lambda: L.sfg_rtg_gen_shares_sampled_dev(ctx.h, g1, 1, z.p, out.p, C.byref(first)),
                   lambda: L.sfg_rkg_round1_sampled_dev(ctx.h, z.p, out.p, out.p, C.byref(first), C.byref(ui)),
                   lambda: L.sfg_rkg_round2_sampled_dev(ctx.h, z.p, z.p, 0, out.p, C.byref(first))]
        ctx.seed_encryptor(KEY)
        for f in calls + sampled:                                        # no secret key over QP
            assert f() != 0 and b"no secret key over QP" in L.sfg_last_error(ctx.h)
        assert ctx.encryptor_next_index() == 0
        rnd = np.random.default_rng(8)
        ctx.load_secret_key_qp(np.stack([rnd.integers(0, m, N, dtype=np.uint64) for m in list(q) + list(p)]))
        bare = capi.Context(q, p)                                        # a secret key but no sampler key
        try:
            bare.load_secret_key_qp(np.zeros((nmod, N), np.uint64))
            for fn in (lambda: L.sfg_ckg_gen_share_sampled_dev(bare.h, z.p, out.p, None), lambda: L.sfg_rtg_gen_shares_sampled_dev(bare.h, g1, 1, z.p, out.p, None),
                       lambda: L.sfg_rkg_round1_sampled_dev(bare.h, z.p, out.p, out.p, None, C.byref(ui)), lambda: L.sfg_rkg_round2_sampled_dev(bare.h, z.p, z.p, 0, out.p, None)):
                assert fn() != 0 and b"no key" in L.sfg_last_error(bare.h)
        finally:
            bare.close()
        even = (C.c_uint64 * 2)(5, 6)
        assert L.sfg_rtg_gen_shares_dev(ctx.h, even, 2, z.p, zi.p, out.p) != 0 and b"odd" in L.sfg_last_error(ctx.h)
        assert L.sfg_rtg_gen_shares_sampled_dev(ctx.h, even, 2, z.p, out.p, C.byref(first)) != 0 and b"odd" in L.sfg_last_error(ctx.h)
        assert L.sfg_ctx_install_rotkeys_dev(ctx.h, even, 2, z.p, z.p) != 0 and b"odd" in L.sfg_last_error(ctx.h)
        assert not L.sfg_ctx_has_rotkey(ctx.h, 5) and not L.sfg_ctx_has_rotkey(ctx.h, 6)
        big = (C.c_uint64 * 1)(2 * N + 1)
        assert L.sfg_rtg_gen_shares_dev(ctx.h, big, 1, z.p, zi.p, out.p) != 0
        for fn in (lambda n: L.sfg_rtg_gen_shares_dev(ctx.h, g1, n, z.p, zi.p, out.p), lambda n: L.sfg_rtg_gen_shares_sampled_dev(ctx.h, g1, n, z.p, out.p, C.byref(first)),
                   lambda n: L.sfg_ctx_install_rotkeys_dev(ctx.h, g1, n, z.p, z.p)):
            assert fn(-1) != 0 and b"negative" in L.sfg_last_error(ctx.h)
            assert fn(0) == 0
        assert L.sfg_crp_fill_dev(ctx.h, CRP_SEED, 0, 1, (C.c_int * 1)(nmod), out.p) != 0 and b"out of range" in L.sfg_last_error(ctx.h)
        assert L.sfg_crp_fill_dev(ctx.h, CRP_SEED, 0, 0, None, None) == 0
        assert ctx.encryptor_next_index() == 0 and not L.sfg_ctx_has_rotkey(ctx.h, 5)
        ctx.sync()
        assert np.array_equal(out.host(), keep)                          # nothing was launched on the outputs
        for d in (out, z, zi, zu):
            d.free()
    finally:
        ctx.close()
