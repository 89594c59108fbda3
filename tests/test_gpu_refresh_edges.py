"""The collective bootstrap's HIP kernels (csrc/refresh.hip, csrc/recode.hpp) at the rare edges of their big-integer arithmetic: the directed
inputs of tests/refresh_ref.py - held against Python integers, the model and the oracle by tests/test_refresh_ref.py - through
refresh_gen_shares, ckks_to_ss_share and refresh_finish in both forms, on PN14, the 47-bit chain S4 and the 13-modulus chain R13.  Every
comparison is bit-exact: with a zero key, zero crs and zero aggregated shares the rows read back through the oracle's ring.intt are the Python
integers themselves; with a real key and random crs / shares every word is the oracle's.  Then the limb counts and the library's refusals,
each with its message."""
import ctypes as C
import re
from functools import lru_cache

import numpy as np
import pytest

import oracle_lib as ol
import refresh_ref as rr

pytestmark = pytest.mark.gpu
IDS = [rr.case_id(c) for c in rr.CASES]
SS_CASES = [c for c in rr.CASES if c[3] in (None, "ref")]           # ckks_to_ss_share has no scale: one run per (chain, level, W)
N = rr.N


def rows_mod(rnd, moduli):
    return np.stack([rnd.integers(0, q, N, dtype=np.uint64) for q in moduli])


@lru_cache(maxsize=None)
def real_key(name):
    ring = rr.ring_of(name)
    return ol.secret_ntt(ring, ring.gen_secret(4))


def use_key(ctx, ring, name, real):
    ctx.load_secret_key(real_key(name) if real else np.zeros((ring.nq, N), dtype=np.uint64))


def share_batch(c):
    """nct = 3: an all-zero mask with zero e, the directed set moved by one coefficient, the directed set -> (limbs [3][N][W], e [3][N], shifts)"""
    limbs = np.stack([np.zeros_like(c.limbs), np.roll(c.limbs, 1, axis=0), c.limbs])
    e = np.stack([np.zeros_like(c.e), np.roll(c.e, 1), c.e])
    return limbs, e, (None, 1, 0)


def intt_rows(ring, rows):
    return np.stack([ring.intt(j, rows[j]) for j in range(rows.shape[0])])


@pytest.mark.parametrize("case", rr.CASES, ids=IDS)
def test_shares_with_zero_key_are_the_python_integers(case):
    """h0 = NTT((mask + e0) mod q_j), j <= level, and h1 = -NTT((Quo(mask Int(target), Int(scale)) + e1) mod q_j) over all nq moduli;
    the all-zero ciphertext: k_share negating 0 gives 0, not q"""
    c = rr.case_inputs(case)
    ctx, ring = rr.gpu_env(case[0])
    use_key(ctx, ring, case[0], False)
    limbs, e, shifts = share_batch(c)
    cts = np.stack([ring.fill_uniform(c.level, 30 + i) for i in range(3)])
    crs = np.zeros((3, ring.nq, N), dtype=np.uint64)
    h0, h1 = ctx.refresh_gen_shares(cts, c.level, crs, limbs, e, e, scales=c.scales)
    assert not h0[0].any() and not h1[0].any()
    qcol = np.array(c.q, dtype=np.uint64)[:, None]
    for i in (1, 2):
        assert np.array_equal(intt_rows(ring, h0[i]), np.roll(c.want_h0, shifts[i], axis=1)), f"h0 of ciphertext {i}"
        assert np.array_equal(intt_rows(ring, h1[i]), np.roll((qcol - c.want_h1) % qcol, shifts[i], axis=1)), f"h1 of ciphertext {i}"
    if c.scales is not None and rr.ratio(c.scales) is None:
        u0, u1 = ctx.refresh_gen_shares(cts, c.level, crs, limbs, e, e)
        assert np.array_equal(u0, h0) and np.array_equal(u1, h1)


@pytest.mark.parametrize("case", rr.CASES, ids=IDS)
def test_shares_with_a_real_key_are_the_oracles(case):
    c = rr.case_inputs(case)
    ctx, ring = rr.gpu_env(case[0])
    use_key(ctx, ring, case[0], True)
    sk = real_key(case[0])
    limbs, e, _ = share_batch(c)
    e1 = np.ascontiguousarray(e[:, ::-1])
    rnd = np.random.default_rng(40 + rr.CASES.index(case))
    cts = np.stack([ring.fill_uniform(c.level, 50 + i) for i in range(3)])
    crs = np.stack([rows_mod(rnd, c.q) for _ in range(3)])
    h0, h1 = ctx.refresh_gen_shares(cts, c.level, crs, limbs, e, e1, scales=c.scales)
    for i in range(3):
        if c.scales is None:
            w0, w1 = ol.refresh_gen_shares(ring, c.level, cts[i], sk, crs[i], limbs[i], e[i], e1[i])
        else:
            w0, w1 = ol.refresh_gen_shares_scaled(ring, c.level, cts[i], c.scales[0], c.scales[1], sk, crs[i], limbs[i], e[i], e1[i])
        assert np.array_equal(h0[i], w0), f"h0 of ciphertext {i}"
        assert np.array_equal(h1[i], w1), f"h1 of ciphertext {i}"


@pytest.mark.parametrize("case", SS_CASES, ids=[rr.case_id(c) for c in SS_CASES])
def test_ckks_to_ss_share_at_the_mask_and_error_edges(case):
    """zero key: mask_ntt = NTT(mask mod q_j) and h0 = NTT((mask + e0) mod q_j) in Python integers (e0 through k_small_rows at +-(2^31 - 1), -2^31);
    real key: the oracle's decrypt share, every word"""
    c = rr.case_inputs(case)
    ctx, ring = rr.gpu_env(case[0])
    nl = c.level + 1
    limbs, e, shifts = share_batch(c)
    cts = np.stack([ring.fill_uniform(c.level, 70 + i) for i in range(3)])
    use_key(ctx, ring, case[0], False)
    h0, mk = ctx.ckks_to_ss_share(cts, c.level, limbs, e)
    assert not h0[0].any() and not mk[0].any()
    qcol = np.array(c.q[:nl], dtype=np.uint64)[:, None]
    want_mask = (c.want_h0 + qcol - rr.model_small_rows(c.e, c.q[:nl])) % qcol
    for i in (1, 2):
        assert np.array_equal(intt_rows(ring, h0[i]), np.roll(c.want_h0, shifts[i], axis=1)), f"h0 of ciphertext {i}"
        assert np.array_equal(intt_rows(ring, mk[i]), np.roll(want_mask, shifts[i], axis=1)), f"mask plaintext of ciphertext {i}"
    use_key(ctx, ring, case[0], True)
    sk = real_key(case[0])
    g0, gk = ctx.ckks_to_ss_share(cts, c.level, limbs, e)
    zero_e, zero_crs = np.zeros(N, dtype=np.int32), np.zeros((ring.nq, N), dtype=np.uint64)
    assert np.array_equal(gk, mk)
    for i in range(3):
        assert np.array_equal(g0[i], ol.refresh_gen_shares(ring, c.level, cts[i], sk, zero_crs, limbs[i], e[i], zero_e)[0]), f"ciphertext {i}"


def finish_batch(c, ring):
    """nct = 3 ciphertexts whose polynomial 0 is the NTT of the directed x moved by 1, by 7 and not at all"""
    nl, shifts = c.level + 1, (1, 7, 0)
    cts = np.zeros((3, 2, nl, N), dtype=np.uint64)
    for i, s in enumerate(shifts):
        for j in range(nl):
            cts[i, 0, j] = ring.ntt(j, np.roll(c.x_res[j], s))
    return cts, shifts


@pytest.mark.parametrize("case", rr.CASES, ids=IDS)
def test_finish_with_zero_shares_is_the_python_integers(case):
    """polynomial 0 read back through ring.intt: the recentred (a tie is negative), rescaled x modulo every one of the nq moduli; polynomial 1 = crs"""
    c = rr.case_inputs(case)
    ctx, ring = rr.gpu_env(case[0])
    cts, shifts = finish_batch(c, ring)
    rnd = np.random.default_rng(60 + rr.CASES.index(case))
    crs = np.stack([rows_mod(rnd, c.q) for _ in range(3)])
    z0, z1 = np.zeros((3, c.level + 1, N), dtype=np.uint64), np.zeros((3, ring.nq, N), dtype=np.uint64)
    got = ctx.refresh_finish(cts, c.level, z0, z1, crs, scales=c.scales)
    for i in range(3):
        assert np.array_equal(intt_rows(ring, got[i, 0]), np.roll(c.want_x, shifts[i], axis=1)), f"ciphertext {i}"
        assert np.array_equal(got[i, 1], crs[i])
    if c.scales is not None and rr.ratio(c.scales) is None:
        assert np.array_equal(got, ctx.refresh_finish(cts, c.level, z0, z1, crs))


@pytest.mark.parametrize("case", rr.CASES, ids=IDS)
def test_finish_with_random_shares_is_the_oracles(case):
    c = rr.case_inputs(case)
    ctx, ring = rr.gpu_env(case[0])
    cts, _ = finish_batch(c, ring)
    rnd = np.random.default_rng(80 + rr.CASES.index(case))
    crs = np.stack([rows_mod(rnd, c.q) for _ in range(3)])
    h0 = np.stack([rows_mod(rnd, c.q[:c.level + 1]) for _ in range(3)])
    h1 = np.stack([rows_mod(rnd, c.q) for _ in range(3)])
    h0[2] = 0                                               # the directed x itself, with the recrypt share on top
    got = ctx.refresh_finish(cts, c.level, h0, h1, crs, scales=c.scales)
    for i in range(3):
        if c.scales is None:
            want = ol.refresh_finish(ring, c.level, cts[i], h0[i], h1[i], crs[i])
        else:
            want = ol.refresh_finish_scaled(ring, c.level, cts[i], c.scales[0], c.scales[1], h0[i], h1[i], crs[i])
        assert np.array_equal(got[i], want), f"refreshed ciphertext {i}"
    if c.scales is not None and rr.ratio(c.scales) is None:
        assert np.array_equal(got, ctx.refresh_finish(cts, c.level, h0, h1, crs))


# ---------------------------------------------------------------- the entry points called directly: no-ops and refusals
class Raw:
    """the five entry points on one scratch buffer that is large enough for every argument of a one-ciphertext call with W <= 17: a refused call
    touches none of it, a call that should have been refused stays inside it"""

    def __init__(self, ctx):
        from sfgwas_amd import capi
        self.ctx, self.L = ctx, capi.lib()
        self.buf = ctx.malloc(40 * N * 8)
        self.fill = np.full(40 * N, 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
        ctx.check(self.L.sfg_memcpy_h2d(ctx.h, self.buf, self.fill.ctypes.data_as(C.c_void_p), self.fill.nbytes), "h2d")

    def call(self, what, level, W=4, scales=None, nct=1):
        b, h, L = self.buf, self.ctx.h, self.L
        if what == "shares":
            rc = L.sfg_refresh_gen_shares_dev(h, b, nct, level, b, b, W, b, b, b, b) if scales is None else \
                L.sfg_refresh_gen_shares_scaled_dev(h, b, nct, level, float(scales[0]), float(scales[1]), b, b, W, b, b, b, b)
        elif what == "ss":
            rc = L.sfg_ckks_to_ss_share_dev(h, b, nct, level, b, W, b, b, b)
        else:
            rc = L.sfg_refresh_finish_dev(h, b, nct, level, b, b, b, b) if scales is None else \
                L.sfg_refresh_finish_scaled_dev(h, b, nct, level, float(scales[0]), float(scales[1]), b, b, b, b)
        return rc, L.sfg_last_error(h).decode() if rc else ""

    def untouched(self):
        self.ctx.sync()
        return np.array_equal(self.ctx.to_host(self.buf, (40 * N,), np.uint64), self.fill)

    def close(self):
        self.ctx.free(self.buf)


@pytest.fixture
def raw_pn14():
    ctx, ring = rr.gpu_env("PN14")
    use_key(ctx, ring, "PN14", False)
    r = Raw(ctx)
    yield r
    r.close()


def test_zero_ciphertexts_is_a_no_op(raw_pn14):
    for what, scales in (("shares", None), ("shares", rr.PAIRS["ref"]), ("ss", None), ("finish", None), ("finish", rr.PAIRS["ref"])):
        assert raw_pn14.call(what, 4, 4, scales, nct=0) == (0, "")
    assert raw_pn14.untouched()


def test_limb_counts_out_of_range_are_refused(raw_pn14):
    ref = rr.PAIRS["ref"]
    # 8 limbs are as many as the device integer has, and the fit check refuses them: 64 * 8 + 54 bits of mask times mantissa are past 512
    assert raw_pn14.call("shares", 4, 8, ref) == (1, "refresh: a 8-limb mask times the target scale (shift -16) does not fit 512 bits")
    assert raw_pn14.call("shares", 4, 9, ref) == (1, "refresh: mask limb count 9 exceeds 8 in the target-scale form")
    assert raw_pn14.call("shares", 4, 17, ref) == (1, "refresh: mask limb count 17 exceeds 8 in the target-scale form")
    assert raw_pn14.call("shares", 4, 0, ref) == (1, "refresh: mask limb count 0 out of range")
    assert raw_pn14.call("shares", 4, 0) == (1, "refresh: mask limb count 0 out of range")
    assert raw_pn14.call("shares", 4, 17) == (1, "refresh: mask limb count 17 out of range")
    assert raw_pn14.call("ss", 4, 0) == (1, "CMatToSS: mask limb count 0 out of range")
    assert raw_pn14.call("ss", 4, 17) == (1, "CMatToSS: mask limb count 17 out of range")
    assert raw_pn14.untouched()


def test_scales_and_levels_out_of_range_are_refused(raw_pn14):
    for what in ("shares", "finish"):
        assert raw_pn14.call(what, 4, 4, (0.5, 2.0 ** 34)) == (1, "refresh: scale 0.5 out of range")
        assert raw_pn14.call(what, 4, 4, (2.0 ** 68, 0.999)) == (1, "refresh: scale 0.999 out of range")
        assert raw_pn14.call(what, 4, 4, (2.0 ** 401, 2.0 ** 34)) == (1, "refresh: scale %g out of range" % 2.0 ** 401)
        assert raw_pn14.call(what, 4, 4, (2.0 ** 68, 2.0 ** 34 * 1.5 * 2.0 ** 400)) == (1, "refresh: scale %g out of range" % (1.5 * 2.0 ** 434))
        rc, msg = raw_pn14.call(what, 4, 4, (float("nan"), 2.0 ** 34))
        assert rc == 1 and re.fullmatch(r"refresh: scale -?nan out of range", msg)
        rc, msg = raw_pn14.call(what, 4, 4, (2.0 ** 68, float("inf")))
        assert rc == 1 and msg == "refresh: scale inf out of range"
        # PN14 at level 9 has 361.1 bits: + 54 + shift 105 is past 510
        assert raw_pn14.call(what, 9, 4, (2.0 ** 55, 2.0 ** 160)) == (1, "refresh: Q_level * target scale / ciphertext scale does not fit 512 bits")
        assert raw_pn14.call(what, 10, 4, rr.PAIRS["ref"]) == (1, "refresh: level 10 out of range")
        assert raw_pn14.call(what, -1, 4, rr.PAIRS["ref"]) == (1, "refresh: level -1 out of range")
        assert raw_pn14.call(what, 10, 4) == (1, "refresh: level 10 out of range")
        assert raw_pn14.call(what, 4, 4, nct=-1) == (1, "refresh: negative ciphertext count")
    # the share form's own check: Q_9 2^75 fits, a 6-limb mask times 2^53 2^75 does not
    assert raw_pn14.call("shares", 9, 6, rr.PAIRS["l75"]) == (1, "refresh: a 6-limb mask times the target scale (shift 75) does not fit 512 bits")
    assert raw_pn14.untouched()


def test_level_12_is_refused_on_the_13_modulus_chain():
    """RF_MAXL = 12 moduli at the input level: level 11 runs (the R13 cases above), level 12 is a valid level of R13 and is refused"""
    ctx, ring = rr.gpu_env("R13")
    use_key(ctx, ring, "R13", False)
    r = Raw(ctx)
    try:
        for what in ("shares", "ss", "finish"):
            assert r.call(what, 12) == (1, "refresh: more than 12 moduli at the input level")
        assert r.call("shares", 13) == (1, "refresh: level 13 out of range")
        assert r.untouched()
    finally:
        r.close()


def test_share_calls_without_a_secret_key_are_refused():
    from sfgwas_amd import capi
    q, p = rr.chain("PN14")
    ctx = capi.Context(q, p)                                  # a second context: the session's has a key loaded
    r = Raw(ctx)
    try:
        assert r.call("shares", 4) == (1, "refresh: no secret-key shard loaded (sfg_ctx_load_secret_key)")
        assert r.call("shares", 4, 4, rr.PAIRS["ref"]) == (1, "refresh: no secret-key shard loaded (sfg_ctx_load_secret_key)")
        assert r.call("ss", 4) == (1, "CMatToSS: no secret-key shard loaded (sfg_ctx_load_secret_key)")
        assert r.untouched()
    finally:
        r.close()
        ctx.close()
