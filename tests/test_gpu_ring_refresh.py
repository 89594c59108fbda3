"""GPU tests of the general ring's collective bootstrap (sfgwas_amd/csrc/gring_refresh.hip): sfg_ring_refresh_gen_shares_dev, sfg_ring_refresh_finish_dev and
their target-scale forms.

Every word of h0, h1 and out against the Python integers of tests/ring_refresh_ref.py on nine chains (G12, G13, W15, W16, X12, L19, P14, M48, M33) at the levels
top (= nq - 1: no new modulus), middle and 0, in the unscaled form and under two scale pairs a chain (all pairs on P14 and M48, the pair that just fits the
capacity among them), three ciphertexts a call; P14 against the specialised context's four calls word for word; canonical rows; inputs and the words around
the outputs untouched; 1025 ciphertexts across the chunk boundary; two parties end to end on W15 and W16 within a derived bound; every refusal with its message.
PARITY UNPINNED like the PN14 path: expected values state lattigo v2.1.0 / v2.2.0 dckks/refresh.go as oracle/sfgwas_oracle.c restates it.
"""
import atexit
import ctypes as C
import math
from fractions import Fraction

import numpy as np
import pytest

import oracle_lib as ol
import ring_io_ref as rio
import ring_refresh_ref as rf
from sfgwas_amd import capi

pytestmark = pytest.mark.gpu

_DEV = {}
SENT = 0xA5A5A5A5A5A5A5A5


def dev_of(name):
    if name not in _DEV:
        logN, q, p = rf.chain(name)
        _DEV[name] = capi.Ring(logN, q, p)
        _DEV[name].load_secret_key(rf.secret_of(name))
    return _DEV[name]


@atexit.register
def _close_all():
    for d in _DEV.values():
        d.close()
    _DEV.clear()


CASES = [(n, lv, p) for n in rf.NAMES for lv in rf.levels(n) for p in [None] + rf.pairs_of(n, lv)]


def canonical(rows, moduli):
    """rows [..][len(moduli)][N]"""
    return all(int(rows[..., j, :].max()) < q for j, q in enumerate(moduli))


@pytest.mark.parametrize("name,level,pair", CASES, ids=lambda v: str(v))
def test_every_word_against_python_integers(name, level, pair):
    dev = dev_of(name)
    inp = rf.case_inputs(name, level, pair)
    h0, h1, out = rf.expected_of(inp)
    g0, g1 = dev.refresh_gen_shares(inp.cts, level, inp.crs, inp.mask_limbs, inp.e0, inp.e1, scales=inp.scales)
    go = dev.refresh_finish(inp.cts, level, inp.h0agg, inp.h1agg, inp.crs, scales=inp.scales)
    q = inp.ring.moduli[:inp.ring.nq]
    assert canonical(g0, q[:level + 1]) and canonical(g1, q) and canonical(go, q)
    assert np.array_equal(g0, h0), np.argwhere(g0 != h0)[:4]
    assert np.array_equal(g1, h1), np.argwhere(g1 != h1)[:4]
    assert np.array_equal(go, out), np.argwhere(go != out)[:4]
    assert go.shape == (3, 2, inp.ring.nq, inp.ring.N)                        # at level nq - 1


def test_cases_cover_what_the_issue_names():
    assert len({c[0] for c in CASES}) == 9
    for n in rf.NAMES:
        top = len(rf.chain(n)[1]) - 1
        assert {top, 0} <= {c[1] for c in CASES if c[0] == n}
        per_level = [sum(1 for c in CASES if c[0] == n and c[1] == lv and c[2] is not None) for lv in rf.levels(n)]
        assert min(per_level) >= (len(rf.ALL_PAIRS) if n in ("P14", "M48") else 2)
    assert ("M48", 46, "fit") in CASES and set(rf.REFERENCE_PAIRS) <= {c[2] for c in CASES if c[0] == "P14"}
    r = rf.ratio(rf.PAIRS["fit"])
    assert rf.fits_q(rf.q_bits("M48", 46), r[2]) and not rf.fits_q(rf.q_bits("M48", 46), rf.ratio(rf.PAIRS["miss"])[2])
    assert rf.limbs_for(rf.q_bits("M48", 46), r[2]) == 48 and rf.limbs_for(rf.q_bits("M48", 46), 0) == 46 and rf.limbs_for(rf.q_bits("M48", 45), 0) == 45


@pytest.mark.parametrize("level", [9, 4, 0])
@pytest.mark.parametrize("pair", [None, "ref", "ref_np2"])
def test_pn14_parameters_match_the_specialised_context(level, pair):
    """the same inputs through sfg_refresh_* and sfg_ring_refresh_*: equal words"""
    scales = None if pair is None else rf.PAIRS[pair]
    W = min(rf.mask_limbs_of("P14", level, scales), 7)                         # the specialised context holds 8 limbs: 64 W + 54 <= 512
    inp = rf.case_inputs("P14", level, pair, W=W, wide_errors=False)          # the context's lift takes |e| << q only
    dev = dev_of("P14")
    ctx = capi.Context(ol.Q_PN14, ol.P_PN14)
    try:
        ctx.load_secret_key(inp.sk)
        w0, w1 = ctx.refresh_gen_shares(inp.cts, level, inp.crs, inp.mask_limbs, inp.e0, inp.e1, scales=scales)
        wo = ctx.refresh_finish(inp.cts, level, inp.h0agg, inp.h1agg, inp.crs, scales=scales)
    finally:
        ctx.close()
    g0, g1 = dev.refresh_gen_shares(inp.cts, level, inp.crs, inp.mask_limbs, inp.e0, inp.e1, scales=scales)
    go = dev.refresh_finish(inp.cts, level, inp.h0agg, inp.h1agg, inp.crs, scales=scales)
    assert np.array_equal(g0, w0) and np.array_equal(g1, w1) and np.array_equal(go, wo)


# ---------------------------------------------------------------- inputs untouched, nothing written around the outputs
def framed(dev, arr, frame=512):
    """a device buffer [frame | arr | frame] of sentinel words -> (buffer, pointer to arr's place, host image)"""
    arr = np.ascontiguousarray(arr)
    raw = arr.view(np.uint8).reshape(-1)
    pad = (-raw.size) % 8
    host = np.concatenate([np.full(frame * 8, 0xA5, np.uint8), raw, np.full(pad + frame * 8, 0xA5, np.uint8)])
    buf = dev.to_device(host)
    return buf, C.c_void_p(buf.value + frame * 8), host


@pytest.mark.parametrize("name,level,pair", [("G13", 2, "ref_np2"), ("G13", 2, None), ("M33", 16, "l75"), ("X12", 2, None)])
def test_inputs_are_untouched_and_outputs_stay_inside_their_buffers(name, level, pair):
    dev, L = dev_of(name), capi.lib()
    inp = rf.case_inputs(name, level, pair, nct=2)
    scales, nq, N, nl, W = inp.scales, inp.ring.nq, inp.ring.N, level + 1, inp.W
    ins = [framed(dev, a) for a in (inp.cts, inp.crs, inp.mask_limbs, inp.e0, inp.e1, inp.h0agg, inp.h1agg)]
    outs = [framed(dev, np.full(shape, SENT, np.uint64)) for shape in ((2, nl, N), (2, nq, N), (2, 2, nq, N))]
    ct, crs, mask, e0, e1, h0a, h1a = [i[1] for i in ins]
    h0, h1, out = [o[1] for o in outs]
    try:
        if scales is None:
            dev.check(L.sfg_ring_refresh_gen_shares_dev(dev.h, ct, 2, level, crs, mask, W, e0, e1, h0, h1), "gen_shares")
            dev.check(L.sfg_ring_refresh_finish_dev(dev.h, ct, 2, level, h0a, h1a, crs, out), "finish")
        else:
            dev.check(L.sfg_ring_refresh_gen_shares_scaled_dev(dev.h, ct, 2, level, scales[0], scales[1], crs, mask, W, e0, e1, h0, h1), "gen_shares_scaled")
            dev.check(L.sfg_ring_refresh_finish_scaled_dev(dev.h, ct, 2, level, scales[0], scales[1], h0a, h1a, crs, out), "finish_scaled")
        for buf, _, host in ins:
            assert np.array_equal(dev.to_host(buf, host.shape, np.uint8), host)
        w0, w1, wo = rf.expected_of(inp)
        for (buf, _, host), want in zip(outs, (w0, w1, wo)):
            got = dev.to_host(buf, host.shape, np.uint8)
            body = want.view(np.uint8).reshape(-1)
            assert np.all(got[:4096] == 0xA5) and np.all(got[4096 + body.size:] == 0xA5)
            assert np.array_equal(got[4096:4096 + body.size], body)
    finally:
        for b in ins + outs:
            dev.free(b[0])


# ---------------------------------------------------------------- across the chunk boundary
def test_1025_ciphertexts_cross_the_chunk_boundary():
    """level 0 of G12, 1025 ciphertexts (one more than a chunk holds), every word: seven distinct ciphertexts' inputs in turn, so that the expected values are
    computed once each; ciphertext 1024, alone in the second chunk, is number 1024 % 7 = 2 of them"""
    name, level, period, nct = "G12", 0, 7, rf.CHUNK_CAP + 1
    dev = dev_of(name)
    for pair in (None, "ref"):
        inp = rf.case_inputs(name, level, pair, nct=period, seed=5)
        h0, h1, out = rf.expected_of(inp)
        idx = np.arange(nct) % period
        g0, g1 = dev.refresh_gen_shares(inp.cts[idx], level, inp.crs[idx], inp.mask_limbs[idx], inp.e0[idx], inp.e1[idx], scales=inp.scales)
        go = dev.refresh_finish(inp.cts[idx], level, inp.h0agg[idx], inp.h1agg[idx], inp.crs[idx], scales=inp.scales)
        assert np.array_equal(g0, h0[idx]) and np.array_equal(g1, h1[idx]) and np.array_equal(go, out[idx])


# ---------------------------------------------------------------- two parties end to end, wholly on the device
NPARTY, EB = 2, 19


def derived_bound(p, scale, N):
    """Slot error of encrypt -> drop to level 0 -> two-party refresh -> decrypt, in slot units, exactly.
    Encryption under a key s with ||s||_1 <= N: the ModDown of e_pk u + e0 + e1 s, |.| <= 19 N + 19 + 19 N per coefficient, divided by P; the ModDown leaves a
    polynomial off by < 2 + 2 ||s||_1; the encoder rounds by <= 1.  Dropping moduli changes nothing.  The refresh: c0 + sum h0 = m' + sum
    mask_i + sum e0_i exactly (no wrap: |m'| < 2^41 + noise, |sum mask_i| <= Q_0 / 4), and c0' + s c1' = x - sum mask_i - sum e1_i: the plaintext gains
    sum (e0_i - e1_i), at most 2 n 19 per coefficient.  A coefficient error c moves a slot by at most N c / scale."""
    P = math.prod(p)
    c_enc = Fraction(EB * N + EB + EB * N, P) + 2 + 2 * N + 1
    return N * (c_enc + 2 * NPARTY * EB) / Fraction(scale)


@pytest.mark.parametrize("name,scale", [("W15", 2.0 ** 40), ("W16", 2.0 ** 45)])
def test_end_to_end_two_parties(name, scale):
    logN, q, p = rf.chain(name)
    ring = ol.Ring(logN, q, p)
    N, nq, top = ring.N, len(q), len(q) - 1
    s, pk = rio.keypair(ring, 31)
    dev = capi.Ring(logN, q, p)
    parties = [capi.Ring(logN, q, p) for _ in range(NPARTY)]
    try:
        dev.load_public_key(pk)
        dev.seed_encryptor(bytes([7]) * 32)
        dev.load_secret_key(rio.sk_rows(ring, s))
        rnd = np.random.default_rng(77)
        v = rnd.uniform(-1.0, 1.0, N // 2)
        ct = dev.drop_level(dev.encrypt_vectors(v[None], top, scale), top, 0)              # encrypted on the device, then out of levels
        crs = rf.uniform_rows(rnd, q, N)[None]
        bound_mask = q[0] // 4                                                              # masks below Q_0 / 4: uniform in [0, Q_0 / (2 n)), recentred
        H0 = H1 = None
        for party, share in zip(parties, rio.split_secret(s, 11)):
            party.load_secret_key(rio.sk_rows(ring, share))
            masks = [int(m) - bound_mask // 2 for m in rnd.integers(0, bound_mask, N)]
            e0, e1 = (rnd.integers(-EB, EB + 1, (1, N)).astype(np.int32) for _ in range(2))
            h0, h1 = party.refresh_gen_shares(ct, 0, crs, rf.limbs_of(masks, 1)[None], e0, e1)
            H0 = h0 if H0 is None else (H0 + h0) % np.uint64(q[0])
            H1 = h1 if H1 is None else (H1 + h1) % np.array(q, dtype=np.uint64).reshape(1, nq, 1)
        out = parties[0].refresh_finish(ct, 0, H0, H1, crs)
        assert out.shape == (1, 2, nq, N) and np.array_equal(out[0, 1], crs[0])            # at level nq - 1
        re, im = dev.decrypt_vectors(out, top, scale, want_imag=True)
        err = max(np.max(np.abs(re[0] - v)), np.max(np.abs(im[0])))
        bound = derived_bound(p, scale, N)
        print(f"{name}: two-party refresh from level 0 to level {top}: max slot error {err:.3e}, derived bound {float(bound):.3e}")
        assert float(bound) < 0.01                                                          # it means something against slots up to 1
        assert Fraction(err) <= bound
    finally:
        for d in parties + [dev]:
            d.close()


# ---------------------------------------------------------------- refusals
def test_refusals_give_their_message_and_leave_the_output_untouched():
    name, level = "M48", 46
    logN, q, p = rf.chain(name)
    N, nq, nl = 1 << logN, len(q), level + 1
    L = capi.lib()
    dev = capi.Ring(logN, q, p)
    err = lambda: L.sfg_ring_last_error(dev.h).decode()                        # noqa: E731
    bufs = []

    def zeros(nbytes):
        bufs.append(dev.to_device(np.zeros(nbytes, np.uint8)))
        return bufs[-1]

    def sentinel(words):
        bufs.append(dev.to_device(np.full(words, SENT, np.uint64)))
        return bufs[-1]
    try:
        ct, crs, mask, e = zeros(2 * nl * N * 8), zeros(nq * N * 8), zeros(N * 48 * 8), zeros(N * 4)
        h0, h1, out = sentinel(nl * N), sentinel(nq * N), sentinel(2 * nq * N)
        gen = lambda nct=1, lv=level, W=44, c=ct, m=mask, o=h0: L.sfg_ring_refresh_gen_shares_dev(dev.h, c, nct, lv, crs, m, W, e, e, o, h1)      # noqa: E731
        gens = lambda a, b, W=44, lv=level: L.sfg_ring_refresh_gen_shares_scaled_dev(dev.h, ct, 1, lv, a, b, crs, mask, W, e, e, h0, h1)              # noqa: E731
        fin = lambda nct=1, lv=level, c=ct, o=out: L.sfg_ring_refresh_finish_dev(dev.h, c, nct, lv, crs, crs, crs, o)                                 # noqa: E731
        fins = lambda a, b, lv=level: L.sfg_ring_refresh_finish_scaled_dev(dev.h, ct, 1, lv, a, b, crs, crs, crs, out)                                # noqa: E731
        assert gen() == 1 and "no secret-key shard loaded" in err()
        dev.load_secret_key(rf.secret_of(name))
        fit, miss = rf.PAIRS["fit"], rf.PAIRS["miss"]
        for call, msg in [(lambda: gen(c=None), "null"), (lambda: gen(m=None), "null"), (lambda: gen(o=None), "null"),
                          (lambda: fin(c=None), "null"), (lambda: fin(o=None), "null"),
                          (lambda: gen(lv=nq), "level 47 out of range 0..46"), (lambda: gen(lv=-1), "out of range"), (lambda: fin(lv=nq), "out of range"),
                          (lambda: gens(2.0, 4.0, lv=nq), "out of range"), (lambda: fins(2.0, 4.0, lv=-1), "out of range"),
                          (lambda: gen(nct=-1), "negative ciphertext count"), (lambda: fin(nct=-3), "negative ciphertext count"),
                          (lambda: gen(W=0), "mask limb count 0 out of range 1..48"), (lambda: gen(W=49), "mask limb count 49 out of range 1..48"),
                          (lambda: gens(float("nan"), 2.0), "must be finite"), (lambda: gens(2.0, float("inf")), "must be finite"),
                          (lambda: gens(0.5, 2.0), "at least 1"), (lambda: fins(2.0, 2.0 ** 401), "at most 2^400"), (lambda: fins(0.0, 2.0), "at least 1"),
                          (lambda: fins(-8.0, -8.0), "at least 1"),
                          (lambda: fins(*miss), "Q_level (2867 bits)"), (lambda: gens(*miss), "does not fit 3072 bits"),
                          (lambda: gens(*fit, W=45), "a 45-limb mask times the target scale (shift 149) does not fit 3072 bits")]:
            assert call() == 1, msg
            assert msg in err(), (msg, err())
        dev.sync()
        for buf, words in ((h0, nl * N), (h1, nq * N), (out, 2 * nq * N)):
            assert np.all(dev.to_host(buf, (words,)) == np.uint64(SENT))
        # what is no refusal: an empty call (null pointers and all), and the pair that just fits with the widest mask it admits
        assert L.sfg_ring_refresh_gen_shares_dev(dev.h, None, 0, level, None, None, 1, None, None, None, None) == 0
        assert L.sfg_ring_refresh_finish_scaled_dev(dev.h, None, 0, level, 2.0, 4.0, None, None, None, None) == 0
        assert gens(*fit) == 0 and fins(*fit) == 0
        dev.sync()
    finally:
        for b in bufs:
            dev.free(b)
        dev.close()
