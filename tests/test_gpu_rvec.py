"""The ring-vector encoder and decoder on the device (sfgwas_amd/csrc/rvec.hip: sfg_rvec_encode_dev, sfg_rvec_decode_dev, sfg_ckks_to_ss_finish_dev) against the exact
Python-integer reference tests/rvec_ref.py (pinned by tests/test_rvec_ref.py), word for word: the encoder after the exact Python NTT of tests/exactref.py, the decoder
on rows made by that NTT.

Near-tie rule: the device value is within 2^-32 of the exact one before the final rounding, so a comparison is exact wherever the reference's distance to a rounding
tie exceeds 2^-32 (plus the reference's own error, < 2^-100).  Every seeded and directed input used here is further than that from a tie at every output - asserted
with each comparison, so the rule excludes NOTHING and can hide nothing; the one exact tie is a separate directed case.

Word counts reached (rvec_host.hpp; f = 30, scale 2^34 unless stated): encoder W = 3 (limbs 2) and W = 5 (limbs 4); decoder W = 2, 4, 5, 6, 7 at levels 0, 3, 5, 7, 9
and W = 8 at level 9 with f = 58.

PARITY UNPINNED against the lattigo fork's EncodeRVecNew / DecodeRVec (unpublished): what is pinned is the stated arithmetic."""
import ctypes as C
import math
from fractions import Fraction

import numpy as np
import pytest

import exactref
import keygen_ref as kr
import oracle_lib as ol
import rvec_cases as rc
import rvec_ref as rr

pytestmark = pytest.mark.gpu
N, n, F = rc.N, rc.n, rc.F
Q = ol.Q_PN14
LOWEST = {2: 3, 4: 7}                     # bitlen(p) - 1 - f + ceil(log2 scale) + 1 < bitlen(Q_level) - 1 first holds there (f = 30, scale 2^34)
FULL = ["uniform", "boundary", "all_max", "all_min", "one_slot", "pattern"]


@pytest.fixture(scope="module")
def ctx():
    from sfgwas_amd import capi
    c = capi.Context(ol.Q_PN14, ol.P_PN14)
    yield c
    c.close()


def ntt_rows(coeffs_list, level):
    """[k] lists of N integers -> uint64 [k][level+1][N], the exact NTT rows"""
    out = np.empty((len(coeffs_list), level + 1, N), dtype=np.uint64)
    for i in range(level + 1):
        out[:, i, :] = exactref.ntt(coeffs_list, Q[i], exactref.psi_for(Q[i], N))
    return out


@pytest.fixture(scope="module")
def enc_ref():
    """(limbs, name, scale) -> (input elements, expected rows [10][N]); the reference runs once per input, the lower level's rows are a prefix of level 9's"""
    out = {}
    for limbs, p in rc.FIELDS.items():
        todo = [(name, x, rc.SCALE) for name, x in rc.encode_inputs(p).items()]
        todo.append(("uniform", rc.encode_inputs(p)["uniform"], rc.SCALE_ODD))
        wants = []
        for name, x, scale in todo:
            want, tie, err = rr.encode(x, p, N, scale, F)
            assert min(tie) > rc.TIE_BAND + err, (limbs, name)            # nothing is excluded by the near-tie rule
            wants.append(want)
        rows = ntt_rows(wants, 9)
        for (name, x, scale), r in zip(todo, rows):
            out[(limbs, name, scale)] = (x, r)
    return out


@pytest.mark.parametrize("limbs", [2, 4])
def test_encode_word_for_word(ctx, enc_ref, limbs):
    """both fields, the lowest accepted level and level 9, n_elem 1 / 8191 / 8192, scale 2^34 and a scale that is not a power of two; seeded uniform elements, the
    centring boundary 0, 1, p - 1, (p - 1)/2, (p + 1)/2, all slots at +max and at -max (coefficient 0 at its bound, carries through every word), one nonzero
    slot, and the +- pattern that puts the whole sum into coefficient n/2"""
    mod = rc.modulus_words(rc.FIELDS[limbs], limbs)
    batches = [(FULL[:3], rc.SCALE), (FULL[3:], rc.SCALE), (["uniform_8191"], rc.SCALE), (["uniform_1"], rc.SCALE), (["uniform"], rc.SCALE_ODD)]
    for level in (LOWEST[limbs], 9):
        for names, scale in batches:
            shares = np.stack([rc.limbs_of(enc_ref[(limbs, nm, scale)][0], limbs) for nm in names])
            got = ctx.rvec_encode(mod, shares, level, float(scale), F)
            for k, nm in enumerate(names):
                assert np.array_equal(got[k], enc_ref[(limbs, nm, scale)][1][:level + 1]), (level, nm, float(scale))


def test_encode_rounds_an_exact_tie_to_one_of_its_neighbours(ctx):
    """one slot holding 1, scale 2^32, f = 20: coefficient 0 is 2^32 2^-20 / 8192 = 1/2 exactly; |got - exact| = 1/2 means it came out 0 or 1, everything else as
    the reference has it"""
    x, scale, f, level = [1], Fraction(2 ** 32), 20, 9
    want, tie, err = rr.encode(x, rc.FIELDS[2], N, scale, f)
    assert tie[0] == 0 and min(tie[1:]) > rc.TIE_BAND + err
    got = ctx.rvec_encode(rc.modulus_words(rc.FIELDS[2], 2), rc.limbs_of(x, 2)[None], level, float(scale), f)[0]
    cands = ntt_rows([[v] + want[1:] for v in (0, 1)], level)
    assert any(np.array_equal(got, c) for c in cands)


DEC_LEVELS = {0: None, 3: ["uniform"], 5: None, 7: ["uniform"], 9: None}          # None: every directed row


@pytest.fixture(scope="module")
def dec_ref():
    """level -> (names, rows uint64 [k][level+2][N] with a row of other words behind every block: pt_stride exceeds the block; expected signed integers per name)"""
    out = {}
    for level, only in DEC_LEVELS.items():
        Ql = rr.q_product(Q, level)
        cases = {k: v for k, v in rc.decode_inputs(Ql).items() if only is None or k in only}
        want = {}
        for name, res in cases.items():
            n_elem = n - 5 if name == "uniform" else n
            r, tie, err = rr.decode_int([rr.centred_crt(v, Ql) for v in res], N, rc.SCALE, F, n_elem)
            assert min(tie) > rc.TIE_BAND + err, (level, name)
            want[name] = r
        rows = np.full((len(cases), level + 2, N), 12345, dtype=np.uint64)
        rows[:, :level + 1, :] = ntt_rows(list(cases.values()), level)
        out[level] = (list(cases), rows, want)
    return out


@pytest.mark.parametrize("limbs", [2, 4])
@pytest.mark.parametrize("level", sorted(DEC_LEVELS))
def test_decode_word_for_word(ctx, dec_ref, level, limbs):
    """coefficients uniform in the centred range, all at the residue floor(Q/2) (the tie lattigo's rule makes negative), all at the largest positive value, all at
    -floor(Q/2) + 1, zero, a single coefficient, a single coefficient at the tie; a plaintext stride larger than the row block; n_elem < n for the uniform row"""
    p = rc.FIELDS[limbs]
    mod = rc.modulus_words(p, limbs)
    names, rows, want = dec_ref[level]
    for k0 in range(0, len(names), 3):
        for n_elem in sorted({len(want[nm]) for nm in names[k0:k0 + 3]}):
            idx = [k for k in range(k0, min(k0 + 3, len(names))) if len(want[names[k]]) == n_elem]
            got = ctx.rvec_decode(mod, rows[idx], level, float(rc.SCALE), F, n_elem)
            for j, k in enumerate(idx):
                assert rc.ints_of(got[j]) == [v % p for v in want[names[k]]], (level, names[k])


def test_decode_at_eight_words(ctx):
    """level 9 with f = 58, scale 2^34: 24 more fractional bits than f = 30 needs - the widest instantiation"""
    level, f, p = 9, 58, rc.FIELDS[4]
    Ql = rr.q_product(Q, level)
    assert rr.plan("dec", 256, Ql.bit_length(), rc.SCALE, f)[0] == 8
    res = rc.decode_inputs(Ql)["uniform"]
    want, tie, err = rr.decode([rr.centred_crt(v, Ql) for v in res], p, N, rc.SCALE, f, 64)
    assert min(tie) > rc.TIE_BAND + err
    got = ctx.rvec_decode(rc.modulus_words(p, 4), ntt_rows([res], level), level, float(rc.SCALE), f, 64)
    assert rc.ints_of(got[0]) == want


@pytest.mark.parametrize("limbs", [2, 4])
def test_ckks_to_ss_finish_is_finish_two_decodes_and_a_subtraction(ctx, limbs):
    """hub: decode(c0 + h0agg) - decode(mask_ntt) mod p; every other party: -decode(mask_ntt) mod p - each word against sfg_pcks_finish_dev, two
    sfg_rvec_decode_dev calls and Python's subtraction"""
    level, nct, n_elem = 5, 2, 100
    p = rc.FIELDS[limbs]
    mod = rc.modulus_words(p, limbs)
    rnd = np.random.default_rng(61)
    words = lambda *lead: np.stack([rnd.integers(0, Q[i], lead + (N,), dtype=np.uint64) for i in range(level + 1)], axis=-2)        # noqa: E731
    cts, h0agg, mask = words(nct, 2), words(nct), words(nct)
    pt = ctx.pcks_finish(cts, level, h0agg)
    a = [rc.ints_of(r) for r in ctx.rvec_decode(mod, pt, level, float(rc.SCALE), F, n_elem)]
    b = [rc.ints_of(r) for r in ctx.rvec_decode(mod, mask, level, float(rc.SCALE), F, n_elem)]
    hub = ctx.ckks_to_ss_finish(mod, cts, level, float(rc.SCALE), F, h0agg, mask, True, n_elem)
    oth = ctx.ckks_to_ss_finish(mod, None, level, float(rc.SCALE), F, None, mask, False, n_elem)
    for k in range(nct):
        assert rc.ints_of(hub[k]) == [(u - v) % p for u, v in zip(a[k], b[k])]
        assert rc.ints_of(oth[k]) == [(-v) % p for v in b[k]]


def test_results_are_bit_identical_across_calls_forks_and_batch_positions(ctx, enc_ref, dec_ref):
    limbs, level = 4, 9
    mod = rc.modulus_words(rc.FIELDS[limbs], limbs)
    shares = np.stack([rc.limbs_of(enc_ref[(limbs, nm, rc.SCALE)][0], limbs) for nm in FULL[:3]])
    first = ctx.rvec_encode(mod, shares, level, float(rc.SCALE), F)
    assert np.array_equal(first, ctx.rvec_encode(mod, shares, level, float(rc.SCALE), F))
    assert np.array_equal(first[1], ctx.rvec_encode(mod, shares[1:2], level, float(rc.SCALE), F)[0])
    _, rows, _ = dec_ref[5]
    dfirst = ctx.rvec_decode(mod, rows[:3], 5, float(rc.SCALE), F, n)
    assert np.array_equal(dfirst, ctx.rvec_decode(mod, rows[:3], 5, float(rc.SCALE), F, n))
    assert np.array_equal(dfirst[2], ctx.rvec_decode(mod, rows[2:3], 5, float(rc.SCALE), F, n)[0])
    fork = ctx.fork()
    try:
        assert np.array_equal(first, fork.rvec_encode(mod, shares, level, float(rc.SCALE), F))
        assert np.array_equal(dfirst, fork.rvec_decode(mod, rows[:3], 5, float(rc.SCALE), F, n))
    finally:
        fork.close()


def test_refusals_launch_nothing(ctx):
    """limbs = 3, an even modulus, n_elem = 8193, the encoder one level below the lowest accepted level of each field, f = 63, scale 0.5 / NaN / inf: an error
    string, and not a word of the output touched"""
    from sfgwas_amd import capi
    L = capi.lib()
    p2, p4 = rc.modulus_words(rc.FIELDS[2], 2), rc.modulus_words(rc.FIELDS[4], 4)
    even = p2.copy(); even[0] -= 1
    three = np.concatenate([p2, np.zeros(1, dtype=np.uint64)])
    src = capi.DevArray.from_host(ctx, np.full((2, 10, N), 7, dtype=np.uint64))
    out = capi.DevArray.from_host(ctx, np.full((10, N), 0xABCD, dtype=np.uint64))
    S = float(rc.SCALE)
    enc = lambda limbs, mod, n_elem, level, scale, f: L.sfg_rvec_encode_dev(ctx.h, limbs, capi.p64(mod), src.p, n_elem, 1, level, scale, f, out.p)        # noqa: E731
    dec = lambda limbs, mod, n_elem, level, scale, f: L.sfg_rvec_decode_dev(ctx.h, limbs, capi.p64(mod), src.p, 10 * N, 1, level, scale, f, n_elem, out.p)        # noqa: E731
    fin = lambda limbs, mod, n_elem, level, scale, f: L.sfg_ckks_to_ss_finish_dev(ctx.h, limbs, capi.p64(mod), src.p, 1, level, scale, f, src.p, src.p, 1, n_elem, out.p)        # noqa: E731
    bad = [((3, three, 8192, 9, S, 30), b"2 or 4"), ((2, even, 8192, 9, S, 30), b"odd"), ((2, p2, 8193, 9, S, 30), b"element count"),
           ((2, p2, 8192, 9, S, 63), b"frac_bits"), ((2, p2, 8192, 9, 0.5, 30), b"scale"), ((2, p2, 8192, 9, float("nan"), 30), b"scale"),
           ((2, p2, 8192, 9, float("inf"), 30), b"scale"), ((4, p4, 8192, 10, S, 30), b"level"), ((4, p4, 8192, -1, S, 30), b"level")]
    try:
        for args, word in bad:
            for call in (enc, dec, fin):
                assert call(*args) != 0 and word in L.sfg_last_error(ctx.h), (args[0], args[2:], word)
        for limbs, mod in ((2, p2), (4, p4)):
            assert enc(limbs, mod, 8192, LOWEST[limbs] - 1, S, 30) != 0 and b"level too small for the field" in L.sfg_last_error(ctx.h)
        assert L.sfg_rvec_decode_dev(ctx.h, 2, capi.p64(p2), src.p, 10 * N - 1, 1, 9, S, 30, 8192, out.p) != 0 and b"stride" in L.sfg_last_error(ctx.h)
        ctx.sync()
        assert np.all(out.host() == 0xABCD)
    finally:
        src.free(); out.free()


# ---------------------------------------------------------------- two parties end to end: secret shares -> one ciphertext -> secret shares
NPARTY, EB = 2, 19


def derived_bounds(q, p, level, scale, f):
    """DESIGN.md section 12, in units of x (the fixed-point integers), from the worst-case encryption noise of sections 9 and 11.  Under the summed key S
    (|S| <= NPARTY per coefficient, ||S||_1 <= s1 = NPARTY N) one ciphertext decrypts to its plaintext plus, per coefficient,
        enc = (NPARTY EB N + EB + EB s1) / P + (2 + 2 s1) + 1        ((E_pk u + e0 + e1 S) / P, the ModDown's rounding of both polynomials, the encoder's rounding)
    and the sum of the NPARTY parties' ciphertexts plus NPARTY times that.  A slot is a sum of the N coefficients with weights of modulus 1 and the decoded value is
    2^f / scale times it:
        secret shares -> CKKS:   |2^f decrypt_t - x_t| <= N NPARTY enc 2^f / scale + 1         (+ 1: the double rounding of sfg_decrypt_vectors on values below 2^21)
        CKKS -> secret shares:   |share_1 + share_2 - x_t| <= N (NPARTY enc + NPARTY EB) 2^f / scale + 3 (1/2 + 2^-32)
    (the decryption shares add their errors e0_i, |e0_i| <= EB; the hub rounds two decoded values and the other party one)."""
    P = math.prod(p)
    s1 = NPARTY * N
    enc = Fraction(NPARTY * EB * N + EB + EB * s1, P) + (2 + 2 * s1) + 1
    amp = Fraction(2 ** f) / Fraction(scale)
    to_ct = N * NPARTY * enc * amp + 1
    to_ss = N * (NPARTY * enc + NPARTY * EB) * amp + 3 * (Fraction(1, 2) + Fraction(1, 2 ** 32))
    return float(to_ct), float(to_ss)


@pytest.fixture(scope="module")
def two_parties():
    """pid 1 (the hub) and pid 2 with a collectively generated public key (as test_gpu_keygen.py makes one), and a third context holding the summed key"""
    from sfgwas_amd import capi
    ring = ol.Ring(14, ol.Q_PN14, ol.P_PN14)
    nmod = len(ol.Q_PN14) + len(ol.P_PN14)
    rnd = np.random.default_rng(2025)
    secrets = [rnd.integers(-1, 2, N).astype(np.int8) for _ in range(NPARTY)]
    S = (secrets[0].astype(np.int64) + secrets[1]).astype(np.int8)
    parties = [capi.Context(ol.Q_PN14, ol.P_PN14) for _ in range(NPARTY)]
    third = capi.Context(ol.Q_PN14, ol.P_PN14)
    mods = np.array(ring.moduli, dtype=np.uint64).reshape(nmod, 1)
    try:
        for i, c in enumerate(parties):
            c.load_secret_key_qp(kr.to_u64(kr.rows_of(ring, secrets[i])))
            c.seed_encryptor(bytes([i + 1]) * 32)
        third.load_secret_key_qp(kr.to_u64(kr.rows_of(ring, S)))
        third.seed_encryptor(bytes([9]) * 32)
        seed = bytes(range(7, 39))
        crp = [c.crp_fill(seed, 0, list(range(nmod))) for c in parties + [third]]
        shares = []
        for i, c in enumerate(parties):
            d = c.ckg_gen_share(crp[i])[0]
            shares.append(d.host()); d.free()
        pk = (shares[0] + shares[1]) % mods
        for c, d in zip(parties + [third], crp):
            c.install_public_key(pk, d)
            d.free()
        yield parties, third, rnd
    finally:
        for c in parties + [third]:
            c.close()


@pytest.mark.parametrize("limbs", [2, 4])
def test_two_parties_shares_to_ciphertext_and_back(two_parties, limbs):
    """x (f = 30, |x| < 2^50) additively shared mod p.  Python plays the network: the reveal is a sum of masked shares, the aggregations are word-wise sums mod q_i.
    sfg_ss_mask_dev -> reveal -> sfg_ss_hub_share_dev -> sfg_rvec_encode_dev -> sfg_encrypt_explicit_dev under the two-party key: the sum of the two ciphertexts
    decrypts under the summed key to x / 2^f.  sfg_ckks_to_ss_share_dev with masks below Q_level / (2 (nparty - 1)) -> aggregation -> sfg_ckks_to_ss_finish_dev: two
    shares whose sum mod p is x.  Both within the bounds DESIGN.md section 12 derives (derived_bounds above):
        derived:  shares -> CKKS 1.342e+08, CKKS -> shares 1.343e+08 units of x (one unit of x / 2^f is 2^30 = 1.07e+09);
        observed on the MI355X, largest deviation: limbs 2: 4.050e+04 and 4.069e+04; limbs 4: 4.082e+04 and 4.079e+04 (the worst-case bound adds the 2 * 32768
        ModDown roundings of a ciphertext coherently)."""
    from sfgwas_amd import capi
    L = capi.lib()
    parties, third, rnd = two_parties
    p, level, scale = rc.FIELDS[limbs], 7, float(rc.SCALE)
    mod = rc.modulus_words(p, limbs)
    Ql = rr.q_product(Q, level)
    mods = np.array(Q[:level + 1], dtype=np.uint64).reshape(level + 1, 1)
    x = [int(v) for v in rnd.integers(-2 ** 50 + 1, 2 ** 50, n)]
    a = rc.uniform_elems(p, n, 300 + limbs)
    rm = [a, [(v - s) % p for v, s in zip(x, a)]]                       # the two additive shares of x
    # ---- MPC.SSToCMat: mask, reveal, hub share, encode, encrypt
    bound = p // (4 * (NPARTY - 1))
    bnd = rc.modulus_words(bound, limbs)
    masked, mask = [], []
    for i, c in enumerate(parties):
        rand = rc.uniform_elems(bound, n, 310 + 2 * limbs + i)
        d = [capi.DevArray.from_host(c, rc.limbs_of(v, limbs)) for v in (rm[i], rand)]
        o = [capi.DevArray(c, (n, limbs)), capi.DevArray(c, (n, limbs))]
        c.check(L.sfg_ss_mask_dev(c.h, limbs, capi.p64(mod), capi.p64(bnd), d[0].p, d[1].p, o[0].p, o[1].p, n), "ss_mask")
        masked.append(rc.ints_of(o[0].host())); mask.append(o[1])
        for t in d + [o[0]]:
            t.free()
    revealed = [(u + v) % p for u, v in zip(*masked)]                   # RevealSym
    hub = parties[0]
    d_rev, d_sh = capi.DevArray.from_host(hub, rc.limbs_of(revealed, limbs)), capi.DevArray(hub, (n, limbs))
    hub.check(L.sfg_ss_hub_share_dev(hub.h, limbs, capi.p64(mod), d_rev.p, mask[0].p, d_sh.p, n), "ss_hub_share")
    new_share = [d_sh.host(), mask[1].host()]
    for t in (d_rev, d_sh, mask[0], mask[1]):
        t.free()
    assert [(u + v) % p for u, v in zip(*(rc.ints_of(s) for s in new_share))] == [v % p for v in x]
    cts = []
    for i, c in enumerate(parties):
        pt = c.rvec_encode(mod, new_share[i][None], level, scale, F)
        u, e0, e1 = rnd.integers(-1, 2, (1, N)), rnd.integers(-EB, EB + 1, (1, N)), rnd.integers(-EB, EB + 1, (1, N))
        cts.append(c.encrypt_explicit(pt, level, u, e0, e1))
    ct = (cts[0] + cts[1]) % mods
    bound_ct, bound_ss = derived_bounds(ol.Q_PN14, ol.P_PN14, level, scale, F)
    dec = third.decrypt_vectors(ct, level, scale)[0]
    dev_ct = max(abs(Fraction(float(g)) * 2 ** F - v) for g, v in zip(dec, x))
    print(f"limbs {limbs}: shares -> CKKS: largest |2^f decrypt - x| = {float(dev_ct):.3e}, derived bound {bound_ct:.3e}")
    # ---- MPC.CMatToSS: masked decryption shares, aggregation, finish
    h0, mk = [], []
    for i, c in enumerate(parties):
        vals = []
        for _ in range(N):
            m = int.from_bytes(rnd.bytes(64), "little") % (Ql // (2 * (NPARTY - 1)))
            vals.append(m - Ql // (2 * (NPARTY - 1)) if m >= Ql // (4 * (NPARTY - 1)) else m)
        h, m_ntt = c.ckks_to_ss_share(ct, level, ol.bigints_to_limbs(vals, 6)[None], rnd.integers(-EB, EB + 1, (1, N)).astype(np.int32))
        h0.append(h); mk.append(m_ntt)
    h0agg = (h0[0] + h0[1]) % mods
    s1 = parties[0].ckks_to_ss_finish(mod, ct, level, scale, F, h0agg, mk[0], True, n)[0]
    s2 = parties[1].ckks_to_ss_finish(mod, None, level, scale, F, None, mk[1], False, n)[0]
    back = [rr.centre((u + v) % p, p) for u, v in zip(rc.ints_of(s1), rc.ints_of(s2))]
    dev_ss = max(abs(g - v) for g, v in zip(back, x))
    print(f"limbs {limbs}: CKKS -> shares: largest |share_1 + share_2 - x| = {float(dev_ss):.3e}, derived bound {bound_ss:.3e}")
    assert bound_ct < 2 ** 30 and bound_ss < 2 ** 30                    # the bounds mean something against |x| up to 2^50: below one unit of x / 2^f
    assert dev_ct <= bound_ct
    assert dev_ss <= bound_ss


# ---------------------------------------------------------------- a second chunk: the encoder and the decoder take 64 plaintexts a chunk (batch_plan.hpp)
def test_encode_second_chunk_at_65_share_vectors(ctx):
    """65 share vectors of 100 seeded elements, every one different, at the lowest level the 128-bit field is accepted at (the encoder refuses level 0 for it:
    test_refusals_launch_nothing).  Items 63 and 64, either side of the boundary, word for word against rvec_ref; every item against two calls split there"""
    limbs, level, nct, cut, n_elem = 2, LOWEST[2], 65, 64, 100
    p = rc.FIELDS[limbs]
    mod = rc.modulus_words(p, limbs)
    xs = [rc.uniform_elems(p, n_elem, 1000 + k) for k in range(nct)]
    shares = np.stack([rc.limbs_of(x, limbs) for x in xs])
    assert len({s.tobytes() for s in shares}) == nct
    got = ctx.rvec_encode(mod, shares, level, float(rc.SCALE), F)
    wants = []
    for i in (cut - 1, cut):
        want, tie, err = rr.encode(xs[i], p, N, rc.SCALE, F)
        assert min(tie) > rc.TIE_BAND + err, i                                    # nothing is excluded by the near-tie rule
        wants.append(want)
    rows = ntt_rows(wants, level)
    assert np.array_equal(got[cut - 1], rows[0]) and np.array_equal(got[cut], rows[1])
    assert np.array_equal(got[:cut], ctx.rvec_encode(mod, shares[:cut], level, float(rc.SCALE), F))
    assert np.array_equal(got[cut:], ctx.rvec_encode(mod, shares[cut:], level, float(rc.SCALE), F))


def test_decode_second_chunk_at_65_plaintexts(ctx):
    """level 0, 65 plaintexts of uniform residues, every one different, n_elem = 100: items 63 and 64 against rvec_ref, every item against two calls split at 64"""
    limbs, level, nct, cut, n_elem = 2, 0, 65, 64, 100
    p = rc.FIELDS[limbs]
    mod = rc.modulus_words(p, limbs)
    Ql = rr.q_product(Q, level)
    res = np.random.default_rng(65).integers(0, Q[0], (nct, N), dtype=np.uint64)
    rows = ntt_rows([[int(v) for v in r] for r in res], level)
    assert rows.shape == (nct, 1, N) and len({r.tobytes() for r in rows}) == nct
    got = ctx.rvec_decode(mod, rows, level, float(rc.SCALE), F, n_elem)
    for i in (cut - 1, cut):
        want, tie, err = rr.decode_int([rr.centred_crt(int(v), Ql) for v in res[i]], N, rc.SCALE, F, n_elem)
        assert min(tie) > rc.TIE_BAND + err, i
        assert rc.ints_of(got[i]) == [v % p for v in want], i
    assert np.array_equal(got[:cut], ctx.rvec_decode(mod, rows[:cut], level, float(rc.SCALE), F, n_elem))
    assert np.array_equal(got[cut:], ctx.rvec_decode(mod, rows[cut:], level, float(rc.SCALE), F, n_elem))
