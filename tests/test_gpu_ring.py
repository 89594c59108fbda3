"""The general ring (sfgwas_amd/csrc/gring.hip, capi.Ring) on the GPU, word for word against the CPU oracle on the chains of tests/ring_cases.py:
transforms, rotations, conjugation, the evaluator operations, the 19-modulus chain against the Python-integer key switch of tests/ring_ref.py, the PN14 chain
against the specialised Context, an end-to-end rotate / square / rescale on two wide chains, every refusal with its message, and the rotation, the product
and the rescale on batches that need a second chunk of the workspace.  The launch splits at 16384 ciphertexts and at 32768 rows need gigabytes per operand and
are not run here: tests/test_ring_ref.py holds the split helper and the caps on the CPU.
What holds the key switch beyond this file: the words here are uniform or one of five directed rows, which put the basis extension's float sum on an integer with
probability around 2^-50, and the chains add at most 9 terms of 36 bits or 2 of 61 into a 128-bit sum.  tests/test_gpu_ring_edges.py runs directed words on both
float boundaries of every digit and of ModDown, 61-bit chains of 18 + 3, 34 + 4, 47 + 1 and 1 + 47 moduli with the sums at their ceilings, and the rescale onto a
modulus 2^31 times smaller; tests/test_ring_edges_ref.py asserts from the model's trace that those words reach the classes v_float - v_exact = +1, 0 (and -1 from
four moduli a digit on) and that a model which rounds v, takes it exact or multiplies by fl(1/q) gives other words.
One device ring, one oracle ring and one key set per chain for the module."""
import atexit
import ctypes as C

import numpy as np
import pytest

import oracle_lib as ol
import ring_cases as rc
import ring_ref
from sfgwas_amd import capi

pytestmark = pytest.mark.gpu

ORACLE_CHAINS = [n for n in rc.NAMES if n != "L19"]          # L19 has more moduli than one oracle ring holds
_ENV = {}


class Env:
    def __init__(self, name):
        self.name = name
        self.logN, self.q, self.p = rc.chain(name)
        self.dev = capi.Ring(self.logN, self.q, self.p)
        self.ring = ring_ref.SplitRing(self.logN, self.q, self.p) if name == "L19" else ol.Ring(self.logN, self.q, self.p)
        self.N, self.slots, self.moduli = self.ring.N, self.ring.slots, self.ring.moduli
        if name != "L19":
            self.s = self.ring.gen_secret(1234)
            self.keys = ol.RotKeys(self.ring)
            self.rlk = None

    def need_galois(self, g):
        if g not in self.keys.keys:
            key = self.ring.gen_rotkey(self.s, g, 77 + g)
            self.keys.add(g, key)
            self.dev.load_rotkey(g, key)

    def need_right(self, *amounts):
        for k in amounts:
            if k % self.slots:
                self.need_galois(self.ring.galois(self.slots - k % self.slots))

    def need_rlk(self):
        if self.rlk is None:
            self.rlk = np.zeros((self.ring.beta, 2, len(self.moduli), self.N), dtype=np.uint64)
            ol.lib().orc_gen_rlk(self.ring.h, ol.pi8(self.s), 4242, ol.p64(self.rlk))
            self.dev.load_relinkey(self.rlk)
        return self.rlk

    def cts(self, level, seed):
        """two ciphertexts: uniform words, and one whose rows are the directed rows (all q - 1, all 0, one-hot at 0 and N - 1, alternating 0, q - 1)"""
        a, b = self.ring.fill_uniform(level, seed), self.ring.fill_uniform(level, seed + 1)
        for m in range(level + 1):
            d = rc.directed_rows(self.moduli[m], self.N)
            b[1, m] = d[(m + seed) % 5]
            b[0, m] = d[(m + seed + 2) % 5]
        return np.stack([a, b])


def env(name):
    if name not in _ENV:
        _ENV[name] = Env(name)
    return _ENV[name]


@atexit.register
def _close_all():
    for e in _ENV.values():
        e.dev.close()
    _ENV.clear()


def orc(fn, ring, out_shape, *args):
    """one oracle call whose last argument is its output"""
    out = np.zeros(out_shape, dtype=np.uint64)
    rc_ = getattr(ol.lib(), fn)(ring.h, *args, ol.p64(out))
    assert fn not in ("orc_apply_galois", "orc_innersum_all") or rc_ == 0, f"{fn}: missing key"        # the others return nothing
    return out


def c64(a):
    return ol.p64(np.ascontiguousarray(a, dtype=np.uint64))


# ---------------------------------------------------------------- transforms
@pytest.mark.parametrize("name", rc.NAMES)
def test_ntt_and_intt_of_every_modulus_equal_the_oracle(name):
    e = env(name)
    rnd = np.random.default_rng(7)
    rows, idx = [], []
    for m, q in enumerate(e.moduli):
        block = np.concatenate([rc.directed_rows(q, e.N), rnd.integers(0, q, (2, e.N), dtype=np.uint64)])
        rows.append(block)
        idx += [m] * len(block)
    rows = np.concatenate(rows)
    fwd = e.dev.ntt_rows(rows, idx)
    inv = e.dev.ntt_rows(rows, idx, inverse=True)
    for r, m in enumerate(idx):
        assert np.array_equal(fwd[r], e.ring.ntt(m, rows[r])), (name, m, r % 7)
        assert np.array_equal(inv[r], e.ring.intt(m, rows[r])), (name, m, r % 7)
    assert np.array_equal(e.dev.ntt_rows(fwd, idx, inverse=True), rows)


# ---------------------------------------------------------------- rotations and conjugation
@pytest.mark.parametrize("name", ORACLE_CHAINS)
def test_rotate_right_equals_the_oracle(name):
    e = env(name)
    amounts = [0, 1, 7, e.slots - 1]
    e.need_right(*amounts)
    for level in rc.levels(name):
        two = e.cts(level, 10 + level)
        batch = np.stack([two[0], two[1], two[0], two[1]])
        got = e.dev.rotate_right(batch, level, amounts)                              # one batch, four different amounts (0 = copy)
        for j, k in enumerate(amounts):
            assert np.array_equal(got[j], ol.rotate_right(e.ring, e.keys, level, batch[j], k)), (name, level, k)
        got = e.dev.rotate_right(two, level, [7, 7 + e.slots])                       # amounts are taken mod slots
        assert np.array_equal(got[0], ol.rotate_right(e.ring, e.keys, level, two[0], 7)) and np.array_equal(got[1], ol.rotate_right(e.ring, e.keys, level, two[1], 7))


@pytest.mark.parametrize("name", ORACLE_CHAINS)
def test_conjugation_equals_the_oracle(name):
    e = env(name)
    g = 2 * e.N - 1
    e.need_galois(g)
    for level in rc.levels(name):
        two = e.cts(level, 20 + level)
        got = e.dev.apply_galois(two, level, g)
        for j in range(2):
            want = orc("orc_apply_galois", e.ring, two[j].shape, e.keys.h, level, c64(two[j]), g)
            assert np.array_equal(got[j], want), (name, level, j)


# ---------------------------------------------------------------- the remaining operations, two ciphertexts in one batch
@pytest.mark.parametrize("name", ORACLE_CHAINS)
def test_products_and_rescale_equal_the_oracle(name):
    e = env(name)
    rlk = e.need_rlk()
    for level in rc.levels(name):
        a, b = e.cts(level, 30 + level), e.cts(level, 40 + level)
        got = e.dev.mulrelin(a, b, level)
        for j in range(2):
            assert np.array_equal(got[j], orc("orc_mulrelin", e.ring, a[j].shape, level, c64(a[j]), c64(b[j]), c64(rlk))), (name, level, j)
        pt = np.stack([e.ring.fill_uniform(level, 50 + level)[0], b[1, 1]])          # per-ciphertext plaintexts: uniform, and the directed rows
        got_mp, got_ap = e.dev.mul_plain(a, pt, level), e.dev.add_plain(a, pt, level)
        one = e.dev.mul_plain(a, pt[1], level)                                       # stride 0: one plaintext (a mask) for all
        for j in range(2):
            assert np.array_equal(got_mp[j], orc("orc_mul_plain", e.ring, a[j].shape, level, c64(a[j]), c64(pt[j]))), (name, level, j)
            assert np.array_equal(got_ap[j], orc("orc_add_plain", e.ring, a[j].shape, level, c64(a[j]), c64(pt[j]))), (name, level, j)
            assert np.array_equal(one[j], orc("orc_mul_plain", e.ring, a[j].shape, level, c64(a[j]), c64(pt[1]))), (name, level, j)
        if level > 0:
            got = e.dev.rescale(a, level)
            for j in range(2):
                assert np.array_equal(got[j], orc("orc_rescale", e.ring, (2, level, e.N), level, c64(a[j]))), (name, level, j)


@pytest.mark.parametrize("name", ORACLE_CHAINS)
def test_linear_operations_equal_the_oracle_and_python_integers(name):
    e = env(name)
    rnd = np.random.default_rng(3)
    for level in rc.levels(name):
        a, b = e.cts(level, 60 + level), e.cts(level, 70 + level)
        add, sub = e.dev.add(a, b, level), e.dev.sub(a, b, level)
        for j in range(2):
            assert np.array_equal(add[j], orc("orc_ct_addsub", e.ring, a[j].shape, level, c64(a[j]), c64(b[j]), 0))
            assert np.array_equal(sub[j], orc("orc_ct_addsub", e.ring, a[j].shape, level, c64(a[j]), c64(b[j]), 1))
        for sc in ([q - 1 for q in e.moduli[:level + 1]], [0] * (level + 1), [int(rnd.integers(0, q)) for q in e.moduli[:level + 1]]):
            mul, acc, adds = e.dev.mul_scalar(a, sc, level), e.dev.mul_scalar_add(a, sc, b, level), e.dev.add_scalar(a, sc, level)
            for m in range(level + 1):
                q, s = e.moduli[m], sc[m]
                A, B = ring_ref._obj(a[:, :, m].ravel()), ring_ref._obj(b[:, :, m].ravel())
                assert np.array_equal(ring_ref._obj(mul[:, :, m].ravel()), A * s % q), (name, level, m)
                assert np.array_equal(ring_ref._obj(acc[:, :, m].ravel()), (B + A * s) % q), (name, level, m)
                assert np.array_equal(ring_ref._obj(adds[:, 0, m].ravel()), (ring_ref._obj(a[:, 0, m].ravel()) + s) % q), (name, level, m)
                assert np.array_equal(adds[:, 1, m], a[:, 1, m])
        for lo in sorted({level, level // 2, 0}):
            assert np.array_equal(e.dev.drop_level(a, level, lo), a[:, :, :lo + 1])


@pytest.mark.parametrize("name", ["G12", "G13", "X12"])
def test_innersum_equals_the_oracle(name):
    e = env(name)
    k = 1
    while k < e.slots:
        e.need_galois(e.ring.galois(k))
        k *= 2
    for level in rc.levels(name):
        two = e.cts(level, 80 + level)
        want = orc("orc_innersum_all", e.ring, two[0].shape, e.keys.h, level, c64(two), 2)
        assert np.array_equal(e.dev.innersum(two, level), want), (name, level)


# ---------------------------------------------------------------- 19 moduli: the Python-integer key switch
@pytest.mark.parametrize("level", [16, 8])
def test_nineteen_moduli_rotation_and_mulrelin_equal_the_integer_model(level):
    """beta = 9 digits of two moduli (the last one short at both levels).  One key's words serve as rotation key and as relinearisation key, and the product's
    second operand has polynomial 1 = the constant 1 (all ones in the NTT domain), so that both operations switch the same polynomial and the integer model's
    key switch - the slow part - is computed once per level.  Parity needs no valid key."""
    e = env("L19")
    r, g = e.ring, e.ring.galois(e.slots - 1)
    key = capi.random_rotkey(e.moduli, r.beta, e.N, 19)
    e.dev.load_rotkey(g, key)
    e.dev.load_relinkey(key)
    rnd = np.random.default_rng(level)
    a = np.stack([np.stack([rnd.integers(0, q, e.N, dtype=np.uint64) for q in e.moduli[:level + 1]]) for _ in range(2)])
    b = a.copy()
    b[0] = a[1]
    b[1] = 1
    d0, d1 = ring_ref.keyswitch(r, level, a[1], key)
    idx = ring_ref.automorphism_index(r.logN, g)
    rot, mul = np.zeros_like(a), np.zeros_like(a)
    for m in range(level + 1):
        q = e.moduli[m]
        o = ring_ref._obj
        rot[0, m], rot[1, m] = ((o(d0[m]) + o(a[0, m])) % q).astype(np.uint64)[idx], d1[m][idx]
        mul[0, m] = ((o(a[0, m]) * o(b[0, m]) + o(d0[m])) % q).astype(np.uint64)
        mul[1, m] = ((o(a[0, m]) * o(b[1, m]) + o(a[1, m]) * o(b[0, m]) + o(d1[m])) % q).astype(np.uint64)
    assert np.array_equal(e.dev.rotate_right(a[None], level, [1])[0], rot)
    assert np.array_equal(e.dev.mulrelin(a[None], b[None], level)[0], mul)


# ---------------------------------------------------------------- PN14: both paths on the same parameters
def test_pn14_general_ring_and_specialised_context_give_identical_words():
    """random key words on both sides (parity needs no valid key); a ring of its own, so that the module's P14 ring keeps the oracle's keys"""
    logN, q, p = rc.chain("P14")
    e = env("P14")
    ctx, dev = capi.Context(q, p), capi.Ring(logN, q, p)
    try:
        gals = sorted({e.ring.galois(1 << i) for i in range(13)} | {e.ring.galois(e.slots - 5)})
        for g in gals:
            key = capi.random_rotkey(e.moduli, e.ring.beta, e.N, 900 + g)
            ctx.load_rotkey(g, key)
            dev.load_rotkey(g, key)
        rlk = capi.random_rotkey(e.moduli, e.ring.beta, e.N, 901)
        ctx.load_relinkey(rlk)
        dev.load_relinkey(rlk)
        for level in (9, 4):
            a, b = e.cts(level, 90 + level), e.cts(level, 95 + level)
            assert np.array_equal(dev.rotate_right(a, level, [5, 5]), ctx.rotate_right(a, level, [5, 5])), level
            prod_g, prod_c = dev.mulrelin(a, b, level), ctx.evalop("sfg_ct_mulrelin_dev", level, a, b)
            assert np.array_equal(prod_g, prod_c), level
            assert np.array_equal(dev.rescale(prod_g, level), ctx.evalop("sfg_ct_rescale_dev", level, prod_c, out_level=level - 1)), level
            assert np.array_equal(dev.innersum(a, level), ctx.innersum(a, level)), level
    finally:
        ctx.close()
        dev.close()


# ---------------------------------------------------------------- end to end
@pytest.mark.parametrize("name,scale", [("W15", 2.0 ** 40), ("X15", 2.0 ** 55)])
def test_end_to_end_rotate_square_rescale(name, scale):
    """encrypt with the oracle; rotate right by 1, square, rescale on the device; decrypt with the oracle.  The words equal the oracle's own run of the same
    sequence, so the slots carry exactly the oracle's noise, and that noise is held to 2^-16 of a unit slot.  Where the bound comes from (W15, the tighter
    case: scale 2^40, q_top about 2^40): a key switch leaves about 2^10 per coefficient (the oracle's own measurement, 354..1232); squaring multiplies it by
    twice the message polynomial, N coefficients of about 2^40 / sqrt(N / 2) each: sqrt(N) 2^33.5 2^10 2 = 2^52 at most per coefficient, 2^12 after the
    division by q_top; a slot sums N of them, sqrt(N) 2^12 = 2^19.5 for independent terms, four deviations 2^21.5, over the output scale 2^40: 2^-18.5.
    2^-16 leaves a factor of five."""
    e = env(name)
    r, top = e.ring, len(e.q) - 1
    e.need_right(1)
    rlk = e.need_rlk()
    rnd = np.random.default_rng(5)
    v = rnd.uniform(-1, 1, e.slots)
    ct = r.encrypt(e.s, top, r.encode_coeffs(v, scale), 99)
    want = ol.rotate_right(r, e.keys, top, ct, 1)
    want = orc("orc_mulrelin", r, want.shape, top, c64(want), c64(want), c64(rlk))
    want = orc("orc_rescale", r, (2, top, e.N), top, c64(want))
    rot = e.dev.rotate_right(ct[None], top, [1])
    got = e.dev.rescale(e.dev.mulrelin(rot, rot, top), top)[0]
    assert np.array_equal(got, want)
    out_scale = scale * scale / e.q[top]
    plain = np.roll(v, 1) ** 2

    def slots_of(c):
        return ring_ref.decode(ring_ref.crt_centered(r.decrypt_residues(e.s, top - 1, c), e.q[:top]), e.N, out_scale)
    err_dev, err_orc = np.max(np.abs(slots_of(got) - plain)), np.max(np.abs(slots_of(want) - plain))
    print(f"{name}: slot error device {err_dev:.3e}, oracle {err_orc:.3e}")
    assert err_dev <= err_orc and err_orc < 2.0 ** -16


# ---------------------------------------------------------------- refusals and key forms
def test_create_refuses_bad_parameters_with_the_cause():
    logN, q, p = rc.chain("G12")

    def refused(match, logN=logN, q=q, p=p, **kw):
        with pytest.raises(capi.SfgError, match=match):
            capi.Ring(logN, q, p, **kw).close()
    refused("logN must be 12..16", logN=11)
    refused("logN must be 12..16", logN=17)
    refused("bad modulus counts", q=[])
    refused("bad modulus counts", p=[])
    refused("bad modulus counts", q=q * 24, p=p)
    refused("modulus 1 must be < 2\\^61 and == 1 mod 2N", q=[q[0], (1 << 61) + 1])
    refused("modulus 0 must be < 2\\^61 and == 1 mod 2N", q=[q[0] + 2, q[1]])
    from sympy import isprime
    refused("modulus 1 is not prime", q=[q[0], next(x for x in range((1 << 30) + 1, 1 << 31, 8192) if not isprime(x))])          # == 1 mod 2N, composite
    refused("repeats modulus 0", q=[q[0], q[0]])
    refused("psi is not a primitive 2N-th root of unity", psi=[1, 1, 1])
    refused("bad device index", device=99)
    refused("bad device index", device=-1)


def test_calls_refuse_bad_arguments_with_the_cause():
    e = env("G12")
    dev, L = e.dev, capi.lib()
    top = len(e.q) - 1
    two = e.cts(top, 1)
    d_in, d_out = dev.to_device(two), dev.malloc(two.nbytes)
    one = (C.c_int * 2)(1, 1)
    sc = (C.c_uint64 * 2)(0, 0)

    def refused(match, rc_):
        assert rc_ == 1 and __import__("re").search(match, L.sfg_ring_last_error(dev.h).decode()), L.sfg_ring_last_error(dev.h).decode()
    try:
        for lvl in (-1, top + 1):
            refused("level -?\\d+ out of range 0..1", L.sfg_ring_rotate_right_dev(dev.h, d_in, d_out, 2, lvl, one))
            refused("level -?\\d+ out of range", L.sfg_ring_ct_add_dev(dev.h, d_in, d_in, d_out, 2, lvl))
            refused("level -?\\d+ out of range", L.sfg_ring_ct_mulrelin_dev(dev.h, d_in, d_in, d_out, 2, lvl))
            refused("level -?\\d+ out of range", L.sfg_ring_ct_rescale_dev(dev.h, d_in, d_out, 2, lvl))
            refused("level -?\\d+ out of range", L.sfg_ring_ct_innersum_dev(dev.h, d_in, 2, lvl, d_out))
            refused("level -?\\d+ out of range", L.sfg_ring_ct_mul_scalar_dev(dev.h, d_in, sc, d_out, 2, lvl))
        refused("level_out 2 out of range 0..1", L.sfg_ring_ct_drop_level_dev(dev.h, d_in, d_out, 2, top, top + 1))
        refused("negative ciphertext count", L.sfg_ring_rotate_right_dev(dev.h, d_in, d_out, -1, top, one))
        refused("negative ciphertext count", L.sfg_ring_ct_sub_dev(dev.h, d_in, d_in, d_out, -2, top))
        refused("negative row count", L.sfg_ring_ntt_rows(dev.h, d_in, -1, one))
        refused("modulus index 3 of row 1 out of range 0..2", L.sfg_ring_ntt_rows(dev.h, d_in, 2, (C.c_int * 2)(0, 3)))
        refused("in and out may not alias", L.sfg_ring_rotate_right_dev(dev.h, d_in, d_in, 2, top, one))
        refused("in and out may not alias", L.sfg_ring_ct_galois_dev(dev.h, d_in, d_in, 2, top, 5))
        refused("out may alias neither input", L.sfg_ring_ct_mulrelin_dev(dev.h, d_in, d_out, d_out, 2, top))
        refused("out may alias neither input", L.sfg_ring_ct_mulrelin_dev(dev.h, d_out, d_in, d_out, 2, top))
        g_missing = e.ring.galois(3)
        assert not dev.has_rotkey(g_missing)
        refused(f"no key loaded for galois element {g_missing}", L.sfg_ring_rotate_right_dev(dev.h, d_in, d_out, 2, top, (C.c_int * 2)(0, e.slots - 3)))
        g_other = next(g for g in range(3, 2 * e.N, 2) if not dev.has_rotkey(g))
        refused(f"no key loaded for galois element {g_other}", L.sfg_ring_ct_galois_dev(dev.h, d_in, d_out, 2, top, g_other))
        refused("not an odd number below 2N", L.sfg_ring_ct_galois_dev(dev.h, d_in, d_out, 2, top, 4))
        refused("cannot rescale at level 0", L.sfg_ring_ct_rescale_dev(dev.h, d_in, d_out, 2, 0))
        refused("needs at least one ciphertext", L.sfg_ring_ct_innersum_dev(dev.h, d_in, 0, top, d_out))
        refused("scalar 1 is not a canonical residue", L.sfg_ring_ct_mul_scalar_dev(dev.h, d_in, (C.c_uint64 * 2)(0, e.q[1]), d_out, 2, top))
        fresh = capi.Ring(e.logN, e.q, e.p)
        try:
            assert L.sfg_ring_ct_mulrelin_dev(fresh.h, d_in, d_in, d_out, 2, top) == 1 and "no relinearisation key loaded" in L.sfg_ring_last_error(fresh.h).decode()
            assert L.sfg_ring_ct_innersum_dev(fresh.h, d_in, 2, top, d_out) == 1 and "no key loaded for the left rotation by 1" in L.sfg_ring_last_error(fresh.h).decode()
        finally:
            fresh.close()
        assert L.sfg_ring_rotate_right_dev(dev.h, d_in, d_out, 0, top, one) == 0                      # an empty batch is no error
    finally:
        dev.free(d_in)
        dev.free(d_out)


def test_context_create_still_refuses_other_presets_with_its_message():
    logN, q, p = rc.chain("G12")
    with pytest.raises(capi.SfgError, match="only logN = 14 \\(PN14QP438\\) is built into this library"):
        capi.Context(q, p, logN=logN)
    with pytest.raises(capi.SfgError, match="modulus must be < 2\\^47"):
        capi.Context(rc.chain("W15")[1][:1] + list(ol.Q_PN14[1:]), ol.P_PN14)


def test_montgomery_form_key_loads_to_the_same_words():
    e = env("G12")
    top = len(e.q) - 1
    g = e.ring.galois(e.slots - 2)
    key = e.ring.gen_rotkey(e.s, g, 5)
    mont = np.zeros_like(key)
    for m, q in enumerate(e.moduli):
        mont[:, :, m] = (ring_ref._obj(key[:, :, m].ravel()) * ((1 << 64) % q) % q).astype(np.uint64).reshape(key[:, :, m].shape)
    two = e.cts(top, 3)
    e.dev.load_rotkey(g, mont, montgomery=True)
    got_m = e.dev.rotate_right(two, top, [2, 2])
    e.dev.load_rotkey(g, key)
    e.keys.add(g, key)
    assert np.array_equal(got_m, e.dev.rotate_right(two, top, [2, 2]))
    assert np.array_equal(got_m[0], ol.rotate_right(e.ring, e.keys, top, two[0], 2))
    rlk = e.need_rlk()
    rmont = np.zeros_like(rlk)
    for m, q in enumerate(e.moduli):
        rmont[:, :, m] = (ring_ref._obj(rlk[:, :, m].ravel()) * ((1 << 64) % q) % q).astype(np.uint64).reshape(rlk[:, :, m].shape)
    want = e.dev.mulrelin(two, two, top)
    e.dev.load_relinkey(rmont, montgomery=True)
    assert np.array_equal(e.dev.mulrelin(two, two, top), want)
    e.dev.load_relinkey(rlk)


# ---------------------------------------------------------------- the evaluator's chunk loops with a second chunk
# The ring's workspace budget is fixed (768 MiB), so a second chunk needs a batch beyond the chunk sizes tests/test_ring_ref.py pins on the CPU - the literals
# below, not read from the library: 1638 key switches at G12 level 0, 6144 rescales at G12 level 1.  Each batch tiles four distinct ciphertexts, so four oracle
# calls cover every output word: got[j] must equal the oracle's result for j % 4.  The launch splits at 16384 ciphertexts and 32768 rows would need gigabytes per
# operand; they are left to the CPU plan test (the X and U lines of tests/host/host_gring_test.cpp).
KS_CHUNK_G12_L0, RESCALE_CHUNK_G12_L1 = 1638, 6144


def four_cts(e, level, seed):
    return np.concatenate([e.cts(level, seed), e.cts(level, seed + 2)])


def assert_tiled(got, want4, what):
    t = got.reshape((-1, 4) + got.shape[1:])
    for k in range(4):
        bad = np.nonzero((t[:, k] != want4[k]).reshape(t.shape[0], -1).any(axis=1))[0]
        assert bad.size == 0, (what, k, "first wrong ciphertexts", (bad[:5] * 4 + k).tolist())


def test_rotation_across_the_chunk_boundary_equals_the_oracle():
    """2192 ciphertexts, amounts 0, 1, 7, 1 tiled: 1644 jobs, a second chunk of 6, and every job's ciphertext index differs from its job index past the first copy"""
    e = env("G12")
    nct, amounts = 2192, [0, 1, 7, 1]
    assert nct * 3 // 4 == KS_CHUNK_G12_L0 + 6
    e.need_right(*amounts)
    four = four_cts(e, 0, 110)
    got = e.dev.rotate_right(np.tile(four, (nct // 4, 1, 1, 1)), 0, amounts * (nct // 4))
    assert_tiled(got, [ol.rotate_right(e.ring, e.keys, 0, four[k], amounts[k]) for k in range(4)], "rotate_right")


def test_mulrelin_across_the_chunk_boundary_equals_the_oracle():
    e = env("G12")
    nct = 1640
    assert KS_CHUNK_G12_L0 < nct < 2 * KS_CHUNK_G12_L0
    rlk = e.need_rlk()
    a, b = four_cts(e, 0, 120), four_cts(e, 0, 130)
    got = e.dev.mulrelin(np.tile(a, (nct // 4, 1, 1, 1)), np.tile(b, (nct // 4, 1, 1, 1)), 0)
    assert_tiled(got, [orc("orc_mulrelin", e.ring, a[k].shape, 0, c64(a[k]), c64(b[k]), c64(rlk)) for k in range(4)], "mulrelin")


def test_rescale_across_the_chunk_boundary_equals_the_oracle():
    e = env("G12")
    nct = 6148
    assert RESCALE_CHUNK_G12_L1 < nct < 2 * RESCALE_CHUNK_G12_L1
    four = four_cts(e, 1, 140)
    got = e.dev.rescale(np.tile(four, (nct // 4, 1, 1, 1)), 1)
    assert_tiled(got, [orc("orc_rescale", e.ring, (2, 1, e.N), 1, c64(four[k])) for k in range(4)], "rescale")
