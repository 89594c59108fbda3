"""The general ring's products re-derive near-tie diagonal coefficients on the device (sfgwas_amd/csrc/gring_matmul.hip: k_gr_mm_tie; gring_tie.hpp), on the GPU:
directed near-ties through sfg_ring_matmul_dev on both sides of the tie and in both orientations, every word against the product composed with tests/exactref.py's
plaintext (and against the oracle's product, whose plaintext is then the same); the exact tie, still refused; ordinary data under a band widened by the test hook
on G12, with SFG_SQUARE on arbitrary int8 and on W16; the list's overflow; the hook's scope.  The arithmetic itself is held on the CPU (tests/test_ring_tie_ref.py).

A single 1 at (I, J) of the operand lies on the diagonal of shift (I - J) mod n, giant g = shift // d and baby b = shift % d, and lands in slot t0 = (J + g d) mod n
of the rotated diagonal.  place(t0, g, b) inverts that."""
import atexit
import ctypes as C
import os
import time

import numpy as np
import pytest

import exactref
import oracle_lib as ol
import ring_cases as rc
import ring_mm_cases as mc
import ring_ref
import ring_tie_ref as tr
from sfgwas_amd import capi

pytestmark = pytest.mark.gpu

SQ, TR = capi.SFG_SQUARE, capi.SFG_TRANSPOSE
GUARD = 4096
SENT = np.uint64(0xA5A5A5A5A5A5A5A5)
TIE_MSG = "coefficients lie within the proven band of a rounding tie"
_ENV = {}


class Env(mc.Party):
    def __init__(self, name):
        super().__init__(name)
        self.dev = capi.Ring(self.logN, self.q, self.p)

    def keys_for(self, nrow, ncol):
        self.need(ol.needed_rotations(self.slots, nrow, ncol)[0], self.dev.load_rotkey)


def g12():
    if "G12" not in _ENV:
        _ENV["G12"] = Env("G12")
    return _ENV["G12"]


@atexit.register
def _close_all():
    for e in _ENV.values():
        e.dev.close()
    _ENV.clear()


def place(n, d, t0, g, b):
    """(I, J) of the single entry whose diagonal (giant g, baby b) holds it in slot t0 after the rotation by g d"""
    J = (t0 - g * d) % n
    return (g * d + b + J) % n, J


def composed_with_exact_rows(e, A, level, L, p, g, b):
    """the product of a matrix whose only non-zero diagonal is (giant g, baby b) with plaintext coefficients p (Python integers): rotate_right, mul_plain by the
    transformed residues of p, rotate_right - the steps of ring_mm_cases.composed_product with exactref's rows in the place of the encoder's"""
    rows = np.array([[x % q for x in p] for q in e.q[:L]], dtype=np.uint64)
    pt = e.dev.ntt_rows(rows, list(range(L)))
    cur = np.ascontiguousarray(A[:, 0, :, :level + 1])
    s = A.shape[0]
    rot = (cur if b == 0 else e.dev.rotate_right(cur, level, [-b] * s))[:, :, :L]
    prod = e.dev.mul_plain(np.ascontiguousarray(rot), pt, L - 1)
    out = prod if g == 0 else e.dev.rotate_right(prod, L - 1, [-g * e.d] * s)
    return out[:, None]


# (t0, j, K, giant, baby, transposed): j below n and above it (the flagged pair is {j, N - j} either way), giants 44 and 2, both orientations
DIRECTED = [(5, 1, 2, 44, 3, 0), (17, 2049, 1, 44, 0, TR), (100, 4095, 3, 2, 3, 0), (7, 1000, 0, 44, 20, TR)]


@pytest.mark.parametrize("t0,j,K,g,b,flags", DIRECTED)
def test_directed_near_ties_are_resolved_to_exactrefs_plaintext_on_both_sides(t0, j, K, g, b, flags):
    """fails on a library without the resolver: the call is refused"""
    e = g12()
    n, N = e.slots, e.N
    I, J = place(n, e.d, t0, g, b)
    X = np.zeros((I + 1, J + 1), dtype=np.int8)
    X[I, J] = 1
    assert t0 != 0 and g != 0 and mc.diag_vector(X, n, 0, 0, g * e.d + b, g * e.d)[t0] == 1
    e.keys_for(*X.shape)
    geno = np.ascontiguousarray(X.T) if flags & TR else X
    A = mc.inputs(e.ring, 1, 1, 1, 4000 + t0)
    s0 = tr.directed_scale(N, t0, j, K)
    scales = [tr.step(s0, u) for u in tr.ULPS]
    v = np.zeros(n)
    v[t0] = 1.0
    sides = set()
    for scale, (p, tie, err) in zip(scales, exactref.encode_scaled(v, N, scales)):
        flagged = {int(c) for c in np.nonzero(tie <= 2.0 ** -50)[0]}
        assert flagged == {j, N - j} and min(tie[j], tie[N - j]) > err           # the reference alone: the intended pair, provably off the tie
        e.dev.encoder_resolved(reset=True)
        got = e.dev.matmul(A, 1, 2, geno, scale, flags)
        assert e.dev.encoder_resolved() == len(flagged)
        want = composed_with_exact_rows(e, A, 1, 2, p, g, b)
        assert got.shape == want.shape and np.array_equal(got, want), int(np.count_nonzero(got != want))
        assert np.array_equal(mc.orc_product(e.ring, e.keys, A, 1, 2, X, scale=scale), want)     # the oracle's plaintext is exactref's here
        sides.add(abs(p[j]))
    assert sides == {K, K + 1}


def guarded(dev, words):
    base = dev.to_device(np.full(words + 2 * GUARD, SENT, dtype=np.uint64))
    return base, C.c_void_p(base.value + GUARD * 8)


def refused_untouched(e, A, geno, scale, flags=0):
    """the product through the C entry point into a guard-banded sentinel buffer: -> (return code, message); asserts that no word was written"""
    L_ = capi.lib()
    nrow, ncol = geno.shape
    outw = A.shape[0] * mc.blocks(nrow if flags & TR else ncol, e.slots) * 2 * 2 * e.N
    dA, dG = e.dev.to_device(A), e.dev.to_device(geno)
    base, out = guarded(e.dev, outw)
    try:
        rc_ = L_.sfg_ring_matmul_dev(e.dev.h, dA, A.shape[0], 1, 2, dG, nrow, ncol, ncol, flags, scale, out)
        msg = L_.sfg_ring_last_error(e.dev.h).decode()
        if rc_:
            assert (e.dev.to_host(base, (outw + 2 * GUARD,)) == SENT).all()
        return rc_, msg
    finally:
        for p_ in (dA, dG, base):
            e.dev.free(p_)


def test_the_exact_tie_is_still_refused_and_out_is_untouched():
    e = g12()
    geno = np.ones((1, 1), dtype=np.int8)                                   # slot 0 of shift 0: p_0 = scale / n
    e.keys_for(1, 1)
    A = mc.inputs(e.ring, 1, 1, 1, 4100)
    e.dev.encoder_resolved(reset=True)
    rc_, msg = refused_untouched(e, A, geno, e.slots * 2.5)
    assert rc_ == 1 and "1 " + TIE_MSG in msg, msg
    assert e.dev.encoder_resolved() == 0
    # one ulp either side is resolved, to 2 and to 3
    for u, want_p0 in ((-1, 2), (1, 3)):
        scale = tr.step(e.slots * 2.5, u)
        v = np.zeros(e.slots)
        v[0] = 1.0
        p, tie, err = exactref.encode(v, e.N, scale)
        assert p[0] == want_p0 and {int(c) for c in np.nonzero(tie <= 2.0 ** -50)[0]} == {0}
        got = e.dev.matmul(A, 1, 2, geno, scale)
        assert np.array_equal(got, composed_with_exact_rows(e, A, 1, 2, p, 0, 0))
    assert e.dev.encoder_resolved(reset=True) == 2


def widened(dev, log2_floor, call):
    dev.set_tie_band_for_test(log2_floor)
    try:
        dev.encoder_resolved(reset=True)
        t = time.perf_counter()
        out = call()
        return out, dev.encoder_resolved(reset=True), time.perf_counter() - t
    finally:
        dev.set_tie_band_for_test(-50)


@pytest.mark.parametrize("flags", [0, SQ], ids=["plain", "square"])
def test_g12_full_block_under_a_band_of_2_to_minus_16_equals_the_unwidened_product(flags):
    """2048 diagonals of 4096 coefficients, each inside 2^-16 of a tie with probability 2^-15: about 256 re-derivations, some six in each of the 45 batches (one giant's
    46 diagonals each), every one of which must give the value the double-double encoder had proven anyway.  SFG_SQUARE on arbitrary int8: negative slot values."""
    e = g12()
    e.keys_for(2048, 2048)
    geno = np.random.default_rng(3).integers(-128, 128, (2048, 2048)).astype(np.int8) if flags & SQ else mc.geno_matrix(2048, 2048, 2)
    if flags & SQ:
        assert (mc.operand(geno, flags) < 0).any()
    A = mc.inputs(e.ring, 1, 1, 1, 4200)
    e.dev.encoder_resolved(reset=True)
    t = time.perf_counter()
    plain = e.dev.matmul(A, 1, 2, geno, mc.SCALE, flags)
    t_plain = time.perf_counter() - t
    assert e.dev.encoder_resolved() == 0
    wide, resolved, t_wide = widened(e.dev, -16, lambda: e.dev.matmul(A, 1, 2, geno, mc.SCALE, flags))
    print(f"G12 2048 x 2048 flags {flags}: resolved {resolved}, unwidened {t_plain * 1e3:.1f} ms, widened {t_wide * 1e3:.1f} ms (host round trips included)")
    assert np.array_equal(wide, plain)
    assert resolved >= 64


def test_w16_one_row_under_a_band_of_2_to_minus_16_equals_the_unwidened_product():
    """n = 32768, d = 182, scale 2^45: the largest table and the tightest margin (S 2^-191 with S up to 2^46).  A 1 x 300 matrix has 300 diagonals of one entry each;
    uniform keys (parity needs no valid key), device against device."""
    logN, q, p = rc.chain("W16")
    dev = capi.Ring(logN, q, p)
    try:
        ring = ring_ref.SplitRing(logN, q, p)
        assert dev.slots == 32768 and mc.d_of(dev.slots) == 182
        for k in mc.rotations(1, 300, dev.slots):
            gk = ring.galois(k)
            dev.load_rotkey(gk, ring_ref.uniform_key(ring, 700 + k))
        geno = mc.geno_matrix(1, 300, 61)
        A = np.stack([np.stack([ring_ref.uniform_ct(ring, 2, 62)])])
        dev.encoder_resolved(reset=True)
        plain = dev.matmul(A, 2, 3, geno, 2.0 ** 45)
        assert dev.encoder_resolved() == 0
        wide, resolved, _ = widened(dev, -16, lambda: dev.matmul(A, 2, 3, geno, 2.0 ** 45))
        print(f"W16 1 x 300: resolved {resolved}")
        assert np.array_equal(wide, plain)
        assert resolved >= 64
    finally:
        dev.close()


def test_a_list_that_overflows_refuses_the_call_as_unproven():
    """a band of 2^-6 flags one coefficient in 32: a batch of a hundred dense diagonals passes the list's 512 entries many times over"""
    e = g12()
    e.keys_for(100, 100)
    geno = mc.geno_matrix(100, 100, 9)
    A = mc.inputs(e.ring, 1, 1, 1, 4300)
    e.dev.set_tie_band_for_test(-6)
    try:
        rc_, msg = refused_untouched(e, A, geno, mc.SCALE)
    finally:
        e.dev.set_tie_band_for_test(-50)
    assert rc_ == 1 and TIE_MSG in msg, msg
    assert np.array_equal(e.dev.matmul(A, 1, 2, geno, mc.SCALE), mc.orc_product(e.ring, e.keys, A, 1, 2, geno))     # and the ring is as it was


def test_the_hook_leaves_the_vector_encoder_alone_and_is_refused_without_the_switch():
    e = g12()
    n = e.slots
    v = np.random.default_rng(17).uniform(-3, 3, (2, n))
    tie = np.full((1, n), 5.5 / 2.0 ** 30)                                  # p_0 = 5 + 1/2 exactly
    e.dev.encoder_resolved(reset=True)
    before = e.dev.encode_vectors(v, 1, 2.0 ** 30)
    with pytest.raises(capi.SfgError, match="1 " + TIE_MSG):
        e.dev.encode_vectors(tie, 1, 2.0 ** 30)
    e.dev.set_tie_band_for_test(-6)
    try:
        assert np.array_equal(e.dev.encode_vectors(v, 1, 2.0 ** 30), before)          # 2^-6 would flag a thirty-second of these coefficients
        with pytest.raises(capi.SfgError, match="1 " + TIE_MSG):
            e.dev.encode_vectors(tie, 1, 2.0 ** 30)
        for bad in (-51, -1, 0, 7):
            with pytest.raises(capi.SfgError, match="outside 2\\^-50"):
                e.dev.set_tie_band_for_test(bad)
    finally:
        e.dev.set_tie_band_for_test(-50)
    assert e.dev.encoder_resolved() == 0
    saved = os.environ.pop("SFG_ENABLE_TEST_HOOKS", None)
    try:
        plain = capi.Ring(e.logN, e.q, e.p)
    finally:
        if saved is not None:
            os.environ["SFG_ENABLE_TEST_HOOKS"] = saved
    try:
        with pytest.raises(capi.SfgError, match="sfg_ring_set_tie_band_for_test: test hook, enabled only"):
            plain.set_tie_band_for_test(-16)
        assert plain.encoder_resolved(reset=True) == 0                       # the counter is no hook
    finally:
        plain.close()
