"""The general ring's key switch, ModDown and rescale on the GPU (sfgwas_amd/csrc/gring.hip) at the float boundaries of the basis extension and on wide chains,
every output word against the oracle where it holds the chain and against the Python-integer model of tests/ring_ref.py where it does not.

What tests/test_gpu_ring.py's uniform words and five directed rows cannot reach, and what is run here:
  * k_gr_ext_v's float sum ON an integer: directed ciphertexts whose digit words are X = k, D - k, D // 2 (ring_ref.directed_ct), rotated and multiplied under a
    uniform key on the chains of ring_cases.EDGE_KS - tests/test_ring_edges_ref.py asserts from the model's trace that every multi-modulus digit of these runs has
    words where the float v is the exact one and words where it is one above, every digit of four moduli also one below, and that a model which multiplies by
    fl(1/q), rounds v or takes v exact gives other words;
  * ModDown's own float sum on both boundaries: the same ciphertexts under ring_ref.identity_key (EDGE_MODDOWN), rotated and conjugated;
  * the 128-bit sums at their ceilings: M48's 47 digits under a uniform key, and under the planted key and input that drive the unreduced key sum above 2^127;
    A48's single ModDown digit of 47 moduli;
  * the real presets' digit shapes at 61 bits: R21 (6 digits of 3; 3, 3, 3, 1 at level 9) and R38 (8 digits of 4 and one of 2);
  * the rescale where the dropped modulus is 2^31 times a remaining one (V12) and on 47 rows (M48), the last row on the rounding boundary (q_L - 1) / 2;
  * V12's raw-copy digits 61 -> 30 and 61 -> 45 bits.
One device ring and one reference ring per chain for the module; the keys and ciphertexts are those of the CPU file (same seeds)."""
import atexit

import numpy as np
import pytest

import oracle_lib as ol
import ring_cases as rc
import ring_ref as rr
from sfgwas_amd import capi

pytestmark = pytest.mark.gpu

KEY_SEED, CT_SEED = rr.KEY_SEED, rr.CT_SEED

_ENV = {}


class Env:
    def __init__(self, name):
        self.name = name
        self.logN, self.q, self.p = rc.chain(name)
        self.ring = rr.chain_ring(name)
        self.dev = capi.Ring(self.logN, self.q, self.p)
        self.N, self.slots, self.moduli = self.ring.N, self.ring.N // 2, self.ring.moduli
        self.oracle = isinstance(self.ring, ol.Ring)                  # the oracle holds the chain: its own key switch is the reference
        self.keys = ol.RotKeys(self.ring) if self.oracle else None
        self.uniform = rr.uniform_key(self.ring, KEY_SEED)

    def galois_right(self, k):
        g = self.ring.galois(self.slots - k)
        assert g == self.dev.galois(self.slots - k)
        return g

    def load(self, g, key):
        self.dev.load_rotkey(g, key)
        if self.oracle:
            self.keys.add(g, key)

    def two(self, level):
        """[uniform, directed]"""
        return np.stack([rr.uniform_ct(self.ring, level, CT_SEED + 1), rr.directed_ct(self.ring, level, CT_SEED)])

    def galois_want(self, level, ct, g, key):
        """one ciphertext under each of the galois elements g (a list) with the same key: one key switch where the model computes it"""
        if self.oracle:
            out = []
            for gi in g:
                want = np.zeros_like(ct)
                assert ol.lib().orc_apply_galois(self.ring.h, self.keys.h, level, ol.p64(np.ascontiguousarray(ct)), gi, ol.p64(want)) == 0
                out.append(want)
            return out
        d0, d1 = rr.keyswitch(self.ring, level, ct[1], key)
        return [rr.galois_from_switch(self.ring, level, ct, d0, d1, gi) for gi in g]

    def rotation_and_product_want(self, level, a, b0, g, key):
        if not self.oracle:
            return rr.rotation_and_product_model(self.ring, level, a, b0, g, key)
        b = np.stack([b0, np.ones_like(b0)])
        mul = np.zeros_like(a)
        ol.lib().orc_mulrelin(self.ring.h, level, ol.p64(np.ascontiguousarray(a)), ol.p64(b), ol.p64(np.ascontiguousarray(key)), ol.p64(mul))
        return self.galois_want(level, a, [g], key)[0], mul


def env(name):
    if name not in _ENV:
        _ENV[name] = Env(name)
    return _ENV[name]


@atexit.register
def _close_all():
    for e in _ENV.values():
        e.dev.close()
    _ENV.clear()


def rotation_and_product(e, level, cts, key):
    """rotate_right by 1 and mulrelin of every ciphertext of cts, `key` serving as the rotation key and as the relinearisation key; the product's partner has
    polynomial 1 = all ones (the NTT of the constant 1), so that a1 b1 is the ciphertext's own polynomial 1 and both operations switch the directed words"""
    g = e.galois_right(1)
    e.load(g, key)
    e.dev.load_relinkey(key)
    partners = cts[:, ::-1].copy()                                # polynomial 0 of the partner: the ciphertext's polynomial 1
    partners[:, 1] = 1
    rot = e.dev.rotate_right(cts, level, [1] * len(cts))
    mul = e.dev.mulrelin(cts, partners, level)
    for j, ct in enumerate(cts):
        want_rot, want_mul = e.rotation_and_product_want(level, ct, partners[j, 0], g, key)
        assert np.array_equal(rot[j], want_rot), (e.name, level, j, "rotate_right")
        assert np.array_equal(mul[j], want_mul), (e.name, level, j, "mulrelin")


# ---------------------------------------------------------------- the digits' float sums on their boundaries; V12's raw copies; A48's ModDown digit
@pytest.mark.parametrize("name,level", rc.EDGE_KS)
def test_directed_rotation_and_product_under_a_uniform_key(name, level):
    e = env(name)
    rotation_and_product(e, level, e.two(level), e.uniform)


# ---------------------------------------------------------------- ModDown's float sum on its boundaries
@pytest.mark.parametrize("name,level", rc.EDGE_MODDOWN)
def test_directed_rotation_and_conjugation_under_the_identity_key(name, level):
    """the P rows are +-X0 extended to P: words k and P - k in both planes (A48: k in plane 0, P - k in plane 1)"""
    e = env(name)
    key = rr.identity_key(e.ring)
    g, conj = e.galois_right(2), 2 * e.N - 1
    e.load(g, key)
    e.load(conj, key)
    cts = e.two(level)
    rot, cj = e.dev.rotate_right(cts, level, [2, 2]), e.dev.apply_galois(cts, level, conj)
    for j, ct in enumerate(cts):
        want_rot, want_cj = e.galois_want(level, ct, [g, conj], key)
        assert np.array_equal(rot[j], want_rot), (name, level, j, "rotate_right")
        assert np.array_equal(cj[j], want_cj), (name, level, j, "conjugation")


# ---------------------------------------------------------------- the key sum's ceiling
def test_m48_top_level_under_a_uniform_key():
    """47 single-modulus digits, each a raw copy to 47 other moduli; 47 uniform products of 122 bits in each 128-bit sum"""
    e = env("M48")
    rotation_and_product(e, 46, rr.uniform_ct(e.ring, 46, CT_SEED)[None], e.uniform)


def test_m48_top_level_at_the_planted_maximum():
    """every input row and every key row all q - 1: the unreduced sums reach 47 (q - 1)^2 > 2^127.5 and pass 2^125 in 38 of the 48 rows
    (tests/test_ring_edges_ref.py asserts it on the model's sums)"""
    e = env("M48")
    cx, key = rr.planted_maximum(e.ring, 46)
    rotation_and_product(e, 46, np.stack([cx, cx])[None], key)


# ---------------------------------------------------------------- rescale
@pytest.mark.parametrize("name,level", rc.EDGE_RESCALE)
def test_rescale_with_the_last_row_on_the_rounding_boundary(name, level):
    """uniform words, and a last row that is the NTT of 0, 1, h - 1, h, h + 1, q_L - 2, q_L - 1, h = (q_L - 1) / 2.  V12 at level 1 drops the 61-bit modulus onto the
    30-bit one (k_gr_rescale_prep reduces a word 2^31 times its modulus), at level 2 the 45-bit one; M48 at level 46 leaves 46 rows"""
    e = env(name)
    cts = np.stack([rr.uniform_ct(e.ring, level, CT_SEED + 2), rr.boundary_last_row(e.ring, level, rr.uniform_ct(e.ring, level, CT_SEED + 3))])
    got = e.dev.rescale(cts, level)
    for j, ct in enumerate(cts):
        assert np.array_equal(got[j], rr.rescale_model(e.ring, level, ct)), (name, level, j)
        if e.oracle:
            want = np.zeros((2, level, e.N), dtype=np.uint64)
            ol.lib().orc_rescale(e.ring.h, level, ol.p64(np.ascontiguousarray(ct)), ol.p64(want))
            assert np.array_equal(got[j], want), (name, level, j, "oracle")
