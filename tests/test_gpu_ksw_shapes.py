"""GPU parity of the hybrid key switch (rotate.hip: rotations, generic Galois elements, relinearisation) beyond the PN14 chain: one, three and
four special primes, eight digits, single-prime and short digits, 47-bit moduli throughout - on random ciphertexts and on directed ones
whose digit words sit where the float correction of the basis extension is off by one (tests/ksw_ref.py).  Every word against the oracle,
whose key switch test_ksw_ref.py pins against Python integers and by decryption at these shapes.  Random keys: parity needs no valid key."""
import numpy as np
import pytest

import ksw_ref as kr
import oracle_lib as ol

pytestmark = pytest.mark.gpu
ROTS = [3, 8191]                       # right rotations with a key; rotation 0 is the copy
CASES = [(name, level) for name in sorted(kr.CHAINS) for level in kr.CHAINS[name][2]]


def _env(name):
    """(context, ring, oracle keys) of a chain with the keys of ROTS, the conjugation and the relinearisation loaded on both sides"""
    from sfgwas_amd import capi
    ctx, ring = kr.gpu_env(name)
    if not hasattr(ctx, "ksw_keys"):
        keys = ol.RotKeys(ring)
        for j, g in enumerate([ring.galois(ring.slots - r) for r in ROTS] + [2 * ring.N - 1, 1]):
            key = capi.random_rotkey(ring.moduli, ring.beta, ring.N, 40 + j)
            keys.add(g, key)
            ctx.load_rotkey(g, key)
        ctx.ksw_keys = keys
    return ctx, ring, ctx.ksw_keys


def _cts(ring, level, kind, n, seed):
    if kind == "random":
        return np.stack([ring.fill_uniform(level, seed + j) for j in range(n)])
    return np.stack([kr.directed_ct(ring, level, seed + 7 * j) for j in range(n)])


def _galois(ctx, cts, level, g):
    from sfgwas_amd import capi
    d_in = ctx.to_device(cts); d_out = ctx.malloc(cts.nbytes)
    try:
        ctx.check(capi.lib().sfg_ct_galois_dev(ctx.h, d_in, d_out, cts.shape[0], level, g), "galois")
        return ctx.to_host(d_out, cts.shape, np.uint64)
    finally:
        ctx.free(d_in); ctx.free(d_out)


@pytest.mark.parametrize("kind", ["random", "directed"])
@pytest.mark.parametrize("name,level", CASES)
def test_rotations_bit_exact(name, level, kind):
    ctx, ring, keys = _env(name)
    nrots = ROTS + [0]
    cts = _cts(ring, level, kind, len(nrots), 100)
    got = ctx.rotate_right(cts, level, nrots)
    for j, r in enumerate(nrots):
        assert np.array_equal(got[j], ol.rotate_right(ring, keys, level, cts[j], r)), f"{name} level {level} ct {j} rot {r}"


@pytest.mark.parametrize("kind", ["random", "directed"])
@pytest.mark.parametrize("name,level", CASES)
def test_conjugation_bit_exact(name, level, kind):
    ctx, ring, keys = _env(name)
    g = 2 * ring.N - 1
    cts = _cts(ring, level, kind, 2, 200)
    got = _galois(ctx, cts, level, g)
    for j in range(2):
        want = np.zeros_like(cts[j])
        assert ol.lib().orc_apply_galois(ring.h, keys.h, level, ol.p64(cts[j]), g, ol.p64(want)) == 0
        assert np.array_equal(got[j], want), f"{name} level {level} ct {j}"


@pytest.mark.parametrize("kind", ["random", "directed"])
@pytest.mark.parametrize("name,level", CASES)
def test_mulrelin_bit_exact(name, level, kind):
    """directed: a1 is the directed polynomial and b1 the constant 1 (all ones in the NTT domain), so the switched term a1 * b1 is the directed one"""
    ctx, ring, keys = _env(name)
    a = _cts(ring, level, kind, 2, 300)
    b = np.stack([kr.directed_ct(ring, level, 350 + j, ones=True) if kind == "directed" else ring.fill_uniform(level, 350 + j) for j in range(2)])
    got = ctx.evalop("sfg_ct_mulrelin_dev", level, a, b)
    for j in range(2):
        want = np.zeros_like(a[j])
        ol.lib().orc_mulrelin(ring.h, level, ol.p64(a[j]), ol.p64(b[j]), ol.p64(keys.keys[1]), ol.p64(want))
        assert np.array_equal(got[j], want), f"{name} level {level} ct {j}"


@pytest.mark.parametrize("name", sorted(kr.CHAINS))
def test_zero_sum_rotation_gives_exact_zeros(name):
    """k_ksw_finish at canon()'s fix-up: c0 is chosen as the negative of what the key switch adds to it, so every word of output polynomial 0
    is 0 - computed as a lazy sum that is 0 or q, the latter in about half of the words, which on an ARM modulus only the equality test turns
    into 0 (a kernel without it returns q there)"""
    ctx, ring, keys = _env(name)
    level = max(kr.CHAINS[name][2])
    r = ROTS[0]
    idx = kr.automorphism_index(ring, ring.galois(ring.slots - r))
    assert np.array_equal(np.sort(idx), np.arange(ring.N))
    ct = kr.directed_ct(ring, level, 400)
    ct[0] = 0
    out0 = ctx.rotate_right(ct[None], level, [r])[0, 0]                     # out0[x] = d0[idx[x]]
    for m in range(level + 1):
        q = np.uint64(ring.moduli[m])
        ct[0, m, idx] = (q - out0[m]) % q
    got = ctx.rotate_right(ct[None], level, [r])[0]
    assert np.count_nonzero(got[0]) == 0, [int(np.count_nonzero(got[0, m])) for m in range(level + 1)]
    assert np.array_equal(got, ol.rotate_right(ring, keys, level, ct, r))


def test_nine_digits_are_refused_and_eight_still_work():
    """S1 at level 8 would need nine digits (KSW_MAXDIG = 8): refused by name, and the context is intact afterwards"""
    from sfgwas_amd.capi import SfgError
    ctx, ring, keys = _env("S1")
    with pytest.raises(SfgError, match="key-switch shape unsupported"):
        ctx.rotate_right(np.stack([ring.fill_uniform(8, 1)]), 8, [ROTS[0]])
    ct = ring.fill_uniform(7, 2)
    assert np.array_equal(ctx.rotate_right(ct[None], 7, [ROTS[1]])[0], ol.rotate_right(ring, keys, 7, ct, ROTS[1]))


def test_five_special_primes_make_a_context_that_refuses_to_switch():
    """np = 5 > KSW_MAXA: sfg_ctx_create takes the chain (the NTT, the MAC and the linear operations do not care), the key switch refuses it"""
    from sfgwas_amd import capi
    q, p = kr.S4[0][:2], kr.S4[1] + [kr.S3[1][2]]
    ctx = capi.Context(q, p)
    try:
        ring = ol.Ring(14, q, p)
        ctx.load_rotkey(ring.galois(ring.slots - 1), capi.random_rotkey(ring.moduli, ring.beta, ring.N, 1))
        with pytest.raises(capi.SfgError, match="key-switch shape unsupported"):
            ctx.rotate_right(np.stack([ring.fill_uniform(1, 1)]), 1, [1])
        rows = np.stack([np.arange(ring.N, dtype=np.uint64)])
        assert np.array_equal(ctx.ntt_rows(rows, [6]), ring.ntt(6, rows[0])[None])      # the refusal left the context usable
    finally:
        ctx.close()
