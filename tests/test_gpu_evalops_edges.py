"""GPU tests of the evaluator operations (evalops.hip, k_ct_add, k_drop_level) at the words random data never holds: sums that are exactly q,
differences that are exactly 0, the rescale's two wrap-arounds - and the first parity tests of sfg_ct_mul_scalar_add_dev and
sfg_ct_drop_level_dev.  On PN14 at level 7 (modulus 7 is the one PN14 modulus where canon()'s fix-up is reachable) and on the all-47-bit
chain S4.  Expected values are Python integers or the oracle."""
import numpy as np
import pytest

import ksw_ref as kr
import oracle_lib as ol

pytestmark = pytest.mark.gpu
L = ol.lib
LEVEL = 7
CHAINS = ["PN14", "S4"]


def _rows(ring, level, seed, n=1):
    """[n][2][level+1][N] uniformly random canonical words"""
    return np.stack([ring.fill_uniform(level, seed + j) for j in range(n)])


def _qcol(ring, level):
    """the moduli broadcast over [.., level+1, N] as Python integers"""
    return np.array(ring.moduli[:level + 1], dtype=object)[:, None]


def _u64(a):
    return np.ascontiguousarray(np.asarray(a, dtype=object).astype(np.uint64))


def _mul_scalar_add(ctx, ct, scalars, acc, level):
    from sfgwas_amd import capi
    d_ct, d_acc = ctx.to_device(ct), ctx.to_device(acc)
    try:
        sc = np.ascontiguousarray(scalars, dtype=np.uint64)
        ctx.check(capi.lib().sfg_ct_mul_scalar_add_dev(ctx.h, d_ct, capi.p64(sc), d_acc, ct.shape[0], level), "mul_scalar_add")
        return ctx.to_host(d_acc, acc.shape, np.uint64)
    finally:
        ctx.free(d_ct); ctx.free(d_acc)


# ---------------------------------------------------------------- first parity tests of two entry points
@pytest.mark.parametrize("name", CHAINS)
def test_mul_scalar_add_accumulates_in_place(name):
    """acc += ct * c[m] for c = 0, 1, q - 1 and random residues, mixed over the moduli and each alone: (a * c + acc) % q in Python integers"""
    ctx, ring = kr.gpu_env(name)
    mods = ring.moduli[:LEVEL + 1]
    ct, acc = _rows(ring, LEVEL, 500, 2), _rows(ring, LEVEL, 510, 2)
    rnd = np.random.default_rng(1)
    kinds = [lambda q: 0, lambda q: 1, lambda q: q - 1, lambda q: int(rnd.integers(2, q - 1))]
    sets = [[kinds[k](q) for q in mods] for k in range(4)] + [[kinds[(m + 1) % 4](q) for m, q in enumerate(mods)]]
    for sc in sets:
        got = _mul_scalar_add(ctx, ct, sc, acc, LEVEL)
        want = (ct.astype(object) * np.array(sc, dtype=object)[:, None] + acc.astype(object)) % _qcol(ring, LEVEL)
        assert np.array_equal(got, _u64(want)), [hex(c) for c in sc]
    from sfgwas_amd.capi import SfgError
    with pytest.raises(SfgError, match="not canonical"):
        _mul_scalar_add(ctx, ct, [mods[0]] + [0] * LEVEL, acc, LEVEL)


@pytest.mark.parametrize("name", CHAINS)
@pytest.mark.parametrize("level_out", [7, 4, 0])
def test_drop_level_keeps_the_first_rows(name, level_out):
    from sfgwas_amd import capi
    ctx, ring = kr.gpu_env(name)
    cts = _rows(ring, LEVEL, 520, 3)
    d_in = ctx.to_device(cts); d_out = ctx.malloc(3 * 2 * (level_out + 1) * ring.N * 8)
    try:
        ctx.check(capi.lib().sfg_ct_drop_level_dev(ctx.h, d_in, d_out, 3, LEVEL, level_out), "drop_level")
        got = ctx.to_host(d_out, (3, 2, level_out + 1, ring.N), np.uint64)
        assert np.array_equal(got, cts[:, :, :level_out + 1])
        with pytest.raises(capi.SfgError, match="DropLevel"):
            ctx.check(capi.lib().sfg_ct_drop_level_dev(ctx.h, d_in, d_out, 3, level_out, LEVEL + 1), "drop_level")
    finally:
        ctx.free(d_in); ctx.free(d_out)


# ---------------------------------------------------------------- planted equalities: the result is 0, never q
@pytest.mark.parametrize("name", CHAINS)
def test_tensor_middle_term_at_exactly_q(name):
    """a = (1, 1), b = (q - v, v): the middle term a0 b1 + a1 b0 is v + (q - v) = q in every word (k_tensor's s >= q at s == q).  With an
    all-zero relinearisation key the key switch adds nothing, so polynomial 1 of the product IS the middle term; with a random key the whole
    product is the oracle's"""
    from sfgwas_amd import capi
    ctx, ring = kr.gpu_env(name)
    q = _qcol(ring, LEVEL)
    v = _rows(ring, LEVEL, 530)[0, 0].astype(object)
    v[v == 0] = 1
    a = np.ones((1, 2, LEVEL + 1, ring.N), dtype=np.uint64)
    b = _u64(np.stack([q - v, v]))[None]
    zero = np.zeros((ring.beta, 2, len(ring.moduli), ring.N), dtype=np.uint64)
    rlk = capi.random_rotkey(ring.moduli, ring.beta, ring.N, 44)
    try:
        ctx.load_relinkey(zero)
        got = ctx.evalop("sfg_ct_mulrelin_dev", LEVEL, a, b)
        assert np.count_nonzero(got[0, 1]) == 0
        assert np.array_equal(got[0, 0], b[0, 0])                                # a0 * b0 = q - v
        ctx.load_relinkey(rlk)
        got = ctx.evalop("sfg_ct_mulrelin_dev", LEVEL, a, b)
        want = np.zeros_like(a[0])
        L().orc_mulrelin(ring.h, LEVEL, ol.p64(a[0]), ol.p64(b[0]), ol.p64(rlk), ol.p64(want))
        assert np.array_equal(got[0], want)
    finally:
        if hasattr(ctx, "ksw_keys"):                                              # the key test_gpu_ksw_shapes.py shares this context with
            ctx.load_relinkey(ctx.ksw_keys.keys[1])


@pytest.mark.parametrize("name", CHAINS)
def test_add_family_at_exactly_q(name):
    """ct + ct, ct + plaintext and ct + scalar with a + b == q in every word: 0 everywhere, never q"""
    ctx, ring = kr.gpu_env(name)
    q = _qcol(ring, LEVEL)
    a = _rows(ring, LEVEL, 540)
    a[a == 0] = 1
    neg = _u64(q - a.astype(object))
    got = ctx.evalop("sfg_ct_add_dev", LEVEL, a, neg)
    assert np.count_nonzero(got) == 0
    got = ctx.evalop("sfg_ct_add_plain_dev", LEVEL, a, np.ascontiguousarray(neg[:, 0]), extra=((LEVEL + 1) * ring.N,))
    assert np.count_nonzero(got[:, 0]) == 0 and np.array_equal(got[:, 1], a[:, 1])
    sc = [int(x) for x in a[0, 0, :, 0]]                                           # one residue per modulus; polynomial 0 = q - that residue
    flat = np.empty_like(a)
    flat[0, 0] = _u64(q - np.array(sc, dtype=object)[:, None] + np.zeros((1, ring.N), dtype=object))
    flat[0, 1] = a[0, 1]
    got = ctx.evalop("sfg_ct_add_scalar_dev", LEVEL, flat, extra=(sc,))
    assert np.count_nonzero(got[:, 0]) == 0 and np.array_equal(got[:, 1], a[:, 1])


@pytest.mark.parametrize("name", CHAINS)
def test_sub_at_equal_operands_and_at_the_largest_borrow(name):
    ctx, ring = kr.gpu_env(name)
    a = _rows(ring, LEVEL, 550)
    assert np.count_nonzero(ctx.evalop("sfg_ct_sub_dev", LEVEL, a, a.copy())) == 0
    qm1 = _u64(_qcol(ring, LEVEL) - 1 + np.zeros((1, 2, LEVEL + 1, ring.N), dtype=object))
    got = ctx.evalop("sfg_ct_sub_dev", LEVEL, np.zeros_like(a), qm1)                 # 0 - (q - 1) = 1
    assert np.array_equal(got, np.ones_like(a))
    got = ctx.evalop("sfg_ct_sub_dev", LEVEL, a, qm1)                                # x - (q - 1) = x + 1 mod q
    assert np.array_equal(got, _u64((a.astype(object) + 1) % _qcol(ring, LEVEL)))


@pytest.mark.parametrize("name", CHAINS)
def test_mul_scalar_add_at_exactly_q(name):
    """acc = q - (ct * c mod q) with a non-zero product: the sum is q in every word and has to come out 0"""
    ctx, ring = kr.gpu_env(name)
    q = _qcol(ring, LEVEL)
    ct = _rows(ring, LEVEL, 560)
    ct[ct == 0] = 1
    sc = [int(np.random.default_rng(2).integers(1, qm)) for qm in ring.moduli[:LEVEL + 1]]
    prod = ct.astype(object) * np.array(sc, dtype=object)[:, None] % q
    assert np.all(prod != 0)
    got = _mul_scalar_add(ctx, ct, sc, _u64(q - prod), LEVEL)
    assert np.count_nonzero(got) == 0


# ---------------------------------------------------------------- rescale at its two wrap-arounds
@pytest.mark.parametrize("name", CHAINS)
def test_rescale_at_the_wraps_of_the_last_row(name):
    """the last row, in the coefficient domain, cycles over t = 0 (w == q_m in k_rescale_prep), 1, half, half + 1 (t + half == qL), half + 2,
    qL - 1 and every t with (t + half) mod qL a non-zero multiple of some q_m below qL; the other rows are random.  Against orc_rescale."""
    ctx, ring = kr.gpu_env(name)
    mods = ring.moduli
    qL = mods[LEVEL]
    half = (qL - 1) // 2
    ts = [0, 1, half, half + 1, half + 2, qL - 1]
    ts += [(k * qm - half) % qL for qm in mods[:LEVEL] for k in (1, 2, 3) if k * qm < qL]
    assert len(ts) > 6 and all(0 <= t < qL for t in ts)
    cts = _rows(ring, LEVEL, 570, 2)
    for j in range(2):
        for p in range(2):
            cts[j, p, LEVEL] = ring.ntt(LEVEL, kr.directed_rows([qL], ts, ring.N, shift=3 * j + p)[0])
    got = ctx.evalop("sfg_ct_rescale_dev", LEVEL, cts, out_level=LEVEL - 1)
    for j in range(2):
        want = np.zeros((2, LEVEL, ring.N), dtype=np.uint64)
        L().orc_rescale(ring.h, LEVEL, ol.p64(np.ascontiguousarray(cts[j])), ol.p64(want))
        assert np.array_equal(got[j], want), f"ct {j}"
