"""The field arithmetic of csrc/beaver.hip at its rare carries: Beaver local products (B1-B3, mpc/beavermult.go:94-147) and the SSToCMat share
algebra (mpc/ss.go:84-110) on directed operands - the third pseudo-Mersenne fold, the final t >= p subtraction, sums equal to p, carries out
of the top word, every bit length B mod 32 the run-time funnel shift serves, both limb counts, the second pass of the grid-stride loops, the
device entry point and the NULL-pointer calling forms.  Expected values are Python integers on every element (tests/field_ref.py); the
oracle is a second witness.  tests/test_field_ref.py shows on the CPU that these operands reach those branches."""
import ctypes as C
import random
from functools import lru_cache

import numpy as np
import pytest

import field_ref as fr
import oracle_lib as ol

pytestmark = pytest.mark.gpu

DEV_MODULI = [(2, (1 << 127) - 1), (4, (1 << 255) - 19)]           # also through sfg_beaver_elem_dev
GRID_N = fr.GRID_N                                                  # 8192 * 256 + 300: 300 elements get a second pass of the grid-stride loops


@pytest.fixture(scope="module")
def ctx():
    from sfgwas_amd import capi
    c = capi.Context(ol.Q_PN14, ol.P_PN14)
    yield c
    c.close()


def p64(a):
    from sfgwas_amd import capi
    return None if a is None else capi.p64(a)


def modarr(p, limbs):
    return fr.to_limbs([p], limbs)[0].copy()


def last_error(ctx):
    from sfgwas_amd import capi
    return capi.lib().sfg_last_error(ctx.h).decode()


def assert_words(got, want_ints, limbs, what, explain=None):
    """every word of got equals the Python integers; on a mismatch name the first element (and what explain(i) knows about it)"""
    want = fr.to_limbs(want_ints, limbs)
    if not np.array_equal(got, want):
        i = int(np.nonzero((got != want).any(axis=1))[0][0])
        raise AssertionError(f"{what}: element {i}: got {fr.from_limbs(got[i:i + 1])[0]:#x}, want {want_ints[i]:#x}" + (f" ({explain(i)})" if explain else ""))


@lru_cache(maxsize=2)
def elem_inputs(limbs, p):
    quads = list(fr.directed_quadruples(p)) + fr.random_quadruples(p)
    return quads, [fr.to_limbs([q[j] for q in quads], limbs) for j in range(4)]


def beaver_elem_dev(ctx, pid, limbs, p, arrs, n, guard=8):
    """sfg_beaver_elem_dev on device buffers; the output buffer carries `guard` elements of a pattern past its end, which must survive"""
    from sfgwas_amd import capi
    dev = [ctx.to_device(a) for a in arrs]
    pattern = np.full((guard, limbs), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    d_out = ctx.malloc((n + guard) * limbs * 8)
    tail = C.c_void_p(d_out.value + n * limbs * 8)
    ctx.check(capi.lib().sfg_memcpy_h2d(ctx.h, tail, pattern.ctypes.data_as(C.c_void_p), pattern.nbytes), "h2d")
    ctx.check(capi.lib().sfg_beaver_elem_dev(ctx.h, pid, limbs, capi.p64(modarr(p, limbs)), *dev, d_out, n), "beaver_elem_dev")
    got = ctx.to_host(d_out, (n + guard, limbs), np.uint64)
    for d in dev + [d_out]:
        ctx.free(d)
    assert np.array_equal(got[n:], pattern), "beaver_elem_dev wrote past its n elements"
    return got[:n]


# ---------------------------------------------------------------- element-wise products, directed
@pytest.mark.parametrize("pid", [0, 1, 2])
@pytest.mark.parametrize("limbs,p", fr.ALL_MODULI, ids=[fr.mod_id(m) for m in fr.ALL_MODULI])
def test_beaver_elem_directed(ctx, limbs, p, pid):
    """all directed quadruples + 3 000 random ones through sfg_beaver_elem: every word against Python integers and against the oracle"""
    from sfgwas_amd import capi
    quads, arrs = elem_inputs(limbs, p)
    n = len(quads)
    mod = modarr(p, limbs)
    want = [fr.expected(pid, p, *q) for q in quads]
    explain = lambda i: f"quadruple {[hex(v) for v in quads[i]]}, model classes {sorted(fr.model_beaver(pid, limbs, p, *quads[i])[1])}"
    got = np.zeros((n, limbs), dtype=np.uint64)
    ctx.check(capi.lib().sfg_beaver_elem(ctx.h, pid, limbs, p64(mod), *[p64(a) for a in arrs], p64(got), n), "beaver_elem")
    assert_words(got, want, limbs, "sfg_beaver_elem", explain)
    orc = np.zeros((n, limbs), dtype=np.uint64)
    ol.lib().orc_beaver_elem(pid, limbs, ol.p64(mod), *[ol.p64(a) for a in arrs], ol.p64(orc), n)
    assert np.array_equal(got, orc)
    if pid == 0:                                            # the dealer's form (beavermult_hip.go): no ar, no br
        null = np.zeros((n, limbs), dtype=np.uint64)
        ctx.check(capi.lib().sfg_beaver_elem(ctx.h, 0, limbs, p64(mod), None, p64(arrs[1]), None, p64(arrs[3]), p64(null), n), "beaver_elem (NULL ar, br)")
        assert np.array_equal(null, got)
    if (limbs, p) in DEV_MODULI:
        assert_words(beaver_elem_dev(ctx, pid, limbs, p, arrs, n), want, limbs, "sfg_beaver_elem_dev", explain)


# ---------------------------------------------------------------- grid-stride loops: a second pass
def tiled(block_ints, limbs, n):
    return np.resize(fr.to_limbs(block_ints, limbs), (n, limbs))           # rows repeat cyclically


@pytest.mark.parametrize("limbs,p", DEV_MODULI + [(2, (1 << 127) - (1 << 40) - 1)], ids=["L2-folded", "L4-folded", "L2-generic"])
def test_beaver_elem_grid_stride(ctx, limbs, p):
    """n = 8192 * 256 + 300 elements, pid 1: field_ref.grid_block's 4 099 directed quadruples tiled (4 099 is prime, so the block falls on other lanes
    in every repetition; test_field_ref.py shows that the 300 elements of the second pass take every rare branch); the output is the block's expected
    output tiled"""
    block = fr.grid_block(limbs, p)
    arrs = [tiled([q[j] for q in block], limbs, GRID_N) for j in range(4)]
    want = tiled([fr.expected(1, p, *q) for q in block], limbs, GRID_N)
    got = beaver_elem_dev(ctx, 1, limbs, p, arrs, GRID_N)
    assert np.array_equal(got[-300:], want[-300:]), "second pass of the grid-stride loop"
    assert np.array_equal(got, want)


def ss_cases(p, bound):
    """(rm, rand) pairs: draws at 0, 1, around bound / 2 and at bound - 1, crossed with rm at the field's edges and at the recentred mask and its neighbours"""
    half = bound >> 1
    out = []
    for rand in (0, 1, half - 1, half, half + 1, bound - 1):
        mask = (rand - bound) % p if rand >= half else rand
        for rm in fr.edge_operands(p) + [mask, (mask + 1) % p, (mask - 1) % p]:
            out.append((rm, rand))
    return out


def ss_expected(p, bound, pairs):
    half = bound >> 1
    masks = [(rand - bound) % p if rand >= half else rand for _, rand in pairs]                 # ss.go:90-99
    return masks, [(rm - m) % p for (rm, _), m in zip(pairs, masks)]                            # ss.go:101-102


@pytest.mark.parametrize("limbs,p", DEV_MODULI, ids=["L2", "L4"])
def test_share_algebra_grid_stride(ctx, limbs, p):
    """the same construction for sfg_ss_mask_dev and sfg_ss_hub_share_dev: a 4 099-element block of directed (rm, rand) pairs tiled over 8192 * 256 + 300"""
    from sfgwas_amd import capi
    bound = p // 8
    cases = ss_cases(p, bound)
    block = [cases[i % len(cases)] for i in range(fr.GRID_BLOCK)]
    masks, masked = ss_expected(p, bound, block)
    n, nb = GRID_N, GRID_N * limbs * 8
    d_rm, d_rand = ctx.to_device(tiled([c[0] for c in block], limbs, n)), ctx.to_device(tiled([c[1] for c in block], limbs, n))
    d_out, d_mask, d_share = ctx.malloc(nb), ctx.malloc(nb), ctx.malloc(nb)
    mod, bnd = modarr(p, limbs), modarr(bound, limbs)
    ctx.check(capi.lib().sfg_ss_mask_dev(ctx.h, limbs, p64(mod), p64(bnd), d_rm, d_rand, d_out, d_mask, n), "ss_mask")
    assert np.array_equal(ctx.to_host(d_mask, (n, limbs), np.uint64), tiled(masks, limbs, n))
    assert np.array_equal(ctx.to_host(d_out, (n, limbs), np.uint64), tiled(masked, limbs, n))
    ctx.check(capi.lib().sfg_ss_hub_share_dev(ctx.h, limbs, p64(mod), d_out, d_mask, d_share, n), "ss_hub_share")
    assert np.array_equal(ctx.to_host(d_share, (n, limbs), np.uint64), tiled([c[0] for c in block], limbs, n))      # revealed + mask = rm
    for d in (d_rm, d_rand, d_out, d_mask, d_share):
        ctx.free(d)


# ---------------------------------------------------------------- dense product
MM_SHAPES = [(1, 1, 1), (8, 1, 8), (1, 257, 1), (8, 5, 8), (13, 3, 5), (15, 15, 7)]     # m n below, at and above one 64-thread block; k = 1; a long accumulation
MM_MODULI = [(2, (1 << 127) - 1), (2, fr.GENERIC[0][1]), (4, (1 << 255) - 19), (4, fr.GENERIC[1][1])]


def mm_operands(p, m, k, n, seed):
    """ar, am [m x k] and br, bm [k x n]: edge operands cyclically (another stride and offset per operand), every fourth element random; and for
    k >= 2 output element (0, 0) is made to start with the terms 1 and p - 1 for every party, so its running sum is exactly p once"""
    ops, rnd = fr.edge_operands(p), random.Random(seed)
    fill = lambda cnt, w: [ops[(i * (w + 1) + w) % len(ops)] if i % 4 != 3 else rnd.randrange(p) for i in range(cnt)]
    ar, am, br, bm = fill(m * k, 0), fill(m * k, 1), fill(k * n, 2), fill(k * n, 3)
    if k >= 2:
        ar[0], ar[1], am[0], am[1] = 0, 0, 1, p - 1                 # pid 0: am bm = 1, p - 1;  pid >= 1 with ar = 0: br am = 1, p - 1
        br[0], br[n], bm[0], bm[n] = 1, 1, 1, 1
    return ar, am, br, bm


def mm_expected(pid, limbs, p, m, k, n, ar, am, br, bm):
    """BeaverMultMat (beavermult.go:135-147) in Python integers, and which events the running sum acc + term meets in the kernel's order"""
    R, out, events = 1 << (64 * limbs), [], set()
    for i in range(m):
        for j in range(n):
            acc = 0
            for x in range(k):
                s = acc + fr.expected(pid, p, ar[i * k + x], am[i * k + x], br[x * n + j], bm[x * n + j])
                if s == p:
                    events.add("equals_p")
                if s >= R:
                    events.add("carry_out")
                acc = s % p
            out.append(acc)
    return out, events


@pytest.mark.parametrize("pid", [0, 1, 2])
@pytest.mark.parametrize("limbs,p", MM_MODULI, ids=[fr.mod_id(m) for m in MM_MODULI])
def test_beaver_matmul_directed(ctx, limbs, p, pid):
    from sfgwas_amd import capi
    mod = modarr(p, limbs)
    events = set()
    for m, k, n in MM_SHAPES:
        ints = mm_operands(p, m, k, n, seed=m * 1000 + k * 10 + n + pid)
        want, ev = mm_expected(pid, limbs, p, m, k, n, *ints)
        assert k < 2 or "equals_p" in ev
        events |= ev
        arrs = [fr.to_limbs(v, limbs) for v in ints]
        got = np.zeros((m * n, limbs), dtype=np.uint64)
        ctx.check(capi.lib().sfg_beaver_matmul(ctx.h, pid, limbs, p64(mod), *[p64(a) for a in arrs], p64(got), m, k, n), "beaver_matmul")
        assert_words(got, want, limbs, f"sfg_beaver_matmul {m}x{k}x{n}")
        orc = np.zeros((m * n, limbs), dtype=np.uint64)
        ol.lib().orc_beaver_matmul(pid, limbs, ol.p64(mod), *[ol.p64(a) for a in arrs], ol.p64(orc), m, k, n)
        assert np.array_equal(got, orc)
        if pid == 0:
            null = np.zeros((m * n, limbs), dtype=np.uint64)
            ctx.check(capi.lib().sfg_beaver_matmul(ctx.h, 0, limbs, p64(mod), None, p64(arrs[1]), None, p64(arrs[3]), p64(null), m, k, n), "beaver_matmul (NULL ar, br)")
            assert np.array_equal(null, got)
    assert ("carry_out" in events) == (p > 1 << (64 * limbs - 1))          # a + b < 2p: a carry out of the top word needs p above 2^(32 NW - 1)


# ---------------------------------------------------------------- share algebra
SS_MODULI = [(2, (1 << 127) - 1), (2, (1 << 128) - 159), (4, (1 << 255) - 19), (4, (1 << 256) - 189)]


@pytest.mark.parametrize("nparty", [2, 3, 4])
@pytest.mark.parametrize("limbs,p", SS_MODULI, ids=[fr.mod_id(m) for m in SS_MODULI])
def test_share_algebra_directed(ctx, limbs, p, nparty):
    """ss.go:84-110 with bound = p / (4 (nParty - 1)): the recentring compare at bound / 2 and its neighbours, rm - mask at zero and at a borrow, the
    hub's sum at exactly p and at a carry out of the top word; mask_dev NULL once more"""
    from sfgwas_amd import capi
    L = capi.lib()
    bound = p // (4 * (nparty - 1))
    if (p, nparty) in (((1 << 127) - 1, 2), ((1 << 255) - 19, 2)):
        assert bound & 1                                    # an odd bound: bound / 2 truncates
    pairs = ss_cases(p, bound)
    n = len(pairs)
    masks, masked = ss_expected(p, bound, pairs)
    a_rm, a_rand = fr.to_limbs([c[0] for c in pairs], limbs), fr.to_limbs([c[1] for c in pairs], limbs)
    mod, bnd = modarr(p, limbs), modarr(bound, limbs)
    d_rm, d_rand = ctx.to_device(a_rm), ctx.to_device(a_rand)
    d_out, d_mask, d_out2, d_share = (ctx.malloc(n * limbs * 8) for _ in range(4))
    ctx.check(L.sfg_ss_mask_dev(ctx.h, limbs, p64(mod), p64(bnd), d_rm, d_rand, d_out, d_mask, n), "ss_mask")
    got_out, got_mask = ctx.to_host(d_out, (n, limbs), np.uint64), ctx.to_host(d_mask, (n, limbs), np.uint64)
    assert_words(got_mask, masks, limbs, "ss_mask: mask", lambda i: f"rand {pairs[i][1]:#x}, bound {bound:#x}")
    assert_words(got_out, masked, limbs, "ss_mask: rm - mask", lambda i: f"rm {pairs[i][0]:#x}, rand {pairs[i][1]:#x}")
    o_out, o_mask = np.zeros((n, limbs), dtype=np.uint64), np.zeros((n, limbs), dtype=np.uint64)
    ol.lib().orc_ss_mask(limbs, ol.p64(mod), ol.p64(bnd), ol.p64(a_rm), ol.p64(a_rand), ol.p64(o_out), ol.p64(o_mask), n)
    assert np.array_equal(got_out, o_out) and np.array_equal(got_mask, o_mask)
    ctx.check(L.sfg_ss_mask_dev(ctx.h, limbs, p64(mod), p64(bnd), d_rm, d_rand, d_out2, None, n), "ss_mask (NULL mask_dev)")
    assert np.array_equal(ctx.to_host(d_out2, (n, limbs), np.uint64), got_out)
    # hub: revealed + mask, with revealed = rm - mask, is rm again
    ctx.check(L.sfg_ss_hub_share_dev(ctx.h, limbs, p64(mod), d_out, d_mask, d_share, n), "ss_hub_share")
    assert np.array_equal(ctx.to_host(d_share, (n, limbs), np.uint64), a_rm)
    for d in (d_rm, d_rand, d_out, d_mask, d_out2, d_share):
        ctx.free(d)
    # hub sums aimed at revealed + mask == p and at the carry: every pair of edge operands
    ops = fr.edge_operands(p)
    xs, ys = [x for x in ops for _ in ops], [y for _ in ops for y in ops]
    cls = set()
    for x, y in zip(xs, ys):
        fr.model_add(limbs, p, x, y, cls)
    assert "add_equals_p" in cls and ("add_carry_out" in cls) == (p > 1 << (64 * limbs - 1))
    a_x, a_y = fr.to_limbs(xs, limbs), fr.to_limbs(ys, limbs)
    d_x, d_y, d_s = ctx.to_device(a_x), ctx.to_device(a_y), ctx.malloc(len(xs) * limbs * 8)
    ctx.check(L.sfg_ss_hub_share_dev(ctx.h, limbs, p64(mod), d_x, d_y, d_s, len(xs)), "ss_hub_share")
    got = ctx.to_host(d_s, (len(xs), limbs), np.uint64)
    assert_words(got, [(x + y) % p for x, y in zip(xs, ys)], limbs, "ss_hub_share", lambda i: f"{xs[i]:#x} + {ys[i]:#x}")
    orc = np.zeros((len(xs), limbs), dtype=np.uint64)
    ol.lib().orc_ss_hub_share(limbs, ol.p64(mod), ol.p64(a_x), ol.p64(a_y), ol.p64(orc), len(xs))
    assert np.array_equal(got, orc)
    for d in (d_x, d_y, d_s):
        ctx.free(d)


# ---------------------------------------------------------------- refusals: an error and its message, no kernel
def test_refusals(ctx):
    from sfgwas_amd import capi
    L = capi.lib()
    p = (1 << 127) - 1
    n = 4
    h = [np.full((n, 4), 7, dtype=np.uint64) for _ in range(4)]                     # wide enough for any limbs <= 4
    mark = np.full((n, 4), 0x5151515151515151, dtype=np.uint64)
    out = mark.copy()
    mod, even, above = modarr(p, 4), modarr(p - 1, 4), modarr(p + 1, 4)
    d = [ctx.to_device(a) for a in h]
    d_out, d_mask = ctx.to_device(mark), ctx.to_device(mark)

    def refused(rc, message):
        assert rc != 0 and message in last_error(ctx)

    limbs_msg, odd_msg = "beaver: limbs must be 2 (128-bit) or 4 (256-bit)", "beaver: modulus must be odd"
    hp = [p64(a) for a in h]
    refused(L.sfg_beaver_elem(ctx.h, 1, 3, p64(mod), *hp, p64(out), n), limbs_msg)
    refused(L.sfg_beaver_elem_dev(ctx.h, 1, 3, p64(mod), *d, d_out, n), limbs_msg)
    refused(L.sfg_beaver_matmul(ctx.h, 1, 3, p64(mod), *hp, p64(out), 2, 2, 2), limbs_msg)
    refused(L.sfg_ss_mask_dev(ctx.h, 3, p64(mod), p64(mod), d[0], d[1], d_out, d_mask, n), limbs_msg)
    refused(L.sfg_ss_hub_share_dev(ctx.h, 3, p64(mod), d[0], d[1], d_out, n), limbs_msg)
    refused(L.sfg_beaver_elem(ctx.h, 1, 2, p64(even), *hp, p64(out), n), odd_msg)
    refused(L.sfg_beaver_elem_dev(ctx.h, 1, 2, p64(even), *d, d_out, n), odd_msg)
    refused(L.sfg_beaver_matmul(ctx.h, 1, 2, p64(even), *hp, p64(out), 2, 2, 2), odd_msg)
    refused(L.sfg_ss_mask_dev(ctx.h, 2, p64(even), p64(even), d[0], d[1], d_out, d_mask, n), odd_msg)
    refused(L.sfg_ss_hub_share_dev(ctx.h, 2, p64(even), d[0], d[1], d_out, n), odd_msg)
    refused(L.sfg_ss_mask_dev(ctx.h, 2, p64(mod), p64(above), d[0], d[1], d_out, d_mask, n), "ss_share: bound exceeds the field modulus")
    for m, k, nn in ((0, 2, 2), (2, 0, 2), (2, 2, 0)):
        refused(L.sfg_beaver_matmul(ctx.h, 1, 2, p64(mod), *hp, p64(out), m, k, nn), "beaver_matmul: bad dimensions")
    ctx.sync()
    assert np.array_equal(out, mark)                                                # nothing ran, nothing was written
    assert np.array_equal(ctx.to_host(d_out, (n, 4), np.uint64), mark) and np.array_equal(ctx.to_host(d_mask, (n, 4), np.uint64), mark)
    # a bound equal to the modulus is not above it, and the context is usable after the refusals
    ctx.check(L.sfg_ss_mask_dev(ctx.h, 2, p64(mod), p64(mod), d[0], d[1], d_out, d_mask, n), "ss_mask")
    assert fr.from_limbs(ctx.to_host(d_mask, (n, 2), np.uint64)) == [7 + (7 << 64)] * n           # 7 + 7 * 2^64 < p / 2: the mask is the draw
    for q in d + [d_out, d_mask]:
        ctx.free(q)
