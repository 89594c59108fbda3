"""GPU parity of the restructured key-switch path (rotate.hip, the finalize and operand gather of matmul.hip), every word with zero tolerance:

  * rotation words against the oracle on PN14 (levels 5 and 4) and on the chains S1 (single-prime digits), S3 and S4 of tests/ksw_ref.py, random and
    directed ciphertexts (the generators of tests/test_gpu_ksw_shapes.py): the extension kernels now take two positions per thread and hand the
    forward transform rows that are already through its first stage;
  * hoisted job lists in the MAC-operand output form, whose unread modulus row is no longer computed: here a one-block-row product is compared as a whole,
    at input level max_level (a dead row) and max_level - 1 (none); the rows themselves, word by word, are held by tests/test_gpu_rotcache.py through
    sfg_rotcache_build_rows_dev / sfg_rotcache_build_jobs_dev;
  * the summed finalize (the giants are added where the key switch finishes them) against rotating with the public single-rotation entry point and
    summing with integers: a giant range that starts above 0, a slot base above 0, accumulate = 1, giant 0 as a plain read, one and two block columns,
    at the default key-switch budget and at the smallest one (sum groups split over input groups and job chunks); on S1 / S3 / S4 as well;
  * the giant-activity table with holes: a 60 x 40 product, s = 2 (giants 0, 89 and 90 only), against the oracle;
  * one whole product at the parity gate's shape, 8192 x 16384, s = 2, both orientations, against the oracle.
"""
import os

import numpy as np
import pytest

import ksw_ref as kr
import oracle_lib as ol
import test_gpu_fullsize as fs
import test_gpu_ksw_shapes as ks

pytestmark = pytest.mark.gpu
SLOTS, D, N, L, LEVEL = fs.SLOTS, fs.D, fs.N, fs.L, fs.LEVEL
GIANTS = [1, 2, 3, 4, 5]                               # giant steps the finalize cases align (plus giant 0, which needs no key)


class LightEnv:
    """a PN14 context and the oracle ring with the same random keys for a short list of left rotations"""

    def __init__(self, left_rots, **env_overrides):
        from sfgwas_amd import capi
        self.capi = capi
        saved = {k: os.environ.get(k) for k in env_overrides}
        os.environ.update({k: str(v) for k, v in env_overrides.items()})
        try:
            self.ctx = capi.Context(ol.Q_PN14, ol.P_PN14)                # the library reads its deployment switches here, once
        finally:
            for k, v in saved.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
        self.ring = ol.Ring(14, ol.Q_PN14, ol.P_PN14)
        self.keys = ol.RotKeys(self.ring)
        for k in left_rots:
            g = self.ring.galois(k)
            key = capi.random_rotkey(self.ring.moduli, self.ring.beta, self.ring.N, 1000 + k)
            self.keys.add(g, key)
            self.ctx.load_rotkey(g, key)

    def close(self):
        self.ctx.close()


@pytest.fixture(scope="module")
def pn14():
    e = LightEnv([SLOTS - r for r in ks.ROTS] + [g * D for g in GIANTS])
    yield e
    e.close()


@pytest.fixture(scope="module")
def pn14_small_budget():
    e = LightEnv([g * D for g in GIANTS], SFG_KSW_BUDGET_MB=16)          # 4 inputs per group, 5 jobs per chunk at level 4
    yield e
    e.close()


@pytest.fixture(scope="module")
def full():
    e = fs.Env()
    yield e
    e.close()


# ---------------------------------------------------------------------------------------------------- rotation words
@pytest.mark.parametrize("kind", ["random", "directed"])
@pytest.mark.parametrize("level", [5, 4])
def test_pn14_rotations_bit_exact(pn14, level, kind):
    nrots = ks.ROTS + [0]
    cts = ks._cts(pn14.ring, level, kind, len(nrots), 500)
    got = pn14.ctx.rotate_right(cts, level, nrots)
    for j, r in enumerate(nrots):
        assert np.array_equal(got[j], ol.rotate_right(pn14.ring, pn14.keys, level, cts[j], r)), f"level {level} ct {j} rot {r}"


@pytest.mark.parametrize("kind", ["random", "directed"])
@pytest.mark.parametrize("name", sorted(kr.CHAINS))
def test_chain_rotations_bit_exact(name, kind):
    ctx, ring, keys = ks._env(name)
    level = max(kr.CHAINS[name][2])
    nrots = ks.ROTS + [0]
    cts = ks._cts(ring, level, kind, len(nrots), 600)
    got = ctx.rotate_right(cts, level, nrots)
    for j, r in enumerate(nrots):
        assert np.array_equal(got[j], ol.rotate_right(ring, keys, level, cts[j], r)), f"{name} level {level} ct {j} rot {r}"


# ---------------------------------------------------------------------------------------------------- the summed finalize
def _finalize_slots(ctx, acc, s, lmax, ncolb, acc_giants, base, g0, g1, out0=None):
    """sfg_matmul_finalize_slots_dev on host arrays: acc [ncolb][acc_giants][s][2][lmax][N]; out0 (accumulated onto) or None"""
    from sfgwas_amd import capi
    d_acc = capi.DevArray.from_host(ctx, acc)
    d_out = capi.DevArray.from_host(ctx, out0) if out0 is not None else capi.DevArray(ctx, (s, ncolb, 2, lmax, N))
    try:
        ctx.check(capi.lib().sfg_matmul_finalize_slots_dev(ctx.h, d_acc.p, s, lmax, ncolb, acc_giants, base, g0, g1, int(out0 is not None), d_out.p), "finalize_slots")
        return d_out.host()
    finally:
        d_acc.free(); d_out.free()


def _rotate_and_sum(ctx, moduli, acc, s, lmax, ncolb, base, g0, g1, out0=None):
    """the same from single rotations (the public entry point; a rotation by 0 is its copy) summed with integers: out[i][j] (+)= sum_g RotateRight(acc[j][g][i], -(base + g) d)"""
    want = np.zeros((s, ncolb, 2, lmax, N), dtype=np.uint64) if out0 is None else out0.copy()
    slots = [g for g in range(g0, g1) if base + g < D]
    if slots:
        cts = np.stack([acc[j, g, i] for j in range(ncolb) for g in slots for i in range(s)])
        nrots = [(-(base + g) * D) % SLOTS for j in range(ncolb) for g in slots for i in range(s)]
        rot = ctx.rotate_right(cts, lmax - 1, nrots).reshape(ncolb, len(slots), s, 2, lmax, N)
        for j in range(ncolb):
            for i in range(s):
                want[i, j] += rot[j, :, i].sum(axis=0)                       # a handful of words below 2^47: no overflow
    for l in range(lmax):
        want[..., l, :] %= np.uint64(moduli[l])
    return want


def _acc(ring, ncolb, acc_giants, s, lmax, seed):
    return np.stack([np.stack([np.stack([ring.fill_uniform(lmax - 1, seed + 100 * j + 10 * g + i) for i in range(s)]) for g in range(acc_giants)]) for j in range(ncolb)])


# (acc_giants, giant_base, g0, g1, accumulate)
FIN_CASES = [(4, 0, 1, 4, False),          # a giant range that starts above 0
             (3, 0, 0, 3, True),           # giant 0 joins as a plain read; accumulated onto an earlier output
             (4, 2, 0, 4, False),          # a rank's slots: slot g holds giant 2 + g
             (2, 0, 0, 1, False),          # giant 0 alone: no key-switch job at all
             (3, 0, 2, 2, True)]           # an empty range: the output stays what it was


@pytest.mark.parametrize("budget", ["default", "smallest"])
@pytest.mark.parametrize("ncolb", [1, 2])
@pytest.mark.parametrize("case", FIN_CASES)
def test_summed_finalize_equals_rotate_and_sum(pn14, pn14_small_budget, case, ncolb, budget):
    acc_giants, base, g0, g1, accumulate = case
    env = pn14 if budget == "default" else pn14_small_budget
    s = 2
    acc = _acc(env.ring, ncolb, acc_giants, s, L, 700 + 7 * base)
    out0 = np.stack([np.stack([env.ring.fill_uniform(L - 1, 900 + 10 * i + j) for j in range(ncolb)]) for i in range(s)]) if accumulate else None
    got = _finalize_slots(env.ctx, acc, s, L, ncolb, acc_giants, base, g0, g1, out0)
    want = _rotate_and_sum(pn14.ctx, env.ring.moduli, acc, s, L, ncolb, base, g0, g1, out0)
    assert np.array_equal(got, want), f"{np.count_nonzero(got != want)} words differ"


@pytest.mark.parametrize("name", sorted(kr.CHAINS))
def test_summed_finalize_on_the_chains_vs_oracle(name):
    """giants 0 and 1 of two outputs at each chain's highest level, against the oracle's rotations summed with integers (S4's moduli have 47 bits)"""
    from sfgwas_amd import capi
    ctx, ring, keys = ks._env(name)
    if not hasattr(ctx, "ksw_giant_key"):
        g = ring.galois(D)
        key = capi.random_rotkey(ring.moduli, ring.beta, ring.N, 77)
        keys.add(g, key)
        ctx.load_rotkey(g, key)
        ctx.ksw_giant_key = True
    lmax = max(kr.CHAINS[name][2]) + 1
    s = 2
    acc = np.stack([np.stack([np.stack([kr.directed_ct(ring, lmax - 1, 800 + i) if g == 1 and i == 0 else ring.fill_uniform(lmax - 1, 810 + 10 * g + i) for i in range(s)])
                              for g in range(2)])])
    got = _finalize_slots(ctx, acc, s, lmax, 1, 2, 0, 0, 2)
    for i in range(s):
        want = acc[0, 0, i] + ol.rotate_right(ring, keys, lmax - 1, acc[0, 1, i], SLOTS - D)
        for l in range(lmax):
            want[:, l, :] %= np.uint64(ring.moduli[l])
        assert np.array_equal(got[i, 0], want), f"{name} output {i}"


# ---------------------------------------------------------------------------------------------------- products
@pytest.mark.parametrize("in_level", [5, 4])
def test_small_product_with_giant_holes_vs_oracle(full, in_level):
    """60 x 40, s = 2: hoisted baby steps in the MAC-operand form (in_level 5: the row of modulus 5 is not computed; in_level 4: every row is read),
    giants 0, 89 and 90 only in the summed finalize"""
    lmax = L
    rnd = np.random.default_rng(31)
    geno = rnd.integers(-1, 3, (60, 40)).astype(np.int8)
    A = fs.host_cts(full.ring, 2, 1, in_level, 13)
    got, _, _ = full.ctx.matmul_stream(A, in_level, lmax, geno)
    want, _, _ = ol.matmult4stream(full.ring, full.keys, fs.SCALE, A, in_level, lmax, geno, enc_prec=1)
    assert np.array_equal(got, want), f"{np.count_nonzero(got != want)} words differ"


@pytest.mark.parametrize("transposed", [False, True])
def test_whole_product_8192x16384_vs_oracle(full, transposed):
    """the parity gate's shape: one block row x two block columns, all 8192 diagonals, s = 2 - and its transposed read (two block rows x one block column)"""
    capi = full.capi
    rnd = np.random.default_rng(32)
    geno = rnd.integers(-1, 3, (SLOTS, 2 * SLOTS)).astype(np.int8)
    A = fs.host_cts(full.ring, 2, 2 if transposed else 1, LEVEL, 17)
    g = full.ctx.geno_upload(geno)
    dA = capi.DevArray.from_host(full.ctx, A)
    got = full.ctx.matmul_resident(dA, 2, LEVEL, L, g, flags=capi.SFG_TRANSPOSE if transposed else 0)
    want = fs.oracle_product(full, A, np.ascontiguousarray(geno.T) if transposed else geno)
    h = got.host()
    dA.free(); got.free(); full.ctx.geno_free(g)
    assert np.array_equal(h, want), f"{np.count_nonzero(h != want)} words differ"
