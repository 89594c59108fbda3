"""GPU parity of the key switch whose Q-row inner product lives in the finish and whose key words are read once per tile of jobs (rotate.hip k_ksw_inner_p,
k_ksw_finish, k_ksw_finish_sum; the tiles of sfgwas_amd/csrc/ksw_plan.hpp), every word with zero tolerance.

A tile is up to T consecutive jobs under one key and one automorphism table - T = 3 (rotate.hip KSW_T) in the plain finish and the special-prime inner product;
the summed finish takes no tiles.  The job lists below hold runs of 1, 2, 3, 4, 5, 6, 7 and 11 jobs, i.e. 1, 2, T, T + 1 and 2 T + 1 for T = 3 and for T = 5 (and
for any T in {1, 2, 3, 5} a later change may pick), two keys interleaved, and a rotation by 0 inside a run:

  * the public rotation entry on PN14 at levels 5 and 4 and on the chains S1, S3, S4 of tests/ksw_ref.py, random and directed ciphertexts: every ciphertext
    against the oracle and against the same job issued alone in a call of its own;
  * the same lists at the smallest key-switch budget (SFG_KSW_BUDGET_MB=16: four inputs per group, four or five jobs per chunk), where groups and chunks cut the runs;
  * the summed finalize (sfg_matmul_finalize_slots_dev) for s = 1 .. 6 outputs: giant ranges that start above 0, a slot base above 0, accumulate 0 / 1, giant 0 as
    the plain member, one and two block columns, both budgets, against rotate-and-sum with integers (tests/test_gpu_ksw_fused.py _rotate_and_sum);
  * the MAC-operand form through sfg_rotcache_build_rows_dev and sfg_rotcache_build_jobs_dev for s = 1, 2, 4, 6 inputs at input levels 5 (a dead row) and 4, baby
    steps {0, 1, 2, 45, 89, 90} against tests/rotcache_ref.py, both budgets (at the smallest, 91 jobs per input pass through chunks of four);
  * relinearisation (add1) and the Galois entry (conjugation key) at level 5 on six ciphertexts (two tiles of three) against the oracle.

The split inverse transform of the same issue was built (ntt.hip k_ntt_inv_split, launch_ntt_inv_split): both inverse transforms of the key switch run through it,
their last stage and 1/N done by the extension kernels, so every list here passes through it; tests/test_ksw_plan.py holds that last stage against integers."""
import numpy as np
import pytest

import ksw_ref as kr
import oracle_lib as ol
import test_gpu_fullsize as fs
import test_gpu_ksw_fused as kf
import test_gpu_ksw_shapes as ks
import test_gpu_rotcache as rc

pytestmark = pytest.mark.gpu
SLOTS, D, N, L = fs.SLOTS, fs.D, fs.N, fs.L
RA, RB = SLOTS - 1, SLOTS - 2                      # right rotations whose keys fs.Env loads (left rotations 1 and 2, two baby steps)
RUNS = [1, 2, 3, 4, 5, 6, 7, 11]
BABIES = [0, 1, 2, 45, 89, 90]


def job_lists(a, b):
    runs = []
    for k, n in enumerate(RUNS):
        runs += [b if k & 1 else a] * n
    return {"runs": runs,                                       # 39 jobs: a x 1, b x 2, a x 3, ... b x 11
            "interleaved": [a, b, a, b, a, b, a],
            "zero inside a run": [a, a, a, 0, a, a, a, a, 0, 0, a]}


@pytest.fixture(scope="module")
def full():
    e = fs.Env()
    yield e
    e.close()


@pytest.fixture(scope="module")
def small():
    e = fs.Env(SFG_KSW_BUDGET_MB=16)
    yield e
    e.close()


def _env_of(request, budget):
    return request.getfixturevalue("full" if budget == "default" else "small")


def check_rotations(ctx, ring, keys, level, kind, nrots, seed, what):
    cts = ks._cts(ring, level, kind, len(nrots), seed)
    got = ctx.rotate_right(cts, level, nrots)
    want = rc.pool_map(lambda j: ol.rotate_right(ring, keys, level, cts[j], nrots[j]), range(len(nrots)))
    for j, r in enumerate(nrots):
        assert np.array_equal(got[j], want[j]), f"{what}: ct {j} rot {r} differs from the oracle ({np.count_nonzero(got[j] != want[j])} words)"
        alone = ctx.rotate_right(cts[j:j + 1], level, [r])[0]
        assert np.array_equal(got[j], alone), f"{what}: ct {j} rot {r} differs from the job issued alone"


# ---------------------------------------------------------------------------------------------------- the public rotation entry
@pytest.mark.parametrize("budget", ["default", "smallest"])
@pytest.mark.parametrize("kind", ["random", "directed"])
@pytest.mark.parametrize("level", [5, 4])
@pytest.mark.parametrize("name", ["runs", "interleaved", "zero inside a run"])
def test_pn14_job_lists_bit_exact(request, name, level, kind, budget):
    e = _env_of(request, budget)
    check_rotations(e.ctx, e.ring, e.keys, level, kind, job_lists(RA, RB)[name], 1100 + level, f"PN14 level {level} {name} ({budget} budget)")


@pytest.mark.parametrize("kind", ["random", "directed"])
@pytest.mark.parametrize("chain", sorted(kr.CHAINS))
def test_chain_job_lists_bit_exact(chain, kind):
    ctx, ring, keys = ks._env(chain)
    level = max(kr.CHAINS[chain][2])
    a, b = ks.ROTS
    nrots = [a] * 4 + [b] * 6 + [a, b, a, 0, a, a]
    check_rotations(ctx, ring, keys, level, kind, nrots, 1200, f"{chain} level {level}")


# ---------------------------------------------------------------------------------------------------- the summed finalize
# (acc_giants, giant_base, g0, g1, accumulate)
FIN_CASES = [(4, 0, 1, 4, False),          # a giant range that starts above 0
             (3, 0, 0, 3, True),           # giant 0 joins as a plain read; accumulated onto an earlier output
             (4, 2, 0, 4, False)]          # a slot base above 0: slot g holds giant 2 + g


@pytest.mark.parametrize("budget", ["default", "smallest"])
@pytest.mark.parametrize("s,ncolb", [(1, 1), (2, 2), (3, 1), (4, 2), (5, 1), (6, 1)])
@pytest.mark.parametrize("case", FIN_CASES)
def test_summed_finalize_equals_rotate_and_sum(request, full, case, s, ncolb, budget):
    acc_giants, base, g0, g1, accumulate = case
    e = _env_of(request, budget)
    acc = kf._acc(e.ring, ncolb, acc_giants, s, L, 1300 + 7 * base + s)
    out0 = np.stack([np.stack([e.ring.fill_uniform(L - 1, 1400 + 10 * i + j) for j in range(ncolb)]) for i in range(s)]) if accumulate else None
    got = kf._finalize_slots(e.ctx, acc, s, L, ncolb, acc_giants, base, g0, g1, out0)
    want = kf._rotate_and_sum(full.ctx, e.ring.moduli, acc, s, L, ncolb, base, g0, g1, out0)
    assert np.array_equal(got, want), f"{np.count_nonzero(got != want)} words differ"


def test_the_reference_rotations_of_the_sum_are_the_oracles(full):
    """what _rotate_and_sum adds up: the public entry's rotation by a giant step, one ciphertext against the oracle"""
    ct = full.ring.fill_uniform(L - 1, 1500)
    r = (-2 * D) % SLOTS
    assert np.array_equal(full.ctx.rotate_right(ct[None], L - 1, [r])[0], ol.rotate_right(full.ring, full.keys, L - 1, ct, r))


# ---------------------------------------------------------------------------------------------------- the MAC-operand form
@pytest.mark.parametrize("budget", ["default", "smallest"])
@pytest.mark.parametrize("in_level", [5, 4])
@pytest.mark.parametrize("s", [1, 2, 4, 6])
def test_mac_operand_rows_vs_reference(request, s, in_level, budget):
    e = _env_of(request, budget)
    ring = e.ring
    A = np.stack([(kr.directed_ct(ring, in_level, 1600 + i) if i == 1 else ring.fill_uniform(in_level, 1610 + 10 * in_level + i))[None] for i in range(s)])
    got, flat = rc.build_rows_host(e.ctx, A, s, in_level, L, 1, 0, 1, ol.Q_PN14)
    rc.check_cache_vs_oracle(ring, e.keys, A, in_level, L, got, BABIES, f"s {s} in_level {in_level} ({budget} budget)")
    rowf, jobw, _ = rc.rr.layout(ol.Q_PN14, L, s, N)
    with rc.Bufs(e.ctx) as b:
        dA = b.up(A)
        staged = b.sentinel(s * jobw)
        e.ctx.rotcache_build_jobs(dA, s, in_level, L, 1, 0, s, staged)
        hs = rc.dl(staged, 0, s * jobw + rc.GUARD)
    assert (hs[s * jobw:] == rc.SENT).all(), "build_jobs wrote past its jobs"
    want = flat[:s * jobw].reshape(D, s, 2 * rowf).transpose(1, 0, 2).reshape(s, jobw)          # job-major: [i][baby][2][rowf]
    assert np.array_equal(hs[:s * jobw].reshape(s, jobw), want), "build_jobs differs from build_rows"


# ---------------------------------------------------------------------------------------------------- relinearisation and the Galois entry
@pytest.mark.parametrize("kind", ["random", "directed"])
def test_relinearisation_of_six_bit_exact(kind):
    ctx, ring, keys = ks._env("PN14")
    level, n = 5, 6
    a = ks._cts(ring, level, kind, n, 1700)
    b = np.stack([kr.directed_ct(ring, level, 1750 + j, ones=True) if kind == "directed" else ring.fill_uniform(level, 1750 + j) for j in range(n)])
    got = ctx.evalop("sfg_ct_mulrelin_dev", level, a, b)
    for j in range(n):
        want = np.zeros_like(a[j])
        ol.lib().orc_mulrelin(ring.h, level, ol.p64(a[j]), ol.p64(b[j]), ol.p64(keys.keys[1]), ol.p64(want))
        assert np.array_equal(got[j], want), f"ct {j}"


@pytest.mark.parametrize("kind", ["random", "directed"])
def test_conjugation_of_six_bit_exact(kind):
    ctx, ring, keys = ks._env("PN14")
    level, n, g = 5, 6, 2 * ring.N - 1
    cts = ks._cts(ring, level, kind, n, 1800)
    got = ks._galois(ctx, cts, level, g)
    for j in range(n):
        want = np.zeros_like(cts[j])
        assert ol.lib().orc_apply_galois(ring.h, keys.h, level, ol.p64(cts[j]), g, ol.p64(want)) == 0
        assert np.array_equal(got[j], want), f"ct {j}"
