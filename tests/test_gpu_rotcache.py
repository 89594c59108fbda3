"""The baby-step rotation cache as an object (include/sfgwas_hip.h: sfg_rotcache_layout / build_jobs / scatter / build_rows / invalidate and the two *_rc_dev
products), every word with zero tolerance:

  * cache words against the oracle: cache[bi][baby][i] == encode_rows(RotateRight(A[i][bi], -baby)) in the MAC's fp64 operand form of tests/rotcache_ref.py.
    PN14, max_level 5, s = 2 (one random, one directed ciphertext), ALL 91 baby steps at input levels 4 (no dead row), 5 (the row of modulus 5 is never
    produced) and 6 (the gather drops a level).  PN14 is the mixed chain (one 46-bit modulus, then 35-bit ones); the chains S1 / S3 / S4 of tests/ksw_ref.py
    (S1, S3: 35-bit moduli only, one and three special primes; S4: 47-bit moduli only - every plane a {lo, hi} pair, no centring) run at their highest level
    with max_level = level and level + 1, where one random key array stands under all 90 baby Galois elements, and compare baby steps {0, 1, 2, 45, 89, 90}
    only: the other 85 baby steps are covered on PN14 only.
  * directed words through the key-switch finish: with all-zero baby keys the output is the automorphism's permutation of c0 and a zero c1, so the boundary
    words of the form (centring boundary, signed 23-bit split) reach rotate.hip store_rot_f64 exactly; baby step 0 takes them through mac_dma.hip k_rot_to_f64.  On PN14 (46-bit and centred 35-bit words) and on S4 at
    max_level 8 (47-bit words only).
  * the sharded build (build_jobs into a concatenated staging buffer, scatter) equals the in-place build, on sentinel-filled buffers with a guard region:
    partial scatters, a single interleaved slot, empty ranges, and one build_jobs call of 66 jobs (more than its chunk of 64 inputs per key-switch call) at
    max_level 1 - the lowest the library takes: rotcache_rowf asks 1 <= max_level <= nq, the key switch 0 <= level < nq, the build in_level + 1 >= max_level.
  * products on a prebuilt cache equal the products that build their own and the oracle (s = 2); s = 16 - the first s whose 2 s = 32 operand rows need more
    than one 30-row walk of launch_mac_bc, and the first at which the scan and the multi-GPU engine fall back to fp64 rows - is pinned against the library's
    own-build product only (its oracle run would take far longer than every other case here together).
  * the stale-copy contract of the int8 MAC's transposed operand copy (sfgwas_hip.h): build_rows, scatter and invalidate announce a rewritten buffer.
  * every host-side refusal of these entries, with the buffers untouched and the context usable afterwards.

Measured on one MI355X (profiles/rotcache_test_durations.txt): the file's 25 tests take 16 s; the slowest is test_x_product_on_a_prebuilt_cache at 2.95 s per
input level (the oracle's 8252 x 40 product); of the all-91-baby-step cases the slowest is in_level 4 at 0.47 s (182 oracle key switches on 16 host threads)
plus 1.5 s once for the module's context and its 180 keys; the 66-job case takes 0.79 s."""
import ctypes as C
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import ksw_ref as kr
import oracle_lib as ol
import rotcache_ref as rr
import test_gpu_fullsize as fs
import test_gpu_ksw_shapes as ks

pytestmark = pytest.mark.gpu
SLOTS, D, N, L = fs.SLOTS, fs.D, fs.N, fs.L
SENT = np.uint64(0x7FF85EA71E1D0001)               # a quiet NaN with a payload: no kernel here produces it
GUARD = 4096                                       # doubles allocated after every documented size


# ---------------------------------------------------------------------------------------------------- plumbing
class Bufs:
    """device buffers of one test, freed when it ends"""

    def __init__(self, ctx):
        from sfgwas_amd import capi
        self.ctx, self.capi, self.items = ctx, capi, []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for d in self.items:
            d.free()

    def add(self, d):
        self.items.append(d)
        return d

    def up(self, arr):
        return self.add(self.capi.DevArray.from_host(self.ctx, arr))

    def sentinel(self, ndoubles):
        """a float64 buffer of ndoubles + GUARD doubles, every one the sentinel"""
        return self.up(np.full(ndoubles + GUARD, SENT, dtype=np.uint64).view(np.float64))


def dl(d, off, n):
    """n doubles of a device buffer from double `off`, as uint64 words"""
    from sfgwas_amd import capi
    out = np.empty(n, dtype=np.uint64)
    d.ctx.check(capi.lib().sfg_memcpy_d2h(d.ctx.h, out.ctypes.data_as(C.c_void_p), C.c_void_p(d.p.value + off * 8), out.nbytes), "d2h")
    return out


def d2d(ctx, dst, src, ndoubles):
    from sfgwas_amd import capi
    ctx.check(capi.lib().sfg_memcpy_d2d(ctx.h, dst.p, src.p, ndoubles * 8), "d2d")


def pool_map(fn, items):
    with ThreadPoolExecutor(min(16, os.cpu_count() or 1)) as ex:
        return list(ex.map(fn, items))


def want_rows(ring, keys, lev, lmax, ct, babies):
    """[len(babies)][2][rowf]: encode_rows(RotateRight(ct at level lev, -baby)); baby 0 is the unrotated input at the dropped level"""
    q = ring.moduli[:ring.nq]
    ct = np.ascontiguousarray(ct[:, :lev + 1])

    def one(baby):
        return rr.encode_rows(ct if baby == 0 else ol.rotate_right(ring, keys, lev, ct, -baby % ring.slots), q, lmax)
    return np.stack(pool_map(one, list(babies)))


def check_f64(got, want, what):
    assert not np.isnan(got).any(), f"{what}: NaN"
    assert not (np.signbit(got) & (got == 0)).any(), f"{what}: -0.0"
    assert np.array_equal(got, want), f"{what}: {np.count_nonzero(got != want)} doubles differ"


def check_cache_vs_oracle(ring, keys, A, in_level, lmax, cache_rows, babies, what):
    """cache_rows: float64 [nrows][91][s][2][rowf] of block rows [0, nrows) of A [s][nbr][2][in_level + 1][N]"""
    lev = min(in_level, lmax)
    for bi in range(cache_rows.shape[0]):
        for i in range(A.shape[0]):
            want = want_rows(ring, keys, lev, lmax, A[i, bi], babies)
            check_f64(cache_rows[bi, list(babies), i], want, f"{what} block row {bi} input {i}")


def build_rows_host(ctx, A, s, in_level, lmax, nbr, b0, b1, q):
    """build_rows into a sentinel-filled buffer: (float64 view [b1 - b0][91][s][2][rowf], the flat uint64 download); tail zero and guard intact asserted"""
    rowf, jobw, tailw = rr.layout(q, lmax, s, N)
    assert ctx.rotcache_layout(s, lmax) == (jobw, tailw)
    with Bufs(ctx) as b:
        dA = b.up(A)
        cache = b.sentinel((b1 - b0) * s * jobw + tailw)
        ctx.rotcache_build_rows(dA, s, in_level, lmax, nbr, b0, b1, cache)
        h = dl(cache, 0, (b1 - b0) * s * jobw + tailw + GUARD)
    body, tail, guard = rr.cache_view(h, b1 - b0, s, rowf)
    assert not tail.any(), "the zero tail"
    assert (guard == SENT).all(), "written past the documented size"
    return body.view(np.float64), h


@pytest.fixture(scope="module")
def pn14():
    e = fs.Env()
    yield e
    e.close()


class ZeroKeyEnv:
    """a context and oracle keys whose 90 baby keys are all-zero arrays"""

    def __init__(self, q, p):
        from sfgwas_amd import capi
        self.q, self.ctx, self.ring = list(q), capi.Context(q, p), ol.Ring(14, q, p)
        self.keys = ol.RotKeys(self.ring)
        z = np.zeros((self.ring.beta, 2, len(self.ring.moduli), N), dtype=np.uint64)
        for k in range(1, D):
            self.keys.add(self.ring.galois(k), z)
            self.ctx.load_rotkey(self.ring.galois(k), z)


@pytest.fixture(scope="module")
def zero_keys():
    e = ZeroKeyEnv(ol.Q_PN14, ol.P_PN14)
    yield e
    e.ctx.close()


@pytest.fixture(scope="module")
def zero_keys_s4():
    e = ZeroKeyEnv(*kr.S4[:2])
    yield e
    e.ctx.close()


# ---------------------------------------------------------------------------------------------------- 2. cache words against the oracle
@pytest.mark.parametrize("in_level", [4, 5, 6])
def test_pn14_every_baby_step_vs_oracle(pn14, in_level):
    ring = pn14.ring
    A = np.stack([ring.fill_uniform(in_level, 40 + in_level)[None], kr.directed_ct(ring, in_level, 50 + in_level)[None]])
    got, _ = build_rows_host(pn14.ctx, A, 2, in_level, L, 1, 0, 1, ol.Q_PN14)
    check_cache_vs_oracle(ring, pn14.keys, A, in_level, L, got, range(D), f"PN14 in_level {in_level}")


def _directed_words_through_the_finish(e, in_level, lmax):
    ct = e.ring.fill_uniform(in_level, 61)
    bws = [rr.boundary_words(q) for q in e.q[:in_level + 1]]
    for l, bw in enumerate(bws):
        ct[0, l] = np.array(bw, dtype=np.uint64)[(np.arange(N) + 3 * l) % len(bw)]
    A = ct[None, None]
    got, _ = build_rows_host(e.ctx, A, 1, in_level, lmax, 1, 0, 1, e.q)
    check_cache_vs_oracle(e.ring, e.keys, A, in_level, lmax, got, range(D), "zero keys")
    assert not got[0, 1:, 0, 1].any(), "c1 of a rotation under a zero key"
    for baby in (0, 1, 45, 90):                                  # the directed words were in what was compared: each of them, as often as the cycle holds it
        words = rr.decode_rows(got[0, baby, 0], e.q, lmax)
        for l in range(lmax):
            vals, counts = np.unique(words[0, l], return_counts=True)
            have = dict(zip(vals.tolist(), counts.tolist()))
            assert all(have.get(w, 0) >= N // len(bws[l]) for w in bws[l]), f"baby {baby} modulus {l}"


def test_directed_words_through_the_finish(zero_keys):
    """row l of c0 cycles through the boundary words of modulus l; zero keys: RotateRight permutes c0 and zeroes c1"""
    _directed_words_through_the_finish(zero_keys, 5, L)


def test_directed_words_through_the_finish_at_47_bits(zero_keys_s4):
    """the same on S4 at level 7 with max_level 8: eight 47-bit moduli, no centring of small words, the largest hi the split produces"""
    _directed_words_through_the_finish(zero_keys_s4, 7, 8)


def _chain_env(name):
    """ks._env with one random key array under every baby Galois element that has none yet, on the context and on the oracle's keys"""
    from sfgwas_amd import capi
    ctx, ring, keys = ks._env(name)
    if not hasattr(ctx, "rotcache_baby_keys"):
        key = capi.random_rotkey(ring.moduli, ring.beta, ring.N, 91)
        for k in range(1, D):
            g = ring.galois(k)
            if g not in keys.keys:
                keys.add(g, key)
                ctx.load_rotkey(g, key)
        ctx.rotcache_baby_keys = True
    return ctx, ring, keys


CHAIN_CASES = [(name, max(kr.CHAINS[name][2]), max(kr.CHAINS[name][2]) + up) for name in sorted(kr.CHAINS) for up in (0, 1)
               if max(kr.CHAINS[name][2]) + up <= len(kr.CHAINS[name][0])]


@pytest.mark.parametrize("name,level,lmax", CHAIN_CASES)
def test_chain_cache_words_vs_oracle(name, level, lmax):
    ctx, ring, keys = _chain_env(name)
    A = np.stack([ring.fill_uniform(level, 70 + lmax)[None], kr.directed_ct(ring, level, 80 + lmax)[None]])
    got, _ = build_rows_host(ctx, A, 2, level, lmax, 1, 0, 1, ring.moduli[:ring.nq])
    check_cache_vs_oracle(ring, keys, A, level, lmax, got, [0, 1, 2, 45, 89, 90], f"{name} level {level} max_level {lmax}")


def test_the_chain_cases_are_the_ones_meant():
    assert len(CHAIN_CASES) == 6
    splits = {name: rr.ModSplit(kr.CHAINS[name][0], max(kr.CHAINS[name][2])) for name in kr.CHAINS}
    assert not any(splits["S1"].is_big) and not any(splits["S3"].is_big) and all(splits["S4"].is_big) and not splits["S4"].centre
    pn14 = rr.ModSplit(ol.Q_PN14, L)
    assert pn14.is_big == [True, False, False, False, False] and pn14.centre          # the mixed chain is PN14 itself


# ---------------------------------------------------------------------------------------------------- three block rows: the reference of item 3
@pytest.fixture(scope="module")
def rows3(pn14):
    """PN14, max_level 5, in_level 5, s = 2, nbr = 3 (6 jobs): A on the device and the host copy of build_rows(0, 3), whose gather addressing
    [s][nbr] the oracle pins at baby steps 0, 1 and 90 of every job"""
    from sfgwas_amd import capi

    class R:
        pass
    r = R()
    r.s, r.nbr, r.in_level = 2, 3, 5
    r.rowf, r.jobw, r.tailw = rr.layout(ol.Q_PN14, L, r.s, N)
    r.A = fs.host_cts(pn14.ring, r.s, r.nbr, r.in_level, 23)
    r.cache, r.flat = build_rows_host(pn14.ctx, r.A, r.s, r.in_level, L, r.nbr, 0, r.nbr, ol.Q_PN14)
    check_cache_vs_oracle(pn14.ring, pn14.keys, r.A, r.in_level, L, r.cache, [0, 1, 90], "three block rows")
    r.body = r.nbr * r.s * r.jobw                              # doubles before the tail
    r.dA = capi.DevArray.from_host(pn14.ctx, r.A)
    r.staged = r.flat[:r.body].reshape(r.nbr, D, r.s, 2 * r.rowf).transpose(0, 2, 1, 3).reshape(r.nbr * r.s, D * 2 * r.rowf)    # job-major [job][jobw], uint64
    yield r
    r.dA.free()


def test_rows_from_a_block_row_above_zero(pn14, rows3):
    r = rows3
    got, flat = build_rows_host(pn14.ctx, r.A, r.s, r.in_level, L, r.nbr, 1, 3, ol.Q_PN14)       # the tail after 2 rows and the guard: asserted there
    assert np.array_equal(flat[:2 * r.s * r.jobw], r.flat[r.s * r.jobw:r.body])


# ---------------------------------------------------------------------------------------------------- 3. the sharded build equals the in-place build
def test_sharded_staging_and_scatter_equal_the_in_place_build(pn14, rows3):
    r, ctx = rows3, pn14.ctx
    with Bufs(ctx) as b:
        staged = b.sentinel(6 * r.jobw)
        for j0, j1 in [(0, 1), (1, 4), (4, 6)]:                # as an all-gather would leave them: each range at its place in one buffer
            ctx.rotcache_build_jobs(r.dA, r.s, r.in_level, L, r.nbr, j0, j1, staged, at=j0 * r.jobw)
        hs = dl(staged, 0, 6 * r.jobw + GUARD)
        assert (hs[6 * r.jobw:] == SENT).all(), "build_jobs wrote past its jobs"
        assert np.array_equal(hs[:6 * r.jobw].reshape(6, r.jobw), r.staged)
        cache = b.sentinel(r.body + r.tailw)
        ctx.rotcache_scatter(staged, r.s, L, 0, 6, 0, 3, cache)
        hc = dl(cache, 0, r.body + r.tailw + GUARD)
        assert np.array_equal(hc, r.flat), "scatter(0, 6) differs from build_rows(0, 3), tail or guard included"


def test_a_job_range_in_the_middle_is_staged_alone(pn14, rows3):
    """build_jobs(2, 5) writes exactly three jobs' doubles, from the start of the buffer it is given"""
    r, ctx = rows3, pn14.ctx
    with Bufs(ctx) as b:
        staged = b.sentinel(3 * r.jobw)
        ctx.rotcache_build_jobs(r.dA, r.s, r.in_level, L, r.nbr, 2, 5, staged)
        hs = dl(staged, 0, 3 * r.jobw + GUARD)
        assert (hs[3 * r.jobw:] == SENT).all()
        assert np.array_equal(hs[:3 * r.jobw].reshape(3, r.jobw), r.staged[2:5])


def test_partial_scatter(pn14, rows3):
    r, ctx = rows3, pn14.ctx
    rows2 = 2 * r.s * r.jobw
    with Bufs(ctx) as b:
        staged = b.up(r.staged.view(np.float64))
        cache = b.sentinel(rows2 + r.tailw)
        ctx.rotcache_scatter(staged, r.s, L, 2, 6, 1, 2, cache, at=2 * r.jobw)          # jobs 2 .. 5 = block rows 1 and 2
        hc = dl(cache, 0, rows2 + r.tailw + GUARD)
        assert np.array_equal(hc[:rows2], r.flat[r.s * r.jobw:r.body]), "block rows 1 and 2"
        assert not hc[rows2:rows2 + r.tailw].any(), "the tail begins after nrows block rows and is zero"
        assert (hc[rows2 + r.tailw:] == SENT).all()
        # job 3 alone = (block row 1, i = 1): the interleaved i = 0 slots keep what they held
        row1 = r.s * r.jobw
        cache1 = b.sentinel(row1 + r.tailw)
        ctx.rotcache_scatter(staged, r.s, L, 3, 4, 1, 1, cache1, at=3 * r.jobw)
        h1 = dl(cache1, 0, row1 + r.tailw + GUARD)
        body, tail, guard = rr.cache_view(h1, 1, r.s, r.rowf)
        assert np.array_equal(body[0, :, 1], r.flat[:r.body].reshape(r.nbr, D, r.s, 2, r.rowf)[1, :, 1])
        assert (body[0, :, 0] == SENT).all() and not tail.any() and (guard == SENT).all()


def test_empty_job_range(pn14, rows3):
    r, ctx = rows3, pn14.ctx
    row1 = r.s * r.jobw
    with Bufs(ctx) as b:
        staged = b.sentinel(r.jobw)
        ctx.rotcache_build_jobs(r.dA, r.s, r.in_level, L, r.nbr, 2, 2, staged)
        assert (dl(staged, 0, r.jobw + GUARD) == SENT).all(), "build_jobs of no job wrote"
        cache = b.sentinel(row1 + r.tailw)
        ctx.rotcache_scatter(staged, r.s, L, 2, 2, 1, 1, cache)
        h = dl(cache, 0, row1 + r.tailw + GUARD)
        assert (h[:row1] == SENT).all() and not h[row1:row1 + r.tailw].any() and (h[row1 + r.tailw:] == SENT).all(), "scatter of no job zeroes the tail only"


def test_66_jobs_in_one_call_cross_the_chunk_of_64(pn14):
    """s = 33, nbr = 2 at max_level = in_level = 1 (one 46-bit modulus: rowf = 2 N; staging and cache about 3 GB each, compared in slices so that the host holds
    two pieces of 13 k-slices at a time): scatter(build_jobs(0, 66)) == build_rows(0, 2) in every word, no cap; jobs 0, 63, 64 and 65 also against the oracle at
    baby steps 0, 1 and 90.  Wall time on one MI355X: 0.79 s."""
    ctx, ring = pn14.ctx, pn14.ring
    s, nbr, lmax, lev = 33, 2, 1, 1
    rowf, jobw, tailw = rr.layout(ol.Q_PN14, lmax, s, N)
    assert ctx.rotcache_layout(s, lmax) == (jobw, tailw)
    with Bufs(ctx) as b:
        dA = b.add(ctx.fill_uniform_cts(s * nbr, lev, 0x66))                      # [s][nbr][2][2][N]
        staged = b.add(ctx.rotcache_build_jobs(dA, s, lev, lmax, nbr, 0, s * nbr))
        sc = b.add(ctx.rotcache_scatter(staged, s, lmax, 0, s * nbr, 0, nbr))
        br = b.add(ctx.rotcache_build_rows(dA, s, lev, lmax, nbr, 0, nbr))
        per_baby = s * 2 * rowf                                                   # one k-slice: [s][2][rowf]
        for bi in range(nbr):
            for baby0 in range(0, D, 13):                                         # 7 pieces of 13 k-slices per block row
                off, n = (bi * D + baby0) * per_baby, 13 * per_baby
                assert np.array_equal(dl(sc, off, n), dl(br, off, n)), f"block row {bi} baby steps {baby0} .. {baby0 + 12}"
        t0, t1 = dl(sc, nbr * D * per_baby, tailw), dl(br, nbr * D * per_baby, tailw)
        assert not t0.any() and not t1.any()
        for job in (0, 63, 64, 65):
            bi, i = job // s, job % s
            ct = dA.host_slice((i * nbr + bi,))
            want = want_rows(ring, pn14.keys, lev, lmax, ct, [0, 1, 90])
            for k, baby in enumerate([0, 1, 90]):
                got = dl(staged, (job * D + baby) * 2 * rowf, 2 * rowf).view(np.float64).reshape(2, rowf)
                check_f64(got, want[k], f"job {job} baby {baby}")


# ---------------------------------------------------------------------------------------------------- 4. products on a prebuilt cache
@pytest.mark.parametrize("in_level", [5, 6])
def test_x_product_on_a_prebuilt_cache(pn14, in_level):
    """(8192 + 60) x 40, s = 2: two operand block rows, one ragged; the cache from build_rows and from build_jobs + scatter"""
    ctx = pn14.ctx
    geno = np.random.default_rng(71).integers(-1, 3, (SLOTS + 60, 40)).astype(np.int8)
    A = fs.host_cts(pn14.ring, 2, 2, in_level, 31 + in_level)
    g = ctx.geno_upload(geno)
    try:
        with Bufs(ctx) as b:
            dA = b.up(A)
            own = b.add(ctx.matmul_resident(dA, 2, in_level, L, g)).host()
            cache = b.add(ctx.rotcache_build_rows(dA, 2, in_level, L, 2, 0, 2))
            got = b.add(ctx.matmul_resident_range_rc(cache, 2, L, g, 0, 0, 1)).host()
            staged = b.add(ctx.rotcache_build_jobs(dA, 2, in_level, L, 2, 0, 4))
            cache2 = b.add(ctx.rotcache_scatter(staged, 2, L, 0, 4, 0, 2))
            got2 = b.add(ctx.matmul_resident_range_rc(cache2, 2, L, g, 0, 0, 1)).host()
    finally:
        ctx.geno_free(g)
    assert np.array_equal(got, own), f"{np.count_nonzero(got != own)} words differ from the own-build product"
    assert np.array_equal(got2, own), "the cache of build_jobs + scatter"
    want = fs.oracle_product(pn14, A, geno, in_level=in_level)
    assert np.array_equal(got, want), f"{np.count_nonzero(got != want)} words differ from the oracle"


def test_xt_product_on_a_cache_of_a_block_row_range(pn14):
    """60 x (2 * 8192 + 40) read transposed: three operand block rows, the cache holds [1, 3) only"""
    from sfgwas_amd import capi
    ctx, T = pn14.ctx, capi.SFG_TRANSPOSE
    geno = np.random.default_rng(72).integers(-1, 3, (60, 2 * SLOTS + 40)).astype(np.int8)
    A = fs.host_cts(pn14.ring, 2, 3, 5, 37)
    g = ctx.geno_upload(geno)
    try:
        with Bufs(ctx) as b:
            dA = b.up(A)
            cache = b.add(ctx.rotcache_build_rows(dA, 2, 5, L, 3, 1, 3))
            own = b.add(ctx.matmul_resident(dA, 2, 5, L, g, flags=T, blk=(1, 3))).host()
            got = b.add(ctx.matmul_resident_range_rc(cache, 2, L, g, T, 1, 3)).host()
            assert np.array_equal(got, own), "resident_range_rc(1, 3)"
            acc_own = b.add(ctx.matmul_accumulate(dA, 2, 5, L, g, T, 1, 3, 0, 1))
            acc = b.add(ctx.matmul_accumulate_rc(cache, 2, L, g, T, 1, 3, 0, 1))
            assert np.array_equal(acc.host(), acc_own.host()), "accumulate_rc, accumulate = 0"
            ctx.matmul_accumulate(dA, 2, 5, L, g, T, 1, 3, 0, 1, acc=acc_own)
            ctx.matmul_accumulate_rc(cache, 2, L, g, T, 1, 3, 0, 1, acc=acc)
            h, h_own = acc.host(), acc_own.host()
            assert np.array_equal(h, h_own), "accumulate_rc, accumulate = 1"
            assert h.any()
    finally:
        ctx.geno_free(g)


def test_s16_product_on_a_prebuilt_cache(pn14):
    """60 x 40, s = 16: 32 operand rows (two walks of launch_mac_bc), against the library's own-build product"""
    ctx, s = pn14.ctx, 16
    geno = np.random.default_rng(73).integers(-1, 3, (60, 40)).astype(np.int8)
    g = ctx.geno_upload(geno)
    try:
        with Bufs(ctx) as b:
            dA = b.add(ctx.fill_uniform_cts(s, 5, 0x516))
            own = b.add(ctx.matmul_resident(dA, s, 5, L, g)).host()
            cache = b.add(ctx.rotcache_build_rows(dA, s, 5, L, 1, 0, 1))
            got = b.add(ctx.matmul_resident_range_rc(cache, s, L, g, 0, 0, 1)).host()
    finally:
        ctx.geno_free(g)
    assert np.array_equal(got, own), f"{np.count_nonzero(got != own)} words differ"
    assert all(got[i].any() for i in range(s))


# ---------------------------------------------------------------------------------------------------- 5. the stale-copy contract
def test_rewritten_cache_buffers_are_announced(pn14):
    """one cache buffer C, rewritten by every documented route between products of the int8 MAC, which keeps a transposed copy per (pointer, generation).
    What a product reads WITHOUT the announcement is not asserted: the header says it "may" be the stale copy."""
    from sfgwas_amd import capi
    ctx, s = pn14.ctx, 2
    geno = np.random.default_rng(74).integers(-1, 3, (60, 40)).astype(np.int8)
    A1, A2 = fs.host_cts(pn14.ring, s, 1, 5, 41), fs.host_cts(pn14.ring, s, 1, 5, 43)
    _, jobw, tailw = rr.layout(ol.Q_PN14, L, s, N)
    words = s * jobw + tailw
    g = ctx.geno_upload(geno)
    try:
        with Bufs(ctx) as b:
            dA1, dA2 = b.up(A1), b.up(A2)
            own1 = b.add(ctx.matmul_resident(dA1, s, 5, L, g)).host()
            own2 = b.add(ctx.matmul_resident(dA2, s, 5, L, g)).host()
            assert not np.array_equal(own1, own2)
            staged2 = b.add(ctx.rotcache_build_jobs(dA2, s, 5, L, 1, 0, s))        # before any product below: this call advances the generation itself

            def product(cache):
                out = ctx.matmul_resident_range_rc(cache, s, L, g, 0, 0, 1)
                h = out.host()
                out.free()
                return h
            # 1. build, multiply
            cbuf = b.add(ctx.rotcache_build_rows(dA1, s, 5, L, 1, 0, 1))
            assert np.array_equal(product(cbuf), own1), "step 1"
            saved1 = b.add(capi.DevArray(ctx, (words,), np.float64))
            d2d(ctx, saved1, cbuf, words)
            # 2. build_rows into the same buffer
            ctx.rotcache_build_rows(dA2, s, 5, L, 1, 0, 1, cbuf)
            assert np.array_equal(product(cbuf), own2), "step 2: build_rows rewrote the buffer"
            # 3. scatter as the only writer between two products
            ctx.rotcache_build_rows(dA1, s, 5, L, 1, 0, 1, cbuf)
            assert np.array_equal(product(cbuf), own1), "step 3, before"
            ctx.rotcache_scatter(staged2, s, L, 0, s, 0, 1, cbuf)
            assert np.array_equal(product(cbuf), own2), "step 3: scatter rewrote the buffer"
            # 4. a plain device copy of a saved cache, then invalidate
            d2d(ctx, cbuf, saved1, words)
            ctx.rotcache_invalidate()
            assert np.array_equal(product(cbuf), own1), "step 4: invalidate after a device copy"
            # 5. two buffers in turn, more products than the MAC keeps copies (sfg_ctx::I8_SLOTS = 16)
            cbuf2 = b.add(ctx.rotcache_build_rows(dA2, s, 5, L, 1, 0, 1))
            for k in range(18):
                assert np.array_equal(product(cbuf2 if k & 1 else cbuf), own2 if k & 1 else own1), f"step 5, product {k}"
            # 6. a product that builds its own operands between two products on C
            assert np.array_equal(product(cbuf), own1), "step 6, before"
            mid = b.add(ctx.matmul_resident(dA2, s, 5, L, g)).host()
            assert np.array_equal(mid, own2)
            assert np.array_equal(product(cbuf), own1), "step 6: after an own-build product"
    finally:
        ctx.geno_free(g)


# ---------------------------------------------------------------------------------------------------- 6. refusals
def test_refusals_leave_buffers_and_context_alone(pn14):
    """host-side argument checks: nonzero with a message, nothing written, and the same context builds and multiplies correctly afterwards"""
    from sfgwas_amd import capi
    ctx, s, nbr, nq = pn14.ctx, 2, 1, len(ol.Q_PN14)
    geno = np.random.default_rng(75).integers(-1, 3, (60, 40)).astype(np.int8)
    A = fs.host_cts(pn14.ring, s, nbr, 5, 47)
    _, jobw, tailw = rr.layout(ol.Q_PN14, L, s, N)
    words = s * jobw + tailw
    g = ctx.geno_upload(geno)
    refused = lambda m: pytest.raises(capi.SfgError, match=m)                      # noqa: E731
    try:
        with Bufs(ctx) as b:
            dA = b.up(A)
            dA_tall = b.add(capi.DevArray(ctx, (s, nbr, 2, nq + 1, N)))             # room for in_level = nq, never read
            before = dl(b.add(ctx.rotcache_build_rows(dA, s, 5, L, nbr, 0, nbr)), 0, words)
            own = b.add(ctx.matmul_resident(dA, s, 5, L, g)).host()
            cache, staged = b.sentinel(words), b.sentinel(words)
            for bad in (0, nq + 1):
                with refused("max_level out of range"):
                    ctx.rotcache_layout(s, bad)
                with refused("max_level out of range"):
                    ctx.rotcache_build_jobs(dA_tall, s, nq - 1, bad, nbr, 0, s, staged)
                with refused("max_level out of range"):
                    ctx.rotcache_scatter(staged, s, bad, 0, s, 0, nbr, cache)
                with refused("max_level out of range"):
                    ctx.rotcache_build_rows(dA_tall, s, nq - 1, bad, nbr, 0, nbr, cache)
            for lvl, src in ((L - 2, dA), (nq, dA_tall)):
                with refused("unusable with max_level"):
                    ctx.rotcache_build_jobs(src, s, lvl, L, nbr, 0, s, staged)
                with refused("unusable with max_level"):
                    ctx.rotcache_build_rows(src, s, lvl, L, nbr, 0, nbr, cache)
            with refused("job range out of bounds"):
                ctx.rotcache_build_jobs(dA, 0, 5, L, nbr, 0, 0, staged)
            with refused("job range outside the cache rows"):
                ctx.rotcache_scatter(staged, 0, L, 0, 0, 0, nbr, cache)
            with refused("block-row range out of bounds"):
                ctx.rotcache_build_rows(dA, 0, 5, L, nbr, 0, nbr, cache)
            for j0, j1 in ((-1, 1), (0, nbr * s + 1), (2, 1)):
                with refused("job range out of bounds"):
                    ctx.rotcache_build_jobs(dA, s, 5, L, nbr, j0, j1, staged)
            for j0, j1, row0, nrows in ((1, 4, 1, 1), (0, 3, 0, 1), (0, 0, 0, 0), (2, 1, 0, 1)):
                with refused("job range outside the cache rows"):
                    ctx.rotcache_scatter(staged, s, L, j0, j1, row0, nrows, cache)
            for b0, b1 in ((-1, 1), (0, nbr + 1), (1, 0)):
                with refused("block-row range out of bounds"):
                    ctx.rotcache_build_rows(dA, s, 5, L, nbr, b0, b1, cache)
            out = b.add(capi.DevArray(ctx, (s, 1, 2, L, N)))
            acc = b.add(capi.DevArray(ctx, (1, D, s, 2, L, N)))
            with refused("null rotation cache"):
                ctx.matmul_resident_range_rc(None, s, L, g, 0, 0, 1, out)
            with refused("null rotation cache"):
                ctx.matmul_accumulate_rc(None, s, L, g, 0, 0, 1, 0, 1, acc)
            with refused("SNP-block range out of bounds"):
                ctx.matmul_resident_range_rc(cache, s, L, g, 0, 0, 2, out)
            with refused("block range out of bounds"):
                ctx.matmul_accumulate_rc(cache, s, L, g, 0, 0, 2, 0, 1, acc)
            assert (dl(cache, 0, words + GUARD) == SENT).all() and (dl(staged, 0, words + GUARD) == SENT).all(), "a refused call wrote"
            # the context afterwards
            ctx.rotcache_build_rows(dA, s, 5, L, nbr, 0, nbr, cache)
            assert np.array_equal(dl(cache, 0, words), before)
            got = b.add(ctx.matmul_resident_range_rc(cache, s, L, g, 0, 0, 1)).host()
            assert np.array_equal(got, own)
    finally:
        ctx.geno_free(g)


def test_a_missing_baby_key_is_refused_by_name(zero_keys):
    """a context that lacks the key of baby step 90 (this refusal comes after the operand gather and the conversion of baby step 0 were queued: the buffer is not
    asserted untouched); with the key loaded the same context gives what the complete one gives"""
    from sfgwas_amd import capi
    e = zero_keys
    ctx = capi.Context(ol.Q_PN14, ol.P_PN14)
    try:
        z = np.zeros((e.ring.beta, 2, len(e.ring.moduli), N), dtype=np.uint64)
        for k in range(1, D - 1):
            ctx.load_rotkey(e.ring.galois(k), z)
        A = e.ring.fill_uniform(5, 67)[None, None]
        want, _ = build_rows_host(e.ctx, A, 1, 5, L, 1, 0, 1, ol.Q_PN14)
        _, jobw, tailw = rr.layout(ol.Q_PN14, L, 1, N)
        with Bufs(ctx) as b:
            dA = b.up(A)
            cache, staged = b.sentinel(jobw + tailw), b.sentinel(jobw)
            with pytest.raises(capi.SfgError, match="no rotation key loaded for right-rotation by 8102"):
                ctx.rotcache_build_rows(dA, 1, 5, L, 1, 0, 1, cache)
            with pytest.raises(capi.SfgError, match="no rotation key loaded"):
                ctx.rotcache_build_jobs(dA, 1, 5, L, 1, 0, 1, staged)
        ctx.load_rotkey(e.ring.galois(D - 1), z)
        got, _ = build_rows_host(ctx, A, 1, 5, L, 1, 0, 1, ol.Q_PN14)
        check_f64(got, want, "after the key was loaded")
    finally:
        ctx.close()
