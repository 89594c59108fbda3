"""From quality control to the PCA on the sharded matrix: sfg_mgpu_geno_filter (the filter that re-shards), sfg_mgpu_sketch and sfg_mgpu_geno_colsums.

Every rank runs on device 0 (the in-process `direct` transport: ranks that share a device read each other's shards with plain loads), at worlds 1, 2, 3 and 8.
A new shard is compared byte for byte with tests/reshard_ref.py - what it downloads, and what lies in device memory behind it (row padding, padding codes) - and
the inputs are those tests/test_reshard_ref.py shows to reach every case: output dwords that take their columns from two old ranks, windows that draw on three,
ranks without a window before or after, an old window dropped whole, a first column at an odd offset of its shard.  Peer access between two physical devices and
the refusal in a world of one rank per process cannot be reached on one device."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as ol
import qc_ref
import reshard_ref as rr
from sfgwas_amd.sharding import SLOTS, snp_block_range

pytestmark = pytest.mark.gpu
D, L, LEVEL, S, T = 91, 5, 5, 2, 2
ROTS = list(range(1, D)) + [g * D for g in range(1, D) if g * D < SLOTS]


@pytest.fixture(scope="module")
def engines():
    """one engine per world size, made when first asked for, all ranks on device 0"""
    from sfgwas_amd import capi
    made = {}

    def get(world):
        if world not in made:
            made[world] = capi.MultiGpu(ol.Q_PN14, ol.P_PN14, devices=[0] * world)
            assert made[world].transport == ("none" if world == 1 else "direct")
        return made[world]
    yield get
    for mg in made.values():
        mg.close()


@pytest.fixture(scope="module")
def ctx():
    from sfgwas_amd import capi
    c = capi.Context(ol.Q_PN14, ol.P_PN14)
    yield c
    c.close()


def pack_sharded(mg, m, nrow, ncol):
    """the 2-bit packed form of a sharded int8 matrix: every rank packs its window, the engine adopts the packed windows"""
    from sfgwas_amd import capi
    lib = capi.lib()
    hs = []
    for i in range(mg.nlocal):
        sh, p = mg.geno_shard(m, i), C.c_void_p()
        if sh is not None:
            mg.ctx[i].check(lib.sfg_geno_pack(mg.ctx[i].h, sh, C.byref(p)), "geno_pack")
        hs.append(p)
    out = C.c_void_p()
    mg.check(lib.sfg_mgpu_geno_adopt(mg.h, nrow, ncol, (C.c_void_p * mg.nlocal)(*hs), C.byref(out)), "adopt")
    return out


def device_image(c, h):
    """the bytes behind a resident handle: [nrow][row stride]"""
    from sfgwas_amd import capi
    nr, nc = C.c_size_t(), C.c_size_t()
    capi.lib().sfg_geno_dims(h, C.byref(nr), C.byref(nc))
    dev, ld, packed = capi.geno_layout(h)
    return c.to_host(C.c_void_p(dev), (nr.value, ld), np.uint8), packed


def check_result(mg, f, geno, rf, cf, packed, what, image=True):
    """every shard of the sharded matrix f against the reference windows of geno[rf][:, cf]; image: also the bytes in device memory, as the filter lays them out"""
    want = rr.windows(geno, rf, cf, mg.world)
    nr, nc = int(rr.mask(rf, geno.shape[0]).sum()), int(rr.mask(cf, geno.shape[1]).sum())
    assert mg.geno_dims(f) == (nr, nc), what
    for i in range(mg.nlocal):
        assert mg.geno_blocks(f, i) == snp_block_range(nc, mg.ranks[i], mg.world)[:2], what
        sh = mg.geno_shard(f, i)
        if want[i] is None:
            assert sh is None, f"{what}: rank {i} has a shard without a window"
            continue
        assert sh is not None, f"{what}: rank {i} has no shard"
        got = mg.ctx[i].geno_to_host(sh)
        assert got.shape == want[i].shape and np.array_equal(got, want[i]), f"{what}: rank {i} differs at {np.argwhere(got != want[i])[:5].tolist()}"
        if not image:
            continue
        img, is_packed = device_image(mg.ctx[i], sh)
        assert is_packed == packed
        ref = rr.packed_image(want[i]).view(np.uint8) if packed else rr.int8_image(want[i]).view(np.uint8)
        assert img.shape == ref.shape and np.array_equal(img, ref), f"{what}: rank {i}: the bytes in device memory (padding included) differ"


def filter_both(mg, geno, rf, cf, what):
    """filter the int8 and the packed form of geno on mg, check both, leave the sources unchanged; returns nothing (everything is freed)"""
    m8 = mg.geno_upload(geno)
    m2 = pack_sharded(mg, m8, *geno.shape)
    for m, packed in ((m8, False), (m2, True)):
        f = mg.geno_filter(m, rf, cf)
        check_result(mg, f, geno, rf, cf, packed, f"{what} {'packed' if packed else 'int8'} world {mg.world}")
        check_result(mg, m, geno, None, None, packed, f"{what}: the source after the call", image=False)
        mg.geno_free(f)
        mg.geno_free(m)


@pytest.mark.parametrize("world", rr.WORLDS)
def test_thirteen_blocks_keep_five_int8_and_packed(engines, world):
    filter_both(engines(world), *rr.case("blocks13"), "13 blocks")


def test_an_old_window_dropped_whole(engines):
    filter_both(engines(3), *rr.case("window_dropped"), "old rank 1 dropped")


def test_five_blocks_at_world_8_three_old_ranks_own_nothing(engines):
    filter_both(engines(8), *rr.case("blocks5"), "5 blocks")


def test_the_source_may_be_freed_at_once(engines):
    """the call returns with every queue drained: the result does not depend on the source's memory"""
    mg = engines(3)
    geno, rf, cf = rr.case("blocks13")
    m = mg.geno_upload(geno)
    f = mg.geno_filter(m, rf, cf)
    mg.geno_free(m)
    junk = mg.geno_upload(np.full(geno.shape, 2, dtype=np.int8))       # most likely the memory the source had
    check_result(mg, f, geno, rf, cf, False, "source freed")
    mg.geno_free(junk)
    mg.geno_free(f)


def _edge_cases():
    nrow, ncol = 9, 2 * SLOTS + 100
    rnd = np.random.default_rng(5)
    rf = (rnd.random(nrow) < 0.6).astype(np.uint8)
    cf = (rnd.random(ncol) < 0.5).astype(np.uint8)

    def keep(k):                                                     # k columns, spread over both old windows
        f = np.zeros(ncol, dtype=np.uint8)
        f[np.sort(rnd.choice(ncol, k, replace=False))] = 1
        assert f[:SLOTS].any() and f[SLOTS:].any()
        return f
    return nrow, ncol, {"copy": (None, None), "rows_only": (rf, None), "cols_only": (None, cf), "5_cols": (rf, keep(5)), "8192_cols": (rf, keep(SLOTS)),
                        "8193_cols": (None, keep(SLOTS + 1))}


@pytest.mark.parametrize("name", ["copy", "rows_only", "cols_only", "5_cols", "8192_cols", "8193_cols"])
def test_small_edge_shapes(engines, name):
    nrow, ncol, cases = _edge_cases()
    rf, cf = cases[name]
    geno = rr.make_geno(nrow, ncol, 6)
    mg = engines(2)
    if name == "copy":                                               # the same windows as the source
        m = mg.geno_upload(geno)
        f = mg.geno_filter(m)
        assert [mg.geno_blocks(f, i) for i in range(2)] == [mg.geno_blocks(m, i) for i in range(2)] and mg.geno_dims(f) == mg.geno_dims(m)
        mg.geno_free(f)
        mg.geno_free(m)
    filter_both(mg, geno, rf, cf, name)


def test_more_rows_than_a_grid_dimension(engines):
    """65 539 x 40 at world 2: one block, rank 1 owns nothing before and after; every third row is kept"""
    nrow, ncol = 65_539, 40
    geno = rr.make_geno(nrow, ncol, 8)
    rf = (np.arange(nrow) % 3 == 0).astype(np.uint8)
    cf = (np.random.default_rng(8).random(ncol) < 0.7).astype(np.uint8)
    filter_both(engines(2), geno, rf, cf, "65539 rows")


def test_products_and_the_scan_over_a_resharded_matrix(engines, ctx):
    """world 3, 3 x 8192 + 5 columns of which about 2.2 blocks are kept: Q X and Q' X^T over the re-sharded matrix give the words of the single-context product
    over sfg_geno_filter of the same matrix; the sharded scan, sketch and column moments of the result are those of the filtered matrix"""
    from sfgwas_amd import capi
    lib = capi.lib()
    nrow, ncol = 60, 3 * SLOTS + 5
    geno = rr.make_geno(nrow, ncol, 9)
    rf, cf = rr.make_filters(nrow, ncol, 9, p_row=0.8, p_col=0.73)
    nc = int(cf.sum())
    assert 2 * SLOTS < nc <= 3 * SLOTS
    ctx.check(lib.sfg_fill_rotkeys_synthetic(ctx.h, (C.c_int * len(ROTS))(*ROTS), len(ROTS), 0xBEEF), "keys")
    g = ctx.geno_upload(geno)
    gf = ctx.geno_filter(g, rf, cf)
    A = {0: ctx.fill_uniform_cts(S * 1, LEVEL, 0xC1), T: ctx.fill_uniform_cts(S * 3, LEVEL, 0xC2)}
    Ah = {f: a.host().reshape(S, -1, 2, LEVEL + 1, ctx.N) for f, a in A.items()}
    want = {}
    for f in (0, T):
        o = ctx.matmul_resident(A[f], S, LEVEL, L, gf, f)
        want[f] = o.host().copy()
        o.free()
        A[f].free()
    mg = engines(3)
    mg.fill_rotkeys_synthetic(ROTS, 0xBEEF)
    filtered = qc_ref.filter_matrix(geno, rf, cf)
    ctrl = (np.arange(filtered.shape[0]) % 2).astype(np.uint8)
    rnd = np.random.default_rng(10)
    bucket, sgn = rnd.integers(0, 7, filtered.shape[0]).astype(np.int32), rnd.choice(np.array([-1, 1], dtype=np.int8), filtered.shape[0])
    m8 = mg.geno_upload(geno)
    m2 = pack_sharded(mg, m8, nrow, ncol)
    for m, packed in ((m8, False), (m2, True)):
        f = mg.geno_filter(m, rf, cf)
        for fl in (0, T):
            got = mg.matmul(Ah[fl], S, LEVEL, L, f, fl)
            assert got.shape == want[fl].shape and want[fl].any()
            assert np.array_equal(got, want[fl]), f"packed {packed} flags {fl}: {np.count_nonzero(got != want[fl])} words differ"
        for a, b in zip(mg.geno_qc_scan(f, None, None, ctrl), qc_ref.scan(filtered, None, None, ctrl)):
            assert np.array_equal(a, b)
        for a, b in zip(mg.geno_colsums(f), ctx.geno_colsums(gf)):
            assert np.array_equal(a, b)
        if not packed:                                               # (the padded row stride of an int8 shard under the sketch)
            for a, b in zip(mg.sketch(f, bucket, sgn, 7), ctx.sketch(gf, bucket, sgn, 7)):
                assert np.array_equal(a, b)
        mg.geno_free(f)
        mg.geno_free(m)
    ctx.geno_free(gf)
    ctx.geno_free(g)


@pytest.fixture(scope="module")
def moments(ctx):
    """the single-context sketch and column moments of the two whole matrices (computed once)"""
    out = {}
    for name in ("blocks13", "blocks5"):
        geno = rr.case(name)[0]
        rnd = np.random.default_rng(len(name))
        bucket, sgn = rnd.integers(0, 10, geno.shape[0]).astype(np.int32), rnd.choice(np.array([-1, 1], dtype=np.int8), geno.shape[0])
        g = ctx.geno_upload(geno)
        out[name] = (bucket, sgn, ctx.sketch(g, bucket, sgn, 10), ctx.geno_colsums(g))
        ctx.geno_free(g)
    return out


@pytest.mark.parametrize("world", [1, 3, 8])
@pytest.mark.parametrize("name", ["blocks13", "blocks5"])
def test_sharded_sketch_and_column_moments_equal_the_single_context_calls(engines, moments, world, name):
    from sfgwas_amd import capi
    mg = engines(world)
    geno = rr.case(name)[0]
    bucket, sgn, want_sk, want_cs = moments[name]
    assert want_sk[0].any() and want_sk[1].any() and want_cs[0].any()
    m = mg.geno_upload(geno)
    got = mg.sketch(m, bucket, sgn, 10)
    for a, b in zip(got, want_sk):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    for a, b in zip(mg.geno_colsums(m), want_cs):
        assert a.dtype == np.float64 and np.array_equal(a, b)
    # NULL outputs
    only_sk, only_sums = mg.sketch(m, bucket, sgn, 10, sums=False), mg.sketch(m, bucket, sgn, 10, sketch=False)
    assert only_sk[1] is None and only_sk[2] is None and only_sums[0] is None
    assert np.array_equal(only_sk[0], want_sk[0]) and np.array_equal(only_sums[1], want_sk[1]) and np.array_equal(only_sums[2], want_sk[2])
    s_only, q_only = mg.geno_colsums(m, sqsums=False), mg.geno_colsums(m, sums=False)
    assert s_only[1] is None and q_only[0] is None and np.array_equal(s_only[0], want_cs[0]) and np.array_equal(q_only[1], want_cs[1])
    if world == 3:                                                   # a packed matrix: refused by the sketch as on one GPU, summed like the int8 one
        p = pack_sharded(mg, m, *geno.shape)
        with pytest.raises(capi.SfgError, match="sfg_sketch: 2-bit packed matrix"):
            mg.sketch(p, bucket, sgn, 10)
        for a, b in zip(mg.geno_colsums(p), want_cs):
            assert np.array_equal(a, b)
        mg.geno_free(p)
    mg.geno_free(m)


def test_refusals_launch_nothing_and_leave_the_engine_usable(engines):
    from sfgwas_amd import capi
    lib = capi.lib()
    mg = engines(2)
    nrow, ncol, cases = _edge_cases()
    geno = rr.make_geno(nrow, ncol, 6)
    m = mg.geno_upload(geno)

    def held():                                                      # device memory the ranks' contexts hold as scratch
        n = C.c_size_t()
        total = 0
        for c in mg.ctx:
            c.check(lib.sfg_ctx_scratch_bytes(c.h, b"qc.", C.byref(n)), "scratch_bytes")
            total += n.value
        return total

    for c in mg.ctx:
        c.check(lib.sfg_ctx_release_scratch(c.h), "release_scratch")
    assert held() == 0
    for rf, cf in ((np.zeros(nrow, np.uint8), None), (None, np.zeros(ncol, np.uint8))):
        out = C.c_void_p(1)
        rfp = None if rf is None else rf.ctypes.data_as(C.c_void_p)
        cfp = None if cf is None else cf.ctypes.data_as(C.c_void_p)
        assert lib.sfg_mgpu_geno_filter(mg.h, m, rfp, cfp, C.byref(out)) != 0 and out.value is None
        assert b"keep nothing" in lib.sfg_mgpu_last_error(mg.h)
    out = C.c_void_p(1)
    assert lib.sfg_mgpu_geno_filter(mg.h, None, None, None, C.byref(out)) != 0 and out.value is None and b"null matrix" in lib.sfg_mgpu_last_error(mg.h)
    assert lib.sfg_mgpu_geno_filter(mg.h, m, None, None, None) != 0 and b"null matrix" in lib.sfg_mgpu_last_error(mg.h)
    with pytest.raises(capi.SfgError, match="keep nothing"):
        mg.geno_filter(m, np.zeros(nrow, np.uint8), np.zeros(ncol, np.uint8))
    assert held() == 0                                               # not even the index tables were asked for
    # after a refusal: a good call on the same engine
    rf, cf = cases["rows_only"][0], cases["cols_only"][1]
    f = mg.geno_filter(m, rf, cf)
    check_result(mg, f, geno, rf, cf, False, "after a refusal")
    kept = int(rr.mask(rf, nrow).sum()) + max(len(c) for c in rr.new_windows(ncol, cf, 2))
    assert 0 < held() <= 2 * 4 * kept                                # the temporaries: index tables only, O(kept rows + window columns) per rank
    mg.geno_free(f)
    mg.geno_free(m)
