"""Quality control on the resident matrix: sfg_geno_qc_scan (one pass, exact counts), sfg_geno_filter (the filtered matrix, resident) and the scan on the sharded
matrix, every count compared for EQUALITY with tests/qc_ref.py (itself pinned against literal loops by tests/test_qc_ref.py).

Shapes: 1 x 1, 3 x 5 (smaller than any tile), 257 x 4099 (ragged both ways; 4099 is no multiple of 16, so a packed row ends in padding codes), 4097 x 300 (17 row
chunks of 256), 70 000 x 48 (more rows than a grid dimension), and 8 200 000 x 1: the one shape at which a row chunk reaches its largest size (1984 rows), so that
the 16-bit lanes are filled as far as they ever are.  Constant rows / columns fill every narrow lane to its limit."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle_lib as ol
import qc_ref

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
FX = np.load(os.path.join(GOLD, "input_formats.npz"))
SHAPES = [(1, 1), (3, 5), (257, 4099), (4097, 300), (70_000, 48)]


@pytest.fixture(scope="module")
def ctx():
    from sfgwas_amd import capi
    c = capi.Context(ol.Q_PN14, ol.P_PN14)
    yield c
    c.close()


def pack(ctx, g):
    from sfgwas_amd import capi
    out = C.c_void_p()
    ctx.check(capi.lib().sfg_geno_pack(ctx.h, g, C.byref(out)), "geno_pack")
    return out


def make_geno(nrow, ncol, seed):
    """every value of -128 .. 2 occurs: every negative is missing, not only -1"""
    rnd = np.random.default_rng(seed)
    geno = rnd.choice(np.array([-1, 0, 1, 2], dtype=np.int8), size=(nrow, ncol), p=[0.1, 0.4, 0.3, 0.2])
    neg = rnd.random((nrow, ncol)) < 0.05
    geno[neg] = rnd.integers(-128, 0, int(neg.sum())).astype(np.int8)
    if nrow >= 4096:                                                   # constant columns: all 1, all missing, all 2
        geno[:, 0], geno[:, 1], geno[:, 2] = 1, -5, 2
    if ncol >= 4096:                                                   # constant rows
        geno[0, :], geno[1, :], geno[2, :] = 1, -128, 2
    return geno


def filters(nrow, ncol, seed):
    rnd = np.random.default_rng(seed + 1000)
    return (rnd.random(nrow) < 0.7).astype(np.uint8), (rnd.random(ncol) < 0.6).astype(np.uint8), (rnd.random(nrow) < 0.5).astype(np.uint8)


def check_scan(ctx, g, geno, rf, cf, ctrl, what):
    want = qc_ref.scan(geno, rf, cf, ctrl)
    got = ctx.geno_qc_scan(g, rf, cf, ctrl)
    for name, a, b in zip(("col_counts", "row_miss", "row_het"), got, want):
        assert a.dtype == np.uint32 and a.shape == b.shape and np.array_equal(a, b), f"{what}: {name} differs at {np.argwhere(a != b)[:5].tolist()}"
    only_cols = ctx.geno_qc_scan(g, rf, cf, ctrl, rows=False)
    only_rows = ctx.geno_qc_scan(g, rf, cf, ctrl, cols=False)
    assert only_cols[1] is None and only_cols[2] is None and only_rows[0] is None
    assert np.array_equal(only_cols[0], got[0]) and np.array_equal(only_rows[1], got[1]) and np.array_equal(only_rows[2], got[2]), f"{what}: partial outputs disagree"
    return got


@pytest.fixture(scope="module")
def cases(ctx):
    """per shape: the host matrix, its int8 handle and its packed handle (made once, shared by the tests below)"""
    out = {}
    for k, (nrow, ncol) in enumerate(SHAPES):
        geno = make_geno(nrow, ncol, 40 + k)
        g = ctx.geno_upload(geno)
        out[(nrow, ncol)] = (geno, g, pack(ctx, g))
    yield out
    for _, g, gp in out.values():
        ctx.geno_free(g)
        ctx.geno_free(gp)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("mode", ["filters", "null", "ctrl_only"])
def test_scan_counts_equal_the_reference_int8_and_packed(ctx, cases, shape, mode):
    geno, g, gp = cases[shape]
    rf, cf, ctrl = filters(*shape, seed=shape[0])
    if mode == "null":
        rf = cf = ctrl = None
    elif mode == "ctrl_only":
        rf = cf = None
    a = check_scan(ctx, g, geno, rf, cf, ctrl, f"int8 {shape} {mode}")
    b = check_scan(ctx, gp, geno, rf, cf, ctrl, f"packed {shape} {mode}")
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    if mode == "null" and shape[0] >= 4096:                            # the constant columns, whole: no narrow counter wrapped
        assert a[0][0, 1, 0] == shape[0] and a[0][0, 3, 1] == shape[0] and a[0][0, 2, 2] == shape[0]
    if mode == "null" and shape[1] >= 4096:
        assert a[2][0] == shape[1] and a[1][1] == shape[1] and a[1][2] == 0


def test_scan_at_the_largest_row_chunk(ctx):
    """8 200 000 x 1: 1984 rows per chunk; a constant column, and a column of every value.  (The handle is made from one flat device copy: a pitched upload of
    eight million one-byte rows takes a minute.)"""
    from sfgwas_amd import capi
    lib = capi.lib()
    nrow = 8_200_000
    for fill in ("ones", "random"):
        geno = np.ones((nrow, 1), dtype=np.int8) if fill == "ones" else np.random.default_rng(8).integers(-128, 3, (nrow, 1)).astype(np.int8)
        ctrl = (np.arange(nrow) % 3 == 0).astype(np.uint8)
        buf = ctx.to_device(geno)
        g = C.c_void_p()
        ctx.check(lib.sfg_geno_from_device(ctx.h, buf, nrow, 1, 1, C.byref(g)), "geno_from_device")
        gp = pack(ctx, g)
        want = qc_ref.scan(geno, None, None, ctrl)
        for h in (g, gp):
            got = ctx.geno_qc_scan(h, None, None, ctrl)
            assert all(np.array_equal(x, y) for x, y in zip(got, want))
        if fill == "ones":
            assert want[0][0, 1, 0] == nrow
        ctx.geno_free(g)
        ctx.geno_free(gp)
        ctx.free(buf)


def test_scan_of_a_handle_on_an_odd_address_with_a_row_stride(ctx):
    from sfgwas_amd import capi
    lib = capi.lib()
    nrow, ncol, ld = 300, 4099, 4099 + 14
    geno = make_geno(nrow, ncol, 77)
    padded = np.full((nrow, ld), 77, dtype=np.int8)                    # the bytes between the rows are not genotypes and must not be looked at
    padded[:, :ncol] = geno
    buf = ctx.malloc(nrow * ld + 16)
    base = C.c_void_p(buf.value + 1)
    ctx.check(lib.sfg_memcpy_h2d(ctx.h, base, padded.ctypes.data_as(C.c_void_p), padded.nbytes), "h2d")
    g = C.c_void_p()
    ctx.check(lib.sfg_geno_from_device(ctx.h, base, nrow, ncol, ld, C.byref(g)), "geno_from_device")
    rf, cf, ctrl = filters(nrow, ncol, 5)
    check_scan(ctx, g, geno, rf, cf, ctrl, "odd base, ld > ncol")
    check_scan(ctx, g, geno, None, None, None, "odd base, ld > ncol, no filters")
    gf = ctx.geno_filter(g, rf, cf)
    assert np.array_equal(ctx.geno_to_host(gf), qc_ref.filter_matrix(geno, rf, cf))
    for h in (gf, g):
        ctx.geno_free(h)
    ctx.free(buf)


def test_value_above_two_fails_only_at_a_kept_position(ctx):
    from sfgwas_amd import capi
    geno = make_geno(300, 500, 9)
    rf, cf, ctrl = filters(300, 500, 9)
    r_drop, c_drop = int(np.flatnonzero(rf == 0)[0]), int(np.flatnonzero(cf == 0)[0])
    r_keep, c_keep = np.flatnonzero(rf)[:2], np.flatnonzero(cf)[:2]
    geno[r_drop, c_keep[0]] = 3                                        # dropped row
    geno[r_keep[0], c_drop] = 100                                      # dropped column
    g = ctx.geno_upload(geno)
    check_scan(ctx, g, geno, rf, cf, ctrl, "bad values at dropped positions")
    with pytest.raises(capi.SfgError, match="2 values above 2"):
        ctx.geno_qc_scan(g)
    ctx.geno_free(g)
    geno[r_keep[0], c_keep[0]], geno[r_keep[1], c_keep[1]], geno[r_keep[1], c_keep[0]] = 3, 127, 4
    g = ctx.geno_upload(geno)
    for kw in ({}, {"rows": False}, {"cols": False}):
        with pytest.raises(capi.SfgError, match="3 values above 2"):
            ctx.geno_qc_scan(g, rf, cf, ctrl, **kw)
    ctx.geno_free(g)


def test_empty_filters_single_entry_and_argument_errors(ctx, cases):
    from sfgwas_amd import capi
    geno, g, gp = cases[(257, 4099)]
    nrow, ncol = geno.shape
    for h in (g, gp):
        for rf, cf in ((np.zeros(nrow, np.uint8), None), (None, np.zeros(ncol, np.uint8)), (np.zeros(nrow, np.uint8), np.zeros(ncol, np.uint8))):
            got = ctx.geno_qc_scan(h, rf, cf, np.ones(nrow, np.uint8))
            assert not got[0].any() and not got[1].any() and not got[2].any()
        rf, cf = np.zeros(nrow, np.uint8), np.zeros(ncol, np.uint8)
        rf[200], cf[4098] = 1, 1                                       # the last column: the last code before a packed row's padding
        check_scan(ctx, h, geno, rf, cf, np.ones(nrow, np.uint8), "single entry")
    with pytest.raises(capi.SfgError, match="no output"):
        ctx.geno_qc_scan(g, cols=False, rows=False)
    with pytest.raises(capi.SfgError, match="null matrix"):
        ctx.geno_qc_scan(None)
    with pytest.raises(capi.SfgError, match="keep nothing"):
        ctx.geno_filter(g, np.zeros(nrow, np.uint8), None)
    with pytest.raises(capi.SfgError, match="keep nothing"):
        ctx.geno_filter(gp, None, np.zeros(ncol, np.uint8))


def test_scratch_does_not_grow_with_the_matrix(ctx):
    """what the context keeps after a scan and a filter is O(nrow + ncol) - no int8 copy of a packed handle, no nrow x ncol temporary"""
    from sfgwas_amd import capi
    lib = capi.lib()

    def held(prefix):
        n = C.c_size_t()
        ctx.check(lib.sfg_ctx_scratch_bytes(ctx.h, prefix.encode(), C.byref(n)), "scratch_bytes")
        return n.value

    ctx.check(lib.sfg_ctx_release_scratch(ctx.h), "release_scratch")
    nrow, ncol = 3000, 3000
    geno = make_geno(nrow, ncol, 13)
    g = ctx.geno_upload(geno)
    gp = pack(ctx, g)
    rf, cf, ctrl = filters(nrow, ncol, 3)
    for h in (g, gp):
        check_scan(ctx, h, geno, rf, cf, ctrl, "3000 x 3000")
        ctx.geno_free(ctx.geno_filter(h, rf, cf))
    bound = 4 * (4 + 6 * ncol + 2 * nrow) + 2 * nrow + ncol + 4 * (nrow + ncol)        # the counts, the filters, the kept-index lists
    assert 0 < held("qc.") <= bound < nrow * ncol // 16                # a small fraction of the packed handle itself
    assert held("") == held("qc.")
    ctx.geno_free(g)
    ctx.geno_free(gp)


def test_scan_of_party1_equals_the_reference_held_genotype_counts(ctx):
    """the 22 chromosome files of the reference's example data, decoded on the device and scanned without filters: HOM_REF_CT, HET_REF_ALT_CTS,
    TWO_ALT_GENO_CTS, MISSING_CT of the geno-count file the reference reads (gwas/qualcontrol.go:595)"""
    ref = np.fromfile(os.path.join(GOLD, "example_party1", "all.gcount.transpose.bin"), dtype=np.uint32).reshape(6, -1)
    got = []
    for c in range(1, 23):
        img = np.fromfile(os.path.join(GOLD, "example_party1", "geno", f"chr{c}.pgen"), dtype=np.uint8)
        g = ctx.geno_from_pgen(img)
        gp = pack(ctx, g)
        a, b = ctx.geno_qc_scan(g, rows=False)[0], ctx.geno_qc_scan(gp, rows=False)[0]
        assert np.array_equal(a, b) and not a[1].any()
        got.append(a[0])
        ctx.geno_free(g)
        ctx.geno_free(gp)
    got = np.concatenate(got, axis=1)
    assert got.shape[1] == ref.shape[1]
    for k, row in enumerate((0, 1, 2, 5)):
        assert np.array_equal(got[k], ref[row]), f"genotype count {k} differs from the reference-held file"


@pytest.mark.parametrize("k", range(6))
def test_filter_equals_the_fixtures_int8_and_packed(ctx, k):
    geno, rf, cf = FX[f"geno_{k}"], FX[f"rowfilt_{k}"], FX[f"colfilt_{k}"]
    g = ctx.geno_upload(geno)
    gp = pack(ctx, g)
    for r, c in ((rf, cf), (None, None), (rf, None), (None, cf)):
        want = qc_ref.filter_matrix(geno, r, c)
        if r is not None and c is not None:
            assert np.array_equal(want, FX[f"filtered_{k}"])
        f8, f2 = ctx.geno_filter(g, r, c), ctx.geno_filter(gp, r, c)
        a, b = ctx.geno_to_host(f8), ctx.geno_to_host(f2)
        assert a.shape == want.shape and np.array_equal(a, want) and np.array_equal(b, want)
        ctx.geno_free(f8)
        ctx.geno_free(f2)
    ctx.geno_free(g)
    ctx.geno_free(gp)


def test_filter_of_a_ragged_matrix_and_of_many_rows(ctx, cases):
    """257 x 4099 (the re-packed rows cross dword boundaries; the last output dword is padded with code 0) and 70 000 rows (more than a grid dimension);
    a filtered packed handle downloads and scans like the filtered matrix"""
    for shape in ((257, 4099), (70_000, 48)):
        geno, g, gp = cases[shape]
        rf, cf, ctrl = filters(*shape, seed=11)
        want = qc_ref.filter_matrix(geno, rf, cf)
        f8, f2 = ctx.geno_filter(g, rf, cf), ctx.geno_filter(gp, rf, cf)
        # (a packed handle holds one missing code: it downloads every negative as -1)
        assert np.array_equal(ctx.geno_to_host(f8), want) and np.array_equal(ctx.geno_to_host(f2), np.where(want < 0, -1, want))
        check_scan(ctx, f2, want, None, None, ctrl[rf != 0], f"filtered packed {shape}")
        for h in (f8, f2):
            ctx.geno_free(h)


def test_product_over_a_filtered_handle_equals_the_product_over_the_host_filtered_matrix(ctx):
    from sfgwas_amd import capi
    lib = capi.lib()
    rots = list(range(1, 91)) + [g * 91 for g in range(1, 91) if g * 91 < 8192]
    ctx.check(lib.sfg_fill_rotkeys_synthetic(ctx.h, (C.c_int * len(rots))(*rots), len(rots), 0xBEEF), "keys")
    rnd = np.random.default_rng(12)
    geno = rnd.integers(-1, 3, (60, 40)).astype(np.int8)
    rf, cf = (rnd.random(60) < 0.7).astype(np.uint8), (rnd.random(40) < 0.7).astype(np.uint8)
    g = ctx.geno_upload(geno)
    gp = pack(ctx, g)
    ghost = ctx.geno_upload(qc_ref.filter_matrix(geno, rf, cf))
    A = ctx.fill_uniform_cts(1, 5, 0x51)
    want = ctx.matmul_resident(A, 1, 5, 5, ghost).host()
    assert want.any()
    for h in (g, gp):
        f = ctx.geno_filter(h, rf, cf)
        assert np.array_equal(ctx.matmul_resident(A, 1, 5, 5, f).host(), want)
        ctx.geno_free(f)
    A.free()
    for h in (g, gp, ghost):
        ctx.geno_free(h)


@pytest.mark.parametrize("devices", [[0, 0], [0, 0, 0]])
def test_sharded_scan_equals_the_single_context_scan(ctx, devices):
    """300 x 20 000: three blocks of 8192 SNP columns, so two ranks own one and two blocks and three ranks one each (the last one ragged)"""
    from sfgwas_amd import capi
    nrow, ncol = 300, 20_000
    geno = make_geno(nrow, ncol, 21)
    rf, cf, ctrl = filters(nrow, ncol, 21)
    g = ctx.geno_upload(geno)
    mg = capi.MultiGpu(ol.Q_PN14, ol.P_PN14, devices=devices)
    assert mg.transport == "direct"
    m = mg.geno_upload(geno)
    assert len({mg.geno_blocks(m, i) for i in range(len(devices))}) == len(devices)
    for a in ((rf, cf, ctrl), (None, None, None), (None, cf, None)):
        single, sharded = ctx.geno_qc_scan(g, *a), mg.geno_qc_scan(m, *a)
        want = qc_ref.scan(geno, *a)
        for x, y, z in zip(single, sharded, want):
            assert np.array_equal(x, y) and np.array_equal(y, z)
    only_rows = mg.geno_qc_scan(m, rf, cf, ctrl, cols=False)
    assert only_rows[0] is None and np.array_equal(only_rows[1], qc_ref.scan(geno, rf, cf, ctrl)[1])
    with pytest.raises(capi.SfgError, match="no output"):
        mg.geno_qc_scan(m, cols=False, rows=False)
    mg.geno_free(m)
    mg.close()
    ctx.geno_free(g)
