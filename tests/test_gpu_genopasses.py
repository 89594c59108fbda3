"""The plaintext passes over the resident genotype matrix at the row counts the workload runs: k_sketch (sketch.hip), k_colsums (matmul.hip), k_geno_pack,
k_geno_unpack<VEC>, k_geno_transpose, k_bed_decode and the 2-D copies of concat / download (genoio.hip).  Every output word is compared for EQUALITY with
tests/genopass_ref.py, which tests/test_genopass_ref.py holds against literal loops and against the oracle at the same tall shapes.

What the shapes are for (genopass_ref.SKETCH_TALL says it once more where they are defined):
  sketch      chunks of 16384 rows (grid.y) clipped at the last row and combined with atomics, strips of 256 columns, tiles of 64 rows;
  column sums chunks of 4096 rows, strips of 256 columns;
  pack/unpack launches of 65535 rows; the 16-byte form of the unpack (ncol a multiple of 16) and its byte form;
  views       a matrix inside a larger device buffer full of a sentinel: odd row strides and bases off a 16-byte boundary select the byte-wise loads, and
              a read outside the window changes a sum.
NOT covered, and not coverable: the sketch's int32 -> fp64 flush after 2^16 rows of one workgroup (a workgroup never has more than 16384 rows), and a
ragged last dword in the 16-byte unpack (sfg_geno_unpack hands it rows of ncol bytes, so that form is taken only when ncol is a multiple of 16; the
products' windows reach it)."""
import ctypes as C

import numpy as np
import pytest

import genopass_ref as gr
import oracle_lib as ol

pytestmark = pytest.mark.gpu
SENTINELS = [77, -128]


@pytest.fixture(scope="module")
def ctx():
    from sfgwas_amd import capi
    c = capi.Context(ol.Q_PN14, ol.P_PN14)
    yield c
    c.close()


def same(got, want, what):
    for n, (a, b) in enumerate(zip(got, want)):
        assert a.dtype == b.dtype and a.shape == b.shape, f"{what}: output {n} is {a.dtype}{a.shape}, expected {b.dtype}{b.shape}"
        if not np.array_equal(a, b):
            at = np.argwhere(a != b)
            first = tuple(at[0])
            raise AssertionError(f"{what}: output {n} differs in {len(at)} words, first at {first}: got {a[first]!r}, expected {b[first]!r}")


class View:
    """X inside a larger device buffer filled with `sentinel`: row i starts at byte off + i * ld"""

    def __init__(self, ctx, X, ld, off, sentinel):
        from sfgwas_amd import capi
        nrow, ncol = X.shape
        assert ld >= ncol and 0 <= off < 16
        host = np.full(16 + nrow * ld + 16, sentinel, dtype=np.int8)
        body = host[off:off + nrow * ld].reshape(nrow, ld)
        body[:, :ncol] = X
        self.ctx, self.buf, self.g = ctx, ctx.to_device(host), C.c_void_p()
        ctx.check(capi.lib().sfg_geno_from_device(ctx.h, C.c_void_p(self.buf.value + off), nrow, ncol, ld, C.byref(self.g)), "geno_from_device")

    def free(self):
        self.ctx.geno_free(self.g)
        self.ctx.free(self.buf)


def views_of(ncol):
    """(ld, base offset): an odd stride, and a stride of whole 16-byte pieces on, one past and one short of a 16-byte boundary"""
    assert ncol % 2 == 0
    ld16 = (ncol + 15) // 16 * 16
    return [(ncol + 1, 0), (ld16, 0), (ld16, 1), (ld16, 15)]


def pack(ctx, g):
    from sfgwas_amd import capi
    out = C.c_void_p()
    ctx.check(capi.lib().sfg_geno_pack(ctx.h, g, C.byref(out)), "geno_pack")
    return out


# ---------------------------------------------------------------------------------------------------------------- sketch and moments
@pytest.mark.parametrize("shape", gr.SKETCH_TALL, ids=lambda s: f"{s[0]}x{s[1]}")
def test_sketch_across_chunks_strips_and_tiles(ctx, shape):
    """uniform int8 with the directed dwords, 16 buckets cycling, random signs"""
    X, bucket, sgn = gr.sketch_case(*shape)
    g = ctx.geno_upload(X)
    same(ctx.sketch(g, bucket, sgn, 16), gr.sketch(X, bucket, sgn, 16), f"sketch {shape}")
    ctx.geno_free(g)


@pytest.mark.parametrize("kp", [1, 2, 15, 16])
@pytest.mark.parametrize("mode", ["cycle", "equal"])
def test_sketch_bucket_counts_and_one_bucket_taking_every_row(ctx, kp, mode):
    nrow, ncol = 32769, 257
    X, bucket, sgn = gr.sketch_case(nrow, ncol, "int8", kp, mode)
    g = ctx.geno_upload(X)
    got = ctx.sketch(g, bucket, sgn, kp)
    assert got[0].shape == (kp, ncol)
    same(got, gr.sketch(X, bucket, sgn, kp), f"sketch kp {kp} {mode}")
    ctx.geno_free(g)


@pytest.mark.parametrize("kind", gr.VALUE_KINDS)
def test_sketch_value_ranges(ctx, kind):
    """dosages, uniform int8, and the constants 127 (signs +1), -128 (xsum wraps modulo 2^64 in every chunk), 11 (121: the largest square that does not
    wrap) and 12 (144 -> -112), with the buckets cycling and with one bucket taking every row of every chunk (the largest int32 partial sums)"""
    nrow, ncol = 65537, 257
    for mode in ("cycle", "equal"):
        X, bucket, sgn = gr.sketch_case(nrow, ncol, kind, 16, mode)
        g = ctx.geno_upload(X)
        want = gr.sketch(X, bucket, sgn, 16)
        same(ctx.sketch(g, bucket, sgn, 16), want, f"sketch of {kind}, buckets {mode}")
        ctx.geno_free(g)
    if kind == "c127":
        assert want[0][15, 0] == 127.0 * nrow
    if kind == "cm128":
        assert int(want[1][0]) == (1 << 64) - 128 * nrow and int(want[2][0]) == 0
    if kind == "c12":
        assert int(want[2][0]) == (1 << 64) - 112 * nrow


@pytest.mark.parametrize("ncol", [1, 257])
def test_sketch_moments_around_the_fast_path_threshold(ctx, ncol):
    """dosages (every dword on the fast path) with the directed dwords of genopass_ref.QUADS at genopass_ref.quad_rows: inside a tile, at its two ends, on both
    sides of a chunk boundary, and in the last, partial tile of the second chunk"""
    nrow = 16384 + 70
    X, bucket, sgn = gr.sketch_case(nrow, ncol, "dosage", 16, "cycle")
    assert gr.quad_rows(nrow)[-1] == 16448 and tuple(X[16448:16452, 0]) in gr.QUADS
    g = ctx.geno_upload(X)
    same(ctx.sketch(g, bucket, sgn, 16), gr.sketch(X, bucket, sgn, 16), f"directed dwords, {ncol} columns")
    ctx.geno_free(g)


@pytest.mark.parametrize("sentinel", SENTINELS)
def test_sketch_and_column_sums_of_views(ctx, sentinel):
    nrow, ncol = 16385 + 70, 300
    X, bucket, sgn = gr.sketch_case(nrow, ncol)
    want_sk, want_cs = gr.sketch(X, bucket, sgn, 16), gr.colsums(X)
    g = ctx.geno_upload(X)
    same(ctx.sketch(g, bucket, sgn, 16), want_sk, "contiguous sketch")
    same(ctx.geno_colsums(g), want_cs, "contiguous column sums")
    ctx.geno_free(g)
    for ld, off in views_of(ncol):
        v = View(ctx, X, ld, off, sentinel)
        same(ctx.sketch(v.g, bucket, sgn, 16), want_sk, f"sketch of a view, ld {ld}, base + {off}, sentinel {sentinel}")
        same(ctx.geno_colsums(v.g), want_cs, f"column sums of a view, ld {ld}, base + {off}, sentinel {sentinel}")
        v.free()


def test_sketch_with_each_output_left_out(ctx):
    from sfgwas_amd import capi
    nrow, ncol, kp = 16385, 257, 5
    X, bucket, sgn = gr.sketch_case(nrow, ncol, "int8", kp)
    want = gr.sketch(X, bucket, sgn, kp)
    g = ctx.geno_upload(X)
    for skip in range(3):
        out = [np.full((kp, ncol), -7.0), np.full(ncol, 99, dtype=np.uint64), np.full(ncol, 99, dtype=np.uint64)]
        ptrs = [out[0].ctypes.data_as(C.POINTER(C.c_double)), capi.p64(out[1]), capi.p64(out[2])]
        ptrs[skip] = None
        ctx.check(capi.lib().sfg_sketch(ctx.h, g, bucket.ctypes.data_as(C.POINTER(C.c_int32)), sgn.ctypes.data_as(C.POINTER(C.c_int8)), kp, *ptrs), "sketch")
        for k in range(3):
            if k != skip:
                same([out[k]], [want[k]], f"output {k} with output {skip} NULL")
    ctx.geno_free(g)


def test_sketch_refusals(ctx):
    from sfgwas_amd import capi
    nrow, ncol = 200, 20
    X, bucket, sgn = gr.sketch_case(nrow, ncol, "dosage", 4, quads=False)             # plain dosages: the packed handle below must exist
    g = ctx.geno_upload(X)
    for kp in (0, 17):
        with pytest.raises(capi.SfgError, match=r"sfg_sketch: kp must be in 1\.\.16"):
            ctx.sketch(g, np.zeros(nrow, np.int32), sgn, kp)
    for bad in (4, -1):
        b = bucket.copy()
        b[nrow - 1] = bad
        with pytest.raises(capi.SfgError, match="sfg_sketch: bucket index out of range"):
            ctx.sketch(g, b, sgn, 4)
    gp = pack(ctx, g)
    with pytest.raises(capi.SfgError, match="sfg_sketch: 2-bit packed matrix"):
        ctx.sketch(gp, bucket, sgn, 4)
    same(ctx.sketch(g, bucket, sgn, 4), gr.sketch(X, bucket, sgn, 4), "a good call after the refusals")
    ctx.geno_free(gp)
    ctx.geno_free(g)


def test_sharded_sketch_and_column_sums_at_world_2_equal_the_reference(ctx):
    """two ranks on one device, two column blocks of 8192 (the second 300 wide), two row chunks: against genopass_ref, not against the single-context call"""
    from sfgwas_amd import capi
    nrow, ncol, kp = 16385 + 70, 8192 + 300, 3
    X, bucket, sgn = gr.sketch_case(nrow, ncol, "int8", kp)
    mg = capi.MultiGpu(ol.Q_PN14, ol.P_PN14, devices=[0, 0])
    try:
        m = mg.geno_upload(X)
        same(mg.sketch(m, bucket, sgn, kp), gr.sketch(X, bucket, sgn, kp), "sharded sketch")
        same(mg.geno_colsums(m), gr.colsums(X), "sharded column sums")
        mg.geno_free(m)
    finally:
        mg.close()


# ---------------------------------------------------------------------------------------------------------------- column sums
@pytest.mark.parametrize("nrow", [4095, 4096, 4097, 8193])
@pytest.mark.parametrize("ncol", [1, 15, 16, 17, 255, 256, 257])
def test_column_sums_across_chunks_and_strips(ctx, nrow, ncol):
    for kind in ("int8", "c12"):
        X = gr.put_quads(gr.values(kind, nrow, ncol, nrow + ncol)) if kind == "int8" else gr.values(kind, nrow, ncol, 0)
        want = gr.colsums(X)
        g = ctx.geno_upload(X)
        same(ctx.geno_colsums(g), want, f"column sums {nrow} x {ncol} of {kind}")
        s_only, q_only = ctx.geno_colsums(g, sqsums=False), ctx.geno_colsums(g, sums=False)
        assert s_only[1] is None and q_only[0] is None
        same([s_only[0], q_only[1]], want, f"sums only / squares only, {nrow} x {ncol} of {kind}")
        ctx.geno_free(g)
    assert (want[1] == -112.0 * nrow).all()


def test_column_sums_at_the_workload_row_count_int8_and_packed(ctx):
    nrow, ncol = 100_000, 48
    for kind in ("int8", "c12"):
        X = gr.values(kind, nrow, ncol, 5)
        g = ctx.geno_upload(X)
        same(ctx.geno_colsums(g), gr.colsums(X), f"column sums 100000 x 48 of {kind}")
        ctx.geno_free(g)
    X = gr.values("dosage", nrow, ncol, 6)
    want = gr.colsums(X)
    g = ctx.geno_upload(X)
    gp = pack(ctx, g)
    got = ctx.geno_colsums(g)
    same(got, want, "column sums 100000 x 48 of dosages")
    same(ctx.geno_colsums(gp), got, "column sums of the packed handle")
    ctx.geno_free(gp)
    ctx.geno_free(g)


# ---------------------------------------------------------------------------------------------------------------- pack, unpack, download
def packable(nrow, ncol, seed):
    """dosages and missing entries, the missing ones spelled -1, -5 and -128"""
    return np.random.default_rng(seed).choice(np.array([-128, -5, -1, 0, 0, 1, 1, 2, 2], dtype=np.int8), (nrow, ncol))


def check_pack(ctx, g, X, what):
    """the packed image in device memory byte for byte, then unpack and download"""
    from sfgwas_amd import capi
    nrow, ncol = X.shape
    want_img, nbad = gr.pack_bytes(X)
    assert nbad == 0
    gp = pack(ctx, g)
    dev, ld, packed = capi.geno_layout(gp)
    assert packed and ld == want_img.shape[1] == 4 * ((ncol + 15) // 16)
    same([ctx.to_host(C.c_void_p(dev), (nrow, ld), np.uint8)], [want_img], f"{what}: packed image")
    want = np.where(X < 0, -1, X).astype(np.int8)
    gu = C.c_void_p()
    ctx.check(capi.lib().sfg_geno_unpack(ctx.h, gp, C.byref(gu)), "geno_unpack")
    udev, uld, upacked = capi.geno_layout(gu)
    assert not upacked and uld == ncol
    same([ctx.to_host(C.c_void_p(udev), (nrow, ncol), np.int8)], [want], f"{what}: unpacked matrix in device memory")
    same([ctx.geno_to_host(gu)], [want], f"{what}: download of the unpacked handle")
    same([ctx.geno_to_host(gp)], [want], f"{what}: download of the packed handle")
    ctx.geno_free(gu)
    ctx.geno_free(gp)


@pytest.mark.parametrize("nrow", [65534, 65535, 65536, 65605])
@pytest.mark.parametrize("ncol", [16, 50])
def test_pack_and_unpack_across_the_launch_loop(ctx, nrow, ncol):
    """65535 rows per launch: 65536 and 65605 rows take a second launch of both kernels; 16 columns unpack in the 16-byte form, 50 in the byte form"""
    X = packable(nrow, ncol, nrow + ncol)
    X[65533:, :] = np.resize(np.array([2, 1, 0, -1, 1, 2, -128], dtype=np.int8), X[65533:, :].shape)          # no row at the seam is all zero
    g = ctx.geno_upload(X)
    same([ctx.geno_to_host(g)], [X], "download of the int8 handle")
    check_pack(ctx, g, X, f"{nrow} x {ncol}")
    ctx.geno_free(g)


@pytest.mark.parametrize("ncol", [1, 15, 16, 17, 1027, 4096 + 16, 4096 + 17])
def test_pack_and_unpack_across_x_blocks(ctx, ncol):
    """1027 and 4113 columns: two and five x-blocks of the byte form; 4112: two x-blocks of the 16-byte form; 1027 / 16 and 4113 / 16 leave padding codes"""
    X = packable(130, ncol, ncol)
    g = ctx.geno_upload(X)
    check_pack(ctx, g, X, f"130 x {ncol}")
    ctx.geno_free(g)


@pytest.mark.parametrize("sentinel", SENTINELS)
def test_pack_and_download_of_a_view(ctx, sentinel):
    nrow, ncol = 130, 50
    X = packable(nrow, ncol, 9)
    v = View(ctx, X, ncol + 1, 1, sentinel)
    same([ctx.geno_to_host(v.g)], [X], "download of a view")
    check_pack(ctx, v.g, X, f"view, sentinel {sentinel}")
    v.free()


def test_pack_counts_the_values_it_cannot_hold_exactly(ctx):
    """five 3s and four 127s, on both sides of the launch seam, are counted; -128 and -5 are missing entries and are not"""
    from sfgwas_amd import capi
    nrow, ncol = 65605, 16
    X = packable(nrow, ncol, 1)
    assert (X == -128).sum() > 1000
    for k, (r, c) in enumerate([(0, 0), (0, 15), (17, 3), (65534, 7), (65535, 0), (65535, 15), (65536, 8), (65604, 15), (40000, 1)]):
        X[r, c] = 3 if k < 5 else 127
    assert gr.pack_bytes(X)[1] == 9
    g = ctx.geno_upload(X)
    with pytest.raises(capi.SfgError, match="sfg_geno_pack: 9 values above 2 do not fit"):
        pack(ctx, g)
    X[0, 0] = 2
    ctx.geno_free(g)
    g = ctx.geno_upload(X)
    with pytest.raises(capi.SfgError, match="sfg_geno_pack: 8 values above 2 do not fit"):
        pack(ctx, g)
    ctx.geno_free(g)


# ---------------------------------------------------------------------------------------------------------------- transpose and concat
def transpose(ctx, g):
    from sfgwas_amd import capi
    t = C.c_void_p()
    ctx.check(capi.lib().sfg_geno_transpose(ctx.h, g, C.byref(t)), "geno_transpose")
    return t


@pytest.mark.parametrize("shape", [(1, 1), (63, 65), (64, 64), (65, 63), (1, 5000), (5000, 1), (130, 257)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_transpose(ctx, shape):
    X = gr.values("int8", *shape, seed=shape[0])
    g = ctx.geno_upload(X)
    t = transpose(ctx, g)
    same([ctx.geno_to_host(t)], [np.ascontiguousarray(X.T)], f"transpose {shape}")
    ctx.geno_free(t)
    ctx.geno_free(g)


def test_transpose_of_a_view_and_of_a_packed_handle(ctx):
    from sfgwas_amd import capi
    X = packable(130, 258, 3)
    for sentinel in SENTINELS:
        v = View(ctx, X, 259, 1, sentinel)
        t = transpose(ctx, v.g)
        same([ctx.geno_to_host(t)], [np.ascontiguousarray(X.T)], "transpose of a view")
        ctx.geno_free(t)
        v.free()
    g = ctx.geno_upload(X)
    gp = pack(ctx, g)
    with pytest.raises(capi.SfgError, match="sfg_geno_transpose: packed matrix"):
        transpose(ctx, gp)
    ctx.geno_free(gp)
    ctx.geno_free(g)


def concat(ctx, hs):
    from sfgwas_amd import capi
    out = C.c_void_p()
    ctx.check(capi.lib().sfg_geno_concat_cols(ctx.h, (C.c_void_p * len(hs))(*[h.value for h in hs]), len(hs), C.byref(out)), "geno_concat_cols")
    return out


def test_concat_cols(ctx):
    from sfgwas_amd import capi
    nrow = 131
    parts = [gr.values("int8", nrow, w, seed=w) for w in (1, 15, 17)]
    for sentinel in SENTINELS:
        v = View(ctx, parts[1], 17, 1, sentinel)                      # 15 columns, rows 17 bytes apart, one byte off the allocation
        hs = [ctx.geno_upload(parts[0]), v.g, ctx.geno_upload(parts[2])]
        m = concat(ctx, hs)
        same([ctx.geno_to_host(m)], [np.concatenate(parts, axis=1)], f"three parts, the middle one a view, sentinel {sentinel}")
        ctx.geno_free(m)
        one = concat(ctx, [v.g])
        same([ctx.geno_to_host(one)], [parts[1]], "k = 1")
        ctx.geno_free(one)
        ctx.geno_free(hs[0]); ctx.geno_free(hs[2])
        v.free()
    a, b = ctx.geno_upload(parts[0]), ctx.geno_upload(np.ascontiguousarray(parts[2][:nrow - 1]))
    with pytest.raises(capi.SfgError, match="sfg_geno_concat_cols: part 1 has 130 rows, expected 131"):
        concat(ctx, [a, b])
    d = ctx.geno_upload(packable(nrow, 17, 2))
    dp = pack(ctx, d)
    with pytest.raises(capi.SfgError, match=r"sfg_geno_concat_cols: part 2 is packed"):
        concat(ctx, [a, d, dp])
    for h in (a, b, d, dp):
        ctx.geno_free(h)


# ---------------------------------------------------------------------------------------------------------------- .bed decode
@pytest.mark.parametrize("ns", [1, 3, 4, 5, 255, 256, 257, 1027])
@pytest.mark.parametrize("nv", [1, 63, 64, 65, 130])
def test_bed_decode_against_an_independent_decode(ctx, ns, nv):
    """random codes; the bit pairs past the last sample of every SNP are 1s (they are not samples); no filter, a row filter, both filters"""
    rnd = np.random.default_rng(ns * 1000 + nv)
    codes = rnd.integers(0, 4, (nv, ns))
    bed = gr.make_bed(codes)
    if ns % 4:
        assert bed[3 + (ns + 3) // 4 - 1] >> (2 * (ns % 4)) == (1 << (2 * (4 - ns % 4))) - 1
    rowf, colf = (rnd.random(ns) < 0.7).astype(np.uint8), (rnd.random(nv) < 0.6).astype(np.uint8)
    rowf[ns // 2] = colf[nv // 2] = 1
    for rf, cf in ((None, None), (rowf, None), (rowf, colf)):
        g = ctx.geno_from_bed(bed, ns, nv, rf, cf)
        same([ctx.geno_to_host(g)], [gr.bed_decode(bed, ns, nv, rf, cf)], f".bed {ns} samples x {nv} SNPs, filters {rf is not None}/{cf is not None}")
        ctx.geno_free(g)
