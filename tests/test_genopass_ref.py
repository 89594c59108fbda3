"""tests/genopass_ref.py against literal Python loops on tiny shapes (every value at which Go's int8 arithmetic does something a plain sum would not:
-128, -1, 11, 12, 16, 127; an xsum that wraps past 2^64), and its sketch against the oracle's C loop at the tall shapes of tests/test_gpu_genopasses.py.
The GPU module then rests on two independent statements that agree."""
import ctypes as C

import numpy as np
import pytest

import genopass_ref as gr
import oracle_lib as ol

M64 = (1 << 64) - 1
EDGE = [-128, -1, 0, 1, 2, 3, 11, 12, 16, 127]


def i8(x):
    """Go's int8(x) of an integer: the low byte, two's complement"""
    x &= 0xFF
    return x - 256 if x >= 128 else x


def tiny(nrow, ncol, seed):
    rnd = np.random.default_rng(seed)
    X = rnd.integers(-128, 128, (nrow, ncol), dtype=np.int8)
    X.ravel()[:min(X.size, len(EDGE))] = EDGE[:X.size]
    return X


def loop_sketch(X, bucket, sgn, kp):
    nrow, ncol = X.shape
    sk = [[0] * ncol for _ in range(kp)]
    xs, x2 = [0] * ncol, [0] * ncol
    for i in range(nrow):
        for j in range(ncol):
            x = int(X[i, j])
            sk[int(bucket[i])][j] += int(sgn[i]) * x
            xs[j] = (xs[j] + (x & M64)) & M64                         # uint64(int8): sign extension
            x2[j] = (x2[j] + (i8(x * x) & M64)) & M64                 # uint64(int8(x * x))
    return sk, xs, x2


@pytest.mark.parametrize("nrow,ncol,kp", [(1, 1, 1), (10, 1, 2), (7, 5, 3), (33, 4, 16), (20, 3, 15)])
def test_sketch_equals_the_literal_loops(nrow, ncol, kp):
    X = tiny(nrow, ncol, nrow)
    rnd = np.random.default_rng(ncol)
    bucket, sgn = rnd.integers(0, kp, nrow).astype(np.int32), rnd.choice(np.array([-1, 1, -128, 127], dtype=np.int8), nrow)
    sk, xs, x2 = gr.sketch(X, bucket, sgn, kp)
    lsk, lxs, lx2 = loop_sketch(X, bucket, sgn, kp)
    assert sk.dtype == np.float64 and xs.dtype == np.uint64 and x2.dtype == np.uint64
    assert [[int(v) for v in row] for row in sk] == lsk and [int(v) for v in xs] == lxs and [int(v) for v in x2] == lx2


def test_the_edge_values_one_by_one():
    for x, sq in ((-128, 0), (-1, 1), (11, 121), (12, -112), (16, 0), (127, 1)):
        assert i8(x * x) == sq
        X = np.array([[x]], dtype=np.int8)
        sk, xs, x2 = gr.sketch(X, np.zeros(1, np.int32), np.array([-1], np.int8), 1)
        assert sk[0, 0] == -x and int(xs[0]) == x & M64 and int(x2[0]) == sq & M64
        s, q = gr.colsums(X)
        assert s[0] == max(x, 0) and q[0] == (sq if x > 0 else 0)


def test_xsum_wraps_past_two_to_the_64():
    """three rows of -1 are 3 (2^64 - 1) = 2 * 2^64 + (2^64 - 3): the sum has wrapped twice; 40 000 rows of -128 wrap 39 999 times"""
    X = np.full((3, 1), -1, dtype=np.int8)
    _, xs, x2 = gr.sketch(X, np.zeros(3, np.int32), np.ones(3, np.int8), 1)
    assert 3 * M64 > M64 and int(xs[0]) == (3 * M64) & M64 == M64 - 2 and int(x2[0]) == 3
    X = np.full((40_000, 2), -128, dtype=np.int8)
    _, xs, x2 = gr.sketch(X, np.zeros(40_000, np.int32), np.ones(40_000, np.int8), 1)
    assert int(xs[0]) == (40_000 * ((-128) & M64)) & M64 == (1 << 64) - 128 * 40_000 and int(x2[1]) == 0


@pytest.mark.parametrize("nrow,ncol", [(1, 1), (9, 3), (40, 2)])
def test_colsums_equal_the_literal_loops(nrow, ncol):
    X = tiny(nrow, ncol, 50 + nrow)
    s, q = gr.colsums(X)
    for j in range(ncol):
        g = [max(int(v), 0) for v in X[:, j]]
        assert s[j] == float(sum(g)) and q[j] == float(sum(i8(v * v) for v in g))
    s, q = gr.colsums(np.full((nrow, ncol), 12, dtype=np.int8))     # 144 -> -112: the sum of squares goes below zero
    assert (s == 12.0 * nrow).all() and (q == -112.0 * nrow).all()


@pytest.mark.parametrize("nrow,ncol", [(1, 1), (2, 15), (3, 16), (2, 17), (2, 33), (1, 64)])
def test_pack_bytes_equal_the_literal_loops(nrow, ncol):
    rnd = np.random.default_rng(ncol)
    X = rnd.choice(np.array([-128, -7, -1, 0, 1, 2, 3, 127], dtype=np.int8), (nrow, ncol))
    img, nbad = gr.pack_bytes(X)
    ldw = (ncol + 15) // 16
    assert img.dtype == np.uint8 and img.shape == (nrow, 4 * ldw)
    bad = 0
    for i in range(nrow):
        for w in range(ldw):
            v = 0
            for k in range(16):
                c = 16 * w + k
                g = int(X[i, c]) if c < ncol else 0
                bad += g > 2
                v |= (3 if g < 0 else g & 3) << (2 * k)
            assert [int(b) for b in img[i, 4 * w:4 * w + 4]] == [(v >> (8 * b)) & 0xFF for b in range(4)]   # a little-endian dword
    assert nbad == bad


@pytest.mark.parametrize("ns,nv", [(1, 1), (3, 2), (4, 3), (5, 1), (9, 4)])
@pytest.mark.parametrize("filt", ["none", "rows", "both"])
def test_bed_decode_equals_the_literal_loops(ns, nv, filt):
    rnd = np.random.default_rng(ns * 10 + nv)
    codes = rnd.integers(0, 4, (nv, ns))
    bps = (ns + 3) // 4
    raw = [0x6C, 0x1B, 0x01]
    for j in range(nv):
        for b in range(bps):
            byte = 0
            for k in range(4):
                byte |= (int(codes[j, 4 * b + k]) if 4 * b + k < ns else 3) << (2 * k)
            raw.append(byte)
    bed = np.array(raw, dtype=np.uint8)
    assert np.array_equal(gr.make_bed(codes), bed)
    rowf = (np.arange(ns) % 3 != 1).astype(np.uint8) if filt != "none" and ns > 1 else None
    colf = (np.arange(nv) % 2 == 0).astype(np.uint8) if filt == "both" else None
    want = [[{0: 2, 1: -1, 2: 1, 3: 0}[int(codes[j, i])] for j in range(nv) if colf is None or colf[j]] for i in range(ns) if rowf is None or rowf[i]]
    got = gr.bed_decode(bed, ns, nv, rowf, colf)
    assert got.dtype == np.int8 and got.flags.c_contiguous and got.tolist() == want


def test_the_directed_dwords_sit_where_the_docstring_says():
    X = gr.put_quads(np.zeros((16384 + 70, 257), dtype=np.int8))
    rows = gr.quad_rows(X.shape[0])
    assert rows == [4, 60, 64, 16380, 16384, 16448] and all(r % 4 == 0 for r in rows)
    for r in rows:
        for k, q in enumerate(gr.QUADS):
            assert tuple(X[r:r + 4, k]) == q and tuple(X[r:r + 4, 256 - k]) == q
    sums = [sum(i8(v * v) for v in q) for q in gr.QUADS]
    assert sum(v * v for v in gr.QUADS[0]) == 127 and sum(v * v for v in gr.QUADS[1]) == 128 and sums[2] == -112
    one = gr.put_quads(np.zeros((16384 + 70, 1), dtype=np.int8))
    assert [tuple(one[r:r + 4, 0]) for r in rows[:4]] == list(gr.QUADS)


@pytest.mark.parametrize("shape", gr.SKETCH_TALL, ids=lambda s: f"{s[0]}x{s[1]}")
def test_sketch_equals_the_oracle_at_the_tall_shapes(shape):
    nrow, ncol = shape
    X, bucket, sgn = gr.sketch_case(nrow, ncol)
    kp = 16
    wsk, wxs, wx2 = np.zeros((kp, ncol)), np.zeros(ncol, dtype=np.uint64), np.zeros(ncol, dtype=np.uint64)
    ol.lib().orc_sketch(ol.pi8(X), nrow, ncol, bucket.ctypes.data_as(C.POINTER(C.c_int32)), ol.pi8(sgn), kp, ol.pd(wsk), ol.p64(wxs), ol.p64(wx2))
    sk, xs, x2 = gr.sketch(X, bucket, sgn, kp)
    assert np.array_equal(sk, wsk) and np.array_equal(xs, wxs) and np.array_equal(x2, wx2)


@pytest.mark.parametrize("kind", gr.VALUE_KINDS)
def test_sketch_equals_the_oracle_for_every_kind_of_value(kind):
    nrow, ncol, kp = 65537, 3, 2
    X, bucket, sgn = gr.sketch_case(nrow, ncol, kind, kp, "equal")
    wsk, wxs, wx2 = np.zeros((kp, ncol)), np.zeros(ncol, dtype=np.uint64), np.zeros(ncol, dtype=np.uint64)
    ol.lib().orc_sketch(ol.pi8(X), nrow, ncol, bucket.ctypes.data_as(C.POINTER(C.c_int32)), ol.pi8(sgn), kp, ol.pd(wsk), ol.p64(wxs), ol.p64(wx2))
    sk, xs, x2 = gr.sketch(X, bucket, sgn, kp)
    assert np.array_equal(sk, wsk) and np.array_equal(xs, wxs) and np.array_equal(x2, wx2)
    if kind == "cm128":
        assert int(xs[0]) == (1 << 64) - 128 * nrow                  # wrapped 65 536 times
    if kind == "c12":
        assert int(x2[0]) == (-112 * nrow) & M64
