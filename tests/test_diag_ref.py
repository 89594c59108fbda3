"""The numpy statement of the generalized diagonals (tests/diag_ref.py) against a literal double loop and against the oracle's GetDiag / GetDiagBool /
rotation (matmult.go:627-672), its int8 squaring against the oracle's, the decoder the GPU test relies on against the oracle's encoder, and the
conditions the GPU test's shape list claims to meet.  CPU only."""
import ctypes as C

import numpy as np
import pytest

import diag_ref as dr
import oracle_lib as ol

SLOTS, D = dr.SLOTS, dr.D


def literal_diag(block, shift, square, dim, d):
    r, c = block.shape
    v = [0] * dim
    for j in range(dim):
        i = (shift + j) % dim
        if i < r and j < c:
            x = int(block[i, j])
            if x < 0:
                x = 0
            if square:
                x = (x * x + 128) % 256 - 128
            v[j] = x
    out = [0] * dim
    for j in range(dim):
        out[(j + d * (shift // d)) % dim] = v[j]
    return np.array(out, dtype=np.int8)


def oracle_diag(cleaned, shift, dim, d):
    """GetDiag(index = -shift) then the right rotation by d * giant, or None when GetDiagBool says the diagonal does not exist"""
    r, c = cleaned.shape
    L = ol.lib()
    have = L.orc_get_diag_bool(r, c, dim, -shift)
    dst = np.zeros(dim)
    ok = L.orc_get_diag(ol.pd(dst), ol.pi8(cleaned), c, r, c, dim, -shift)
    assert bool(ok) == bool(have)
    if not ok:
        return None
    out = np.zeros(dim)
    L.orc_rot_right(ol.pd(dst), ol.pd(out), dim, d * (shift // d))
    return out


def oracle_clean(block, square):
    b = np.where(block < 0, 0, block).astype(np.int64)
    if square:
        b = (b * b + 128) % 256 - 128
    return np.ascontiguousarray(b.astype(np.int8))


@pytest.mark.parametrize("square", [False, True])
def test_statement_against_a_literal_double_loop(square):
    rnd = np.random.default_rng(1)
    for dim, d, shapes in ((16, 4, [(16, 16), (5, 9), (1, 16), (16, 1), (8, 8), (9, 8)]), (SLOTS, D, [(130, 70), (8192, 3), (2, 8192)])):
        for r, c in shapes:
            X = dr.gen_uniform((r, c), int(rnd.integers(1 << 30)))
            shifts = list(range(dim)) if dim == 16 else [0, 1, r - 1, r % dim, 90, 91, dim - c, (dim - c + 1) % dim, dim - 1]
            got = dr.diags(X, shifts, square, dim, d)
            for k, sh in enumerate(shifts):
                assert np.array_equal(got[k], literal_diag(X, sh, square, dim, d)), (dim, r, c, sh)
                assert np.array_equal(got[k], dr.diag(X, sh, square, dim, d))


def test_exists_and_runs_agree():
    for dim in (16, SLOTS):
        shapes = [(r, c) for r in range(1, 17) for c in range(1, 17)] if dim == 16 else [(cs.r, cs.c) for cs in dr.CASES]
        for r, c in shapes:
            in_runs = np.zeros(dim, dtype=bool)
            for lo, hi in dr.runs(r, c, dim):
                assert 0 <= lo < hi <= dim
                in_runs[lo:hi] = True
            assert [dr.exists(r, c, s, dim) for s in range(dim)] == in_runs.tolist(), (dim, r, c)


def test_statement_against_the_oracle_exhaustively_at_dim_16():
    rnd = np.random.default_rng(2)
    dim, d = 16, 4
    for r in range(1, dim + 1):
        for c in range(1, dim + 1):
            X = dr.gen_uniform((r, c), int(rnd.integers(1 << 30)))
            X[X == 0] = 3                                            # an existing diagonal is then told from a missing one by its values
            for square in (False, True):
                cl = oracle_clean(X, square)
                got = dr.diags(X, range(dim), square, dim, d)
                for sh in range(dim):
                    want = oracle_diag(cl, sh, dim, d)
                    assert (want is not None) == dr.exists(r, c, sh, dim), (r, c, sh)
                    if want is None:
                        assert not got[sh].any(), f"{r} x {c}: the statement has values on the missing diagonal {sh}"
                    else:
                        assert np.array_equal(got[sh].astype(np.float64), want), (r, c, sh, square)


@pytest.mark.parametrize("cs", dr.CASES, ids=[cs.id for cs in dr.CASES])
def test_statement_against_the_oracle_on_the_gpu_shapes(cs):
    X = np.ascontiguousarray(dr.logical(cs))
    shifts = dr.boundary_shifts(cs)
    for square in (False, True):
        cl = oracle_clean(X, square)
        got = dr.diags(X, shifts, square)
        for k, sh in enumerate(shifts):
            want = oracle_diag(cl, sh, SLOTS, D)
            assert (want is not None) == dr.exists(cs.r, cs.c, sh), sh
            if want is None:
                assert not got[k].any(), sh
            else:
                assert np.array_equal(got[k].astype(np.float64), want), (sh, square)


def test_int8_squaring_against_the_oracle_on_all_256_values():
    x = np.arange(-128, 128).astype(np.int8).reshape(1, 256)
    sk = np.zeros(256)
    xs, x2 = np.zeros(256, dtype=np.uint64), np.zeros(256, dtype=np.uint64)
    ol.lib().orc_sketch(ol.pi8(x), 1, 256, np.zeros(1, dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int32)), ol.pi8(np.ones(1, dtype=np.int8)), 1,
                        ol.pd(sk), ol.p64(xs), ol.p64(x2))
    want = x2.view(np.int64)                                         # (u64)(int64_t)(int8_t)(x * x): sign-extended
    assert np.array_equal(dr.square8(x[0]).astype(np.int64), want)
    assert dr.square8(np.int8(12)) == -112 and dr.square8(np.int8(11)) == 121 and dr.square8(np.int8(127)) == 1 and dr.square8(np.int8(-128)) == 0
    # and in the statement, after missing -> 0
    assert np.array_equal(dr.clean(x[0], True).astype(np.int64), np.where(x[0] < 0, 0, want))


def test_generators():
    u = dr.gen_uniform((512, 512), 3)
    assert len(np.unique(u)) == 256 and 0.2 < (u < 0).mean() < 0.3
    g = dr.gen_genotype((64, 64), 3)
    assert set(np.unique(g).tolist()) == {-1, 0, 1, 2}
    s = dr.gen_signs((16, 64), 3)
    assert (s != 0).all()
    for row in s:
        pats = {int(sum(1 << k for k in range(4) if row[4 * q + k] < 0)) for q in range(16)}
        assert pats == set(range(16))
    for name, v in (("c127", 127), ("cm128", -128), ("c11", 11), ("c12", 12)):
        assert (dr.GENERATORS[name]((3, 5), 0) == v).all()


@pytest.fixture(scope="module")
def ring():
    return ol.Ring(14, ol.Q_PN14, ol.P_PN14)


def test_decode_rows_inverts_the_oracle_encoder_within_the_derived_bound(ring):
    """encode_ntt -> intt -> decode_rows returns the int8 slot vector exactly; the residual stays under N * (1/2) / 2^34 = 2^-21 (asserted: < 2^-20), the
    imaginary parts too: the tolerance of the GPU test is met by the reference alone"""
    assert ol.Q_PN14[0] == dr.Q0
    rnd = np.random.default_rng(4)
    alt = np.where(np.arange(SLOTS) % 2 == 0, 127, -128)
    vecs = np.stack([np.full(SLOTS, 127), np.full(SLOTS, -128), alt, rnd.integers(-128, 128, SLOTS), rnd.integers(-1, 3, SLOTS)]).astype(np.int8)
    words = np.stack([ring.intt(0, ring.encode_ntt(v.astype(np.float64), 2.0 ** 34, 1, prec=1)[0]) for v in vecs])
    ints, resid = dr.decode_rows(words)
    assert np.array_equal(ints, vecs.astype(np.int64))
    V = dr.slot_values(words)
    print(f"residual {resid:.3g}, imaginary parts {np.abs(V.imag).max():.3g}")
    assert resid < dr.RESIDUAL_BOUND
    assert np.abs(V.imag).max() < 2.0 ** -20
    # a single changed coefficient is seen: the rounded slots move or the residual leaves the bound
    bad = words.copy()
    bad[3, 77] = (int(bad[3, 77]) + (1 << 21)) % dr.Q0
    ints2, resid2 = dr.decode_rows(bad)
    assert not np.array_equal(ints2, ints) or resid2 >= dr.RESIDUAL_BOUND


def test_the_shape_list_reaches_what_it_claims():
    paths = set()
    for cs in dr.CASES:
        w = cs.r if cs.tr else cs.c
        assert cs.ld >= w and (cs.sentinel or (cs.ld == w and cs.off == 0))
        chk = dr.checked_shifts(cs)
        assert len(chk) == len(set(chk)) and (cs.every or len(chk) <= 1024)
        edges = {s for s in (cs.r - 1, cs.r, SLOTS - cs.c, SLOTS - cs.c + 1, SLOTS - 1) if s < SLOTS}
        assert edges | {0} <= set(chk) and edges <= set(dr.boundary_shifts(cs))
        gap = dr.missing(cs)
        if gap:
            have = [dr.exists(cs.r, cs.c, s) for s in chk]
            assert any(have) and not all(have), f"{cs.id}: the checked shifts do not see both sides of the gap"
            assert gap[0] in chk and gap[1] - 1 in chk and gap[0] - 1 in chk and (gap[1] == SLOTS or gap[1] in chk)
        paths |= dr.load_paths(cs)
    assert paths == {"b16", "b4", "bytes"}
    for name in ("b16", "b4", "bytes"):
        for tr in (False, True):
            assert any(name in dr.load_paths(cs) for cs in dr.CASES if cs.tr == tr), f"no {'transposed' if tr else 'stored'} case takes the {name} path"
    assert {cs.c % 16 for cs in dr.CASES if not cs.tr} >= set(range(1, 16)), "a residue of c mod 16 is missing among the stored cases"
    assert {(cs.r, cs.c) for cs in dr.CASES if dr.missing(cs) and dr.missing(cs)[1] - dr.missing(cs)[0] == 1} >= {(4096, 4096), (8191, 1)}
    assert {cs.tr for cs in dr.CASES if cs.gen == "signs" and min(cs.r, cs.c) >= 100} == {False, True}, "the sign-pattern matrix must occur in both orientations"
    assert {cs.gen for cs in dr.EDGE_CASES} == set(dr.ROTATION)
    assert sorted(cs.off for cs in dr.EDGE_CASES if cs.sentinel) == [1, 2, 4, 8]
    assert len({cs.id for cs in dr.CASES}) == len(dr.CASES)
