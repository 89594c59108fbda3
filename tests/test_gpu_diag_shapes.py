"""Diagonal extraction (k_skew, csrc/encode.hip) at every shift, and the shift plan of a product (encode_block, csrc/matmul.hip) at its edges.

(a) sfg_encode_diags_dev at L = 1 -> sfg_intt_rows -> tests/diag_ref.decode_rows must give the numpy statement's diagonal (tests/diag_ref.diags) on every
    slot, as integers, with a residual below the derived 2^-20; a shift that does not exist must encode to all-zero words.  The block pointer and its
    stride are the test's own: odd strides, misaligned bases, views inside buffers filled with the sentinel 0x55.
(b) the encoder's words at L = 2 against the oracle's exactly rounded encode of the statement's diagonal, at the shifts next to the plan's edges.
(c) whole products against the oracle at the shapes where the plan changes: nr + nc = 8192 and 8193, single rows and columns, a full and a gapped block
    row in one panel followed by a ragged product on the same context (stale plaintext slots), SFG_SQUARE on arbitrary int8, packed handles.

Every comparison is exact; the residual of (a) is the only tolerance (tests/test_diag_ref.py shows that the reference alone meets it)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import diag_ref as dr
import oracle_lib as ol

pytestmark = pytest.mark.gpu
SLOTS, D, N = dr.SLOTS, dr.D, dr.N
SCALE = 2.0 ** 34
CHUNK = 1024                            # shifts per encode call and download


# ------------------------------------------------------------------------------------------------ (a), (b): extraction
class Blocks:
    """one context; the uploaded buffer of every case, made on first use"""

    def __init__(self):
        from sfgwas_amd import capi
        self.capi, self.lib = capi, capi.lib()
        self.ctx = capi.Context(ol.Q_PN14, ol.P_PN14)
        self.ring = ol.Ring(14, ol.Q_PN14, ol.P_PN14)
        self.dev = {}

    def block(self, cs):
        if cs.id not in self.dev:
            self.dev[cs.id] = self.ctx.to_device(dr.buffer(cs))
        return C.c_void_p(self.dev[cs.id].value + cs.off)

    def encode(self, cs, shift0, nshift, L, to_coefficients=False):
        """sfg_encode_diags_dev on the case's view -> [nshift][L][N] words (L = 1 and to_coefficients: after the device inverse NTT at q0)"""
        ctx = self.ctx
        d_pt = ctx.malloc(nshift * L * N * 8)
        try:
            ctx.check(self.lib.sfg_encode_diags_dev(ctx.h, self.block(cs), cs.ld, cs.r, cs.c, int(cs.tr), shift0, nshift, L, d_pt), "sfg_encode_diags_dev")
            if to_coefficients:
                assert L == 1
                ctx.check(self.lib.sfg_intt_rows(ctx.h, d_pt, nshift, (C.c_int * nshift)(*([0] * nshift))), "sfg_intt_rows")
            return ctx.to_host(d_pt, (nshift, L, N), np.uint64)
        finally:
            ctx.free(d_pt)

    def close(self):
        for p in self.dev.values():
            self.ctx.free(p)
        self.ctx.close()


@pytest.fixture(scope="module")
def blocks():
    b = Blocks()
    yield b
    b.close()


def check_decoded(blocks, cs, shift0, nshift):
    words = blocks.encode(cs, shift0, nshift, 1, to_coefficients=True)[:, 0, :]
    shifts = np.arange(shift0, shift0 + nshift)
    want = dr.diags(dr.logical(cs), shifts)
    there = np.array([dr.exists(cs.r, cs.c, int(s)) for s in shifts])
    if not there.all():
        bad = shifts[~there][words[~there].any(axis=1)]
        assert bad.size == 0, f"{cs.id}: shifts {bad[:8]} do not exist but encode to non-zero words"
        assert not want[~there].any()
    got, resid = dr.decode_rows(words)
    print(f"{cs.id} shifts [{shift0}, {shift0 + nshift}): residual {resid:.3g}")
    if not np.array_equal(got, want):
        k, p = np.argwhere(got != want)[0]
        n_bad = np.count_nonzero((got != want).any(axis=1))
        leak = " (85 = the sentinel: a read outside the view)" if cs.sentinel and got[k, p] == dr.SENTINEL else ""
        raise AssertionError(f"{cs.id}: {n_bad} of {nshift} diagonals differ; first at shift {shifts[k]}, slot {p}: decoded {got[k, p]}, statement {want[k, p]}{leak}")
    assert resid < dr.RESIDUAL_BOUND, f"{cs.id}: residual {resid} at shifts [{shift0}, {shift0 + nshift})"


EVERY = [cs for cs in dr.CASES if cs.every]


@pytest.mark.parametrize("shift0", range(0, SLOTS, CHUNK))
@pytest.mark.parametrize("cs", EVERY, ids=[cs.id for cs in EVERY])
def test_every_shift_decodes_to_the_statement(blocks, cs, shift0):
    check_decoded(blocks, cs, shift0, CHUNK)


@pytest.mark.parametrize("cs", dr.EDGE_CASES, ids=[cs.id for cs in dr.EDGE_CASES])
def test_edge_tiles_decode_to_the_statement(blocks, cs):
    """whole 128-shift tiles: those of shifts 0, r - 1, r, 8192 - c, 8192 - c + 1, 8191, the middle of each run and of the gap"""
    tiles = dr.tiles(cs)
    assert 128 * len(tiles) <= CHUNK
    for t in tiles:
        check_decoded(blocks, cs, t * dr.TILE, dr.TILE)


@pytest.mark.parametrize("cs", dr.EDGE_CASES, ids=[cs.id for cs in dr.EDGE_CASES])
def test_encoder_words_at_the_boundary_shifts(blocks, cs):
    """L = 2, word for word against the oracle's encode of the statement's diagonal (its exact rounding, its NTT)"""
    X = dr.logical(cs)
    shifts = dr.boundary_shifts(cs)
    want_diag = dr.diags(X, shifts)
    for k, sh in enumerate(shifts):
        got = blocks.encode(cs, sh, 1, 2)[0]
        if not dr.exists(cs.r, cs.c, sh):
            assert not got.any(), f"{cs.id}: the non-existent diagonal {sh} must encode to zero"
            assert not want_diag[k].any()
        else:
            want = blocks.ring.encode_ntt(want_diag[k].astype(np.float64), SCALE, 2, prec=1)
            assert np.array_equal(got, want), f"{cs.id}: shift {sh}"


# ------------------------------------------------------------------------------------------------ (c): whole products
IN_LEVEL, MAX_LEVEL, KEY_SEED = 2, 2, 1000


def all_keys(ring):
    from sfgwas_amd import capi
    from sfgwas_amd.params import rotations_for_matmul
    return {ring.galois(k): capi.random_rotkey(ring.moduli, ring.beta, ring.N, KEY_SEED + k) for k in rotations_for_matmul()}


class Products:
    """a context and the oracle ring with the same uniform random rotation keys, every baby and giant step; oracle results are computed once per matrix"""

    def __init__(self):
        from sfgwas_amd import capi
        self.capi = capi
        self.ring = ol.Ring(14, ol.Q_PN14, ol.P_PN14)
        self.keys = ol.RotKeys(self.ring)
        self.keymap = all_keys(self.ring)
        for g, key in self.keymap.items():
            self.keys.add(g, key)
        self.ctx = self.fresh_ctx()
        self.wants = {}

    def fresh_ctx(self):
        ctx = self.capi.Context(ol.Q_PN14, ol.P_PN14)
        for g, key in self.keymap.items():
            ctx.load_rotkey(g, key)
        return ctx

    def cts(self, nbr, seed):
        return np.stack([np.stack([self.ring.fill_uniform(IN_LEVEL, seed * 100 + b) for b in range(nbr)])])          # s = 1

    def want(self, name, logical, square=False):
        """(A, oracle words, oracle column sums, oracle column sums of squares) of the logical matrix, once"""
        key = (name, square)
        if key not in self.wants:
            A = self.cts((logical.shape[0] - 1) // SLOTS + 1, 7 + len(self.wants))
            out, sm, sq = ol.matmult4stream(self.ring, self.keys, SCALE, A, IN_LEVEL, MAX_LEVEL, np.ascontiguousarray(logical),
                                            compute_sqsum=True, square=square, enc_prec=1)
            assert out.any() or not dr.clean(logical).any()
            self.wants[key] = (A, out, sm, sq)
        return self.wants[key]

    def check(self, name, logical, transposed, square=False, ctx=None):
        A, want, wsm, wsq = self.want(name, logical, square)
        stored = np.ascontiguousarray(logical.T) if transposed else np.ascontiguousarray(logical)
        flags = (self.capi.SFG_TRANSPOSE if transposed else 0) | (self.capi.SFG_SQUARE if square else 0)
        got, sm, sq = (ctx or self.ctx).matmul_stream(A, IN_LEVEL, MAX_LEVEL, stored, flags=flags, want_sums=True)
        assert got.shape == want.shape
        assert np.array_equal(got, want), f"{name}: {np.count_nonzero(got != want)} ciphertext words differ, first at {np.argwhere(got != want)[0]}"
        if not transposed:
            assert np.array_equal(sm, wsm) and np.array_equal(sq, wsq)

    def close(self):
        self.ctx.close()


@pytest.fixture(scope="module")
def prod():
    p = Products()
    yield p
    p.close()


# the plan's edges as logical r x c: nr + nc = 8192 (one shift missing), 8193 (none), one column, one row, 8191 x 1 (only shift 8191 missing)
PLAN_EDGES = {"4096x4096": ("genotype", 4096, 4096), "4096x4097": ("uniform", 4096, 4097), "8192x1": ("genotype", 8192, 1),
              "1x8192": ("uniform", 1, 8192), "8191x1": ("genotype", 8191, 1)}


def plan_edge_matrix(name):
    gen, r, c = PLAN_EDGES[name]
    return dr.GENERATORS[gen]((r, c), 500 + r + c)


@pytest.mark.parametrize("transposed", [False, True], ids=["plain", "transpose"])
@pytest.mark.parametrize("name", list(PLAN_EDGES))
def test_product_at_the_plan_edges(prod, name, transposed):
    prod.check(name, plan_edge_matrix(name), transposed)


BIG, SMALL = (SLOTS + 4096, 4096), (60, 40)


def seq_matrices():
    return dr.gen_genotype(BIG, 77), dr.gen_genotype(SMALL, 78)


def run_sequence(prod, ctx, order):
    big, small = seq_matrices()
    for which in order:
        prod.check(which, big if which == "big" else small, False, ctx=ctx)


@pytest.mark.parametrize("order", [("big", "small"), ("small", "big")], ids=["full+gapped then ragged", "ragged then full+gapped"])
def test_full_and_gapped_block_rows_in_one_panel_then_a_ragged_product(prod, order):
    """(8192 + 4096) x 4096: a full block row (only the 89 slots past shift 8191 are zeroed) and a gapped one (every slot zeroed, 8191 written) share
    a panel; the 60 x 40 product straight after it on the same context writes 99 of the 8281 slots and must find the others zero.  Both orders, each on a
    fresh context, both against the oracle."""
    ctx = prod.fresh_ctx()
    try:
        run_sequence(prod, ctx, order)
    finally:
        ctx.close()


_CHILD_SEQ = r"""
import sys, numpy as np
sys.path.insert(0, 'tests'); sys.path.insert(0, '.')
import oracle_lib as ol
from sfgwas_amd import capi
from sfgwas_amd.params import rotations_for_matmul
d = np.load(sys.argv[1])
keys = None
out = {}
for order in (("big", "small"), ("small", "big")):
    ctx = capi.Context(ol.Q_PN14, ol.P_PN14)
    if keys is None:
        mods = list(ol.Q_PN14) + list(ol.P_PN14)
        keys = {ctx.galois(k): capi.random_rotkey(mods, ctx.beta, ctx.N, int(d["key_seed"]) + k) for k in rotations_for_matmul()}
    for g, key in keys.items():
        ctx.load_rotkey(g, key)
    for which in order:
        got, _, _ = ctx.matmul_stream(d["A_" + which], int(d["in_level"]), int(d["max_level"]), d["geno_" + which])
        out[which + "_in_" + "_".join(order)] = got
    ctx.close()
np.savez(sys.argv[2], **out)
"""


def test_the_same_sequences_without_the_riding_transposition(prod, tmp_path):
    """SFG_PT_RIDE=0 (the transposition pass before every MAC launch, the switch tests/test_gpu_properties.py uses for it; it exists in the
    experimenters' build, which a child process loads): both orders of the sequence above, every word against the same oracle results"""
    big, small = seq_matrices()
    A_big, want_big = prod.want("big", big)[:2]
    A_small, want_small = prod.want("small", small)[:2]
    fin, fout = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(fin, A_big=A_big, A_small=A_small, geno_big=big, geno_small=small, in_level=IN_LEVEL, max_level=MAX_LEVEL, key_seed=KEY_SEED)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    e = dict(os.environ)
    e.update(prod.capi.env_for({"SFG_PT_RIDE": "0"}))
    assert e.get("SFG_LIB_PATH") == prod.capi.AB_LIB_PATH
    r = subprocess.run([sys.executable, "-c", _CHILD_SEQ, fin, fout], cwd=root, env=e, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    got = np.load(fout)
    for order in ("big_small", "small_big"):
        assert np.array_equal(got["big_in_" + order], want_big), f"order {order}: the full + gapped product differs from the oracle"
        assert np.array_equal(got["small_in_" + order], want_small), f"order {order}: the ragged product differs from the oracle"


@pytest.mark.parametrize("transposed", [False, True], ids=["plain", "transpose"])
@pytest.mark.parametrize("gen", ["uniform", "c11", "c12", "c127", "cm128"])
def test_square_on_arbitrary_int8(prod, gen, transposed):
    """SFG_SQUARE squares in int8 arithmetic after missing -> 0: 11 -> 121, 12 -> -112, 127 -> 1, -128 -> 0"""
    prod.check("sq70x50-" + gen, dr.GENERATORS[gen]((70, 50), 900), transposed, square=True)


def test_square_on_two_block_columns_of_uniform_int8(prod):
    prod.check("sq30x8217", dr.gen_uniform((30, SLOTS + 25), 901), False, square=True)


@pytest.mark.parametrize("name", [n for n, (gen, _, _) in PLAN_EDGES.items() if gen == "genotype"] + ["big", "small"])
def test_packed_handle_gives_the_int8_handle_words(prod, name):
    """the genotype-valued matrices above as resident handles, int8 and 2-bit packed, X and X^T: the same words (and the oracle's, since they are at hand)"""
    capi, ctx = prod.capi, prod.ctx
    logical = {"big": seq_matrices()[0], "small": seq_matrices()[1]}.get(name)
    if logical is None:
        logical = plan_edge_matrix(name)
    A, want = prod.want(name, logical)[:2]
    dA = capi.DevArray.from_host(ctx, A)
    for flags, stored in ((0, logical), (capi.SFG_TRANSPOSE, np.ascontiguousarray(logical.T))):
        g = ctx.geno_upload(stored)
        gp = C.c_void_p()
        ctx.check(capi.lib().sfg_geno_pack(ctx.h, g, C.byref(gp)), "pack")
        a = ctx.matmul_resident(dA, 1, IN_LEVEL, MAX_LEVEL, g, flags)
        b = ctx.matmul_resident(dA, 1, IN_LEVEL, MAX_LEVEL, gp, flags)
        ha, hb = a.host(), b.host()
        a.free(); b.free()
        ctx.geno_free(g); ctx.geno_free(gp)
        assert np.array_equal(ha, hb), f"{name}, flags {flags}: packed and int8 handles disagree"
        assert np.array_equal(ha, want), f"{name}, flags {flags}: the resident product differs from the oracle"
    dA.free()
