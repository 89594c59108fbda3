"""The int8 MAC's plaintext transposition in the PRODUCT library - the pass k_i8_pack_pt_digits, the mover k_i8_move_pt alone, and the mover riding in front of
plaintext-NTT launches (k_ntt_half3_move) - against tests/i8tile_ref.py, a numpy statement of the tile buffers that is not the pass.  Reached through the test hook
sfg_i8_move_for_test, which prepares, deals and launches exactly as matmul.hip / encode.hip do (i8_ride_prepare, i8_ride_take, launch_move_alone,
launch_ntt_plain_half, i8_ride_finish).

The panel is random bytes (the transposition is a byte permutation: the bytes need not be digits of canonical words); the tile buffers and a guard band behind each
are filled with a sentinel first, so a skipped item, a byte outside the slice or past the buffer shows.  Every assertion is np.array_equal; there is no tolerance.
A failing comparison names the first differing byte's (item, unit, row, column) through i8tile_ref.locate.

(tests/test_gpu_mover.py keeps the A/B-only depths and the non-streaming form of the mover against the pass.)"""
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

import i8tile_ref as R
import ksw_ref
import oracle_lib as ol
from test_i8tile_ref import DIRECTED_SHAPES

pytestmark = pytest.mark.gpu
H = 8192
SENT = 0xA5


def _q47():
    return ol.small_primes(14, 47, 1)[0]          # the first prime below 2^47: above SFG_I8_BIG_QMAX (tests/test_gpu_mac.py builds the same chain)


CHAINS = {"pn14": lambda: (list(ol.Q_PN14), list(ol.P_PN14)), "s1": lambda: (list(ksw_ref.S1[0]), list(ksw_ref.S1[1])),
          "q47": lambda: ([_q47()] + list(ol.Q_PN14[1:3]), list(ol.P_PN14))}


class Env:
    def __init__(self):
        self.ctx, self.panels, self.nomover = {}, {}, {}

    def context(self, chain):
        if chain not in self.ctx:
            from sfgwas_amd import capi
            q, p = CHAINS[chain]()
            self.ctx[chain] = capi.Context(q, p)
        return self.ctx[chain]

    def nd(self, chain, L):
        return [5 if q < (1 << 36) else 6 for q in self.context(chain).q[:L]]

    def panel(self, chain, L, K, Ncols, layout):
        """(placed panel bytes, pt_k, pt_n, reference small tiles, reference big tiles or None), computed once and never written"""
        key = (chain, L, K, Ncols, layout)
        if key not in self.panels:
            self.panels.clear()                                  # (one shape at a time: the cases of a shape are adjacent)
            nd = self.nd(chain, L)
            rnd = np.random.default_rng(zlib.crc32(repr(key).encode()))
            P = rnd.integers(0, 256, (K, Ncols, sum(nd), H), dtype=np.uint8)
            P[P == SENT] = SENT ^ 0xFF                           # no panel byte equals the sentinel (nor zero below): a byte left in place cannot pass for a moved one
            P[P == 0] = 1
            buf, pt_k, pt_n = R.PLACE[layout](P, nd, rnd)
            big_first = nd[0] == 6
            assert nd.count(6) <= 1 and (6 not in nd or big_first)
            p0 = 6 if big_first else 0
            ns = nd.count(5)
            small = R.tile_buffer(np.ascontiguousarray(P[:, :, p0:]), K, Ncols, ns, 5) if ns else None
            big = R.tile_buffer(np.ascontiguousarray(P[:, :, :6]), K, Ncols, 1, 6) if big_first else None
            for a in (buf, small, big):
                if a is not None:
                    a.setflags(write=False)
            self.panels[key] = (buf, pt_k, pt_n, small, big)
        return self.panels[key]

    def close(self):
        for c in self.ctx.values():
            c.close()


@pytest.fixture(scope="module")
def env():
    e = Env()
    yield e
    e.close()


def first_diff(name, got, want, K, Ncols, ND, base=0):
    i = int(np.flatnonzero(got != want)[0])
    return f"{name}: {np.count_nonzero(got != want)} bytes differ, first at {base + i}: got {got[i]:#x}, want {want[i]:#x}, {R.locate(base + i, K, Ncols, ND, H)}"


def check_full(r, small, big, K, Ncols):
    """every tile byte is the reference's (rows past K and columns past Ncols zero), the guard bands hold the sentinel"""
    for name, got, want, ND in (("small", r["small"], small, 5), ("big", r["big"], big, 6)):
        if want is None:
            assert got is None or name == "small"
            continue
        assert got.size == want.size + R.GUARD
        assert np.array_equal(got[:want.size], want), first_diff(name, got[:want.size], want, K, Ncols, ND)
        assert (got[want.size:] == SENT).all(), f"{name}: guard band written"


def check_slice(r, small, big, K, Ncols, first, count):
    """bytes of items inside [first, first + count) are the reference's, bytes of every other item still hold the sentinel, and so do the guard bands"""
    n5 = r["n5"]
    for name, got, want, ND, base in (("small", r["small"], small, 5, 0), ("big", r["big"], big, 6, n5)):
        if want is None:
            continue
        nl = want.size // (H * ND * 1024 * np.prod(R.tile_geometry(K, Ncols)))
        item = R.item_of_piece(K, Ncols, int(nl), ND, H).reshape(-1) + base
        inside = (item >= first) & (item < first + count)
        g, w = got[:want.size].reshape(-1, 256), want.reshape(-1, 256)
        if not np.array_equal(g[inside], w[inside]):
            bad = np.flatnonzero((g != w).any(axis=1) & inside)[0]
            raise AssertionError(first_diff(f"{name}, first differing piece inside the slice", g[bad], w[bad], K, Ncols, ND, base=int(bad) * 256))
        out = g[~inside]
        assert (out == SENT).all(), f"{name}: {np.count_nonzero((out != SENT).any(axis=1))} pieces outside the slice written, first piece {np.flatnonzero((g != SENT).any(axis=1) & ~inside)[0]}"
        assert (got[want.size:] == SENT).all(), f"{name}: guard band written"


def run(env, chain, L, K, Ncols, layout, mode, a0=0, a1=0, a2=0, **kw):
    buf, pt_k, pt_n, small, big = env.panel(chain, L, K, Ncols, layout)
    r = env.context(chain).i8_move_for_test(buf, layout, pt_k, pt_n, K, Ncols, L, mode, a0, a1, a2, sentinel=SENT, **kw)
    assert np.array_equal(r["panel_after"], buf), "the input panel was written"
    return r, small, big


def pass_and_alone(env, chain, L, K, Ncols, layout=2):
    nd = env.nd(chain, L)
    n5 = R.items_of_run(K, Ncols, nd.count(5), H)
    n6 = R.items_of_run(K, Ncols, 1, H) if 6 in nd else 0
    for mode, args in ((0, (0, 0, 0)), (1, (0, n5 + n6, 192)), (1, (0, n5 + n6, 2048))):
        r, small, big = run(env, chain, L, K, Ncols, layout, mode, *args)
        assert r["on"] and (r["n5"], r["n6"]) == (n5, n6)
        check_full(r, small, big, K, Ncols)


# ---------------------------------------------------------------- the whole job: the pass, and the mover alone over every item
# K: a unit with one valid row, both sides of a 16-row unit and of a 64-row chunk, the product's 91 (units kq = 6, 7 have no valid row, kq = 5 eleven) and 2 * 91
@pytest.mark.parametrize("Ncols", [1, 17])
@pytest.mark.parametrize("K", [1, 15, 16, 17, 63, 64, 65, 91, 182])
def test_every_tile_byte_at_the_row_count_edges(env, K, Ncols):
    pass_and_alone(env, "pn14", 2, K, Ncols)


@pytest.mark.parametrize("Ncols", [2, 15, 16, 31, 32])          # (1 and 17 at K = 91: above)
def test_every_tile_byte_at_the_column_count_edges(env, Ncols):
    pass_and_alone(env, "pn14", 2, 91, Ncols)


@pytest.mark.parametrize("Ncols", [91, 96])
def test_every_tile_byte_at_six_column_tiles(env, Ncols):
    """the product's 91 columns and the 96 the MAC admits: njt = 6, on the all-35-bit chain at L = 1 (the one case above eight 40 MiB tile groups)"""
    pass_and_alone(env, "s1", 1, 91, Ncols)


@pytest.mark.parametrize("chain,L", [("pn14", 3), ("s1", 1), ("s1", 2)])          # (pn14 at L = 2: above)
def test_every_tile_byte_on_other_moduli_sets(env, chain, L):
    """two five-digit moduli behind the six-digit one (both arg blocks, both tile buffers, m = 1 of the small run); no six-digit modulus at all (n6 = 0)"""
    pass_and_alone(env, chain, L, 91, 17)


@pytest.mark.parametrize("layout", [0, 1, 2])
def test_every_tile_byte_from_each_panel_layout(env, layout):
    pass_and_alone(env, "pn14", 2, 91, 17, layout)


@pytest.mark.parametrize("chain,L", [("q47", 2), ("pn14", 1)])
def test_the_ride_declines_and_writes_nothing(env, chain, L):
    """a six-digit modulus above SFG_I8_BIG_QMAX; no 35-bit modulus: the hook reports that the ride declines, and launched nothing"""
    for mode, args in ((0, (0, 0, 0)), (1, (0, 1, 8)), (2, (1, 8, 1))):
        buf, pt_k, pt_n, _, _ = env.panel(chain, L, 17, 1, 2)
        pc = np.zeros((8, H)) if mode == 2 else None
        r = env.context(chain).i8_move_for_test(buf, 2, 0, 0, 17, 1, L, mode, *args, pc=pc, sentinel=SENT)
        assert not r["on"] and (r["n5"], r["n6"], r["leftover"]) == (0, 0, 0)
        assert not r["small"].any() and (r["big"] is None or not r["big"].any()) and (r["panel2"] is None or not r["panel2"].any())       # the host buffers as they were handed in
        assert np.array_equal(r["panel_after"], buf)


# ---------------------------------------------------------------- the mover alone on directed slices
@pytest.mark.parametrize("nblocks", R.NBLOCKS)
@pytest.mark.parametrize("shape", list(DIRECTED_SHAPES))
def test_directed_slices_move_their_items_and_no_others(env, shape, nblocks):
    """the slices of i8tile_ref.directed_slices (tests/test_i8tile_ref.py shows that they reach every class): the 5 / 6 boundary inside the slice at a first item
    that is no multiple of the workgroup count, fewer items than workgroups, one item, a slice ending exactly at n5"""
    chain, L = ("pn14", 2) if shape == "pn14_l2" else ("s1", 1)
    K, Ncols = 63, 15
    n5, n6 = DIRECTED_SHAPES[shape]
    for name, (first, count) in R.directed_slices(n5, n6, nblocks).items():
        r, small, big = run(env, chain, L, K, Ncols, 2, 1, first, count, nblocks)
        assert r["on"] and (r["n5"], r["n6"]) == (n5, n6), name
        try:
            check_slice(r, small, big, K, Ncols, first, count)
        except AssertionError as e:
            raise AssertionError(f"slice {name} = [{first}, {first} + {count}) at {nblocks} workgroups: {e}") from None


# ---------------------------------------------------------------- riding in plaintext-NTT launches
def coefficients(made):
    rnd = np.random.default_rng(made)
    return rnd.integers(-(1 << 20), 1 << 20, (max(made, 1) * 8, H)).astype(np.float64)


def ride_case(env, chain, L, predicted, nblocks, made, K=91, Ncols=17):
    pc = coefficients(made)
    r, small, big = run(env, chain, L, K, Ncols, 2, 2, predicted, nblocks, made, pc=pc)
    total = r["n5"] + r["n6"]
    carried, (lfirst, lcount) = R.ride_deal(total, predicted, made)
    assert r["on"] and r["per"] == R.launch_slices(total, predicted)[1]
    assert r["leftover"] == lcount, f"the leftover launch took {r['leftover']} items, the dealing leaves {lcount} (from {lfirst})"
    check_full(r, small, big, K, Ncols)
    key = (chain, L, made)
    if key not in env.nomover:
        env.nomover[key] = run(env, chain, L, K, Ncols, 2, 2, predicted, nblocks, made, pc=pc, no_mover=True)[0]
    ref = env.nomover[key]
    assert (ref["small"] == SENT).all() and (ref["big"] is None or (ref["big"] == SENT).all()), "NTT launches without mover workgroups wrote tiles"
    assert made == 0 or (ref["panel2"] != SENT).any()
    assert np.array_equal(r["panel2"], ref["panel2"]), "the second panel differs from the one the same NTT launches write without mover workgroups"
    return r, carried


@pytest.mark.parametrize("launches", [1, 3, 7])
def test_riding_with_as_many_launches_as_predicted(env, launches):
    r, carried = ride_case(env, "pn14", 2, launches, 192, launches)
    assert r["leftover"] == 0 and all(c > 0 for _, c in carried)


def test_riding_with_fewer_launches_than_predicted_leaves_exactly_the_rest(env):
    r, _ = ride_case(env, "pn14", 2, 7, 192, 3)
    assert r["leftover"] == 2048 - 3 * 293                       # per = ceil(2048 / 7) = 293


def test_riding_with_no_launch_at_all_leaves_everything_to_the_finish(env):
    r, _ = ride_case(env, "pn14", 2, 4, 192, 0)
    assert r["leftover"] == 2048


def test_riding_with_fewer_items_per_launch_than_mover_workgroups(env):
    r, _ = ride_case(env, "pn14", 2, 11, 192, 11)               # per = ceil(2048 / 11) = 187 < 192
    assert r["per"] == 187 and r["per"] < 192 and r["leftover"] == 0


def test_riding_with_more_launches_than_predicted(env):
    r, carried = ride_case(env, "pn14", 2, 2, 192, 5)           # the late launches carry nothing
    assert [c for _, c in carried] == [1024, 1024, 0, 0, 0] and r["leftover"] == 0


@pytest.mark.parametrize("predicted,nblocks,made", [(3, 8, 3), (5, 64, 2)])
def test_riding_without_a_six_digit_modulus_and_at_other_workgroup_counts(env, predicted, nblocks, made):
    ride_case(env, "s1", 2, predicted, nblocks, made)


# ---------------------------------------------------------------- in the product
_CHILD = r"""
import sys, numpy as np
sys.path.insert(0, 'tests'); sys.path.insert(0, '.')
import test_gpu_i8_move as T
out = T.two_block_column_product()
np.savez(sys.argv[1], words=out[0], ride=out[1], ride_plain=out[2], pack=out[3])
"""


def two_block_column_product():
    """the two-block-column product of tests/test_gpu_matmul.py (30 x (8192 + 25), squared, s = 1, level 5) with one random key for every rotation:
    (words, launches counted in ntt_ride_all, in ntt_plain_all, in mac_i8_pack_pt)"""
    from sfgwas_amd import capi
    from sfgwas_amd.params import rotations_for_matmul
    ctx = capi.Context(ol.Q_PN14, ol.P_PN14)
    try:
        key = capi.random_rotkey(list(ol.Q_PN14) + list(ol.P_PN14), ctx.beta, ctx.N, 5)
        for k in rotations_for_matmul():
            ctx.load_rotkey(ctx.galois(k), key)
        rnd = np.random.default_rng(2)
        geno = rnd.integers(-1, 3, (30, 8192 + 25)).astype(np.int8)
        A = np.stack([np.stack([np.stack([np.stack([rnd.integers(0, q, ctx.N, dtype=np.uint64) for q in ol.Q_PN14[:6]]) for _ in range(2)])])])
        words, _, _ = ctx.matmul_stream(A, 5, 5, geno, flags=capi.SFG_SQUARE)
        n = [capi.lib().sfg_last_phase_launches(ctx.h, ph.encode()) for ph in ("ntt_ride_all", "ntt_plain_all", "mac_i8_pack_pt")]
    finally:
        ctx.close()
    return words, n[0], n[1], n[2]


def test_the_two_block_column_product_rides_and_gives_the_words_of_the_pass(tmp_path):
    """What tells a reader that the product tests which claim to cover riding do ride: after the call the phase counters say that plaintext-NTT launches carried
    mover workgroups (ntt_ride_all), and the same product with SFG_PT_RIDE=0 (a child on the experimenters' build) counts none and gives identical words.
    mac_i8_pack_pt counts the transposition launches that are not riding: riding, the LAST MAC launch's two passes (35-bit run, 46-bit modulus) - nothing follows it
    to ride in - and no leftover launch (the first block column's items are all taken by the second column's NTT launches); without the ride, two passes for each
    of the two MAC launches."""
    from sfgwas_amd import capi
    words, ride, plain, pack = two_block_column_product()
    print(f"riding: ntt_ride_all {ride}, ntt_plain_all {plain}, mac_i8_pack_pt {pack}")
    assert ride > 0 and plain > 0
    assert pack == 2
    e = dict(os.environ)
    e.update(capi.env_for({"SFG_PT_RIDE": "0"}))
    assert e.get("SFG_LIB_PATH") == capi.AB_LIB_PATH
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    fout = str(tmp_path / "out.npz")
    r = subprocess.run([sys.executable, "-c", _CHILD, fout], cwd=root, env=e, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    got = np.load(fout)
    print(f"SFG_PT_RIDE=0: ntt_ride_all {int(got['ride'])}, ntt_plain_all {int(got['ride_plain'])}, mac_i8_pack_pt {int(got['pack'])}")
    assert int(got["ride"]) <= 0 and int(got["ride_plain"]) == ride + plain
    assert int(got["pack"]) == 4
    assert np.array_equal(got["words"], words)
