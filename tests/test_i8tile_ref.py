"""CPU checks of tests/i8tile_ref.py: the tile statement against a literal loop, the layouts against each other, the dealing of items to launches and workgroups as an
exact partition, and the condition that the directed slices tests/test_gpu_i8_move.py moves reach every class of slice."""
import itertools

import numpy as np
import pytest

import i8tile_ref as R


@pytest.mark.parametrize("K,Ncols,nl,ND", [(1, 1, 1, 5), (5, 3, 2, 5), (17, 2, 1, 6), (65, 17, 1, 5), (64, 16, 2, 5)])
def test_tile_buffer_is_the_literal_statement(K, Ncols, nl, ND):
    rnd = np.random.default_rng(K * 100 + Ncols)
    H = 128
    P = rnd.integers(1, 256, (K, Ncols, nl * ND, H), dtype=np.uint8)          # no zero byte: a zero in the tiles is a row past K or a column past Ncols
    got = R.tile_buffer(P, K, Ncols, nl, ND)
    want = R.tile_buffer_literal(P, K, Ncols, nl, ND)
    assert np.array_equal(got, want)
    nch, njt = R.tile_geometry(K, Ncols)
    t = got.reshape(nl, H, njt, nch, ND, 4, 16, 16)                          # m c jt ch d g j kk
    k = (64 * np.arange(nch)[:, None, None] + 16 * np.arange(4)[None, :, None] + np.arange(16)[None, None, :])       # ch g kk
    n = 16 * np.arange(njt)[:, None] + np.arange(16)[None, :]                                                           # jt j
    valid = (k < K)[None, :, :, None, :] & (n < Ncols)[:, None, None, :, None]                                          # jt ch g j kk
    tt = t.transpose(0, 1, 4, 2, 3, 5, 6, 7)                                                                              # m c d jt ch g j kk
    assert (tt[..., ~valid] == 0).all() and (tt[..., valid] != 0).all()


def test_locate_inverts_the_tile_address_and_item_of_piece_agrees():
    K, Ncols, nl, ND, H = 91, 17, 2, 5, 256
    nch, njt = R.tile_geometry(K, Ncols)
    items = R.item_of_piece(K, Ncols, nl, ND, H)
    assert items.max() + 1 == R.items_of_run(K, Ncols, nl, H) and items.min() == 0
    rnd = np.random.default_rng(1)
    for off in rnd.integers(0, nl * H * njt * nch * ND * 1024, 200):
        w = R.locate(off, K, Ncols, ND, H)
        assert ((((w["m"] * H + w["c"]) * njt + w["jt"]) * nch + w["ch"]) * ND + w["d"]) * 1024 + w["g"] * 256 + w["j"] * 16 + w["kk"] == off
        assert items[w["m"], w["c"], w["jt"], w["ch"], w["d"], w["g"]] == w["item"]
    # every item owns ND * 128 pieces
    assert (np.bincount(items.reshape(-1)) == ND * 128).all()


def test_the_three_layouts_hold_the_same_panel():
    rnd = np.random.default_rng(2)
    K, Ncols, H, nd = 5, 3, 256, [6, 5, 5]
    P = rnd.integers(0, 256, (K, Ncols, sum(nd), H), dtype=np.uint8)
    b0, k0, n0 = R.place_rows(P, nd, rnd)
    b1, k1, n1 = R.place_compact(P, nd, rnd)
    b2, _, _ = R.place_kmajor(P, nd, rnd)
    assert b2.size == P.size + (64 - K) * 128
    below = np.concatenate([[0], np.cumsum(nd)])
    for k, n, l, c in itertools.product(range(K), range(Ncols), range(3), (0, 1, 127, 128, 255)):
        for d in range(nd[l]):
            p = below[l] + d
            assert b0[(k * k0 + n * n0) * 8 + l * H * 8 + d * H + c] == P[k, n, p, c]                 # i8_panel_rows: pt_l0_off = l H words, pt_d_stride = H
            assert b1[(k * k1 + n * n1) * 8 + p * H + c] == P[k, n, p, c]                             # pt_l0_off = below H / 8 words
            assert b2[(((n * sum(nd) + p) * (H // 128) + c // 128) * K + k) * 128 + c % 128] == P[k, n, p, c]


def test_block_items_is_the_round_robin_with_its_phase_kept_and_an_exact_partition():
    checked = 0
    for nb in (1, 2, 3, 5, 8):
        for n5, n6 in itertools.product((0, 1, 4, 7, 8, 16), (0, 3, 8, 9)):
            total = n5 + n6
            for first in range(total):
                for count in range(1, total - first + 1):
                    per_block = [R.block_items(first, count, n5, n6, nb, mb) for mb in range(nb)]
                    for mb, got in enumerate(per_block):
                        assert got == [i for i in range(first, first + count) if (i - first) % nb == mb], (n5, n6, first, count, nb, mb)
                    assert sorted(sum(per_block, [])) == list(range(first, first + count))
                    checked += 1
    assert checked > 10000


@pytest.mark.parametrize("total", [1, 7, 8, 1024, 2048, 2049, 6144])
def test_launch_slices_partition_the_items_and_ride_deal_hands_the_rest_to_the_finish(total):
    for launches in (1, 2, 3, 7, 11, 100, total, total + 5):
        sl, per = R.launch_slices(total, launches)
        assert per == -(-total // launches) and len(sl) <= launches
        assert [f for f, _ in sl] == [i * per for i in range(len(sl))] and sum(c for _, c in sl) == total
        assert all(c == per for _, c in sl[:-1]) and 1 <= sl[-1][1] <= per
        for made in (0, 1, launches - 1, launches, launches + 3):
            if made < 0:
                continue
            carried, (lf, lc) = R.ride_deal(total, launches, made)
            assert len(carried) == made and sum(c for _, c in carried) + lc == total and lf == total - lc
            assert all(c == 0 for _, c in carried[len(sl):])
            if made >= len(sl):
                assert lc == 0


# the shapes of the directed-slice cases of tests/test_gpu_i8_move.py: K = 63, Ncols = 15 on PN14 at L = 2 (one five-digit and the six-digit modulus) and on the
# all-35-bit chain at L = 1
DIRECTED_SHAPES = {"pn14_l2": (256, 256), "s1_l1": (256, 0)}


def test_directed_slices_reach_every_class():
    H = 8192
    assert R.items_of_run(63, 15, 1, H) == 256
    seen = set()
    for n5, n6 in DIRECTED_SHAPES.values():
        for nb in R.NBLOCKS:
            sl = R.directed_slices(n5, n6, nb)
            for name, (first, count) in sl.items():
                assert 0 <= first and count >= 1 and first + count <= n5 + n6, (name, nb)
                seen |= R.classify(first, count, n5, n6, nb)
            if n6:
                f, c = sl["crossing"]
                assert f % nb != 0 and f < n5 < f + c
                f, c = sl["crossing_short"]
                assert c < nb and f < n5 < f + c
            assert sl["ends_at_n5"][0] + sl["ends_at_n5"][1] == n5
            assert sl["one_item_five"][1] == 1
    assert seen == set(R.CLASSES)
    # both kinds of crossing come from the choice of workgroup counts: 256 is a multiple of 8 and 64, not of 192 or 2048
    n5, n6 = DIRECTED_SHAPES["pn14_l2"]
    kinds = {nb: R.classify(*R.directed_slices(n5, n6, nb)["crossing"], n5, n6, nb) & {"cross_aligned", "cross_unaligned"} for nb in R.NBLOCKS}
    assert kinds == {8: {"cross_aligned"}, 64: {"cross_aligned"}, 192: {"cross_unaligned"}, 2048: {"cross_unaligned"}}
