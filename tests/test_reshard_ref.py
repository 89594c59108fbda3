"""tests/reshard_ref.py against literal loops, and the inputs of tests/test_gpu_reshard.py against the cases the re-sharding kernels distinguish (conditions on
the inputs, not measurements: a seed that misses one is changed)."""
import numpy as np

import reshard_ref as rr
from sfgwas_amd.sharding import SLOTS, snp_block_range


def test_windows_and_memory_images_equal_literal_loops():
    nrow, ncol, world = 5, 2 * SLOTS + 9, 3
    geno = rr.make_geno(nrow, ncol, 7)
    rf, cf = rr.make_filters(nrow, ncol, 7, p_row=0.6, p_col=0.55)
    rows = [i for i in range(nrow) if rf[i]]
    cols = [j for j in range(ncol) if cf[j]]
    assert len(cols) > SLOTS
    got = rr.windows(geno, rf, cf, world)
    seen = 0
    for r in range(world):
        nblk = (len(cols) + SLOTS - 1) // SLOTS
        c0, c1 = min(nblk * r // world * SLOTS, len(cols)), min(nblk * (r + 1) // world * SLOTS, len(cols))
        assert (c0, c1) == snp_block_range(len(cols), r, world)[2:]
        if c1 == c0:
            assert got[r] is None
            continue
        assert got[r].shape == (len(rows), c1 - c0) and got[r].dtype == np.int8
        for a, i in enumerate(rows):
            for b in range(c1 - c0):
                assert got[r][a, b] == geno[i, cols[c0 + b]]
        seen += c1 - c0
        img8, img2 = rr.int8_image(got[r]), rr.packed_image(got[r])
        w, ld = c1 - c0, (c1 - c0 + 15) // 16 * 16
        assert img8.shape == (len(rows), ld) and img2.shape == (len(rows), ld // 16) and img2.dtype == np.uint32
        for a in range(len(rows)):
            for b in range(ld):
                v = int(got[r][a, b]) if b < w else 0
                assert img8[a, b] == v
                assert (int(img2[a, b // 16]) >> (2 * (b % 16))) & 3 == (3 if v < 0 else v)
    assert seen == len(cols)
    # no filters: the old windows themselves
    for r, win in enumerate(rr.windows(geno, None, None, world)):
        c0, c1 = rr.old_windows(ncol, world)[r]
        assert (win is None and c0 == c1) or np.array_equal(win, geno[:, c0:c1])


def test_owners_equal_a_literal_search():
    ncol, world = rr.NCOL5, 8
    cols = np.arange(0, ncol, 997)
    own = rr.owners(ncol, cols, world)
    for c, o in zip(cols, own):
        assert [r for r, (c0, c1) in enumerate(rr.old_windows(ncol, world)) if c0 <= c < c1] == [o]


def _draws(name, world):
    """per new rank with a window: (source columns, their old owners)"""
    geno, rf, cf = rr.case(name)
    return [(cols, rr.owners(geno.shape[1], cols, world)) for cols in rr.new_windows(geno.shape[1], cf, world) if len(cols)]


def test_the_gpu_inputs_reach_every_case():
    geno, rf, cf = rr.case("blocks13")
    assert geno.shape == (rr.NROW, rr.NCOL13) and set(np.unique(geno)) == {-1, 0, 1, 2}
    assert 0 < rf.sum() < rr.NROW and 4 * SLOTS < cf.sum() <= 5 * SLOTS                     # about 5 blocks are kept
    # (a) a packed output dword whose 16 kept columns come from two old ranks - at every world
    for world in rr.WORLDS:
        split = 0
        for cols, own in _draws("blocks13", world):
            for d in range(0, len(cols) - 15, 16):
                split += own[d] != own[d + 15]
        assert split > 0, world
    # (b) a new window that draws on at least 3 old ranks
    assert max(len(set(own)) for _, own in _draws("blocks13", 8)) >= 3
    # (c) a new rank without a window; an old rank that owns no block
    assert any(len(c) == 0 for c in rr.new_windows(rr.NCOL13, cf, 8))
    assert sum(c0 == c1 for c0, c1 in rr.old_windows(rr.NCOL5, 8)) == 3
    assert any(len(set(own)) >= 2 for _, own in _draws("blocks5", 8))
    # (d) an old rank all of whose columns are dropped, between two ranks that keep some
    _, _, cfd = rr.case("window_dropped")
    (a0, a1), (b0, b1), (c0, c1) = rr.old_windows(rr.NCOL13, 3)
    assert b1 > b0 and not cfd[b0:b1].any() and cfd[a0:a1].any() and cfd[c0:c1].any()
    assert any(set(own) == {0, 2} for _, own in _draws("window_dropped", 3))                # a window that jumps over the dropped rank
    # (e) a new window whose first kept column is not a multiple of 4 in its source shard
    odd = 0
    for world in rr.WORLDS:
        for cols, own in _draws("blocks13", world):
            odd += (cols[0] - rr.old_windows(rr.NCOL13, world)[own[0]][0]) % 4 != 0
    assert odd > 0
