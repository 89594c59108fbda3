"""CPU check of the multi-GPU engine's sharding arithmetic for every world size up to 64 (the engine's limit of local ranks): the library's SNP-block shard
(sfg_mgpu_shard, mgpu.hip) against sfgwas_amd/sharding.py, and the giant-slot windows of Q'*X^T's reduce-scatter (gpr = ceil(91 / world) slots per rank, rank r
holding giant steps [r gpr, r gpr + gpr); mgpu.hip rank_contract) - including the worlds in which a rank holds nothing but padding slots."""
import ctypes as C

from sfgwas_amd.sharding import SLOTS, D, ceil_div, snp_block_range, giant_slots

WORLDS = range(1, 65)

# world sizes <= 64 whose last rank holds padding slots only (gpr (world - 1) >= 91): its finalize aligns no giant step and must contribute zeros to the all-reduce
# (tests/test_gpu_mgpu_wide.py runs world 14 on the GPU).  16, 19, 23, 31 and 46 avoid it; world 24 is three 8-GPU nodes.
NO_GIANT_WORLDS = [14, 15, 17, 18, 20, 21, 22] + list(range(24, 31)) + list(range(32, 46)) + list(range(47, 65))


def test_library_shard_equals_the_python_arithmetic_and_partitions_the_blocks():
    from sfgwas_amd import capi
    lib = capi.lib()
    v = [C.c_size_t() for _ in range(4)]
    refs = [C.byref(x) for x in v]
    for nblk in range(1, 41):
        for ncol in sorted({(nblk - 1) * SLOTS + 1, nblk * SLOTS - 77, nblk * SLOTS}):
            assert ceil_div(ncol, SLOTS) == nblk
            for world in WORLDS:
                nxt_blk, nxt_col, empty = 0, 0, 0
                for r in range(world):
                    assert lib.sfg_mgpu_shard(world, ncol, r, *refs) == 0
                    got = tuple(x.value for x in v)
                    assert got == snp_block_range(ncol, r, world), (nblk, ncol, world, r, got)
                    b0, b1, c0, c1 = got
                    assert (b0, c0) == (nxt_blk, nxt_col), (nblk, ncol, world, r)          # contiguous, in rank order, no gap and no overlap
                    assert b0 <= b1 and c0 <= c1 and (c1 > c0) == (b1 > b0)
                    assert b1 - b0 in (nblk // world, ceil_div(nblk, world))                 # balanced to within one block
                    nxt_blk, nxt_col = b1, c1
                    empty += b1 == b0
                assert (nxt_blk, nxt_col) == (nblk, ncol), (nblk, ncol, world)
                assert empty == max(0, world - nblk), (nblk, ncol, world)
    for bad in ((0, 100, 0), (4, 100, 4), (4, 100, -1), (4, 0, 0)):
        assert lib.sfg_mgpu_shard(*bad, None, None, None, None) != 0, bad


def test_giant_slots_cover_every_giant_step_once_with_padding_to_world_times_gpr():
    no_giant = []
    for world in WORLDS:
        gpr = ceil_div(D, world)
        seen = []
        for r in range(world):
            g, lo, hi = giant_slots(r, world)
            assert g == gpr and lo == r * gpr
            assert hi == min(lo + gpr, D) and (hi >= lo or lo >= D)
            seen += list(range(lo, max(lo, hi)))
        assert seen == list(range(D)), world                            # 0 .. 90, each exactly once, in rank order
        assert world * gpr >= D and world * gpr - D < world             # padded slot count: the least multiple of world >= 91
        if any(giant_slots(r, world)[1] >= D for r in range(world)):
            no_giant.append(world)
            assert giant_slots(world - 1, world)[1] >= D                # only ever the last rank(s)
    assert no_giant == NO_GIANT_WORLDS
    assert {4, 8, 16} & set(no_giant) == set() and 14 in no_giant and 24 in no_giant
