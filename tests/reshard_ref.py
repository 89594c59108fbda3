"""What sfg_mgpu_geno_filter must give, stated in numpy: the filtered matrix X[rows][:, cols] cut into the windows sfgwas_amd/sharding.py gives the ranks over
the KEPT columns, the bytes those windows have in device memory (int8 rows padded with zeros to 16 bytes; 2-bit codes, 16 to a little-endian dword, code 3 =
missing, padding codes 0), and which old ranks a new window draws on.  tests/test_reshard_ref.py pins this file against literal loops and asserts that the
inputs below reach every case the kernels distinguish; tests/test_gpu_reshard.py holds the library to it."""
import numpy as np

from sfgwas_amd.sharding import SLOTS, snp_block_range

NROW, NCOL13, NCOL5 = 37, 13 * SLOTS - 77, 5 * SLOTS
WORLDS = (2, 3, 8)


def mask(f, n):
    return np.ones(n, dtype=bool) if f is None else np.asarray(f) != 0


def make_geno(nrow, ncol, seed):
    """values 0, 1, 2 and -1 (the one missing value a packed matrix gives back)"""
    return np.random.default_rng(seed).choice(np.array([-1, 0, 1, 2], dtype=np.int8), size=(nrow, ncol), p=[0.1, 0.4, 0.3, 0.2])


def make_filters(nrow, ncol, seed, p_row=0.9, p_col=0.37):
    rnd = np.random.default_rng(seed + 1000)
    return (rnd.random(nrow) < p_row).astype(np.uint8), (rnd.random(ncol) < p_col).astype(np.uint8)


def old_windows(ncol, world):
    """[c0, c1) of every old rank (c0 == c1: the rank owns no block)"""
    return [snp_block_range(ncol, r, world)[2:] for r in range(world)]


def new_windows(ncol, col_filter, world):
    """per new rank: the global source columns of its window, in order (empty: the rank has no window)"""
    kept = np.flatnonzero(mask(col_filter, ncol))
    return [kept[c0:c1] for c0, c1 in (snp_block_range(len(kept), r, world)[2:] for r in range(world))]


def windows(geno, row_filter, col_filter, world):
    """per new rank: its window of the filtered matrix (None: no window)"""
    rows = geno[mask(row_filter, geno.shape[0])]
    return [np.ascontiguousarray(rows[:, cols]) if len(cols) else None for cols in new_windows(geno.shape[1], col_filter, world)]


def owners(ncol, cols, world):
    """the old rank that holds each global column of `cols`"""
    starts = np.array([c0 for c0, _ in old_windows(ncol, world)])
    ends = np.array([c1 for _, c1 in old_windows(ncol, world)])
    own = np.searchsorted(ends, cols, side="right")
    assert np.all((starts[own] <= cols) & (cols < ends[own]))
    return own


def int8_image(win):
    """a window's rows as they lie in device memory: row stride = the width rounded up to 16 bytes, padding 0"""
    ld = (win.shape[1] + 15) // 16 * 16
    img = np.zeros((win.shape[0], ld), dtype=np.int8)
    img[:, :win.shape[1]] = win
    return img


def packed_image(win):
    """a window's rows as 2-bit codes: [nrow][ceil(w / 16)] uint32, column 16 d + k in bits 2 k .. 2 k + 1 of dword d, negative -> 3, padding codes 0"""
    nrow, w = win.shape
    ldw = (w + 15) // 16
    code = np.zeros((nrow, ldw * 16), dtype=np.uint32)
    code[:, :w] = np.where(win < 0, 3, win).astype(np.uint32)
    return (code.reshape(nrow, ldw, 16) << (2 * np.arange(16, dtype=np.uint32))).sum(axis=2, dtype=np.uint32)


# ---- the inputs of tests/test_gpu_reshard.py (made once per process; nothing below changes them)
_cache = {}


def case(name):
    """(geno, row_filter, col_filter) of a named input"""
    if name not in _cache:
        if name == "blocks13":                       # about 5 blocks kept of 13: at world 8 new ranks without a window, and windows that draw on three old ranks
            geno, (rf, cf) = make_geno(NROW, NCOL13, 1), make_filters(NROW, NCOL13, 1)
        elif name == "window_dropped":               # case (d), world 3: every column of old rank 1 (blocks 4 .. 7) is dropped
            geno, (rf, cf) = make_geno(NROW, NCOL13, 2), make_filters(NROW, NCOL13, 2, p_col=0.6)
            c0, c1 = old_windows(NCOL13, 3)[1]
            cf[c0:c1] = 0
        elif name == "blocks5":                      # 5 blocks at world 8: the old ranks 0, 2 and 5 own nothing
            geno, (rf, cf) = make_geno(NROW, NCOL5, 3), make_filters(NROW, NCOL5, 3, p_col=0.5)
        else:
            raise KeyError(name)
        for a in (geno, rf, cf):
            a.setflags(write=False)
        _cache[name] = (geno, rf, cf)
    return _cache[name]
