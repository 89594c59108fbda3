"""The int8 MAC's plaintext tile buffers, the three panel layouts they are made from and the dealing of the transposition's items, stated in numpy and plain
integers - independent of k_i8_pack_pt_digits, which tests/test_gpu_mover.py uses as the mover's reference.  No GPU.

THE TILE BUFFER of one modulus run (moduli l0 .. l0 + nl - 1, all with ND = 5 digit planes, or the one modulus with ND = 6):

    byte ((((m H + c) njt + jt) nch + ch) ND + d) 1024 + g 256 + j 16 + kk
        = plane byte d of panel row (k = 64 ch + 16 g + kk, column n = 16 jt + j, modulus l0 + m) at coefficient c,   ZERO where k >= K or n >= Ncols

with H = N/2 coefficients, nch = ceil(K / 64), njt = ceil(Ncols / 16).  (Read off i8_tile_off and the store of k_i8_pack_pt_digits in mac_i8.hip; i8_move_item /
i8_move_finish in i8_move.hpp address the same bytes: piece (c, d) of unit (m, jt, kq = 4 ch + g) is the 256 bytes at g 256 of that tile, lane j holds 16 k.)

AN ITEM of the transposition is (m, jt, kq, cb): 128 coefficients c = 128 cb .. + 127 of one 16-row unit, all ND planes; items are numbered
    ((m njt + jt) (4 nch) + kq) (H / 128) + cb
the five-digit run first (n5 items), then the six-digit modulus (n6 items).

A PANEL is the array P[k][n][plane][c] of bytes, plane running over the moduli's 5 / 6 planes in modulus order, placed in one of the layouts of i8_panel_rows."""
import numpy as np

GUARD = 4096


# ---------------------------------------------------------------- tiles
def tile_geometry(K, Ncols):
    return (K + 63) // 64, (Ncols + 15) // 16


def tile_buffer(planes, K, Ncols, nl, ND):
    """planes: uint8 [K][Ncols][nl * ND][H] (the run's planes only) -> the run's tile buffer, flat uint8"""
    H = planes.shape[-1]
    nch, njt = tile_geometry(K, Ncols)
    assert planes.shape == (K, Ncols, nl * ND, H)
    x = np.zeros((nch * 64, njt * 16, nl, ND, H), dtype=np.uint8)
    x[:K, :Ncols] = planes.reshape(K, Ncols, nl, ND, H)
    x = x.reshape(nch, 4, 16, njt, 16, nl, ND, H)               # ch g kk jt j m d c
    return np.ascontiguousarray(x.transpose(5, 7, 3, 0, 6, 1, 4, 2)).reshape(-1)      # m c jt ch d g j kk


def tile_buffer_literal(planes, K, Ncols, nl, ND):
    """the statement of the module docstring as four nested loops over the panel's bytes (tiny shapes only)"""
    H = planes.shape[-1]
    nch, njt = tile_geometry(K, Ncols)
    out = np.zeros(nl * H * njt * nch * ND * 1024, dtype=np.uint8)
    for k in range(K):
        for n in range(Ncols):
            for p in range(nl * ND):
                for c in range(H):
                    m, d = divmod(p, ND)
                    ch, g, kk, jt, j = k // 64, (k % 64) // 16, k % 16, n // 16, n % 16
                    out[((((m * H + c) * njt + jt) * nch + ch) * ND + d) * 1024 + g * 256 + j * 16 + kk] = planes[k, n, p, c]
    return out


def item_of_piece(K, Ncols, nl, ND, H):
    """int32 [nl][H][njt][nch][ND][4]: the item (numbered within its run) that writes each 256-byte piece of the run's tile buffer"""
    nch, njt = tile_geometry(K, Ncols)
    m = np.arange(nl).reshape(nl, 1, 1, 1, 1, 1)
    c = np.arange(H).reshape(1, H, 1, 1, 1, 1)
    jt = np.arange(njt).reshape(1, 1, njt, 1, 1, 1)
    ch = np.arange(nch).reshape(1, 1, 1, nch, 1, 1)
    g = np.arange(4).reshape(1, 1, 1, 1, 1, 4)
    it = ((m * njt + jt) * (4 * nch) + 4 * ch + g) * (H // 128) + c // 128
    return np.broadcast_to(it, (nl, H, njt, nch, ND, 4)).astype(np.int32)


def items_of_run(K, Ncols, nl, H):
    nch, njt = tile_geometry(K, Ncols)
    return nl * njt * nch * 4 * (H // 128)


def locate(offset, K, Ncols, ND, H):
    """a byte offset of a run's tile buffer -> dict(m, c, jt, ch, d, g, j, kk, k, n, item): where a differing byte belongs"""
    nch, njt = tile_geometry(K, Ncols)
    r, kk = divmod(int(offset), 16)
    r, j = divmod(r, 16)
    r, g = divmod(r, 4)
    r, d = divmod(r, ND)
    r, ch = divmod(r, nch)
    r, jt = divmod(r, njt)
    m, c = divmod(r, H)
    item = ((m * njt + jt) * (4 * nch) + 4 * ch + g) * (H // 128) + c // 128
    return dict(m=m, c=c, jt=jt, ch=ch, d=d, g=g, j=j, kk=kk, k=64 * ch + 16 * g + kk, n=16 * jt + j, item=item)


# ---------------------------------------------------------------- panel layouts (i8_panel_rows).  Each takes P uint8 [K][Ncols][planes][H], nd = the planes per
# modulus in modulus order, and a generator for the filler bytes: everything that is not a plane byte - the unused part of a word row, the rows between K and the end
# of the last 64-row chunk, which the mover addresses - is RANDOM, so that a byte wrongly taken from there shows.  Returns (buffer uint8, pt_k, pt_n), strides in words.
def place_rows(P, nd, rnd):
    """layout 0: a plaintext is L rows of H words (8 H bytes); the 5 / 6 planes of a modulus are the first 5 H / 6 H bytes of its row"""
    K, Ncols, planes, H = P.shape
    L = len(nd)
    assert sum(nd) == planes
    rows = ((K + 63) // 64) * 64
    buf = rnd.integers(0, 256, (rows, Ncols, L, 8 * H), dtype=np.uint8)
    p0 = 0
    for l in range(L):
        buf[:K, :, l, :nd[l] * H] = P[:, :, p0:p0 + nd[l], :].reshape(K, Ncols, nd[l] * H)
        p0 += nd[l]
    return buf.reshape(-1), Ncols * L * H, L * H


def place_compact(P, nd, rnd):
    """layout 1: a plaintext's planes back to back"""
    K, Ncols, planes, H = P.shape
    rows = ((K + 63) // 64) * 64
    buf = rnd.integers(0, 256, (rows, Ncols, planes, H), dtype=np.uint8)
    buf[:K] = P
    assert planes * H % 8 == 0
    return buf.reshape(-1), Ncols * planes * H // 8, planes * H // 8


def place_kmajor(P, nd, rnd):
    """layout 2: [column][plane][128-byte coefficient block][k < K][128 B], and (64 ceil(K/64) - K) * 128 filler bytes behind the last block"""
    K, Ncols, planes, H = P.shape
    body = np.ascontiguousarray(P.reshape(K, Ncols, planes, H // 128, 128).transpose(1, 2, 3, 0, 4)).reshape(-1)
    tail = rnd.integers(0, 256, (((K + 63) // 64) * 64 - K) * 128, dtype=np.uint8)
    return np.concatenate([body, tail]), 0, 0


PLACE = {0: place_rows, 1: place_compact, 2: place_kmajor}


# ---------------------------------------------------------------- the dealing
def launch_slices(total, launches):
    """(first, count) of the slice every NTT launch of a ride carries when `launches` were predicted (i8_ride_prepare: per = ceil(total / launches);
    i8_ride_take: `per` items from where the last launch stopped, the last slice whatever is left), and `per`"""
    per = (total + launches - 1) // launches
    out, nxt = [], 0
    while nxt < total:
        cnt = min(per, total - nxt)
        out.append((nxt, cnt))
        nxt += cnt
    return out, per


def ride_deal(total, predicted, made):
    """the slices of `made` launches ((first, 0): carries nothing) and the (first, count) i8_ride_finish takes"""
    sl, _ = launch_slices(total, predicted)
    carried = [sl[i] if i < len(sl) else (total, 0) for i in range(made)]
    nxt = sum(c for _, c in carried)
    return carried, (nxt, total - nxt)


def block_items(first, count, n5, n6, nblocks, mb):
    """the items (numbered over both runs) that i8_move_block gives mover workgroup mb of nblocks for the slice [first, first + count): the arithmetic of the
    kernel, start = lo6 + (ph + nb - r) % nb included"""
    lo, hi, nb = first, first + count, nblocks
    out = []
    hi5 = min(hi, n5)
    if lo < hi5:
        out += list(range(lo + mb, hi5, nb))
    if hi > n5:
        lo6 = max(lo, n5)
        ph, r = (lo + mb) % nb, lo6 % nb
        start = lo6 + (ph + nb - r) % nb
        out += [n5 + i for i in range(start - n5, hi - n5, nb)]
    return out


CLASSES = ("five", "six", "cross_aligned", "cross_unaligned", "short", "n6_zero")


def classify(first, count, n5, n6, nblocks):
    """the classes of CLASSES a slice belongs to (they overlap)"""
    c = set()
    hi = first + count
    if hi <= n5:
        c.add("five")
    elif first >= n5:
        c.add("six")
    else:
        c.add("cross_aligned" if n5 % nblocks == 0 else "cross_unaligned")
    if count < nblocks:
        c.add("short")
    if n6 == 0:
        c.add("n6_zero")
    return c


NBLOCKS = (8, 64, 192, 2048)


def directed_slices(n5, n6, nblocks):
    """the slices tests/test_gpu_i8_move.py moves alone at `nblocks` workgroups: named (first, count)"""
    nb, total = nblocks, n5 + n6
    s = {}
    if n6:
        f = max(1, n5 - 2 * nb - 3)
        if f % nb == 0:
            f += 1
        s["crossing"] = (f, min(n5 - f + 2 * nb + 5, total - f))                 # the boundary inside, first no multiple of nblocks
        s["crossing_short"] = (n5 - 3, min(nb - 1, 7))                          # fewer items than workgroups, across the boundary
        s["six_only"] = (n5 + 3, min(2 * nb + 1, n6 - 3))
        s["one_item_six"] = (n5 + 5, 1)
    f = max(3, n5 - nb - 3)
    s["ends_at_n5"] = (f, n5 - f)                                               # ends exactly at n5
    s["five_only"] = (3, min(2 * nb + 1, n5 - 8))
    s["one_item_five"] = (7, 1)
    return s
