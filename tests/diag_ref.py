"""The generalized-diagonal statement of the matrix products, in numpy, independent of the oracle (matmult.go:636-672, 1292-1303):

    clean(x)       = 0 for x < 0 (a missing genotype), else x; squared in int8 arithmetic when asked (12 -> 144 -> -112)
    v[shift][j]    = clean(X)[(shift + j) mod 8192][j]   where that row is < r and j < c, else 0
    diag(shift)    = v[shift] rotated right by 91 * (shift // 91)
    exists(shift)  = shift < r  or  shift > 8192 - c     (GetDiagBool with index = -shift)

and what the tests of the extraction share: decode_rows (plaintext words at q0 -> slot integers, one batched FFT), the input generators, the list of
block shapes / strides / base offsets, the shifts and 128-shift tiles checked on each, and a restatement of which of k_skew's three load paths a
shape takes.  Nothing here touches the GPU."""
import functools
from collections import namedtuple

import numpy as np

SLOTS, D, N = 8192, 91, 16384
Q0 = 0x200000440001                      # the 46-bit modulus of the PN14 chain (sfgwas_amd/params.py: Q_PN14[0])
SCALE_LOG2 = 34
SENTINEL = 0x55                          # fill of the buffers around a view: 85 in a diagonal is a read outside the view
TILE = 128                               # shifts per workgroup of k_skew


# ------------------------------------------------------------------------------------------------ the statement
def exists(r, c, shift, dim=SLOTS):
    return shift < r or shift > dim - c


def runs(r, c, dim=SLOTS):
    """the existing shifts as half-open runs: [0, r) and (dim - c, dim), or everything when they meet"""
    if r + c > dim:
        return [(0, dim)]
    return [(0, r)] + ([(dim - c + 1, dim)] if c > 1 else [])


def square8(x):
    """x * x in int8 arithmetic (Go: int8 * int8 wraps), for an int8 array"""
    x = np.asarray(x, dtype=np.int8).astype(np.int32)
    return ((x * x) & 0xFF).astype(np.uint8).view(np.int8)


def clean(block, square=False):
    b = np.asarray(block, dtype=np.int8)
    b = np.where(b < 0, np.int8(0), b)
    return square8(b) if square else b


def diags(block, shifts, square=False, dim=SLOTS, d=D):
    """[len(shifts)][dim] int8: the rotated diagonals of the logical r x c block, by index arithmetic"""
    r, c = block.shape
    X = clean(block, square)
    sh = np.asarray(shifts, dtype=np.int32).reshape(-1, 1)
    p = np.arange(dim, dtype=np.int32).reshape(1, -1)
    j = (p - d * (sh // d)) % dim                    # slot p of the rotated vector holds column j
    i = (sh + j) % dim
    ok = (i < r) & (j < c)
    v = X[np.minimum(i, r - 1), np.minimum(j, c - 1)]
    return np.where(ok, v, np.int8(0)).astype(np.int8)


def diag(block, shift, square=False, dim=SLOTS, d=D):
    return diags(block, [shift], square, dim, d)[0]


# ------------------------------------------------------------------------------------------------ decoding
@functools.lru_cache(maxsize=None)
def _embedding(n):
    M = 4 * n
    idx = np.zeros(n, dtype=np.int64)
    g = 1
    for t in range(n):
        idx[t] = ((g - 1) // 4) % n
        g = g * 5 % M
    return np.exp(2j * np.pi * np.arange(n) / M), idx


def slot_values(words_q0, q0=Q0, scale_log2=SCALE_LOG2):
    """[rows][N] canonical coefficient-domain words mod q0 -> [rows][N/2] complex slot values (pyref.decode's formula, batched):
    v_t = sum_c w_c zeta^(5^t c), w_c = (p_c + i p_{c+n}) / 2^34 with p centred at q0 / 2"""
    w = np.asarray(words_q0, dtype=np.uint64)
    assert w.ndim == 2 and int(w.max(initial=0)) < q0
    n = w.shape[1] // 2
    p = w.astype(np.int64)
    p = np.where(p > q0 // 2, p - q0, p).astype(np.float64) * 2.0 ** -scale_log2       # |p| < 2^45: exact
    tw, idx = _embedding(n)
    V = np.fft.ifft((p[:, :n] + 1j * p[:, n:]) * tw, axis=1) * n
    return V[:, idx]


def decode_rows(words_q0, q0=Q0, scale_log2=SCALE_LOG2):
    """-> (the slot values rounded to integers [rows][N/2] int64, the largest distance of a slot value from its integer)"""
    V = slot_values(words_q0, q0, scale_log2)
    ints = np.rint(V.real)
    resid = float(np.abs(V - ints).max(initial=0.0))
    return ints.astype(np.int64), resid


RESIDUAL_BOUND = 2.0 ** -20      # N coefficients each off by at most 1/2 after rounding: N * (1/2) / 2^34 = 2^-21 on a slot; asserted with one bit to spare


# ------------------------------------------------------------------------------------------------ inputs
def gen_uniform(shape, seed):
    """all 256 int8 values; about a quarter of the entries negative"""
    rnd = np.random.default_rng(seed)
    neg = rnd.random(shape) < 0.25
    return np.where(neg, rnd.integers(-128, 0, shape), rnd.integers(0, 128, shape)).astype(np.int8)


def gen_genotype(shape, seed):
    return np.random.default_rng(seed).integers(-1, 3, shape).astype(np.int8)


def gen_signs(shape, seed):
    """every 4-byte group along the contiguous axis takes one of the 16 sign patterns (bit k of the pattern: byte k negative); the pattern advances
    with the group and with the row, so that every aligned dword of k_skew's missing -> 0 mask sees all 16.  Magnitudes 1..127."""
    rows, cols = shape
    rnd = np.random.default_rng(seed)
    mag = rnd.integers(1, 128, shape)
    col = np.arange(cols).reshape(1, -1)
    pat = (col // 4 + np.arange(rows).reshape(-1, 1)) % 16
    neg = (pat >> (col % 4)) & 1
    return np.where(neg == 1, -mag, mag).astype(np.int8)


def gen_const(v):
    return lambda shape, seed: np.full(shape, v, dtype=np.int8)


GENERATORS = {"uniform": gen_uniform, "genotype": gen_genotype, "signs": gen_signs,
              "c127": gen_const(127), "cm128": gen_const(-128), "c11": gen_const(11), "c12": gen_const(12)}
ROTATION = ["uniform", "genotype", "signs", "c127", "cm128", "c11", "c12"]


# ------------------------------------------------------------------------------------------------ the shape list
# r x c: the logical block.  tr: stored transposed (c rows of r contiguous bytes).  ld: stride of a stored row in bytes.  off: first byte of the view
# inside its buffer (the buffer itself starts on an allocation boundary).  sentinel: the bytes around the view are SENTINEL.  every: all 8192 shifts.
Case = namedtuple("Case", "id r c tr ld off sentinel gen seed every")


def _cases():
    out = []

    def add(r, c, tr, gen, ld=None, off=0, sentinel=False, every=False):
        w = r if tr else c
        cid = f"{r}x{c}{'T' if tr else ''}-ld{ld or w}+{off}-{gen}"
        out.append(Case(cid, r, c, tr, ld or w, off, sentinel, gen, 1000 + len(out), every))

    # 1-3: every shift, random int8
    add(8192, 8192, False, "uniform", every=True)
    add(8192, 8192, True, "uniform", every=True)
    add(8191, 8191, False, "uniform", every=True)                                   # ld = 8191: every row at another alignment
    add(8191, 8191, True, "uniform", ld=8208, off=3, sentinel=True, every=True)      # a ragged view inside a larger buffer
    k = 0

    def rot():
        nonlocal k
        k += 1
        return ROTATION[(k - 1) % len(ROTATION)]

    # 4: the plan's edges
    for r, c in [(4096, 4096), (4096, 4097), (4097, 4096), (8192, 1), (1, 8192), (8191, 1), (1, 1)]:
        for tr in (False, True):
            add(r, c, tr, rot())
    # 5: tile edges; every other one at a base offset inside a sentinel buffer
    offs = iter([1, 2, 4, 8])
    for n5, (r, c) in enumerate([(r, c) for r in (127, 128, 129) for c in (255, 256, 257)]):
        tr = (n5 // 2) % 2 == 1
        if n5 % 2:
            add(r, c, tr, rot(), ld=(r if tr else c) + 5, off=next(offs), sentinel=True)
        else:
            add(r, c, tr, rot())
    # 6: row tails
    for t in range(1, 18):
        add(100, 384 + t, False, rot())
    for t in (1, 5, 15, 16, 17):
        add(384 + t, 100, True, rot())
    return out


CASES = _cases()
EDGE_CASES = [cs for cs in CASES if not cs.every]


@functools.lru_cache(maxsize=None)
def stored(cs):
    """the matrix as stored: c x r when transposed, else r x c"""
    shape = (cs.c, cs.r) if cs.tr else (cs.r, cs.c)
    return GENERATORS[cs.gen](shape, cs.seed)


def logical(cs):
    s = stored(cs)
    return s.T if cs.tr else s


def buffer(cs):
    """the bytes to upload: the stored matrix at byte `off`, rows `ld` apart; SENTINEL everywhere else"""
    s = stored(cs)
    rows, w = s.shape
    if not cs.sentinel:
        assert cs.ld == w and cs.off == 0
        return np.ascontiguousarray(s)
    buf = np.full(cs.off + rows * cs.ld + 64, SENTINEL, dtype=np.int8)
    np.lib.stride_tricks.as_strided(buf[cs.off:], shape=(rows, w), strides=(cs.ld, 1))[:] = s
    return buf


def boundary_shifts(cs):
    """the shifts next to the plan's edges, the giant-step and tile boundaries, and the last two"""
    want = [cs.r - 1, cs.r, SLOTS - cs.c, SLOTS - cs.c + 1, 90, 91, 127, 128, 8190, 8191]
    return sorted({s for s in want if 0 <= s < SLOTS})


def tiles(cs):
    """the 128-shift tiles checked on an edge case: those of shifts 0, r - 1, r, 8192 - c, 8192 - c + 1, 8191, the middle of each run and of the gap"""
    pts = [0, cs.r - 1, cs.r, SLOTS - cs.c, SLOTS - cs.c + 1, SLOTS - 1]
    rs = runs(cs.r, cs.c)
    pts += [(lo + hi - 1) // 2 for lo, hi in rs]
    gap = missing(cs)
    if gap:
        pts.append((gap[0] + gap[1] - 1) // 2)
    return sorted({p // TILE for p in pts if 0 <= p < SLOTS})


def missing(cs):
    """the gap [lo, hi) of shifts that do not exist, or None"""
    if cs.r + cs.c > SLOTS:
        return None
    return (cs.r, SLOTS - cs.c + 1)


def checked_shifts(cs):
    if cs.every:
        return list(range(SLOTS))
    return [t * TILE + s for t in tiles(cs) for s in range(TILE)]


def load_paths(cs):
    """which of k_skew's load paths the case takes: "b16" (nvalid >= 16 && 16-byte aligned), "b4" (nvalid >= 4 && 4-byte aligned), "bytes" (neither).
    A stored row is read in 16-byte pieces at multiples of 16 from its start; nvalid is what is left of the row."""
    rows, w = (cs.c, cs.r) if cs.tr else (cs.r, cs.c)
    paths = set()
    for i in range(min(rows, 16)):                      # the alignment of a row start has a period that divides 16
        for p in range(0, w, 16):
            addr, nvalid = cs.off + i * cs.ld + p, w - p
            if nvalid >= 16 and addr % 16 == 0:
                paths.add("b16")
                continue
            for q in range(4):
                nv = nvalid - 4 * q
                if nv <= 0:
                    break
                paths.add("b4" if nv >= 4 and (addr + 4 * q) % 4 == 0 else "bytes")
    return paths
