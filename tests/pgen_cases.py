"""Directed .pgen files at the decoder's record, difflist and header boundaries, shared by the CPU test of the oracle (test_pgen_edges.py) and the device test
(test_gpu_pgen_edges.py).  Every file is written by tests/pgen_writer.py from a code matrix; that matrix (3 -> -1) is the ground truth of both tests, so the device
decoder and the CPU oracle are each held to the writer's statement of the specification, not to each other.

A case is built on first use and kept (`get(name)`): image, code matrix, vrtypes and the variant windows [v0, v1) to decode besides the whole file.
"""
import functools

import numpy as np

import pgen_writer as pw

LOHI = sorted(pw.TYPE1_CODE_BYTES)                       # the six legal type-1 code bytes 1, 2, 3, 5, 6, 9
TAILS = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65)
IDWIDTH = (255, 256, 257, 65535, 65536, 65537, (1 << 24) - 1, 1 << 24)
DIFF_LENGTHS = (0, 1, 63, 64, 65, 128, 129)
BLOCK = 65536


class Case:
    def __init__(self, name, img, codes, vrt, windows=(), diff=None):
        self.name, self.img, self.codes, self.vrt, self.diff = name, img, codes, np.asarray(vrt, dtype=np.uint8), diff or {}
        self.nv, self.ns = codes.shape
        self.windows = [(int(a), int(b)) for a, b in windows]

    def want(self, v0=0, v1=None, rows=None, cols=None):
        """[samples][variants of [v0, v1)] int8, missing = -1, under optional boolean filters"""
        c = self.codes[v0:self.nv if v1 is None else v1]
        if cols is not None:
            c = c[np.asarray(cols, dtype=bool)]
        if rows is not None:
            c = c[:, np.asarray(rows, dtype=bool)]
        return np.where(c == 3, -1, c).astype(np.int8).T

    def counts(self, keep=None):
        """plink2 --geno-counts layout [6][nv]: hom ref, het, hom alt, 0, 0, missing over the kept samples"""
        c = self.codes if keep is None else self.codes[:, np.asarray(keep, dtype=bool)]
        out = np.zeros((6, self.nv), dtype=np.uint32)
        for code, row in ((0, 0), (1, 1), (2, 2), (3, 5)):
            out[row] = (c == code).sum(axis=1)
        return out


def spread_ids(ns, n, rnd):
    """n ascending ids of [0, ns) that contain 0 and ns - 1 (n >= 2), the rest drawn uniformly"""
    if n == 0:
        return np.zeros(0, dtype=np.int64)
    if n == 1:
        return np.array([ns - 1], dtype=np.int64)
    mid = rnd.choice(ns - 2, n - 2, replace=False) + 1 if n > 2 else np.zeros(0, dtype=np.int64)
    return np.sort(np.concatenate([[0, ns - 1], mid])).astype(np.int64)


def row_for(t, ns, ids, rnd, base=None, lohi=None):
    """a row that a type-t record with the difflist `ids` decodes to: arbitrary codes at the ids, the underlying vector elsewhere"""
    if t == 1:
        lo, hi = lohi
        row = np.where(rnd.random(ns) < 0.4, hi, lo).astype(np.uint8)
    elif t in (4, 6, 7):
        row = np.full(ns, t & 3, dtype=np.uint8)
    else:
        row = (pw.invert(base) if t == 3 else base).copy()
    row[ids] = rnd.integers(0, 4, len(ids))
    return row


class Builder:
    """collects variants; LD records take the last non-LD row as their base"""

    def __init__(self, ns, seed):
        self.ns, self.rnd, self.rows, self.vrt, self.diff, self.base = ns, np.random.default_rng(seed), [], [], {}, None

    def add(self, t, ids=None, lohi=None, row=None):
        """type t with the difflist ids (None: type 0, a random row; or the difflist the row implies)"""
        if row is None:
            if t == 0:
                row = self.rnd.integers(0, 4, self.ns).astype(np.uint8)
            else:
                if t == 1 and lohi is None:
                    lohi = LOHI[len(self.rows) % 6]
                row = row_for(t, self.ns, ids, self.rnd, self.base, lohi)
        v = len(self.rows)
        if ids is not None:
            self.diff[v] = (np.asarray(ids, dtype=np.int64), lohi) if t == 1 else np.asarray(ids, dtype=np.int64)
        self.rows.append(np.asarray(row, dtype=np.uint8)); self.vrt.append(t)
        if t not in (2, 3):
            self.base = self.rows[-1]
        return v

    def case(self, name, windows=(), **opts):
        codes = np.stack(self.rows)
        img = pw.write_pgen(codes, self.vrt, difflists=self.diff, **opts)
        return Case(name, img, codes, self.vrt, windows, self.diff)


# ---------------------------------------------------------------------------------------------------------------- tails
def tails(ns):
    """every main type at a sample count around the 4-, 8- and 16-sample units of the row; the difflists hold sample 0 and sample ns - 1; all six type-1 code bytes"""
    b = Builder(ns, 1000 + ns)
    ends = np.unique([0, ns - 1])
    b.add(0)
    for lohi in LOHI:
        b.add(1, ends, lohi)
    for t in (4, 6, 7):
        b.add(t, ends)
        b.add(2, ends); b.add(3, ends)
    b.add(1, np.arange(ns), (0, 2))                       # every sample listed
    b.add(3, np.zeros(0, dtype=np.int64))                 # the inverse of a base and nothing else: padding codes become 2 before the mask clears them
    b.add(7, np.arange(ns))
    b.add(0); b.add(2, ends[-1:])
    nv = len(b.rows)
    return b.case(f"tails-{ns}", windows=[(1, 4), (nv - 1, nv)], wmode=ns % 8)


# ---------------------------------------------------------------------------------------------------------------- idwidth
def idwidth(ns):
    """both sides of each switch of the sample-id width (1 | 2 | 3 | 4 bytes), difflists of 0, 1, 63, 64, 65, 128 and 129 entries.  At 2^24 - 1 and 2^24 a row is
    4 MiB: four variants each, which between them hold the lengths 0, 1, 63, 64, 65, 128, 129 once more"""
    b = Builder(ns, 2000 + ns % 1000)
    ids = lambda n: spread_ids(ns, n, b.rnd)
    if ns < (1 << 24) - 1:
        for k, n in enumerate(DIFF_LENGTHS):
            b.add((4, 6, 7)[k % 3], ids(n))
            b.add(2 + k % 2, ids(DIFF_LENGTHS[(k + 3) % 7]))
            b.add(1, ids(n))
        wins = [(2, 5), (13, 15)]
    elif ns == (1 << 24) - 1:
        b.add(4, ids(128)); b.add(3, ids(63)); b.add(1, ids(129)); b.add(2, ids(0))
        wins = [(1, 2), (3, 4)]
    else:
        b.add(6, ids(129)); b.add(2, ids(1)); b.add(1, ids(65)); b.add(3, ids(64))
        wins = [(1, 2), (3, 4)]
    return b.case(f"idwidth-{ns}", windows=wins, wmode=6)


# ---------------------------------------------------------------------------------------------------------------- deltas
def deltas_ids():
    """197 ids below 2^24: a full first group whose deltas take 1, 2, 2, 3, 3 and 4 bytes (then 57 of one byte: 72 delta bytes, size byte 9), two full groups
    whose 63 deltas all take 3 bytes (size byte 126), a last group of 5 entries"""
    ids = [0]
    for d in (127, 128, 16383, 16384, 2097151, 2097152) + (1,) * 57:
        ids.append(ids[-1] + d)
    for g in range(2):
        ids.append(ids[-1] + 70000 + g)
        for k in range(63):
            ids.append(ids[-1] + 16384 + 1000 * k)
    ids.append(ids[-1] + 5)
    for d in (1, 300, 20000, 2100000):
        ids.append(ids[-1] + d)
    assert len(ids) == 197 and ids[-1] < (1 << 24)
    return np.array(ids, dtype=np.int64)


def deltas():
    ns = 1 << 24
    b = Builder(ns, 31)
    ids = deltas_ids()
    b.add(4, ids); b.add(2, ids[60:140]); b.add(1, ids)
    return b.case("deltas", windows=[(1, 3)], wmode=3)


# ---------------------------------------------------------------------------------------------------------------- groups
def groups():
    """difflists of 256, 256 + 1 and 512 + 1 groups: one thread decodes one group, so the second and third pass of the 256-thread loop"""
    ns = 40000
    b = Builder(ns, 41)
    for n in (16384, 16385, 32769):
        b.add(4, spread_ids(ns, n, b.rnd))
        b.add(1, spread_ids(ns, n, b.rnd))
        b.add(2, spread_ids(ns, n, b.rnd))
    return b.case("groups", windows=[(2, 3), (5, 9)], wmode=7)


def groups_all():
    ns = 129
    b = Builder(ns, 42)
    for t in (4, 1, 2, 3, 6, 7):
        b.add(t, np.arange(ns))
    return b.case("groups-all-129", windows=[(2, 4)], wmode=4)


# ---------------------------------------------------------------------------------------------------------------- ld
def ld():
    """a run of LD-compressed records over each kind of base; windows start at every variant"""
    ns = 70
    b = Builder(ns, 51)
    some = lambda n: np.sort(b.rnd.choice(ns, n, replace=False))
    none = np.zeros(0, dtype=np.int64)
    b.add(0); b.add(2, some(9)); b.add(3, some(3))
    b.add(1, some(5), (1, 3))                              # a base of 1s and 3s (and five others): the inversion of the type-3 record below must leave them alone
    b.add(3, none); b.add(2, none); b.add(3, some(66))
    b.add(4, some(7)); b.add(3, some(1)); b.add(2, some(65))
    b.add(6, none); b.add(2, some(64)); b.add(3, np.arange(ns)); b.add(2, none)
    b.add(7, some(2)); b.add(3, none); b.add(2, some(11))  # the file ends in an LD record
    nv = len(b.rows)
    assert [t for t in b.vrt if t not in (2, 3)] == [0, 1, 4, 6, 7] and nv == 17
    return b.case("ld", windows=[(v, min(nv, v + 3)) for v in range(nv)] + [(nv - 1, nv)], wmode=5)


def single():
    b = Builder(19, 52)
    b.add(1, np.array([0, 18]), (0, 3))
    return b.case("single-variant", windows=[(0, 1)], wmode=0)


# ---------------------------------------------------------------------------------------------------------------- blocks
def blocks(variant):
    """65 536 + 71 variants of 5 samples: two header blocks, the second with an odd count of 4-bit vrtypes.  An LD run ends at variant 65 535, variant 65 536 is its
    own base and an LD run over it starts at 65 537."""
    ns, nv = 5, BLOCK + 71
    rnd = np.random.default_rng(61)
    codes = rnd.integers(0, 4, (nv, ns)).astype(np.uint8)
    vrt = np.zeros(nv, dtype=np.uint8)
    for v in range(1, nv, 97):                             # difflist records throughout, so that a wrong table offset shows everywhere
        vrt[v] = (4, 6, 7, 1)[(v // 97) % 4]
        if vrt[v] != 1:
            codes[v] = vrt[v] & 3
            codes[v, v % ns] = (v // 7) % 4
    vrt[BLOCK - 3], vrt[BLOCK], vrt[nv - 2] = 1, 6, 0
    codes[BLOCK] = [2, 2, 1, 2, 3]
    for v, t, b in ((BLOCK - 2, 2, BLOCK - 3), (BLOCK - 1, 3, BLOCK - 3), (BLOCK + 1, 3, BLOCK), (BLOCK + 2, 2, BLOCK), (nv - 1, 2, nv - 2)):
        vrt[v] = t
        codes[v] = codes[b] if t == 2 else pw.invert(codes[b])
        codes[v, v % ns] = (codes[v, v % ns] + 1) % 4
    opts = {"4bit": dict(wmode=1), "8bit": dict(wmode=4), "acgap": dict(wmode=2, ac_bytes=2, nonref=3, gap_blocks=37)}[variant]
    img = pw.write_pgen(codes, vrt, **opts)
    return Case(f"blocks-{variant}", img, codes, vrt, [(BLOCK - 6, BLOCK + 9), (BLOCK - 1, BLOCK), (BLOCK, BLOCK + 1), (BLOCK + 1, BLOCK + 3), (nv - 1, nv)])


# ---------------------------------------------------------------------------------------------------------------- headers
def headers(wmode):
    """every width mode, with a record whose length needs all the mode's length bytes: 255 bytes (1-byte lengths), 256 and 65 535 (2-byte), 65 537 (3- and 4-byte:
    a type-0 record of 262 145 samples); each allele-count width, each nonref value, and a gap before the first record"""
    lb = (wmode & 3) + 1
    ns = {1: 1020, 2: 262140}.get(lb, 262145)
    b = Builder(ns, 70 + wmode)
    b.add(0); b.add(4, spread_ids(ns, 70, b.rnd)); b.add(3, spread_ids(ns, 3, b.rnd)); b.add(1, spread_ids(ns, 65, b.rnd)); b.add(0)
    if lb == 2:                                            # a 256-byte record beside the 65 535-byte one: 1 + 2 * 3 + 1 + 28 + 110 * 2 bytes
        ids = np.arange(112) * 2000
        v = b.add(7, ids)
        assert len(pw.record(b.rows[v], 7, None, ns, ids)) == 256
    assert len(pw.pack2(b.rows[0])) == {1: 255, 2: 65535}.get(lb, 65537)
    return b.case(f"headers-{wmode}", windows=[(1, 4)], wmode=wmode, ac_bytes=wmode & 3, nonref=(1, 2, 3, 0, 3, 2, 1, 0)[wmode], gap_first=(0, 5, 64, 1)[wmode & 3])


# ---------------------------------------------------------------------------------------------------------------- tracks
def tracks(wmode):
    """bytes after the main track of every record type, announced by the vrtype bits 0x10 (phase), 0x20 (dosage) and 0x60 (dosage + its phase): to be skipped"""
    ns = 37
    b = Builder(ns, 80 + wmode)
    tr = {}
    for k, bits in enumerate((0x10, 0x20, 0x60)):
        for t in (0, 1, 2, 3, 4, 2, 6, 3, 7):
            ids = None if t == 0 else spread_ids(ns, (0, 2, 5, 36)[(k + t) % 4], b.rnd)
            v = b.add(t, ids)
            tr[v] = (bits, 1 + (3 * v) % 11)
    return b.case(f"tracks-{wmode}", windows=[(2, 6), (12, 20)], wmode=wmode, tracks=tr)


# ---------------------------------------------------------------------------------------------------------------- fixed
def fixed(ns):
    nv = 11
    codes = np.random.default_rng(90 + ns).integers(0, 4, (nv, ns)).astype(np.uint8)
    return Case(f"fixed-{ns}", pw.write_fixed(codes), codes, np.zeros(nv, dtype=np.uint8), [(3, 8), (10, 11)])


BUILDERS = {}
BUILDERS.update({f"tails-{ns}": functools.partial(tails, ns) for ns in TAILS})
BUILDERS.update({f"idwidth-{ns}": functools.partial(idwidth, ns) for ns in IDWIDTH})
BUILDERS.update({"deltas": deltas, "groups": groups, "groups-all-129": groups_all, "ld": ld, "single-variant": single})
BUILDERS.update({f"blocks-{k}": functools.partial(blocks, k) for k in ("4bit", "8bit", "acgap")})
BUILDERS.update({f"headers-{m}": functools.partial(headers, m) for m in range(8)})
BUILDERS.update({f"tracks-{m}": functools.partial(tracks, m) for m in (4, 5, 6, 7)})
BUILDERS.update({f"fixed-{ns}": functools.partial(fixed, ns) for ns in (1, 4, 5, 13, 64)})
NAMES = list(BUILDERS)


@functools.lru_cache(maxsize=None)
def get(name):
    c = BUILDERS[name]()
    assert c.name == name
    return c


def filters(case, v0, v1, seed=7):
    """a random row and column filter for the window [v0, v1) that keep at least one sample and one variant, the last sample among them every other time"""
    rnd = np.random.default_rng(seed + case.ns + v0)
    rf = rnd.random(case.ns) < 0.6
    cf = rnd.random(v1 - v0) < 0.6
    rf[rnd.integers(0, case.ns)] = True; cf[rnd.integers(0, v1 - v0)] = True
    return rf, cf


def keep_mask(case, seed=9):
    """a keep mask whose last kept sample is ns - 1"""
    k = np.random.default_rng(seed + case.ns).random(case.ns) < 0.5
    k[case.ns - 1] = True
    return k


# ---------------------------------------------------------------------------------------------------------------- files to refuse
def _le(x, n):
    return np.frombuffer(int(x).to_bytes(n, "little"), dtype=np.uint8)


def _with_record(t, rec):
    """a good five-variant file of 100 samples whose variant 2 (variant 0 for an LD type) is the type-t record `rec`"""
    b = Builder(100, 95)
    b.add(0); b.add(4, np.array([3, 50, 99])); b.add(6, np.array([7])); b.add(2, np.array([1, 2])); b.add(1, np.arange(0, 100, 3), (0, 1))
    v = 0 if t in (2, 3) else 2
    vrt = list(b.vrt); vrt[v] = t
    return pw.write_pgen(np.stack(b.rows), vrt, wmode=5, ac_bytes=1, nonref=3, difflists=b.diff, raw={v: rec})


def _good():
    return _with_record(6, pw.difflist(np.array([7]), np.array([1]), 100))


def _type1(code):
    return _with_record(1, bytes([code]) + bytes(13) + pw.varint(0))


def _edit(img, at, data):
    img = img.copy(); img[at:at + len(data)] = data
    return img


def _unterminated():
    d = bytearray(pw.difflist(np.array([0, 5, 9]), np.array([1, 1, 1]), 100))
    d[-1] |= 0x80                                          # the last delta announces a byte that the record does not have
    return _with_record(4, bytes(d))


# name -> (image, what the device's message must say).  Every one is refused on the host or by a bounds check of k_pgen_decode BEFORE the read it guards:
# the kernel reads record bytes only below `end` (pg_varint, the length checks of types 0 and 1, sh_delta <= end ahead of the group table and the values).
MALFORMED = {
    "block-offset-below-the-header-end": lambda: (_edit(_good(), 12, _le(pw.header_end(_good()) - 1, 8)), "block 0 starts"),
    "block-offset-past-the-file": lambda: (_edit(_good(), 12, _le(len(_good()) + 1, 8)), "block 0 starts"),
    "record-past-the-file": lambda: (_good()[:-1].copy(), "past the end"),
    "nv-too-large-for-the-file": lambda: (_edit(_good(), 3, _le(0xFFFFFFF0, 4)), "do not fit the file"),
    "no-variants": lambda: (_edit(_good(), 3, _le(0, 4)), "empty file"),
    "no-samples": lambda: (_edit(_good(), 7, _le(0, 4)), "empty file"),
    "width-mode-8": lambda: (_edit(_good(), 11, _le(0x58, 1)), "control byte"),
    "storage-mode-0x01": lambda: (_edit(_good(), 2, _le(0x01, 1)), "storage mode"),
    "storage-mode-0x11": lambda: (_edit(_good(), 2, _le(0x11, 1)), "storage mode"),
    "record-type-5": lambda: (_with_record(5, pw.varint(0)), "type 5"),
    "type-1-code-byte-0": lambda: (_type1(0), "malformed variant record"),
    "type-1-code-byte-4": lambda: (_type1(4), "malformed variant record"),
    "type-1-code-byte-7": lambda: (_type1(7), "malformed variant record"),
    "difflist-longer-than-the-samples": lambda: (_with_record(4, pw.varint(101) + bytes(60)), "malformed variant record"),
    "first-sample-id-at-ns": lambda: (_with_record(7, pw.difflist(np.array([100]), np.array([1]), 100)), "malformed variant record"),
    "delta-reaches-ns": lambda: (_with_record(7, pw.difflist(np.array([98, 100]), np.array([1, 2]), 100)), "malformed variant record"),
    "group-table-past-the-record": lambda: (_with_record(4, pw.varint(100) + bytes(2)), "malformed variant record"),
    "unterminated-delta": lambda: (_unterminated(), "malformed variant record"),
    "unterminated-length": lambda: (_with_record(6, b"\xff\xff"), "malformed variant record"),
    "truncated-fixed-width-file": lambda: (pw.write_fixed(np.ones((4, 9), dtype=np.uint8))[:-1].copy(), "truncated fixed-width"),
    "ld-compressed-first-variant": lambda: (_with_record(2, pw.varint(0)), "first variant is LD-compressed"),
}
NOT_FOR_THE_ORACLE = {"nv-too-large-for-the-file"}       # the oracle's index allocates by the header's variant count


def malformed(name):
    return MALFORMED[name]()
