"""Test-side WRITER of PLINK 2 .pgen files (storage modes 0x10 and 0x02), written independently of the decoders from the published PGEN
specification (plink-ng 2.0 pgenlib, pgen_spec): lets the tests produce every main-track record type - the reference's example data only
contains types 0 and 1 - with difflists of several groups, all header width modes and LD-compressed runs.  Self-consistency only: the
types the reference data does not use stay "parity unpinned" (DESIGN.md).

Beyond the matrix-driven path (`write_pgen(codes, vrtypes)`), a test can direct what the format leaves open:
  * the difflist of a record (`difflists`): the sample ids it lists - entries that repeat the underlying value are legal - and, for type 1, which
    two codes the bit array distinguishes; the writer checks that the record still decodes to the row of the matrix;
  * the header: allele-count bytes, the nonref flags and their bit array, a gap before the first record and before each later block;
  * bytes after the main track of a record, with the vrtype bits that announce them (`tracks`);
  * a record's bytes outright (`raw`), for files a decoder has to refuse;
  * storage mode 0x02 (`write_fixed`).
"""
import numpy as np


def varint(x):
    out = bytearray()
    while True:
        b = x & 0x7F
        x >>= 7
        if x:
            out.append(b | 0x80)
        else:
            out.append(b)
            return bytes(out)


def pack2(codes):
    c = np.zeros((len(codes) + 3) // 4 * 4, dtype=np.uint8)
    c[:len(codes)] = codes
    c = c.reshape(-1, 4)
    return (c[:, 0] | (c[:, 1] << 2) | (c[:, 2] << 4) | (c[:, 3] << 6)).astype(np.uint8).tobytes()


def id_bytes(ns):
    return (ns.bit_length() - 1) // 8 + 1


def difflist(ids, vals, ns):
    """ids ascending sample indices, vals their 2-bit values"""
    n = len(ids)
    out = bytearray(varint(n))
    if n == 0:
        return bytes(out)
    idb = id_bytes(ns)
    groups = [(ids[k:k + 64], vals[k:k + 64]) for k in range(0, n, 64)]
    deltas = []
    for gi, _ in groups:
        d = bytearray()
        for a, b in zip(gi[:-1], gi[1:]):
            d += varint(int(b) - int(a))
        deltas.append(bytes(d))
    for gi, _ in groups:
        out += int(gi[0]).to_bytes(idb, "little")
    for d in deltas[:-1]:
        assert 0 <= len(d) - 63 < 256
        out.append(len(d) - 63)
    out += pack2(np.asarray(vals, dtype=np.uint8))
    for d in deltas:
        out += d
    return bytes(out)


def invert(codes):
    c = codes.copy()
    c[codes == 0] = 2
    c[codes == 2] = 0
    return c


TYPE1_CODE_BYTES = {(0, 1): 1, (0, 2): 2, (0, 3): 3, (1, 2): 5, (1, 3): 6, (2, 3): 9}        # lo * 4 + (hi - lo): the six a file may hold


def record(codes, vrtype, base, ns, ids=None, lohi=None):
    """the main track of one variant.  ids = None: the difflist holds exactly the samples that differ from the underlying vector (for type 1 the two most
    frequent codes are the bit array's).  ids given: the difflist holds exactly those samples, which must include every one that differs; lohi = (lo, hi) sets
    the two codes of a type-1 bit array."""
    codes = np.asarray(codes, dtype=np.uint8)
    if vrtype == 0:
        assert ids is None
        return pack2(codes)
    if vrtype == 1:
        if lohi is None:
            cnt = np.bincount(codes, minlength=4)
            lo, hi = sorted(np.argsort(-cnt, kind="stable")[:2].tolist())
        else:
            lo, hi = lohi
        bits = np.zeros((ns + 7) // 8 * 8, dtype=np.uint8)
        bits[:ns] = (codes == hi)
        head = bytes([TYPE1_CODE_BYTES[(lo, hi)]]) + np.packbits(bits, bitorder="little").tobytes()
        under, tgt = np.where(codes == hi, hi, lo).astype(np.uint8), codes
    elif vrtype in (4, 6, 7):
        head, under, tgt = b"", np.full(ns, vrtype & 3, dtype=np.uint8), codes
    elif vrtype in (2, 3):
        head, under, tgt = b"", np.asarray(base, dtype=np.uint8), (invert(codes) if vrtype == 3 else codes)
    else:
        raise ValueError(vrtype)
    differ = np.nonzero(tgt != under)[0]
    if ids is None:
        ids = differ
    else:
        ids = np.asarray(ids, dtype=np.int64)
        assert ids.size == 0 or (np.all(np.diff(ids) > 0) and 0 <= ids[0] and ids[-1] < ns), "difflist ids must ascend inside [0, ns)"
        assert np.isin(differ, ids).all(), "the given difflist does not produce the row of the matrix"
    return head + difflist(ids, tgt[ids], ns)


def _filler(n, salt):
    """n bytes, none of them zero"""
    return bytes(1 + (salt * 7 + k * 13) % 255 for k in range(n))


def write_pgen(codes, vrtypes, wmode=7, extra_vrtype_bits=0, difflists=None, ac_bytes=0, nonref=0, gap_first=0, gap_blocks=0, tracks=None, raw=None):
    """codes [nv][ns] in {0,1,2,3}; vrtypes[nv] main-track types; wmode = low nibble of the header control byte.
    difflists: {v: ids} or {v: (ids, (lo, hi))} - see record().  ac_bytes 0..3: allele-count bytes per variant in the header (non-zero filler);
    nonref 0..3: bits 6-7 of the control byte, 3 adds one flag bit per variant.  gap_first / gap_blocks: filler bytes between the header's end and the
    first record / before the first record of every later block.  tracks: {v: (vrtype bits among 0x10..0x40, trailing bytes)} - what a phase or dosage
    track looks like to a hard-call decoder (wmode >= 4).  raw: {v: bytes} replaces the record of v."""
    codes = np.asarray(codes, dtype=np.uint8)
    nv, ns = codes.shape
    difflists, tracks, raw = difflists or {}, tracks or {}, raw or {}
    assert 0 <= ac_bytes <= 3 and 0 <= nonref <= 3 and 0 <= wmode <= 7
    assert not tracks or wmode >= 4, "4-bit vrtypes cannot carry track bits"
    recs, base = [], None
    for v in range(nv):
        t = int(vrtypes[v])
        if v in raw:
            r = bytes(raw[v])
        else:
            d = difflists.get(v)
            ids, lohi = (d if isinstance(d, tuple) else (d, None))
            r = record(codes[v], t, base, ns, ids, lohi)
        if v in tracks:
            r += _filler(tracks[v][1], v)
        recs.append(r)
        if t not in (2, 3):
            base = codes[v]
    lb = (wmode & 3) + 1
    assert all(len(r) < (1 << (8 * lb)) for r in recs)
    nblk = (nv + 65535) // 65536
    hdr_len = 12 + 8 * nblk
    per_blk = []
    for b in range(nblk):
        v0, v1 = b * 65536, min(nv, (b + 1) * 65536)
        vt = [int(vrtypes[v]) | extra_vrtype_bits | (tracks[v][0] if v in tracks else 0) for v in range(v0, v1)]
        if wmode < 4:
            vt = vt + [0] * (len(vt) & 1)
            vb = bytes(vt[k] | (vt[k + 1] << 4) for k in range(0, len(vt), 2))
        else:
            vb = bytes(vt)
        lens = b"".join(len(recs[v]).to_bytes(lb, "little") for v in range(v0, v1))
        tail = _filler((v1 - v0) * ac_bytes, b) + (_filler((v1 - v0 + 7) // 8, b + 100) if nonref == 3 else b"")
        per_blk.append(vb + lens + tail)
        hdr_len += len(per_blk[-1])
    out = bytearray([0x6C, 0x1B, 0x10]) + nv.to_bytes(4, "little") + ns.to_bytes(4, "little") + bytes([wmode | ac_bytes << 4 | nonref << 6])
    pos = hdr_len
    for b in range(nblk):
        pos += gap_blocks if b else gap_first
        out += pos.to_bytes(8, "little")
        pos += sum(len(recs[v]) for v in range(b * 65536, min(nv, (b + 1) * 65536)))
    for pb in per_blk:
        out += pb
    assert len(out) == hdr_len
    for v, r in enumerate(recs):
        if v % 65536 == 0:
            out += _filler(gap_blocks if v else gap_first, v >> 16)
        out += r
    assert len(out) == pos
    return np.frombuffer(bytes(out), dtype=np.uint8).copy()


def header_end(img):
    """the byte after the per-block tables of a mode-0x10 image"""
    nv, ctrl = int(img[3:7].view("<u4")[0]), int(img[11])
    wmode, ac_bytes, nonref = ctrl & 15, (ctrl >> 4) & 3, ctrl >> 6
    p = 12 + 8 * ((nv + 65535) // 65536)
    for b in range(0, nv, 65536):
        cnt = min(65536, nv - b)
        p += ((cnt + 1) // 2 if wmode < 4 else cnt) + cnt * ((wmode & 3) + 1) + cnt * ac_bytes + ((cnt + 7) // 8 if nonref == 3 else 0)
    return p


def write_fixed(codes):
    """storage mode 0x02: a 12-byte header (magic, mode, variant count, sample count, one control byte) and one 2-bit row of ceil(ns / 4) bytes per variant"""
    codes = np.asarray(codes, dtype=np.uint8)
    nv, ns = codes.shape
    out = bytearray([0x6C, 0x1B, 0x02]) + nv.to_bytes(4, "little") + ns.to_bytes(4, "little") + bytes([0x40])
    for v in range(nv):
        out += pack2(codes[v])
    return np.frombuffer(bytes(out), dtype=np.uint8).copy()


def synthetic(nv, ns, seed, types=(0, 1, 2, 3, 4, 6, 7)):
    """a genotype matrix whose variants suit the record types drawn for them (sparse rows for difflists, correlated rows for LD)"""
    rnd = np.random.default_rng(seed)
    codes = np.zeros((nv, ns), dtype=np.uint8)
    vrt = np.zeros(nv, dtype=np.uint8)
    base = None
    for v in range(nv):
        t = int(rnd.choice(types)) if v else int(rnd.choice([x for x in types if x not in (2, 3)] or [0]))
        if t in (2, 3) and base is None:
            t = 0
        if t == 0:
            row = rnd.integers(0, 4, ns)
        elif t == 1:
            row = rnd.choice([0, 1, 2, 3], ns, p=[0.55, 0.38, 0.05, 0.02])
            row = rnd.permutation(4)[row]
        elif t in (4, 6, 7):
            row = np.full(ns, t & 3)
            k = int(rnd.integers(0, max(2, ns // 6)))
            idx = rnd.choice(ns, k, replace=False)
            row[idx] = rnd.integers(0, 4, k)
        else:
            row = base.copy()
            k = int(rnd.integers(0, max(2, ns // 5)))
            idx = rnd.choice(ns, k, replace=False)
            row[idx] = rnd.integers(0, 4, k)
            if t == 3:
                row = invert(row.astype(np.uint8))
        codes[v] = row
        vrt[v] = t
        if t not in (2, 3):
            base = codes[v].copy()
    return codes, vrt
