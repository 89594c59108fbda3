"""The plaintext passes over the genotype matrix, stated in numpy / Python integers - independent of the oracle and of the library:
the count-sketch projection with the column moments (gwas/pca.go:157-160), the column sums (gwas/matmult.go:1292-1303), the 2-bit
packed layout (sfgwas_amd/csrc/genoio.hip) and the PLINK .bed decode with its filters (scripts/plinkBedToBinary.py, filterMatrix.py).
Transpose and concatenation are X.T and np.concatenate and need no statement.  tests/test_genopass_ref.py holds every function here
against literal Python loops and `sketch` against the oracle's C loop; tests/test_gpu_genopasses.py holds the kernels against these.

Go's integer semantics, which the kernels reproduce: uint64(int8) sign-extends, so a negative entry adds 2^64 - |x| and the sum is
taken modulo 2^64; x*x is an int8 product and wraps (12 * 12 = 144 -> -112) BEFORE it is widened."""
import numpy as np

BED_VALUE = np.array([2, -1, 1, 0], dtype=np.int8)              # .bed code 00 -> 2, 01 -> missing, 10 -> 1, 11 -> 0


def _sq_i8(X):
    """x*x as int8 (wrapping), for an int8 array"""
    w = X.astype(np.int16)
    return (w * w).astype(np.uint16).astype(np.uint8).view(np.int8)


def sketch(X, bucket, sgn, kp):
    """(localSketch [kp][ncol] float64, xsum [ncol] uint64, x2sum [ncol] uint64).  The sketch is summed in int64 and is an integer below 2^53
    (|x| <= 128, |sgn| <= 128, fewer than 2^31 rows are far below it), so its float64 is exact whatever order the reference adds in."""
    X = np.asarray(X)
    assert X.dtype == np.int8 and X.ndim == 2
    bucket, sgn = np.asarray(bucket), np.asarray(sgn).astype(np.int64)
    nrow, ncol = X.shape
    assert bucket.shape == (nrow,) and sgn.shape == (nrow,) and bucket.min() >= 0 and bucket.max() < kp
    sk = np.zeros((kp, ncol), dtype=np.int64)
    for b in range(kp):
        for s in np.unique(sgn[bucket == b]):                     # the rows of one bucket and one sign: s times their plain sum
            sk[b] += int(s) * X[(bucket == b) & (sgn == s)].sum(0, dtype=np.int64)
    xsum = X.sum(0, dtype=np.int64).view(np.uint64)               # two's complement: the int64 sum IS the sum of sign-extended words modulo 2^64
    x2sum = _sq_i8(X).sum(0, dtype=np.int64).view(np.uint64)
    assert np.abs(sk).max(initial=0) < 1 << 53
    return sk.astype(np.float64), xsum, x2sum


def colsums(X):
    """(sum [ncol], sqsum [ncol]) float64 after negatives -> 0; the square wraps in int8 before float64()"""
    X = np.asarray(X)
    assert X.dtype == np.int8 and X.ndim == 2
    g = np.where(X < 0, 0, X).astype(np.int8)
    return g.sum(0, dtype=np.int64).astype(np.float64), _sq_i8(g).sum(0, dtype=np.int64).astype(np.float64)


def pack_bytes(X):
    """(image [nrow][4 * ceil(ncol / 16)] uint8, number of entries above 2).  Code = the genotype 0 / 1 / 2, 3 for every negative; an entry above 2 keeps its
    two low bits (the library refuses such a matrix, the count is what its message carries); column c sits in byte c // 4 at bits 2 (c % 4); a row is whole
    dwords, the padding codes are 0."""
    X = np.asarray(X)
    assert X.dtype == np.int8 and X.ndim == 2
    nrow, ncol = X.shape
    ldb = 4 * ((ncol + 15) // 16)
    code = np.zeros((nrow, ldb * 4), dtype=np.uint8)
    code[:, :ncol] = np.where(X < 0, 3, X.astype(np.int16) & 3)
    c = code.reshape(nrow, ldb, 4)
    return (c[:, :, 0] | (c[:, :, 1] << 2) | (c[:, :, 2] << 4) | (c[:, :, 3] << 6)).astype(np.uint8), int((X > 2).sum())


def make_bed(codes):
    """the .bed file (magic + SNP-major packed codes) of codes [nv][ns] in 0..3; the unused bit pairs of each SNP's last byte are set to 1s"""
    codes = np.asarray(codes, dtype=np.uint8)
    nv, ns = codes.shape
    bps = (ns + 3) // 4
    c = np.full((nv, bps * 4), 3, dtype=np.uint8)
    c[:, :ns] = codes
    c = c.reshape(nv, bps, 4)
    body = (c[:, :, 0] | (c[:, :, 1] << 2) | (c[:, :, 2] << 4) | (c[:, :, 3] << 6)).astype(np.uint8)
    return np.concatenate([np.array([0x6C, 0x1B, 0x01], dtype=np.uint8), body.ravel()])


def bed_decode(bed, ns, nv, rowf=None, colf=None):
    """sample-major int8 [kept samples][kept SNPs] of a SNP-major .bed: sample i of SNP j is bit pair i % 4 (low bits first) of byte i // 4 of the SNP's
    ceil(ns / 4) bytes; then the byte filters (nonzero = keep) over samples and SNPs"""
    bed = np.asarray(bed, dtype=np.uint8)
    bps = (ns + 3) // 4
    assert bed.size == 3 + nv * bps and tuple(bed[:3]) == (0x6C, 0x1B, 0x01)
    body = bed[3:].reshape(nv, bps)
    codes = np.stack([(body >> (2 * k)) & 3 for k in range(4)], axis=2).reshape(nv, bps * 4)[:, :ns]
    out = BED_VALUE[codes].T
    if rowf is not None:
        out = out[np.asarray(rowf) != 0]
    if colf is not None:
        out = out[:, np.asarray(colf) != 0]
    return np.ascontiguousarray(out)


# ---- the cases the CPU and the GPU module share (tests/test_genopass_ref.py holds `sketch` against the oracle at exactly these)
# Rows around the sketch kernel's 16384-row chunks (one short of, exactly, one past; a chunk plus a last tile of 63 and of 64 rows; two and four chunks plus
# one row - the last past 2^16 rows in total), each one column and 257 columns wide; the workload's 100 000 rows (7 chunks, the last of 1696 rows = 26 1/2
# tiles) with rows 300 bytes apart, so that most rows start off a 16-byte boundary; and the edges of the 256-column strips.
# What no shape here reaches: the kernel's flush of its int32 partial sums into fp64 after 2^16 rows of ONE workgroup.  A workgroup never sees more than
# one chunk of 16384 rows, so that branch cannot run whatever the matrix; 65 537 rows are four chunks and a row, not one long accumulation.
SKETCH_TALL = list(dict.fromkeys([(r, c) for r in (16383, 16384, 16385, 16384 + 63, 16384 + 64, 32769, 65537) for c in (1, 257)] + [(100_000, 300)] +
                                 [(16385, c) for c in (255, 256, 257, 512 + 16)]))          # (16385, 257) belongs to both lists: once
VALUE_KINDS = ("dosage", "int8", "c127", "cm128", "c11", "c12")
# four consecutive rows of one column = one dword of the moments' dot product: its sum of squares is 127 (fast path), 128 (byte path, nothing wrapped),
# one wrapped square, and four extreme bytes
QUADS = ((11, 2, 1, 1), (8, 8, 0, 0), (12, 0, 0, 0), (-1, -128, 127, 16))


def values(kind, nrow, ncol, seed):
    rnd = np.random.default_rng(seed)
    if kind == "dosage":
        return rnd.integers(-1, 3, (nrow, ncol), dtype=np.int8)
    if kind == "int8":
        return rnd.integers(-128, 128, (nrow, ncol), dtype=np.int8)
    return np.full((nrow, ncol), {"c127": 127, "cm128": -128, "c11": 11, "c12": 12}[kind], dtype=np.int8)


def buckets_signs(nrow, kp, mode, seed, plus_only=False):
    """mode "cycle": bucket i % kp; "equal": every row in the LAST bucket (one bucket takes every row of every chunk: the largest partial sums)"""
    rnd = np.random.default_rng(seed + 7)
    bucket = (np.arange(nrow) % kp if mode == "cycle" else np.full(nrow, kp - 1)).astype(np.int32)
    sgn = np.ones(nrow, dtype=np.int8) if plus_only else rnd.choice(np.array([-1, 1], dtype=np.int8), nrow)
    return bucket, sgn


def quad_rows(nrow):
    """multiples of 4 with the four rows inside the matrix: inside the first 64-row tile, at its end, at the start of the next tile, the last and the first
    dword of a 16384-row chunk, and the last (possibly partial) tile of the matrix"""
    want = [4, 60, 64, 16380, 16384, (nrow - 4) // 4 * 4, ((nrow - 1) // 64 * 64)]
    return sorted({r for r in want if 0 <= r and r + 4 <= nrow})


def put_quads(X):
    """writes the four directed dwords at quad_rows into the first four and the last four columns (a matrix narrower than 8: into column 0, the patterns
    taking turns down the rows); returns X"""
    nrow, ncol = X.shape
    for n, r in enumerate(quad_rows(nrow)):
        if ncol < 8:
            X[r:r + 4, 0] = QUADS[n % 4]
            continue
        for k, q in enumerate(QUADS):
            X[r:r + 4, k] = q
            X[r:r + 4, ncol - 1 - k] = q
    return X


def sketch_case(nrow, ncol, kind="int8", kp=16, mode="cycle", seed=None, quads=True):
    seed = nrow * 1000 + ncol if seed is None else seed
    X = values(kind, nrow, ncol, seed)
    if quads and kind in ("dosage", "int8"):
        put_quads(X)
    bucket, sgn = buckets_signs(nrow, kp, mode, seed, plus_only=kind == "c127")
    return X, bucket, sgn
