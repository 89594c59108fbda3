"""Test-side reference for the hybrid key switch's basis extension (csrc/ksw.hpp ext_prepare / ext_target, the oracle's basis_extend)
and the modulus chains that pin it beyond PN14.

Four things, none of which touches the GPU by itself:
  * the chains S1 / S3 / S4 (np = 1, 3, 4) with the predicate ARM(q) that says whether canon()'s equality fix-up is reachable for q;
  * ext_model(): y_m, the float correction v computed as the kernel and the oracle compute it (IEEE division, summed in modulus order,
    truncated) and the exact floor by Fraction - the only source of the classes v_float - v_exact in {-1, 0, +1};
  * keyswitch_model(): orc_keyswitch restated with Python integers around ext_model (the transforms are the oracle's, pinned elsewhere);
  * the directed inputs both GPU files use, and one context + oracle ring per chain shared by the GPU files (gpu_env).
"""
import atexit
import ctypes as C
from fractions import Fraction
from math import prod

import numpy as np

import oracle_lib as ol

N = 1 << 14


def ARM(q):
    """canon(x, q) computes floor(fl(x * fl(1/q))): for x = k q that product can fall below k only if fl(q * fl(1/q)) < 1 - then the exact
    remainder is q and the equality fix-up fires.  For every other modulus the fix-up is dead code at k = 1."""
    return float(q) * (1.0 / float(q)) < 1.0


def canon_model(x, q, fixup=True):
    """common.hpp canon() on the integer x, |x| < 2^51: the floor of the rounded product, the exact remainder (the fma's result is an integer
    in [0, q], so it is not rounded), the equality fix-up.  fixup=False is canon_le()."""
    import math
    r = x - math.floor(float(x) * (1.0 / float(q))) * q
    return 0 if fixup and r == q else r


# name -> (q, p, levels the GPU parity runs at)
S1 = ([0x7fffb0001, 0x7fff80001, 0x800280001, 0x7ffd80001, 0x7ffc80001, 0x7ff9c0001, 0x800008001, 0x8000f8001, 0x800250001],
      [0x80000050001], [7, 1, 0])
S3 = ([0x7fffb0001] + ol.Q_PN14[1:7], ol.P_PN14 + [0x7ffffffc8001], [6, 4, 1, 0])
S4 = ([0x7fffffda0001, 0x7fffffc48001, 0x7ffffffc8001, 0x7ffffff00001, 0x7fffffe70001, 0x7fffffe48001, 0x7fffffe40001, 0x7fffffd08001],
      [0x7fffffc80001, 0x7fffffc18001, 0x7fffffbc0001, 0x7fffffbb8001], [7, 5, 2, 0])
CHAINS = {"S1": S1, "S3": S3, "S4": S4}
ARM_INDICES = {"S1": [0], "S3": [0], "S4": [0, 1]}           # the ARM moduli of each chain's q (asserted by test_ksw_ref.py)


def digits(nq_level, alpha):
    """modulus indices of every digit at a level: ceil((level + 1) / alpha) runs of alpha, the last one short"""
    nl = nq_level + 1
    return [list(range(s, min(s + alpha, nl))) for s in range(0, nl, alpha)]


# ---------------------------------------------------------------- the extension in Python integers
def ext_model(xs, qs, recip=False):
    """(y, v_float, v_exact) of one digit word: xs[m] = X mod qs[m].  recip=True is the MISTAKE y * fl(1/q) in place of y / q."""
    D = prod(qs)
    y = [x * pow(D // q, -1, q) % q for x, q in zip(xs, qs)]
    vf = 0.0
    for ym, q in zip(y, qs):
        vf += float(ym) * (1.0 / float(q)) if recip else float(ym) / float(q)
    exact = sum(Fraction(ym, q) for ym, q in zip(y, qs))
    return y, int(vf), exact.numerator // exact.denominator


def ext_value(y, v, qs, qt):
    """the extension's residue at target qt for correction v: sum y_m (D / q_m) - v D"""
    D = prod(qs)
    return (sum(ym * (D // q) for ym, q in zip(y, qs)) - v * D) % qt


def basis_extend_model(rows, qs, qt):
    """rows[m][x] coefficient-domain residues of a digit -> the row at target qt, as the oracle's basis_extend defines it"""
    n = len(rows[0])
    if len(qs) == 1:
        return [int(rows[0][x]) % qt for x in range(n)]
    out = []
    for x in range(n):
        y, vf, _ = ext_model([int(r[x]) for r in rows], qs)
        out.append(ext_value(y, vf, qs, qt))
    return out


def keyswitch_model(ring, level, cx, key):
    """orc_keyswitch in Python integers: cx [level+1][N] NTT rows, key [beta][2][nmod][N] -> (d0, d1) [level+1][N]"""
    nq, np_, n = ring.nq, ring.np_, ring.N
    nl, mods = level + 1, ring.moduli
    c2 = [ring.intt(m, cx[m]) for m in range(nl)]
    tmod = list(range(nl)) + [nq + p for p in range(np_)]
    acc = [[[0] * n for _ in tmod] for _ in range(2)]
    for i, dg in enumerate(digits(level, np_)):
        qs = [mods[m] for m in dg]
        for t, mod in enumerate(tmod):
            qt = mods[mod]
            if mod in dg:
                e = [int(v) for v in cx[mod]]
            else:
                e = ring.ntt(mod, np.array(basis_extend_model([c2[m] for m in dg], qs, qt), dtype=np.uint64))
            for pl in range(2):
                k = key[i, pl, mod]
                acc[pl][t] = [(a + int(ev) * int(kv)) % qt for a, ev, kv in zip(acc[pl][t], e, k)]
    out = []
    ps = [mods[nq + p] for p in range(np_)]
    P = prod(ps)
    for pl in range(2):
        rows = [ring.intt(nq + p, np.array(acc[pl][nl + p], dtype=np.uint64)) for p in range(np_)]
        d = []
        for t in range(nl):
            qt = mods[t]
            ext = ring.ntt(t, np.array(basis_extend_model(rows, ps, qt), dtype=np.uint64))
            pinv = pow(P % qt, -1, qt)
            d.append([(a - int(e)) * pinv % qt for a, e in zip(acc[pl][t], ext)])
        out.append(np.array(d, dtype=np.uint64))
    return out[0], out[1]


# ---------------------------------------------------------------- directed inputs
SMALL = [0, 1, -1, 2, -2, 5, -5, 12345, -12345, 12, -12, 17, -17, 22, -22]


def directed_values(q, alpha, level):
    """the signed integers whose residues put every digit's extension on the float boundary: 0, +-1, +-2, +-5, +-12345 (X = D - k rounds the
    float sum up, X = k can round it down), +-12, +-17, +-22 (the smallest words that round it down on the digits of S3 and S4 where none of
    the former does), each digit's D // 2 and D // 2 + 1 (the generic class 0), and each ARM modulus itself - the one
    word < q_src that is a non-zero multiple of an ARM target, which is what a single-prime digit's raw copy has to reduce to 0"""
    vals = list(SMALL)
    for dg in digits(level, alpha):
        D = prod(q[m] for m in dg)
        vals += [D // 2, D // 2 + 1]
    vals += [qm for qm in q[:level + 1] if ARM(qm)]
    return vals


def directed_rows(moduli, vals, n=N, shift=0):
    """coefficient-domain residue rows [len(moduli)][n] of the cycle vals[(x + shift) % len(vals)]"""
    idx = (np.arange(n) + shift) % len(vals)
    return np.stack([np.array([v % qm for v in vals], dtype=np.uint64)[idx] for qm in moduli])


def directed_ct(ring, level, seed, ones=False):
    """a ciphertext [2][level+1][N] whose polynomial 1 is the NTT of the directed cycle (polynomial 0 uniformly random);
    ones=True: polynomial 1 is all ones instead - the NTT of the constant 1, the tensor partner that keeps a1 * b1 directed"""
    ct = ring.fill_uniform(level, seed)
    if ones:
        ct[1] = 1
        return ct
    rows = directed_rows(ring.moduli[:level + 1], directed_values(ring.moduli[:ring.nq], ring.np_, level), ring.N, shift=seed)
    for m in range(level + 1):
        ct[1, m] = ring.ntt(m, rows[m])
    return ct


def classify(q, alpha, level, recip=False):
    """per digit of the level: {directed value index: v_float - v_exact} (None for a single-prime digit); recip=True: v_float of the mistake"""
    vals = directed_values(q, alpha, level)
    out = []
    for dg in digits(level, alpha):
        if len(dg) == 1:
            out.append(None)
            continue
        qs = [q[m] for m in dg]
        cls = {}
        for k, c in enumerate(vals):
            _, vf, ve = ext_model([c % qm for qm in qs], qs, recip)
            cls[k] = vf - ve
        out.append(cls)
    return out


def automorphism_index(ring, g):
    idx = np.zeros(ring.N, dtype=np.uint32)
    ol.lib().orc_automorphism_index(ring.h, int(g), idx.ctypes.data_as(C.POINTER(C.c_uint32)))
    return idx


# ---------------------------------------------------------------- one context and oracle ring per chain, shared by the GPU files
_ENV = {}


def gpu_env(name):
    """(context, ring) of a chain - or of "PN14" -, made at first use and kept for the session: creating a context costs more than any test here"""
    if name not in _ENV:
        from sfgwas_amd import capi
        q, p = (ol.Q_PN14, ol.P_PN14) if name == "PN14" else CHAINS[name][:2]
        _ENV[name] = (capi.Context(q, p), ol.Ring(14, q, p))
    return _ENV[name]


@atexit.register
def _close_all():
    for ctx, _ in _ENV.values():
        ctx.close()
    _ENV.clear()
