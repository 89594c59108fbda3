"""Independent Python-integer statement of the collective key generation (sfgwas_amd/csrc/keygen.hip): the local shares of lattigo v2.1's
CKGProtocol / RTGProtocol / RKGProtocol in the key convention the library's key switch consumes (orc_gen_rotkey / orc_gen_rlk), and the map from a 32-byte seed
to the common reference polynomials on top of tests/encrypt_ref.py's ChaCha20.  tests/test_keygen_ref.py pins this file; tests/test_gpu_keygen.py compares the
library against it.

A `ring` is anything with N, nq, np_, moduli and ntt(mod, coefficients): encrypt_ref.TinyRing (object arrays) or oracle_lib.Ring (uint64 arrays, N = 2^14).
Secrets, errors and the ephemeral u are signed integer COEFFICIENT polynomials; crp and every result are NTT-domain rows [nq+np][N] (object arrays of ints)."""
import numpy as np

import encrypt_ref as er


def _obj(a):
    return np.asarray(a).astype(object)              # Python integers: products of two 47-bit words do not fit 64 bits


def beta_of(ring):
    return (ring.nq + ring.np_ - 1) // ring.np_


def nmod_of(ring):
    return ring.nq + ring.np_


def ntt_small(ring, m, poly):
    """NTT at modulus m of a signed integer polynomial"""
    q = ring.moduli[m]
    red = _obj(poly) % q
    return _obj(ring.ntt(m, red.astype(np.uint64) if ring.N > 64 else red))


def rows_of(ring, poly):
    return [ntt_small(ring, m, poly) for m in range(nmod_of(ring))]


def g_term(ring, digit, m):
    """g_i at modulus m: P mod q_m when m < nq and m // np == i, else 0"""
    if m >= ring.nq or m // ring.np_ != digit:
        return 0
    P = 1
    for p in ring.moduli[ring.nq:]:
        P *= p
    return P % ring.moduli[m]


def automorphism(poly, g, N):
    """phi_g: X^i -> X^(i g mod 2N), with the sign of X^N = -1"""
    out = [0] * N
    for i in range(N):
        e = (i * g) % (2 * N)
        if e < N:
            out[e] += int(poly[i])
        else:
            out[e - N] -= int(poly[i])
    return out


def galois_inverse(g, N):
    return pow(int(g), -1, 2 * N)


def ckg_share(ring, s, crp, e):
    """h = -crp (.) sk + NTT(e)"""
    sk, eh = rows_of(ring, s), rows_of(ring, e)
    return [(-_obj(crp[m]) * sk[m] + eh[m]) % ring.moduli[m] for m in range(nmod_of(ring))]


def rtg_share(ring, s, g, crp, e):
    """one Galois element: crp [beta][nmod][N], e [beta][N] -> h_i = -crp_i (.) phi_{g^-1}(sk) + NTT(e_i) + g_i sk"""
    sk, sg = rows_of(ring, s), rows_of(ring, automorphism(s, galois_inverse(g, ring.N), ring.N))
    out = []
    for i in range(beta_of(ring)):
        eh = rows_of(ring, e[i])
        out.append([(-_obj(crp[i][m]) * sg[m] + eh[m] + g_term(ring, i, m) * sk[m]) % ring.moduli[m] for m in range(nmod_of(ring))])
    return out


def rkg_round1(ring, s, crp, u, e0, e1):
    """h0_i = -NTT(u) (.) crp_i + g_i sk + NTT(e0_i),  h1_i = sk (.) crp_i + NTT(e1_i)"""
    sk, uh = rows_of(ring, s), rows_of(ring, u)
    h0, h1 = [], []
    for i in range(beta_of(ring)):
        a, b = rows_of(ring, e0[i]), rows_of(ring, e1[i])
        h0.append([(-uh[m] * _obj(crp[i][m]) + g_term(ring, i, m) * sk[m] + a[m]) % ring.moduli[m] for m in range(nmod_of(ring))])
        h1.append([(sk[m] * _obj(crp[i][m]) + b[m]) % ring.moduli[m] for m in range(nmod_of(ring))])
    return h0, h1


def rkg_round2(ring, s, h0agg, h1agg, u, e2, e3):
    """out_i = sk (.) H0agg_i + NTT(e2_i) + (NTT(u) - sk) (.) H1agg_i + NTT(e3_i)"""
    sk, uh = rows_of(ring, s), rows_of(ring, u)
    out = []
    for i in range(beta_of(ring)):
        a, b = rows_of(ring, e2[i]), rows_of(ring, e3[i])
        out.append([(sk[m] * _obj(h0agg[i][m]) + a[m] + (uh[m] - sk[m]) * _obj(h1agg[i][m]) + b[m]) % ring.moduli[m] for m in range(nmod_of(ring))])
    return out


def aggregate(ring, shares):
    """sum over the parties of rows [..][nmod][N] (any leading shape), modulus by modulus"""
    acc = np.array(shares[0], dtype=object)
    for s in shares[1:]:
        acc = acc + np.array(s, dtype=object)
    mods = np.array(ring.moduli, dtype=object).reshape((1,) * (acc.ndim - 2) + (nmod_of(ring), 1))
    return acc % mods


def to_u64(rows):
    return np.array(rows, dtype=object).astype(np.uint64)


# ---------------------------------------------------------------- the common reference polynomials
def crp_row(key32, row, q, n, want_tries=False):
    """coefficients 0..n-1 of global row `row` at modulus q: ChaCha20 block under key32, block counter j, nonce (row low word, row high word, try t); the sixteen
    words form eight 64-bit candidates (word 2k low, 2k+1 high) masked to bitlen(q) bits; the first candidate < q, else the same with t + 1 (t from 0)"""
    mask = np.uint64((1 << int(q).bit_length()) - 1)
    out = np.zeros(n, dtype=np.uint64)
    tries = np.zeros(n, dtype=np.int64)
    pending = np.arange(n)
    t = 0
    while pending.size:
        W = er.chacha20_blocks(key32, pending, (row & 0xFFFFFFFF, (row >> 32) & 0xFFFFFFFF, t)).astype(np.uint64)
        cand = (W[:, 0::2] | (W[:, 1::2] << np.uint64(32))) & mask
        ok = cand < np.uint64(q)
        has = ok.any(axis=1)
        out[pending[has]] = cand[has, ok[has].argmax(axis=1)]
        tries[pending[has]] = t
        pending = pending[~has]
        t += 1
    return (out, tries) if want_tries else out


def crp_rows(key32, first_row, mod_idx, moduli, n):
    return np.stack([crp_row(key32, first_row + r, moduli[m], n) for r, m in enumerate(mod_idx)])
