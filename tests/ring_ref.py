"""Test-side references of the general ring beyond what one oracle ring holds.

  * SplitRing: a ring of more than ORC_MAXMOD = 16 moduli, its transforms served by two oracle rings that together hold every modulus;
  * keyswitch(): orc_keyswitch restated in Python integers, vectorised over the coefficients (numpy object arrays).  The float correction comes from
    ksw_ref.ext_model word by word, the extension's residue from ksw_ref.ext_value on whole rows; the transforms are the oracle's;
  * decode(): slot values of a coefficient vector (plain complex FFT - the end-to-end tests compare within the scheme's noise, far above fp64's);
  * crt_centered(): residue rows -> signed Python integers.
"""
from math import prod

import numpy as np

import ksw_ref
import oracle_lib as ol


class SplitRing:
    def __init__(self, logN, q, p):
        self.logN, self.N, self.nq, self.np_ = logN, 1 << logN, len(q), len(p)
        self.moduli = list(q) + list(p)
        self.slots, self.beta = self.N // 2, (len(q) + len(p) - 1) // len(p)
        h = (len(self.moduli) + 1) // 2
        self.parts = [(0, ol.Ring(logN, self.moduli[:h - 1], self.moduli[h - 1:h])), (h, ol.Ring(logN, self.moduli[h:-1], self.moduli[-1:]))]

    def _at(self, mod):
        off, r = self.parts[0] if mod < self.parts[1][0] else self.parts[1]
        return r, mod - off

    def ntt(self, mod, a):
        r, m = self._at(mod)
        return r.ntt(m, a)

    def intt(self, mod, a):
        r, m = self._at(mod)
        return r.intt(m, a)

    def galois(self, k):
        return self.parts[0][1].galois(k)


def _obj(a):
    return np.array([int(v) for v in a], dtype=object)


def extend_rows(rows, qs, targets):
    """coefficient-domain rows of one digit -> {qt: row} (uint64), as the oracle's basis_extend defines it"""
    if len(qs) == 1:
        x = _obj(rows[0])
        return {qt: (x % qt).astype(np.uint64) for qt in targets}
    n = len(rows[0])
    ys, v = [np.empty(n, dtype=object) for _ in qs], np.empty(n, dtype=object)
    for x in range(n):
        y, vf, _ = ksw_ref.ext_model([int(r[x]) for r in rows], qs)
        for m in range(len(qs)):
            ys[m][x] = y[m]
        v[x] = vf
    return {qt: ksw_ref.ext_value(ys, v, qs, qt).astype(np.uint64) for qt in targets}


def keyswitch(ring, level, cx, key):
    """cx [level+1][N] NTT rows, key [beta][2][nmod][N] -> (d0, d1) [level+1][N]"""
    nq, np_, mods, nl = ring.nq, ring.np_, ring.moduli, level + 1
    c2 = [ring.intt(m, cx[m]) for m in range(nl)]
    tmod = list(range(nl)) + [nq + p for p in range(np_)]
    acc = [[np.zeros(ring.N, dtype=object) for _ in tmod] for _ in range(2)]
    for i, dg in enumerate(ksw_ref.digits(level, np_)):
        qs = [mods[m] for m in dg]
        ext = extend_rows([c2[m] for m in dg], qs, [mods[m] for m in tmod if m not in dg])
        for t, mod in enumerate(tmod):
            e = _obj(cx[mod] if mod in dg else ring.ntt(mod, ext[mods[mod]]))
            for pl in range(2):
                acc[pl][t] = (acc[pl][t] + e * _obj(key[i, pl, mod])) % mods[mod]
    ps = [mods[nq + p] for p in range(np_)]
    out = []
    for pl in range(2):
        rows = [ring.intt(nq + p, acc[pl][nl + p].astype(np.uint64)) for p in range(np_)]
        ext = extend_rows(rows, ps, [mods[t] for t in range(nl)])
        d = []
        for t in range(nl):
            qt = mods[t]
            e = _obj(ring.ntt(t, ext[qt]))
            d.append(((acc[pl][t] - e) * pow(prod(ps) % qt, -1, qt) % qt).astype(np.uint64))
        out.append(np.stack(d))
    return out[0], out[1]


def automorphism_index(logN, g):
    """lattigo ring.PermuteNTTIndex: out[i] = in[index[i]]"""
    N = 1 << logN

    def brev(x):
        return int(format(x, f"0{logN}b")[::-1], 2)
    return np.array([brev((((g * (2 * brev(i) + 1)) & (2 * N - 1)) - 1) >> 1) for i in range(N)], dtype=np.int64)


def rotate_model(ring, level, ct, g, key):
    """orc_apply_galois around keyswitch(): ct [2][level+1][N]"""
    d0, d1 = keyswitch(ring, level, ct[1], key)
    idx = automorphism_index(ring.logN, g)
    out = np.zeros_like(ct)
    for m in range(level + 1):
        q = ring.moduli[m]
        out[0, m] = ((_obj(d0[m]) + _obj(ct[0, m])) % q).astype(np.uint64)[idx]
        out[1, m] = d1[m][idx]
    return out


def mulrelin_model(ring, level, a, b, rlk):
    """orc_mulrelin around keyswitch()"""
    out, c2 = np.zeros_like(a), np.zeros_like(a[0])
    for m in range(level + 1):
        q = ring.moduli[m]
        a0, a1, b0, b1 = _obj(a[0, m]), _obj(a[1, m]), _obj(b[0, m]), _obj(b[1, m])
        out[0, m], out[1, m], c2[m] = (a0 * b0 % q).astype(np.uint64), ((a0 * b1 + a1 * b0) % q).astype(np.uint64), (a1 * b1 % q).astype(np.uint64)
    d0, d1 = keyswitch(ring, level, c2, rlk)
    for m in range(level + 1):
        q = ring.moduli[m]
        out[0, m] = ((_obj(out[0, m]) + _obj(d0[m])) % q).astype(np.uint64)
        out[1, m] = ((_obj(out[1, m]) + _obj(d1[m])) % q).astype(np.uint64)
    return out


def crt_centered(rows, moduli):
    """[len(moduli)][N] residues -> list of N signed Python integers in (-Q/2, Q/2]"""
    Q = prod(moduli)
    x = np.zeros(rows.shape[1], dtype=object)
    for r, q in zip(rows, moduli):
        x = x + _obj(r) * ((Q // q) * pow(Q // q, -1, q))
    x = x % Q
    return [int(v) - Q if int(v) > Q // 2 else int(v) for v in x]


def decode(coeffs, N, scale):
    """slot t of the plaintext with integer coefficients p: sum_c w_c zeta^(5^t c), w_c = (p_c + i p_{c+n}) / scale, zeta = exp(2 pi i / 2N)"""
    n = N // 2
    w = (np.array([float(c) for c in coeffs[:n]]) + 1j * np.array([float(c) for c in coeffs[n:]])) / float(scale)
    a = w * np.exp(1j * np.pi * np.arange(n) / N)                  # w_c zeta^c; 5^t = 4 m_t + 1 turns the sum into a length-n transform at m_t
    V = np.fft.ifft(a) * n
    m_t, g = np.empty(n, dtype=np.int64), 1
    for t in range(n):
        m_t[t] = ((g - 1) // 4) % n
        g = g * 5 % (2 * N)
    return V[m_t]
