"""Test-side reference for the collective bootstrap's local arithmetic (csrc/refresh.hip with the Garner and share helpers of csrc/recode.hpp).

Three things, none of which touches the GPU by itself:
  * the expected values in Python integers - the ONLY source of them (expected_rows, expected_recode, from_digits): Int(big.Float(f)) = int(f),
    Quo truncates towards zero, a tie x == Q // 2 counts as negative;
  * a word-exact model of the kernels' steps (model_rows, model_recode, model_share_tail), vectorised over the coefficients with numpy: 64-bit
    limbs as uint64, the fp64 Horner / Garner steps as int64 with the quotient estimate taken in float64 exactly as the kernel takes it.  The model
    only CLASSIFIES inputs (which branch classes a coefficient takes); tests/test_refresh_ref.py holds its values against the Python integers and
    breaks it one mistake at a time (MUTANTS);
  * the directed inputs by chain, level and scale pair (CASES, case_inputs), placed at coefficients 0, 255, 256, N - 1 and a seeded spread, the rest
    a seeded random fill; one context + oracle ring per chain, kept for the session (gpu_env).

How a float64 scale becomes (m, e) - scale_parts(): Int(f) = m * 2^e with m < 2^53, and m keeps ALL 53 mantissa bits of f >= 2^52 (2^98 is
2^52 * 2^46, not 1 * 2^98).  The shift of a scale pair is therefore e_target - e_ct with e = max(log2 f - 52, 0): (2^98, 2^34) shifts by -46 and
(2^104, 2^34) by -52, both inside one limb.  The pairs that reach the other shift classes are (2^116, 2^34): -64, (2^122, 2^34): -70,
(2^55, 2^119): +64, (2^55, 2^130): +75; the short division sees d == 1 only for a ciphertext scale in [1, 2): (1.5, 2^34).

Branch classes that are unreachable by construction (left out of the coverage requirement; the model still watches them and test_refresh_ref.py
asserts they stay empty):
  * rows_canon / mod_canon / garner_canon: a positive multiple of q handed to canon() by the Horner steps of k_bigint_rows and bg_mod or by the
    Garner step.  mulmod_lazy rounds its quotient to nearest, so its result lies in [-q/2 - 1, q/2 + 1]; plus a 32-bit digit that is below
    q/2 + 2^32 + 1 < q for q > 2^33 + 2 (every modulus here has >= 35 bits), and the Garner step adds nothing.
  * mul_overflow: a carry out of limb 7 of bg_mul_add - scale_ratio() and the mask fit check keep every product below 2^510.
  * cy_limb_{W-1}: the "+ 1" of a negative mask carries out of its top limb only for the limbs of 0, which is not negative.
  * mul_carry in the rescale when the target mantissa is a power of two 2^t: the low word of a_i * 2^t has t zero bits below and the carry is < 2^t.
  * rsub_equal_borrow when Q_level has fewer than 3 limbs: an equal limb with a borrow coming in needs a lower limb (the borrow) and a higher
    one (x < Q must be decided above it).
  * the `== 0 ? 0 :` guards of k_bigint_rows and k_bigint_rows_scaled are reachable (neg_zero) but REDUNDANT: q - 0 = q is followed by
    `v += e; v >= q ? v - q : v`, which folds it back for e >= 0, and for e < 0 q + e is already the canonical value of -0 + e.  The guards of
    k_share (share_neg_zero) and k_recode_scaled (recode_neg_zero) are the live ones.

R13 = ol.small_primes(14, 36, 13) + one 40-bit special prime is accepted by the context (14 moduli <= SFG_MAXMOD = 16), so the RF_MAXL bound is
tested on it: level 11 runs, level 12 is refused."""
import atexit
from functools import lru_cache
from math import gcd, log2, prod

import numpy as np

import ksw_ref as kr
import oracle_lib as ol

N = 1 << 14
BG = 8                                      # 64-bit limbs of the device big integer
RF_MAXL = 12
M64 = (1 << 64) - 1
F8, I8, U8 = np.float64, np.int64, np.uint64
U32, UM32 = np.uint64(32), np.uint64(0xFFFFFFFF)
REPS = 8                                    # every directed value sits at 8 coefficients


# ---------------------------------------------------------------- chains, scale pairs, cases
@lru_cache(maxsize=None)
def chain(name):
    """(q, p) of a chain"""
    if name == "PN14":
        return list(ol.Q_PN14), list(ol.P_PN14)
    if name == "R13":
        return ol.small_primes(14, 36, 13), ol.small_primes(14, 40, 1)
    return list(kr.CHAINS[name][0]), list(kr.CHAINS[name][1])


PAIRS = {
    "ref": (2.0 ** 68, 2.0 ** 34),                                   # the reference's: a fresh product, sh = -16
    "ref_np2": (2.0 ** 68 / 34359410689.0 * 2.0 ** 34, 2.0 ** 34),   # the reference's: a product of a rescaled operand
    "one": (2.0 ** 34, 2.0 ** 34),                                   # ratio 1: the unscaled kernels
    "i98": (2.0 ** 98, 2.0 ** 34),                                   # sh = -46
    "i104": (2.0 ** 104, 2.0 ** 34),                                 # sh = -52
    "r64": (2.0 ** 116, 2.0 ** 34),                                  # sh = -64: right, ws = 1, bs == 0
    "r70": (2.0 ** 122, 2.0 ** 34),                                  # sh = -70: right, ws = 1, bs != 0
    "l45": (2.0 ** 55, 2.0 ** 100),                                  # sh = +45: left, ws = 0
    "l64": (2.0 ** 55, 2.0 ** 119),                                  # sh = +64: left, ws = 1, bs == 0
    "l75": (2.0 ** 55, 2.0 ** 130),                                  # sh = +75: left, ws = 1, bs != 0
    "m1": (2.0 ** 53 + 2.0, 1.0),                                    # target mantissa 1, Int(ct scale) = (2^52 + 1) * 2
    "d1": (1.5, 2.0 ** 34),                                          # Int(ct scale) = 1: bg_div_small returns at once
    "c60": (2.0 ** 60, 2.0 ** 53),                                   # Int(ct scale) = 2^52 * 2^8
    "np2_up": (1234567.0 * 2.0 ** 20, 2.0 ** 40 + 2.0 ** 7),         # not powers of two, target above the input, sh = 0
    "np2_l48": (1234567.0 * 2.0 ** 20, (2.0 ** 40 + 2.0 ** 7) * 2.0 ** 60),   # not powers of two and a left shift: the division after the shift is not exact
}
REFERENCE_PAIRS = ("ref", "ref_np2")

# (chain, level, mask limbs W, pair or None for the unscaled form)
CASES = [("PN14", 9, 16, None), ("PN14", 9, 6, "ref"), ("PN14", 9, 6, "ref_np2"), ("PN14", 9, 6, "one"), ("PN14", 9, 6, "i98"), ("PN14", 9, 6, "i104"),
         ("PN14", 9, 7, "r64"), ("PN14", 9, 6, "r70"), ("PN14", 9, 6, "l45"), ("PN14", 9, 6, "l64"), ("PN14", 9, 5, "l75"), ("PN14", 9, 6, "m1"),
         ("PN14", 9, 6, "d1"), ("PN14", 9, 7, "c60"), ("PN14", 9, 7, "np2_up"), ("PN14", 9, 6, "np2_l48"),
         ("PN14", 6, 7, None), ("PN14", 6, 7, "ref"), ("PN14", 6, 5, "r70"), ("PN14", 6, 5, "l75"), ("PN14", 6, 7, "np2_up"),
         ("PN14", 0, 1, None), ("PN14", 0, 1, "ref"), ("PN14", 0, 2, "l64"),
         ("S4", 7, 16, None), ("S4", 7, 7, "ref"), ("S4", 7, 7, "r64"), ("S4", 7, 6, "l45"), ("S4", 7, 7, "np2_up"),
         ("S4", 0, 1, None), ("S4", 0, 1, "ref_np2"),
         ("R13", 11, 7, None), ("R13", 11, 7, "ref"), ("R13", 11, 7, "r70"), ("R13", 11, 7, "np2_up")]


def case_id(case):
    return f"{case[0]}-L{case[1]}-W{case[2]}-{case[3] or 'unscaled'}"


def scales_of(case):
    return None if case[3] is None else PAIRS[case[3]]


def scale_parts(f):
    """Int(big.Float(f)) = m * 2^e as the kernel's scale_int() splits it: the 53-bit mantissa and its exponent, e = 0 below 2^53"""
    i = int(f)
    e = max(i.bit_length() - 53, 0)
    assert (i >> e) << e == i
    return i >> e, e


def ratio(scales):
    """(mo, mi, sh) of the kernel's ScaleRatio, or None where the library takes the unscaled kernels"""
    if scales is None or scales[0] == scales[1]:
        return None
    (mi, ei), (mo, eo) = scale_parts(scales[0]), scale_parts(scales[1])
    return mo, mi, eo - ei


def shift_class(sh):
    if sh == 0:
        return "shift_none"
    k = abs(sh)
    return f"shift_{'left' if sh > 0 else 'right'}_ws{min(k >> 6, 1)}_{'bs0' if k & 63 == 0 else 'bs'}"


def fits(case):
    """scale_ratio()'s and the share form's fit checks"""
    name, level, W, _ = case
    r = ratio(scales_of(case))
    if r is None:
        return True
    bits = sum(log2(q) for q in chain(name)[0][:level + 1])
    up = max(r[2], 0)
    return bits + 54 + up <= 64 * BG - 2 and W <= BG and 64 * W + 54 + up <= 64 * BG


# ---------------------------------------------------------------- expected values: Python integers
def quo(a, b):
    """big.Int.Quo: truncated towards zero"""
    return abs(a) // b * (1 if a >= 0 else -1)


def rescaled(v, scales):
    return v if scales is None else quo(v * int(scales[1]), int(scales[0]))


def expected_rows(vals, es, moduli, scales=None):
    """rows[j][c] = (Quo(mask_c * Int(target), Int(scale)) + e_c) mod q_j; scales=None: the mask itself"""
    s = [rescaled(int(v), scales) + int(e) for v, e in zip(vals, es)]
    return np.array([[v % q for v in s] for q in moduli], dtype=U8)


def expected_recode(xs, level_mods, moduli, scales=None):
    """x in [0, Q) -> x - Q if x >= Q // 2 -> Quo -> the residue modulo every q_j"""
    Q = prod(level_mods)
    s = [rescaled(x - Q if x >= Q // 2 else x, scales) for x in xs]
    return np.array([[v % q for v in s] for q in moduli], dtype=U8)


def from_digits(d, mods):
    """x = v0 + q0 (v1 + q1 (...))"""
    x = 0
    for v, q in zip(reversed(d), reversed(mods)):
        assert 0 <= v < q
        x = x * q + v
    return x


def to_digits(x, mods):
    d = []
    for q in mods:
        d.append(x % q)
        x //= q
    return d


# ---------------------------------------------------------------- the model: helpers
MUTANTS = ["no_zero_guard",         # no `== 0` guard on a live negation (k_share, k_recode_scaled)
           "tie_strict",            # `>` for `>=` in the tie rule: all digits equal counts as positive
           "mul_drop_carry",        # bg_mul_add without `+ (s < lo)`
           "rsub_no_dlt",           # bg_rsub without `| (d < br)`
           "bs0_as_64",             # bg_shift without the `bs ?` guard: bs == 0 handled as a shift of the partner word by 64, which the hardware takes as 0
           "canon_nofix",           # canon without its equality fix-up
           "shift_after_div"]       # bg_rescale as mul, div, shift


def _mark(cls, name, arr):
    if name in cls:
        cls[name] = cls[name] | arr
    else:
        cls[name] = np.array(arr, dtype=bool)


def canon_v(x, q, cls, site, mutant=None):
    """common.hpp canon() on integer-valued x (ksw_ref.canon_model's formula): floor of the rounded product, exact remainder, equality fix-up"""
    assert int(np.abs(x).max(initial=0)) < 1 << 51
    k = np.floor(x.astype(F8) * (1.0 / float(q))).astype(I8)
    r = x - k * I8(q)
    fix = r == q
    mult = (x > 0) & (x % I8(q) == 0)
    assert not np.any(fix & ~mult)
    _mark(cls, site + "_mult_fix", mult & fix)
    _mark(cls, site + "_mult_nofix", mult & ~fix)
    out = r if mutant == "canon_nofix" else np.where(fix, I8(0), r)
    return out


def mulmod_lazy_v(x, w, q):
    """common.hpp mulmod_lazy(): x w - rint(x * fl(w / q)) q.  The kernel's two-product form is exact for |result| < 2^52, so the integer is taken modulo 2^64"""
    wq = float(w) * (1.0 / float(q))
    qh = np.rint(x.astype(F8) * wq).astype(I8)
    r = (np.ascontiguousarray(x).view(U8) * U8(w) - qh.view(U8) * U8(q)).view(I8)
    assert int(np.abs(r).max(initial=0)) < 1 << 51
    return r


def horner_mod(limbs, q, cls, site):
    """Horner over the 32-bit digits of [n][L] uint64 limbs, top down, as k_bigint_rows and bg_mod run it"""
    B = kr.canon_model(1 << 32, q)
    acc = np.zeros(limbs.shape[0], dtype=I8)
    for i in range(limbs.shape[1] - 1, -1, -1):
        for dgt in (limbs[:, i] >> U32, limbs[:, i] & UM32):
            acc = canon_v(mulmod_lazy_v(acc, B, q) + dgt.astype(I8), q, cls, site)
    return acc


def mul64(a, m):
    """(low, high) words of a * m, a uint64 array, m < 2^64"""
    ml, mh = U8(m & 0xFFFFFFFF), U8(m >> 32)
    al, ah = a & UM32, a >> U32
    ll, lh, hl, hh = al * ml, al * mh, ah * ml, ah * mh
    mid = (ll >> U32) + (lh & UM32) + (hl & UM32)
    return (ll & UM32) | (mid << U32), hh + (lh >> U32) + (hl >> U32) + (mid >> U32)


def bg_mul_add_v(a, m, add, cls, site, mutant=None):
    c = add.astype(U8)
    for i in range(BG):
        lo, hi = mul64(a[:, i], m)
        s = lo + c
        carry = s < lo
        _mark(cls, f"{site}_carry_limb{i}", carry)
        a[:, i] = s
        c = hi if mutant == "mul_drop_carry" else hi + carry.astype(U8)
    _mark(cls, "mul_overflow", c != 0)


def bg_rsub_v(a, b, cls, mutant=None):
    br = np.zeros(a.shape[0], dtype=U8)
    for i in range(BG):
        bi = U8(b[i])
        d = bi - a[:, i]
        d2 = d - br
        through = d < br
        _mark(cls, "rsub_equal_borrow", through)
        nbr = bi < a[:, i]
        br = (nbr if mutant == "rsub_no_dlt" else nbr | through).astype(U8)
        a[:, i] = d2
    _mark(cls, "rsub_underflow", br != 0)


def bg_shift_v(a, sh, cls, mutant=None):
    _mark(cls, shift_class(sh), np.ones(a.shape[0], dtype=bool))
    if not sh:
        return
    k = abs(sh)
    ws, bs = k >> 6, k & 63
    zero = np.zeros(a.shape[0], dtype=U8)
    limb = lambda i: a[:, i] if 0 <= i < BG else zero
    t = np.zeros_like(a)
    for i in range(BG):
        own, partner = (limb(i - ws), limb(i - ws - 1)) if sh > 0 else (limb(i + ws), limb(i + ws + 1))
        if bs:
            t[:, i] = (own << U8(bs)) | (partner >> U8(64 - bs)) if sh > 0 else (own >> U8(bs)) | (partner << U8(64 - bs))
        else:
            t[:, i] = own | partner if mutant == "bs0_as_64" else own    # the mistake: a 64-bit shift by 64 takes its count modulo 64 and leaves the partner whole
    a[:] = t


def bg_div_small_v(a, d, cls):
    _mark(cls, "div_d1" if d == 1 else "div_bytes", np.ones(a.shape[0], dtype=bool))
    if d == 1:
        return
    r = np.zeros(a.shape[0], dtype=U8)
    for i in range(BG - 1, -1, -1):
        w, q = a[:, i].copy(), np.zeros(a.shape[0], dtype=U8)
        for b in range(7, -1, -1):
            r = (r << U8(8)) | ((w >> U8(8 * b)) & U8(0xFF))
            qb = r // U8(d)
            r = r - qb * U8(d)
            q = (q << U8(8)) | qb
        a[:, i] = q


def bg_rescale_v(a, r, cls, mutant=None):
    mo, mi, sh = r
    bg_mul_add_v(a, mo, np.zeros(a.shape[0], dtype=U8), cls, "rescale_mul", mutant)
    if mutant == "shift_after_div":
        bg_div_small_v(a, mi, cls)
        bg_shift_v(a, sh, cls, mutant)
    else:
        bg_shift_v(a, sh, cls, mutant)
        bg_div_small_v(a, mi, cls)


def limbs_of(vals, L):
    return ol.bigints_to_limbs(vals, L)


def ints_of(limbs):
    return [sum(int(w) << (64 * i) for i, w in enumerate(row)) for row in limbs]


# ---------------------------------------------------------------- the model: kernels
def model_rows(limbs, e, moduli, scales=None, mutant=None):
    """k_bigint_rows (scales None or ratio 1) / k_bigint_rows_scaled on [n][W] two's-complement limbs and [n] int32 -> (rows [nmod][n] uint64, classes)"""
    cls = {}
    n, W = limbs.shape
    neg = (limbs[:, W - 1] >> U8(63)) != 0
    _mark(cls, "mask_neg", neg)
    mag = np.where(neg[:, None], ~limbs, limbs)
    ev = e.astype(I8)
    r = ratio(scales)
    out = []
    if r is not None:
        a = np.zeros((n, BG), dtype=U8)
        a[:, :W] = mag
        cy = neg.astype(U8)
        for i in range(BG):
            live = cy != 0
            a[:, i] = a[:, i] + cy
            cy = (live & (a[:, i] == 0)).astype(U8)
            _mark(cls, f"cy_limb{i}", cy != 0)
        a[:, W:] = np.where(neg[:, None], U8(0), a[:, W:])
        bg_rescale_v(a, r, cls, mutant)
    for q in moduli:
        if r is None:
            acc = horner_mod(mag, q, cls, "rows_canon")
            acc = np.where(neg, acc + 1, acc)
            wrap = neg & (acc >= q)
            _mark(cls, "plus1_wrap", wrap)
            acc = np.where(wrap, acc - q, acc)
        else:
            acc = horner_mod(a, q, cls, "mod_canon")
        zero = neg & (acc == 0)
        _mark(cls, "neg_zero", zero)
        v = np.where(neg & ~zero, q - acc, acc) + ev          # the guard's absence is folded back by the corrections below: no mutant
        below = v < 0
        _mark(cls, "e_below", below)
        v = np.where(below, v + q, v)
        above = v >= q
        _mark(cls, "e_above", above)
        out.append(np.where(above, v - q, v).astype(U8))
    return np.array(out), cls


def model_share_tail(r, q, neg, mutant=None):
    """k_share after share_word: the negate-unless-zero tail on canonical words"""
    cls = {}
    r = r.astype(I8)
    zero = r == 0
    if neg:
        _mark(cls, "share_neg_zero", zero)
        r = q - r if mutant == "no_zero_guard" else np.where(zero, I8(0), q - r)
    return r.astype(U8), cls


def model_small_rows(e, moduli):
    v = e.astype(I8)
    return np.array([np.where(v < 0, I8(q) + v, v).astype(U8) for q in moduli])


def model_recode(res, level, q_all, scales=None, mutant=None):
    """k_recode (scales None or ratio 1) / k_recode_scaled on residues [level+1][n] -> (rows [nq][n] uint64, classes)"""
    cls = {}
    nl, nq, n = level + 1, len(q_all), res.shape[1]
    mods = q_all[:nl]
    Q = prod(mods)
    half = to_digits(Q >> 1, mods)
    rr = [res[i].astype(I8) for i in range(nl)]
    # garner_digits
    v = []
    for i in range(nl):
        q = mods[i]
        t = rr[i]
        for s in range(i):
            d = t - canon_v(v[s], q, cls, "digit_canon", mutant)
            t = canon_v(mulmod_lazy_v(d, pow(mods[s], -1, q), q), q, cls, "garner_canon", mutant)
        v.append(t)
    # garner_negative
    neg = np.zeros(n, dtype=bool) if mutant == "tie_strict" else np.ones(n, dtype=bool)
    open_ = np.ones(n, dtype=bool)
    for i in range(nl - 1, -1, -1):
        dec = open_ & (v[i] != half[i])
        _mark(cls, f"tie_digit{i}", dec)
        neg = np.where(dec, v[i] > half[i], neg)
        open_ = open_ & ~dec
    _mark(cls, "tie_all_equal", open_)
    _mark(cls, "x_neg", neg)
    r = ratio(scales)
    out = []
    if r is None:
        for j in range(nl):
            out.append(rr[j].astype(U8))
        for j in range(nl, nq):
            q = q_all[j]
            acc = canon_v(v[nl - 1], q, cls, "digit_canon", mutant)
            for i in range(nl - 2, -1, -1):
                acc = canon_v(mulmod_lazy_v(acc, mods[i] % q, q) + canon_v(v[i], q, cls, "digit_canon", mutant), q, cls, "sum_canon", mutant)
            acc = np.where(neg, acc - Q % q, acc)
            wrap = acc < 0
            _mark(cls, "recode_neg_wrap", wrap)
            out.append(np.where(wrap, acc + q, acc).astype(U8))
        return np.array(out), cls
    a = np.zeros((n, BG), dtype=U8)
    a[:, 0] = v[nl - 1].astype(U8)
    for i in range(nl - 2, -1, -1):
        bg_mul_add_v(a, mods[i], v[i].astype(U8), cls, "garner_mul", mutant)
    Ql = [(Q >> (64 * i)) & M64 for i in range(BG)]
    an = a.copy()
    bg_rsub_v(an, Ql, cls, mutant)
    for name in ("rsub_equal_borrow", "rsub_underflow"):                   # only the lanes that take bg_rsub count
        cls[name] = cls[name] & neg
    a = np.where(neg[:, None], an, a)
    bg_rescale_v(a, r, cls, mutant)
    for q in q_all:
        acc = horner_mod(a, q, cls, "mod_canon")
        zero = neg & (acc == 0)
        _mark(cls, "recode_neg_zero", zero)
        if mutant == "no_zero_guard":
            out.append(np.where(neg, q - acc, acc).astype(U8))
        else:
            out.append(np.where(neg & ~zero, q - acc, acc).astype(U8))
    return np.array(out), cls


DEAD = ["rows_canon_mult_fix", "rows_canon_mult_nofix", "mod_canon_mult_fix", "mod_canon_mult_nofix", "garner_canon_mult_fix", "garner_canon_mult_nofix",
        "mul_overflow", "rsub_underflow"]
# probability under 2^-20 per uniformly random coefficient: the seeded fill must take none of them
RARE = ["plus1_wrap", "rsub_equal_borrow", "tie_all_equal", "digit_canon_mult_fix", "digit_canon_mult_nofix", "sum_canon_mult_fix", "sum_canon_mult_nofix"]
RARE_WIDE = ["neg_zero", "e_below", "e_above", "recode_neg_zero"]


def rare_in(case):
    """the classes a uniformly random coefficient of this case takes with probability under 2^-20: RARE; a tie decided below the top digit; the
    zero and the e corrections where the rescaled values still spread over more than 2^20 q (at level 0 the reference's ratio 2^-34 leaves ten bits
    and these classes are common); the ~limbs + 1 carries (2^-64 and less);
    bg_mul_add's carries in the Garner accumulation where every multiplier has 36 bits (a carry out of a limb has probability about q_i / 2^64 per
    step: 2^-28, some 2^-22 over all steps and limbs - but 2^-18 per limb for a 46- or 47-bit multiplier, which is uncommon and not rare)"""
    name, level, W, _ = case
    q = chain(name)[0]
    out = RARE + [f"tie_digit{i}" for i in range(level)] + [f"cy_limb{i}" for i in range(BG)]
    spread = rescaled(prod(q[:level + 1]) // 8, scales_of(case))
    if spread > max(q) << 20:
        out += RARE_WIDE
    if level and max(q[:level]) < 1 << 40:
        out += [f"garner_mul_carry_limb{i}" for i in range(BG)]
    return out


def arm_any(qs):
    return {"fix" if kr.ARM(q) else "nofix" for q in qs}


def required(case):
    """(mask classes, recode classes) the directed inputs of a case must reach: everything the model's steps can take at this chain, level, limb count
    and scale pair.  What is left out is unreachable, with the argument in the module docstring or here."""
    name, level, W, _ = case
    q = chain(name)[0]
    nl, mods = level + 1, chain(name)[0][:level + 1]
    Q = prod(mods)
    r = ratio(scales_of(case))
    mask = ["mask_neg", "neg_zero", "e_below", "e_above"]
    x = ["x_neg", "tie_all_equal"] + [f"tie_digit{i}" for i in range(nl)]
    # a digit v_s that is a positive multiple of a smaller modulus read later: the level's own (Garner) and, unscaled, the new ones (k_recode's Horner)
    later = len(q) if r is None else nl
    kinds = set()
    for s in range(nl):
        for i in range(s + 1, later):
            if q[i] < q[s]:
                ks = range(1, min((q[s] - 1) // q[i], 2000) + 1)
                kinds |= {"fix" if kr.canon_model(k * q[i], q[i], fixup=False) == q[i] else "nofix" for k in ks}
    x += [f"digit_canon_mult_{k}" for k in sorted(kinds)]
    if r is None:
        mask += ["plus1_wrap"]
        if nl < len(q):
            # the last Horner sum of a new modulus is congruent to x: for x = k q_j it is 0 or exactly q_j (the sum is below 3 q_j / 2), so k = 1 decides
            # (with one modulus at the level there is no sum: the single digit is reduced and that is all)
            x += ["recode_neg_wrap"] + ([f"sum_canon_mult_{k}" for k in sorted(arm_any(q[nl:]))] if nl > 1 else [])
        return mask, x
    mo, mi, sh = r
    both = [shift_class(sh), "div_d1" if mi == 1 else "div_bytes"]
    mask += ["u_" + k for k in mask + ["plus1_wrap"]]          # h0 comes from k_bigint_rows on the mask itself
    mask += both + [f"cy_limb{i}" for i in range(W - 1)]
    x += both + ["recode_neg_zero"]
    if mo & (mo - 1):                                          # a carry out of limb i needs the product to reach 2^(64 (i + 1)): limbs 1 .. top
        mask += [f"rescale_mul_carry_limb{i}" for i in range(1, W)]
        x += [f"rescale_mul_carry_limb{i}" for i in range(1, (((Q >> 1) * mo).bit_length() - 1) // 64)]
    if Q.bit_length() > 128:
        x += ["rsub_equal_borrow"]
    x += [f"garner_mul_carry_limb{i}" for i in range((Q.bit_length() - 1) // 64)]
    return mask, x


# ---------------------------------------------------------------- directed inputs
E_EDGES = [0, 19, -19, (1 << 31) - 1, -((1 << 31) - 1), -(1 << 31)]


def preimages(s, scales, q=None):
    """magnitudes m with Quo(m * Int(target), Int(scale)) == s; where the up-scaling skips s, the multiple m = Int(scale) u whose rescaled value
    u Int(target) is s modulo q"""
    if scales is None:
        return [s]
    T, I = int(scales[1]), int(scales[0])
    m = -(-s * I // T)
    if m * T // I == s:
        return [m]
    if q is not None and T % q:
        u = s % q * pow(T, -1, q) % q
        return [I * (u or q)]
    return []


def remainder_edges(scales):
    """magnitudes m > 0 with m * Int(target) mod Int(scale) in {0, Int(scale) - 1}; the latter exists only for coprime integers"""
    if scales is None:
        return []
    T, I = int(scales[1]), int(scales[0])
    out = [I // gcd(I, T), 3 * (I // gcd(I, T))]
    if I > 1 and gcd(I, T) == 1:
        m = (I - 1) * pow(T, -1, I) % I
        out += [m, m + I]
    return [m for m in out if m > 0]


def directed_masks(q_all, level, W, scales):
    """[(mask, e)]: the word, residue and remainder edges of the mask path that fit W limbs, each residue edge with every edge of e"""
    lo, hi = -(1 << (64 * W - 1)), (1 << (64 * W - 1)) - 1
    Ql = prod(q_all[:level + 1])
    edge, plain = [], [0, 1, -1, hi, lo, hi - 1, lo + 1]
    for q in q_all:
        for s in (q, q - 1):                                   # magnitude == 0 / q - 1 modulo q_j: the mask itself, and its rescaled value
            for m in [s] + preimages(s, scales, q):
                edge += [m, -m]
        for k in (2, 12345):
            for s in (k * q, k * q - 1):
                for m in [s] + preimages(s, scales):
                    plain += [m, -m]
        plain += [q << 64, -(q << 64)]
    plain += [Ql, -Ql, Ql >> 1, -(Ql >> 1), (1 << 64) - 1, 1 - (1 << 64)]
    for i in range(1, BG):
        plain += [1 << (64 * i), -(1 << (64 * i))]                # zero low limbs: the ~limbs + 1 carry crosses i limbs
    if scales is not None:
        I = int(scales[0])
        plain += [I, -I, I + 1, -I - 1, I - 1, 1 - I]
        for m in remainder_edges(scales):
            plain += [m, -m]
        r = ratio(scales)
        if r is not None:                                      # limb i - 1 all ones, limb i just below a multiple of 2^64 / mo: bg_mul_add carries out of limb i
            for i in range(1, W):
                for k in (1, 2, 3, 5, 7, 11):
                    ai = ((k << 64) - 1) // r[0]
                    if 0 < ai < 1 << 63:
                        m = (ai << (64 * i)) | (M64 << (64 * (i - 1)))
                        plain += [m, -m]
    seen, out = set(), []
    for group, es in ((edge, E_EDGES), (plain, None)):
        for v in group:
            if lo <= v <= hi and (v, group is edge) not in seen:
                seen.add((v, group is edge))
                out += [(v, e) for e in es] if es else [(v, E_EDGES[len(out) % len(E_EDGES)])]
    return out


def canon_multiples(qs, qi, limit=2000):
    """k with k qi < qs, at most three whose canon() needs the fix-up and three whose does not, plus the largest"""
    kmax = (qs - 1) // qi
    fix, nofix = [], []
    for k in range(1, min(kmax, limit) + 1):
        (fix if kr.canon_model(k * qi, qi, fixup=False) == qi else nofix).append(k)
    out = fix[:3] + nofix[:3] + ([kmax] if kmax >= 1 else [])
    return sorted(set(out))


def directed_x(q_all, level, scales, seed=1):
    """x in [0, Q_level) by mixed-radix digits: the sign rule's ties, digit edges, digits and values that are multiples of another modulus, the
    remainder edges of the rescale, and the limb patterns that make bg_mul_add carry and bg_rsub borrow through an equal limb"""
    nl = level + 1
    mods = q_all[:nl]
    Q = prod(mods)
    H = Q >> 1
    h = to_digits(H, mods)
    rnd = np.random.default_rng(seed)
    rand_digits = lambda: [int(rnd.integers(0, q)) for q in mods]
    xs = [0, 1, Q - 1, H, H - 1, H + 1]
    for p in range(nl):                                        # equal to H above digit p, different at p (both sides), random below
        for dv in (h[p] + 1, h[p] - 1, 0, mods[p] - 1):
            if 0 <= dv < mods[p] and dv != h[p]:
                for low in (h[:p], rand_digits()[:p]):
                    xs.append(from_digits(low + [dv] + h[p + 1:], mods))
    xs.append(from_digits([q - 1 for q in mods], mods))
    for i in range(nl):
        for dv in (0, mods[i] - 1):
            for top in (0, mods[-1] - 1) if i < nl - 1 else (dv,):
                d = rand_digits()
                d[i], d[-1] = dv, top if i < nl - 1 else dv
                xs.append(from_digits(d, mods))
    for s in range(nl):                                        # digit v_s = k q_i, for the later moduli of the level and the new moduli
        for i in range(s + 1, len(q_all)):
            if q_all[i] < mods[s]:
                for k in canon_multiples(mods[s], q_all[i]):
                    for top in (1, mods[-1] - 2):
                        d = rand_digits()
                        d[s] = k * q_all[i]
                        if s < nl - 1:
                            d[-1] = top
                        xs.append(from_digits(d, mods))
    for j in range(nl, len(q_all)):                            # x = k q_j and Q - k q_j for the new moduli
        for k in sorted(set(list(range(1, 9)) + canon_multiples(Q, q_all[j]))):
            xs += [k * q_all[j], Q - k * q_all[j]]
    if scales is not None:
        for m in remainder_edges(scales):
            xs += [m, Q - m]
        for q in q_all:                                        # rescaled magnitude == 0 modulo q_j
            for k in (1, 2):
                for m in preimages(k * q, scales, q):
                    xs += [m, Q - m]
        I = int(scales[0])
        xs += [I, Q - I, I - 1, Q - I + 1, I + 1, Q - I - 1]
    nlimb = (Q.bit_length() + 63) // 64
    if ratio(scales) is not None:
        for i in range(1, nlimb - 1):                          # limb i equal to Q's, limb i - 1 above Q's (a borrow comes in), the top limb one below Q's
            ql = [(Q >> (64 * t)) & M64 for t in range(nlimb)]
            if ql[i - 1] < M64 and ql[-1] >= 2:
                xl = list(ql)
                xl[i - 1] += 1
                xl[-1] -= 1
                xs.append(sum(w << (64 * t) for t, w in enumerate(xl)))
        # bg_mul_add(a, q_i, v_i): the partial value P of the digits above i is any integer below their product; limb l - 1 all ones and limb l just
        # below a multiple of 2^64 / q_i carry out of limb l.  Limb 0 carries when (P q_i mod 2^64) + v_i wraps.
        for i in range(nl - 1):
            above = prod(mods[i + 1:])
            below = prod(mods[:i])
            for l in range(0, (above.bit_length() - 1) // 64 + 1):
                for k in (1, 2, 3, 5, 7, 11, 13):
                    al = ((k << 64) - 1) // mods[i]
                    P = (al << (64 * l)) | ((M64 << (64 * (l - 1))) if l else 0)
                    if 0 < P < above:
                        x = (P * mods[i] + mods[i] - 1) * below + (below - 1 if below > 1 else 0)
                        xs.append(x)
        r = ratio(scales)
        for i in range(1, nlimb):                              # the rescale's own multiplication, on |x| for both signs
            for k in (1, 2, 3, 5, 7, 11):
                ai = ((k << 64) - 1) // r[0]
                m = (ai << (64 * i)) | (M64 << (64 * (i - 1)))
                if 0 < m < H:
                    xs += [m, Q - m]
    out, seen = [], set()
    for x in xs:
        if 0 <= x < Q and x not in seen:
            seen.add(x)
            out.append(x)
    return out


def place(directed, fill, seed):
    """the directed items REPS times over: the first four at coefficients 0, 255, 256, N - 1, the rest at a seeded spread; fill elsewhere.
    -> (items [N], is_directed [N])"""
    n = len(directed) * REPS
    assert 4 <= n <= 3 * N // 4, n
    rnd = np.random.default_rng(seed)
    fixed = [0, 255, 256, N - 1]
    rest = np.setdiff1d(np.arange(N), fixed)
    pos = fixed + [int(p) for p in rnd.permutation(rest)[:n - 4]]
    items, flag = list(fill), np.zeros(N, dtype=bool)
    for k, p in enumerate(pos):
        items[p] = directed[k % len(directed)]
        flag[p] = True
    return items, flag


def random_masks(rnd, bound, n=N):
    """uniform in [-bound / 2, bound / 2)"""
    nb = (bound.bit_length() + 7) // 8 + 8
    return [int.from_bytes(rnd.bytes(nb), "little") % bound - (bound >> 1) for _ in range(n)]


class Inputs:
    """what case_inputs() returns: case, scales, q, level, W, Q; masks, e, limbs, mask_directed, want_h0, want_h1; x, x_res, x_directed, want_x"""


@lru_cache(maxsize=None)
def case_inputs(case):
    """the inputs of a case and their expected values, built once: masks (values, limbs, e, directed flags) and recode values (x, residues, flags)"""
    name, level, W, _ = case
    scales = scales_of(case)
    q_all = chain(name)[0]
    mods = q_all[:level + 1]
    Q = prod(mods)
    seed = CASES.index(case) if case in CASES else 999
    rnd = np.random.default_rng(1000 + seed)
    c = Inputs()
    c.case, c.scales, c.q, c.level, c.W, c.Q = case, scales, q_all, level, W, Q
    bound = min(Q // 4, 1 << (64 * W - 1))
    fill = list(zip(random_masks(rnd, bound), [int(v) for v in rnd.integers(-19, 20, N)]))
    items, c.mask_directed = place(directed_masks(q_all, level, W, scales), fill, 2000 + seed)
    c.masks = [m for m, _ in items]
    c.e = np.array([e for _, e in items], dtype=np.int32)
    c.limbs = limbs_of(c.masks, W)
    c.want_h0 = expected_rows(c.masks, c.e, mods)                           # the decrypt share: the mask itself
    c.want_h1 = expected_rows(c.masks, c.e, q_all, scales)                  # the recrypt share, before its negation
    xfill = [int.from_bytes(rnd.bytes(80), "little") % Q for _ in range(N)]
    c.x, c.x_directed = place(directed_x(q_all, level, scales), xfill, 3000 + seed)
    c.x_res = np.array([[x % q for x in c.x] for q in mods], dtype=U8)
    c.want_x = expected_recode(c.x, mods, q_all, scales)
    return c


# ---------------------------------------------------------------- one context and oracle ring per chain, shared by the GPU tests
_ENV = {}


def gpu_env(name):
    """(context, ring) of a chain, made at first use and kept for the session"""
    if name not in _ENV:
        from sfgwas_amd import capi
        q, p = chain(name)
        _ENV[name] = (capi.Context(q, p), ring_of(name))
    return _ENV[name]


@lru_cache(maxsize=None)
def ring_of(name):
    q, p = chain(name)
    return ol.Ring(14, q, p)


@atexit.register
def _close_all():
    for ctx, _ in _ENV.values():
        ctx.close()
    _ENV.clear()
