"""Test-side reference for the multi-word field arithmetic of csrc/beaver.hip (Beaver local products, SSToCMat share algebra).

Three things, none of which touches the GPU:
  * expected(): the local products of mpc/beavermult.go:94-106 in plain Python integers - the only source of expected values;
  * edge_operands() / directed_quadruples(): the operands that drive the kernels into the branches which uniformly random operands
    reach with probability ~2^-80 (third fold, final subtraction, sum == p, carry out of the top word);
  * a model of the kernels' reductions with the kernels' exact word widths (pm_fold chain, f_add, CIOS Montgomery product).  The model
    only CLASSIFIES inputs - which branches does this operand take - and is itself held against expected() by test_field_ref.py.
    A fold works on integers of a stated number of 32-bit words: a word loop with a carry computes (lo + c * H) mod 2^(32 * nout)
    exactly, so the integer form and the word form (pm_fold_words, the literal restatement) are the same function; the test checks that.
"""
import itertools
import random
from functools import lru_cache

import numpy as np

M32 = 0xFFFFFFFF

# ---- the modulus table: (limbs, p)
FOLDED = [(2, (1 << 127) - 1), (2, (1 << 128) - 159), (2, (1 << 127) - (1 << 32) + 1), (2, (1 << 128) - (1 << 32) + 1),
          (2, (1 << 97) - 141), (2, (1 << 97) - (1 << 32) + 1), (2, (1 << 120) - 119), (2, (1 << 126) - 137),
          (4, (1 << 255) - 19), (4, (1 << 256) - 189), (4, (1 << 256) - (1 << 32) + 1),
          (4, (1 << 225) - 49), (4, (1 << 225) - (1 << 32) + 1), (4, (1 << 240) - 467), (4, (1 << 254) - 245)]
GENERIC = [(2, 0xC3A5C85C97CB3127B492B66FBE98F273), (4, 0x9E3779B97F4A7C15F39CC0605CEDC8341082276BF3A27251F86C6A11D0C18E95),
           (2, (1 << 127) - (1 << 40) - 1),
           (2, (1 << 127) - (1 << 32) - 1), (4, (1 << 255) - (1 << 32) - 1),           # c = 2^32 + 1: just outside the folded form
           (2, (1 << 96) - 17)]                                                        # top word empty: must not take the folded path
ALL_MODULI = FOLDED + GENERIC


def mod_id(lp):
    limbs, p = lp
    B = p.bit_length()
    c = (1 << B) - p
    return f"L{limbs}-2^{B}-{c}" if c < (1 << 48) else f"L{limbs}-{p >> (B - 16):x}.."


# ---- expected values: Python integers
def expected(pid, p, ar, am, br, bm):
    """beavermult.go:94-106: pid 0 multiplies the masks, pid 1 adds ar*br, every other party has the two cross terms"""
    if pid == 0:
        return am * bm % p
    return (ar * bm + br * am + (ar * br if pid == 1 else 0)) % p


# ---- directed operands
def edge_operands(p):
    B = p.bit_length()
    c = (1 << B) - p
    last = (1 << B) - 2 * c
    vals = [0, 1, 2, p - 1, p - 2, 1 << (B - 1), (1 << (B - 1)) - 1, c, c + 1, (p - 1) // 2, (p + 1) // 2, last if last < p else 3]
    out = []
    for v in vals:
        v %= p
        if v not in out:
            out.append(v)
    return out


GRID_N = 8192 * 256 + 300   # the element-wise grids stop at 8192 blocks x 256 lanes: 300 elements get a second pass of the grid-stride loop
RARE = ["fold3_high_nonzero", "final_subtract", "zero_from_nonzero", "add_equals_p", "add_carry_out"]       # what random operands do not reach
GRID_BLOCK = 4099       # elements of the block the grid-stride tests tile (a prime: the block falls on other lanes in every repetition)
_STRIDE = 7919          # prime, larger than any prime factor of len(edge_operands)^4


@lru_cache(maxsize=None)
def directed_quadruples(p):
    """The full 4-fold product of edge_operands(p) as (ar, am, br, bm).  The product's own order keeps ar fixed for the first quarter, so the
    quadruples are handed out in a fixed stride through it (a permutation: the stride is coprime to the count): every prefix of a few
    thousand then mixes all four operands, which is what the grid-stride tests need from their 4 099-element block."""
    full = list(itertools.product(edge_operands(p), repeat=4))
    n = len(full)
    return tuple(full[i * _STRIDE % n] for i in range(n))


def grid_block(limbs, p, pid=1):
    """The GRID_BLOCK-element block the grid-stride tests tile over GRID_N elements: the directed quadruples in their order (repeated from the start
    where there are fewer: 2^127 - 1 has 7^4 = 2 401), with every 7th place given in turn to one representative of each rare class the model finds
    among them for this party.  Any 35 consecutive elements then take every rare branch, so the 300 elements of the second pass do."""
    quads = directed_quadruples(p)
    reps = []
    for cls in RARE:
        q = next((q for q in quads if cls in model_beaver(pid, limbs, p, *q)[1]), None)
        if q is not None and q not in reps:
            reps.append(q)
    return [reps[i // 7 % len(reps)] if i % 7 == 0 else quads[i % len(quads)] for i in range(GRID_BLOCK)]


def random_quadruples(p, count=3000, seed=0):
    rnd = random.Random((p % 1000003) * 31 + seed)
    return [tuple(rnd.randrange(p) for _ in range(4)) for _ in range(count)]


# ---- numpy packing: a field element is `limbs` little-endian 64-bit words
def to_limbs(vals, limbs):
    buf = b"".join(v.to_bytes(8 * limbs, "little") for v in vals)
    return np.frombuffer(buf, dtype="<u8").reshape(len(vals), limbs).copy()


def from_limbs(arr):
    arr = np.ascontiguousarray(arr, dtype="<u8")
    w = 8 * arr.shape[-1]
    raw = arr.tobytes()
    return [int.from_bytes(raw[i:i + w], "little") for i in range(0, len(raw), w)]


# ---- the model: field constants as field_setup() derives them
def pm_params(limbs, p):
    """(W, s, c) with p = 2^(32 W + s) - c if field_setup() selects the folded reduction, else None: the top 32-bit word is in use and every bit
    from 32 up to the top one is set, so c = 2^B - p < 2^32"""
    nw = 2 * limbs
    if p >> (32 * (nw - 1)) == 0:
        return None
    B = p.bit_length()
    if p >> 32 != (1 << (B - 32)) - 1:
        return None
    return B // 32, B % 32, (-p) & M32


def mont_consts(limbs, p):
    nw = 2 * limbs
    return pow(1 << (32 * nw), 2, p), (-pow(p, -1, 1 << 32)) & M32          # R^2 mod p, -p^-1 mod 2^32


def _mask(words):
    return (1 << (32 * words)) - 1


def pm_fold(x, nin, W, s, c, nout, cls):
    """pm_fold<NIN, W, NOUT>: x (nin words) -> (x mod 2^B) + c * (x >> B) in nout words, B = 32 W + s.  The kernel reads the high part through
    min(nin - W, nout) words and keeps nout words of the sum: what does not fit is an error class, never silently correct."""
    assert x >> (32 * nin) == 0 and nout >= W + 1
    B = 32 * W + s
    lo, H = x & ((1 << B) - 1), x >> B
    if H >> (32 * nout):
        cls.add("high_words_dropped")
        H &= _mask(nout)
    v = lo + c * H
    if v >> (32 * nout):
        cls.add("carry_lost")
        v &= _mask(nout)
    return v


def pm_fold_words(inw, W, s, c, nout):
    """the same fold word by word as the kernel writes it (funnel shift, one 32 x 32 product and a carry per output word); returns (words, carry out)"""
    nin = len(inw)
    nh = nin - W
    lowmask = (1 << s) - 1 if s else 0
    out, carry = [], 0
    for k in range(nout):
        lo = inw[k] if k < W else (inw[W] & lowmask if k == W else 0)
        h = 0
        if k < nh:
            hi = inw[W + k + 1] if W + k + 1 < nin else 0
            h = (((hi << 32) | inw[W + k]) >> s) & M32
        v = h * c + lo + carry
        out.append(v & M32)
        carry = v >> 32
    return out, carry


def model_add(limbs, p, a, b, cls, mutant=None):
    """f_add: NW-word sum, then subtract p if the sum carried out of the top word or is >= p"""
    nw = 2 * limbs
    s = a + b
    carry = s >> (32 * nw)
    s &= _mask(nw)
    if carry:
        cls.add("add_carry_out")
    elif s == p:
        cls.add("add_equals_p")
    ge = bool(carry) or (s > p if mutant == "add_no_equal" else s >= p)
    return (s - p) & _mask(nw) if ge else s


def model_mulsum_pm(limbs, p, a1, b1, a2, b2, two, cls, mutant=None):
    """f_mulsum_pm: a1*b1 (+ a2*b2) as one integer of 2 NW + 1 words, three folds (-> NW + 4 -> W + 2 -> W + 1 words), one compare-and-subtract"""
    nw = 2 * limbs
    W, s, c = pm_params(limbs, p)
    B = 32 * W + s
    T = a1 * b1 + (a2 * b2 if two else 0)
    if T >> (32 * (2 * nw + 1)):
        cls.add("carry_lost")
        T &= _mask(2 * nw + 1)
    S1 = pm_fold(T, 2 * nw + 1, W, s, c, nw + 4, cls)
    if S1 >> B:
        cls.add("fold2_high_nonzero")
    S2 = pm_fold(S1, nw + 4, W, s, c, W + 2, cls)
    if S2 >> B:
        cls.add("fold3_high_nonzero")
    if mutant == "skip_fold3":                  # the fold's line deleted: the compare reads S2's low W + 1 words
        S3 = S2 & _mask(W + 1)
    elif mutant == "drop_fold3_high":           # the fold kept, its high part never added
        S3 = S2 & ((1 << B) - 1)
    else:
        S3 = pm_fold(S2, W + 2, W, s, c, W + 1, cls)
    if S3 >> (32 * nw):                         # t[] has NW words
        cls.add("high_words_dropped")
    t = S3 & _mask(nw)
    ge = t > p if mutant == "strict_compare" else t >= p
    if ge:
        cls.add("final_subtract")
    out = (t - p) & _mask(nw) if ge else t
    if out == 0 and T != 0:
        cls.add("zero_from_nonzero")
    return out


def model_montmul(limbs, p, a, b, n0inv, cls):
    """f_montmul (CIOS on 32-bit words): the accumulator has NW + 2 words inside a round and NW + 1 after its shift"""
    nw = 2 * limbs
    t = 0
    for i in range(nw):
        t += a * ((b >> (32 * i)) & M32)
        if t >> (32 * (nw + 2)):
            cls.add("carry_lost")
            t &= _mask(nw + 2)
        m = ((t & M32) * n0inv) & M32
        t = (t + m * p) >> 32
        if t >> (32 * (nw + 1)):
            cls.add("carry_lost")
            t &= _mask(nw + 1)
    extra = t >> (32 * nw)
    if extra:
        cls.add("mont_extra_word_nonzero")
    low = t & _mask(nw)
    ge = bool(extra) or low >= p
    if ge:
        cls.add("mont_subtract")
    return (low - p) & _mask(nw) if ge else low


def model_mul(limbs, p, a, b, consts, cls):
    r2, n0inv = consts
    return model_montmul(limbs, p, model_montmul(limbs, p, a, b, n0inv, cls), r2, n0inv, cls)


def model_beaver(pid, limbs, p, ar, am, br, bm, mutant=None):
    """k_beaver_elem_pm / k_beaver_elem as sfg_beaver_elem_dev dispatches them; returns (value, set of branch classes taken)"""
    cls = set()
    if pm_params(limbs, p) is not None:
        if pid == 0:
            return model_mulsum_pm(limbs, p, am, bm, am, bm, False, cls, mutant), cls
        if pid == 1:
            t = model_add(limbs, p, bm, br, cls, mutant)
            return model_mulsum_pm(limbs, p, ar, t, br, am, True, cls, mutant), cls
        return model_mulsum_pm(limbs, p, ar, bm, br, am, True, cls, mutant), cls
    k = mont_consts(limbs, p)
    if pid == 0:
        return model_mul(limbs, p, am, bm, k, cls), cls
    if pid == 1:
        u = model_mul(limbs, p, ar, model_add(limbs, p, bm, br, cls, mutant), k, cls)
    else:
        u = model_mul(limbs, p, ar, bm, k, cls)
    t = model_mul(limbs, p, br, am, k, cls)
    return model_add(limbs, p, u, t, cls, mutant), cls
