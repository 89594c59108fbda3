"""The general ring's matrix products (sfgwas_amd/csrc/gring_matmul.hip, capi.Ring.matmul*) on the GPU, every word compared for equality with the CPU oracle's
orc_matmult_accumulate / orc_matmult_finalize / orc_matmult4stream on the chains of tests/ring_cases.py (shapes and expectations: tests/ring_mm_cases.py):
accumulator, active giants and output on a small block; a full 2048 x 2048 block plain, transposed and squared; ragged blocks, single rows and columns and the sums
nr + nc around `slots`; the level drop; logN 15 and 16; 61-bit words, where the expectation past the reference's wrapping sum is the range sum and partial accumulators
must add up; 19 moduli against the composition of the ring's other entry points; PN14's parameters against the specialised Context; chunks of ciphertexts and batches
of diagonals forced by the budget; guard bands round out and acc; two parties end to end; every refusal with its message.
Keys: oracle_lib.RotKeys.gen_for_rotations over oracle_lib.needed_rotations at logN 12 and 13, over the rotations the shape needs (ring_mm_cases.rotations) at
logN 14 - 16, where all 2 (d - 1) keys would take the oracle a minute.  One device ring, one oracle ring and one key set per chain for the module."""
import atexit
import ctypes as C
import os

import numpy as np
import pytest

import oracle_lib as ol
import ring_cases as rc
import ring_io_ref as rio
import ring_mm_cases as mc
import ring_ref
from sfgwas_amd import capi

pytestmark = pytest.mark.gpu

SCALE = mc.SCALE
SQ, TR = capi.SFG_SQUARE, capi.SFG_TRANSPOSE
_ENV = {}
_SHARED = {}


class Env(mc.Party):
    def __init__(self, name):
        super().__init__(name)
        self.dev = capi.Ring(self.logN, self.q, self.p)

    def keys_for(self, nrow, ncol):
        """the operand's keys, on both sides"""
        rots = ol.needed_rotations(self.slots, nrow, ncol)[0] if self.logN <= 13 else mc.rotations(nrow, ncol, self.slots)
        self.need(rots, self.dev.load_rotkey)


def env(name):
    if name not in _ENV:
        _ENV[name] = Env(name)
    return _ENV[name]


@atexit.register
def _close_all():
    for e in _ENV.values():
        e.dev.close()
    _ENV.clear()


def check_product(e, s, nrow, ncol, in_level, max_level, seed, flags=0, geno=None, scale=SCALE):
    """device product of a seeded matrix against the oracle's on the operand it states (its transpose for SFG_TRANSPOSE)"""
    geno = mc.geno_matrix(nrow, ncol, seed) if geno is None else geno
    view = np.ascontiguousarray(geno.T) if flags & TR else geno
    e.keys_for(*view.shape)
    A = mc.inputs(e.ring, s, mc.blocks(view.shape[0], e.slots), in_level, 1000 + seed)
    got = e.dev.matmul(A, in_level, max_level, geno, scale, flags)
    want = mc.orc_product(e.ring, e.keys, A, in_level, max_level, view, square=bool(flags & SQ), scale=scale)
    assert got.shape == want.shape
    assert np.array_equal(got, want), (e.name, nrow, ncol, flags, int(np.count_nonzero(got != want)))
    return A, geno, got


# ---------------------------------------------------------------- G12
def test_g12_accumulator_active_giants_output_and_finalize_of_accumulate():
    e = env("G12")
    e.keys_for(100, 100)
    geno = mc.geno_matrix(100, 100, 1)
    A = mc.inputs(e.ring, 2, 1, 1, 10)
    acc, active = e.dev.matmul_accumulate(A, 1, 2, geno, SCALE)
    want_acc, want_active = mc.orc_accumulate(e.ring, e.keys, A, 1, 2, geno)
    assert np.array_equal(active, want_active) and 0 < active.sum() < e.d
    assert np.array_equal(acc, want_acc)
    assert not acc[:, active == 0].any()
    out = e.dev.matmul(A, 1, 2, geno, SCALE)
    assert np.array_equal(out, mc.orc_product(e.ring, e.keys, A, 1, 2, geno))
    assert np.array_equal(e.dev.matmul_finalize(acc, active, 2), out)
    # the finalize in two giant ranges, the second added to the first
    half = e.dev.matmul_finalize(acc, active, 2, 0, 20)
    assert np.array_equal(e.dev.matmul_finalize(acc, active, 2, 20, e.d, into=half), out)
    assert np.array_equal(half, mc.orc_finalize(e.ring, e.keys, want_acc, want_active, 2, 0, 20))


@pytest.mark.parametrize("flags", [0, TR, SQ], ids=["plain", "transpose", "square"])
def test_g12_one_full_block_every_shift(flags):
    """2048 x 2048: every shift exists, 45 giants, the last with 24 babies because 46^2 > 2048"""
    e = env("G12")
    baby, giant, shift = mc.shift_tables(2048, 2048, e.slots, 0)
    assert shift.all() and giant.sum() == 45 and int(shift[44 * 46:].sum()) == 24
    if "full" not in _SHARED:
        _SHARED["full"] = (mc.geno_matrix(2048, 2048, 2), np.random.default_rng(3).integers(-128, 128, (2048, 2048)).astype(np.int8))
    geno = _SHARED["full"][1 if flags & SQ else 0]                        # the square on arbitrary int8 values: products that wrap
    check_product(e, 1, 2048, 2048, 1, 2, 20, flags, geno)


@pytest.mark.parametrize("nrow,ncol,flags", [(2078, 2065, 0), (2078, 2065, TR), (1, 300, 0), (300, 1, 0), (300, 1, TR), (1000, 1048, 0), (1000, 1049, 0), (1049, 1000, SQ | TR)])
def test_g12_ragged_blocks_single_rows_and_the_sums_round_slots(nrow, ncol, flags):
    check_product(env("G12"), 1, nrow, ncol, 1, 2, 30 + nrow % 7, flags)


# ---------------------------------------------------------------- G13, W15, W16
@pytest.mark.parametrize("in_level,max_level", [(5, 3), (3, 3)])
def test_g13_three_ciphertexts_with_and_without_the_level_drop(in_level, max_level):
    check_product(env("G13"), 3, 300, 200, in_level, max_level, 40)


def test_w15_a_row_that_spans_workgroups():
    e = env("W15")
    assert e.d == 128
    check_product(e, 1, 40, 60, 3, 3, 50)


def test_w16_the_largest_row():
    e = env("W16")
    assert e.d == 182
    check_product(e, 1, 20, 30, 2, 3, 60)


# ---------------------------------------------------------------- X12: 61-bit words
def test_x12_one_block_row():
    check_product(env("X12"), 1, 50, 60, 2, 2, 70)


def x12_eight_rows(e):
    if "x12" not in _SHARED:
        nrow, ncol = 8 * e.slots, 8
        e.keys_for(nrow, ncol)
        geno = mc.geno_matrix(nrow, ncol, 5)
        A = mc.inputs(e.ring, 1, 8, 2, 900)
        _SHARED["x12"] = (geno, A, mc.range_sum_accumulate(e.ring, e.keys, A, 2, 2, geno))
    return _SHARED["x12"]


def test_x12_eight_block_rows_equal_the_range_sum_where_the_reference_wraps():
    e = env("X12")
    assert all(mc.fold_terms(q) < 8 * 46 for q in e.q[:2])
    geno, A, (want_acc, want_active) = x12_eight_rows(e)
    acc, active = e.dev.matmul_accumulate(A, 2, 2, geno, SCALE)
    assert np.array_equal(active, want_active) and np.array_equal(acc, want_acc)
    assert np.array_equal(e.dev.matmul(A, 2, 2, geno, SCALE), mc.orc_finalize(e.ring, e.keys, want_acc, want_active, 2))


def test_x12_partial_accumulators_of_block_row_ranges_add_up_to_the_whole():
    """the contract orc_matmult_accumulate documents, at ranges of 1, 2 and 8 block rows"""
    e = env("X12")
    geno, A, (want_acc, want_active) = x12_eight_rows(e)
    for step in (1, 2, 8):
        total, seen = None, np.zeros(e.d, np.uint8)
        for b0 in range(0, 8, step):
            acc, active = e.dev.matmul_accumulate(A, 2, 2, geno, SCALE, b0=b0, b1=b0 + step)
            total = acc if total is None else mc.add_mod(total, acc, e.ring.moduli)
            seen |= active
        assert np.array_equal(total, want_acc) and np.array_equal(seen, want_active), step


def test_x15_a_giant_with_more_babies_than_fold_terms_takes_the_fold():
    """1 x 128 at logN 15 (d = 128): giant 127 holds babies 1 .. 127, so a thread sums 127 products of 61-bit words and folds after the 64th.  Two expectations:
    the composition of the ring's other entry points, exact modulo q whatever the term count, and the oracle, whose own 128-bit sum stays below 2^128 on these
    uniform words (127 terms of mean q^2 / 4 are about 2^127).  What the fold must not do is change the words; that an absent or late fold is wrong is held on
    the CPU on near-maximal words (tests/test_ring_mm_plan.py), which uniform ciphertexts never are."""
    e = env("X15")
    assert e.d == 128 and all(mc.fold_terms(q) == 64 for q in e.q)
    baby, giant, shift = mc.shift_tables(1, 128, e.slots, 0)
    assert int(shift[127 * 128:].sum()) == 127 and giant.sum() == 2
    A, geno, got = check_product(e, 1, 1, 128, 2, 2, 75)
    assert np.array_equal(got, mc.composed_product(e.dev, A, 2, 2, geno))


# ---------------------------------------------------------------- L19: more moduli than one oracle ring holds
def test_l19_seventeen_moduli_equal_the_composition_of_the_rings_other_entry_points():
    """no oracle ring holds 19 moduli: the expectation is the same product composed from rotate_right, encode_vectors, mul_plain and add, each of which
    tests/test_gpu_ring.py and tests/test_gpu_ring_io.py hold on this chain (the rotation against the Python-integer key switch of tests/ring_ref.py)"""
    logN, q, p = rc.chain("L19")
    dev = capi.Ring(logN, q, p)
    try:
        ring = ring_ref.SplitRing(logN, q, p)
        nrow, ncol = 3, 4                                                  # six shifts: babies 0, 1, 2 of giant 0 and 21, 22, 23 of giant 44
        for k in mc.rotations(nrow, ncol, dev.slots):
            g = ring.galois(k)
            dev.load_rotkey(g, ring_ref.uniform_key(ring, 300 + g))
        geno = mc.geno_matrix(nrow, ncol, 80)
        A = np.stack([np.stack([ring_ref.uniform_ct(ring, 16, 81 + i)]) for i in range(2)])
        got = dev.matmul(A, 16, 17, geno, SCALE)
        assert got.shape == (2, 1, 2, 17, dev.N)
        assert np.array_equal(got, mc.composed_product(dev, A, 16, 17, geno))
    finally:
        dev.close()


# ---------------------------------------------------------------- P14: both paths on the same parameters
def test_p14_equals_the_specialised_context_and_the_oracle():
    e = env("P14")
    A, geno, got = check_product(e, 1, 300, 200, 9, 9, 90, scale=2.0 ** 34)
    ctx = capi.Context(e.q, e.p)
    try:
        for g, key in e.keys.keys.items():
            ctx.load_rotkey(g, key)
        assert np.array_equal(ctx.matmul_stream(A, 9, 9, geno)[0], got)
    finally:
        ctx.close()


# ---------------------------------------------------------------- chunks
def test_chunks_of_ciphertexts_and_batches_of_diagonals_give_the_unsplit_words():
    """a budget of six diagonals' bytes: half of it holds a batch of three diagonals, what is left not one ciphertext, so s = 3 runs in three chunks of one, every
    giant's diagonals in batches of three, and the key switches one to a chunk"""
    e = env("G12")
    e.keys_for(100, 100)
    geno = mc.geno_matrix(100, 100, 6)
    A = mc.inputs(e.ring, 3, 1, 1, 600)
    whole = e.dev.matmul(A, 1, 2, geno, SCALE)
    acc_whole, active = e.dev.matmul_accumulate(A, 1, 2, geno, SCALE)
    assert np.array_equal(whole, mc.orc_product(e.ring, e.keys, A, 1, 2, geno))
    N = e.N
    per_vec = ((N // 2) * 4 + 2 * N + 4) * 8                               # gring_matmul_plan.hpp: the DFT points, L = 2 plaintext rows and the tables of one diagonal
    try:
        e.dev.set_ws_budget_for_test(6 * per_vec)
        assert np.array_equal(e.dev.matmul(A, 1, 2, geno, SCALE), whole)
        acc, act = e.dev.matmul_accumulate(A, 1, 2, geno, SCALE)
        assert np.array_equal(acc, acc_whole) and np.array_equal(act, active)
        assert np.array_equal(e.dev.matmul_finalize(acc, act, 2), whole)
    finally:
        e.dev.close()                                                       # the budget is the ring's: the next test makes its own
        del _ENV["G12"]


# ---------------------------------------------------------------- buffer bounds
GUARD = 4096
SENT = np.uint64(0xA5A5A5A5A5A5A5A5)


def guarded(dev, words):
    """a sentinel-filled buffer of `words` words between two guard bands -> (allocation, pointer to the words)"""
    base = dev.to_device(np.full(words + 2 * GUARD, SENT, dtype=np.uint64))
    return base, C.c_void_p(base.value + GUARD * 8)


def test_nothing_is_written_outside_out_and_acc_and_inactive_giants_are_zero():
    e = env("G12")
    nrow, ncol = 2078, 2065
    e.keys_for(nrow, ncol)
    L_ = capi.lib()
    geno = mc.geno_matrix(nrow, ncol, 7)
    A = mc.inputs(e.ring, 2, 2, 1, 700)
    s, m_ct, d, N, ml = 2, 2, e.d, e.N, 2
    outw, accw = s * m_ct * 2 * ml * N, m_ct * d * s * 2 * ml * N
    dA, dG = e.dev.to_device(A), e.dev.to_device(geno)
    out_base, out = guarded(e.dev, outw)
    acc_base, acc = guarded(e.dev, accw)
    try:
        active = np.zeros(d, dtype=np.uint8)
        e.dev.check(L_.sfg_ring_matmul_dev(e.dev.h, dA, s, 1, ml, dG, nrow, ncol, ncol, 0, SCALE, out), "matmul")
        e.dev.check(L_.sfg_ring_matmul_accumulate_dev(e.dev.h, dA, s, 1, ml, dG, nrow, ncol, ncol, 0, SCALE, 0, 2, acc, active.ctypes.data_as(C.POINTER(C.c_uint8))), "accumulate")
        ho, ha = e.dev.to_host(out_base, (outw + 2 * GUARD,)), e.dev.to_host(acc_base, (accw + 2 * GUARD,))
        for h in (ho, ha):
            assert (h[:GUARD] == SENT).all() and (h[-GUARD:] == SENT).all()
        got_out, got_acc = ho[GUARD:-GUARD].reshape(s, m_ct, 2, ml, N), ha[GUARD:-GUARD].reshape(m_ct, d, s, 2, ml, N)
        want_acc, want_active = mc.orc_accumulate(e.ring, e.keys, A, 1, ml, geno)
        assert np.array_equal(active, want_active) and np.array_equal(got_acc, want_acc) and not got_acc[:, active == 0].any()
        assert np.array_equal(got_out, mc.orc_finalize(e.ring, e.keys, want_acc, want_active, ml))
        # the finalize into a guarded buffer, and one block row of the accumulate: the rest of acc is zero, not the sentinel
        e.dev.check(L_.sfg_ring_memcpy_h2d(e.dev.h, out_base, np.full(outw + 2 * GUARD, SENT, dtype=np.uint64).ctypes.data_as(C.c_void_p), (outw + 2 * GUARD) * 8), "refill")
        e.dev.check(L_.sfg_ring_matmul_finalize_dev(e.dev.h, acc, active.ctypes.data_as(C.POINTER(C.c_uint8)), s, ml, m_ct, 0, d, 0, out), "finalize")
        ho = e.dev.to_host(out_base, (outw + 2 * GUARD,))
        assert (ho[:GUARD] == SENT).all() and (ho[-GUARD:] == SENT).all() and np.array_equal(ho[GUARD:-GUARD].reshape(got_out.shape), got_out)
    finally:
        for p_ in (dA, dG, out_base, acc_base):
            e.dev.free(p_)


# ---------------------------------------------------------------- end to end
def test_end_to_end_encrypt_multiply_and_decrypt_between_two_parties():
    """W15: a vector v of 40 values in (-1, 1) encrypted on the device at scale 2^40, multiplied by a 40 x 60 matrix X with entries in {0, 1, 2} whose diagonals
    are encoded at scale 2^30, decrypted by two parties from additive key shares and decoded at scale 2^70 (Q_2 = q0 q1 q2 is about 2^130): slot j < 60 holds (v X)_j.
    The bound, derived as tests/test_gpu_ring_io.py derives its own on the same chain (N = 2^15):
      * a rotated ciphertext carries the fresh encryption's 2^8.5 and a key switch's 2^10 per coefficient: 2^10.5;
      * a diagonal has at most 40 non-zero entries <= 2, so its plaintext's coefficients are about 2^30 sqrt(40 * 4) / (N / 2) = 2^19.7 (2^22.3 at the very worst);
      * a coefficient of noise x plaintext sums N terms of random sign: sqrt(N) 2^10.5 2^19.7 = 2^37.7; at most 99 diagonals add as sqrt(99) < 2^3.4: 2^41;
      * a slot sums N coefficients, sqrt(N) = 2^7.5: 2^48.5; four deviations: 2^50.5; over the output scale 2^70: 2^-19.5;
      * the encoder's rounding, 1/2 a coefficient of every plaintext against message coefficients of about 2^28, stays below that: sqrt(N) 2^28 2^-1 sqrt(99) = 2^38;
      * the giant rotations add 2^10 and the two shares at most 4 per coefficient, at scale 2^70 nothing.
    2^-16 leaves a factor of eight."""
    e = env("W15")
    nrow, ncol = 40, 60
    e.keys_for(nrow, ncol)
    s_, pk = rio.keypair(e.ring, 1234)
    assert np.array_equal(s_, e.secret)
    e.dev.load_public_key(pk)
    e.dev.seed_encryptor(bytes(range(32)))
    rnd = np.random.default_rng(8)
    geno = rnd.integers(0, 3, (nrow, ncol)).astype(np.int8)
    v = np.zeros(e.slots)
    v[:nrow] = rnd.uniform(-1, 1, nrow)
    ct_scale = 2.0 ** 40
    ct = e.dev.encrypt_vectors(v[None], 3, ct_scale)
    out = e.dev.matmul(ct[:, None], 3, 3, geno, SCALE)[0]                   # [m_ct = 1][2][3][N] at level 2
    lvl, out_scale = 2, ct_scale * SCALE
    agg = None
    for share in rio.split_secret(e.secret, 11):
        e.dev.load_secret_key(rio.sk_rows(e.ring, share))
        h0, _ = e.dev.pcks_gen_share(out, lvl, rnd.integers(-38, 39, (1, e.N)).astype(np.int32))
        agg = h0 if agg is None else np.stack([np.stack([(agg[0][m] + h0[0][m]) % np.uint64(e.ring.moduli[m]) for m in range(lvl + 1)])])
    re = e.dev.decode_vectors(e.dev.pcks_finish(out, lvl, agg), lvl, out_scale)
    want = np.zeros(e.slots)
    want[:ncol] = v[:nrow] @ geno.astype(np.float64)
    err = float(np.max(np.abs(re[0] - want)))
    print(f"W15 product: slot error {err:.3e}")
    assert err < 2.0 ** -16


# ---------------------------------------------------------------- refusals
def test_every_refusal_names_its_cause_and_writes_nothing():
    e = env("G12")
    nrow, ncol = 100, 100
    e.keys_for(nrow, ncol)
    L_ = capi.lib()
    N, d = e.N, e.d
    geno = mc.geno_matrix(nrow, ncol, 9)
    A = mc.inputs(e.ring, 1, 1, 1, 800)
    outw, accw = 2 * 2 * N, d * 2 * 2 * N
    # one buffer holds A and the matrix so that overlaps can be stated; out and acc are sentinel-filled
    dA, dG = e.dev.to_device(A), e.dev.to_device(geno)
    dout, dacc = e.dev.to_device(np.full(outw, SENT, dtype=np.uint64)), e.dev.to_device(np.full(accw, SENT, dtype=np.uint64))
    act = (C.c_uint8 * d)()

    def mm(A_=dA, s=1, il=1, ml=2, G=dG, nr=nrow, nc=ncol, ld=ncol, flags=0, scale=SCALE, out=dout):
        return L_.sfg_ring_matmul_dev(e.dev.h, A_, s, il, ml, G, nr, nc, ld, flags, scale, out)

    def ac(A_=dA, s=1, il=1, ml=2, G=dG, nr=nrow, nc=ncol, ld=ncol, flags=0, scale=SCALE, b0=0, b1=1, acc=dacc):
        return L_.sfg_ring_matmul_accumulate_dev(e.dev.h, A_, s, il, ml, G, nr, nc, ld, flags, scale, b0, b1, acc, act)

    def fin(acc=dacc, s=1, ml=2, m_ct=1, g0=0, g1=d, out=dout):
        return L_.sfg_ring_matmul_finalize_dev(e.dev.h, acc, None, s, ml, m_ct, g0, g1, 0, out)

    def refused(rc_, text):
        msg = L_.sfg_ring_last_error(e.dev.h).decode()
        assert rc_ == 1 and text in msg, (rc_, text, msg)

    try:
        for call in (mm, ac):
            refused(call(s=0), "s = 0 must be positive")
            refused(call(s=-1), "must be positive")
            refused(call(nr=0), "at least one row and one column")
            refused(call(nc=0), "at least one row and one column")
            refused(call(ld=ncol - 1), "ld 99 is below ncol 100")
            refused(call(il=2), "in_level 2 out of range 0..1")
            refused(call(il=-1), "in_level -1 out of range")
            refused(call(ml=0), "max_level 0 must be at least 1")
            refused(call(ml=3), "max_level 3 out of range 1..2")
            refused(call(il=0, ml=2), "in_level 0 leaves 1 moduli")
            refused(call(flags=4), "unknown flag bits 0x4")
            for bad in (0.5, 0.0, -2.0, float("nan"), float("inf")):
                refused(call(scale=bad), "must be finite and at least 1")
            refused(call(A_=None), "null ciphertexts or matrix")
            refused(call(G=None), "null ciphertexts or matrix")
            refused(call(G=dA), "the matrix overlaps A")
        refused(mm(out=dA), "out overlaps A")
        refused(mm(out=None), "null output")
        refused(ac(acc=dA), "acc overlaps A")
        refused(ac(acc=None), "null accumulator")
        refused(ac(b0=-1), "block rows [-1, 1) out of range 0..1")
        refused(ac(b1=2), "block rows [0, 2) out of range 0..1")
        refused(ac(b0=1, b1=0), "block rows [1, 0) out of range")
        refused(fin(g0=-1), "giants [-1, 46) out of range 0..46")
        refused(fin(g1=d + 1), "giants [0, 47) out of range")
        refused(fin(g0=3, g1=2), "giants [3, 2) out of range")
        refused(fin(s=0), "must be positive")
        refused(fin(m_ct=0), "must be positive")
        refused(fin(ml=0), "max_level 0 out of range 1..2")
        refused(fin(ml=3), "max_level 3 out of range 1..2")
        refused(fin(out=dacc), "out overlaps acc")
        refused(fin(acc=None), "null accumulator or output")
        # a missing key, one baby and one giant in turn: a ring that holds all the keys but that one
        rots = mc.rotations(nrow, ncol, e.slots)
        baby, giant = next(k for k in rots if 1 < k < d), next(k for k in rots if k >= d)
        for missing in (baby, giant):
            other = capi.Ring(e.logN, e.q, e.p)
            try:
                for k in rots:
                    if k != missing:
                        other.load_rotkey(e.ring.galois(k), e.keys.keys[e.ring.galois(k)])
                oA, oG, oout = other.to_device(A), other.to_device(geno), other.to_device(np.full(outw, SENT, dtype=np.uint64))
                assert L_.sfg_ring_matmul_dev(other.h, oA, 1, 1, 2, oG, nrow, ncol, ncol, 0, SCALE, oout) == 1
                assert f"no key loaded for the left rotation by {missing}" in L_.sfg_ring_last_error(other.h).decode()
                assert (other.to_host(oout, (outw,)) == SENT).all()
                if missing == giant:                                        # the accumulate needs no giant key; the finalize of an accumulator does
                    oacc = other.to_device(np.zeros(accw, dtype=np.uint64))
                    assert L_.sfg_ring_matmul_accumulate_dev(other.h, oA, 1, 1, 2, oG, nrow, ncol, ncol, 0, SCALE, 0, 1, oacc, act) == 0
                    assert L_.sfg_ring_matmul_finalize_dev(other.h, oacc, act, 1, 2, 1, 0, d, 0, oout) == 1
                    assert f"no key loaded for the left rotation by {missing}" in L_.sfg_ring_last_error(other.h).decode()
                    assert (other.to_host(oout, (outw,)) == SENT).all()
                else:
                    oacc = other.to_device(np.full(accw, SENT, dtype=np.uint64))
                    assert L_.sfg_ring_matmul_accumulate_dev(other.h, oA, 1, 1, 2, oG, nrow, ncol, ncol, 0, SCALE, 0, 1, oacc, act) == 1
                    assert f"no key loaded for the left rotation by {missing}" in L_.sfg_ring_last_error(other.h).decode()
                    assert (other.to_host(oacc, (accw,)) == SENT).all()
                for p_ in (oA, oG, oout, oacc):
                    other.free(p_)
            finally:
                other.close()
        # the encoder's contract: a scale that takes a coefficient outside |p| < 2^62 fails the call with the encoder's message and leaves out untouched
        refused(mm(scale=2.0 ** 70), "coefficients are outside the domain |p| < 2^62")
        # nothing above wrote a word
        assert (e.dev.to_host(dout, (outw,)) == SENT).all() and (e.dev.to_host(dacc, (accw,)) == SENT).all()
        assert np.array_equal(e.dev.to_host(dA, A.shape), A)
    finally:
        for p_ in (dA, dG, dout, dacc):
            e.dev.free(p_)
    # the budget hook without the switch
    saved = os.environ.pop("SFG_ENABLE_TEST_HOOKS", None)
    try:
        plain = capi.Ring(e.logN, e.q, e.p)
    finally:
        if saved is not None:
            os.environ["SFG_ENABLE_TEST_HOOKS"] = saved
    try:
        with pytest.raises(capi.SfgError, match="test hook, enabled only"):
            plain.set_ws_budget_for_test(1 << 20)
    finally:
        plain.close()
