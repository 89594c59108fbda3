"""CPU checks of tests/field_ref.py: the word-width model of beaver.hip's reductions agrees with Python integers on the directed operand set,
the set reaches the rare branches for every modulus of the table, and the set has teeth - mutants of the model (a fold's high part never
added, a strict final compare, f_add without its equality arm) are caught by it.  The GPU side is tests/test_gpu_field.py."""
from functools import lru_cache

import pytest

import field_ref as fr

CLASSES = ["fold2_high_nonzero", "fold3_high_nonzero", "final_subtract", "zero_from_nonzero", "add_equals_p", "add_carry_out",
           "mont_extra_word_nonzero", "mont_subtract", "carry_lost", "high_words_dropped"]
BIT = {c: 1 << i for i, c in enumerate(CLASSES)}
ERRORS = BIT["carry_lost"] | BIT["high_words_dropped"]
ids = lambda mods: [fr.mod_id(m) for m in mods]


@lru_cache(maxsize=None)
def run(limbs, p):
    """the model over directed + 3 000 random quadruples x pid 0, 1, 2: per pid the class bit mask of every quadruple, and the quadruples whose
    value is not expected()'s"""
    quads = list(fr.directed_quadruples(p)) + fr.random_quadruples(p)
    masks, wrong = {}, []
    for pid in (0, 1, 2):
        seen = {}
        row = []
        for q in quads:
            key = q[1::2] if pid == 0 else q              # the dealer's product reads am and bm only
            m = seen.get(key)
            if m is None:
                v, cls = fr.model_beaver(pid, limbs, p, *q)
                if v != fr.expected(pid, p, *q):
                    wrong.append((pid, q))
                m = seen[key] = sum(BIT[c] for c in cls)
            row.append(m)
        masks[pid] = row
    return quads, masks, wrong


def reached(limbs, p, cls, part="directed"):
    """number of (pid, quadruple) pairs of that part which take the branch"""
    quads, masks, _ = run(limbs, p)
    nd = len(fr.directed_quadruples(p))
    sl = slice(0, nd) if part == "directed" else slice(nd, None) if part == "random" else slice(None)
    return sum(1 for pid in masks for m in masks[pid][sl] if m & BIT[cls])


def flagged(limbs, p, cls):
    """the directed (pid, quadruple) pairs that take the branch: a mutant of that branch computes what the model computes on every other input"""
    quads, masks, _ = run(limbs, p)
    nd = len(fr.directed_quadruples(p))
    return [(pid, quads[i]) for pid in masks for i in range(nd) if masks[pid][i] & BIT[cls]]


def mutant_misses(limbs, p, mutant, cls):
    return sum(1 for pid, q in flagged(limbs, p, cls) if fr.model_beaver(pid, limbs, p, *q, mutant=mutant)[0] != fr.expected(pid, p, *q))


def test_edge_operands_and_quadruples():
    p = (1 << 255) - 19
    ops = fr.edge_operands(p)
    assert ops == [0, 1, 2, p - 1, p - 2, 1 << 254, (1 << 254) - 1, 19, 20, (p - 1) // 2, (p + 1) // 2, (1 << 255) - 38]
    assert fr.edge_operands((1 << 127) - 1) == [0, 1, 2, (1 << 127) - 2, (1 << 127) - 3, 1 << 126, (1 << 126) - 1]        # c = 1: the rest are duplicates
    for limbs, p in fr.ALL_MODULI:
        ops = fr.edge_operands(p)
        assert len(set(ops)) == len(ops) and all(0 <= v < p for v in ops)
        quads = fr.directed_quadruples(p)
        assert len(quads) == len(ops) ** 4 == len(set(quads)) and set(q[2] for q in quads) == set(ops)


def test_limb_packing_round_trips():
    vals = [0, 1, (1 << 64) - 1, 1 << 64, (1 << 255) - 19, (1 << 256) - 1]
    arr = fr.to_limbs(vals, 4)
    assert arr.shape == (6, 4) and int(arr[3, 1]) == 1 and int(arr[3, 0]) == 0 and fr.from_limbs(arr) == vals


def test_path_selection():
    """the folded form is p = 2^B - c with c < 2^32 and the top 32-bit word in use; the four kernels serve W = NW - 1 and W = NW"""
    for limbs, p in fr.FOLDED:
        W, s, c = fr.pm_params(limbs, p)
        assert (1 << (32 * W + s)) - c == p and 0 < c < 1 << 32 and W in (2 * limbs - 1, 2 * limbs) and (W < 2 * limbs or s == 0)
    for limbs, p in fr.GENERIC:
        assert fr.pm_params(limbs, p) is None
    assert {fr.pm_params(l, p)[1] for l, p in fr.FOLDED} == {0, 1, 24, 30, 31, 16}     # s = B mod 32: the funnel shift at other amounts than 31 and 0


@pytest.mark.parametrize("limbs,p", fr.ALL_MODULI, ids=ids(fr.ALL_MODULI))
def test_model_equals_python_integers(limbs, p):
    """every directed and random quadruple, pid 0, 1, 2: the model's value is expected()'s and no fold or Montgomery round loses a word or a carry"""
    quads, masks, wrong = run(limbs, p)
    assert wrong == []
    assert not any(m & ERRORS for pid in masks for m in masks[pid])


@pytest.mark.parametrize("limbs,p", fr.FOLDED, ids=ids(fr.FOLDED))
def test_fold_word_form_is_the_integer_form(limbs, p):
    """pm_fold on integers and the word loop of the kernel are the same function, on all three folds of every 5th directed quadruple (pid 1)"""
    nw = 2 * limbs
    W, s, c = fr.pm_params(limbs, p)
    words = lambda x, n: [(x >> (32 * i)) & fr.M32 for i in range(n)]
    for ar, am, br, bm in fr.directed_quadruples(p)[::5]:
        x, nin = ar * ((bm + br) % p) + br * am, 2 * nw + 1
        for nout in (nw + 4, W + 2, W + 1):
            cls = set()
            y = fr.pm_fold(x, nin, W, s, c, nout, cls)
            assert (words(y, nout), 0) == fr.pm_fold_words(words(x, nin), W, s, c, nout) and not cls
            x, nin = y, nout


@pytest.mark.parametrize("limbs,p", fr.FOLDED, ids=ids(fr.FOLDED))
def test_directed_set_reaches_the_folded_branches(limbs, p):
    for cls in ("fold2_high_nonzero", "fold3_high_nonzero", "final_subtract", "zero_from_nonzero", "add_equals_p"):
        assert reached(limbs, p, cls) > 0, cls
    if p > 1 << (64 * limbs - 1):
        assert reached(limbs, p, "add_carry_out") > 0
    else:                                                   # a + b < 2p <= 2^(32 NW): no carry out of the top word exists
        assert reached(limbs, p, "add_carry_out", "all") == 0
    # what the 3 000 random quadruples reach of these: the second fold's high part and nothing else
    for cls in ("fold3_high_nonzero", "final_subtract", "zero_from_nonzero", "add_equals_p"):
        assert reached(limbs, p, cls, "random") == 0, cls


@pytest.mark.parametrize("limbs,p", [(2, (1 << 127) - 1), (4, (1 << 255) - 19), (2, (1 << 127) - (1 << 40) - 1)], ids=["L2-folded", "L4-folded", "L2-generic"])
def test_grid_stride_second_pass_reaches_the_rare_branches(limbs, p):
    """the block test_gpu_field.py tiles past the grid's end (pid 1): the 300 elements of the second pass, GRID_N - 300 .. GRID_N - 1, take every
    rare branch of their path, and so does the first pass"""
    block = fr.grid_block(limbs, p)
    assert len(block) == fr.GRID_BLOCK and set(block) <= set(fr.directed_quadruples(p))
    want = ["fold3_high_nonzero", "final_subtract", "zero_from_nonzero", "add_equals_p"] if fr.pm_params(limbs, p) else ["add_equals_p", "mont_subtract"]
    tail, body = set(), set()
    for i in range(fr.GRID_N - 300, fr.GRID_N):
        tail |= fr.model_beaver(1, limbs, p, *block[i % fr.GRID_BLOCK])[1]
    for q in block:
        body |= fr.model_beaver(1, limbs, p, *q)[1]
    assert all(c in tail for c in want) and all(c in body for c in want)
    assert not (tail | body) & {"carry_lost", "high_words_dropped"}


@pytest.mark.parametrize("limbs,p", fr.GENERIC, ids=ids(fr.GENERIC))
def test_directed_and_random_reach_the_generic_branches(limbs, p):
    R = 1 << (64 * limbs)
    assert reached(limbs, p, "add_equals_p") > 0
    if p > R // 2:
        assert reached(limbs, p, "add_carry_out") > 0
    else:                                                   # a + b < 2p <= 2^(32 NW)
        assert reached(limbs, p, "add_carry_out", "all") == 0
    # the conditional subtraction of the Montgomery product fires for every modulus, 2^96 - 17 included (there only on directed operands:
    # t >= p needs m = -ab/p mod R within ab/p < 2^96 of R, about 2^-32 for a random product)
    assert reached(limbs, p, "mont_subtract", "all") > 0
    # the product's extra word: t = (a b + m p) / R <= ((p - 1)^2 + (R - 1) p) / R, with a, b < p (the second product's operand R^2 mod p included) and m < R
    tmax = ((p - 1) ** 2 + (R - 1) * p) // R
    _, masks, _ = run(limbs, p)
    n_all = sum(len(masks[pid]) for pid in masks)
    if tmax < R:
        # unreachable: t never needs the extra word.  True of every modulus below 2^(32 NW - 1) (t < 2p <= R), and of 0x9E37..8E95 although it is above:
        # p / R is just under 1 / golden ratio, so p (1 + p / R) < R
        assert p < R // 2 or (limbs, p) == fr.GENERIC[1]
        assert reached(limbs, p, "mont_extra_word_nonzero", "all") == 0
    else:
        assert 0 < reached(limbs, p, "mont_extra_word_nonzero", "all") < n_all                    # both outcomes
        assert (limbs, p) == fr.GENERIC[0]


@pytest.mark.parametrize("limbs,p", fr.FOLDED, ids=ids(fr.FOLDED))
def test_mutants_of_the_folded_reduction_are_caught(limbs, p):
    W, s, c = fr.pm_params(limbs, p)
    assert mutant_misses(limbs, p, "drop_fold3_high", "fold3_high_nonzero") > 0       # third fold's high part never added
    assert mutant_misses(limbs, p, "strict_compare", "final_subtract") > 0            # `>` for `>=`: t == p comes out as p
    if s == 0:
        assert mutant_misses(limbs, p, "skip_fold3", "fold3_high_nonzero") > 0        # third fold deleted: bit B = 32 NW does not fit t[]
    else:
        # Not a wrong kernel, so nothing can catch it: with s > 0 the compare's NW words hold bit B of S2 = 2^B + lo (lo is a few words, so S2 < 2p), and
        # subtracting p = 2^B - c from it gives lo + c, which is what the third fold and a compare that does not fire give.
        assert mutant_misses(limbs, p, "skip_fold3", "fold3_high_nonzero") == 0
    # f_add without its equality arm is not wrong here either: its only use on the folded path is bm + br (pid 1), which feeds the folds, and they
    # reduce ar * p + br * am as well as ar * 0 + br * am.  The generic path is where that arm decides an output word (next test).
    assert mutant_misses(limbs, p, "add_no_equal", "add_equals_p") == 0


@pytest.mark.parametrize("limbs,p", fr.GENERIC, ids=ids(fr.GENERIC))
def test_mutant_of_f_add_is_caught_on_the_generic_path(limbs, p):
    assert mutant_misses(limbs, p, "add_no_equal", "add_equals_p") > 0
