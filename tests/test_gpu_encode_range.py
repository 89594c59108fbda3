"""The real-slot encoder (sfg_encode_coeffs_host, sfg_encode_vectors_dev) and the int8 diagonal encoder (sfg_encode_diags_dev) against
tests/exactref.py - an exact encoder and NTT independent of the kernels and of the C oracle - word for word, across the coefficient range.

The real-slot encoder's domain: finite slot values and |Delta w_c| < 2^53 for every coefficient.  Inside it every coefficient and every NTT
word at every modulus must equal the reference's; outside it (and for NaN / inf) the call must raise, never return words."""
import ctypes as C

import numpy as np
import pytest

import exactref
import pyref
from sfgwas_amd.params import Q_PN14, P_PN14

pytestmark = pytest.mark.gpu
N, SLOTS, SCALE, D = 16384, 8192, 2.0 ** 34, 91
LIMIT = 2.0 ** 53
TARGETS = [34, 41, 42, 45, 47, 49, 50, 50.5, 51, 51.5, 52, 52.9]        # log2 of the coefficient magnitude aimed at
SHAPES = ["const", "single", "dense", "adv_alt", "adv_rand", "adv_same"]


def _base(shape, T):
    """a slot vector whose coefficients have magnitude ~T (units of p)"""
    rnd = np.random.default_rng(SHAPES.index(shape) + 17)
    if shape == "const":                                     # (20 fraction bits: p_0 is an integer, not an exact tie, at every 2^k multiple)
        return np.full(SLOTS, np.round(T / SCALE * 2.0 ** 20) / 2.0 ** 20)
    if shape == "single":
        v = np.zeros(SLOTS)
        v[777] = np.round(T * SLOTS / SCALE * 2.0 ** 20) / 2.0 ** 20      # (likewise for the coefficients where the cosine is +-1)
        return v
    if shape == "dense":                                     # rms |p| ~ T
        return rnd.normal(size=SLOTS) * (T * np.sqrt(2.0 * SLOTS) / SCALE)
    # adversarial: decode a pattern with every |p_c| = T (the symmetry of a real vector: p_n = 0, p_{N-c} = -p_c), keep the doubles
    half = {"adv_alt": (-1.0) ** np.arange(SLOTS), "adv_rand": rnd.choice([-1.0, 1.0], SLOTS), "adv_same": np.ones(SLOTS)}[shape]
    P = np.zeros(N)
    P[:SLOTS] = half
    P[SLOTS + 1:] = -half[1:][::-1]
    return np.ascontiguousarray(pyref.decode(P * T / SCALE, N).real)


def build_cases():
    """[{name, v, p (list of N ints), tie (min distance to a rounding tie), inside}] for every shape x target x sign.  A target 2^(k + f)
    is 2^k times the base vector at 2^(34 + f): one exact transform per (shape, f) serves every k."""
    cases = []
    for shape in SHAPES:
        for f in sorted({round(e - int(e), 3) for e in TARGETS}):
            es = [e for e in TARGETS if abs((e - int(e)) - f) < 1e-9]
            b = _base(shape, 2.0 ** (34 + f))
            refs = exactref.encode_scaled(b, N, [SCALE * 2.0 ** (int(e) - 34) for e in es])
            for e, (p, tie, err) in zip(es, refs):
                v = b * 2.0 ** (int(e) - 34)                   # exact: a power of two
                pmax = max(abs(x) for x in p)
                assert abs(pmax - LIMIT) > 1, "a case on the domain's edge"
                # far from every tie: the device must prove each rounding (its widest band, 2^-88 Sp at Sp < 2^60, is 2^-28)
                assert tie.min() > max(1e6 * err, 2.0 ** -27), (shape, e, tie.min(), err)
                for sg in (1, -1):
                    cases.append(dict(name=f"{shape}@2^{e}{'+' if sg > 0 else '-'}", v=sg * v, p=[sg * x for x in p], tie=float(tie.min()),
                                      inside=pmax < LIMIT))
    return cases


@pytest.fixture(scope="module")
def cases():
    return build_cases()


@pytest.fixture(scope="module")
def ntt_ref(cases):
    """reference NTT words [case][modulus][N] of the in-domain cases (negated vectors from their partners: NTT(-p) = -NTT(p))"""
    pos = [k for k, c in enumerate(cases) if c["inside"] and c["name"].endswith("+")]
    out = {}
    for m, q in enumerate(Q_PN14):
        w = exactref.ntt([cases[k]["p"] for k in pos], q, exactref.psi_for(q, N))
        for k, row in zip(pos, w):
            out.setdefault(k, [None] * len(Q_PN14))[m] = row
            out.setdefault(k + 1, [None] * len(Q_PN14))[m] = (np.uint64(q) - row) % np.uint64(q)
    return {k: np.stack(v) for k, v in out.items()}


@pytest.fixture(scope="module")
def ctx():
    from sfgwas_amd import capi
    c = capi.Context(Q_PN14, P_PN14)
    yield c
    c.close()


def encode_coeffs(ctx, vals):
    from sfgwas_amd import capi
    vals = np.ascontiguousarray(vals, dtype=np.float64)
    out = np.zeros((vals.shape[0], N), dtype=np.int64)
    ctx.check(capi.lib().sfg_encode_coeffs_host(ctx.h, vals.ctypes.data_as(C.POINTER(C.c_double)), vals.shape[0],
                                                out.ctypes.data_as(C.POINTER(C.c_int64))), "encode_coeffs")
    return out


def test_domain_cases_cover_both_sides(cases):
    inside = {c["name"] for c in cases if c["inside"]}
    assert {"adv_same@2^52.9+", "const@2^52.9-", "adv_rand@2^52+"} <= inside
    assert {c["name"] for c in cases} - inside >= {"dense@2^51.5+", "dense@2^52.9-"}


def test_coeffs_in_domain_match_exactref(ctx, cases):
    """every in-domain vector in ONE call (mixed magnitudes 2^34 .. 2^52.9), every coefficient"""
    inn = [c for c in cases if c["inside"]]
    got = encode_coeffs(ctx, np.stack([c["v"] for c in inn]))
    bad = [c["name"] for c, g in zip(inn, got) if [int(x) for x in g] != c["p"]]
    assert not bad, f"coefficients differ from the exact encoder: {bad}"
    ctx.sync()                                                 # and no rounding was left unproven


def test_ntt_words_in_domain_match_exactref_every_modulus(ctx, cases, ntt_ref):
    """EncodeFloatVector at the top level: the 46-bit q0 and every 35/36-bit modulus, word for word"""
    idx = sorted(ntt_ref)
    got = ctx.encode_vectors(np.stack([cases[k]["v"] for k in idx]), len(Q_PN14) - 1)
    bad = [(cases[k]["name"], m) for j, k in enumerate(idx) for m in range(len(Q_PN14)) if not np.array_equal(got[j, m], ntt_ref[k][m])]
    assert not bad, f"NTT words differ from the exact reference (case, modulus): {bad}"
    ctx.sync()


@pytest.mark.parametrize("level", [0, 1, 5])
def test_lower_levels_are_the_reference_rows(ctx, cases, ntt_ref, level):
    names = ["const@2^52.9+", "adv_same@2^52.9-", "adv_alt@2^52+", "single@2^51.5+", "dense@2^47-"]
    idx = [k for k, c in enumerate(cases) if c["name"] in names]
    assert len(idx) == len(names)
    got = ctx.encode_vectors(np.stack([cases[k]["v"] for k in idx]), level)
    for j, k in enumerate(idx):
        assert np.array_equal(got[j], ntt_ref[k][:level + 1]), cases[k]["name"]


def test_out_of_domain_raises(ctx, cases):
    """|Delta w_c| >= 2^53: both entry points refuse, alone and in a call with in-domain vectors; the context stays usable"""
    from sfgwas_amd import capi
    out = [c for c in cases if not c["inside"]]
    assert out
    vecs = [c["v"] for c in out]
    vecs += [np.full(SLOTS, 2.0 ** 19), -np.full(SLOTS, 2.0 ** 19 + 2.0 ** -20), np.full(SLOTS, 1e200)]       # p_0 = 2^53, just above, far above
    one = np.zeros(SLOTS)
    one[5] = 2.0 ** 54 * SLOTS / SCALE
    vecs.append(one)
    for v in vecs:
        with pytest.raises(capi.SfgError, match="2\\^53"):
            encode_coeffs(ctx, v[None])
        with pytest.raises(capi.SfgError, match="2\\^53"):
            ctx.encode_vectors(v[None], 3)
    good = next(c for c in cases if c["inside"] and c["name"].startswith("adv_rand@2^50.5"))
    with pytest.raises(capi.SfgError, match="2\\^53"):
        ctx.encode_vectors(np.stack([good["v"], out[0]["v"], good["v"]]), 2)
    got = encode_coeffs(ctx, good["v"][None])
    assert [int(x) for x in got[0]] == good["p"]
    ctx.sync()


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_non_finite_slot_values_raise(ctx, bad):
    from sfgwas_amd import capi
    v = np.random.default_rng(3).normal(size=(2, SLOTS))
    v[1, 4321] = bad
    with pytest.raises(capi.SfgError, match="not finite"):
        encode_coeffs(ctx, v)
    with pytest.raises(capi.SfgError, match="not finite"):
        ctx.encode_vectors(v, 1)
    got = encode_coeffs(ctx, v[:1])                           # the next call starts clean
    assert [int(x) for x in got[0]] == exactref.encode(v[0], N, SCALE)[0]
    ctx.sync()


# ---------------------------------------------------------------- int8 extremes through sfg_encode_diags_dev (the fixed-grid FFT)
def _pattern(name):
    i = np.arange(SLOTS, dtype=np.int64)[:, None]
    j = np.arange(SLOTS, dtype=np.int64)[None, :]
    if name == "all127":
        return np.full((SLOTS, SLOTS), 127, dtype=np.int8)
    if name == "col_alt":                                   # 127 / -128 by column (missing -> 0 on the way in)
        return np.ascontiguousarray(np.broadcast_to(np.where(j % 2 == 0, 127, -128).astype(np.int8), (SLOTS, SLOTS)))
    if name == "stripes":
        return np.where((i * 7 + j * 3) % 5 < 3, 127, -127).astype(np.int8)
    return np.random.default_rng(5).choice(np.array([127, -128, -127, 0, 1], dtype=np.int8), (SLOTS, SLOTS))


@pytest.mark.parametrize("name", ["all127", "col_alt", "stripes", "rand"])
def test_encode_diags_int8_extremes_match_exactref(ctx, name):
    X = _pattern(name)
    L = len(Q_PN14)
    for shift0, nshift in [(0, 2), (90, 2), (8190, 2)]:
        got = ctx.encode_diags(X, shift0, nshift, L)
        for k in range(nshift):
            s = shift0 + k
            diag = X[(s + np.arange(SLOTS)) % SLOTS, np.arange(SLOTS)].astype(np.float64)
            diag[diag < 0] = 0.0                                                   # missing calls are zero
            p = exactref.encode(np.roll(diag, D * (s // D)), N, SCALE)[0]
            want = np.stack([exactref.ntt([p], q, exactref.psi_for(q, N))[0] for q in Q_PN14])
            assert np.array_equal(got[k], want), f"{name} shift {s}"
    ctx.sync()
