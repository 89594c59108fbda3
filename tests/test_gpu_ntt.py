"""GPU parity: NTT / inverse NTT rows through the C-ABI vs the CPU oracle (bit-exact)."""
import numpy as np
import pytest

import oracle_lib as ol

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    from sfgwas_amd import capi
    ctx = capi.Context(ol.Q_PN14, ol.P_PN14)
    ring = ol.Ring(14, ol.Q_PN14, ol.P_PN14)
    yield ctx, ring
    ctx.close()


def test_ntt_rows_bit_exact(env):
    ctx, ring = env
    rnd = np.random.default_rng(1)
    nmod = len(ring.moduli)
    mods = list(range(nmod))
    rows = np.stack([rnd.integers(0, ring.moduli[m], ring.N, dtype=np.uint64) for m in mods])
    # edge values: 0, q-1
    rows[:, 0] = 0
    for m in mods:
        rows[m, 1] = ring.moduli[m] - 1
    got = ctx.ntt_rows(rows, mods)
    for m in mods:
        assert np.array_equal(got[m], ring.ntt(m, rows[m])), f"forward NTT differs for modulus {m}"
    back = ctx.ntt_rows(got, mods, inverse=True)
    assert np.array_equal(back, rows)
    inv = ctx.ntt_rows(rows, mods, inverse=True)
    for m in mods:
        assert np.array_equal(inv[m], ring.intt(m, rows[m])), f"inverse NTT differs for modulus {m}"


def test_ntt_all_max_rows(env):
    ctx, ring = env
    mods = [0, 1, 10, 11]
    rows = np.stack([np.full(ring.N, ring.moduli[m] - 1, dtype=np.uint64) for m in mods])
    got = ctx.ntt_rows(rows, mods)
    inv = ctx.ntt_rows(rows, mods, inverse=True)
    for i, m in enumerate(mods):
        assert np.array_equal(got[i], ring.ntt(m, rows[i]))
        assert np.array_equal(inv[i], ring.intt(m, rows[i]))


# ---------------------------------------------------------------- directed rows, on PN14 and on the all-47-bit chain S4 (tests/ksw_ref.py)
import ksw_ref as kr  # noqa: E402

NTT_CHAINS = ["PN14", "S4"]


def _both_ways(ctx, ring, rows, mods):
    """forward and inverse transform of every row on the device, each against the oracle's integer NTT; returns (forward, inverse)"""
    got, inv = ctx.ntt_rows(rows, mods), ctx.ntt_rows(rows, mods, inverse=True)
    for i, m in enumerate(mods):
        assert np.array_equal(got[i], ring.ntt(m, rows[i])), f"forward, modulus {m}, row {i}"
        assert np.array_equal(inv[i], ring.intt(m, rows[i])), f"inverse, modulus {m}, row {i}"
    return got, inv


@pytest.mark.parametrize("name", NTT_CHAINS)
def test_ntt_extreme_rows_every_modulus(name):
    """rows of all q - 1 (the largest lazy sums) and rows alternating q - 1 and 0, over every modulus of the chain"""
    ctx, ring = kr.gpu_env(name)
    mods = list(range(len(ring.moduli))) * 2
    rows = np.stack([np.full(ring.N, ring.moduli[m] - 1, dtype=np.uint64) for m in mods])
    rows[len(ring.moduli):, 1::2] = 0
    _both_ways(ctx, ring, rows, mods)


@pytest.mark.parametrize("name", NTT_CHAINS)
def test_ntt_single_deltas(name):
    """one non-zero coefficient (1, and q - 1 at the last position) at 0, 1, 511, 512 and N - 1: a spectrum of twiddle powers"""
    ctx, ring = kr.gpu_env(name)
    pos = [0, 1, 511, 512, ring.N - 1]
    nmod = len(ring.moduli)
    mods = list(range(nmod)) * (len(pos) + 1)                  # row i: modulus i % nmod, delta i // nmod
    rows = np.zeros((len(mods), ring.N), dtype=np.uint64)
    for i, m in enumerate(mods):
        k = i // nmod
        rows[i, pos[min(k, len(pos) - 1)]] = 1 if k < len(pos) else ring.moduli[m] - 1
    _both_ways(ctx, ring, rows, mods)


@pytest.mark.parametrize("name", NTT_CHAINS)
def test_ntt_sparse_spectra_give_exact_zeros(name):
    """the final canon() at non-zero multiples of q: the input is the oracle's transform of a vector that vanishes at half of its positions,
    so the device's transform back has to return exactly 0 there - from lazy sums that are multiples of q, not from zero inputs"""
    ctx, ring = kr.gpu_env(name)
    rnd = np.random.default_rng(9)
    nmod = len(ring.moduli)
    mods = list(range(nmod))
    mask = rnd.random((nmod, ring.N)) < 0.5
    mask[:, :512] = np.arange(512) % 2 == 0                   # a regular stretch too
    sparse = np.stack([rnd.integers(1, ring.moduli[m], ring.N, dtype=np.uint64) for m in mods])
    sparse[mask] = 0
    nzero = int(np.count_nonzero(mask))
    assert ring.N * nmod * 0.45 < nzero < ring.N * nmod * 0.55
    spectrum = np.stack([ring.ntt(m, sparse[m]) for m in mods])          # forward by the oracle, back on the device
    assert np.count_nonzero(spectrum == 0) < 8
    back = ctx.ntt_rows(spectrum, mods, inverse=True)
    assert int(np.count_nonzero(back[mask])) == 0 and int(np.count_nonzero(back == 0)) == nzero
    assert np.array_equal(back, sparse)
    coeffs = np.stack([ring.intt(m, sparse[m]) for m in mods])           # inverse by the oracle, forward on the device
    fwd = ctx.ntt_rows(coeffs, mods)
    assert int(np.count_nonzero(fwd[mask])) == 0 and int(np.count_nonzero(fwd == 0)) == nzero
    assert np.array_equal(fwd, sparse)
