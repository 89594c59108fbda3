"""k_pgen_decode, the host index and the window planner (sfgwas_amd/csrc/pgen.hip) on the directed files of tests/pgen_cases.py: sample counts around the
4-, 8- and 16-sample units of a row, each sample-id width, difflists of 0 to 513 groups, delta varints of 1 to 4 bytes, LD runs over every kind of base with
windows that start at every variant, two header blocks, every header form, trailing tracks, storage mode 0x02 - and the files each check of the decoder refuses.

Ground truth is the code matrix handed to the writer (3 -> -1); tests/test_pgen_edges.py holds the CPU oracle to the same matrices.  These tests pin the decoder
to the specification as tests/pgen_writer.py states it, not to plink2: parity stays unpinned beyond record types 0 and 1."""
import ctypes as C
import numpy as np
import pytest

import oracle_lib as ol
import pgen_cases as pc
from test_gpu_fullsize import Env, host_cts, SLOTS, N, L, LEVEL, SCALE

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    e = Env()
    yield e
    e.close()


def decode(env, img, *args):
    g = env.ctx.geno_from_pgen(img, *args)
    try:
        return env.ctx.geno_to_host(g)
    finally:
        env.capi.lib().sfg_geno_free(env.ctx.h, g)


def first_difference(got, want):
    if got.shape != want.shape:
        return f"shape {got.shape}, expected {want.shape}"
    i, v = np.argwhere(got != want)[0]
    return f"{int((got != want).sum())} of {want.size} differ; first: sample {i}, variant {v} of the window: {got[i, v]}, expected {want[i, v]}"


@pytest.mark.parametrize("name", pc.NAMES)
def test_device_decodes_the_file_and_its_windows(env, name):
    c = pc.get(name)
    got, want = decode(env, c.img), c.want()
    assert np.array_equal(got, want), first_difference(got, want)
    for v0, v1 in c.windows:
        got, want = decode(env, c.img, v0, v1), c.want(v0, v1)
        assert np.array_equal(got, want), f"[{v0}, {v1}): " + first_difference(got, want)
    v0, v1 = c.windows[0]
    rf, cf = pc.filters(c, v0, v1)                                            # the filters are fused into the transposing kernel
    got, want = decode(env, c.img, v0, v1, rf, cf), c.want(v0, v1, rf, cf)
    assert np.array_equal(got, want), f"[{v0}, {v1}) filtered: " + first_difference(got, want)


@pytest.mark.parametrize("name", pc.NAMES)
def test_device_counts_genotypes(env, name):
    c = pc.get(name)
    assert np.array_equal(env.ctx.pgen_geno_counts(c.img), c.counts())
    keep = pc.keep_mask(c)                                                    # its last kept sample is ns - 1
    assert np.array_equal(env.ctx.pgen_geno_counts(c.img, keep), c.counts(keep))


def dims(env, img):
    ns, nv = C.c_size_t(), C.c_size_t()
    env.ctx.check(env.capi.lib().sfg_pgen_dims(env.ctx.h, img.ctypes.data_as(C.c_void_p), img.size, C.byref(ns), C.byref(nv)), "pgen_dims")
    return ns.value, nv.value


@pytest.mark.parametrize("name", pc.NAMES)
def test_device_reports_the_dimensions(env, name):
    c = pc.get(name)
    assert dims(env, c.img) == (c.ns, c.nv)


@pytest.mark.parametrize("name", pc.MALFORMED)
def test_device_refuses(env, name):
    """every refusal is an explicit check of pgen_index_unchecked, pgen_window or k_pgen_decode (PGEN_ERR_*), made before the read it guards; the context decodes
    a good file afterwards"""
    img, cause = pc.malformed(name)
    with pytest.raises(env.capi.SfgError, match=cause):
        decode(env, img)
    with pytest.raises(env.capi.SfgError, match=cause):
        env.ctx.pgen_geno_counts(img)
    good = pc.get("tails-5")
    assert np.array_equal(decode(env, good.img), good.want())


def test_scan_over_the_block_boundary_streamed_and_in_memory(env, tmp_path):
    """GenoBlockMult over the two-block file: about 250 kept variants on both sides of variant 65 536, batches of 100.  sfg_assoc_pgen and sfg_assoc_stream_pgen
    (plain and SFG_STREAM_DIRECT) give the same words; the batch that contains variant 65 536 equals the oracle's product of the ground-truth matrix."""
    lib = env.capi.lib()
    c = pc.get("blocks-acgap")
    path = str(tmp_path / "blocks.pgen"); c.img.tofile(path)
    rnd = np.random.default_rng(3)
    colf = np.zeros(c.nv, dtype=np.uint8)
    colf[pc.BLOCK - 140: pc.BLOCK + 71] = rnd.random(211) < 0.93
    colf[:40] = 1                                                             # and a batch from the start of the first block
    colf[pc.BLOCK - 2: pc.BLOCK + 3] = 1
    rowf = np.array([1, 1, 0, 1, 1], dtype=np.uint8)
    batch, s = 100, 2
    kept = np.flatnonzero(colf)
    nb = -(-len(kept) // batch)
    A = host_cts(env.ring, s, 1, LEVEL, 43)
    dA = env.capi.DevArray.from_host(env.ctx, A)
    outs = []
    for mode in ("memory", "stream", "direct"):
        dout = env.capi.DevArray(env.ctx, (s, nb, 2, L, N))
        sums = np.zeros(nb * SLOTS); got_ct = C.c_size_t()
        if mode == "memory":
            rc = lib.sfg_assoc_pgen(env.ctx.h, c.img.ctypes.data_as(C.c_void_p), c.img.size, rowf.ctypes.data_as(C.c_void_p), colf.ctypes.data_as(C.c_void_p), batch,
                                    dA.p, s, LEVEL, L, 0, dout.p, nb, C.byref(got_ct), sums.ctypes.data_as(C.c_void_p), None)
        else:
            flags = env.capi.SFG_STREAM_DIRECT if mode == "direct" else 0
            rc = lib.sfg_assoc_stream_pgen(env.ctx.h, path.encode(), rowf.ctypes.data_as(C.c_void_p), colf.ctypes.data_as(C.c_void_p), batch,
                                           dA.p, s, LEVEL, L, flags, dout.p, nb, C.byref(got_ct), sums.ctypes.data_as(C.c_void_p), None)
            if rc and mode == "direct" and b"O_DIRECT" in lib.sfg_last_error(env.ctx.h):
                dout.free(); continue                                         # a file system without O_DIRECT
        env.ctx.check(rc, mode)
        assert got_ct.value == nb
        outs.append((mode, dout.host(), sums.copy()))
        dout.free()
    assert len(outs) >= 2
    for mode, o, sm in outs[1:]:
        assert np.array_equal(o, outs[0][1]) and np.array_equal(sm, outs[0][2]), f"{mode} differs from the in-memory scan"
    k = int(np.searchsorted(kept, pc.BLOCK)) // batch                         # the batch that holds variant 65 536
    cols = kept[k * batch:(k + 1) * batch]
    assert cols[0] < pc.BLOCK - 1 and cols[-1] > pc.BLOCK + 1
    sub = np.ascontiguousarray(c.want()[rowf.astype(bool)][:, cols])
    want, wsum, _ = ol.matmult4stream(env.ring, env.keys, SCALE, A, LEVEL, L, sub, compute_sqsum=True, enc_prec=1)
    assert np.array_equal(outs[0][1][:, k:k + 1], want), "the batch across the block boundary vs the oracle"
    assert np.array_equal(outs[0][2][k * SLOTS: k * SLOTS + len(cols)], wsum)
    dA.free()
