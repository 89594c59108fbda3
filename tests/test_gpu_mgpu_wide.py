"""The multi-GPU engine (sfg_mgpu_*, sfgwas_amd/csrc/mgpu.hip) at the world sizes it is built for - 4 and 8 ranks, one 8-GPU node - and at 14, the smallest world in
which a rank holds padding giant slots only.  Every rank shares device 0, so the engine takes its in-process `direct` transport: the same sequence as over RCCL
(SNP-block shards, per-column reduce-scatter over world * ceil(91 / world) padded giant slots, reduce, finalize of the owned giants, all-reduce, reduce).
  * world 8:  13 SNP blocks -> 1 or 2 per rank, gpr = 12 (5 padding slots); 5 SNP blocks -> ranks 0, 2 and 5 own none; k_sum_peers sums 8 peers.
  * world 4:  gpr = 23, one padding slot.
  * world 14: gpr = 7, rank 13 holds slots 91 - 97 (no real giant: its finalize aligns nothing and must contribute zeros, not the stale words of its pooled output);
              with 5 SNP blocks nine ranks own no block.
  * the engine against the oracle with real key-switching keys at world 8 (3 SNP blocks: five ranks own none);
  * a failure on ONE rank (test hook sfg_mgpu_inject_failure_for_test) at worlds 3 and 8, before the agreement point and in the I/O pass: the call fails naming that
    rank and cause, and the next calls on the same engine are right in every word (the rendezvous forgot the failed round: tests/test_rendezvous.py);
  * the association scan's round-robin batches at 8 ranks.
Every comparison is every output word.  The single-GPU products are checked against the oracle elsewhere (tests/test_gpu_matmul.py, test_gpu_fullsize.py)."""
import ctypes as C
import numpy as np
import pytest

import oracle_lib as ol
from test_gpu_mgpu import make_engine, ROTS

pytestmark = pytest.mark.gpu
SLOTS, D, L, LEVEL, S = 8192, 91, 5, 5, 2
T, SQ = 2, 1
M13 = (SLOTS + 300, 12 * SLOTS + 77)          # 2 block rows, 13 SNP blocks: Q'X^T changes column buffers with PW = 2
M5 = (100, 4 * SLOTS + 40)                    # 5 SNP blocks
SEED13 = 0x13B10C
_MEM = {"peak_gib": 0.0, "where": ""}
# up to 14 contexts share one GPU and its 288 GB: smaller MAC groups, accumulator passes and rank-local rotation caches, as tests/test_gpu_multirank.py's
# LIB_SHARED_ENV (the words do not depend on them: tests/test_gpu_properties.py)
SHARED = {"SFG_MM_GROUP": "4", "SFG_MM_ACC_BUDGET_MB": "4096", "SFG_MGPU_CACHE_GB": "24"}


def engine(monkeypatch, n, **env):
    mg = make_engine(monkeypatch, [0] * n, dict(SHARED, **env))
    assert (mg.world, mg.nlocal, mg.transport) == (n, n, "direct")
    return mg


def _hip():
    """the HIP runtime the library itself loaded (not a second copy)"""
    from sfgwas_amd import capi
    capi.lib()
    path = next(l.split()[-1] for l in open("/proc/self/maps") if "libamdhip64" in l)
    return C.CDLL(path)


def note_memory(where):
    free, total = C.c_size_t(), C.c_size_t()
    assert _hip().hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    used = (total.value - free.value) / 2 ** 30
    if used > _MEM["peak_gib"]:
        _MEM.update(peak_gib=used, where=where)
    print(f"device memory in use at {where}: {used:.1f} GiB of {total.value / 2 ** 30:.0f} (peak so far {_MEM['peak_gib']:.1f} GiB at {_MEM['where']})")


@pytest.fixture(scope="module")
def ref():
    """the single-context products: M13 (the synthetic matrix every rank generates its window of) and M5 (uploaded from the host)"""
    from sfgwas_amd import capi
    ctx = capi.Context(ol.Q_PN14, ol.P_PN14)
    lib = capi.lib()
    ctx.check(lib.sfg_fill_rotkeys_synthetic(ctx.h, (C.c_int * len(ROTS))(*ROTS), len(ROTS), 0xBEEF), "keys")
    rng = np.random.default_rng(1408)
    geno5 = (np.frombuffer(rng.bytes(M5[0] * M5[1]), dtype=np.uint8) % 4).astype(np.int8).reshape(M5) - 1
    nbr13, mct13 = 2, 13
    A13 = {0: ctx.fill_uniform_cts(S * nbr13, LEVEL, 0xC1), T: ctx.fill_uniform_cts(S * mct13, LEVEL, 0xC2)}
    A5 = {0: ctx.fill_uniform_cts(S * 1, LEVEL, 0xC3), T: ctx.fill_uniform_cts(S * 5, LEVEL, 0xC4)}
    Ah13 = {f: a.host().reshape(S, -1, 2, LEVEL + 1, ctx.N) for f, a in A13.items()}
    Ah5 = {f: a.host().reshape(S, -1, 2, LEVEL + 1, ctx.N) for f, a in A5.items()}
    d13, g13 = ctx.fill_geno(M13[0], M13[1], SEED13)
    g5 = ctx.geno_upload(geno5)
    want13, want5 = {}, {}
    for f in (0, T, T | SQ):
        o = ctx.matmul_resident(A13[f & T], S, LEVEL, L, g13, f); want13[f] = o.host().copy(); o.free()
    for f in (0, T):
        o = ctx.matmul_resident(A5[f & T], S, LEVEL, L, g5, f); want5[f] = o.host().copy(); o.free()
    note_memory("the single-context reference")
    ctx.geno_free(g13); d13.free(); ctx.geno_free(g5)
    for a in list(A13.values()) + list(A5.values()):
        a.free()
    ctx.close()
    yield {"A13": Ah13, "A5": Ah5, "want13": want13, "want5": want5, "geno5": geno5}
    print(f"peak device memory of tests/test_gpu_mgpu_wide.py: {_MEM['peak_gib']:.1f} GiB ({_MEM['where']})")


def same(got, want, what):
    assert got.shape == want.shape, what
    assert np.array_equal(got, want), f"{what}: {np.count_nonzero(got != want)} of {want.size} words differ"


def products(mg, g, A, want, flag_sets, what):
    for f in flag_sets:
        same(mg.matmul(A[f & T], S, LEVEL, L, g, f), want[f], f"{what}, flags {f}")


def blocks_of(mg, g):
    return [mg.geno_blocks(g, i) for i in range(mg.nlocal)]


def test_world_4_thirteen_blocks(ref, monkeypatch):
    """gpr = 23: 92 slots, one of padding; 3 + 3 + 3 + 4 SNP blocks"""
    mg = engine(monkeypatch, 4)
    try:
        mg.preflight(1000)
        g = mg.geno_synthetic(M13[0], M13[1], SEED13)
        assert [b1 - b0 for b0, b1 in blocks_of(mg, g)] == [3, 3, 3, 4]
        note_memory("world 4, 13 blocks")
        products(mg, g, ref["A13"], ref["want13"], (0, T), "world 4, M13")
        note_memory("world 4, after the products")
        mg.geno_free(g)
    finally:
        mg.close()


def test_world_8_products_and_one_rank_failures(ref, monkeypatch):
    """13 blocks over 8 ranks (1 or 2 each), then 5 blocks (ranks 0, 2, 5 own none); then a failure on one rank - before the agreement point on a rank that owns a
    block while the zero-block ranks are already waiting there, and in the I/O pass - each followed by products that must be right in every word"""
    from sfgwas_amd import capi
    mg = engine(monkeypatch, 8, SFG_ENABLE_TEST_HOOKS="1")
    try:
        mg.preflight(1000)
        mg.preflight(1)
        g = mg.geno_synthetic(M13[0], M13[1], SEED13)
        assert [b1 - b0 for b0, b1 in blocks_of(mg, g)] == [1, 2, 1, 2, 2, 1, 2, 2]
        products(mg, g, ref["A13"], ref["want13"], (0, T, T | SQ), "world 8, M13")
        note_memory("world 8, after the 13-block products")
        mg.geno_free(g)
        g = mg.geno_upload(ref["geno5"])
        nb = [b1 - b0 for b0, b1 in blocks_of(mg, g)]
        assert [r for r in range(8) if nb[r] == 0] == [0, 2, 5]
        products(mg, g, ref["A5"], ref["want5"], (0, T), "world 8, M5")
        for rank, phase, cause in ((3, 1, "prepare"), (5, 0, "I/O pass"), (7, 1, "prepare"), (6, 0, "I/O pass")):
            mg.inject_failure_for_test(rank, phase)
            with pytest.raises(capi.SfgError, match=rf"rank {rank} \(device 0\): injected test failure \({cause}\)"):
                mg.matmul(ref["A5"][T], S, LEVEL, L, g, T)
            products(mg, g, ref["A5"], ref["want5"], (T, 0), f"world 8, M5, after an injected failure on rank {rank} ({cause})")
        mg.geno_free(g)
    finally:
        mg.close()


def test_world_3_one_rank_failure_then_good_products(ref, monkeypatch):
    """5 blocks over 3 ranks (1 + 2 + 2): a failure before the agreement point with both peers on their way to it, then one in the I/O pass"""
    from sfgwas_amd import capi
    mg = engine(monkeypatch, 3, SFG_ENABLE_TEST_HOOKS="1")
    try:
        g = mg.geno_upload(ref["geno5"])
        for rank, phase, cause in ((1, 1, "prepare"), (0, 1, "prepare"), (2, 0, "I/O pass")):
            mg.inject_failure_for_test(rank, phase)
            with pytest.raises(capi.SfgError, match=rf"rank {rank} \(device 0\): injected test failure \({cause}\)"):
                mg.matmul(ref["A5"][T], S, LEVEL, L, g, T)
            products(mg, g, ref["A5"], ref["want5"], (T, 0), f"world 3, after an injected failure on rank {rank} ({cause})")
        with pytest.raises(capi.SfgError, match="phase"):
            mg.inject_failure_for_test(0, 2)
        mg.geno_free(g)
    finally:
        mg.close()
    monkeypatch.delenv("SFG_ENABLE_TEST_HOOKS")
    mg = engine(monkeypatch, 2)                            # without the test switch the hook is refused
    try:
        with pytest.raises(capi.SfgError, match="test hook"):
            mg.inject_failure_for_test(0, 1)
    finally:
        mg.close()


def test_world_14_rank_without_a_real_giant_contributes_zeros(ref, monkeypatch):
    """gpr = 7: rank 13 holds slots 91 - 97 only.  A 13-block Q'X^T first leaves non-zero words in every rank's pooled output buffer; the 5-block products after it
    (nine ranks without a block) must not see any of them"""
    mg = engine(monkeypatch, 14)
    try:
        mg.preflight(1000)
        g = mg.geno_synthetic(M13[0], M13[1], SEED13)
        products(mg, g, ref["A13"], ref["want13"], (T,), "world 14, M13")
        note_memory("world 14, after the 13-block product")
        mg.geno_free(g)
        g = mg.geno_upload(ref["geno5"])
        assert sum(b1 == b0 for b0, b1 in blocks_of(mg, g)) == 9
        products(mg, g, ref["A5"], ref["want5"], (T, 0), "world 14, M5 after M13")
        mg.geno_free(g)
    finally:
        mg.close()


def test_world_8_products_against_the_oracle_directly(monkeypatch):
    """real key-switching keys; X = 70 x (2 * 8192 + 40): 3 SNP blocks, so ranks 2, 5 and 7 own one and the other five none (the CPU oracle takes about 20 s per full
    block and direction, hence not 5 blocks).  Q X and Q' X^T against orc_matmult4stream (gwas/matmult.go:1043-1505), every word - no single-context product in between"""
    from sfgwas_amd import capi
    ring = ol.Ring(14, ol.Q_PN14, ol.P_PN14)
    keys = ol.RotKeys(ring)
    rnd = np.random.default_rng(808)
    nrow, ncol, s, level = 70, 2 * SLOTS + 40, 2, 5
    geno = rnd.integers(-1, 3, (nrow, ncol)).astype(np.int8)
    for k, v in SHARED.items():
        monkeypatch.setenv(k, v)
    mg = capi.MultiGpu(ol.Q_PN14, ol.P_PN14, devices=[0] * 8)
    try:
        assert mg.transport == "direct"
        for k in sorted(set(range(1, D)) | {g * D for g in range(1, D) if g * D < SLOTS}):
            key = capi.random_rotkey(ring.moduli, ring.beta, ring.N, 800 + k)
            keys.add(ring.galois(k), key)
            mg.load_rotkey(ring.galois(k), key)
        g = mg.geno_upload(geno)
        assert [b1 - b0 for b0, b1 in blocks_of(mg, g)] == [0, 0, 1, 0, 0, 1, 0, 1]
        A = np.stack([np.stack([ring.fill_uniform(level, 250 + i)]) for i in range(s)])
        AT = np.stack([np.stack([ring.fill_uniform(level, 270 + 3 * i + b) for b in range(3)]) for i in range(s)])
        got = mg.matmul(A, s, level, L, g, 0)
        want, _, _ = ol.matmult4stream(ring, keys, 2.0 ** 34, A, level, L, geno)
        same(got, want, "world 8, Q X against the oracle")
        got_t = mg.matmul(AT, s, level, L, g, T)
        want_t, _, _ = ol.matmult4stream(ring, keys, 2.0 ** 34, AT, level, L, np.ascontiguousarray(geno.T))
        same(got_t, want_t, "world 8, Q' X^T against the oracle")
        mg.geno_free(g)
    finally:
        mg.close()


def test_world_8_association_scan_round_robin(tmp_path, monkeypatch):
    """sfg_mgpu_assoc_stream_bed: batch k goes to rank k % 8; 10 batches, so ranks 0 and 1 stream two and the others one.  Outputs and padded column sums against the
    single-context scan (tests/test_gpu_stream.py holds that one against the oracle), with row and column filters, plain and SFG_SQUARE"""
    from sfgwas_amd import capi
    from test_gpu_stream import write_bed
    lib = capi.lib()
    ns, nv, batch, s, level, maxl, cap = 130, 1100, 100, 2, 5, 5, 12
    rnd = np.random.default_rng(88)
    geno = rnd.choice(np.array([2, -1, 1, 0], dtype=np.int8), size=(ns, nv), p=[0.2, 0.05, 0.35, 0.4])
    rowf = (rnd.random(ns) < 0.9).astype(np.uint8)
    colf = (rnd.random(nv) < 0.9).astype(np.uint8)
    path = str(tmp_path / "chr.bed")
    write_bed(path, geno)
    N = 16384
    ctx = capi.Context(ol.Q_PN14, ol.P_PN14)
    ctx.check(lib.sfg_fill_rotkeys_synthetic(ctx.h, (C.c_int * len(ROTS))(*ROTS), len(ROTS), 0xBEEF), "keys")
    dA = ctx.fill_uniform_cts(s, level, 0xA58)
    A = dA.host().copy()
    want = {}
    for flags in (0, SQ):
        dout = capi.DevArray(ctx, (s, cap, 2, maxl, N))
        ctx.check(lib.sfg_memcpy_h2d(ctx.h, dout.p, np.zeros(s * cap * 2 * maxl * N, dtype=np.uint64).ctypes.data_as(C.c_void_p), s * cap * 2 * maxl * N * 8), "zero")
        sums = np.full(cap * SLOTS, -7.0); sq = np.full(cap * SLOTS, -7.0); n_ct = C.c_size_t()
        ctx.check(lib.sfg_assoc_stream_bed(ctx.h, path.encode(), ns, nv, rowf.ctypes.data_as(C.c_void_p), colf.ctypes.data_as(C.c_void_p), batch, dA.p, s, level, maxl, flags,
                                           dout.p, cap, C.byref(n_ct), sums.ctypes.data_as(C.c_void_p), sq.ctypes.data_as(C.c_void_p)), "assoc_stream_bed")
        assert n_ct.value == 10
        want[flags] = (dout.host().copy(), sums, sq)
        dout.free()
    dA.free(); ctx.close()
    mg = engine(monkeypatch, 8)
    try:
        for flags in (0, SQ):
            out = np.zeros((s, cap, 2, maxl, N), dtype=np.uint64)
            sums = np.full(cap * SLOTS, -7.0); sq = np.full(cap * SLOTS, -7.0); n_ct = C.c_size_t()
            mg.check(lib.sfg_mgpu_assoc_stream_bed(mg.h, path.encode(), ns, nv, rowf.ctypes.data_as(C.c_void_p), colf.ctypes.data_as(C.c_void_p), batch,
                                                   capi.p64(A), s, level, maxl, flags, capi.p64(out), cap, C.byref(n_ct),
                                                   sums.ctypes.data_as(C.c_void_p), sq.ctypes.data_as(C.c_void_p)), "mgpu_assoc_stream_bed")
            assert n_ct.value == 10
            same(out, want[flags][0], f"world 8 association scan, flags {flags}")
            assert np.array_equal(sums, want[flags][1]) and np.array_equal(sq, want[flags][2]), f"world 8 association scan, flags {flags}: column sums"
    finally:
        mg.close()
