"""Times of the general ring (sfgwas_amd/csrc/gring.hip) - one JSON line per case, appended to --out (profiles/ring_bench.jsonl).

  P14    the general ring beside the specialised context on PN14QP438's own parameters, alternating in one run: the transform of 1845 x 10 rows
         (sfg_ring_ntt_rows / sfg_ntt_rows) and a rotation batch of 64 ciphertexts at level 9 (sfg_ring_rotate_right_dev / sfg_rotate_right_dev); the words of the
         two paths are compared and must be equal.  The ratio general / specialised of the transform is reported against the aim of 3.0 (an integer Shoup butterfly
         costed at 2.5 fp64 butterflies, plus a fifth for the second HBM crossing); it does not gate anything.
  PN15   18 + 3 moduli at logN 15 and
  PN16   34 + 4 moduli at logN 16 (the shapes of PN15QP880 / PN16QP1761; NTT-friendly primes of 40..55 bits found here): the transform of a batch's rows, a rotation
         batch and mulrelin + rescale at the top level.  First measurements: no yardstick exists for them.

Host clock around single calls that end in a device synchronise, every shape warmed up first, --rounds (30) alternations: medians, the largest single time beside
them.  `hbm_bytes` of a transform: rows x N x 8 bytes read and written by each of its two passes; `io_bytes` of the other calls: operands read once and results
written once (ciphertexts in and out, the key) - the intermediate rows of the key switch are not counted, so those rates are end-to-end figures, not HBM rates."""
import argparse, ctypes as C, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from sfgwas_amd import capi, params as P

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--rounds", type=int, default=30)
ap.add_argument("--cases", default="P14,PN15,PN16")
ap.add_argument("--ntt-cts", type=int, default=923, help="P14: ciphertexts at level 9 whose first 1845 x 10 rows are transformed")
args = ap.parse_args()
L = capi.lib()


def primes(logN, bits, count, skip=0):
    from sympy import isprime
    M, out, x = 2 << logN, [], (1 << bits) + 1 - (2 << logN)
    while len(out) < count + skip:
        if isprime(x):
            out.append(x)
        x -= M
    return out[skip:]


def timed(calls, sync, rounds):
    for fn in calls.values():
        fn(); fn(); sync()
    t = {k: [] for k in calls}
    for _ in range(rounds):
        for k, fn in calls.items():
            t0 = time.perf_counter(); fn(); sync(); t[k].append(time.perf_counter() - t0)
    return {k: (float(np.median(v)) * 1e3, float(np.max(v)) * 1e3) for k, v in t.items()}


def emit(rec):
    print(json.dumps(rec), flush=True)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write(json.dumps(rec) + "\n")


def equal_on_device(owner, a, b, nbytes, chunk=256 << 20):
    """compare two device buffers through the host, chunk by chunk"""
    for off in range(0, nbytes, chunk):
        n = min(chunk, nbytes - off)
        x = owner.to_host(C.c_void_p(a.value + off), (n // 8,), np.uint64)
        y = owner.to_host(C.c_void_p(b.value + off), (n // 8,), np.uint64)
        if not np.array_equal(x, y):
            return False
    return True


def case_p14():
    q, p = list(P.Q_PN14), list(P.P_PN14)
    ctx, ring = capi.Context(q, p), capi.Ring(14, q, p)
    N, level, nrows = ctx.N, 9, 1845 * 10
    src = ctx.fill_uniform_cts(args.ntt_cts, level, 11)                         # canonical rows [nct][2][10][N]: row r has modulus r % 10
    nbytes = nrows * N * 8
    a, b = ctx.malloc(nbytes), ctx.malloc(nbytes)
    for d in (a, b):
        ctx.check(L.sfg_memcpy_d2d(ctx.h, d, src.p, nbytes), "d2d")
    ctx.sync()
    mi = (C.c_int * nrows)(*[r % 10 for r in range(nrows)])
    ctx.check(L.sfg_ntt_rows(ctx.h, a, nrows, mi), "ntt"); ring.check(L.sfg_ring_ntt_rows(ring.h, b, nrows, mi), "ntt"); ctx.sync(); ring.sync()
    ntt_equal = equal_on_device(ctx, a, b, nbytes)
    ctx.check(L.sfg_intt_rows(ctx.h, a, nrows, mi), "intt"); ring.check(L.sfg_ring_intt_rows(ring.h, b, nrows, mi), "intt"); ctx.sync(); ring.sync()
    ntt_equal = ntt_equal and equal_on_device(ctx, a, b, nbytes) and equal_on_device(ctx, a, src.p, nbytes)

    def both():
        ctx.sync(); ring.sync()
    t = timed({"ring_ntt": lambda: ring.check(L.sfg_ring_ntt_rows(ring.h, b, nrows, mi), "ntt"), "ctx_ntt": lambda: ctx.check(L.sfg_ntt_rows(ctx.h, a, nrows, mi), "ntt"),
               "ring_intt": lambda: ring.check(L.sfg_ring_intt_rows(ring.h, b, nrows, mi), "intt"), "ctx_intt": lambda: ctx.check(L.sfg_intt_rows(ctx.h, a, nrows, mi), "intt")},
              both, args.rounds)
    nct = 64
    g = ring.galois(ring.slots - 3)
    key = capi.random_rotkey(q + p, ring.beta, N, 5)
    ctx.load_rotkey(g, key); ring.load_rotkey(g, key)
    ctw = 2 * (level + 1) * N * 8
    o1, o2 = ctx.malloc(nct * ctw), ctx.malloc(nct * ctw)
    rots = (C.c_int * nct)(*([3] * nct))
    tr = timed({"ring_rotate": lambda: ring.check(L.sfg_ring_rotate_right_dev(ring.h, src.p, o2, nct, level, rots), "rot"),
                "ctx_rotate": lambda: ctx.check(L.sfg_rotate_right_dev(ctx.h, src.p, o1, nct, level, rots), "rot")}, both, args.rounds)
    rot_equal = equal_on_device(ctx, o1, o2, nct * ctw)
    ratio = t["ring_ntt"][0] / t["ctx_ntt"][0]
    rec = {"case": "P14", "logN": 14, "nq": len(q), "np": len(p), "rounds": args.rounds, "ntt_rows": nrows, "ntt_hbm_bytes": 4 * nbytes, "ntt_words_equal": ntt_equal,
           "rotate_cts": nct, "rotate_level": level, "rotate_words_equal": rot_equal, "rotate_io_bytes": 2 * nct * ctw + key.nbytes}
    for k, (med, mx) in {**t, **tr}.items():
        rec[k + "_ms"], rec[k + "_max_ms"] = round(med, 3), round(mx, 3)
    rec["ring_ntt_tb_per_s"] = round(4 * nbytes / t["ring_ntt"][0] / 1e9, 3)
    rec["ntt_ratio_general_over_specialised"] = round(ratio, 2)
    rec["intt_ratio_general_over_specialised"] = round(t["ring_intt"][0] / t["ctx_intt"][0], 2)
    rec["rotate_ratio_general_over_specialised"] = round(tr["ring_rotate"][0] / tr["ctx_rotate"][0], 2)
    rec["ntt_ratio_aim"] = 3.0
    rec["ntt_ratio_aim_met"] = bool(ratio <= 3.0)
    emit(rec)
    for d in (a, b, o1, o2):
        ctx.free(d)
    src.free(); ctx.close(); ring.close()
    if not (ntt_equal and rot_equal):
        raise SystemExit("bench_ring: the two paths' words differ")


def case_wide(name, logN, q, p, nct):
    ring = capi.Ring(logN, q, p)
    N, level, mods = ring.N, len(q) - 1, q + p
    rnd = np.random.default_rng(logN)
    cts = np.empty((nct, 2, level + 1, N), dtype=np.uint64)
    for m in range(level + 1):
        cts[:, :, m] = rnd.integers(0, q[m], (nct, 2, N), dtype=np.uint64)
    g = ring.galois(ring.slots - 3)
    ring.load_rotkey(g, capi.random_rotkey(mods, ring.beta, N, 5))
    ring.load_relinkey(capi.random_rotkey(mods, ring.beta, N, 6))
    key_bytes = ring.beta * 2 * len(mods) * N * 8
    a, rows = ring.to_device(cts), ring.to_device(cts)
    o, o2 = ring.malloc(cts.nbytes), ring.malloc(cts.nbytes)
    nrows = nct * 2 * (level + 1)
    mi = (C.c_int * nrows)(*[r % (level + 1) for r in range(nrows)])
    rots = (C.c_int * nct)(*([3] * nct))

    def mulrelin_rescale():
        ring.check(L.sfg_ring_ct_mulrelin_dev(ring.h, a, a, o, nct, level), "mulrelin")
        ring.check(L.sfg_ring_ct_rescale_dev(ring.h, o, o2, nct, level), "rescale")
    t = timed({"ntt": lambda: ring.check(L.sfg_ring_ntt_rows(ring.h, rows, nrows, mi), "ntt"), "intt": lambda: ring.check(L.sfg_ring_intt_rows(ring.h, rows, nrows, mi), "intt"),
               "rotate": lambda: ring.check(L.sfg_ring_rotate_right_dev(ring.h, a, o, nct, level, rots), "rot"), "mulrelin_rescale": mulrelin_rescale}, ring.sync, args.rounds)
    rec = {"case": name, "logN": logN, "nq": len(q), "np": len(p), "beta": ring.beta, "rounds": args.rounds, "cts": nct, "level": level, "ntt_rows": nrows,
           "ntt_hbm_bytes": 4 * cts.nbytes, "rotate_io_bytes": 2 * cts.nbytes + key_bytes, "mulrelin_rescale_io_bytes": 3 * cts.nbytes + cts.nbytes * level // (level + 1) + key_bytes}
    for k, (med, mx) in t.items():
        rec[k + "_ms"], rec[k + "_max_ms"] = round(med, 3), round(mx, 3)
    rec["ntt_tb_per_s"] = round(rec["ntt_hbm_bytes"] / t["ntt"][0] / 1e9, 3)
    rec["intt_tb_per_s"] = round(rec["ntt_hbm_bytes"] / t["intt"][0] / 1e9, 3)
    rec["rotate_io_gb_per_s"] = round(rec["rotate_io_bytes"] / t["rotate"][0] / 1e6, 1)
    rec["mulrelin_rescale_io_gb_per_s"] = round(rec["mulrelin_rescale_io_bytes"] / t["mulrelin_rescale"][0] / 1e6, 1)
    rec["yardstick"] = "none: first measurement"
    emit(rec)
    for d in (a, rows, o, o2):
        ring.free(d)
    ring.close()


for case in args.cases.split(","):
    if case == "P14":
        case_p14()
    elif case == "PN15":
        case_wide("PN15", 15, primes(15, 50, 1) + primes(15, 40, 17), primes(15, 50, 3, skip=1), 8)
    elif case == "PN16":
        case_wide("PN16", 16, primes(16, 55, 1) + primes(16, 45, 33), primes(16, 55, 4, skip=1), 8)
    elif case == "PN12":                                                        # 2 + 1 moduli at logN 12: a rehearsal size, overheads only
        case_wide("PN12", 12, primes(12, 37, 1) + primes(12, 32, 1), primes(12, 38, 1), 2)
    else:
        raise SystemExit(f"unknown case {case}")
