"""Times of the general ring's two ends (sfgwas_amd/csrc/gring_io.hip) - one JSON line per case, appended to --out (profiles/ring_io_bench.jsonl).

  P14    the general ring beside the specialised context on PN14QP438's own parameters, 1845 vectors / ciphertexts at level 4, alternating in one run, same public
         key, same sampler key, same secret key, scale 2^34: encode + encrypt (sfg_ring_encrypt_vectors_dev / sfg_encrypt_vectors_dev) and decrypt + decode
         (sfg_ring_decrypt_vectors / sfg_decrypt_vectors) - the yardsticks of the aim: general / specialised at most 4.3 (what the general transform costs beside the
         specialised one); the aim is reported as met or missed and gates nothing.  Beside them ct += Enc(0) and the collective decryption's share (both polynomials on
         both paths).  The words of the two paths are compared and must be equal (decoded doubles are not compared: the transforms differ).
  PN15   18 + 3 moduli at logN 15 and
  PN16   34 + 4 moduli at logN 16 (the chains tools/bench_ring.py builds), 8 vectors / ciphertexts at the top level: encode + encrypt, ct += Enc(0), the share, the
         finish, decode_coeffs, decode_vectors (polynomial 0 read in place) and decrypt + decode.  First measurements: no yardstick exists for them.

Host clock around single calls that end in a device synchronise, every shape warmed up first, --rounds (30) alternations: medians, the largest single time beside
them.  `io_bytes`: operands read once and results written once (the key included); the core's intermediate rows are not counted: end-to-end figures, not HBM rates.
The CPU cost these calls replace (lattigo's encoder, encryptor, PCKS protocol and decoder) cannot be measured without a Go toolchain."""
import argparse, ctypes as C, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from sympy import isprime                # at the top: a machine without sympy fails before any record is appended
from sfgwas_amd import capi, params as P

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--rounds", type=int, default=30)
ap.add_argument("--cases", default="P14,PN15,PN16")
ap.add_argument("--p14-cts", type=int, default=1845)
args = ap.parse_args()
L = capi.lib()
KEY = bytes(range(100, 132))


def primes(logN, bits, count, skip=0):
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


def uniform_rows(rnd, mods, lead, N):
    out = np.empty(tuple(lead) + (len(mods), N), dtype=np.uint64)
    for m, q in enumerate(mods):
        out[..., m, :] = rnd.integers(0, q, tuple(lead) + (N,), dtype=np.uint64)
    return out


def equal_on_device(owner, a, b, nbytes, chunk=256 << 20):
    for off in range(0, nbytes, chunk):
        n = min(chunk, nbytes - off)
        if not np.array_equal(owner.to_host(C.c_void_p(a.value + off), (n // 8,), np.uint64), owner.to_host(C.c_void_p(b.value + off), (n // 8,), np.uint64)):
            return False
    return True


def case_p14():
    q, p = list(P.Q_PN14), list(P.P_PN14)
    ctx, ring = capi.Context(q, p), capi.Ring(14, q, p)
    N, level, nct = ctx.N, 4, args.p14_cts
    rnd = np.random.default_rng(14)
    pk, sk = uniform_rows(rnd, q + p, (2,), N), uniform_rows(rnd, q, (), N)          # parity and time need no valid key
    for o in (ctx, ring):
        o.load_public_key(pk); o.load_secret_key(sk); o.seed_encryptor(KEY)
    ctb, rowb = nct * 2 * (level + 1) * N * 8, nct * (level + 1) * N * 8
    a, b, ha, hb, ga, gb = ring.malloc(ctb), ring.malloc(ctb), ring.malloc(rowb), ring.malloc(rowb), ring.malloc(rowb), ring.malloc(rowb)
    e0, e1 = ring.to_device(rnd.integers(-38, 39, (nct, N)).astype(np.int32)), ring.to_device(rnd.integers(-38, 39, (nct, N)).astype(np.int32))

    def both():
        ctx.sync(); ring.sync()
    ring.check(L.sfg_ring_memcpy_h2d(ring.h, a, np.zeros(ctb // 8, np.uint64).ctypes.data_as(C.c_void_p), ctb), "zero")
    ring.check(L.sfg_ring_memcpy_h2d(ring.h, b, np.zeros(ctb // 8, np.uint64).ctypes.data_as(C.c_void_p), ctb), "zero")
    ctx.check(L.sfg_ct_add_fresh_zero_dev(ctx.h, a, nct, level), "ctx zero"); ring.check(L.sfg_ring_ct_add_fresh_zero_dev(ring.h, b, nct, level), "ring zero"); both()
    enc_equal = equal_on_device(ring, a, b, ctb)                                       # both from index 0 under one key, onto zeros
    ctx.check(L.sfg_pcks_gen_share_dev(ctx.h, a, nct, level, e0, e1, ha, ga), "ctx share"); ring.check(L.sfg_ring_pcks_gen_share_dev(ring.h, b, nct, level, e0, e1, hb, gb), "ring share"); both()
    share_equal = equal_on_device(ring, ha, hb, rowb) and equal_on_device(ring, ga, gb, rowb)
    vals = rnd.uniform(-4, 4, (nct, N // 2))
    pv = vals.ctypes.data_as(C.POINTER(C.c_double))
    re = np.empty((nct, N // 2))
    pre = re.ctypes.data_as(C.POINTER(C.c_double))
    for o in (ctx, ring):
        o.seed_encryptor(KEY)
    ctx.check(L.sfg_encrypt_vectors_dev(ctx.h, pv, nct, level, a), "ctx encrypt"); ring.check(L.sfg_ring_encrypt_vectors_dev(ring.h, pv, nct, level, 2.0 ** 34, b), "ring encrypt"); both()
    encv_equal = equal_on_device(ring, a, b, ctb)
    tv = timed({"ring_encrypt_vectors": lambda: ring.check(L.sfg_ring_encrypt_vectors_dev(ring.h, pv, nct, level, 2.0 ** 34, b), "ring encrypt"),
                "ctx_encrypt_vectors": lambda: ctx.check(L.sfg_encrypt_vectors_dev(ctx.h, pv, nct, level, a), "ctx encrypt"),
                "ring_decrypt_vectors": lambda: ring.check(L.sfg_ring_decrypt_vectors(ring.h, b, nct, level, 2.0 ** 34, pre, None), "ring decrypt"),
                "ctx_decrypt_vectors": lambda: ctx.check(L.sfg_decrypt_vectors(ctx.h, a, nct, level, 2.0 ** 34, re.ctypes.data_as(C.c_void_p), None), "ctx decrypt")}, both, args.rounds)
    t = timed({"ring_add_fresh_zero": lambda: ring.check(L.sfg_ring_ct_add_fresh_zero_dev(ring.h, b, nct, level), "ring zero"),
               "ctx_add_fresh_zero": lambda: ctx.check(L.sfg_ct_add_fresh_zero_dev(ctx.h, a, nct, level), "ctx zero"),
               "ring_pcks_gen_share": lambda: ring.check(L.sfg_ring_pcks_gen_share_dev(ring.h, b, nct, level, e0, e1, hb, gb), "ring share"),
               "ctx_pcks_gen_share": lambda: ctx.check(L.sfg_pcks_gen_share_dev(ctx.h, a, nct, level, e0, e1, ha, ga), "ctx share")}, both, args.rounds)
    rec = {"case": "P14", "logN": 14, "nq": len(q), "np": len(p), "rounds": args.rounds, "cts": nct, "level": level, "encrypt_words_equal": enc_equal, "share_words_equal": share_equal,
           "add_fresh_zero_io_bytes": 2 * ctb + pk.nbytes, "pcks_gen_share_io_bytes": ctb // 2 + 2 * rowb + 2 * nct * N * 4}
    t = {**tv, **t}
    rec["encrypt_vectors_words_equal"] = encv_equal
    for k, (med, mx) in t.items():
        rec[k + "_ms"], rec[k + "_max_ms"] = round(med, 3), round(mx, 3)
    for what in ("encrypt_vectors", "decrypt_vectors", "add_fresh_zero", "pcks_gen_share"):
        ratio = t["ring_" + what][0] / t["ctx_" + what][0]
        rec[what + "_ratio_general_over_specialised"] = round(ratio, 2)
        if what.endswith("_vectors"):
            rec[what + "_ratio_aim"] = 4.3
            rec[what + "_ratio_aim_met"] = bool(ratio <= 4.3)
    emit(rec)
    for d in (a, b, ha, hb, ga, gb, e0, e1):
        ring.free(d)
    ctx.close(); ring.close()
    if not (enc_equal and share_equal and encv_equal):
        raise SystemExit("bench_ring_io: the two paths' words differ")


def case_wide(name, logN, q, p, nct):
    ring = capi.Ring(logN, q, p)
    N, level = ring.N, len(q) - 1
    rnd = np.random.default_rng(logN)
    pk, sk = uniform_rows(rnd, q + p, (2,), N), uniform_rows(rnd, q, (), N)
    ring.load_public_key(pk); ring.load_secret_key(sk); ring.seed_encryptor(KEY)
    ctb, rowb = nct * 2 * (level + 1) * N * 8, nct * (level + 1) * N * 8
    ct, h0, h1, out = ring.to_device(uniform_rows(rnd, q, (nct, 2), N)), ring.malloc(rowb), ring.malloc(rowb), ring.malloc(rowb)
    e0, e1 = ring.to_device(rnd.integers(-38, 39, (nct, N)).astype(np.int32)), ring.to_device(rnd.integers(-38, 39, (nct, N)).astype(np.int32))
    coeffs = np.empty((nct, N), dtype=np.float64)
    vals, re = rnd.uniform(-4, 4, (nct, N // 2)), np.empty((nct, N // 2))
    pv, pre, encd = vals.ctypes.data_as(C.POINTER(C.c_double)), re.ctypes.data_as(C.POINTER(C.c_double)), ring.malloc(ctb)
    scale = 2.0 ** 40
    t = timed({"add_fresh_zero": lambda: ring.check(L.sfg_ring_ct_add_fresh_zero_dev(ring.h, ct, nct, level), "zero"),
               "pcks_gen_share": lambda: ring.check(L.sfg_ring_pcks_gen_share_dev(ring.h, ct, nct, level, e0, e1, h0, h1), "share"),
               "pcks_finish": lambda: ring.check(L.sfg_ring_pcks_finish_dev(ring.h, ct, nct, level, h0, out), "finish"),
               "encrypt_vectors": lambda: ring.check(L.sfg_ring_encrypt_vectors_dev(ring.h, pv, nct, level, scale, encd), "encrypt"),
               "decode_vectors": lambda: ring.check(L.sfg_ring_decode_vectors(ring.h, ct, 2 * (level + 1) * N, nct, level, scale, pre, None), "decode"),
               "decrypt_vectors": lambda: ring.check(L.sfg_ring_decrypt_vectors(ring.h, ct, nct, level, scale, pre, None), "decrypt"),
               "decode_coeffs": lambda: ring.check(L.sfg_ring_decode_coeffs(ring.h, ct, 2 * (level + 1) * N, nct, level, 2.0 ** 40, coeffs.ctypes.data_as(C.POINTER(C.c_double))), "decode")},
              ring.sync, args.rounds)
    rec = {"case": name, "logN": logN, "nq": len(q), "np": len(p), "rounds": args.rounds, "cts": nct, "level": level,
           "add_fresh_zero_io_bytes": 2 * ctb + pk.nbytes, "pcks_gen_share_io_bytes": ctb // 2 + 2 * rowb + 2 * nct * N * 4 + sk.nbytes,
           "pcks_finish_io_bytes": ctb // 2 + 2 * rowb, "decode_coeffs_io_bytes": rowb + nct * N * 8,
           "encrypt_vectors_io_bytes": nct * N * 4 + ctb + pk.nbytes, "decode_vectors_io_bytes": rowb + nct * N * 4, "decrypt_vectors_io_bytes": ctb + sk.nbytes + nct * N * 4}
    for k, (med, mx) in t.items():
        rec[k + "_ms"], rec[k + "_max_ms"] = round(med, 3), round(mx, 3)
        rec[k + "_io_gb_per_s"] = round(rec[k + "_io_bytes"] / med / 1e6, 1)
    rec["yardstick"] = "none: first measurement"
    emit(rec)
    for d in (ct, h0, h1, out, e0, e1, encd):
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
