"""Times of the general ring's collective bootstrap (sfgwas_amd/csrc/gring_refresh.hip) - one JSON line per case, appended to --out
(profiles/ring_refresh_bench.jsonl).

  P14    the general ring beside the specialised context on PN14QP438's own parameters: 1845 ciphertexts at level 4, the reference's scale pair (2^68, 2^34),
         four-limb masks, alternating in one run on the same device buffers: share generation (sfg_ring_refresh_gen_shares_scaled_dev / sfg_refresh_gen_shares_scaled_dev)
         and the finish (sfg_ring_refresh_finish_scaled_dev / sfg_refresh_finish_scaled_dev).  The aim: general / specialised at most 4.3 for each (what the general
         transform costs beside the specialised one); reported as met or missed, gates nothing.  The words of the two paths are compared on a
         sample of ciphertexts (first, last, every 16th) and must be equal.
  PN15   18 + 3 moduli at logN 15, 8 ciphertexts, level 2 -> 17, and
  PN16   34 + 4 moduli at logN 16, 8 ciphertexts, level 2 -> 33 (the chains tools/bench_ring.py builds), three-limb masks, both forms.  First measurements: no yardstick.

Host clock around single calls that end in a device synchronise, every shape warmed up first, --rounds (30) alternations: medians, the largest single time beside
them.  --only NAME restricts the timed calls to those whose key contains NAME (a profiler run of one call).  Input words are one block of 45 ciphertexts repeated:
no kernel's time depends on the values.  The CPU cost these calls replace (lattigo's dckks.RefreshProtocol) cannot be measured without a Go toolchain."""
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
ap.add_argument("--only", default="")
args = ap.parse_args()
L = capi.lib()
REF_PAIR = (2.0 ** 68, 2.0 ** 34)


def primes(logN, bits, count, skip=0):
    M, out, x = 2 << logN, [], (1 << bits) + 1 - (2 << logN)
    while len(out) < count + skip:
        if isprime(x):
            out.append(x)
        x -= M
    return out[skip:]


def timed(calls, sync, rounds):
    calls = {k: fn for k, fn in calls.items() if args.only in k}
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


def repeated(ring, block, nct):
    """a device buffer of nct items: the host block of some items, repeated"""
    per = block.nbytes // block.shape[0]
    d = ring.malloc(nct * per)
    for c0 in range(0, nct, block.shape[0]):
        n = min(block.shape[0], nct - c0)
        ring.check(L.sfg_ring_memcpy_h2d(ring.h, C.c_void_p(d.value + c0 * per), block.ctypes.data_as(C.c_void_p), n * per), "upload")
    return d


def inputs(ring, rnd, q, level, nct, W, block=45):
    N, nl, b = ring.N, level + 1, min(block, nct)
    Q = 1
    for m in q[:nl]:
        Q *= m
    masks = np.zeros((b, N, W), dtype=np.uint64)
    bound = min(Q // 8, 1 << (64 * W - 1))
    lim = rnd.integers(0, 1 << 62, (b, N, W + 1), dtype=np.uint64)
    for c in range(b):
        for x in range(0, N, 97):                                             # a spread of full-width signed masks; the rest one-limb values
            v = (sum(int(lim[c, x, i]) << (62 * i) for i in range(W + 1)) % (2 * bound)) - bound
            u = v % (1 << (64 * W))
            masks[c, x] = [(u >> (64 * i)) & ((1 << 64) - 1) for i in range(W)]
    masks[..., 0] |= lim[..., 0]
    d = {"ct": repeated(ring, uniform_rows(rnd, q[:nl], (b, 2), N), nct), "crs": repeated(ring, uniform_rows(rnd, q, (b,), N), nct),
         "mask": repeated(ring, masks, nct), "e0": repeated(ring, rnd.integers(-19, 20, (b, N)).astype(np.int32), nct),
         "e1": repeated(ring, rnd.integers(-19, 20, (b, N)).astype(np.int32), nct),
         "h0agg": repeated(ring, uniform_rows(rnd, q[:nl], (b,), N), nct), "h1agg": repeated(ring, uniform_rows(rnd, q, (b,), N), nct)}
    return d


def sample_equal(owner, a, b, per_bytes, nct):
    for c in sorted(set(range(0, nct, 16)) | {nct - 1}):
        off = c * per_bytes
        if not np.array_equal(owner.to_host(C.c_void_p(a.value + off), (per_bytes // 8,), np.uint64), owner.to_host(C.c_void_p(b.value + off), (per_bytes // 8,), np.uint64)):
            return False
    return True


def case_p14():
    q, p = list(P.Q_PN14), list(P.P_PN14)
    ctx, ring = capi.Context(q, p), capi.Ring(14, q, p)
    N, level, nct, W, nq = ctx.N, 4, args.p14_cts, 4, len(q)
    nl = level + 1
    rnd = np.random.default_rng(14)
    sk = uniform_rows(rnd, q, (), N)                                           # parity and time need no valid key
    ctx.load_secret_key(sk); ring.load_secret_key(sk)
    d = inputs(ring, rnd, q, level, nct, W)
    h0b, h1b, outb = nl * N * 8, nq * N * 8, 2 * nq * N * 8
    o = {k: ring.malloc(nct * n) for k, n in (("rh0", h0b), ("rh1", h1b), ("rout", outb), ("ch0", h0b), ("ch1", h1b), ("cout", outb))}
    s = REF_PAIR

    def both():
        ctx.sync(); ring.sync()
    calls = {"ring_gen_shares": lambda: ring.check(L.sfg_ring_refresh_gen_shares_scaled_dev(ring.h, d["ct"], nct, level, s[0], s[1], d["crs"], d["mask"], W, d["e0"], d["e1"], o["rh0"], o["rh1"]), "ring shares"),
             "ctx_gen_shares": lambda: ctx.check(L.sfg_refresh_gen_shares_scaled_dev(ctx.h, d["ct"], nct, level, s[0], s[1], d["crs"], d["mask"], W, d["e0"], d["e1"], o["ch0"], o["ch1"]), "ctx shares"),
             "ring_finish": lambda: ring.check(L.sfg_ring_refresh_finish_scaled_dev(ring.h, d["ct"], nct, level, s[0], s[1], d["h0agg"], d["h1agg"], d["crs"], o["rout"]), "ring finish"),
             "ctx_finish": lambda: ctx.check(L.sfg_refresh_finish_scaled_dev(ctx.h, d["ct"], nct, level, s[0], s[1], d["h0agg"], d["h1agg"], d["crs"], o["cout"]), "ctx finish")}
    for fn in calls.values():
        fn()
    both()
    equal = sample_equal(ring, o["rh0"], o["ch0"], h0b, nct) and sample_equal(ring, o["rh1"], o["ch1"], h1b, nct) and sample_equal(ring, o["rout"], o["cout"], outb, nct)
    t = timed(calls, both, args.rounds)
    rec = {"case": "P14", "logN": 14, "nq": nq, "np": len(p), "rounds": args.rounds, "cts": nct, "level": level, "mask_limbs": W, "scales": list(s),
           "words_equal_on_sample": equal, "sampled_cts": len(set(range(0, nct, 16)) | {nct - 1})}
    for k, (med, mx) in t.items():
        rec[k + "_ms"], rec[k + "_max_ms"] = round(med, 3), round(mx, 3)
    for what in ("gen_shares", "finish"):
        if "ring_" + what in t and "ctx_" + what in t:
            ratio = t["ring_" + what][0] / t["ctx_" + what][0]
            rec[what + "_ratio_general_over_specialised"], rec[what + "_ratio_aim"], rec[what + "_ratio_aim_met"] = round(ratio, 2), 4.3, bool(ratio <= 4.3)
    emit(rec)
    for x in list(d.values()) + list(o.values()):
        ring.free(x)
    ctx.close(); ring.close()
    if not equal:
        raise SystemExit("bench_ring_refresh: the two paths' words differ")


def case_wide(name, logN, q, p, nct, level=2, W=3):
    ring = capi.Ring(logN, q, p)
    N, nq, nl = ring.N, len(q), level + 1
    rnd = np.random.default_rng(logN)
    ring.load_secret_key(uniform_rows(rnd, q, (), N))
    d = inputs(ring, rnd, q, level, nct, W)
    h0, h1, out = ring.malloc(nct * nl * N * 8), ring.malloc(nct * nq * N * 8), ring.malloc(nct * 2 * nq * N * 8)
    s = REF_PAIR
    t = timed({"gen_shares": lambda: ring.check(L.sfg_ring_refresh_gen_shares_dev(ring.h, d["ct"], nct, level, d["crs"], d["mask"], W, d["e0"], d["e1"], h0, h1), "shares"),
               "gen_shares_scaled": lambda: ring.check(L.sfg_ring_refresh_gen_shares_scaled_dev(ring.h, d["ct"], nct, level, s[0], s[1], d["crs"], d["mask"], W, d["e0"], d["e1"], h0, h1), "shares"),
               "finish": lambda: ring.check(L.sfg_ring_refresh_finish_dev(ring.h, d["ct"], nct, level, d["h0agg"], d["h1agg"], d["crs"], out), "finish"),
               "finish_scaled": lambda: ring.check(L.sfg_ring_refresh_finish_scaled_dev(ring.h, d["ct"], nct, level, s[0], s[1], d["h0agg"], d["h1agg"], d["crs"], out), "finish")},
              ring.sync, args.rounds)
    rec = {"case": name, "logN": logN, "nq": nq, "np": len(p), "rounds": args.rounds, "cts": nct, "level": level, "level_out": nq - 1, "mask_limbs": W, "scales": list(s),
           "gen_shares_io_bytes": nct * N * (nl * 8 + nq * 8 + W * 8 + 8 + nl * 8 + nq * 8) + nq * N * 8,
           "finish_io_bytes": nct * N * 8 * (nl + nl + nq + nq + 2 * nq)}
    for k, (med, mx) in t.items():
        rec[k + "_ms"], rec[k + "_max_ms"] = round(med, 3), round(mx, 3)
    rec["yardstick"] = "none: first measurement"
    emit(rec)
    for x in list(d.values()) + [h0, h1, out]:
        ring.free(x)
    ring.close()


for case in args.cases.split(","):
    if case == "P14":
        case_p14()
    elif case == "PN15":
        case_wide("PN15", 15, primes(15, 50, 1) + primes(15, 40, 17), primes(15, 50, 3, skip=1), 8)
    elif case == "PN16":
        case_wide("PN16", 16, primes(16, 55, 1) + primes(16, 45, 33), primes(16, 55, 4, skip=1), 8)
    elif case == "PN12":                                                        # 2 + 1 moduli at logN 12: a rehearsal size, overheads only
        case_wide("PN12", 12, primes(12, 37, 1) + primes(12, 32, 1), primes(12, 38, 1), 2, level=0, W=1)
    else:
        raise SystemExit(f"unknown case {case}")
