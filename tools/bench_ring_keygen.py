"""Time of the general ring's collective key generation (sfgwas_amd/csrc/gring_keygen.hip), in the shape of tools/bench_keygen.py.  Three workloads:
  p14    PN14's parameters, the full set of mpc.CollectiveInit (GenerateRotKeys(slots, 20, true) plus the conjugate: 212 keys) in batches of 16, as DESIGN 11 measured it
  pn15   16 keys at 18 + 3 moduli, logN 15 (beta = 6)
  pn16   4 keys at 34 + 4 moduli, logN 16 (beta = 9)
Per repetition, over the workload's keys in its batches:
  gen      sfg_ring_rtg_gen_shares_sampled_dev (errors drawn on the device)
  crp      sfg_ring_crp_fill_dev for the same rows
  install  sfg_ring_install_rotkeys_dev (device to device)
  (a)      sfg_ring_ntt_rows on as many rows (nkeys * beta * (nq + np)): the yardstick of share generation
  (b)      sfg_ring_load_rotkey of as many keys from pinned host memory: the yardstick of installation
30 repetitions, the five legs alternating inside every repetition, each ending in a device synchronise under the host clock; medians.  Aims (reported, never a
gate): gen <= 2.0 x (a), install <= 0.25 x (b); crp has no yardstick.  Without --workload every workload runs in a fresh child process under its own time limit
and the run stops at the first that fails; one JSON line per workload, appended to --out.  The CPU cost replaced (lattigo's GenShare per key) is NOT measured here."""
import argparse, ctypes as C, json, os, subprocess, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WORKLOADS = {"p14": 240, "pn15": 240, "pn16": 300}           # name -> time limit of its child process in seconds

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--workload", choices=list(WORKLOADS), default=None)
args = ap.parse_args()

if args.workload is None:
    for name, limit in WORKLOADS.items():
        cmd = [sys.executable, os.path.abspath(__file__), "--workload", name, "--reps", str(args.reps)] + (["--out", args.out] if args.out else [])
        try:
            rc = subprocess.run(cmd, timeout=limit).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc:
            print(f"workload {name} ended with status {rc}: nothing more is started", flush=True)
            sys.exit(rc)
    sys.exit(0)

import numpy as np
from sfgwas_amd import capi, params as P


def is_prime(n):
    if n < 2:
        return False
    for p in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37):
        if n % p == 0:
            return n == p
    d, s = n - 1, 0
    while d % 2 == 0:
        d, s = d // 2, s + 1
    for a in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37):       # deterministic below 2^64
        x = pow(a, d, n)
        if x in (1, n - 1):
            continue
        for _ in range(s - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


def primes_below(logN, bits, count, skip=0):
    """NTT-friendly primes == 1 mod 2N just below 2^bits"""
    M, out, x = 2 << logN, [], (1 << bits) + 1 - (2 << logN)
    while len(out) < count + skip:
        if is_prime(x):
            out.append(x)
        x -= M
    return out[skip:]


if args.workload == "p14":
    logN, q, p, batch = 14, list(P.Q_PN14), list(P.P_PN14), 16
    gal = list(P.galois_elements_for_rot_keys())
elif args.workload == "pn15":
    logN, q, p, batch = 15, primes_below(15, 50, 1) + primes_below(15, 40, 17), primes_below(15, 50, 3, skip=1), 16
    gal = None
else:
    logN, q, p, batch = 16, primes_below(16, 55, 1) + primes_below(16, 45, 33), primes_below(16, 55, 4, skip=1), 4
    gal = None
ring = capi.Ring(logN, q, p)
if gal is None:
    gal = [ring.galois(k) for k in range(1, batch + 1)]
L = capi.lib()
hip = C.CDLL("libamdhip64.so")
hip.hipHostMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t, C.c_uint]
hip.hipHostFree.argtypes = [C.c_void_p]
N, nmod, beta, nkeys = ring.N, len(ring.moduli), ring.beta, len(gal)
poly_bytes = nmod * N * 8
key_bytes = beta * 2 * poly_bytes
print(f"{args.workload}: {nkeys} switching keys of [{beta}][2][{nmod}][{N}] words = {nkeys * key_bytes} bytes ({nkeys * key_bytes / 2 ** 30:.2f} GiB) in batches of {batch}; "
      f"shares and common reference polynomials {nkeys * beta * poly_bytes} bytes each", flush=True)

rnd = np.random.default_rng(1)
ring.load_secret_key_qp(np.stack([rnd.integers(0, m, N, dtype=np.uint64) for m in ring.moduli]))      # uniform words: timing does not need a ternary key
ring.seed_encryptor(os.urandom(32))
seed = os.urandom(32)
batches = [gal[i:i + batch] for i in range(0, nkeys, batch)]
crp, shares = ring.malloc(batch * beta * poly_bytes), ring.malloc(batch * beta * poly_bytes)
garr = [(C.c_uint64 * len(b))(*b) for b in batches]
mods = [(C.c_int * (len(b) * beta * nmod))(*(list(range(nmod)) * (len(b) * beta))) for b in batches]
pinned = C.c_void_p()
assert hip.hipHostMalloc(C.byref(pinned), key_bytes, 0) == 0
C.memset(pinned, 0, key_bytes)
pinned_u64 = C.cast(pinned, C.POINTER(C.c_uint64))


def gen():
    for b, g in zip(batches, garr):
        ring.check(L.sfg_ring_rtg_gen_shares_sampled_dev(ring.h, g, len(b), crp, shares, None), "gen")


def fill():
    row = 0
    for b, m in zip(batches, mods):
        ring.check(L.sfg_ring_crp_fill_dev(ring.h, seed, row, len(m), m, crp), "crp"); row += len(m)


def install():
    for b, g in zip(batches, garr):
        ring.check(L.sfg_ring_install_rotkeys_dev(ring.h, g, len(b), shares, crp), "install")


def ntt():
    for b, m in zip(batches, mods):
        ring.check(L.sfg_ring_ntt_rows(ring.h, shares, len(m), m), "ntt")


def upload():
    for g in gal:
        ring.check(L.sfg_ring_load_rotkey(ring.h, g, pinned_u64, 0), "load_rotkey")


legs = {"gen": gen, "crp": fill, "install": install, "ntt_rows_same_count": ntt, "load_rotkey_pinned": upload}
times = {k: [] for k in legs}
for rep in range(args.reps + 1):                                  # repetition 0 warms every leg up (and allocates the key storage)
    for name, fn in legs.items():
        ring.sync()
        t = time.perf_counter(); fn(); ring.sync(); dt = time.perf_counter() - t
        if rep:
            times[name].append(dt)
med = {k: float(np.median(v)) for k, v in times.items()}
rec = {"workload": args.workload, "logN": logN, "nq": len(q), "np": len(p), "nkeys": nkeys, "batch": batch, "beta": beta, "nmod": nmod, "rows": nkeys * beta * nmod,
       "key_set_bytes": nkeys * key_bytes, "reps": args.reps,
       "median_ms": {k: round(v * 1e3, 3) for k, v in med.items()},
       "min_ms": {k: round(min(v) * 1e3, 3) for k, v in times.items()}, "max_ms": {k: round(max(v) * 1e3, 3) for k, v in times.items()},
       "gen_over_ntt_rows": round(med["gen"] / med["ntt_rows_same_count"], 3), "aim_gen_within_2x_ntt_rows": "met" if med["gen"] <= 2.0 * med["ntt_rows_same_count"] else "missed",
       "install_over_load_rotkey": round(med["install"] / med["load_rotkey_pinned"], 3),
       "aim_install_within_0.25x_load_rotkey": "met" if med["install"] <= 0.25 * med["load_rotkey_pinned"] else "missed",
       "crp_over_ntt_rows": round(med["crp"] / med["ntt_rows_same_count"], 3)}
print(json.dumps(rec), flush=True)
hip.hipHostFree(pinned)
ring.free(crp); ring.free(shares)
ring.close()
if args.out:
    with open(args.out, "a") as f:
        f.write(json.dumps(rec) + "\n")
