"""Time of the collective key generation's local work (sfgwas_amd/csrc/keygen.hip) on the FULL key set of mpc.CollectiveInit: the Galois elements of
GenerateRotKeys(slots, 20, true) plus the conjugate, PN14 chain.  Per repetition, over the whole set in batches of 16 keys:
  gen      sfg_rtg_gen_shares_sampled_dev (errors drawn in the kernel)
  crp      sfg_crp_fill_dev for the same rows
  install  sfg_ctx_install_rotkeys_dev (device to device)
  (a)      sfg_ntt_rows on as many rows (nkeys * beta * (nq + np)): the measure DESIGN section 9 uses
  (b)      sfg_ctx_load_rotkey of as many keys from pinned host memory: what installation replaces on the device side
30 repetitions, the five legs alternating inside every repetition, each ending in a device synchronise under the host clock; medians.  Aim (reported, not a
gate): gen <= 2 x (a).  One JSON line; --out writes it to a file as well.  The CPU cost replaced (lattigo's GenShare per key) is NOT measured here."""
import argparse, ctypes as C, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from sfgwas_amd import capi, params as P

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--batch", type=int, default=16)
args = ap.parse_args()

ctx = capi.Context(P.Q_PN14, P.P_PN14)
L = capi.lib()
hip = C.CDLL("libamdhip64.so")
hip.hipHostMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t, C.c_uint]
hip.hipHostFree.argtypes = [C.c_void_p]
N, nmod, beta = ctx.N, ctx.nq + ctx.np_, ctx.beta
gal = P.galois_elements_for_rot_keys()
nkeys = len(gal)
poly_bytes = nmod * N * 8
key_bytes = beta * 2 * poly_bytes
print(f"key set: {nkeys} switching keys of [{beta}][2][{nmod}][{N}] words = {nkeys * key_bytes} bytes ({nkeys * key_bytes / 2 ** 30:.2f} GiB); "
      f"shares and common reference polynomials {nkeys * beta * poly_bytes} bytes each", flush=True)

rnd = np.random.default_rng(1)
ctx.load_secret_key_qp(np.stack([rnd.integers(0, q, N, dtype=np.uint64) for q in P.Q_PN14 + P.P_PN14]))      # uniform words: timing does not need a ternary key
ctx.seed_encryptor(os.urandom(32))
seed = os.urandom(32)
B = args.batch
batches = [gal[i:i + B] for i in range(0, nkeys, B)]
crp = capi.DevArray(ctx, (B * beta * nmod, N))
shares = capi.DevArray(ctx, (B * beta * nmod, N))
garr = [(C.c_uint64 * len(b))(*b) for b in batches]
mods = [(C.c_int * (len(b) * beta * nmod))(*(list(range(nmod)) * (len(b) * beta))) for b in batches]
pinned = C.c_void_p()
assert hip.hipHostMalloc(C.byref(pinned), key_bytes, 0) == 0
C.memset(pinned, 1, key_bytes)
pinned_u64 = C.cast(pinned, C.POINTER(C.c_uint64))


def gen():
    for b, g in zip(batches, garr):
        ctx.check(L.sfg_rtg_gen_shares_sampled_dev(ctx.h, g, len(b), crp.p, shares.p, None), "gen")


def fill():
    row = 0
    for b, m in zip(batches, mods):
        ctx.check(L.sfg_crp_fill_dev(ctx.h, seed, row, len(m), m, crp.p), "crp"); row += len(m)


def install():
    for b, g in zip(batches, garr):
        ctx.check(L.sfg_ctx_install_rotkeys_dev(ctx.h, g, len(b), shares.p, crp.p), "install")


def ntt():
    for b, m in zip(batches, mods):
        ctx.check(L.sfg_ntt_rows(ctx.h, shares.p, len(m), m), "ntt")


def upload():
    for g in gal:
        ctx.check(L.sfg_ctx_load_rotkey(ctx.h, g, pinned_u64, 0), "load_rotkey")


legs = {"gen": gen, "crp": fill, "install": install, "ntt_rows_same_count": ntt, "load_rotkey_pinned": upload}
times = {k: [] for k in legs}
for rep in range(args.reps + 1):                                  # repetition 0 warms every leg up (and allocates the key storage)
    for name, fn in legs.items():
        ctx.sync()
        t = time.perf_counter(); fn(); ctx.sync(); dt = time.perf_counter() - t
        if rep:
            times[name].append(dt)
med = {k: float(np.median(v)) for k, v in times.items()}
rec = {"nkeys": nkeys, "batch": B, "beta": beta, "nmod": nmod, "rows": nkeys * beta * nmod, "key_set_bytes": nkeys * key_bytes, "reps": args.reps,
       "median_ms": {k: round(v * 1e3, 3) for k, v in med.items()},
       "min_ms": {k: round(min(v) * 1e3, 3) for k, v in times.items()}, "max_ms": {k: round(max(v) * 1e3, 3) for k, v in times.items()},
       "gen_over_ntt_rows": round(med["gen"] / med["ntt_rows_same_count"], 3), "aim_gen_within_2x_ntt_rows": "met" if med["gen"] <= 2 * med["ntt_rows_same_count"] else "missed",
       "crp_over_ntt_rows": round(med["crp"] / med["ntt_rows_same_count"], 3), "install_over_load_rotkey": round(med["install"] / med["load_rotkey_pinned"], 3)}
print(json.dumps(rec), flush=True)
hip.hipHostFree(pinned)
crp.free(); shares.free()
ctx.close()
if args.out:
    with open(args.out, "w") as f:
        f.write(json.dumps(rec) + "\n")
