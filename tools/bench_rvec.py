"""Time of the ring-vector encoder and decoder (sfgwas_amd/csrc/rvec.hip) at the association scan's own workload - computeStdInv's CVecToSS -> SqrtInv -> SSToCVec
over ceil(1M SNPs / 8192 slots) = 123 ciphertexts, mpc_field_size 256 (limbs = 4), mpc_frac_bits 30, scale 2^34: sfg_rvec_encode_dev at level 9, sfg_rvec_decode_dev
at levels 9 and 5 - and, in the same run and alternating with them, the double-double calls sfg_encode_vectors_dev and sfg_decode_vectors_dev on the same count and
levels as the yardstick.  Host clock around single calls that end in a device synchronise, every shape warmed up first, `--rounds` (30) alternations: medians, and the
largest single time (`max_ms`) beside them.  No pass / fail aim.  One JSON line; --out writes it to a file as well.  Per pass: the bytes a pass of the transform moves
through HBM (2 W 65,536 B read and written per ciphertext), for the rate once a kernel trace gives its time.  The CPU cost this replaces (the fork's big.Float
embedding per ciphertext) is NOT measured here: there is no Go toolchain."""
import argparse, ctypes as C, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from sfgwas_amd import capi, params as P

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--nct", type=int, default=123)
ap.add_argument("--rounds", type=int, default=30)
args = ap.parse_args()

ctx = capi.Context(P.Q_PN14, P.P_PN14)
L = capi.lib()
N, n, nct = ctx.N, ctx.slots, args.nct
limbs, f, scale = 4, 30, 2.0 ** 34
p = 2 ** 256 - 189
mod = np.array([(p >> (64 * i)) & (2 ** 64 - 1) for i in range(limbs)], dtype=np.uint64)
rnd = np.random.default_rng(1)
shares = np.frombuffer(rnd.bytes(nct * n * limbs * 8), dtype=np.uint64).reshape(nct, n, limbs).copy()
shares[..., limbs - 1] >>= np.uint64(1)                                       # below p: timing does not need more
d_sh = capi.DevArray.from_host(ctx, shares)
d_out = capi.DevArray(ctx, (nct, n, limbs))
vals = rnd.uniform(-1, 1, (nct, n))
vp = vals.ctypes.data_as(C.POINTER(C.c_double))
d_re = capi.DevArray(ctx, (nct, n), np.float64)
pts = {lv: ctx.fill_uniform_cts((nct + 1) // 2, lv, 7 + lv) for lv in (9, 5)}            # uniform words read as plaintext rows [nct][level+1][N]
d_pt9 = capi.DevArray(ctx, (nct, 10, N))

calls = {
    "rvec_encode_l9": lambda: ctx.check(L.sfg_rvec_encode_dev(ctx.h, limbs, capi.p64(mod), d_sh.p, n, nct, 9, scale, f, d_pt9.p), "rvec_encode"),
    "encode_vectors_l9": lambda: ctx.check(L.sfg_encode_vectors_dev(ctx.h, vp, nct, 9, d_pt9.p), "encode_vectors"),
    "rvec_decode_l9": lambda: ctx.check(L.sfg_rvec_decode_dev(ctx.h, limbs, capi.p64(mod), pts[9].p, 10 * N, nct, 9, scale, f, n, d_out.p), "rvec_decode"),
    "decode_vectors_l9": lambda: ctx.check(L.sfg_decode_vectors_dev(ctx.h, pts[9].p, 10 * N, nct, 9, scale, d_re.p, None), "decode_vectors"),
    "rvec_decode_l5": lambda: ctx.check(L.sfg_rvec_decode_dev(ctx.h, limbs, capi.p64(mod), pts[5].p, 6 * N, nct, 5, scale, f, n, d_out.p), "rvec_decode"),
    "decode_vectors_l5": lambda: ctx.check(L.sfg_decode_vectors_dev(ctx.h, pts[5].p, 6 * N, nct, 5, scale, d_re.p, None), "decode_vectors"),
}
for fn in calls.values():                                                      # warm-up: code objects, scratch
    fn(); fn(); ctx.sync()
t = {k: [] for k in calls}
for _ in range(args.rounds):
    for k, fn in calls.items():
        t0 = time.perf_counter(); fn(); ctx.sync(); t[k].append(time.perf_counter() - t0)
rec = {"nct": nct, "limbs": limbs, "frac_bits": f, "log2_scale": 34, "rounds": args.rounds,
       "words": {"rvec_encode_l9": 5, "rvec_decode_l9": 7, "rvec_decode_l5": 5}}
for k, v in t.items():
    rec[k + "_ms"] = round(float(np.median(v)) * 1e3, 3)
    rec[k + "_max_ms"] = round(float(np.max(v)) * 1e3, 3)
for a, b in (("rvec_encode_l9", "encode_vectors_l9"), ("rvec_decode_l9", "decode_vectors_l9"), ("rvec_decode_l5", "decode_vectors_l5")):
    rec[a + "_over_" + b] = round(rec[a + "_ms"] / rec[b + "_ms"], 2)
rec["pass_bytes"] = {k: 2 * 2 * w * 65536 * nct for k, w in rec["words"].items()}          # read + write of one pass over the call's ciphertexts
rec["cpu_cost_replaced"] = "not measured (no Go toolchain)"
print(json.dumps(rec), flush=True)
for a in (d_sh, d_out, d_re, d_pt9, pts[9], pts[5]):
    a.free()
ctx.close()
if args.out:
    with open(args.out, "w") as fh:
        fh.write(json.dumps(rec) + "\n")
