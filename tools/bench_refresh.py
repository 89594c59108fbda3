"""Time of the collective bootstrap's local work (sfgwas_amd/csrc/refresh.hip): one round trip sfg_refresh_gen_shares_dev -> sfg_refresh_finish_dev, and
sfg_ckks_to_ss_share_dev, on `--nct` (64) ciphertexts at level `--level` (4) with `--limbs` (8) 64-bit mask limbs, everything resident on the device.  The words are
uniform (the aggregation over the network is not part of it: the party's own shares stand in for the aggregate), which is all a timing needs.  Host clock around
single calls that end in a device synchronise, every call warmed up first, `--rounds` (30) alternations: medians, and the largest single time beside them.
No pass / fail aim.  One JSON line; --out writes it to a file as well."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from sfgwas_amd import capi, params as P

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--nct", type=int, default=64)
ap.add_argument("--level", type=int, default=4)
ap.add_argument("--limbs", type=int, default=8)
ap.add_argument("--rounds", type=int, default=30)
args = ap.parse_args()

ctx = capi.Context(P.Q_PN14, P.P_PN14)
L = capi.lib()
N, nq, nct, level, W = ctx.N, ctx.nq, args.nct, args.level, args.limbs
nl = level + 1
rnd = np.random.default_rng(1)
ctx.load_secret_key(np.stack([rnd.integers(0, q, N, dtype=np.uint64) for q in P.Q_PN14]))
cts = ctx.fill_uniform_cts(nct, level, 11)
crs = ctx.fill_uniform_cts((nct + 1) // 2, nq - 1, 12)                         # uniform words read as [nct][nq][N]
mask = capi.DevArray.from_host(ctx, np.frombuffer(rnd.bytes(nct * N * W * 8), dtype=np.uint64).reshape(nct, N, W).copy())
e0 = capi.DevArray.from_host(ctx, rnd.integers(-19, 20, (nct, N)).astype(np.int32))
e1 = capi.DevArray.from_host(ctx, rnd.integers(-19, 20, (nct, N)).astype(np.int32))
h0, h1 = capi.DevArray(ctx, (nct, nl, N)), capi.DevArray(ctx, (nct, nq, N))
m_ntt = capi.DevArray(ctx, (nct, nl, N))
out = capi.DevArray(ctx, (nct, 2, nq, N))

calls = {
    "gen_shares": lambda: ctx.check(L.sfg_refresh_gen_shares_dev(ctx.h, cts.p, nct, level, crs.p, mask.p, W, e0.p, e1.p, h0.p, h1.p), "refresh_gen_shares"),
    "finish": lambda: ctx.check(L.sfg_refresh_finish_dev(ctx.h, cts.p, nct, level, h0.p, h1.p, crs.p, out.p), "refresh_finish"),
    "ckks_to_ss_share": lambda: ctx.check(L.sfg_ckks_to_ss_share_dev(ctx.h, cts.p, nct, level, mask.p, W, e0.p, h0.p, m_ntt.p), "ckks_to_ss_share"),
}
for fn in calls.values():                                                      # warm-up: code objects, scratch
    fn(); fn(); ctx.sync()
t = {k: [] for k in calls}
for _ in range(args.rounds):
    for k, fn in calls.items():
        t0 = time.perf_counter(); fn(); ctx.sync(); t[k].append(time.perf_counter() - t0)
rec = {"nct": nct, "level": level, "limbs": W, "rounds": args.rounds}
for k, v in t.items():
    rec[k + "_ms"] = round(float(np.median(v)) * 1e3, 3)
    rec[k + "_max_ms"] = round(float(np.max(v)) * 1e3, 3)
rec["round_trip_ms"] = round(rec["gen_shares_ms"] + rec["finish_ms"], 3)
print(json.dumps(rec), flush=True)
for a in (cts, crs, mask, e0, e1, h0, h1, m_ntt, out):
    a.free()
ctx.close()
if args.out:
    with open(args.out, "w") as fh:
        fh.write(json.dumps(rec) + "\n")
