"""Times of the general ring's matrix product (sfgwas_amd/csrc/gring_matmul.hip) - one JSON line per case, appended to --out (profiles/ring_matmul_bench.jsonl).

  P14    one 8192 x 8192 block on PN14QP438's own parameters, in_level = max_level = 9, s ciphertexts (64: the rotation batch of tools/bench_ring.py), three paths
         alternating in one run:
           fused      sfg_ring_matmul_dev
           composed   the same product from entry points that existed before it: sfg_ring_rotate_right_dev per baby (a batch of s), sfg_ring_ct_drop_level_dev to
                      the plaintexts' level, per giant sfg_ring_encode_vectors_dev of its diagonals in one call (the slot vectors are made on the host beforehand and
                      not timed), sfg_ring_ct_mul_plain_dev and sfg_ring_ct_add_dev per diagonal, sfg_ring_rotate_right_dev and sfg_ring_ct_add_dev per giant
           context    sfg_matmul_resident_dev of the specialised context (int8 matrix core, fp64 transforms)
         The three outputs must be equal word for word.  Condition: fused / composed <= 1.0.  fused / context is recorded; no aim is set for it.
  PN15   one block at 18 + 3 moduli, logN 15, and
  PN16   one block at 34 + 4 moduli, logN 16 (the chains tools/bench_ring.py builds), at s = 1 and s = 8: first measurements, no yardstick.

Keys are uniform words (capi.random_rotkey): the words of a product need no valid key.  Host clock around single calls that
end in a device synchronise, every path warmed up first, --rounds (30) alternations: medians, the largest single time beside them."""
import argparse, ctypes as C, json, math, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from sfgwas_amd import capi, params as P

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--rounds", type=int, default=30)
ap.add_argument("--cases", default="P14,PN15,PN16")
ap.add_argument("--s", type=int, default=64, help="P14: ciphertexts")
ap.add_argument("--block", type=int, default=0, help="rows and columns of the matrix (0: one full block, slots x slots)")
ap.add_argument("--once", action="store_true", help="one fused call per case and no timing (for a kernel trace)")
args = ap.parse_args()
L = capi.lib()
SCALE = 2.0 ** 34


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
        fn(); sync()
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


def rotations(n, dim):
    """left rotations of a dim x dim block at n slots: babies 1 .. d-1 and d g"""
    d = math.isqrt(n - 1) + 1
    shifts = [s for s in range(n) if s < dim or s > n - dim]
    return d, sorted({s % d for s in shifts} - {0}), sorted({(s // d) * d for s in shifts} - {0})


def uniform_cts(ring, q, s, level, seed):
    rnd = np.random.default_rng(seed)
    cts = np.empty((s, 1, 2, level + 1, ring.N), dtype=np.uint64)
    for m in range(level + 1):
        cts[:, :, :, m] = rnd.integers(0, q[m], (s, 1, 2, ring.N), dtype=np.uint64)
    return cts


class Composed:
    """the product of one block from the ring's other entry points, ciphertexts resident"""

    def __init__(self, ring, A, s, level, max_level, geno, scale):
        self.ring, self.A, self.s, self.level, self.L, self.scale = ring, A, s, level, max_level, scale
        n, N = ring.slots, ring.N
        self.d, babies, giants = rotations(n, geno.shape[0])
        self.babies = [0] + babies
        X = np.where(geno < 0, 0, geno).astype(np.float64)
        j = np.arange(n)
        ok_j = j < X.shape[1]
        self.giants = []                                   # (g, [babies], slot vectors [nb][n]) made once, outside the timing
        for g in sorted({0} | {x // self.d for x in giants}):
            bs, vals = [], []
            for b in self.babies:
                shift = g * self.d + b
                if shift >= n or not (shift < geno.shape[0] or shift > n - geno.shape[1] or shift == 0):
                    continue
                i = (shift + j) % n
                ok = ok_j & (i < X.shape[0])
                v = np.zeros(n)
                v[ok] = X[i[ok], j[ok]]
                bs.append(b)
                vals.append(np.roll(v, g * self.d))
            if bs:
                self.giants.append((g, bs, np.ascontiguousarray(np.stack(vals))))
        ctw_in, ctw = 2 * (level + 1) * N * 8, 2 * max_level * N * 8
        self.rot = {b: ring.malloc(s * ctw_in) for b in self.babies if b}
        self.low = {b: ring.malloc(s * ctw) for b in self.babies}
        self.pt = ring.malloc(max(len(bs) for _, bs, _ in self.giants) * max_level * N * 8)
        self.acc, self.tmp, self.out = ring.malloc(s * ctw), ring.malloc(s * ctw), ring.malloc(s * ctw)
        self.ctw = ctw

    def run(self):
        r, s, lvl, pl = self.ring, self.s, self.level, self.L - 1
        ck = r.check
        for b in self.babies:
            src = self.A
            if b:
                ck(L.sfg_ring_rotate_right_dev(r.h, self.A, self.rot[b], s, lvl, (C.c_int * s)(*([-b] * s))), "rotate")
                src = self.rot[b]
            ck(L.sfg_ring_ct_drop_level_dev(r.h, src, self.low[b], s, lvl, pl), "drop")
        first_out = True
        for g, bs, vals in self.giants:
            ck(L.sfg_ring_encode_vectors_dev(r.h, vals.ctypes.data_as(C.POINTER(C.c_double)), len(bs), pl, self.scale, self.pt), "encode")
            ptw = self.L * r.N * 8
            for k, b in enumerate(bs):
                pt = C.c_void_p(self.pt.value + k * ptw)
                if k == 0:
                    ck(L.sfg_ring_ct_mul_plain_dev(r.h, self.low[b], pt, 0, self.acc, s, pl), "mul_plain")
                else:
                    ck(L.sfg_ring_ct_mul_plain_dev(r.h, self.low[b], pt, 0, self.tmp, s, pl), "mul_plain")
                    ck(L.sfg_ring_ct_add_dev(r.h, self.acc, self.tmp, self.acc, s, pl), "add")
            src = self.acc
            if g:
                ck(L.sfg_ring_rotate_right_dev(r.h, self.acc, self.tmp, s, pl, (C.c_int * s)(*([-g * self.d] * s))), "rotate")
                src = self.tmp
            if first_out:
                ck(L.sfg_ring_ct_drop_level_dev(r.h, src, self.out, s, pl, pl), "copy")        # level_out == level_in copies
                first_out = False
            else:
                ck(L.sfg_ring_ct_add_dev(r.h, self.out, src, self.out, s, pl), "add")

    def free(self):
        for p in list(self.rot.values()) + list(self.low.values()) + [self.pt, self.acc, self.tmp, self.out]:
            self.ring.free(p)


def case_p14():
    q, p = list(P.Q_PN14), list(P.P_PN14)
    ctx, ring = capi.Context(q, p), capi.Ring(14, q, p)
    N, n, level, s = ring.N, ring.slots, 9, args.s
    dim = args.block or n
    d, babies, giants = rotations(n, dim)
    for k in babies + giants:
        g, key = ring.galois(k), capi.random_rotkey(q + p, ring.beta, N, 5 + k)
        ctx.load_rotkey(g, key); ring.load_rotkey(g, key)
    geno = np.random.default_rng(1).integers(-1, 3, (dim, dim)).astype(np.int8)
    A_host = uniform_cts(ring, q, s, level, 2)
    A, G = ring.to_device(A_host), ring.to_device(geno)
    outw = s * 2 * level * N
    fused = ring.malloc(outw * 8)

    def run_fused():
        ring.check(L.sfg_ring_matmul_dev(ring.h, A, s, level, level, G, dim, dim, dim, 0, SCALE, fused), "matmul")
    if args.once:
        run_fused(); ring.sync()
        return
    comp = Composed(ring, A, s, level, level, geno, SCALE)
    cA = capi.DevArray.from_host(ctx, A_host)
    cg = ctx.geno_upload(geno)
    held = {}

    def run_ctx():
        if "o" in held:
            held["o"].free()
        held["o"] = ctx.matmul_resident(cA, s, level, level, cg)

    def both():
        ring.sync(); ctx.sync()
    t = timed({"fused": run_fused, "composed": comp.run, "context": run_ctx}, both, args.rounds)
    got = ring.to_host(fused, (outw,))
    eq_comp = bool(np.array_equal(got, ring.to_host(comp.out, (outw,))))
    eq_ctx = bool(np.array_equal(got, held["o"].host().reshape(-1)))
    ratio = t["fused"][0] / t["composed"][0]
    rec = {"case": "P14", "logN": 14, "nq": len(q), "np": len(p), "rounds": args.rounds, "s": s, "block": dim, "in_level": level, "max_level": level, "diagonals": sum(len(b) for _, b, _ in comp.giants),
           "words_equal_composed": eq_comp, "words_equal_context": eq_ctx}
    for k, (med, mx) in t.items():
        rec[k + "_ms"], rec[k + "_max_ms"] = round(med, 3), round(mx, 3)
    rec["ratio_fused_over_composed"] = round(ratio, 3)
    rec["ratio_condition"] = 1.0
    rec["ratio_condition_met"] = bool(ratio <= 1.0)
    rec["ratio_fused_over_context"] = round(t["fused"][0] / t["context"][0], 2)
    rec["ratio_fused_over_context_aim"] = "none"
    emit(rec)
    comp.free(); held["o"].free(); cA.free(); ctx.geno_free(cg)
    for d_ in (A, G, fused):
        ring.free(d_)
    ctx.close(); ring.close()
    if not (eq_comp and eq_ctx):
        raise SystemExit("bench_ring_matmul: the paths' words differ")


def case_wide(name, logN, q, p):
    ring = capi.Ring(logN, q, p)
    N, n, level, mods = ring.N, ring.slots, len(q) - 1, q + p
    dim = args.block or n
    d, babies, giants = rotations(n, dim)
    key = capi.random_rotkey(mods, ring.beta, N, 5)          # one set of uniform words under every Galois element: the time of a key switch does not depend on them
    for k in babies + giants:
        ring.load_rotkey(ring.galois(k), key)
    geno = np.random.default_rng(1).integers(-1, 3, (dim, dim)).astype(np.int8)
    G = ring.to_device(geno)
    rec = {"case": name, "logN": logN, "nq": len(q), "np": len(p), "beta": ring.beta, "rounds": args.rounds, "block": dim, "in_level": level, "max_level": level, "d": d,
           "keys": len(babies) + len(giants), "yardstick": "none: first measurement"}
    for s in (1, 8):
        A = ring.to_device(uniform_cts(ring, q, s, level, 2))
        out = ring.malloc(s * 2 * level * N * 8)

        def run():
            ring.check(L.sfg_ring_matmul_dev(ring.h, A, s, level, level, G, dim, dim, dim, 0, SCALE, out), "matmul")
        if args.once:
            run(); ring.sync()
        else:
            med, mx = timed({"fused": run}, ring.sync, args.rounds)["fused"]
            rec[f"s{s}_ms"], rec[f"s{s}_max_ms"] = round(med, 3), round(mx, 3)
        ring.free(A); ring.free(out)
    if not args.once:
        emit(rec)
    ring.free(G)
    ring.close()


for case in args.cases.split(","):
    if case == "P14":
        case_p14()
    elif case == "PN15":
        case_wide("PN15", 15, primes(15, 50, 1) + primes(15, 40, 17), primes(15, 50, 3, skip=1))
    elif case == "PN16":
        case_wide("PN16", 16, primes(16, 55, 1) + primes(16, 45, 33), primes(16, 55, 4, skip=1))
    elif case == "PN12":                                                        # 2 + 1 moduli at logN 12: a rehearsal size
        case_wide("PN12", 12, primes(12, 37, 1) + primes(12, 32, 1), primes(12, 38, 1))
    else:
        raise SystemExit(f"unknown case {case}")
