"""Time of the device encryption (sfgwas_amd/csrc/encrypt.hip) at the shapes one power iteration of the quoted configuration asks for (100 000 x 1 000 000, kp = 15):
sfg_ct_add_fresh_zero_dev for 1845 and 195 ciphertexts at level 4, sfg_encrypt_vectors_dev for 15 x 13 vectors at level 9 - and, in the same run and alternating with
them, the library's own sfg_ntt_rows / sfg_intt_rows on the SAME NUMBER of row transforms (per ciphertext 3 (l + 1 + np) + 2 (l + 1) forward, 2 np inverse).  The
fused call should stay within 2 x that transform time.  Host clock around repetitions that end in a device synchronise; every shape warmed up first.
One JSON line per shape; --out writes them to a file as well.  The CPU cost this replaces (lattigo's EncryptNew, one ciphertext at a time) is NOT measured here."""
import argparse, ctypes as C, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from sfgwas_amd import capi, params as P

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--min-window", type=float, default=0.6, help="seconds of timed work per measurement")
args = ap.parse_args()

ctx = capi.Context(P.Q_PN14, P.P_PN14)
L = capi.lib()
hip = C.CDLL("libamdhip64.so")
hip.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
N, nq, np_ = ctx.N, ctx.nq, ctx.np_
rnd = np.random.default_rng(1)
pk = np.stack([np.stack([rnd.integers(0, q, N, dtype=np.uint64) for q in P.Q_PN14 + P.P_PN14]) for _ in range(2)])      # uniform words: timing does not need a valid key
ctx.load_public_key(pk)
ctx.seed_encryptor(os.urandom(32))


def timed(fn):
    fn(); ctx.sync()                                              # warm-up of this shape
    t = time.perf_counter(); fn(); ctx.sync(); one = time.perf_counter() - t
    reps = max(3, int(args.min_window / max(one, 1e-6)))
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    ctx.sync()
    return (time.perf_counter() - t) / reps, reps


lines = []
for what, nct, level in (("add_fresh_zero", 1845, 4), ("add_fresh_zero", 195, 4), ("encrypt_vectors", 15 * 13, 9)):
    nl, nt = level + 1, level + 1 + np_
    fwd_rows, inv_rows = nct * (3 * nt + 2 * nl), nct * 2 * np_
    cts = ctx.fill_uniform_cts(nct, level, 7)
    vals = rnd.uniform(-1, 1, (nct, ctx.slots))
    vp = vals.ctypes.data_as(C.POINTER(C.c_double))
    if what == "add_fresh_zero":
        fused = lambda: ctx.check(L.sfg_ct_add_fresh_zero_dev(ctx.h, cts.p, nct, level), what)
    else:
        fused = lambda: ctx.check(L.sfg_encrypt_vectors_dev(ctx.h, vp, nct, level, cts.p), what)
        encode_only = lambda: ctx.check(L.sfg_encode_vectors_dev(ctx.h, vp, nct, level, cts.p), "encode")
    # the same number of row transforms by the library's own row NTTs, in place on a buffer of nct * nt rows (the shape of the encryption's scratch)
    rows = capi.DevArray(ctx, (nct * max(nt, 2 * nl), N))
    hip.hipMemset(rows.p, 0, rows.nbytes)                         # (fp64 butterflies: the time does not depend on the words)
    tmods = list(range(nl)) + [nq + k for k in range(np_)]
    m_t = (C.c_int * (nct * nt))(*(tmods * nct)); m_q = (C.c_int * (nct * 2 * nl))(*(list(range(nl)) * (2 * nct))); m_p = (C.c_int * inv_rows)(*([nq + k for k in range(np_)] * (2 * nct)))

    def transforms():
        for _ in range(3):
            ctx.check(L.sfg_ntt_rows(ctx.h, rows.p, nct * nt, m_t), "ntt")
        ctx.check(L.sfg_ntt_rows(ctx.h, rows.p, nct * 2 * nl, m_q), "ntt")
        ctx.check(L.sfg_intt_rows(ctx.h, rows.p, inv_rows, m_p), "intt")

    t_f, t_n = [], []
    for _ in range(3):                                            # alternate the two, three times: the spread is part of the result
        t_f.append(timed(fused)[0]); t_n.append(timed(transforms)[0])
    rec = {"call": what, "nct": nct, "level": level, "row_transforms": fwd_rows + inv_rows, "fused_ms": [round(x * 1e3, 3) for x in t_f],
           "ntt_rows_same_count_ms": [round(x * 1e3, 3) for x in t_n], "ratio_of_medians": round(float(np.median(t_f) / np.median(t_n)), 3)}
    if what == "encrypt_vectors":
        t_e = timed(encode_only)[0]                               # includes the host-to-device copy of the values and the encoder's synchronise
        rec["encode_vectors_alone_ms"] = round(t_e * 1e3, 3)
        rec["ratio_without_encode"] = round(float((np.median(t_f) - t_e) / np.median(t_n)), 3)
    lines.append(rec)
    print(json.dumps(rec), flush=True)
    rows.free(); cts.free()
ctx.close()
if args.out:
    with open(args.out, "w") as f:
        for r in lines:
            f.write(json.dumps(r) + "\n")
