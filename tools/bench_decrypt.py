"""Time of the device decryption and decoding (sfgwas_amd/csrc/decrypt.hip) at the count tools/bench_encrypt.py uses: sfg_decrypt_vectors and sfg_pcks_finish_decode
for 1845 ciphertexts at level 4 (real parts only, the common call; and with the imaginary parts) - and, in the same run and alternating with them, sfg_intt_rows on
the number of rows the call transforms (nct * (level + 1)) and sfg_encrypt_vectors_dev on 1845 vectors at level 4.  The aim: decoding 1845 ciphertexts costs no more
than encrypting 1845 vectors.  Host clock around repetitions that end in a device synchronise (the decode calls synchronise themselves and include the download of
their results; the encryption includes the upload of its values); every shape warmed up first; three alternations, all three figures kept: the spread is part of the
result.  One JSON line; --out writes it to a file as well.  The CPU cost this replaces (lattigo's decoder) is NOT measured here."""
import argparse, ctypes as C, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from sfgwas_amd import capi, params as P

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--nct", type=int, default=1845)
ap.add_argument("--level", type=int, default=4)
ap.add_argument("--min-window", type=float, default=0.6, help="seconds of timed work per measurement")
args = ap.parse_args()

ctx = capi.Context(P.Q_PN14, P.P_PN14)
L = capi.lib()
N, nq, np_ = ctx.N, ctx.nq, ctx.np_
nct, level = args.nct, args.level
nl = level + 1
rnd = np.random.default_rng(1)
mods = P.Q_PN14 + P.P_PN14
pk = np.stack([np.stack([rnd.integers(0, q, N, dtype=np.uint64) for q in mods]) for _ in range(2)])      # uniform words: timing does not need valid keys
ctx.load_public_key(pk)
ctx.load_secret_key(np.stack([rnd.integers(0, q, N, dtype=np.uint64) for q in P.Q_PN14]))
ctx.seed_encryptor(os.urandom(32))


def timed(fn):
    fn(); ctx.sync()
    t = time.perf_counter(); fn(); ctx.sync(); one = time.perf_counter() - t
    reps = max(3, int(args.min_window / max(one, 1e-6)))
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    ctx.sync()
    return (time.perf_counter() - t) / reps


cts = ctx.fill_uniform_cts(nct, level, 7)
h0 = capi.DevArray(ctx, (nct, nl, N)); ctx.check(L.sfg_memcpy_d2d(ctx.h, h0.p, cts.p, h0.nbytes), "d2d"); ctx.sync()
enc_out = capi.DevArray(ctx, (nct, 2, nl, N))
rows = capi.DevArray(ctx, (nct * nl, N)); ctx.check(L.sfg_memcpy_d2d(ctx.h, rows.p, cts.p, rows.nbytes), "d2d"); ctx.sync()
m_q = (C.c_int * (nct * nl))(*(list(range(nl)) * nct))
re, im = np.empty((nct, ctx.slots)), np.empty((nct, ctx.slots))
pre, pim = re.ctypes.data_as(C.c_void_p), im.ctypes.data_as(C.c_void_p)
vals = rnd.uniform(-1, 1, (nct, ctx.slots))
vp = vals.ctypes.data_as(C.POINTER(C.c_double))
scale = 2.0 ** 68
calls = {
    "decrypt_vectors_ms": lambda: ctx.check(L.sfg_decrypt_vectors(ctx.h, cts.p, nct, level, scale, pre, None), "decrypt_vectors"),
    "pcks_finish_decode_ms": lambda: ctx.check(L.sfg_pcks_finish_decode(ctx.h, cts.p, nct, level, scale, h0.p, pre, None), "pcks_finish_decode"),
    "decrypt_vectors_complex_ms": lambda: ctx.check(L.sfg_decrypt_vectors(ctx.h, cts.p, nct, level, scale, pre, pim), "decrypt_vectors"),
    "intt_rows_same_count_ms": lambda: ctx.check(L.sfg_intt_rows(ctx.h, rows.p, nct * nl, m_q), "intt"),
    "encrypt_vectors_ms": lambda: ctx.check(L.sfg_encrypt_vectors_dev(ctx.h, vp, nct, level, enc_out.p), "encrypt_vectors"),
}
t = {k: [] for k in calls}
for _ in range(3):
    for k, fn in calls.items():
        t[k].append(timed(fn))
rec = {"nct": nct, "level": level, "intt_rows": nct * nl}
rec.update({k: [round(x * 1e3, 3) for x in v] for k, v in t.items()})
med = {k: float(np.median(v)) for k, v in t.items()}
rec["decrypt_over_encrypt_ratio_of_medians"] = round(med["decrypt_vectors_ms"] / med["encrypt_vectors_ms"], 3)
rec["pcks_finish_decode_over_encrypt_ratio_of_medians"] = round(med["pcks_finish_decode_ms"] / med["encrypt_vectors_ms"], 3)
rec["aim_decode_no_more_than_encrypt"] = "met" if max(med["decrypt_vectors_ms"], med["pcks_finish_decode_ms"]) <= med["encrypt_vectors_ms"] else "missed"
print(json.dumps(rec), flush=True)
for a in (cts, h0, enc_out, rows):
    a.free()
ctx.close()
if args.out:
    with open(args.out, "w") as f:
        f.write(json.dumps(rec) + "\n")
