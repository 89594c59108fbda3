#!/usr/bin/env python3
"""Times the quality-control scan (sfg_geno_qc_scan) on a resident synthetic matrix, int8 and 2-bit packed, beside sfg_geno_colsums on the same int8 handle -
existing code that reads the same bytes once, the yardstick.  Not part of bench.py.

    python tools/bench_qcscan.py [--rows 32768] [--cols 262144] [--warmup 3] [--repeats 30] [--out profiles/qcscan_bench.jsonl]

Every timed call ends in a device synchronise (its outputs are host arrays), so a host clock around it is the call's time: kernel, the O(nrow + ncol) copies of
filters and counts, and the host's share.  The variants are alternated inside every repeat, so drift of the machine hits them alike.  Prints one JSON line per
variant and one summary line; --out appends them to a file.  The CPU cost this replaces (the Go loops of gwas/qualcontrol.go) cannot be timed without a Go
toolchain and is not estimated here."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=32768)
    ap.add_argument("--cols", type=int, default=262144)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import oracle_lib as ol                               # moduli only
    from sfgwas_amd import capi
    ctx = capi.Context(ol.Q_PN14, ol.P_PN14)
    lib = capi.lib()
    nrow, ncol = a.rows, a.cols
    buf, g8 = ctx.fill_geno(nrow, ncol, 0x5EED)
    g2 = C.c_void_p()
    ctx.check(lib.sfg_geno_pack(ctx.h, g8, C.byref(g2)), "geno_pack")
    rnd = np.random.default_rng(1)
    ctrl = (rnd.random(nrow) < 0.5).astype(np.uint8)
    # every output is allocated once, outside the timed calls, for the scan as for the yardstick
    s1, s2 = np.zeros(ncol), np.zeros(ncol)
    cc, rm, rh = np.zeros((2, 4, ncol), np.uint32), np.zeros(nrow, np.uint32), np.zeros(nrow, np.uint32)
    pd = C.POINTER(C.c_double)
    vp = lambda x: x.ctypes.data_as(C.c_void_p)           # noqa: E731

    def colsums():
        ctx.check(lib.sfg_geno_colsums(ctx.h, g8, s1.ctypes.data_as(pd), s2.ctypes.data_as(pd)), "colsums")

    def scan(g, rows):
        return lambda: ctx.check(lib.sfg_geno_qc_scan(ctx.h, g, None, None, vp(ctrl), vp(cc), vp(rm) if rows else None, vp(rh) if rows else None), "qc_scan")

    def scanned(g):
        scan(g, True)()
        return cc.copy(), rm.copy(), rh.copy()

    packed_bytes = nrow * ((ncol + 15) // 16) * 4
    variants = [
        ("colsums_int8", nrow * ncol, colsums),
        ("scan_both_int8", nrow * ncol, scan(g8, True)),
        ("scan_cols_int8", nrow * ncol, scan(g8, False)),
        ("scan_both_packed", packed_bytes, scan(g2, True)),
        ("scan_cols_packed", packed_bytes, scan(g2, False)),
    ]
    # the timed calls must compute the same thing: int8 and packed scans agree, and the scan's sums are colsums' sums
    both8, both2 = scanned(g8), scanned(g2)
    assert all(np.array_equal(x, y) for x, y in zip(both8, both2)), "int8 and packed scans disagree"
    colsums()
    assert np.array_equal(s1, both8[0][0, 1].astype(np.float64) + 2.0 * both8[0][0, 2]), "scan and colsums disagree"
    for _ in range(a.warmup):
        for _, _, fn in variants:
            fn()
    times = {name: [] for name, _, _ in variants}
    for _ in range(a.repeats):
        for name, _, fn in variants:
            ctx.sync()
            t0 = time.perf_counter()
            fn()
            times[name].append(time.perf_counter() - t0)
    lines = []
    med = {}
    for name, nbytes, _ in variants:
        t = np.sort(np.array(times[name]))
        med[name] = float(np.median(t))
        lines.append({"what": name, "nrow": nrow, "ncol": ncol, "matrix_bytes": nbytes, "warmup": a.warmup, "repeats": a.repeats,
                      "median_ms": round(1e3 * med[name], 4), "min_ms": round(1e3 * float(t[0]), 4), "max_ms": round(1e3 * float(t[-1]), 4),
                      "matrix_GB_per_s_at_median": round(nbytes / med[name] / 1e9, 1)})
    lines.append({"what": "summary", "nrow": nrow, "ncol": ncol,
                  "scan_both_int8_over_colsums": round(med["scan_both_int8"] / med["colsums_int8"], 3),
                  "scan_cols_int8_over_colsums": round(med["scan_cols_int8"] / med["colsums_int8"], 3),
                  "scan_both_packed_over_scan_both_int8": round(med["scan_both_packed"] / med["scan_both_int8"], 3),
                  "aim_full_scan_within_1.5x_of_colsums_met": bool(med["scan_both_int8"] <= 1.5 * med["colsums_int8"]),
                  "aim_packed_faster_than_int8_met": bool(med["scan_both_packed"] < med["scan_both_int8"])})
    for ln in lines:
        print(json.dumps(ln))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")
    ctx.geno_free(g2)
    ctx.geno_free(g8)
    buf.free()
    ctx.close()


if __name__ == "__main__":
    main()
