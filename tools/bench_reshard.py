#!/usr/bin/env python3
"""Times the re-sharding filter (sfg_mgpu_geno_filter) on a resident synthetic matrix, int8 and 2-bit packed, at world 1 beside sfg_geno_filter on the SAME
resident matrix and filters (the single-GPU filter is the yardstick: the same gather, with byte stores), and beside sfg_geno_colsums, which reads the matrix once.
World 8 with every rank on one device is recorded too; it carries no aim - ranks that share a device say nothing about the links between devices, and no
cross-device rate is measured here.  Not part of bench.py.

    python tools/bench_reshard.py [--rows 32768] [--cols 262144] [--warmup 3] [--repeats 30] [--out profiles/reshard_bench.jsonl]

Every timed call ends with the device drained (the filters return a finished matrix), so a host clock around it is the call's time: building and uploading the
index tables, allocating the result, the kernel.  Freeing the result is outside the timed window for every variant.  The variants are alternated inside every
repeat, so drift of the machine hits them alike.  Before anything is timed the two filters' results are compared: every count of a full quality-control scan, and
three slabs of rows byte for byte.  Prints one JSON line per variant and a summary line; --out appends them to a file.

Every filter call allocates its result (6.5 GB for the int8 matrix) with the runtime's allocator and the result is freed again after the clock stops.  Runs of
this tool show one or two calls in a variant's 30 at 4 to 5 s where the median is milliseconds: only in the variants that produce the 6.5 GB int8 result, in
sfg_geno_filter as in the re-sharding filter, at another repeat in every run.  To narrow that down the variant "alloc_only_int8" times nothing but an allocation of
the int8 result's size (never written, freed outside the window like the results), and every line records where its slowest call fell ("max_at_repeat") and how
many calls took more than ten times the median ("calls_over_10x_median").  The bare allocation has not stalled (0.3 ms every time), so the stall is where such a
buffer is first written, not in the allocation call and not in one filter's kernel; its cause in the runtime or driver is not established.  The aim is judged
by the medians, which one or two calls in 30 do not move."""
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
    ap.add_argument("--world", type=int, default=8, help="the second world size, every rank on device 0 (0: skip)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import oracle_lib as ol                               # moduli only
    from sfgwas_amd import capi
    lib = capi.lib()
    nrow, ncol = a.rows, a.cols
    rnd = np.random.default_rng(1)
    rf, cf = (rnd.random(nrow) < 0.95).astype(np.uint8), (rnd.random(ncol) < 0.80).astype(np.uint8)
    nr, nc = int(rf.sum()), int(cf.sum())
    out_bytes = {False: nr * nc, True: nr * ((nc + 15) // 16) * 4}
    vp = lambda x: x.ctypes.data_as(C.c_void_p)           # noqa: E731
    lines, med = [], {}

    def run(variants):
        """variants: (name, bytes moved, call -> a result to free, free); alternated"""
        for _ in range(a.warmup):
            for _, _, fn, free in variants:
                free(fn())
        times = {v[0]: [] for v in variants}
        for _ in range(a.repeats):
            for name, _, fn, free in variants:
                t0 = time.perf_counter()
                r = fn()
                times[name].append(time.perf_counter() - t0)
                free(r)
        for name, nbytes, _, _ in variants:
            t = np.sort(np.array(times[name]))
            med[name] = float(np.median(t))
            lines.append({"what": name, "nrow": nrow, "ncol": ncol, "kept_rows": nr, "kept_cols": nc, "bytes_moved": nbytes, "warmup": a.warmup, "repeats": a.repeats,
                          "median_ms": round(1e3 * med[name], 4), "min_ms": round(1e3 * float(t[0]), 4), "max_ms": round(1e3 * float(t[-1]), 4),
                          "max_at_repeat": int(np.argmax(times[name])), "calls_over_10x_median": int((t > 10 * med[name]).sum()),
                          "GB_per_s_at_median": round(nbytes / med[name] / 1e9, 1)})

    def mfilter(mg, m):
        def call():
            out = C.c_void_p()
            mg.check(lib.sfg_mgpu_geno_filter(mg.h, m, vp(rf), vp(cf), C.byref(out)), "sfg_mgpu_geno_filter")
            return out
        return call

    # ---- world 1: the re-sharding filter, the single-GPU filter on the same resident matrix, and colsums
    mg = capi.MultiGpu(ol.Q_PN14, ol.P_PN14, devices=[0])
    ctx = mg.ctx[0]
    m8, m2 = mg.geno_synthetic(nrow, ncol, 0x5EED), mg.geno_synthetic(nrow, ncol, 0x5EED, packed=True)
    g8, g2 = mg.geno_shard(m8, 0), mg.geno_shard(m2, 0)

    def gfilter(g):
        def call():
            out = C.c_void_p()
            ctx.check(lib.sfg_geno_filter(ctx.h, g, vp(rf), vp(cf), C.byref(out)), "sfg_geno_filter")
            return out
        return call

    s1, s2 = np.zeros(ncol), np.zeros(ncol)
    pd = C.POINTER(C.c_double)

    def colsums():
        ctx.check(lib.sfg_geno_colsums(ctx.h, g8, s1.ctypes.data_as(pd), s2.ctypes.data_as(pd)), "colsums")

    # the timed calls must compute the same thing
    for m, g, packed in ((m8, g8, False), (m2, g2, True)):
        new, old = mfilter(mg, m)(), gfilter(g)()
        sh = mg.geno_shard(new, 0)
        assert mg.geno_dims(new) == (nr, nc)
        for x, y in zip(ctx.geno_qc_scan(sh), ctx.geno_qc_scan(old)):
            assert np.array_equal(x, y), "the two filters' results scan differently"
        (dn, ldn, _), (do, ldo, _) = capi.geno_layout(sh), capi.geno_layout(old)
        width = out_bytes[packed] // nr
        for r0 in (0, nr // 2, nr - min(nr, 256)):
            k = min(nr - r0, 256)
            x = ctx.to_host(C.c_void_p(dn + r0 * ldn), (k, ldn), np.uint8)[:, :width]
            y = ctx.to_host(C.c_void_p(do + r0 * ldo), (k, ldo), np.uint8)[:, :width]
            assert np.array_equal(x, y), "the two filters' results differ"
        mg.geno_free(new)
        ctx.geno_free(old)
    run([
        ("reshard_int8_world1", 2 * out_bytes[False], mfilter(mg, m8), mg.geno_free),
        ("geno_filter_int8", 2 * out_bytes[False], gfilter(g8), ctx.geno_free),
        ("reshard_packed_world1", 2 * out_bytes[True], mfilter(mg, m2), mg.geno_free),
        ("geno_filter_packed", 2 * out_bytes[True], gfilter(g2), ctx.geno_free),
        ("colsums_int8", nrow * ncol, colsums, lambda _: None),
        ("alloc_only_int8", out_bytes[False], lambda: ctx.malloc(nr * ((nc + 15) // 16 * 16)), ctx.free),
    ])
    mg.geno_free(m8)
    mg.geno_free(m2)
    mg.close()
    # ---- world 8 on one device: recorded, no aim
    if a.world > 1:
        mg = capi.MultiGpu(ol.Q_PN14, ol.P_PN14, devices=[0] * a.world)
        m8, m2 = mg.geno_synthetic(nrow, ncol, 0x5EED), mg.geno_synthetic(nrow, ncol, 0x5EED, packed=True)
        run([(f"reshard_int8_world{a.world}_one_device", 2 * out_bytes[False], mfilter(mg, m8), mg.geno_free),
             (f"reshard_packed_world{a.world}_one_device", 2 * out_bytes[True], mfilter(mg, m2), mg.geno_free)])
        mg.geno_free(m8)
        mg.geno_free(m2)
        mg.close()
    r8, r2 = med["reshard_int8_world1"] / med["geno_filter_int8"], med["reshard_packed_world1"] / med["geno_filter_packed"]
    lines.append({"what": "summary", "nrow": nrow, "ncol": ncol, "kept_rows": nr, "kept_cols": nc,
                  "reshard_int8_world1_over_geno_filter_int8": round(r8, 3), "reshard_packed_world1_over_geno_filter_packed": round(r2, 3),
                  "aim_world1_within_1.10x_of_geno_filter_met": bool(r8 <= 1.10 and r2 <= 1.10),
                  "bytes_moved": "kept entries read once and written once (2 x the result's bytes); colsums: the matrix read once",
                  "cross_device_rates": "not measured"})
    for ln in lines:
        print(json.dumps(ln))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
