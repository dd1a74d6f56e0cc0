"""GxB_Matrix_sort on R-MAT graphs (gb_sort.hip): the length-classed sort (sort_method 0) next to
the segmented radix sort of every row (sort_method 1), and next to sort_method 0 with the
workgroup class switched off (sort_block_max = sort_wave_max: those rows go to hipCUB too).

Workloads: R-MAT scale 18 / 20 / 22, edge factor 16, values INT32, INT64 (integers in [1, 255],
so a row has many ties) and FP64 (uniform in [0, 1)), GrB_LT of the value type; values only,
permutation only, both.  Between HIP events on the library stream, after warm-up, the
configurations interleaved in one process, the median of RUNS runs.  The yardstick is the bytes
the call must move -- the read of rowptr, colidx and the values, the write of rowptr, colidx and
values of every requested output -- over the time, as a fraction of the stream-copy ceiling
measured here the way bench.py --full measures it.  The timed call includes the allocation of
the results and their install into C and P.
Writes one JSON document (default profiles/sort_probe.json) and prints a table.

    python tools/sort_probe.py [--out profiles/sort_probe.json] [--scales 18,20,22] [--types INT32,INT64,FP64]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "graph-python_amd"))
import graphblas_amd as gb  # noqa: E402

RUNS, WARMUP, EF = 5, 2, 16
lib = gb.lib
TYPES = [("INT32", 1, 4), ("INT64", 1, 8), ("FP64", 2, 8)]  # name, GxB_Matrix_rmat values code, bytes
OUTPUTS = [("both", True, True), ("values", True, False), ("permutation", False, True)]
CONFIGS = {"classes": {}, "block_max_512": {"sort_block_max": 512}, "no_block_class": {"sort_block_max": 64},
           "hipcub_all": {"sort_method": 1}}
KNOBS = ["sort_method", "sort_block_max"]


def nvals_of(h):
    nv = ctypes.c_uint64()
    assert lib.GrB_Matrix_nvals(ctypes.byref(nv), h) == 0
    return nv.value


def stream_copy_ceiling():
    xs = torch.empty(1 << 31, dtype=torch.uint8, device="cuda")
    ys = torch.empty_like(xs)
    ys.copy_(xs)
    torch.cuda.synchronize()
    c0 = time.perf_counter()
    for _ in range(5):
        ys.copy_(xs)
    torch.cuda.synchronize()
    return 5 * 2 * xs.numel() / (time.perf_counter() - c0) / 1e9


def new_matrix(tname, n):
    M = ctypes.c_void_p()
    assert lib.GrB_Matrix_new(ctypes.byref(M), getattr(lib, f"GrB_{tname}"), n, n) == 0
    return M


def probe(scale, tname, vcode, vsize, stream, ceiling):
    n = 1 << scale
    A = ctypes.c_void_p()
    assert lib.GxB_Matrix_rmat(ctypes.byref(A), scale, EF, 42, vcode, 2, 0, 0) == 0
    if tname == "INT32":  # the generator's INT64 values, cast
        B = new_matrix("INT32", n)
        assert lib.GrB_Matrix_apply(B, None, None, lib.GrB_IDENTITY_INT32, A, None) == 0
        lib.GrB_Matrix_free(ctypes.byref(A))
        A = B
    nnz = nvals_of(A)
    C, P = new_matrix(tname, n), new_matrix("UINT64", n)
    op = getattr(lib, f"GrB_LT_{tname}")
    out = {}
    for oname, wc, wp in OUTPUTS:
        configs = list(CONFIGS) if oname == "both" else ["classes", "hipcub_all"]

        def run(cfg):
            for k in KNOBS:
                gb.set_knob(k, CONFIGS[cfg].get(k, 0))
            assert lib.GxB_Matrix_sort(C if wc else None, P if wp else None, op, A, None) == 0

        ms = {c: [] for c in configs}
        try:
            for _ in range(WARMUP):
                for c in configs:
                    run(c)
            torch.cuda.synchronize()
            for _ in range(RUNS):
                for c in configs:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    run(c)
                    e1.record(stream)
                    torch.cuda.synchronize()
                    ms[c].append(e0.elapsed_time(e1))
            run("classes")
            stats = {k: gb.get_knob(f"stat_sort_rows_{k}") for k in ("wave", "block", "long")}
        finally:
            for k in KNOBS:
                gb.set_knob(k, 0)
        structure = 8 * (n + 1) + 4 * nnz
        by = structure + vsize * nnz + (structure + vsize * nnz if wc else 0) + (structure + 8 * nnz if wp else 0)
        res = {"bytes": by, "rows_per_class": stats}
        for c in configs:
            t = statistics.median(ms[c]) * 1e-3
            res[c] = {"ms": t * 1e3, "runs_ms": ms[c], "GBps": by / t / 1e9, "fraction_of_stream_copy": by / t / 1e9 / ceiling}
        out[oname] = res
    for h in (C, P, A):
        lib.GrB_Matrix_free(ctypes.byref(h))
    torch.cuda.empty_cache()
    return {"scale": scale, "edge_factor": EF, "type": tname, "nrows": n, "nvals": nnz, "outputs": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sort_probe.json"))
    ap.add_argument("--scales", default="18,20,22")
    ap.add_argument("--types", default=",".join(t[0] for t in TYPES))
    args = ap.parse_args()
    stream = torch.cuda.Stream()
    gb.set_stream(stream)
    ceiling = stream_copy_ceiling()
    doc = {"device": torch.cuda.get_device_name(0), "runs": RUNS, "warmup": WARMUP, "statistic": "median",
           "timer": "HIP events on the library stream, configurations interleaved",
           "configurations": CONFIGS, "stream_copy_GBps": ceiling, "results": []}
    print(f"stream copy {ceiling:.0f} GB/s")
    print(f"{'workload':<16}{'outputs':<13}" + "".join(f"{c + ' ms':>18}{'GB/s':>8}" for c in CONFIGS), flush=True)
    for scale in [int(s) for s in args.scales.split(",")]:
        for tname, vcode, vsize in [t for t in TYPES if t[0] in args.types.split(",")]:
            r = probe(scale, tname, vcode, vsize, stream, ceiling)
            doc["results"].append(r)
            for oname, res in r["outputs"].items():
                cells = "".join(f"{res[c]['ms']:>18.3f}{res[c]['GBps']:>8.0f}" if c in res else f"{'-':>18}{'-':>8}"
                                for c in CONFIGS)
                print(f"{'s%d %s' % (scale, tname):<16}{oname:<13}{cells}", flush=True)
            with open(args.out, "w") as f:  # after every workload: a later one may run out of time
                json.dump(doc, f, indent=1)
                f.write("\n")


if __name__ == "__main__":
    main()
