"""ss.scan on R-MAT graphs (gb_scan.hip) next to the recipe it replaced and to the stream-copy ceiling.

Workload: R-MAT scale 18 / 20 / 22, edge factor 16, FP64 values uniform in [0, 1), monoid PLUS,
every row scanned.
  scan       ``A.ss.scan(gb.monoid.plus)``: one GxB_Matrix_scan.  The bytes the call must move --
             the values in and out (2 x 8 B per entry), the row pointer in (8 B per row), and the
             structure copied to the result (column indices and row pointer, read and written:
             2 x (4 B per entry + 8 B per row)) -- over the time, as a fraction of the stream-copy
             ceiling measured here the way bench.py --full measures it.
  recipe     ``ss.prefix_scan(A, gb.monoid.plus)`` on the same build: to_coo, the compaction on the
             host, from_coo, about 2 log2(longest row) masked mxm calls, to_coo and from_coo again.
Between HIP events on the library stream around the whole call (allocation and install of the
result included; for the recipe that spans its host work too, so the wall clock is recorded as
well), after warm-up, the median of the runs; every run is kept, so that a difference can be judged
against the run-to-run spread.  The recipe takes seconds at the larger scales and runs fewer times
(RECIPE_RUNS).  At the scales where the host copy is small the two results are compared bit for bit.
Writes one JSON document (default profiles/scan_probe.json) and prints a table.

    python tools/scan_probe.py [--out profiles/scan_probe.json] [--scales 18,20,22] [--no-recipe]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "graph-python_amd"))
import graphblas_amd as gb  # noqa: E402
from graphblas_amd.ss import prefix_scan  # noqa: E402

RUNS, WARMUP, EF = 5, 2, 16
RECIPE_RUNS = {18: (1, 5), 20: (1, 3), 22: (0, 1)}  # scale: (warm-up, runs)
lib = gb.lib


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


def rmat(scale):
    h = ctypes.c_void_p()
    assert lib.GxB_Matrix_rmat(ctypes.byref(h), scale, EF, 42, 2, 2, 0, 0) == 0
    A = gb.Matrix.__new__(gb.Matrix)
    A._h, A.dtype, A.name = h, gb.FP64, "rmat"
    A._nrows = A._ncols = 1 << scale
    return A


def timed(f, stream, warmup, runs):
    """([ms between HIP events of every run], [wall-clock ms of every run])"""
    for _ in range(warmup):
        f()
    torch.cuda.synchronize()
    ms, wall = [], []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record(stream)
        f()
        e1.record(stream)
        torch.cuda.synchronize()
        wall.append(1e3 * (time.perf_counter() - t0))
        ms.append(e0.elapsed_time(e1))
    return ms, wall


def summary(runs):
    return {"ms": statistics.median(runs), "min_ms": min(runs), "max_ms": max(runs), "runs_ms": runs}


def same(a, b):
    x, y = a.to_coo(), b.to_coo()
    return all(np.array_equal(p, q) for p, q in zip(x[:-1], y[:-1])) and \
        np.array_equal(x[-1].view(np.uint64), y[-1].view(np.uint64))


def probe(scale, stream, ceiling, recipe, save):
    A = rmat(scale)
    n, nnz = A.nrows, A.nvals
    out = {"scale": scale, "edge_factor": EF, "type": "FP64", "monoid": "plus", "nrows": n, "nvals": nnz}
    ms, wall = timed(lambda: A.ss.scan(gb.monoid.plus), stream, WARMUP, RUNS)
    by = 2 * 8 * nnz + 8 * (n + 1) + 2 * (4 * nnz + 8 * (n + 1))
    s = summary(ms)
    s.update(wall_ms=statistics.median(wall), bytes=by, GBps=by / (s["ms"] * 1e-3) / 1e9)
    s["fraction_of_stream_copy"] = s["GBps"] / ceiling
    s["rows_per_class"] = {c: gb.get_knob(f"stat_scan_rows_{c}") for c in ("wave", "block", "long")}
    out["scan"] = s
    save(out)
    if recipe:
        warm, runs = RECIPE_RUNS.get(scale, (0, 1))
        identical = None  # not compared: the host copies of 2^26 entries and their indices, twice
        if nnz <= 1 << 23:
            identical = same(A.ss.scan(gb.monoid.plus), prefix_scan(A, gb.monoid.plus))
            assert identical, f"scale {scale}: ss.scan and ss.prefix_scan differ"
        ms, wall = timed(lambda: prefix_scan(A, gb.monoid.plus), stream, warm, runs)
        r = summary(ms)
        r.update(wall_ms=statistics.median(wall), warmup=warm, runs=runs, identical=identical)
        r["times_the_scan"] = r["ms"] / s["ms"]
        out["recipe"] = r
        save(out)
    del A
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scan_probe.json"))
    ap.add_argument("--scales", default="18,20,22")
    ap.add_argument("--no-recipe", action="store_true")
    args = ap.parse_args()
    stream = torch.cuda.Stream()
    gb.set_stream(stream)
    ceiling = stream_copy_ceiling()
    doc = {"device": torch.cuda.get_device_name(0), "runs": RUNS, "warmup": WARMUP, "statistic": "median",
           "timer": "HIP events on the library stream around the whole call",
           "bytes": "values in and out, row pointer in, structure (column indices, row pointer) read and written",
           "stream_copy_GBps": ceiling, "results": []}
    print(f"stream copy {ceiling:.0f} GB/s")

    def save(partial):  # after every measurement: a later one may run out of time
        with open(args.out, "w") as f:
            json.dump(dict(doc, results=doc["results"] + [partial]), f, indent=1)
            f.write("\n")

    for scale in [int(s) for s in args.scales.split(",")]:
        r = probe(scale, stream, ceiling, not args.no_recipe, save)
        doc["results"].append(r)
        s = r["scan"]
        print(f"s{scale} scan    {s['ms']:>12.3f} ms  [{s['min_ms']:.3f}, {s['max_ms']:.3f}]{s['GBps']:>8.0f} GB/s "
              f"{100 * s['fraction_of_stream_copy']:>5.1f} %  rows {s['rows_per_class']}", flush=True)
        if "recipe" in r:
            q = r["recipe"]
            print(f"s{scale} recipe  {q['ms']:>12.3f} ms  [{q['min_ms']:.3f}, {q['max_ms']:.3f}]  "
                  f"{q['times_the_scan']:.0f} x the scan  identical {q['identical']}", flush=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
