"""ss.compactify / ss.selectk on R-MAT graphs (gb_selectk.hip) next to what a user wrote before them.

Workloads: R-MAT scale 18 / 20 / 22, edge factor 16, FP64 values uniform in [0, 1).
  top-k      ``A.ss.compactify("largest", k)`` and ``A.ss.compactify("largest", k, asindex=True)``
             for k = 8 and 32, next to ``A.ss.sort(">")`` of the one output needed followed by
             ``select("col<=", k - 1)``, on the same build.  The two results are compared first
             (entries, order, values; the recipe's result has A's shape, compactify's k columns).
  selectk    ``A.ss.selectk(how, k)`` for first / largest / random: the bytes the call must move
             (both row pointers, the kept entries' columns and values in and out, and for
             "largest" every value once) over the time, as a fraction of the stream-copy ceiling
             measured here the way bench.py --full measures it.
Between HIP events on the library stream around the whole call (allocation and install of the
result included), after warm-up, the configurations interleaved in one process, the median of RUNS
runs; every run is kept, so that a difference can be judged against the run-to-run spread.
Writes one JSON document (default profiles/selectk_probe.json) and prints a table.

    python tools/selectk_probe.py [--out profiles/selectk_probe.json] [--scales 18,20,22]
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

RUNS, WARMUP, EF = 5, 2, 16
KS = (8, 32)
SEED = 12345
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


def timed(configs, stream):
    """{name: [ms of every run]} of the callables in configs, interleaved"""
    ms = {c: [] for c in configs}
    for _ in range(WARMUP):
        for f in configs.values():
            f()
    torch.cuda.synchronize()
    for _ in range(RUNS):
        for c, f in configs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            f()
            e1.record(stream)
            torch.cuda.synchronize()
            ms[c].append(e0.elapsed_time(e1))
    return ms


def summary(runs):
    return {"ms": statistics.median(runs), "min_ms": min(runs), "max_ms": max(runs), "runs_ms": runs}


def same(a, b):
    x, y = a.to_coo(), b.to_coo()
    return all(np.array_equal(p, q) for p, q in zip(x, y))


def probe(scale, stream, ceiling):
    A = rmat(scale)
    n, nnz = A.nrows, A.nvals
    out = {"scale": scale, "edge_factor": EF, "type": "FP64", "nrows": n, "nvals": nnz, "top_k": {}, "selectk": {}}
    for k in KS:
        recipes = {
            "compactify_values": lambda: A.ss.compactify("largest", k),
            "sort_select_values": lambda: A.ss.sort(">", permutation=False)[0].select("col<=", k - 1).new(),
            "compactify_asindex": lambda: A.ss.compactify("largest", k, asindex=True),
            "sort_select_permutation": lambda: A.ss.sort(">", values=False)[1].select("col<=", k - 1).new(),
        }
        identical = None  # not compared: the host copies of 2^27 entries and their indices, four times
        if n * k <= 1 << 25:
            identical = same(recipes["compactify_values"](), recipes["sort_select_values"]()) and \
                same(recipes["compactify_asindex"](), recipes["sort_select_permutation"]())
            assert identical, f"scale {scale} k {k}: compactify and sort + select differ"
        ms = timed(recipes, stream)
        res = {c: summary(r) for c, r in ms.items()}
        res["identical"] = identical
        res["rows_per_class"] = {c: gb.get_knob(f"stat_selectk_rows_{c}") for c in ("all", "wave", "block", "long")}
        out["top_k"][str(k)] = res
        hows = {how: (lambda how=how: A.ss.selectk(how, k, seed=SEED)) for how in ("first", "largest", "random")}
        kept = hows["first"]().nvals
        ms = timed(hows, stream)
        for how, runs in ms.items():
            by = 2 * 8 * (n + 1) + 2 * kept * (4 + 8) + (8 * nnz if how == "largest" else 0)
            s = summary(runs)
            s.update(bytes=by, kept=kept, GBps=by / (s["ms"] * 1e-3) / 1e9)
            s["fraction_of_stream_copy"] = s["GBps"] / ceiling
            out["selectk"][f"{how}_{k}"] = s
    del A
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "selectk_probe.json"))
    ap.add_argument("--scales", default="18,20,22")
    args = ap.parse_args()
    stream = torch.cuda.Stream()
    gb.set_stream(stream)
    ceiling = stream_copy_ceiling()
    doc = {"device": torch.cuda.get_device_name(0), "runs": RUNS, "warmup": WARMUP, "statistic": "median",
           "timer": "HIP events on the library stream around the whole call, configurations interleaved",
           "stream_copy_GBps": ceiling, "results": []}
    print(f"stream copy {ceiling:.0f} GB/s")
    for scale in [int(s) for s in args.scales.split(",")]:
        r = probe(scale, stream, ceiling)
        doc["results"].append(r)
        for k, res in r["top_k"].items():
            for c, s in res.items():
                if isinstance(s, dict) and "ms" in s:
                    print(f"s{scale} top-{k:<3} {c:<26}{s['ms']:>10.3f} ms  [{s['min_ms']:.3f}, {s['max_ms']:.3f}]", flush=True)
        for c, s in r["selectk"].items():
            print(f"s{scale} selectk {c:<24}{s['ms']:>10.3f} ms  [{s['min_ms']:.3f}, {s['max_ms']:.3f}]"
                  f"{s['GBps']:>8.0f} GB/s {100 * s['fraction_of_stream_copy']:>5.1f} %", flush=True)
        with open(args.out, "w") as f:  # after every scale: a later one may run out of time
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
