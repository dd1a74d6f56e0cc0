"""Sparse import and export from device arrays (gb_sparse_io.hip) next to the host-array path of the
same build and to the stream-copy ceiling.

Workload: the edge list of R-MAT scale 18 / 20 / 22, edge factor 16, FP64 values, already on the
device as int64 row and column tensors and a float64 value tensor (what `A.to_coo(device=True)`
gives: sorted, no duplicates), the same list shuffled by one device permutation, and its CSR arrays.
  coo_sorted    Matrix.from_coo of the sorted list: the keys are found strictly increasing (path 0)
  coo_shuffled  Matrix.from_coo of the shuffled list: sort and fold (path 1)
  csr           Matrix.from_csr of int64 pointer and indices: checked, narrowed, installed (path 0)
  to_coo, to_csr   the exports, int64 indices
Each through the device path (the tensors go in and come out as they are) and through the
host-array path, which is what a caller with device tensors had before: the tensors are copied to
the host (`.cpu().numpy()`, inside the timed region), the numpy arrays go through the typed entry
points, and for the exports the numpy results are copied back to the device.  The bytes a call must
move -- its arrays once, and the object's storage (8 B pointer per row, 4 B index and 8 B value
per entry) once -- over the device path's time, as a fraction of the stream-copy ceiling measured
here the way bench.py --full measures it.  Between HIP events on the library stream around the
whole call for the device path; the host path spends its time on the host, so both are compared by
wall clock, after warm-up, the median of the runs; every run is kept.  The host path takes seconds
at the larger scales and runs fewer times (HOST_RUNS).
Writes one JSON document (default profiles/sparse_io_probe.json) and prints a table.

    python tools/sparse_io_probe.py [--out profiles/sparse_io_probe.json] [--scales 18,20,22] [--no-host]
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
HOST_RUNS = {18: (1, 3), 20: (1, 3), 22: (0, 1)}  # scale: (warm-up, runs)
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


def summary(ms, wall):
    return {"ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "runs_ms": ms,
            "wall_ms": statistics.median(wall), "wall_runs_ms": wall}


def to_host(*tensors):
    return [t.cpu().numpy() for t in tensors]


def to_device(*arrays):
    return [torch.from_numpy(a).cuda() for a in arrays]


def probe(scale, stream, ceiling, with_host, save):
    A = rmat(scale)
    n, nnz = A.nrows, A.nvals
    r, c, v = A.to_coo(device=True)
    ptr, idx, _ = A.to_csr(device=True)
    A.wait()
    perm = torch.randperm(nnz, device="cuda", generator=torch.Generator("cuda").manual_seed(7))
    sr, sc, sv = r[perm].contiguous(), c[perm].contiguous(), v[perm].contiguous()
    del perm
    torch.cuda.synchronize()
    storage = 8 * (n + 1) + 12 * nnz
    coo_bytes, csr_bytes = 24 * nnz + storage, 8 * (n + 1) + 16 * nnz + storage
    kw = dict(nrows=n, ncols=n)
    cases = {
        "coo_sorted": (coo_bytes, lambda: gb.Matrix.from_coo(r, c, v, **kw),
                       lambda: gb.Matrix.from_coo(*to_host(r, c, v), **kw), 0),
        "coo_shuffled": (coo_bytes, lambda: gb.Matrix.from_coo(sr, sc, sv, **kw),
                         lambda: gb.Matrix.from_coo(*to_host(sr, sc, sv), **kw), 1),
        "csr": (csr_bytes, lambda: gb.Matrix.from_csr(ptr, idx, v, ncols=n),
                lambda: gb.Matrix.from_csr(*to_host(ptr, idx, v), ncols=n), 0),
        "to_coo": (coo_bytes, lambda: A.to_coo(device=True), lambda: to_device(*A.to_coo()), None),
        "to_csr": (csr_bytes, lambda: A.to_csr(device=True), lambda: to_device(*A.to_csr()), None),
    }
    out = {"scale": scale, "edge_factor": EF, "type": "FP64", "index": "int64", "nrows": n, "nvals": nnz}
    for name, (by, device_call, host_call, path) in cases.items():
        ms, wall = timed(device_call, stream, WARMUP, RUNS)
        s = summary(ms, wall)
        s.update(bytes=by, GBps=by / (s["ms"] * 1e-3) / 1e9)
        s["fraction_of_stream_copy"] = s["GBps"] / ceiling
        if path is not None:
            s["import_path"] = gb.get_knob("stat_sparse_import_path")
            assert s["import_path"] == path, (name, s["import_path"])
        out[name] = {"device": s}
        save(out)
        if with_host:
            warm, runs = HOST_RUNS.get(scale, (0, 1))
            hms, hwall = timed(host_call, stream, warm, runs)
            h = summary(hms, hwall)
            h.update(warmup=warm, runs=runs)
            out[name]["host"] = h
            out[name]["host_over_device_wall"] = h["wall_ms"] / s["wall_ms"]
            save(out)
    out["shuffled_over_sorted"] = out["coo_shuffled"]["device"]["ms"] / out["coo_sorted"]["device"]["ms"]
    save(out)
    del A, r, c, v, sr, sc, sv, ptr, idx
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sparse_io_probe.json"))
    ap.add_argument("--scales", default="18,20,22")
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()
    stream = torch.cuda.Stream()
    gb.set_stream(stream)
    ceiling = stream_copy_ceiling()
    doc = {"device": torch.cuda.get_device_name(0), "runs": RUNS, "warmup": WARMUP, "statistic": "median",
           "timer": "HIP events on the library stream around the whole call; wall clock for the comparison with "
                    "the host-array path",
           "bytes": "the call's arrays once and the object's storage once",
           "stream_copy_GBps": ceiling, "results": []}
    print(f"stream copy {ceiling:.0f} GB/s")

    def save(partial):  # after every measurement: a later one may run out of time
        with open(args.out, "w") as f:
            json.dump(dict(doc, results=doc["results"] + [partial]), f, indent=1)
            f.write("\n")

    for scale in [int(s) for s in args.scales.split(",")]:
        res = probe(scale, stream, ceiling, not args.no_host, save)
        doc["results"].append(res)
        for name in ("coo_sorted", "coo_shuffled", "csr", "to_coo", "to_csr"):
            s = res[name]["device"]
            line = (f"s{scale} {name:<13}{s['ms']:>10.3f} ms  [{s['min_ms']:.3f}, {s['max_ms']:.3f}] wall {s['wall_ms']:.3f}"
                    f"{s['GBps']:>8.0f} GB/s {100 * s['fraction_of_stream_copy']:>5.1f} %")
            if "host" in res[name]:
                h = res[name]["host"]
                line += f"   host path wall {h['wall_ms']:.1f} ms = {res[name]['host_over_device_wall']:.1f} x"
            print(line, flush=True)
        print(f"s{scale} shuffled / sorted import: {res['shuffled_over_sorted']:.2f} x", flush=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
