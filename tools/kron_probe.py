"""GrB_kronecker on R-MAT seeds (gb_kron.hip): the entry-parallel kernel (kron_method 0) next to
the one-thread-per-output-row fallback (kron_method 1).

Three workloads, each the Kronecker square K = A (x) A of an R-MAT adjacency (edge factor 16):
  iso_bool_s11   BOOL iso, scale 11, land: about 1 G entries, iso result (4 B per entry)
  iso_bool_s10   BOOL iso, scale 10, land: about a quarter of that
  fp64_s10       FP64 values, scale 10, times: 12 B per entry, about the bytes of the first
Between HIP events on the library stream, after warm-up, the two methods interleaved, the median
of RUNS runs.  The yardstick is the bytes the call must write,
  nvals(T) (4 + value size) + 8 (m p + 1),
over the time, as a fraction of the stream-copy ceiling measured here the way bench.py --full
measures it (device-to-device copy of 2 GiB, read + write bytes).  The timed call includes the
row-pointer kernel, the allocation of T and the install into C (no mask, no accum).
Writes one JSON document (default profiles/kron_probe.json) and prints it.

    python tools/kron_probe.py [--out profiles/kron_probe.json]
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
from graphblas_amd.device import matrix_view  # noqa: E402

RUNS, WARMUP, EF = 7, 2, 16
lib = gb.lib
WORKLOADS = [("iso_bool_s11", 11, 0, "GrB_BOOL", "GrB_LAND", 0), ("iso_bool_s10", 10, 0, "GrB_BOOL", "GrB_LAND", 0),
             ("fp64_s10", 10, 2, "GrB_FP64", "GrB_TIMES_FP64", 8)]


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


def probe(name, scale, values, ctype, opname, vsize, stream, ceiling):
    n = 1 << scale
    A = ctypes.c_void_p()
    assert lib.GxB_Matrix_rmat(ctypes.byref(A), scale, EF, 42, values, 2, 0, 0) == 0
    nnz = nvals_of(A)
    C = ctypes.c_void_p()
    assert lib.GrB_Matrix_new(ctypes.byref(C), getattr(lib, ctype), n * n, n * n) == 0
    op = getattr(lib, opname)

    def run(method):
        gb.set_knob("kron_method", method)
        assert lib.GrB_Matrix_kronecker_BinaryOp(C, None, None, op, A, A, None) == 0

    ms = {0: [], 1: []}
    try:
        for _ in range(WARMUP):
            run(0)
            run(1)
        torch.cuda.synchronize()
        for _ in range(RUNS):
            for method in (0, 1):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                run(method)
                e1.record(stream)
                torch.cuda.synchronize()
                ms[method].append(e0.elapsed_time(e1))
    finally:
        gb.set_knob("kron_method", 0)
    nvt = nvals_of(C)
    assert nvt == nnz * nnz
    view = matrix_view(C)
    assert bool(view.iso) == (vsize == 0)
    t0, t1 = statistics.median(ms[0]) * 1e-3, statistics.median(ms[1]) * 1e-3
    by = nvt * (4 + vsize) + 8 * (n * n + 1)
    res = {"scale": scale, "edge_factor": EF, "type": ctype, "op": opname, "nvals_A": nnz, "nvals_T": nvt,
           "rows_T": n * n, "iso_result": vsize == 0, "bytes_written": by,
           "entry_parallel_s": t0, "per_row_s": t1, "entry_parallel_runs_ms": ms[0], "per_row_runs_ms": ms[1],
           "entry_parallel_GBps": by / t0 / 1e9, "per_row_GBps": by / t1 / 1e9,
           "fraction_of_stream_copy": by / t0 / 1e9 / ceiling, "speedup_vs_per_row": t1 / t0}
    lib.GrB_Matrix_free(ctypes.byref(C))
    lib.GrB_Matrix_free(ctypes.byref(A))
    torch.cuda.empty_cache()
    return name, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kron_probe.json"))
    args = ap.parse_args()
    stream = torch.cuda.Stream()
    gb.set_stream(stream)
    ceiling = stream_copy_ceiling()
    doc = {"device": torch.cuda.get_device_name(0), "runs": RUNS, "warmup": WARMUP, "statistic": "median",
           "timer": "HIP events on the library stream, methods interleaved",
           "stream_copy_GBps": ceiling, "results": {}}
    for w in WORKLOADS:
        name, res = probe(*w, stream, ceiling)
        doc["results"][name] = res
        print(name, json.dumps(res), flush=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
