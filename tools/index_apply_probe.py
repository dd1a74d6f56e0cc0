"""GrB_apply with an index-unary operator on R-MAT (gb_apply_index.hip) next to GrB_Matrix_apply with
GrB_IDENTITY_INT64 on the same matrix: the unary apply makes the same copies of rowptr and colidx
and writes a value array of the same size, so the difference is what the values cost -- identity
reads 8 B per entry, ROWINDEX searches rowptr per 256-entry chunk, COLINDEX re-reads colidx.

Per scale (default 20 and 22, edge factor 16, INT64 values in [1, 255], the structure of the
benchmark's adjacency), between HIP events on the library stream, after warm-up, the three calls
alternate for 20 rounds; the median and the minimum of each are reported.  Algorithmic bytes of a
call (n rows, nnz entries): the structure copy 16 (n + 1) + 8 nnz, and
  identity   8 nnz read + 8 nnz written
  rowindex   8 (n + 1) read (rowptr, once) + 8 nnz written
  colindex   4 nnz read + 8 nnz written
Writes one JSON document (default profiles/index_apply_probe.json) and prints it.

    python tools/index_apply_probe.py [--scales 20 22] [--out profiles/index_apply_probe.json]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "graph-python_amd"))
import graphblas_amd as gb  # noqa: E402

RUNS, WARMUP, EF = 20, 3, 16
lib = gb.lib


def probe_scale(scale, stream):
    n = 1 << scale
    A, C = ctypes.c_void_p(), ctypes.c_void_p()
    assert lib.GxB_Matrix_rmat(ctypes.byref(A), scale, EF, 42, 1, 2, 0, 0) == 0
    nv = ctypes.c_uint64()
    assert lib.GrB_Matrix_nvals(ctypes.byref(nv), A) == 0
    nnz = nv.value
    assert lib.GrB_Matrix_new(ctypes.byref(C), lib.GrB_INT64, n, n) == 0
    calls = {
        "identity": lambda: lib.GrB_Matrix_apply(C, None, None, lib.GrB_IDENTITY_INT64, A, None),
        "rowindex": lambda: lib.GrB_Matrix_apply_IndexOp_INT64(C, None, None, lib.GrB_ROWINDEX_INT64, A, 0, None),
        "colindex": lambda: lib.GrB_Matrix_apply_IndexOp_INT64(C, None, None, lib.GrB_COLINDEX_INT64, A, 0, None),
    }
    structure = 16 * (n + 1) + 8 * nnz
    nbytes = {"identity": structure + 16 * nnz, "rowindex": structure + 8 * (n + 1) + 8 * nnz,
              "colindex": structure + 12 * nnz}
    for _ in range(WARMUP):
        for fn in calls.values():
            assert fn() == 0
    torch.cuda.synchronize()
    ms = {k: [] for k in calls}
    for _ in range(RUNS):
        for k, fn in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            assert fn() == 0
            e1.record(stream)
            torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    res = {"scale": scale, "edge_factor": EF, "nrows": n, "nnz": nnz}
    for k in calls:
        med = statistics.median(ms[k]) * 1e-3
        res[k] = {"median_s": med, "min_s": min(ms[k]) * 1e-3, "bytes": nbytes[k], "GBps": nbytes[k] / med / 1e9}
    for k in ("rowindex", "colindex"):
        res[k]["ratio_to_identity"] = res[k]["median_s"] / res["identity"]["median_s"]
    lib.GrB_Matrix_free(ctypes.byref(C))
    lib.GrB_Matrix_free(ctypes.byref(A))
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scales", type=int, nargs="+", default=[20, 22])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "index_apply_probe.json"))
    args = ap.parse_args()
    stream = torch.cuda.Stream()
    gb.set_stream(stream)
    doc = {"device": torch.cuda.get_device_name(0), "runs": RUNS, "warmup": WARMUP,
           "statistic": "median and minimum of alternating rounds", "timer": "HIP events on the library stream",
           "results": [probe_scale(s, stream) for s in args.scales]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
