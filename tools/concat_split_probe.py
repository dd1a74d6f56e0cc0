"""GxB_Matrix_split / GxB_Matrix_concat on R-MAT graphs (gb_tile.hip) next to the calls they replace.

Per scale (default 10, 20 and 22, edge factor 16, INT64 values): A is the graph, cut 4 x 4 into
equal tiles.  Between HIP events on the library stream, after the warm-ups, the median of the runs of
  (a) A.ss.split(4 x 4)                                   one call
  (b) the 16 GrB_Matrix_extract calls it replaces          T_ij = A[rows_i, cols_j] into new matrices
  (c) ss.concat(tiles)                                     one call, into a new matrix
and, for the 4 x 1 row-panel case,
  (d) ss.concat of the four row panels
  (e) dist.concat_row_panels on device views of the same panels (torch.cat, same device)
each group timed in turn within every run, so its members see the same machine state.  Before
timing, (a) and (b) must give identical tiles, (c) the matrix A, (d) and (e) the same CSR.
(b) passes the explicit index arrays the front end passes for a slice, built once outside the
timed window: the baseline does not pay for numpy.  (c) has no composition to stand next to: a
GrB_Matrix_assign into a submatrix is GrB_NOT_IMPLEMENTED in this library (gb_ops.hip accepts
GrB_ALL only), so the 16 assigns a 4 x 4 concat would replace cannot be issued; its time and
rate are reported alone.  When one untimed pass of a group takes more than 4 s the group is
timed with 2 warm-ups and 7 runs, and the result says so.
Algorithmic bytes, 8-byte values (n rows, nnz entries, tr x tc tiles):
  split   count 16 n tc (row bounds, read per tile column) + 4 nnz log-searched columns (counted
          once) + 12 n tc (counts and cuts); scan 12 n tc; rowptr 32 n tc; fill 12 nnz (A) +
          8 n tc (delta) + 12 nnz (tiles)          = 24 nnz + 4 nnz + 80 n tc
  concat  rowptr 16 n tc (tile row pointers, twice) + 8 n tc (start) + 8 n; fill 12 nnz (tiles) +
          8 n tc (start, row pointers for the row search) + 12 nnz (out)  = 24 nnz + 40 n tc + 8 n
Writes one JSON document (default profiles/concat_split_probe.json) and prints it.

    python tools/concat_split_probe.py [--scales 10 20 22] [--out profiles/concat_split_probe.json]
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
from graphblas_amd import device as gdev  # noqa: E402
from graphblas_amd import dist as gdist  # noqa: E402
from graphblas_amd.base import call  # noqa: E402
from graphblas_amd.matrix import Matrix, _CArray  # noqa: E402

RUNS, WARMUP, EF, GRID = 20, 3, 16, 4
SLOW_PASS_S, SLOW_RUNS, SLOW_WARMUP = 4.0, 7, 2
lib = gb.lib


def rmat(scale, dtype, name):
    n = 1 << scale
    A = Matrix.__new__(Matrix)
    A.dtype, A.name, A._h, A._nrows, A._ncols = gb.dtypes.lookup_dtype(dtype), name, ctypes.c_void_p(), n, n
    assert lib.GxB_Matrix_rmat(ctypes.byref(A._h), scale, EF, 42, 1, 2, 0, 0) == 0
    return A


def timed_in_turn(stream, fns):
    """(median seconds of each fn, runs, warm-ups), the fns alternating within every run"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    slow = time.perf_counter() - t0 > SLOW_PASS_S
    runs, warmup = (SLOW_RUNS, SLOW_WARMUP) if slow else (RUNS, WARMUP)
    for _ in range(warmup - 1):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(runs):
        for k, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    return [statistics.median(m) * 1e-3 for m in ms], runs, warmup


def same(x, y):
    cx, cy = x.to_coo(), y.to_coo()
    return x.shape == y.shape and all(a.dtype == b.dtype and np.array_equal(a, b) for a, b in zip(cx, cy))


def panel_tensors(T):
    v = gdev.matrix_view(T._h)
    return (gdev.device_tensor(torch, v.rowptr, v.nrows + 1), gdev.device_tensor(torch, v.colidx, v.nvals, "<i4"),
            gdev.device_tensor(torch, v.values, 1 if v.iso else v.nvals, "<i8"), bool(v.iso))


def probe(scale, stream):
    dtype = "INT64"
    n = 1 << scale
    A = rmat(scale, dtype, "A")
    nnz = A.nvals
    step = n // GRID
    cuts = [_CArray(np.arange(k * step, (k + 1) * step, dtype=np.uint64), "I") for k in range(GRID)]
    keep = {}

    def split():
        keep["split"] = A.ss.split(step)

    def extracts():
        out = [[gb.Matrix(dtype, step, step) for _ in cuts] for _ in cuts]
        for I, row in zip(cuts, out):
            for J, T in zip(cuts, row):
                call("GrB_Matrix_extract", [T, None, None, A, I, step, J, step, None])
        keep["extract"] = out

    split()
    extracts()
    tiles = keep["split"]
    assert len(tiles) == GRID and all(len(row) == GRID for row in tiles)
    assert all(same(t, e) for trow, erow in zip(tiles, keep["extract"]) for t, e in zip(trow, erow)), \
        "split differs from the 16 extracts"
    keep["extract"] = None

    def concat():
        keep["concat"] = gb.ss.concat(tiles)

    concat()
    assert same(keep["concat"], A), "concat of the tiles differs from A"

    panels = [row[0] for row in A.ss.split([step, None])]
    tensors = [panel_tensors(T) for T in panels]

    def concat_panels():
        keep["panels"] = gb.ss.concat([[T] for T in panels])

    def torch_panels():
        with torch.cuda.stream(stream):
            keep["torch"] = gdist.concat_row_panels(torch, tensors)

    concat_panels()
    torch_panels()
    torch.cuda.synchronize()
    got = panel_tensors(keep["panels"])
    assert all(torch.equal(a, b) for a, b in zip(got[:3], keep["torch"][:3])) and got[3] == keep["torch"][3], \
        "concat of the row panels differs from dist.concat_row_panels"
    del got
    print(f"scale {scale}: results equal, {nnz} entries; timing", file=sys.stderr, flush=True)
    (t_split, t_extract), runs_s, warm_s = timed_in_turn(stream, [split, extracts])
    keep["split"] = keep["extract"] = None
    (t_concat,), runs_c, warm_c = timed_in_turn(stream, [concat])
    keep["concat"] = None
    (t_panels, t_torch), runs_p, warm_p = timed_in_turn(stream, [concat_panels, torch_panels])
    split_bytes = 28 * nnz + 80 * n * GRID
    concat_bytes = 24 * nnz + 40 * n * GRID + 8 * n
    return {"scale": scale, "edge_factor": EF, "dtype": dtype, "nrows": n, "nnz": nnz, "grid": [GRID, GRID],
            "split_s": t_split, "extract16_s": t_extract, "extract16_over_split": t_extract / t_split,
            "split_runs": runs_s, "split_warmup": warm_s,
            "concat_s": t_concat, "assign16_s": None,
            "concat_runs": runs_c, "concat_warmup": warm_c,
            "concat_panels_s": t_panels, "torch_cat_panels_s": t_torch, "torch_cat_over_concat_panels": t_torch / t_panels,
            "panels_runs": runs_p, "panels_warmup": warm_p,
            "split_bytes": split_bytes, "split_GBps": split_bytes / t_split / 1e9,
            "concat_bytes": concat_bytes, "concat_GBps": concat_bytes / t_concat / 1e9}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scales", type=int, nargs="+", default=[10, 20, 22])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "concat_split_probe.json"))
    args = ap.parse_args()
    stream = torch.cuda.Stream()
    gb.set_stream(stream)
    results = []
    for s in args.scales:
        results.append(probe(s, stream))
        torch.cuda.empty_cache()
        doc = {"device": torch.cuda.get_device_name(0), "runs": RUNS, "warmup": WARMUP, "statistic": "median",
               "slow_groups": f"a group whose untimed pass takes more than {SLOW_PASS_S} s: {SLOW_RUNS} runs after "
                              f"{SLOW_WARMUP} warm-ups (see the *_runs fields)",
               "timer": "HIP events on the library stream, the calls of a group in turn within every run",
               "checked": "split equals the 16 extracts, concat equals A, concat of the row panels equals "
                          "dist.concat_row_panels, before timing",
               "assign16_s": "not measurable: GrB_Matrix_assign into a submatrix is GrB_NOT_IMPLEMENTED", "results": results}
        with open(args.out, "w") as f:  # after every scale: a long run leaves what it has measured
            json.dump(doc, f, indent=1)
            f.write("\n")
    print(json.dumps(doc))

if __name__ == "__main__":
    main()
