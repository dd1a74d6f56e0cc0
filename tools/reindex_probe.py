"""diag, reshape and flatten on R-MAT (gb_reindex.hip) next to two yardsticks: GrB_Matrix_apply with
GrB_IDENTITY_INT64 on the same matrix (one read and one write of every entry, plus the structure
copy), and the host route each operation replaces (to_coo, numpy, from_coo).

Per scale (default 10, 20 and 22, edge factor 16, INT64 values, the structure of the benchmark's
adjacency; n rows, nnz entries), between HIP events on the library stream, after warm-up, the device
calls alternate for 20 rounds; the median and the minimum of each are reported:
  identity         GrB_Matrix_apply(C, IDENTITY, A)
  reshape_dup      GxB_Matrix_reshapeDup(&C, A, row-major, 2 n, n / 2): new row pointer and columns,
                   the values copied
  reshape_inplace  GxB_Matrix_reshape(A, row-major, 2 n, n / 2): the values stay; the reshape back
                   to n x n between two timed calls is not timed
  matrix_diag      GxB_Vector_diag(w, A, 0): n binary searches
  vector_diag      GrB_Matrix_diag(&D, d, 0) of the degree vector d (row sums of A)
  flatten          GxB_Vector_flatten(w, A, row-major), at scale 10 only: w has n * n positions (8 MiB
                   of values at scale 10, 8 TiB at scale 20), so no larger scale has such a vector
Algorithmic bytes: identity 16 (n + 1) + 8 nnz (structure copy) + 16 nnz; reshape_dup 8 (n + 1) +
4 nnz read, 8 (2 n + 1) + 4 nnz written, + 16 nnz for the values; reshape_inplace the same without
the values.  The host routes are timed with a host clock around calls that end in a device
synchronise, 3 rounds (their data crosses the bus twice and is sorted again by from_coo).
Writes one JSON document (default profiles/reindex_probe.json) and prints it.

    python tools/reindex_probe.py [--scales 10 20 22] [--out profiles/reindex_probe.json]
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

RUNS, WARMUP, HOST_RUNS, EF = 20, 3, 3, 16
lib = gb.lib


def wrap(handle, n):
    """a front-end Matrix around a handle made through the C ABI (it frees the handle)"""
    M = gb.Matrix.__new__(gb.Matrix)
    M.dtype, M.name, M._h, M._nrows, M._ncols = gb.dtypes.INT64, "A", handle, n, n
    return M


def host_time(fn):
    out = []
    for _ in range(HOST_RUNS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return {"median_s": statistics.median(out), "min_s": min(out), "runs": HOST_RUNS}


def probe_scale(scale, stream):
    n = 1 << scale
    h = ctypes.c_void_p()
    assert lib.GxB_Matrix_rmat(ctypes.byref(h), scale, EF, 42, 1, 2, 0, 0) == 0
    A = wrap(h, n)
    nnz = A.nvals
    C = gb.Matrix("INT64", n, n)
    d = A.reduce_rowwise(gb.monoid.plus).new()
    w = gb.Vector("INT64", n)
    flat = gb.Vector("INT64", n * n) if scale <= 10 else None
    made = ctypes.c_void_p()

    def reshape_dup():
        rc = lib.GxB_Matrix_reshapeDup(ctypes.byref(made), A._h, False, 2 * n, n // 2, None)
        return rc

    def vector_diag():
        return lib.GrB_Matrix_diag(ctypes.byref(made), d._h, 0)

    calls = {
        "identity": (lambda: lib.GrB_Matrix_apply(C._h, None, None, lib.GrB_IDENTITY_INT64, A._h, None), None),
        "reshape_dup": (reshape_dup, lambda: lib.GrB_Matrix_free(ctypes.byref(made))),
        "reshape_inplace": (lambda: lib.GxB_Matrix_reshape(A._h, False, 2 * n, n // 2, None),
                            lambda: lib.GxB_Matrix_reshape(A._h, False, n, n, None)),
        "matrix_diag": (lambda: lib.GxB_Vector_diag(w._h, A._h, 0, None), None),
        "vector_diag": (vector_diag, lambda: lib.GrB_Matrix_free(ctypes.byref(made))),
    }
    if flat is not None:
        calls["flatten"] = (lambda: lib.GxB_Vector_flatten(flat._h, A._h, False, None), None)
    structure = 16 * (n + 1) + 8 * nnz
    reshape_bytes = 8 * (n + 1) + 4 * nnz + 8 * (2 * n + 1) + 4 * nnz
    nbytes = {"identity": structure + 16 * nnz, "reshape_dup": reshape_bytes + 16 * nnz, "reshape_inplace": reshape_bytes}
    for _ in range(WARMUP):
        for fn, after in calls.values():
            assert fn() == 0
            assert after is None or after() == 0
    torch.cuda.synchronize()
    ms = {k: [] for k in calls}
    for _ in range(RUNS):
        for k, (fn, after) in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            assert fn() == 0
            e1.record(stream)
            torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1))
            assert after is None or after() == 0
    res = {"scale": scale, "edge_factor": EF, "nrows": n, "nnz": nnz, "degree_vector_nvals": d.nvals,
           "diagonal_nvals": w.nvals, "reshape_div64": gb.get_knob("stat_reshape_div64")}
    for k in calls:
        med = statistics.median(ms[k]) * 1e-3
        res[k] = {"median_s": med, "min_s": min(ms[k]) * 1e-3}
        if k in nbytes:
            res[k].update(bytes=nbytes[k], GBps=nbytes[k] / med / 1e9)
        if k != "identity":
            res[k]["ratio_to_identity"] = med / res["identity"]["median_s"]

    # the host routes: what each operation took before
    def host_reshape():
        r, c, x = A.to_coo()
        lin = r * np.uint64(n) + c
        return gb.Matrix.from_coo(lin // np.uint64(n // 2), lin % np.uint64(n // 2), x, nrows=2 * n, ncols=n // 2)

    def host_matrix_diag():
        r, c, x = A.to_coo()
        on = r == c
        return gb.Vector.from_coo(r[on], x[on], size=n)

    def host_vector_diag():
        i, x = d.to_coo()
        return gb.Matrix.from_coo(i, i, x, nrows=n, ncols=n)

    def host_flatten():
        r, c, x = A.to_coo()
        return gb.Vector.from_coo(r * np.uint64(n) + c, x, size=n * n)

    routes = {"reshape_dup": host_reshape, "matrix_diag": host_matrix_diag, "vector_diag": host_vector_diag}
    if flat is not None:
        routes["flatten"] = host_flatten
    for k, fn in routes.items():
        fn()  # warm-up
        res[k]["host_route"] = host_time(fn)
        res[k]["host_route_over_device"] = res[k]["host_route"]["median_s"] / res[k]["median_s"]
    res["reshape_inplace"]["host_route_over_device"] = \
        res["reshape_dup"]["host_route"]["median_s"] / res["reshape_inplace"]["median_s"]
    del A, C, d, w, flat
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scales", type=int, nargs="+", default=[10, 20, 22])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reindex_probe.json"))
    args = ap.parse_args()
    stream = torch.cuda.Stream()
    gb.set_stream(stream)
    doc = {"device": torch.cuda.get_device_name(0), "runs": RUNS, "warmup": WARMUP,
           "statistic": "median and minimum of alternating rounds", "timer": "HIP events on the library stream",
           "host_route_timer": "host clock around calls that end in a device synchronise",
           "results": [probe_scale(s, stream) for s in args.scales]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
