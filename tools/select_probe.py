"""GrB_select on R-MAT (gb_select.hip) next to the same filter written in torch on the
GxB_Matrix_device_view arrays -- what a user had to do before select existed: expand the rows,
take a boolean mask, index with it, rebuild rowptr with bincount + cumsum.

Per scale (default 20 and 22, edge factor 16), between HIP events on the library stream, after
warm-up, the median of 20 runs of
  tril(A, -1)        on the BOOL iso graph          (positional: colidx and rowptr only)
  A.select(">", t)   on an INT64-valued copy, t the median value (about half kept)
Algorithmic bytes of a call (n rows, nnz entries, kept of them; the keep words, their byte
counts and bases add 17 B per 64 entries and are left out):
  positional  4 nnz (colidx, mark) + 4 nnz (colidx, scatter) + 4 kept (colidx out) + 16 (n + 1) (rowptr in, out)
  value       8 nnz (values, mark) + 4 nnz (colidx, scatter) + 8 kept (values, scatter)
              + 12 kept (colidx + values out) + 16 (n + 1)
Writes one JSON document (default profiles/select_probe.json) and prints it.

    python tools/select_probe.py [--scales 20 22] [--out profiles/select_probe.json]
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
from graphblas_amd.device import device_tensor, matrix_view  # noqa: E402

RUNS, WARMUP, EF = 20, 3, 16
lib = gb.lib


def timed(stream, fn):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(RUNS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms) * 1e-3


def nvals_of(h):
    nv = ctypes.c_uint64()
    assert lib.GrB_Matrix_nvals(ctypes.byref(nv), h) == 0
    return nv.value


def torch_filter(stream, view, n, nnz, keep_of, with_values):
    rowptr = device_tensor(torch, view.rowptr, n + 1, "<i8")
    col = device_tensor(torch, view.colidx, nnz, "<i4")
    vals = device_tensor(torch, view.values, nnz, "<i8") if with_values else None
    out = {}

    def run():
        with torch.cuda.stream(stream):
            rows = torch.repeat_interleave(torch.arange(n, device="cuda"), rowptr[1:] - rowptr[:-1])
            keep = keep_of(rows, col, vals)
            out["col"] = col[keep]
            if with_values:
                out["vals"] = vals[keep]
            counts = torch.bincount(rows[keep], minlength=n)
            out["rowptr"] = torch.cat([counts.new_zeros(1), torch.cumsum(counts, 0)])

    return run, out


def probe_scale(scale, stream):
    n = 1 << scale
    res = {"scale": scale, "edge_factor": EF, "nrows": n}
    # ---- tril(A, -1) on the BOOL iso graph
    A = ctypes.c_void_p()
    assert lib.GxB_Matrix_rmat(ctypes.byref(A), scale, EF, 42, 0, 0, 0, 0) == 0
    nnz = nvals_of(A)
    C = ctypes.c_void_p()
    assert lib.GrB_Matrix_new(ctypes.byref(C), lib.GrB_BOOL, n, n) == 0

    def tril():
        assert lib.GrB_Matrix_select_INT64(C, None, None, lib.GrB_TRIL, A, -1, None) == 0

    t_new = timed(stream, tril)
    kept = nvals_of(C)
    run, out = torch_filter(stream, matrix_view(A), n, nnz, lambda r, c, v: c < r, False)
    t_torch = timed(stream, run)
    assert int(out["rowptr"][-1]) == kept and out["col"].numel() == kept
    by = 8 * nnz + 4 * kept + 16 * (n + 1)
    res["tril_bool_iso"] = {"nnz": nnz, "kept": kept, "select_s": t_new, "torch_s": t_torch, "bytes": by,
                            "select_GBps": by / t_new / 1e9, "speedup_vs_torch": t_torch / t_new}
    del out
    lib.GrB_Matrix_free(ctypes.byref(C))
    lib.GrB_Matrix_free(ctypes.byref(A))
    torch.cuda.empty_cache()
    # ---- A.select(">", t) on INT64 values in [1, 255]
    assert lib.GxB_Matrix_rmat(ctypes.byref(A), scale, EF, 42, 1, 2, 0, 0) == 0
    nnz = nvals_of(A)
    assert lib.GrB_Matrix_new(ctypes.byref(C), lib.GrB_INT64, n, n) == 0
    view = matrix_view(A)
    t = int(torch.median(device_tensor(torch, view.values, nnz, "<i8")))

    def gt():
        assert lib.GrB_Matrix_select_INT64(C, None, None, lib.GrB_VALUEGT_INT64, A, t, None) == 0

    t_new = timed(stream, gt)
    kept = nvals_of(C)
    run, out = torch_filter(stream, view, n, nnz, lambda r, c, v: v > t, True)
    t_torch = timed(stream, run)
    assert int(out["rowptr"][-1]) == kept and out["vals"].numel() == kept
    by = 12 * nnz + 20 * kept + 16 * (n + 1)
    res["valuegt_int64"] = {"nnz": nnz, "kept": kept, "thunk": t, "selectivity": kept / nnz, "select_s": t_new,
                            "torch_s": t_torch, "bytes": by, "select_GBps": by / t_new / 1e9,
                            "speedup_vs_torch": t_torch / t_new}
    del out
    lib.GrB_Matrix_free(ctypes.byref(C))
    lib.GrB_Matrix_free(ctypes.byref(A))
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scales", type=int, nargs="+", default=[20, 22])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "select_probe.json"))
    args = ap.parse_args()
    stream = torch.cuda.Stream()
    gb.set_stream(stream)
    doc = {"device": torch.cuda.get_device_name(0), "runs": RUNS, "warmup": WARMUP, "statistic": "median",
           "timer": "HIP events on the library stream", "results": [probe_scale(s, stream) for s in args.scales]}
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
