"""GxB_eWiseUnion on R-MAT graphs (gb_ewise_union.hip) next to what the library offered before it.

Per scale (default 20 and 22, edge factor 16) and value type (INT64, then FP64): A is the graph,
B its transpose, C = A - B on the union of their structures.  Between HIP events on the library
stream, after 3 warm-ups, the median of 20 runs of each of
  (a) C << A.ewise_union(B, binary.minus, 0, 0)           one call, one write-back
  (b) the five-call composition python-graphblas falls back to without GxB_eWiseUnion
      (reference core/matrix.py:70-79): two bound-scalar applies, two eWiseAdds, one eWiseMult
  (c) C << A.ewise_add(B, binary.minus)                    the same structure through the
      row-per-thread k_ewise_mat; its B-only values are +b, not the union's -b
timed in turn within every run, so all three see the same machine state.  Before timing, (a) and
(b) must give identical to_coo() output.
Algorithmic bytes of (a), 8-byte values (n rows, na / nb entries, `both` of them shared,
bonly = nb - both; the mark words, their counts and bases add 17 B per 64 entries of B and are
left out; a binary-searched row counts once):
  mark    4 nb (B columns) + 4 na (A columns, searched) + 16 (n + 1) (both row pointers)
  rowptr  24 (n + 1)
  fill A  4 na + 8 na (A) + 4 nb (B columns, searched) + 8 both (B values) + 12 na (out) + 16 (n + 1)
  fill B  4 nb + 8 bonly (B) + 4 na (A columns, searched) + 12 bonly (out) + 16 (n + 1)
  total   32 na + 12 nb + 8 both + 20 bonly + 72 (n + 1)
Writes one JSON document (default profiles/ewise_union_probe.json) and prints it.

    python tools/ewise_union_probe.py [--scales 20 22] [--out profiles/ewise_union_probe.json]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "graph-python_amd"))
import graphblas_amd as gb  # noqa: E402
from graphblas_amd.matrix import Matrix  # noqa: E402

RUNS, WARMUP, EF = 20, 3, 16
lib = gb.lib


def rmat(scale, values, transposed, dtype, name):
    """the seeded R-MAT graph (or its transpose) as a front-end Matrix"""
    n = 1 << scale
    A = Matrix.__new__(Matrix)
    A.dtype, A.name, A._h, A._nrows, A._ncols = gb.dtypes.lookup_dtype(dtype), name, ctypes.c_void_p(), n, n
    assert lib.GxB_Matrix_rmat(ctypes.byref(A._h), scale, EF, 42, values | (0x100 if transposed else 0), 2, 0, 0) == 0
    return A


def timed_in_turn(stream, fns):
    """median seconds of each fn, the fns alternating within every run"""
    for _ in range(WARMUP):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(RUNS):
        for k, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    return [statistics.median(m) * 1e-3 for m in ms]


def probe(scale, dtype, values, stream):
    n = 1 << scale
    A, B = rmat(scale, values, False, dtype, "A"), rmat(scale, values, True, dtype, "B")
    zero = gb.Scalar.from_value(0, dtype)
    minus, first, second = gb.binary.minus[dtype], gb.binary.first[dtype], gb.binary.second[dtype]
    Ca, Cb, Cc = (gb.Matrix(dtype, n, n) for _ in range(3))
    nl, nr = gb.Matrix(dtype, n, n), gb.Matrix(dtype, n, n)

    def union():
        Ca << A.ewise_union(B, minus, zero, zero)

    def composition():
        nl << B.apply(second, right=zero)
        nl << A.ewise_add(nl, first)
        nr << A.apply(second, right=zero)
        nr << B.ewise_add(nr, first)
        Cb << nl.ewise_mult(nr, minus)

    def add():
        Cc << A.ewise_add(B, minus)

    union()
    counts = {c: gb.get_knob(f"stat_union_{c}") for c in ("both", "a_only", "b_only")}
    composition()
    got, ref = Ca.to_coo(), Cb.to_coo()
    assert all(x.dtype == y.dtype and np.array_equal(x, y, equal_nan=x.dtype.kind == "f") for x, y in zip(got, ref)), \
        "ewise_union differs from the five-call composition"
    total = int(got[0].size)
    del got, ref
    print(f"scale {scale} {dtype}: results equal, {total} entries; timing", file=sys.stderr, flush=True)
    t_a, t_b, t_c = timed_in_turn(stream, [union, composition, add])
    na, nb = A.nvals, B.nvals
    both, bonly = counts["both"], counts["b_only"]
    assert total == na + bonly and Cc.nvals == total
    by = 32 * na + 12 * nb + 8 * both + 20 * bonly + 72 * (n + 1)
    return {"scale": scale, "edge_factor": EF, "dtype": dtype, "nrows": n, "nnz_A": na, "nnz_B": nb, "both": both,
            "a_only": counts["a_only"], "b_only": bonly, "nnz_C": total, "union_s": t_a, "composition_s": t_b,
            "ewise_add_s": t_c, "union_bytes": by, "union_GBps": by / t_a / 1e9,
            "composition_over_union": t_b / t_a, "ewise_add_over_union": t_c / t_a}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scales", type=int, nargs="+", default=[20, 22])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ewise_union_probe.json"))
    args = ap.parse_args()
    stream = torch.cuda.Stream()
    gb.set_stream(stream)
    results = []
    for dtype, values in (("INT64", 1), ("FP64", 2)):
        for s in args.scales:
            results.append(probe(s, dtype, values, stream))
            torch.cuda.empty_cache()
    doc = {"device": torch.cuda.get_device_name(0), "runs": RUNS, "warmup": WARMUP, "statistic": "median",
           "timer": "HIP events on the library stream, the three calls in turn within every run",
           "checked": "to_coo() of ewise_union equals the five-call composition, before timing", "results": results}
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
