"""Per-level profile of the headline BFS (bench.py's notebook loop, any_pair, R-MAT s22, the
bench's 16 roots) with the level speculation off (knob bfs_spec=1): one k_iso_work launch per
level, so the launches of a kernel trace / PMC pass map one to one onto (root, level).

  run (the workload, under tools/pmc_passes.sh on the GPU box):
      bash tools/pmc_passes.sh NAME k_iso_work python3 <repo>/tools/pull_levels.py run NAME DIR [SCALE]
    (DIR: the directory the passes write their NAME_trace / NAME_pmcN output to, absolute);
    a warm pass over the 16 roots (builds the matrix's cached tables), then the measured pass;
    writes DIR/NAME_levels.json: per root and level the frontier size, the next
    frontier's size and the direction.  The direction is the device's rule replayed on the host
    from the level vector the BFS left: the root's level pushes (host-decided), then push while
    m_f * alpha < open rows * average degree (gb_dir_decide; m_f = out-edges of the frontier,
    which both kernels' hints give exactly; open = rows outside v after the level's stamp).
  table (after the passes, anywhere):
      python3 tools/pull_levels.py table NAME DIR OUT
    joins the last launches of k_iso_work in the trace and in the FETCH_SIZE / WRITE_SIZE passes
    (by dispatch order) with DIR/NAME_levels.json and writes profiles/OUT.json.
  compare:
      python3 tools/pull_levels.py compare BEFORE AFTER OUT
    two such files side by side (per launch, per BFS, per direction) -> profiles/OUT.json."""
import csv
import ctypes
import glob
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALPHA = 48  # gb_spmv_iso's default (knob push_alpha)


def run(name, out_dir, scale):
    import torch

    sys.path.insert(0, os.path.join(ROOT, "graph-python_amd"))
    import graphblas_amd as gb

    lib = gb.lib
    gb.set_knob("bfs_spec", 1)
    stream = torch.cuda.Stream()
    gb.set_stream(stream)
    n = 1 << scale
    A = ctypes.c_void_p()
    assert lib.GxB_Matrix_rmat(ctypes.byref(A), scale, 16, 42, 0, 0, 0, 0) == 0
    assert lib.GxB_Matrix_prepare_transpose(A) == 0
    nv = ctypes.c_uint64()
    lib.GrB_Matrix_nvals(ctypes.byref(nv), A)
    nnz = nv.value
    ap = np.empty(n + 1, np.uint64)
    ai = np.empty(nnz, np.uint64)
    ax = np.empty(nnz, np.bool_)
    lens = [ctypes.c_uint64(n + 1), ctypes.c_uint64(nnz), ctypes.c_uint64(nnz)]
    lib.GrB_Matrix_export_BOOL(ctypes.c_void_p(ap.ctypes.data), ctypes.c_void_p(ai.ctypes.data),
                               ctypes.c_void_p(ax.ctypes.data), *[ctypes.byref(x) for x in lens], 0, A)
    deg = np.diff(ap.astype(np.int64))
    del ai, ax
    roots = np.random.default_rng(42).choice(np.flatnonzero(deg > 0), 16, replace=False)
    q, v = ctypes.c_void_p(), ctypes.c_void_p()
    lib.GrB_Vector_new(ctypes.byref(q), lib.GrB_BOOL, n)
    lib.GrB_Vector_new(ctypes.byref(v), lib.GrB_INT32, n)
    sr = lib.GxB_ANY_PAIR_BOOL

    def bfs(src):
        lib.GrB_Vector_clear(q)
        lib.GrB_Vector_clear(v)
        lib.GrB_Vector_setElement_BOOL(q, True, int(src))
        d = 0
        while True:
            d += 1
            lib.GrB_Vector_assign_INT32(v, q, None, d, lib.GrB_ALL, n, None)
            lib.GrB_vxm(q, v, None, sr, q, A, lib.GrB_DESC_RSC)
            lib.GrB_Vector_nvals(ctypes.byref(nv), q)
            if nv.value == 0:
                return d

    for r in roots:
        bfs(r)
    torch.cuda.synchronize()
    per_root = []
    for r in roots:
        depth = bfs(r)
        lib.GrB_Vector_nvals(ctypes.byref(nv), v)
        idx = np.empty(nv.value, np.uint64)
        lv = np.empty(nv.value, np.int32)
        lib.GrB_Vector_extractTuples_INT32(ctypes.c_void_p(idx.ctypes.data), ctypes.c_void_p(lv.ctypes.data),
                                           ctypes.byref(nv), v)
        size = np.bincount(lv, minlength=depth + 2)
        edges = np.bincount(lv, weights=deg[idx.astype(np.int64)], minlength=depth + 2)
        levels, seen = [], 0
        for d in range(1, depth + 1):
            seen += int(size[d])
            push = d == 1 or edges[d] * ALPHA < (n - seen) * (nnz / n)
            levels.append({"level": d, "frontier": int(size[d]), "frontier_edges": int(edges[d]),
                           "open_rows": n - seen, "next": int(size[d + 1]), "direction": "push" if push else "pull"})
        per_root.append({"root_index": len(per_root), "root": int(r), "levels": levels})
    os.makedirs(out_dir, exist_ok=True)
    json.dump({"scale": scale, "n": n, "nnz": int(nnz), "alpha": ALPHA, "roots": per_root},
              open(os.path.join(out_dir, f"{name}_levels.json"), "w"))
    print(f"{name}: {sum(len(r['levels']) for r in per_root)} measured levels over {len(per_root)} roots")


def launches(pattern, kernel, value):
    """rows of the rocprofv3 csv files matching `pattern` whose kernel name holds `kernel`, summed
    per dispatch by value(row), in dispatch order"""
    per = {}
    for f in glob.glob(pattern, recursive=True):
        for r in csv.DictReader(open(f)):
            if kernel not in r["Kernel_Name"]:
                continue
            x = value(r)
            if x is not None:
                k = int(r["Dispatch_Id"])
                per[k] = per.get(k, 0.0) + x
    return [per[k] for k in sorted(per)]


def table(name, out_dir, out, kernel="k_iso_work"):
    meta = json.load(open(os.path.join(out_dir, f"{name}_levels.json")))
    m = sum(len(r["levels"]) for r in meta["roots"])
    dur = launches(os.path.join(out_dir, f"{name}_trace", "**", "*kernel_trace.csv"), kernel,
                   lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    cols = {"us": dur}
    for c in ("FETCH_SIZE", "WRITE_SIZE"):
        cols[c] = launches(os.path.join(out_dir, f"{name}_pmc*", "**", "*counter_collection.csv"), kernel,
                           lambda r, c=c: float(r["Counter_Value"]) if r["Counter_Name"] == c else None)
    for c, xs in cols.items():
        assert len(xs) >= m, f"{c}: {len(xs)} launches of {kernel}, {m} measured levels"
    i = 0
    tot = {"us": 0.0, "FETCH_SIZE": 0.0, "WRITE_SIZE": 0.0}
    for r in meta["roots"]:
        for lv in r["levels"]:
            for c, xs in cols.items():
                x = xs[len(xs) - m + i]
                lv["us" if c == "us" else c.lower() + "_kib"] = round(x, 2)
                tot[c] += x
            i += 1
    nb = len(meta["roots"])
    meta.update({
        "kernel": kernel, "launches": m, "launches_in_trace": len(dur),
        "method": "tools/pmc_passes.sh (kernel trace, then FETCH_SIZE and WRITE_SIZE in passes of their own) on "
                  "tools/pull_levels.py run: bfs_spec=1, a warm pass, then the measured pass whose launches are the "
                  "last `launches` of the kernel; durations from the trace; KiB as the counters report them "
                  "(bytes_per_launch = 2 x FETCH_SIZE + WRITE_SIZE, KiB -> bytes, as profiles/traffic_r06.json)",
        "us_per_bfs": tot["us"] / nb,
        "fetch_kib_per_launch": tot["FETCH_SIZE"] / m, "write_kib_per_launch": tot["WRITE_SIZE"] / m,
        "bytes_per_launch": (2 * tot["FETCH_SIZE"] + tot["WRITE_SIZE"]) * 1024 / m,
        "bytes_per_bfs": (2 * tot["FETCH_SIZE"] + tot["WRITE_SIZE"]) * 1024 / nb,
    })
    json.dump(meta, open(os.path.join(ROOT, "profiles", f"{out}.json"), "w"), indent=1)
    print(f"{out}: {m} levels, {meta['us_per_bfs']:.1f} us of {kernel} per BFS, "
          f"{meta['bytes_per_launch'] / 1e6:.1f} MB per launch")
    for r in meta["roots"]:
        print(f"root {r['root_index']:2d}: " + " ".join(
            f"{lv['direction'][:3]}:{lv['us']:.0f}us/{lv['fetch_size_kib'] / 1024:.0f}M" for lv in r["levels"]))


def compare(before, after, out):
    """profiles/OUT.json: the kernel's FETCH_SIZE / WRITE_SIZE and time of two `table` files side
    by side -- per launch, per BFS, and per BFS split by the levels' direction"""
    res = {"kernel": "k_iso_work"}
    for tag, name in (("before", before), ("after", after)):
        t = json.load(open(os.path.join(ROOT, "profiles", f"{name}.json")))
        res["method"] = t["method"]
        nb = len(t["roots"])
        r = {"file": f"profiles/{name}.json", "launches": t["launches"]}
        for k in ("fetch_kib_per_launch", "write_kib_per_launch", "bytes_per_launch", "bytes_per_bfs", "us_per_bfs"):
            r[k] = t[k]
        for d in ("pull", "push"):
            lv = [x for root in t["roots"] for x in root["levels"] if x["direction"] == d]
            r[d] = {"levels_per_bfs": len(lv) / nb, "us_per_bfs": sum(x["us"] for x in lv) / nb,
                    "fetch_kib_per_bfs": sum(x["fetch_size_kib"] for x in lv) / nb,
                    "write_kib_per_bfs": sum(x["write_size_kib"] for x in lv) / nb}
        res[tag] = r
    b, a = res["before"], res["after"]
    res["fetch_size_drop_kib_per_launch"] = b["fetch_kib_per_launch"] - a["fetch_kib_per_launch"]
    res["bytes_drop_per_launch"] = b["bytes_per_launch"] - a["bytes_per_launch"]
    res["bytes_drop_per_bfs"] = b["bytes_per_bfs"] - a["bytes_per_bfs"]
    json.dump(res, open(os.path.join(ROOT, "profiles", f"{out}.json"), "w"), indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(sys.argv[2], sys.argv[3], int(sys.argv[4]) if len(sys.argv) > 4 else 22)
    elif sys.argv[1] == "compare":
        compare(sys.argv[2], sys.argv[3], sys.argv[4])
    else:
        table(sys.argv[2], sys.argv[3], sys.argv[4])
