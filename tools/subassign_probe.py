"""GxB_Matrix_subassign on R-MAT graphs (gb_subassign.hip) next to the calls it stands beside.

Per scale (default 10, 20 and 22, edge factor 16, INT64 values): A is the graph, cut 4 x 4 into
equal tiles (A.ss.split).  Between HIP events on the library stream, after the warm-ups, the median
of the runs of
  (a) 16 GxB_Matrix_subassign calls placing the tiles into an empty C   against
  (b) one ss.concat of the same tiles, into a new matrix;
  (c) one unmasked, accumulator-free overwrite of tile (1, 2) in a copy of A   against
  (d) GrB_Matrix_dup of A: the cost of rewriting C once, which every subassign pays;
  (e) one masked, accumulated subassign of the same tile (mask: the tile's structure, accum plus).
The members of a group are timed in turn within every run, so they see the same machine state.
Before timing, (a) and (b) must both give A, (c) must leave A as it is (the tile is A's own), and
(e) must double the tile's entries and nothing else.  The index lists are the explicit arrays the
front end passes for a slice, built once outside the timed window.  (c) and (e) work on a copy of
A made outside the timed window: (c) writes the entries that are there, (e) adds the tile to itself
once more in every run, which changes values only, so the structure and the work stay the same.
Writes one JSON document (default profiles/subassign_probe.json) and prints it.

    python tools/subassign_probe.py [--scales 10 20 22] [--out profiles/subassign_probe.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from concat_split_probe import EF, GRID, RUNS, WARMUP, SLOW_PASS_S, SLOW_RUNS, SLOW_WARMUP, rmat, same, timed_in_turn  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "graph-python_amd"))
import graphblas_amd as gb  # noqa: E402
from graphblas_amd.base import call, descriptor_lookup  # noqa: E402
from graphblas_amd.matrix import _CArray  # noqa: E402


def probe(scale, stream):
    dtype = "INT64"
    n = 1 << scale
    A = rmat(scale, dtype, "A")
    nnz = A.nvals
    step = n // GRID
    cuts = [_CArray(np.arange(k * step, (k + 1) * step, dtype=np.uint64), "I") for k in range(GRID)]
    tiles = A.ss.split(step)
    keep = {}

    def place16():
        C = gb.Matrix(dtype, n, n)
        for I, row in zip(cuts, tiles):
            for J, T in zip(cuts, row):
                call("GxB_Matrix_subassign", [C, None, None, T, I, step, J, step, None])
        keep["placed"] = C

    def concat():
        keep["concat"] = gb.ss.concat(tiles)

    place16()
    concat()
    assert same(keep["placed"], A), "the 16 subassigns do not rebuild A"
    assert same(keep["concat"], A), "concat of the tiles differs from A"
    keep.clear()

    T, I, J = tiles[1][2], cuts[1], cuts[2]
    B = A.dup()
    plus = gb.binary.plus[dtype]
    s_desc = descriptor_lookup(mask_structure=True)

    def overwrite():
        call("GxB_Matrix_subassign", [B, None, None, T, I, step, J, step, None])

    def dup():
        keep["dup"] = A.dup()

    def masked():
        call("GxB_Matrix_subassign", [B, T, plus, T, I, step, J, step, s_desc])

    overwrite()
    assert same(B, A), "overwriting a tile with itself changed A"
    masked()
    twice = A.dup()
    twice(accum=gb.binary.plus)[np.arange(step, 2 * step), np.arange(2 * step, 3 * step)] << T
    assert same(B, twice), "the masked, accumulated subassign differs from the unmasked accumulated one"
    assert B.nvals == nnz
    del twice
    B = A.dup()
    print(f"scale {scale}: results equal, {nnz} entries, tile (1, 2) holds {T.nvals}; timing", file=sys.stderr,
          flush=True)
    (t_place, t_concat), runs_p, warm_p = timed_in_turn(stream, [place16, concat])
    keep.clear()
    (t_over, t_dup), runs_o, warm_o = timed_in_turn(stream, [overwrite, dup])
    keep.clear()
    # the values of the tile grow by T each run; structure, and with it the work, stays
    (t_masked,), runs_m, warm_m = timed_in_turn(stream, [masked])
    return {"scale": scale, "edge_factor": EF, "dtype": dtype, "nrows": n, "nnz": nnz, "grid": [GRID, GRID],
            "tile_nnz": T.nvals,
            "subassign16_s": t_place, "concat_s": t_concat, "subassign16_over_concat": t_place / t_concat,
            "place_runs": runs_p, "place_warmup": warm_p,
            "overwrite_tile_s": t_over, "dup_s": t_dup, "overwrite_over_dup": t_over / t_dup,
            "overwrite_runs": runs_o, "overwrite_warmup": warm_o,
            "masked_accum_tile_s": t_masked, "masked_runs": runs_m, "masked_warmup": warm_m}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scales", type=int, nargs="+", default=[10, 20, 22])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "subassign_probe.json"))
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
               "checked": "the 16 subassigns and the concat both rebuild A; overwriting a tile with itself leaves A; "
                          "the masked accumulated subassign equals the unmasked accumulated one, before timing",
               "results": results}
        with open(args.out, "w") as f:  # after every scale: a long run leaves what it has measured
            json.dump(doc, f, indent=1)
            f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
