"""The numpy model of concat / split on the (present, values) pairs of dense_model.py, written
from the rule of the C API (include/graphblas_amd.h), not from the kernels: a concat is np.block of
the tiles cast to the output's type, a split is slicing, and the chunks argument is normalised by
a pure function.  A vector is a 1-D pair; inside a matrix concat it counts as N x 1."""
import json
import os

import numpy as np

import dense_model as dm

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "concat_split_golden.json")


def as_matrix(A):
    p, v = A
    return (p.reshape(-1, 1), v.reshape(-1, 1)) if p.ndim == 1 else (p, v)


def concat(tiles, dtype):
    """tiles: a flat list of 1-D pairs (-> a vector) or a list of lists of pairs (-> a matrix)"""
    t = dm.NP[dtype]
    if not isinstance(tiles[0], (list, tuple)) or isinstance(tiles[0][0], np.ndarray):
        p = np.concatenate([q[0] for q in tiles])
        v = np.concatenate([dm.cast(q[1], dtype) for q in tiles])
        return p, np.where(p, v, t(0)).astype(t)
    rows = [[as_matrix(q) for q in row] for row in tiles]
    p = np.block([[q[0] for q in row] for row in rows])
    v = np.block([[dm.cast(q[1], dtype) for q in row] for row in rows])
    return p, np.where(p, v, t(0)).astype(t)


def is_iso(tiles, dtype):
    """the rule of the result's iso flag, given (pair, tile is iso) for every tile: every tile with
    entries is iso and their values cast to dtype have equal bits"""
    seen = set()
    for (p, v), iso in tiles:
        if not p.any():
            continue
        if not iso:
            return False
        seen.add(dm.cast(v[p][:1], dtype).tobytes())
    return len(seen) == 1


def bounds(sizes):
    return np.concatenate([[0], np.cumsum(np.asarray(sizes, np.int64))]).astype(np.int64)


def split(A, chunks):
    """chunks already normalised: [row sizes, column sizes] for a matrix, [sizes] for a vector"""
    p, v = A
    if p.ndim == 1:
        b = bounds(chunks[0])
        assert b[-1] == p.shape[0]
        return [(p[b[i]:b[i + 1]], v[b[i]:b[i + 1]]) for i in range(len(b) - 1)]
    rb, cb = bounds(chunks[0]), bounds(chunks[1])
    assert rb[-1] == p.shape[0] and cb[-1] == p.shape[1]
    return [[(p[rb[i]:rb[i + 1], cb[j]:cb[j + 1]], v[rb[i]:rb[i + 1], cb[j]:cb[j + 1]])
             for j in range(len(cb) - 1)] for i in range(len(rb) - 1)]


def _whole(x):
    if isinstance(x, (int, np.integer)) and not isinstance(x, bool):
        return int(x)
    if isinstance(x, float) and x.is_integer():
        return int(x)
    return None


def normalize_chunks(chunks, shape):
    """one list of sizes per dimension.  Per dimension: an integer k (size // k chunks of k and the
    remainder), a list / tuple with at most one None ("the rest"), None (the whole dimension) or
    a 1-D integer array; one integer stands for every dimension.  TypeError / ValueError as the
    golden file's error cases say."""
    k = _whole(chunks)
    if k is not None:
        chunks = [k] * len(shape)
    elif isinstance(chunks, np.ndarray):
        chunks = list(chunks)
    elif not isinstance(chunks, (list, tuple)):
        raise TypeError("chunks")
    if len(chunks) != len(shape):
        raise ValueError("length")
    out = []
    for size, c in zip(shape, chunks):
        k = _whole(c)
        if c is None:
            cur = [size]
        elif k is not None:
            if k < 0:
                raise ValueError("negative")
            cur = [k] * (size // k) + ([size % k] if size % k else [])
        elif isinstance(c, np.ndarray):
            if c.ndim != 1 or not np.issubdtype(c.dtype, np.integer):
                raise TypeError("array")
            if (c < 0).any():
                raise ValueError("negative")
            cur = [int(x) for x in c]
        elif isinstance(c, (list, tuple)):
            if sum(x is None for x in c) > 1:
                raise TypeError("two rests")
            known = []
            for x in c:
                if x is None:
                    continue
                w = _whole(x)
                if w is None:
                    raise TypeError("element")
                if w < 0:
                    raise ValueError("negative")
                known.append(w)
            if len(known) < len(c) and sum(known) > size:
                raise ValueError("too large")
            cur = [size - sum(known) if x is None else _whole(x) for x in c]
        else:
            raise TypeError("dimension")
        out.append(cur)
    return out


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def golden_operand(d):
    """(present, values) of a golden operand: a vector has no "cols" """
    t = dm.NP[d["dtype"]]
    if "cols" not in d:
        p, v = np.zeros(d["size"], bool), np.zeros(d["size"], t)
        idx = (np.asarray(d["rows"], np.int64),)
    else:
        p, v = np.zeros((d["nrows"], d["ncols"]), bool), np.zeros((d["nrows"], d["ncols"]), t)
        idx = (np.asarray(d["rows"], np.int64), np.asarray(d["cols"], np.int64))
    p[idx] = True
    v[idx] = np.asarray(d["vals"], t)
    return p, v


def golden_chunks(x):
    """a chunks argument as the golden file spells it: {"array": [...]} is a numpy array,
    {"tuple": [...]} a tuple, anything else itself (lists, integers, floats, null)"""
    if isinstance(x, dict) and "array" in x:
        return np.array(x["array"])
    if isinstance(x, dict) and "tuple" in x:
        return tuple(golden_chunks(y) for y in x["tuple"])
    if isinstance(x, list):
        return [golden_chunks(y) for y in x]
    return x
