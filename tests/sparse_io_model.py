"""numpy model of the sparse import and export (GxB_{Matrix,Vector}_{import,export}_sparse and the
front end over them): COO and compressed input to the canonical form -- a pair (present, values) of
dense arrays, as every model of this suite -- and the canonical form to each export format in each
index width.  The typecast is dense_model.cast, the duplicate fold dense_model.build (stable sort,
fold in input order with the operator); without an operator the last duplicate is kept, which is
the fold with `second`."""
import json
import os

import numpy as np

import dense_model as dm

HERE = os.path.dirname(os.path.abspath(__file__))
INDEX = {"INT32": np.int32, "INT64": np.int64, "UINT64": np.uint64}


class IndexOutOfBound(Exception):
    pass


class InvalidValue(Exception):
    pass


def golden():
    with open(os.path.join(HERE, "golden", "sparse_io_golden.json")) as f:
        return json.load(f)


def value_type(values, dtype=None):
    """the type an import gives its result: `dtype`, else the values' own (a Python int is INT64)"""
    return dtype if dtype is not None else dm.name_of(np.asarray(values).dtype)


# ---------------------------------------------------------------------- import
def from_coo(shape, indices, values, dup_op=None, dtype=None):
    """indices: one array per dimension, signed or unsigned; values: an array or one scalar"""
    shape = tuple(int(n) for n in shape)
    idx = [np.asarray(i) for i in indices]
    n = idx[0].size
    dt = value_type(values, dtype)
    vals = np.broadcast_to(np.asarray(values), (n,)) if np.ndim(values) == 0 else np.asarray(values)
    if any(i.size != n for i in idx) or vals.size != n:
        raise ValueError("lengths must match")
    for i, dim in zip(idx, shape):
        if i.size and (int(i.min()) < 0 or int(i.max()) >= dim):  # a negative index does not wrap
            raise IndexOutOfBound
    if n == 0:
        return np.zeros(shape, bool), np.zeros(shape, dm.NP[dt])
    return dm.build(shape, tuple(i.astype(np.int64) for i in idx), vals, dup_op or "second", dt)


def has_duplicates(indices, shape):
    idx = [np.asarray(i).astype(np.int64) for i in indices]
    if idx[0].size == 0:
        return False
    return np.unique(np.stack(idx), axis=1).shape[1] < idx[0].size


def check_pointer(indptr, n_indices, n_values):
    """the pointer check of the compressed import; returns Ap[last]"""
    p = np.asarray(indptr)
    if p.size < 1 or int(p[0]) != 0 or (np.diff(p.astype(object)) < 0).any() or int(p[-1]) > n_indices:
        raise InvalidValue
    last = int(p[-1])
    if not (n_values == 1 or n_values >= last):
        raise InvalidValue
    return last


def from_csx(shape, indptr, indices, values, dtype=None, by_col=False):
    """rows of a compressed input may be jumbled or hold duplicates (the last one is kept)"""
    shape = tuple(int(n) for n in shape)
    major, minor = (shape[1], shape[0]) if by_col else shape
    p = np.asarray(indptr)
    if p.size != major + 1:
        raise InvalidValue
    scalar = np.ndim(values) == 0
    last = check_pointer(p, np.asarray(indices).size, 1 if scalar else np.asarray(values).size)
    inner = np.asarray(indices)[:last]
    if scalar:
        vals = values
    else:  # one value for more than one index: every entry has it
        va = np.asarray(values)
        vals = va[0] if va.size == 1 and last > 1 else va[:last]
    outer = np.repeat(np.arange(major), np.diff(p.astype(np.int64)))
    A = from_coo((major, minor), (outer, inner), vals, None, value_type(values, dtype))
    return dm.transpose(A) if by_col else A


def path_of_coo(indices, shape):
    """stat_sparse_import_path of a COO import: 0 when the keys are strictly increasing"""
    idx = [np.asarray(i).astype(np.int64) for i in indices]
    if idx[0].size == 0:
        return 0
    flat = idx[0] if len(idx) == 1 else idx[0] * (1 << 32) + idx[1]
    return 0 if (np.diff(flat) > 0).all() else 1


def path_of_csx(indptr, indices):
    """0 when every row is strictly increasing, else 2"""
    p, j = np.asarray(indptr).astype(np.int64), np.asarray(indices).astype(np.int64)
    for a, b in zip(p[:-1], p[1:]):
        if (np.diff(j[a:b]) <= 0).any():
            return 2
    return 0


# ---------------------------------------------------------------------- export
def to_coo(A, index="INT64", dtype=None):
    """row-major sorted (rows, columns, values), or (indices, values) of a vector"""
    p, v = A
    idx = np.nonzero(p)
    vals = v[idx] if dtype is None else dm.cast(v[idx], dtype)
    return tuple(i.astype(INDEX[index]) for i in idx) + (vals,)


def to_csr(A, index="INT64", dtype=None):
    p, v = A
    r, c, vals = to_coo(A, index, dtype)
    indptr = np.concatenate([[0], np.cumsum(p.sum(axis=1))]).astype(INDEX[index])
    return indptr, c, vals


def to_csc(A, index="INT64", dtype=None):
    return to_csr(dm.transpose(A), index, dtype)


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[x.dtype.itemsize])


# ---------------------------------------------------------------------- the golden cases
def _dtype(x):
    return x["dtype"] if isinstance(x, dict) else x


def _fixture(G):
    f = G["fixture_A"]
    return from_coo((7, 7), (f["rows"], f["columns"]), np.asarray(f["values"]))


def _export(G, ex):
    A = _fixture(G)
    if ex["of"] == "A.T":
        A = dm.transpose(A)
    dtype = _dtype(ex["kwargs"].get("dtype"))
    return {"to_csr": to_csr, "to_csc": to_csc, "to_coo": to_coo}[ex["export"]](A, "INT64", dtype)


def golden_object(G, desc):
    """the model pair of a recorded object, with the reference's rules for what is not given: a
    dimension is the largest index + 1 and cannot be inferred from nothing; duplicates need dup_op"""
    if "fixture" in desc:
        A = _fixture(G)
        return (A[0], dm.cast(A[1], _dtype(desc["dup"]))) if "dup" in desc else A
    args = []
    for a in desc["args"]:
        args += list(_export(G, a["star"])) if isinstance(a, dict) and "star" in a else [a]
    kw = dict(desc["kwargs"])
    dtype = _dtype(kw.pop("dtype", None))
    if desc["how"] == "new":
        dims = [kw[k] for k in ("nrows", "ncols", "size") if k in kw] or args[1:]
        shape = tuple(dims)
        return np.zeros(shape, bool), np.zeros(shape, dm.NP[_dtype(args[0])])
    dup = kw.pop("dup_op", None)
    dup = None if dup is None else dup["op"].split(".")[1]
    if desc["how"] == "from_coo":
        *idx, values = args
        scalar = np.ndim(values) == 0
        if scalar and dup is not None:
            raise ValueError("dup_op must be None if values is a scalar")
        names = ("nrows", "ncols") if desc["kind"] == "Matrix" else ("size",)
        shape = []
        for i, name in zip(idx, names):
            if kw.get(name) is None and len(i) == 0:
                what = {"nrows": "row indices", "ncols": "column indices", "size": "indices"}[name]
                raise ValueError(f"No {what} provided. Unable to infer {name}.")
            shape.append(kw[name] if kw.get(name) is not None else int(np.max(i)) + 1)
        lens = [len(i) for i in idx] + ([] if scalar else [len(values)])
        if len(set(lens)) > 1:
            what = "`rows` and `columns` and `values`" if desc["kind"] == "Matrix" else "`indices` and `values`"
            raise ValueError(f"{what} lengths must match: " + ", ".join(str(n) for n in lens))
        values = values if scalar else np.asarray(values)
        if dup is None and not scalar and has_duplicates(idx, shape):
            from_coo(shape, idx, values)  # an index out of bounds comes first
            raise ValueError("Duplicate indices found, must provide `dup_op` BinaryOp")
        return from_coo(shape, idx, values, dup, value_type(values, dtype))
    by_col = desc["how"] == "from_csc"
    indptr, inner, values = args
    major = len(indptr) - 1
    given, other = ("ncols", "nrows") if by_col else ("nrows", "ncols")
    if kw.get(given) is not None and kw[given] != major:
        raise ValueError(f"{given} must be None or equal to len(indptr) - 1; expected {major}, got {kw[given]}")
    minor = kw[other] if kw.get(other) is not None else (int(np.max(inner)) + 1 if len(inner) else 0)
    shape = (minor, major) if by_col else (major, minor)
    values = values if np.ndim(values) == 0 else np.asarray(values)
    return from_csx(shape, indptr, inner, values, value_type(values, dtype), by_col)


def same_object(A, B, check_dtype):
    """isequal"""
    return A[0].shape == B[0].shape and np.array_equal(A[0], B[0]) and (not check_dtype or A[1].dtype == B[1].dtype) \
        and np.array_equal(A[1][A[0]], B[1][B[0]])
