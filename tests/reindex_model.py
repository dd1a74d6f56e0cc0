"""numpy model of diag, reshape and flatten on the repository's (present, values) pairs, written
from the rule of the C API (include/graphblas_amd.h), not from the kernels: a diagonal is np.diag of
the pattern and of the values, a reshape is ndarray.reshape in C or Fortran order, a flatten is a
reshape to one dimension.  Shapes too large to hold densely have a COO form, which is the rule's
own arithmetic: lin = i * ncols + j (row-major) or i + j * nrows (column-major)."""
import json
import os

import numpy as np

import dense_model as dm

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "diag_reshape_golden.json")
NP_ORDER = {"rowwise": "C", "columnwise": "F"}


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def cast(A, dtype):
    p, v = A
    return p, np.where(p, dm.cast(v, dtype), dm.NP[dtype](0)).astype(dm.NP[dtype])


def diag_matrix(v, k=0, dtype=None):
    """the (size + |k|)-square matrix with v on diagonal k"""
    p, x = v
    A = np.diag(p, k), np.diag(x, k)
    return A if dtype is None else cast(A, dtype)


def diag_size(nrows, ncols, k):
    return max(0, min(ncols - k, nrows)) if k >= 0 else max(0, min(nrows + k, ncols))


def diag_vector(A, k=0, dtype=None):
    """diagonal k of A: position p holds A(p + max(-k, 0), p + max(k, 0))"""
    p, x = A
    n = diag_size(p.shape[0], p.shape[1], k)
    if n == 0:  # np.diag of a matrix without rows or columns, or of a diagonal outside it
        w = np.zeros(0, bool), np.zeros(0, x.dtype)
    else:
        w = np.diag(p, k).copy(), np.diag(x, k).copy()
    assert w[0].shape == (n,)
    return w if dtype is None else cast(w, dtype)


def reshape(A, shape, order="rowwise"):
    p, x = A
    return p.reshape(shape, order=NP_ORDER[order]), x.reshape(shape, order=NP_ORDER[order])


def flatten(A, order="rowwise", dtype=None):
    w = reshape(A, (-1,), order)
    return w if dtype is None else cast(w, dtype)


# ---------------------------------------------------------------------- COO form
def linear(rows, cols, shape, order):
    rows, cols = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
    return rows * shape[1] + cols if order == "rowwise" else rows + cols * shape[0]


def reshape_coo(rows, cols, vals, shape, new_shape, order="rowwise"):
    """the tuples of the reshaped matrix, sorted by (row, column) as to_coo() gives them"""
    assert shape[0] * shape[1] == new_shape[0] * new_shape[1]
    lin = linear(rows, cols, shape, order)
    if order == "rowwise":
        r, c = np.divmod(lin, new_shape[1])
    else:
        c, r = np.divmod(lin, new_shape[0])
    at = np.lexsort((c, r))
    return r[at], c[at], np.asarray(vals)[at]


def flatten_coo(rows, cols, vals, shape, order="rowwise"):
    lin = linear(rows, cols, shape, order)
    at = np.argsort(lin, kind="stable")
    return lin[at], np.asarray(vals)[at]


# ---------------------------------------------------------------------- golden operands
def pair_of(shape, index, vals, dtype="INT64"):
    """(present, values) from index arrays (one per dimension) and values"""
    t = dm.NP[dtype]
    p, v = np.zeros(shape, bool), np.zeros(shape, t)
    index = tuple(np.asarray(i, np.int64) for i in index)
    p[index] = True
    v[index] = np.asarray(vals, t)
    return p, v


def golden_A(g, resize=None):
    a = g["A"]
    shape = (a["nrows"], a["ncols"]) if resize is None else tuple(resize)
    return pair_of(shape, (a["rows"], a["cols"]), a["vals"])


def golden_v(g):
    return pair_of((g["v"]["size"],), (g["v"]["idx"],), g["v"]["vals"])
