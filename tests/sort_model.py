"""A numpy model of GxB_Matrix_sort / GxB_Vector_sort on dense_model's ``(present, values)``
pairs, written from the rules in include/graphblas_amd.h, not from the kernels.

Every row (column, if columnwise) is ordered by its values cast to the operator's type,
ascending for ``lt`` and descending for ``gt``; equal values (``-0.0 == +0.0``) keep ascending
original index; the entries move to positions 0 .. len-1.  C holds the values (A's own, cast to
C's type), P the indices they came from.  One whole-matrix ``lexsort`` does it: the key of an
entry is the rank of its value among the distinct values (``np.unique``), negated for ``gt``,
so that no Python loop runs per row.  NaNs: ``np.unique`` puts them last (first under ``gt``);
the library leaves their place unspecified and the tests compare NaN inputs another way.
"""
import numpy as np

import dense_model as dm


def _ranks(x, desc):
    _, inv = np.unique(x, return_inverse=True)
    inv = np.asarray(inv, np.int64).reshape(-1)
    return -inv if desc else inv


def sort_matrix(A, op="lt", op_dtype=None, columnwise=False, out_dtype=None):
    """(C, P) of A's shape; P's values are uint64"""
    p, v = A
    if columnwise:
        C, P = sort_matrix((p.T, v.T), op, op_dtype, False, out_dtype)
        return (C[0].T.copy(), C[1].T.copy()), (P[0].T.copy(), P[1].T.copy())
    assert op in ("lt", "gt")
    dt = dm.name_of(v.dtype)
    rows, cols = np.nonzero(p)  # row-major: ascending column inside a row
    vals = v[rows, cols]
    key = _ranks(dm.cast(vals, op_dtype or dt), op == "gt")
    order = np.lexsort((cols, key, rows))
    rs, cs, vs = rows[order], cols[order], vals[order]
    start = np.zeros(p.shape[0] + 1, np.int64)
    np.cumsum(np.bincount(rows, minlength=p.shape[0]), out=start[1:])
    rank = np.arange(rs.size, dtype=np.int64) - start[rs]
    out = out_dtype or dt
    Cp = np.zeros(p.shape, bool)
    Cp[rs, rank] = True
    Cv = np.zeros(p.shape, dm.NP[out])
    Cv[rs, rank] = dm.cast(vs, out)
    Pv = np.zeros(p.shape, np.uint64)
    Pv[rs, rank] = cs.astype(np.uint64)
    return (Cp, Cv), (Cp.copy(), Pv)


def sort_vector(u, op="lt", op_dtype=None, out_dtype=None):
    """(w, p) of u's size"""
    p, v = u
    C, P = sort_matrix((p[None, :], v[None, :]), op, op_dtype, False, out_dtype)
    return (C[0][0], C[1][0]), (P[0][0], P[1][0])
