"""A numpy model of GxB_Matrix_scan / GxB_Vector_scan on dense_model's ``(present, values)``
pairs, written from the rule in include/graphblas_amd.h, not from the kernels.

The result at position p (0-based, among a row's stored entries) folds the first p + 1 values.
p + 1 is written in binary; every set bit, from the highest down, stands for the next aligned
block of 2^k entries, folded as a balanced pairwise tree (left half (+) right half); the blocks
are combined left to right, largest first.  With B(k, n) the tree of the 2^k entries that end
at position n - 1 and P(n) the result of the first n values, that is

    P(n) = B(k, n)                   if n = 2^k
    P(n) = P(n - 2^k) (+) B(k, n)    otherwise, k the lowest set bit of n

which is an up-sweep (the trees, level by level) and a down-sweep (the positions whose lowest
set bit is k, from the highest k down) over the rows' entries compacted to the left.  Every
level is one vectorised call over all rows; what lies past a row's end never reaches a real
position, since a level only ever reads to the left.  All arithmetic is in the monoid's type.
"""
import numpy as np

import dense_model as dm

IDEMPOTENT = ("min", "max", "any", "lor", "land", "bor", "band")


def scan_compact(x, monoid, dtype):
    """the inclusive scans of the rows of the 2-d array x (already of the monoid's type), every
    row taken as if it were full: the caller reads the positions below its row's length"""
    x = np.array(x, dm.NP[dtype])
    n = x.shape[1]
    if monoid == "any" or n < 2:
        return x
    pos = np.arange(1, n + 1)  # 1-based
    levels = int(n).bit_length()
    for k in range(levels):  # up-sweep: B(k + 1, n) = B(k, n - 2^k) (+) B(k, n)
        at = pos[pos % (2 << k) == 0] - 1
        if at.size:
            x[:, at] = dm.binop(monoid, dtype, x[:, at - (1 << k)], x[:, at])
    for k in range(levels - 1, -1, -1):  # down-sweep: P(n) = P(n - 2^k) (+) B(k, n)
        at = pos[(pos % (2 << k) == (1 << k)) & (pos > (1 << k))] - 1
        if at.size:
            x[:, at] = dm.binop(monoid, dtype, x[:, at - (1 << k)], x[:, at])
    return x


def scan_matrix(A, monoid, dtype, columnwise=False):
    """(present, values of `dtype`) of A's shape: the scan of every row (column)"""
    p, v = A
    if columnwise:
        cp, cv = scan_matrix((np.ascontiguousarray(p.T), np.ascontiguousarray(v.T)), monoid, dtype)
        return np.ascontiguousarray(cp.T), np.ascontiguousarray(cv.T)
    t = dm.NP[dtype]
    out = np.zeros(p.shape, t)
    rows, cols = np.nonzero(p)  # row-major: ascending column inside a row
    if rows.size:
        start = np.zeros(p.shape[0] + 1, np.int64)
        np.cumsum(np.bincount(rows, minlength=p.shape[0]), out=start[1:])
        rank = np.arange(rows.size, dtype=np.int64) - start[rows]
        x = np.zeros((p.shape[0], int(rank.max()) + 1), t)
        x[rows, rank] = dm.cast(v[rows, cols], dtype)
        out[rows, cols] = scan_compact(x, monoid, dtype)[rows, rank]
    return p.copy(), out


def scan_vector(u, monoid, dtype):
    p, v = u
    cp, cv = scan_matrix((p[None, :], v[None, :]), monoid, dtype)
    return cp[0], cv[0]
