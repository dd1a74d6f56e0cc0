"""The numpy model of eWiseUnion on (present, values) pairs, written from the rule of the C API
(include/graphblas_amd.h), not from the kernel: T has the structure of A union B and the type of
the operator's result; both present: op(a, b); only in A: op(a, beta); only in B: op(alpha, b).
A, B, alpha and beta are all cast to the operator's input type first."""
import json
import os

import numpy as np

import dense_model as dm

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ewise_union_golden.json")


def scalar_as(value, dtype):
    """one value (a numpy or Python scalar of any type) cast to `dtype` by the library's rules"""
    return dm.cast(np.atleast_1d(np.asarray(value)), dtype)[0]


def ewise_union(op, dtype, A, alpha, B, beta):
    """T = A union B under op[dtype] with alpha standing in for a missing A, beta for a missing B"""
    (ap, av), (bp, bv) = A, B
    assert ap.shape == bp.shape
    zt = dm.binop_return_dtype(op, dtype)
    x = np.where(ap, dm.cast(av, dtype), scalar_as(alpha, dtype))
    y = np.where(bp, dm.cast(bv, dtype), scalar_as(beta, dtype))
    z = dm.cast(dm.binop(op, dtype, x, y), zt)
    present = ap | bp
    return present, np.where(present, z, dm.NP[zt](0))


def case_counts(A, B):
    """(both, A only, B only): what the library's stat_union_* counters hold after the call"""
    ap, bp = A[0], B[0]
    return int((ap & bp).sum()), int((ap & ~bp).sum()), int((bp & ~ap).sum())


def golden_cases():
    with open(GOLDEN) as f:
        return json.load(f)["cases"]


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


def golden_default(d):
    return dm.NP[d["dtype"]](d["value"])
