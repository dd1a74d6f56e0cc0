"""CPU checks of the scan surface: GxB_Matrix_scan / GxB_Vector_scan are exported, declared in both
headers and typed in _lib; ``ss.scan`` has the reference's argument order (core/ss/matrix.py:3701,
core/ss/vector.py:1365) and its TypeError for a BinaryOp without a monoid; and the numpy model the
GPU tests compare with (tests/scan_model.py) is a prefix scan: exactly numpy's accumulate where
the arithmetic is exact, and within the first-order bound of any summation order for float plus
and times.  No compute calls (no GPU here)."""
import ctypes
import inspect
import math
import os
from fractions import Fraction

import numpy as np
import pytest

import dense_model as dm
import scan_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = ctypes.c_void_p
ENTRY_POINTS = {
    "GxB_Matrix_scan": "GrB_Info GxB_Matrix_scan(GrB_Matrix C, const GrB_Monoid op, const GrB_Matrix A, "
                       "const GrB_Descriptor desc);",
    "GxB_Vector_scan": "GrB_Info GxB_Vector_scan(GrB_Vector w, const GrB_Monoid op, const GrB_Vector u, "
                       "const GrB_Descriptor desc);",
}
LENGTHS = list(range(301)) + [4095, 4096, 4097]
NCOLS = 4200


def test_entry_points_are_exported_and_declared():
    import graphblas_amd
    from graphblas_amd import _lib

    dll = ctypes.CDLL(graphblas_amd.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "graphblas_amd.h")).read()
    cdef = open(os.path.join(ROOT, "include", "graphblas_amd_cdef.h")).read()
    for n, decl in ENTRY_POINTS.items():
        getattr(dll, n)  # AttributeError: not exported
        assert decl in header, n
        assert decl in cdef, n
        assert _lib._SIGS[n] == [P] * 4, n
        assert n in dir(_lib.lib)
    assert "balanced pairwise tree" in header  # the association order is part of the contract
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "GxB_Matrix_scan" in integration and "GxB_Vector_scan" in integration


def test_front_end_signatures_and_type_error():
    import graphblas_amd as gb
    from graphblas_amd import ss
    from graphblas_amd.ss import MatrixSS, VectorSS

    KW = inspect.Parameter.KEYWORD_ONLY
    ps = inspect.signature(MatrixSS.scan).parameters
    assert list(ps) == ["self", "op", "order", "name"]
    assert ps["order"].default == "rowwise" and ps["name"].kind is KW and ps["op"].default is None
    ps = inspect.signature(VectorSS.scan).parameters
    assert list(ps) == ["self", "op", "name"] and ps["name"].kind is KW and ps["op"].default is None
    ps = inspect.signature(ss.prefix_scan).parameters  # the recipe stays public
    assert list(ps) == ["A", "op", "name"] and ps["name"].kind is KW
    # the operator check comes before any library call: no GPU is needed to see it
    A, v = gb.Matrix.__new__(gb.Matrix), gb.Vector.__new__(gb.Vector)
    for obj in (A, v):
        obj.dtype = gb.dtypes.INT64
        with pytest.raises(TypeError, match="Bad type for argument `op`"):
            obj.ss.scan(op=gb.binary.first)
    with pytest.raises(ValueError, match="Bad value for order"):
        A.ss.scan(gb.monoid.plus, "diagonal")


# ---------------------------------------------------------------------- the model against itself
def ragged(dt, seed):
    rng = np.random.default_rng(seed)
    p = np.zeros((len(LENGTHS), NCOLS), bool)
    for i, n in enumerate(LENGTHS):
        p[i, rng.choice(NCOLS, n, replace=False)] = True
    if dt == "BOOL":
        v = rng.random(p.shape) < 0.5
    else:
        v = rng.integers(dm.tmin(dt), dm.tmax(dt), p.shape, dtype=dm.NP[dt], endpoint=True)
    return p, np.where(p, v, dm.NP[dt](0))


def bxnor_accumulate(x):
    """~(a ^ b) = a ^ b ^ ones: a prefix of n values carries n - 1 complements"""
    r = np.bitwise_xor.accumulate(x)
    odd = (np.arange(x.size) & 1).astype(bool)
    return np.where(odd, ~r, r)


def _add(x):
    return np.add.accumulate(x, dtype=x.dtype)  # in the type itself: integers wrap


def _mul(x):
    return np.multiply.accumulate(x, dtype=x.dtype)


EXACT = {
    "INT64": {"plus": _add, "times": _mul, "min": np.minimum.accumulate,
              "max": np.maximum.accumulate},
    "UINT8": {"plus": _add, "times": _mul, "min": np.minimum.accumulate,
              "max": np.maximum.accumulate, "bor": np.bitwise_or.accumulate, "band": np.bitwise_and.accumulate,
              "bxor": np.bitwise_xor.accumulate, "bxnor": bxnor_accumulate},
    "BOOL": {"plus": np.logical_or.accumulate, "times": np.logical_and.accumulate, "min": np.logical_and.accumulate,
             "max": np.logical_or.accumulate, "lor": np.logical_or.accumulate, "land": np.logical_and.accumulate,
             "lxor": np.logical_xor.accumulate, "lxnor": lambda x: ~np.logical_xor.accumulate(~x)},
}


@pytest.mark.parametrize("dt,monoid", [(dt, m) for dt in EXACT for m in EXACT[dt]])
def test_model_is_numpys_accumulate_where_exact(dt, monoid):
    A = ragged(dt, 11)
    for columnwise in (False, True):
        M = (np.ascontiguousarray(A[0].T), np.ascontiguousarray(A[1].T)) if columnwise else A
        p, v = sm.scan_matrix(M, monoid, dt, columnwise=columnwise)
        if columnwise:
            p, v = p.T, v.T
        assert v.dtype == dm.NP[dt] and np.array_equal(p, A[0])
        assert not v[~p].any()
        for i, n in enumerate(LENGTHS):
            x = A[1][i][A[0][i]]
            with np.errstate(over="ignore"):
                want = EXACT[dt][monoid](x) if n else x
            assert np.array_equal(v[i][p[i]], want), (dt, monoid, n, columnwise)
        if columnwise:
            break  # the transpose once is enough
    # ANY: the values themselves
    p, v = sm.scan_matrix(A, "any", dt)
    assert np.array_equal(v, A[1])
    # a vector is the 1 x n matrix
    u = (A[0][-1], A[1][-1])
    wp, wv = sm.scan_vector(u, monoid, dt)
    p, v = sm.scan_matrix(A, monoid, dt)
    assert np.array_equal(wp, p[-1]) and np.array_equal(wv, v[-1])


@pytest.mark.parametrize("dt,u", [("FP64", 2.0 ** -53), ("FP32", 2.0 ** -24)])
def test_model_float_plus_and_times_within_the_first_order_bound(dt, u):
    """|model - exact| <= (n - 1) u sum|x| for plus (n the prefix length; the first-order bound
    that holds for any summation order), and <= (n - 1) u |exact| for times on values in [0.5, 2]"""
    t = dm.NP[dt]
    rng = np.random.default_rng(23)
    n = 4097
    check_at = [k for k in LENGTHS if k >= 1]
    x = (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, n)).astype(t)
    got = sm.scan_compact(x[None, :], "plus", dt)[0]
    assert got.dtype == t
    xs = [float(a) for a in x]
    for k in check_at:
        exact = math.fsum(xs[:k])
        bound = (k - 1) * u * math.fsum(abs(a) for a in xs[:k])
        assert abs(float(got[k - 1]) - exact) <= bound, (dt, "plus", k, float(got[k - 1]), exact, bound)
    y = (2.0 ** rng.uniform(-1, 1, n)).astype(t)
    assert y.min() >= 0.5 and y.max() <= 2
    got = sm.scan_compact(y[None, :], "times", dt)[0]
    exact, want = Fraction(1), {}
    for k in range(1, n + 1):
        exact *= Fraction(float(y[k - 1]))
        if k in check_at:
            want[k] = exact
    for k in check_at:
        assert np.isfinite(got[k - 1]) and got[k - 1] > 0
        err = abs(Fraction(float(got[k - 1])) - want[k])
        assert err <= (k - 1) * Fraction(u) * want[k], (dt, "times", k)


def test_model_order_is_the_documented_one():
    """position 5 of a row: ((x0 + x1) + (x2 + x3)) + (x4 + x5), and position 6 adds x6 last"""
    x = np.array([1e16, 1.0, -1e16, 1.0, 3.0, 1e-3, 7.0])
    got = sm.scan_compact(x[None, :], "plus", "FP64")[0]
    assert got[5] == ((x[0] + x[1]) + (x[2] + x[3])) + (x[4] + x[5])
    assert got[6] == (((x[0] + x[1]) + (x[2] + x[3])) + (x[4] + x[5])) + x[6]
    assert got[2] == (x[0] + x[1]) + x[2] and got[3] == (x[0] + x[1]) + (x[2] + x[3])
    assert got[5] != np.add.accumulate(x)[5]  # and that is not the sequential order
