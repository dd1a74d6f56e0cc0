"""CPU checks of the sort surface: GxB_Matrix_sort / GxB_Vector_sort are exported, declared in
both headers and typed in _lib; ``A.ss.sort`` / ``v.ss.sort`` have the reference's signature
(core/ss/matrix.py:3991, core/ss/vector.py:1562); and the numpy model the GPU tests compare with
reproduces the reference's own test cases (tests/golden/sort_golden.json) and a set of
hand-worked ones.  No compute calls (no GPU here)."""
import ctypes
import inspect
import json
import os

import numpy as np
import pytest

import dense_model as dm
import sort_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["GxB_Matrix_sort", "GxB_Vector_sort"]


def golden():
    with open(os.path.join(ROOT, "tests", "golden", "sort_golden.json")) as f:
        return json.load(f)


def golden_matrix(g):
    a = g["A"]
    p = np.zeros((a["nrows"], a["ncols"]), bool)
    v = np.zeros(p.shape, dm.NP[a["dtype"]])
    p[a["rows"], a["cols"]] = True
    v[a["rows"], a["cols"]] = a["vals"]
    return p, v


def golden_vector(g):
    u = g["v"]
    p = np.zeros(u["size"], bool)
    v = np.zeros(u["size"], dm.NP[u["dtype"]])
    p[u["idx"]] = True
    v[u["idx"]] = u["vals"]
    return p, v


def dense(shape, idx, vals, dtype):
    p = np.zeros(shape, bool)
    v = np.zeros(shape, dtype)
    p[idx] = True
    v[idx] = vals
    return p, v


def test_entry_points_are_exported_and_declared():
    import graphblas_amd
    from graphblas_amd import _lib

    dll = ctypes.CDLL(graphblas_amd.LIB_PATH)
    missing = [n for n in ENTRY_POINTS if not hasattr(dll, n)]
    assert not missing, missing
    header = open(os.path.join(ROOT, "include", "graphblas_amd.h")).read()
    cdef = open(os.path.join(ROOT, "include", "graphblas_amd_cdef.h")).read()
    decls = ["GrB_Info GxB_Matrix_sort(GrB_Matrix C, GrB_Matrix P, GrB_BinaryOp op, const GrB_Matrix A, "
             "const GrB_Descriptor desc);",
             "GrB_Info GxB_Vector_sort(GrB_Vector w, GrB_Vector p, GrB_BinaryOp op, const GrB_Vector u, "
             "const GrB_Descriptor desc);"]
    for n, d in zip(ENTRY_POINTS, decls):
        assert d in header, n
        assert d in cdef, n
        assert _lib._SIGS[n] == [ctypes.c_void_p] * 5, n
        assert n in dir(_lib.lib)


def test_adapter_exposes_the_symbols():
    cdef = open(os.path.join(ROOT, "include", "graphblas_amd_cdef.h")).read()
    adapter = open(os.path.join(ROOT, "graph-python_amd", "suitesparse_graphblas_amd", "__init__.py")).read()
    assert "graphblas_amd_cdef.h" in adapter  # the adapter's cdef() is that header
    for n in ENTRY_POINTS:
        assert f"GrB_Info {n}(" in cdef


def test_front_end_signatures():
    import graphblas_amd as gb
    from graphblas_amd.ss import MatrixSS, VectorSS

    ps = inspect.signature(MatrixSS.sort).parameters
    assert list(ps) == ["self", "op", "order", "values", "permutation", "opts"]
    assert ps["op"].default is gb.binary.lt and ps["order"].default == "rowwise"
    assert ps["values"].default is True and ps["permutation"].default is True
    assert ps["values"].kind is inspect.Parameter.KEYWORD_ONLY and ps["permutation"].kind is inspect.Parameter.KEYWORD_ONLY
    assert ps["opts"].kind is inspect.Parameter.VAR_KEYWORD
    ps = inspect.signature(VectorSS.sort).parameters
    assert list(ps) == ["self", "op", "values", "permutation", "opts"]
    assert ps["op"].default is gb.binary.lt
    assert ps["values"].kind is inspect.Parameter.KEYWORD_ONLY and ps["opts"].kind is inspect.Parameter.VAR_KEYWORD


@pytest.mark.parametrize("case", golden()["matrix_cases"], ids=lambda c: c["source"])
def test_model_reproduces_the_golden_matrix_cases(case):
    A = golden_matrix(golden())
    (cp, cv), (pp, pv) = sm.sort_matrix(A, case["op"], columnwise=case["order"] == "columnwise")
    idx = (np.asarray(case["rows"]), np.asarray(case["cols"]))
    want = np.zeros(A[0].shape, bool)
    want[idx] = True
    assert np.array_equal(cp, want) and np.array_equal(pp, want)
    assert cv.dtype == np.int64 and pv.dtype == np.uint64
    assert np.array_equal(cv[idx], case["C"]) and np.array_equal(pv[idx], np.asarray(case["P"], np.uint64))


@pytest.mark.parametrize("case", golden()["vector_cases"], ids=lambda c: c["source"])
def test_model_reproduces_the_golden_vector_cases(case):
    u = golden_vector(golden())
    (wp, wv), (pp, pv) = sm.sort_vector(u, case["op"])
    want = np.zeros(u[0].shape, bool)
    want[case["idx"]] = True
    assert np.array_equal(wp, want) and np.array_equal(pp, want)
    assert np.array_equal(wv[case["idx"]], case["w"])
    if case["p"] is not None:
        assert np.array_equal(pv[case["idx"]], np.asarray(case["p"], np.uint64))


def test_model_signed_zeros_tie_by_index_and_keep_their_sign():
    # -0.0 and +0.0 interleaved by column, one negative and one positive value
    vals = np.array([0.0, -0.0, 1.5, -0.0, 0.0, -2.0])
    u = dense((8,), [0, 1, 2, 4, 5, 7], vals, np.float64)
    (wp, wv), (_, pv) = sm.sort_vector(u, "lt")
    assert np.array_equal(pv[:6], [7, 0, 1, 4, 5, 2]) and not wp[6:].any()
    assert np.array_equal(wv[:6], [-2.0, 0.0, -0.0, -0.0, 0.0, 1.5])
    assert np.array_equal(np.signbit(wv[:6]), [True, False, True, True, False, False])
    (_, wv), (_, pv) = sm.sort_vector(u, "gt")
    assert np.array_equal(pv[:6], [2, 0, 1, 4, 5, 7])
    assert np.array_equal(np.signbit(wv[:6]), [False, False, True, True, False, True])


def test_model_integer_extremes_under_gt():
    lo = np.iinfo(np.int64).min
    u = dense((5,), [0, 1, 2, 3, 4], [0, lo, -1, np.iinfo(np.int64).max, lo], np.int64)
    (_, wv), (_, pv) = sm.sort_vector(u, "gt")
    assert np.array_equal(pv, [3, 0, 2, 1, 4]) and wv[3] == lo and wv[4] == lo
    (_, wv), (_, pv) = sm.sort_vector(u, "lt")
    assert np.array_equal(pv, [1, 4, 2, 0, 3])
    big = np.array([2 ** 63 + 5, 7, 2 ** 64 - 1, 2 ** 63, 2 ** 63 + 5], np.uint64)
    u = dense((5,), [0, 1, 2, 3, 4], big, np.uint64)
    (_, wv), (_, pv) = sm.sort_vector(u, "gt")
    assert np.array_equal(pv, [2, 0, 4, 3, 1]) and wv[0] == np.uint64(2 ** 64 - 1)
    # the same bits compared as INT64 (GrB_GT_INT64 on a UINT64 vector): values above 2^63 wrap negative
    (_, wv), (_, pv) = sm.sort_vector(u, "gt", op_dtype="INT64")
    assert np.array_equal(pv, [1, 2, 0, 4, 3]) and wv.dtype == np.uint64 and wv[1] == np.uint64(2 ** 64 - 1)


def test_model_bool_iso_and_casts():
    A = dense((2, 5), ([0, 0, 0, 0, 1, 1], [0, 1, 3, 4, 2, 4]), [True, False, True, False, True, True], np.bool_)
    (cp, cv), (_, pv) = sm.sort_matrix(A, "lt")
    assert np.array_equal(pv[0, :4], [1, 4, 0, 3]) and np.array_equal(cv[0, :4], [False, False, True, True])
    assert np.array_equal(pv[1, :2], [2, 4]) and cp.sum() == 6
    (_, cv), (_, pv) = sm.sort_matrix(A, "gt")
    assert np.array_equal(pv[0, :4], [0, 3, 1, 4]) and np.array_equal(cv[0, :4], [True, True, False, False])
    # an iso input: every value equal, so P is the columns in order and C keeps the value
    I = dense((2, 6), ([0, 0, 0, 1], [5, 1, 3, 2]), 7, np.int16)
    for op in ("lt", "gt"):
        (cp, cv), (_, pv) = sm.sort_matrix(I, op)
        assert np.array_equal(pv[0, :3], [1, 3, 5]) and pv[1, 0] == 2 and (cv[cp] == 7).all()
    # columnwise keeps A's shape (3 x 2 here), entries moved to the top
    T = dense((3, 2), ([0, 2, 1, 2], [0, 0, 1, 1]), [5, 4, 1, 0], np.int32)
    (cp, cv), (_, pv) = sm.sort_matrix(T, "lt", columnwise=True)
    assert cp.shape == (3, 2) and np.array_equal(cp, [[True, True], [True, True], [False, False]])
    assert np.array_equal(cv[:2], [[4, 0], [5, 1]]) and np.array_equal(pv[:2], [[2, 2], [0, 1]])
    # the comparison type: INT8 values 100, -100 compared as UINT8 put -100 (156) last; C cast to INT32
    u = dense((3,), [0, 1, 2], [100, -100, 3], np.int8)
    (_, wv), (_, pv) = sm.sort_vector(u, "lt", op_dtype="UINT8", out_dtype="INT32")
    assert np.array_equal(pv, [2, 0, 1]) and wv.dtype == np.int32 and np.array_equal(wv, [3, 100, -100])
    # FP64 values compared as INT32 truncate: 1.7 and 1.2 tie, index order decides
    u = dense((3,), [0, 1, 2], [1.7, 1.2, 0.5], np.float64)
    (_, wv), (_, pv) = sm.sort_vector(u, "lt", op_dtype="INT32")
    assert np.array_equal(pv, [2, 0, 1]) and np.array_equal(wv, [0.5, 1.7, 1.2])
