"""CPU checks of the dense import / export surface: the four entry points are exported, declared
with their exact signatures in both headers, typed in _lib and named in INTEGRATION.md; the numpy
model the GPU tests compare with (tests/dense_io_model.py) reproduces the reference's own cases
(tests/golden/dense_io_golden.json); the front end's argument errors are raised before any library
call (reference core/matrix.py:1486-1496, core/vector.py:924-932); and the grid-sweep suite's scan
of csrc/ still finds the call sites it has cases for.  No compute calls: objects are stubs without
handles."""
import ctypes
import os
import re

import numpy as np
import pytest

import dense_io_model as dio
import dense_model as dm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = {
    "GxB_Matrix_import_dense": "GrB_Matrix *A, GrB_Type type, GrB_Index nrows, GrB_Index ncols, const void *X, "
                               "const int8_t *Ab, const GrB_Scalar missing, bool by_col, bool on_device",
    "GxB_Vector_import_dense": "GrB_Vector *v, GrB_Type type, GrB_Index n, const void *X, const int8_t *Ab, "
                               "const GrB_Scalar missing, bool on_device",
    "GxB_Matrix_export_dense": "void *X, int8_t *Ab, const GrB_Matrix A, const GrB_Scalar fill, bool by_col, "
                               "bool on_device",
    "GxB_Vector_export_dense": "void *X, int8_t *Ab, const GrB_Vector v, const GrB_Scalar fill, bool on_device",
}
G = dio.golden()
EXC = {"TypeError": TypeError, "ValueError": ValueError}


def ident(case):
    return case["src"]


# ---------------------------------------------------------------------- the C ABI
def test_entry_points_are_exported_and_declared():
    import graphblas_amd
    from graphblas_amd import _lib

    dll = ctypes.CDLL(graphblas_amd.LIB_PATH)
    for path in ("graphblas_amd.h", "graphblas_amd_cdef.h"):
        text = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", path)).read())
        for name, args in ENTRY_POINTS.items():
            assert f"GrB_Info {name}({args});" in text, (path, name)
    P, I, B = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_bool
    sigs = {"GxB_Matrix_import_dense": [P, P, I, I, P, P, P, B, B], "GxB_Vector_import_dense": [P, P, I, P, P, P, B],
            "GxB_Matrix_export_dense": [P, P, P, P, B, B], "GxB_Vector_export_dense": [P, P, P, P, B]}
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ENTRY_POINTS:
        assert hasattr(dll, name), name
        assert _lib._SIGS[name] == sigs[name], name
        assert name in dir(_lib.lib)
        assert name in text, name


def test_the_grid_sweep_scan_is_unchanged():
    """every new launch takes its grid from chunk_grid() or runs inside bitmap_csr: the sweep
    suite's cases clamp both, and its scan finds the call sites it found before"""
    import test_grid_sweeps_gpu as sweeps

    assert len(sweeps.grid_sites()) == 148
    sweeps.test_not_reached_table_matches_the_sources()


# ---------------------------------------------------------------------- the model
@pytest.mark.parametrize("case", [c for c in G if c["check"] == "isequal"], ids=ident)
def test_model_import_reproduces_the_golden_cases(case):
    left, right = dio.golden_object(case["left"]), dio.golden_object(case["right"])
    assert dio.same_object(left, right)


@pytest.mark.parametrize("case", [c for c in G if c["check"] == "to_dense"], ids=ident)
def test_model_export_reproduces_the_golden_cases(case):
    A = dio.golden_object(case["of"])
    if case["T"]:
        A = dm.transpose(A)
    fill, dtype = dio.golden_call(case)
    got, _ = dio.export_dense(A, fill, dtype)
    want = np.asarray(case["expect"])
    assert got.shape == want.shape and np.array_equal(got, want)
    assert got.dtype.kind == want.dtype.kind, (got.dtype, want.dtype)


def test_model_refuses_a_missing_fill_as_the_golden_cases_do():
    for case in G:
        if case["check"] == "raises" and case["method"] == "to_dense" and not case["args"]:
            with pytest.raises(EXC[case["raises"]], match=case["match"]):
                dio.export_dense(dio.golden_object(case["of"]))


def test_model_hand_worked_cases():
    nan = np.nan
    X = np.array([0.0, -0.0, nan, 1.5])
    assert dio.import_dense(X, 0.0)[0].tolist() == [False, False, True, True]  # both zeros go
    assert dio.import_dense(X, nan)[0].tolist() == [True] * 4                  # NaN != NaN: nothing goes
    assert dio.import_dense(X, 1)[0].tolist() == [True, True, True, True]      # INT64 1 as FP64 1.0
    assert dio.import_dense(X, 1.5, bitmap=[2, 0, -1, 1])[0].tolist() == [True, False, True, False]
    p, v = dio.import_dense(X)
    assert np.array_equal(dio.bits(v), dio.bits(X)) and p.all()
    # an INT64 missing value given to an INT8 array: 300 wraps to 44
    assert dio.import_dense(np.array([44, 3], np.int8), 300)[0].tolist() == [False, True]
    assert dio.import_dense(np.array([True, False]), False)[0].tolist() == [True, False]
    A = (np.array([[True, False], [True, True]]), np.array([[7, 0], [-3, 4]], np.int64))
    out, ab = dio.export_dense(A, 6.5)
    assert out.dtype == np.float64 and out.tolist() == [[7, 6.5], [-3, 4]] and ab.tolist() == [[1, 0], [1, 1]]
    assert dio.export_dense(A, 6.5, "INT64")[0].tolist() == [[7, 6], [-3, 4]]
    assert dio.export_dense(A, 6.5, upcast=False)[0].dtype == np.int64
    assert dio.export_dense(A, bitmap=True)[0].tolist() == [[7, 0], [-3, 4]]
    with pytest.raises(TypeError, match="fill_value must be given"):
        dio.export_dense(A)
    full = (np.ones(2, bool), np.array([1, 2], np.int8))
    assert dio.export_dense(full)[0].dtype == np.int8
    assert dio.export_dense(full, 4.5)[0].dtype == np.int8  # the fill of a full object is never used


# ---------------------------------------------------------------------- the front end, before any call
def stub(kind, shape, transposed=False):
    """a Matrix, its transpose or a Vector without a handle"""
    import graphblas_amd as gb

    if kind == "Vector":
        v = gb.Vector.__new__(gb.Vector)
        v.dtype, v.name, v._size, v._h = gb.dtypes.INT64, "v", shape[0], None
        return v
    A = gb.Matrix.__new__(gb.Matrix)
    A.dtype, A.name, A._nrows, A._ncols, A._h = gb.dtypes.INT64, "A", shape[0], shape[1], None
    return A.T if transposed else A


def argument(x):
    if isinstance(x, dict) and "object" in x:
        return object()
    if isinstance(x, dict) and "type" in x:
        return {"int": int, "float": float}[x["type"]]
    return x


# the cases the front end decides from its arguments alone; a missing fill is known only once the
# object's nvals is, and is tested on the device
ARGUMENT_ERRORS = [c for c in G if c["check"] == "raises" and (c["method"] == "from_dense" or c["args"])]


@pytest.mark.parametrize("case", ARGUMENT_ERRORS, ids=ident)
def test_golden_argument_errors(case):
    import graphblas_amd as gb

    args = [argument(a) for a in case["args"]]
    kwargs = {k: argument(v) for k, v in case["kwargs"].items()}
    cls = getattr(gb, case["kind"])
    with pytest.raises(EXC[case["raises"]], match=case["match"]):
        if case["method"] == "from_dense":
            cls.from_dense(*args, **kwargs)
        else:
            getattr(stub(case["kind"], dio.golden_object(case["of"])[0].shape), case["method"])(*args, **kwargs)


def test_every_golden_error_case_is_run_somewhere():
    rest = [c for c in G if c["check"] == "raises" and c not in ARGUMENT_ERRORS]
    assert [c["match"] for c in rest] == ["fill_value must be given"] * len(rest) and len(rest) == 2


def test_argument_errors_of_the_methods():
    import graphblas_amd as gb

    A, At, v = stub("Matrix", (2, 3)), stub("Matrix", (2, 3), True), stub("Vector", (4,))
    for cls, bad in ((gb.Matrix, 1), (gb.Matrix, np.float64(2)), (gb.Vector, 1), (gb.Vector, np.array(3))):
        with pytest.raises(TypeError, match=f"use `{cls.__name__}.from_scalar`"):
            cls.from_dense(bad)
    with pytest.raises(ValueError, match="A 2d array or scalar is required to create a dense Matrix"):
        gb.Matrix.from_dense(np.arange(3))
    with pytest.raises(ValueError, match="values array must be 2d to create dense Matrix with dtype INT64"):
        gb.Matrix.from_dense(np.zeros((2, 2, 2), np.int64))
    with pytest.raises(ValueError, match="values array must be 1d to create dense Vector with dtype FP64"):
        gb.Vector.from_dense(np.zeros((2, 2)))
    with pytest.raises(ValueError, match="does not match the values' shape"):
        gb.Matrix.from_dense(np.zeros((2, 3)), bitmap=np.ones((3, 2), bool))
    with pytest.raises(TypeError, match="must be bool, int8 or uint8"):
        gb.Vector.from_dense(np.zeros(3), bitmap=np.ones(3))
    with pytest.raises(TypeError, match="Bad type for keyword argument `missing_value`"):
        gb.Vector.from_dense(np.zeros(3), object())
    for x in (A, At, v):
        shape = x.shape
        with pytest.raises(TypeError, match="Bad type for keyword argument `fill_value` in to_dense"):
            x.to_dense([1, 2], out=np.zeros(shape, np.int64))
        with pytest.raises(ValueError, match="`out` of shape"):
            x.to_dense(0, out=np.zeros(shape + (1,), np.int64))
        with pytest.raises(TypeError, match="conflicts with the dtype of `out`"):
            x.to_dense(0, dtype=float, out=np.zeros(shape, np.int64))
        with pytest.raises(ValueError, match="`out` must be C- or F-contiguous"):
            x.to_dense(0, out=np.zeros(tuple(2 * n for n in shape), np.int64)[tuple(slice(None, None, 2) for _ in shape)])
        with pytest.raises(TypeError, match="Bad type for argument `out`"):
            x.to_dense(0, out=[[0] * 3] * 2)
        with pytest.raises(ValueError, match="`bitmap` of shape"):
            x.to_dense(0, bitmap=np.zeros(shape + (2,), np.int8))
        with pytest.raises(TypeError, match="`bitmap` must be bool, int8 or uint8"):
            x.to_dense(0, bitmap=np.zeros(shape, np.int32))
    with pytest.raises(ValueError, match="`bitmap` must be in the same order as `out`"):
        A.to_dense(0, out=np.zeros((2, 3), np.int64), bitmap=np.zeros((2, 3), np.int8, order="F"))


def test_order_detection():
    from graphblas_amd import dense

    f = dense._strides_order
    assert f((2, 3), (24, 8), 8) == "C" and f((2, 3), (8, 16), 8) == "F" and f((2, 3), (48, 16), 8) is None
    assert f((2, 3), None, 8) == "C" and f((0, 5), (0, 0), 8) == "C" and f((1, 5), (8, 8), 8) == "C"
    assert f((5, 1), (8, 8), 8) == "C" and f((4,), (4,), 4) == "C" and f((4,), (8,), 4) is None
    a = np.zeros((3, 4), np.int16)
    assert dense._Array(a, "x").order == "C" and dense._Array(a.T, "x").order == "F"
    assert dense._Array(np.asfortranarray(a), "x").order == "F"
