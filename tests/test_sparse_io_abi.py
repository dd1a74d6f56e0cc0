"""CPU checks of the sparse import / export surface: the four entry points are exported, declared
with their exact signatures in both headers, typed in _lib and named in INTEGRATION.md; the numpy
model the GPU tests compare with (tests/sparse_io_model.py) reproduces the reference's own cases
(tests/golden/sparse_io_golden.json); the front end raises every argument error of a device call
before any library call (the device arrays are stubs with a made-up address, and `call` fails when
reached); and the grid-sweep suite's scan of csrc/ still finds the call sites it has cases for."""
import ctypes
import os
import re

import numpy as np
import pytest

import sparse_io_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = {
    "GxB_Matrix_import_sparse": "GrB_Matrix *A, GrB_Type type, GrB_Index nrows, GrB_Index ncols, const void *Ap, "
                                "const void *Ai, const void *Ax, GrB_Type index_type, GrB_Type value_type, "
                                "GrB_Index Ap_len, GrB_Index Ai_len, GrB_Index Ax_len, GrB_Format format, "
                                "const GrB_BinaryOp dup, bool on_device",
    "GxB_Vector_import_sparse": "GrB_Vector *v, GrB_Type type, GrB_Index n, const void *Ai, const void *Ax, "
                                "GrB_Type index_type, GrB_Type value_type, GrB_Index Ai_len, GrB_Index Ax_len, "
                                "const GrB_BinaryOp dup, bool on_device",
    "GxB_Matrix_export_sparse": "void *Ap, void *Ai, void *Ax, GrB_Type index_type, GrB_Type value_type, "
                                "GrB_Index *Ap_len, GrB_Index *Ai_len, GrB_Index *Ax_len, GrB_Format format, "
                                "const GrB_Matrix A, bool on_device",
    "GxB_Vector_export_sparse": "void *Ai, void *Ax, GrB_Type index_type, GrB_Type value_type, GrB_Index *Ai_len, "
                                "GrB_Index *Ax_len, const GrB_Vector v, bool on_device",
}
G = sm.golden()
CASES = G["cases"]
EXC = {"ValueError": ValueError, "IndexOutOfBound": sm.IndexOutOfBound, "InvalidValue": sm.InvalidValue}


def ident(case):
    return case["src"].split("/")[-1]


# ---------------------------------------------------------------------- the C ABI
def test_entry_points_are_exported_and_declared():
    import graphblas_amd
    from graphblas_amd import _lib

    dll = ctypes.CDLL(graphblas_amd.LIB_PATH)
    for path in ("graphblas_amd.h", "graphblas_amd_cdef.h"):
        text = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", path)).read())
        for name, args in ENTRY_POINTS.items():
            assert f"GrB_Info {name}({args});" in text, (path, name)
    P, I, E, B = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_bool
    sigs = {"GxB_Matrix_import_sparse": [P, P, I, I, P, P, P, P, P, I, I, I, E, P, B],
            "GxB_Vector_import_sparse": [P, P, I, P, P, P, P, I, I, P, B],
            "GxB_Matrix_export_sparse": [P, P, P, P, P, P, P, P, E, P, B],
            "GxB_Vector_export_sparse": [P, P, P, P, P, P, P, B]}
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ENTRY_POINTS:
        assert hasattr(dll, name), name
        assert _lib._SIGS[name] == sigs[name], name
        assert name in dir(_lib.lib)
        assert name in text, name


def test_the_grid_sweep_scan_is_unchanged():
    """every new launch takes its grid from gb_sort_grid, and the build's launches stay in
    gb_object.hip: the sweep suite's scan finds the call sites it found before"""
    import test_grid_sweeps_gpu as sweeps

    assert len(sweeps.grid_sites()) == 148
    sweeps.test_not_reached_table_matches_the_sources()
    with open(os.path.join(ROOT, "graph-python_amd", "csrc", "gb_sparse_io.hip")) as f:
        assert not re.search(r"\bgb_grid\(", f.read())


# ---------------------------------------------------------------------- the model
@pytest.mark.parametrize("case", [c for c in CASES if c["check"] == "attribute"], ids=ident)
def test_model_reproduces_the_golden_attributes(case):
    p, v = sm.golden_object(G, case["of"])
    attr, want = case["attribute"], case["expect"]
    got = {"nrows": lambda: p.shape[0], "ncols": lambda: p.shape[1], "size": lambda: p.shape[0],
           "nvals": lambda: int(p.sum()), "dtype": lambda: sm.dm.name_of(v.dtype)}[attr]()
    assert got == want


@pytest.mark.parametrize("case", [c for c in CASES if c["check"] == "element"], ids=ident)
def test_model_reproduces_the_golden_elements(case):
    p, v = sm.golden_object(G, case["of"])
    assert p[tuple(case["index"])] and v[tuple(case["index"])] == case["expect"]


@pytest.mark.parametrize("case", [c for c in CASES if c["check"] == "isequal"], ids=ident)
def test_model_reproduces_the_golden_equalities(case):
    left, right = sm.golden_object(G, case["left"]), sm.golden_object(G, case["right"])
    assert sm.same_object(left, right, case["check_dtype"])


@pytest.mark.parametrize("case", [c for c in CASES if c["check"] == "raises"], ids=ident)
def test_model_refuses_what_the_golden_cases_refuse(case):
    with pytest.raises(EXC[case["raises"]], match=case["match"]):
        sm.golden_object(G, case["call"])


def test_golden_file_holds_the_cases_the_suite_needs():
    hows = {(c.get("call") or c.get("right") or c.get("of") or {}).get("how") for c in CASES}
    assert {"from_coo", "from_csr", "from_csc"} <= hows
    assert any(c["check"] == "isequal" and c["right"].get("args") == [[0, 1, 2, 2], [1, 0], [20, 10]] for c in CASES)
    assert sorted(c["raises"] for c in CASES if c["test"] == "test_to_csr_from_csc" and c["check"] == "raises") == \
        ["InvalidValue", "ValueError", "ValueError"]
    assert G["fixture_A"]["rows"] == [3, 0, 3, 5, 6, 0, 6, 1, 6, 2, 4, 1]


def test_model_hand_worked_cases():
    # duplicates fold in input order; without an operator the last one is kept
    p, v = sm.from_coo((2, 3), ([1, 0, 1, 1], [2, 0, 2, 2]), np.array([1.5, 2.0, 4.0, 8.0], np.float32), "plus")
    assert p.tolist() == [[True, False, False], [False, False, True]] and v[1, 2] == np.float32(13.5)
    assert sm.from_coo((2, 3), ([1, 0, 1, 1], [2, 0, 2, 2]), np.array([1, 2, 4, 8]))[1][1, 2] == 8
    assert sm.from_coo((2, 3), ([1, 1], [2, 2]), np.array([5, 3]), "first")[1][1, 2] == 5
    assert sm.from_coo((2, 3), ([1, 1], [2, 2]), np.array([5, 3]), "min")[1][1, 2] == 3
    # the cast comes before the fold: 300.0 saturates to 127, and 127 + 1 wraps
    assert sm.from_coo((1, 1), ([0, 0], [0, 0]), np.array([300.0, 1.0]), "plus", "INT8")[1][0, 0] == 127 + 1 - 256
    for bad in (-1, 3):
        with pytest.raises(sm.IndexOutOfBound):
            sm.from_coo((3, 3), (np.array([0, bad]), np.array([0, 0])), 1)
    # compressed input: jumbled rows are sorted, of duplicates the last is kept
    A = sm.from_csx((2, 4), [0, 3, 4], [3, 1, 3, 0], np.array([1, 2, 3, 4]))
    assert np.argwhere(A[0]).tolist() == [[0, 1], [0, 3], [1, 0]] and A[1][0, 3] == 3
    assert sm.path_of_csx([0, 3, 4], [3, 1, 3, 0]) == 2 and sm.path_of_csx([0, 2, 3], [1, 3, 0]) == 0
    assert sm.path_of_coo(([0, 0, 1], [1, 2, 0]), (2, 3)) == 0 and sm.path_of_coo(([0, 0], [1, 1]), (2, 3)) == 1
    B = sm.from_csx((4, 2), [0, 3, 4], [3, 1, 3, 0], np.array([1, 2, 3, 4]), by_col=True)
    assert sm.same_object(B, sm.dm.transpose(A), True)
    for ptr in ([1, 2, 4], [0, 3, 2], [0, 2, 5]):
        with pytest.raises(sm.InvalidValue):
            sm.from_csx((2, 4), ptr, [0, 1, 2, 3], np.array([1, 2, 3, 4]))
    with pytest.raises(sm.InvalidValue):
        sm.from_csx((2, 4), [0, 2, 4], [0, 1, 2, 3], np.array([1, 2, 3]))
    # Ap[last] below len(Ai): the tail is not read
    C = sm.from_csx((2, 4), [0, 1, 2], [0, 1, 9, 9], np.array([7, 8]))
    assert int(C[0].sum()) == 2
    # exports
    r, c, x = sm.to_coo(A, "INT32", "FP32")
    assert r.dtype == np.int32 and r.tolist() == [0, 0, 1] and c.tolist() == [1, 3, 0] and x.dtype == np.float32
    ptr, idx, x = sm.to_csr(A)
    assert ptr.tolist() == [0, 2, 3] and idx.tolist() == [1, 3, 0] and x.tolist() == [2, 3, 4]
    ptr, idx, x = sm.to_csc(A)
    assert ptr.tolist() == [0, 1, 2, 2, 3] and idx.tolist() == [1, 0, 0] and x.tolist() == [4, 2, 3]


# ---------------------------------------------------------------------- the front end, before any call
class Stub:
    """a device array that is only described: nothing may read the address"""

    def __init__(self, n, np_type=np.int64, strides=None, shape=None):
        t = np.dtype(np_type)
        self.__cuda_array_interface__ = {"shape": (n,) if shape is None else shape, "typestr": t.str,
                                         "data": (0xdead0000, False), "version": 3, "strides": strides}


@pytest.fixture
def no_calls(monkeypatch):
    import graphblas_amd.base
    import graphblas_amd.dense
    import graphblas_amd.matrix
    import graphblas_amd.sparse
    import graphblas_amd.vector

    def refuse(name, args):
        raise AssertionError(f"{name} was called")

    for mod in (graphblas_amd.base, graphblas_amd.dense, graphblas_amd.matrix, graphblas_amd.sparse,
                graphblas_amd.vector):
        monkeypatch.setattr(mod, "call", refuse)


def test_argument_errors_come_before_any_library_call(no_calls):
    import graphblas_amd as gb

    M, V = gb.Matrix, gb.Vector
    i, x, host = Stub(5), Stub(5, np.float64), np.arange(5)
    # mixing host and device arrays
    for call in (lambda: M.from_coo(i, host, x, nrows=9, ncols=9), lambda: M.from_coo(i, i, [1.0] * 5, nrows=9, ncols=9),
                 lambda: M.from_coo(host, host, x), lambda: M.from_csr(host, i, x, ncols=9),
                 lambda: M.from_csc(i, i, host, nrows=9), lambda: V.from_coo(host, x, size=9),
                 lambda: V.from_coo(i, [1.0] * 5, size=9)):
        with pytest.raises(ValueError, match="host and device arrays cannot be mixed"):
            call()
    # a device array that is not contiguous
    strided = Stub(5, np.int64, strides=(16,))
    for call in (lambda: M.from_coo(strided, i, x, nrows=9, ncols=9), lambda: M.from_coo(i, i, Stub(5, np.float64, (16,)),
                                                                                         nrows=9, ncols=9),
                 lambda: M.from_csr(i, strided, x, ncols=9), lambda: V.from_coo(strided, x, size=9)):
        with pytest.raises(ValueError, match="contiguous"):
            call()
    with pytest.raises(ValueError, match="one-dimensional"):
        M.from_coo(Stub(0, shape=(2, 5)), i, x, nrows=9, ncols=9)
    # index types
    for bad in (np.int16, np.uint32, np.float64, np.bool_):
        with pytest.raises(TypeError, match="must be int32, int64 or uint64"):
            M.from_coo(Stub(5, bad), Stub(5, bad), x, nrows=9, ncols=9)
        with pytest.raises(TypeError, match="must be int32, int64 or uint64"):
            V.from_coo(Stub(5, bad), x, size=9)
        with pytest.raises(TypeError, match="must be int32, int64 or uint64"):
            M.from_csr(Stub(3, bad), Stub(5, bad), x, ncols=9)
    with pytest.raises(TypeError, match="must have the same dtype"):
        M.from_coo(i, Stub(5, np.int32), x, nrows=9, ncols=9)
    with pytest.raises(TypeError, match="must have the same dtype"):
        M.from_csc(Stub(3, np.int32), i, x, nrows=9)
    # dimensions that would need a maximum over device indices
    for call, name in ((lambda: M.from_coo(i, i, x, ncols=9), "nrows"), (lambda: M.from_coo(i, i, x, nrows=9), "ncols"),
                       (lambda: M.from_csr(Stub(3), i, x), "ncols"), (lambda: M.from_csc(Stub(3), i, x), "nrows"),
                       (lambda: V.from_coo(i, x), "size")):
        with pytest.raises(ValueError, match=f"`{name}` must be given"):
            call()
    # a 0-d numpy array is a scalar, not a host array mixed in
    with pytest.raises(ValueError, match="`nrows` must be given"):
        M.from_coo(i, i, np.array(7), ncols=9)
    with pytest.raises(ValueError, match="dup_op must be None if values is a scalar"):
        V.from_coo(i, np.float32(7), size=9, dup_op=gb.binary.plus)
    # the reference's errors
    with pytest.raises(ValueError, match="nrows must be None or equal to len\\(indptr\\) - 1; expected 2, got 8"):
        M.from_csr(Stub(3), i, x, nrows=8, ncols=9)
    with pytest.raises(ValueError, match="ncols must be None or equal to len\\(indptr\\) - 1; expected 2, got 8"):
        M.from_csc(Stub(3), i, x, nrows=9, ncols=8)
    with pytest.raises(ValueError, match="nrows must"):
        M.from_csr(np.array([0, 1, 2]), np.array([0, 1]), np.array([1, 2]), nrows=8)
    with pytest.raises(ValueError, match="ncols must"):
        M.from_csc(np.array([0, 1, 2]), np.array([0, 1]), np.array([1, 2]), ncols=8)
    with pytest.raises(ValueError, match="dup_op must be None if values is a scalar"):
        M.from_coo(i, i, 7, nrows=9, ncols=9, dup_op=gb.binary.plus)
    with pytest.raises(ValueError, match="dup_op must be None if values is a scalar"):
        V.from_coo(i, 7, size=9, dup_op=gb.binary.plus)
    with pytest.raises(ValueError, match="`rows` and `columns` and `values` lengths must match: 5, 4, 5"):
        M.from_coo(i, Stub(4), x, nrows=9, ncols=9)
    with pytest.raises(ValueError, match="`indices` and `values` lengths must match: 5, 4"):
        V.from_coo(i, Stub(4, np.float64), size=9)


def test_build_checks_its_arguments_before_it_touches_the_object(no_calls):
    import graphblas_amd as gb

    A = gb.Matrix.__new__(gb.Matrix)
    A.dtype, A.name, A._nrows, A._ncols, A._h = gb.dtypes.INT64, "A", 9, 9, None
    v = gb.Vector.__new__(gb.Vector)
    v.dtype, v.name, v._size, v._h = gb.dtypes.INT64, "v", 9, None
    i = Stub(5)
    with pytest.raises(ValueError, match="cannot be mixed"):
        A.build(i, np.arange(5), Stub(5), clear=True)
    with pytest.raises(TypeError, match="must be int32, int64 or uint64"):
        A.build(Stub(5, np.int8), Stub(5, np.int8), Stub(5), clear=True)
    with pytest.raises(ValueError, match="lengths must match"):
        v.build(i, Stub(4), clear=True)
    with pytest.raises(AssertionError, match="GrB_Vector_clear was called"):  # good arguments reach the library
        v.build(i, Stub(5), clear=True)


def test_export_argument_errors():
    import graphblas_amd as gb

    A = gb.Matrix.__new__(gb.Matrix)
    A.dtype, A.name, A._nrows, A._ncols, A._h = gb.dtypes.INT64, "A", 2, 3, None
    for method in (A.to_coo, A.to_csr, A.to_csc, A.T.to_csr, A.T.to_csc):
        with pytest.raises(TypeError, match="index_dtype must be int64 or int32"):
            method(device=True, index_dtype="uint8")
