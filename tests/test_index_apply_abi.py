"""CPU checks of the surface of GrB_apply with an index-unary operator: the six index-valued
builtin GrB_IndexUnaryOp objects (GrB_ROWINDEX / COLINDEX / DIAGINDEX _INT32 / _INT64) are exported
data symbols the registry knows, the 24 entry points exist and are declared for the adapter, the
front end names the operators as python-graphblas does (reference tests/test_matrix.py:1203-1235),
and the numpy model of tests/index_apply_model.py agrees with hand-worked cases.  No compute calls
(no GPU here)."""
import ctypes
import os
import pickle

import numpy as np
import pytest

import index_apply_model as im

TYPES = ["BOOL", "INT8", "UINT8", "INT16", "UINT16", "INT32", "UINT32", "INT64", "UINT64", "FP32", "FP64"]
OBJECTS = [f"GrB_{op}_{t}" for op in ("ROWINDEX", "COLINDEX", "DIAGINDEX") for t in ("INT32", "INT64")]
ENTRY_POINTS = ["GrB_Matrix_apply_IndexOp_Scalar", "GrB_Vector_apply_IndexOp_Scalar"] + \
    [f"GrB_{k}_apply_IndexOp_{t}" for k in ("Matrix", "Vector") for t in TYPES]
KIND_INDEXUNARY = 6


@pytest.fixture(scope="module")
def dll():
    import graphblas_amd

    return ctypes.CDLL(graphblas_amd.LIB_PATH)


def test_index_valued_objects_are_exported(dll):
    assert len(OBJECTS) == 6
    for n in OBJECTS:
        assert ctypes.c_void_p.in_dll(dll, n).value, n


def test_builtin_lookup_kind_and_name(dll):
    h, kind = ctypes.c_void_p(), ctypes.c_int()
    f = dll.GxB_builtin_lookup
    f.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_char_p]
    g = dll.GxB_name
    g.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    for name in OBJECTS:
        assert f(ctypes.byref(h), ctypes.byref(kind), name.encode()) == 0
        assert kind.value == KIND_INDEXUNARY
        assert h.value == ctypes.c_void_p.in_dll(dll, name).value
        s = ctypes.c_char_p()
        assert g(ctypes.byref(s), h) == 0 and s.value == name.encode()
    assert len({ctypes.c_void_p.in_dll(dll, n).value for n in OBJECTS}) == 6


def test_index_unary_free_is_a_noop(dll):
    dll.GrB_IndexUnaryOp_free.argtypes = [ctypes.c_void_p]
    before = ctypes.c_void_p.in_dll(dll, "GrB_ROWINDEX_INT64").value
    h = ctypes.c_void_p(before)
    assert dll.GrB_IndexUnaryOp_free(ctypes.byref(h)) == 0
    assert ctypes.c_void_p.in_dll(dll, "GrB_ROWINDEX_INT64").value == before


def test_entry_points_are_exported_and_declared(dll):
    assert len(ENTRY_POINTS) == 24
    missing = [n for n in ENTRY_POINTS if not hasattr(dll, n)]
    assert not missing, missing
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cdef = open(os.path.join(root, "include", "graphblas_amd_cdef.h")).read()
    for n in ENTRY_POINTS:
        assert f"GrB_Info {n}(" in cdef, n
    for n in OBJECTS:
        assert f"extern GrB_IndexUnaryOp {n};" in cdef, n
    from graphblas_amd import _lib

    for n in ENTRY_POINTS + OBJECTS:
        assert n in dir(_lib.lib), n
    assert len(_lib._SIGS["GrB_Matrix_apply_IndexOp_FP32"]) == 7
    assert _lib._SIGS["GrB_Vector_apply_IndexOp_FP32"][5] is ctypes.c_float


def test_front_end_naming(dll):
    import graphblas_amd as gb

    iu = gb.indexunary
    for name in ("rowindex", "colindex", "diagindex"):
        op = getattr(iu, name)
        up = name.upper()
        assert op[int].gb_name == f"GrB_{up}_INT64"
        assert op[int].gb_obj.value == ctypes.c_void_p.in_dll(dll, f"GrB_{up}_INT64").value
        assert op["INT32"].gb_name == f"GrB_{up}_INT32"
        assert op["INT32"].return_type == gb.INT32 and op[int].return_type == gb.INT64
        # any other input type takes the INT64 operator, as the positional binaries do
        for dt in (float, bool, "FP32", "INT8", "UINT32", "UINT64"):
            assert op[dt].gb_name == f"GrB_{up}_INT64", (name, dt)
        assert op.is_positional and op[int].is_positional
        assert gb.operator.get_typed_op(op, gb.INT32).gb_name == f"GrB_{up}_INT32"
        assert gb.operator.get_typed_op(op, gb.FP64).gb_name == f"GrB_{up}_INT64"
        assert not hasattr(gb.select, name)
    assert iu.index is iu.rowindex
    assert not hasattr(gb.select, "index")
    for s in ("rowindex", "colindex", "diagindex", "index", "ROWINDEX", " colindex "):
        assert iu.from_string(s) is getattr(iu, s.strip().lower()), s
    assert iu.from_string("rowindex[INT32]").gb_name == "GrB_ROWINDEX_INT32"
    with pytest.raises(ValueError):
        gb.select.from_string("rowindex")
    with pytest.raises(ValueError):
        iu.from_string("nope")
    # the select operators as value producers: BOOL results, the same library objects
    assert iu.tril is gb.select.tril
    assert iu.from_string("tril") is gb.select.tril and iu.from_string("col<=") is gb.select.colle
    assert iu.valueeq["FP64"].gb_name == "GrB_VALUEEQ_FP64" and iu.valueeq["FP64"].return_type == gb.BOOL
    assert iu.from_string("==") is iu.valueeq
    assert iu.valueeq["INT8"].gb_obj.value == gb.select.valueeq["INT8"].gb_obj.value
    # the select tables are what they were
    assert len(gb._builtins.INDEXUNARYOPS) == 74
    assert not set(OBJECTS) & set(gb._builtins.INDEXUNARYOPS)
    assert sorted(gb._builtins.INDEXVALUEOPS) == sorted(OBJECTS)
    assert sorted(n for n in vars(gb.select) if n != "from_string") == sorted(
        ["tril", "triu", "diag", "offdiag", "colle", "colgt", "rowle", "rowgt", "indexle", "indexgt", "valueeq",
         "valuene", "valuegt", "valuege", "valuelt", "valuele"])


def test_index_unary_ops_pickle_to_the_same_object():
    import graphblas_amd as gb

    iu = gb.indexunary
    for op in (iu.rowindex, iu.colindex, iu.diagindex, iu.index, iu.valueeq, iu.tril):
        assert pickle.loads(pickle.dumps(op)) is op
    for op in (iu.rowindex[int], iu.rowindex["INT32"], iu.diagindex[float], iu.valueeq["INT8"], iu.tril[int]):
        assert pickle.loads(pickle.dumps(op)) is op


def test_opcodes_are_appended():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    codes = open(os.path.join(root, "include", "gbamd_codes.h")).read()
    for line in ("GBAMD_IOP_TRIL = 0,", "GBAMD_IOP_ROWGT = 7,", "GBAMD_IOP_VALUEEQ = 8,", "GBAMD_IOP_VALUELE = 13,",
                 "GBAMD_IOP_ROWINDEX = 14,", "GBAMD_IOP_COLINDEX = 15,", "GBAMD_IOP_DIAGINDEX = 16,",
                 "GBAMD_IOP_COUNT = 17"):
        assert line in codes, line


# ------------------------------------------------------------------ the model, by hand
# 3 x 4, entries (0,1) (0,3) (1,0) (2,2) (2,3) with values 5, -2, 0, 7, 5
P = np.array([[0, 1, 0, 1], [1, 0, 0, 0], [0, 0, 1, 1]], bool)
V = np.array([[0, 5, 0, -2], [0, 0, 0, 0], [0, 0, 7, 5]], np.int64)


def triples(T):
    p, z = T
    r, c = np.nonzero(p)
    return list(zip(r.tolist(), c.tolist(), z[r, c].tolist()))


def test_model_index_valued():
    p, z = im.index_apply((P, V), "rowindex", "INT64", 10)
    assert z.dtype == np.int64 and np.array_equal(p, P)
    assert triples((p, z)) == [(0, 1, 10), (0, 3, 10), (1, 0, 11), (2, 2, 12), (2, 3, 12)]
    assert triples(im.index_apply((P, V), "colindex", "INT64", -1)) == \
        [(0, 1, 0), (0, 3, 2), (1, 0, -1), (2, 2, 1), (2, 3, 2)]  # a stored 0 stays an entry
    assert triples(im.index_apply((P, V), "diagindex", "INT64", 0)) == \
        [(0, 1, 1), (0, 3, 3), (1, 0, -1), (2, 2, 0), (2, 3, 1)]
    # INT32: the thunk is cast first (2.9 -> 2), the 64-bit sum wraps in the cast
    p, z = im.index_apply((P, V), "rowindex", "INT32", 2.9)
    assert z.dtype == np.int32 and triples((p, z)) == [(0, 1, 2), (0, 3, 2), (1, 0, 3), (2, 2, 4), (2, 3, 4)]
    p, z = im.index_apply((P, V), "rowindex", "INT32", 2**31 - 1)
    assert triples((p, z)) == [(0, 1, 2**31 - 1), (0, 3, 2**31 - 1), (1, 0, -2**31), (2, 2, -2**31 + 1),
                               (2, 3, -2**31 + 1)]
    # a thunk beyond INT32 wraps in its own cast: 2^32 + 5 -> 5
    assert triples(im.index_apply((P, V), "colindex", "INT32", 2**32 + 5))[:2] == [(0, 1, 6), (0, 3, 8)]
    assert im.result_dtype("rowindex", "INT32") == "INT32" and im.result_dtype("tril", None) == "BOOL"


def test_model_positional_predicates():
    p, z = im.index_apply((P, V), "tril", None, 0)
    assert z.dtype == np.bool_
    assert triples((p, z)) == [(0, 1, False), (0, 3, False), (1, 0, True), (2, 2, True), (2, 3, False)]
    assert triples(im.index_apply((P, V), "triu", None, 1)) == \
        [(0, 1, True), (0, 3, True), (1, 0, False), (2, 2, False), (2, 3, True)]
    assert triples(im.index_apply((P, V), "colgt", None, 2.7)) == \
        [(0, 1, False), (0, 3, True), (1, 0, False), (2, 2, False), (2, 3, True)]  # 2.7 -> 2
    assert triples(im.index_apply((P, V), "rowle", None, -2**63)) == \
        [(0, 1, False), (0, 3, False), (1, 0, False), (2, 2, False), (2, 3, False)]
    # a vector entry is at (i, 0)
    vp, vv = np.array([1, 0, 1, 1], bool), np.array([4, 0, 5, 6])
    assert triples3(im.index_apply((vp, vv), "diagindex", "INT64", 10)) == [(0, 10), (2, 8), (3, 7)]
    assert triples3(im.index_apply((vp, vv), "colindex", "INT64", 10)) == [(0, 10), (2, 10), (3, 10)]
    assert triples3(im.index_apply((vp, vv), "diag", None, -2)) == [(0, False), (2, True), (3, False)]


def triples3(T):
    p, z = T
    i = np.flatnonzero(p)
    return list(zip(i.tolist(), z[i].tolist()))


def test_model_value_predicates():
    assert triples(im.index_apply((P, V), "valueeq", "INT64", 5)) == \
        [(0, 1, True), (0, 3, False), (1, 0, False), (2, 2, False), (2, 3, True)]
    # in UINT8 the entry -2 is 254 and the thunk 260 is 4
    assert triples(im.index_apply((P, V), "valuegt", "UINT8", 260)) == \
        [(0, 1, True), (0, 3, True), (1, 0, False), (2, 2, True), (2, 3, True)]
    F = np.where(P, np.array([[0, np.nan, 0, -0.0], [1.5, 0, 0, 0], [0, 0, np.inf, 2.0]]), 0.0)
    assert triples(im.index_apply((P, F), "valuene", "FP64", np.nan)) == \
        [(0, 1, True), (0, 3, True), (1, 0, True), (2, 2, True), (2, 3, True)]
    assert triples(im.index_apply((P, F), "valuele", "FP64", 0.0)) == \
        [(0, 1, False), (0, 3, True), (1, 0, False), (2, 2, False), (2, 3, False)]  # NaN false, -0.0 <= 0.0
    assert triples(im.index_apply((P, F), "valueeq", "BOOL", True)) == \
        [(0, 1, True), (0, 3, False), (1, 0, True), (2, 2, True), (2, 3, True)]  # NaN is true as BOOL
