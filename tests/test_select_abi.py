"""CPU checks of the select surface: the 74 builtin GrB_IndexUnaryOp objects the reference's
discovery expects (core/operator/indexunary.py:98-114) are exported data symbols, the select
entry points exist, and the front end names them as python-graphblas does (reference
tests/test_matrix.py:1238-1273).  No compute calls (no GPU here)."""
import ctypes
import pickle

import pytest

TYPES = ["BOOL", "INT8", "UINT8", "INT16", "UINT16", "INT32", "UINT32", "INT64", "UINT64", "FP32", "FP64"]
POSITIONAL = ["TRIL", "TRIU", "DIAG", "OFFDIAG", "COLLE", "COLGT", "ROWLE", "ROWGT"]
VALUE = ["EQ", "NE", "GT", "GE", "LT", "LE"]
OBJECTS = [f"GrB_{p}" for p in POSITIONAL] + [f"GrB_VALUE{c}_{t}" for c in VALUE for t in TYPES]
KIND_INDEXUNARY = 6


@pytest.fixture(scope="module")
def dll():
    import graphblas_amd

    return ctypes.CDLL(graphblas_amd.LIB_PATH)


def test_all_index_unary_objects_are_exported(dll):
    assert len(OBJECTS) == 74
    missing = []
    for n in OBJECTS:
        try:
            if not ctypes.c_void_p.in_dll(dll, n).value:
                missing.append(n)
        except ValueError:
            missing.append(n)
    assert not missing, missing


def test_builtin_lookup_kind_and_name(dll):
    h, kind = ctypes.c_void_p(), ctypes.c_int()
    f = dll.GxB_builtin_lookup
    f.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_char_p]
    g = dll.GxB_name
    g.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    for name in ("GrB_TRIL", "GrB_VALUEGT_FP64"):
        assert f(ctypes.byref(h), ctypes.byref(kind), name.encode()) == 0
        assert kind.value == KIND_INDEXUNARY
        assert h.value == ctypes.c_void_p.in_dll(dll, name).value
        s = ctypes.c_char_p()
        assert g(ctypes.byref(s), h) == 0 and s.value == name.encode()
    # the kinds that existed before keep their numbers
    for name, k in [("GrB_INT64", 0), ("GrB_PLUS_INT64", 1), ("GrB_PLUS_MONOID_INT64", 2),
                    ("GrB_LOR_LAND_SEMIRING_BOOL", 3), ("GrB_DESC_T0", 4), ("GrB_AINV_INT64", 5)]:
        assert f(ctypes.byref(h), ctypes.byref(kind), name.encode()) == 0 and kind.value == k, name


def test_index_unary_free_is_a_noop_on_builtins(dll):
    dll.GrB_IndexUnaryOp_free.argtypes = [ctypes.c_void_p]
    h = ctypes.c_void_p(ctypes.c_void_p.in_dll(dll, "GrB_TRIL").value)
    assert dll.GrB_IndexUnaryOp_free(ctypes.byref(h)) == 0
    assert ctypes.c_void_p.in_dll(dll, "GrB_TRIL").value


def test_select_entry_points_are_exported(dll):
    names = ["GrB_Matrix_select_Scalar", "GrB_Vector_select_Scalar"]
    names += [f"GrB_{k}_select_{t}" for k in ("Matrix", "Vector") for t in TYPES]
    assert len(names) == 24
    missing = [n for n in names if not hasattr(dll, n)]
    assert not missing, missing


def test_adapter_declares_select():
    import os

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cdef = open(os.path.join(root, "include", "graphblas_amd_cdef.h")).read()
    assert "typedef struct GB_IndexUnaryOp_opaque *GrB_IndexUnaryOp;" in cdef
    assert "extern GrB_IndexUnaryOp GrB_TRIL;" in cdef
    assert "GrB_Info GrB_Matrix_select_FP64(" in cdef and "GrB_Info GrB_Vector_select_Scalar(" in cdef


def test_front_end_naming(dll):
    import graphblas_amd as gb

    assert gb.select.valuegt["FP64"].gb_name == "GrB_VALUEGT_FP64"
    assert gb.select.valuegt["FP64"].gb_obj.value == ctypes.c_void_p.in_dll(dll, "GrB_VALUEGT_FP64").value
    assert gb.select.tril[bool].gb_name == "GrB_TRIL"
    assert gb.select.tril[float].gb_name == "GrB_TRIL" and gb.select.tril.is_positional
    assert gb.select.tril[bool].is_positional and not gb.select.valueeq.is_positional
    assert gb.select.from_string("col<=") is gb.select.colle
    assert gb.select.from_string("TRIU") is gb.select.triu
    assert gb.select.from_string("tril") is gb.select.tril
    assert gb.select.from_string("index>") is gb.select.rowgt
    assert gb.select.indexle is gb.select.rowle and gb.select.indexgt is gb.select.rowgt
    assert gb.indexunary.tril is gb.select.tril
    for s, name in [("<", "valuelt"), (">", "valuegt"), ("<=", "valuele"), (">=", "valuege"),
                    ("!=", "valuene"), ("==", "valueeq"), ("col>", "colgt"), ("row<=", "rowle"),
                    ("row>", "rowgt"), ("index<=", "rowle")]:
        assert gb.select.from_string(s) is getattr(gb.select, name), s
    assert gb.operator.get_typed_op(">", gb.INT64, gb.FP64, kind="select").gb_name == "GrB_VALUEGT_FP64"
    with pytest.raises(ValueError):
        gb.select.from_string("nope")
    assert sorted(gb._builtins.INDEXUNARYOPS) == sorted(OBJECTS)


def test_select_ops_pickle_to_the_same_object():
    import graphblas_amd as gb

    # reference tests/test_matrix.py:1272-1273
    assert pickle.loads(pickle.dumps(gb.select.tril)) is gb.select.tril
    assert pickle.loads(pickle.dumps(gb.select.tril[bool])) is gb.select.tril[bool]
    assert pickle.loads(pickle.dumps(gb.select.valueeq["INT8"])) is gb.select.valueeq["INT8"]
    assert pickle.loads(pickle.dumps(gb.indexunary.tril)) is gb.indexunary.tril
