"""CPU checks of the eWiseUnion surface: GxB_Matrix_eWiseUnion / GxB_Vector_eWiseUnion are
exported, declared in both headers and typed in _lib; the numpy model the GPU tests compare with
(tests/union_model.py) reproduces the reference's own cases (tests/golden/ewise_union_golden.json)
and a few hand-worked ones; and Matrix / TransposedMatrix / Vector.ewise_union, the functional
style and `A - B` build the expression python-graphblas builds (reference core/matrix.py:2044-2161,
core/vector.py:1141-1260, core/operator/binary.py:81-97, core/infixmethods.py:237-242).
No compute calls: objects are stubs without handles, literal defaults become stub Scalars."""
import ctypes
import os
import re

import numpy as np
import pytest

import dense_model as dm
import union_model as um

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = {
    "GxB_Matrix_eWiseUnion": "GrB_Matrix C, const GrB_Matrix Mask, const GrB_BinaryOp accum, const GrB_BinaryOp add, "
                             "const GrB_Matrix A, const GrB_Scalar alpha, const GrB_Matrix B, const GrB_Scalar beta, "
                             "const GrB_Descriptor desc",
    "GxB_Vector_eWiseUnion": "GrB_Vector w, const GrB_Vector mask, const GrB_BinaryOp accum, const GrB_BinaryOp add, "
                             "const GrB_Vector u, const GrB_Scalar alpha, const GrB_Vector v, const GrB_Scalar beta, "
                             "const GrB_Descriptor desc",
}
POSITIONAL = ("firsti", "firsti1", "firstj", "firstj1", "secondi", "secondi1", "secondj", "secondj1")


# ---------------------------------------------------------------------- the C ABI
def test_entry_points_are_exported_and_declared():
    import graphblas_amd
    from graphblas_amd import _lib

    dll = ctypes.CDLL(graphblas_amd.LIB_PATH)
    for path in ("graphblas_amd.h", "graphblas_amd_cdef.h"):
        text = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", path)).read())
        for name, args in ENTRY_POINTS.items():
            assert f"GrB_Info {name}({args});" in text, (path, name)
    for name in ENTRY_POINTS:
        assert hasattr(dll, name), name
        assert _lib._SIGS[name] == [ctypes.c_void_p] * 9, name
        assert name in dir(_lib.lib)


# ---------------------------------------------------------------------- the model
@pytest.mark.parametrize("case", um.golden_cases(), ids=lambda c: c["source"].split(" ")[0])
def test_model_reproduces_the_golden_cases(case):
    A, B = um.golden_operand(case["A"]), um.golden_operand(case["B"])
    if case["at"]:
        A = dm.transpose(A)
    if case["bt"]:
        B = dm.transpose(B)
    want = um.golden_operand(case["expect"])
    got = um.ewise_union(case["op"], case["dtype"], A, um.golden_default(case["left_default"]), B,
                         um.golden_default(case["right_default"]))
    assert np.array_equal(got[0], want[0])
    assert got[1].dtype == want[1].dtype == dm.NP[case["expect"]["dtype"]]
    if case["close"]:
        assert np.allclose(got[1], want[1], rtol=1e-7, atol=0)
    else:
        assert np.array_equal(got[1], want[1])


def test_model_hand_worked_cases():
    t, f = True, False
    # a comparison: BOOL result; -5 < beta = 0, alpha = 7 < 9, 3 < 3 is false
    A = (np.array([t, f, t, f]), np.array([-5, 0, 3, 0], np.int16))
    B = (np.array([f, t, t, f]), np.array([0, 9, 3, 0], np.int16))
    p, v = um.ewise_union("lt", "INT16", A, np.int16(7), B, np.int16(0))
    assert v.dtype == np.bool_ and p.tolist() == [t, t, t, f] and v.tolist() == [t, t, f, f]
    assert um.case_counts(A, B) == (1, 1, 1)
    # casts that saturate: FP64 defaults into INT8 plus; NaN -> 0, 1e9 -> 127, -1e9 -> -128, then
    # the INT8 addition wraps: 100 + 127 = 227 - 256
    A8 = (np.array([t, f, t]), np.array([100, 0, 1], np.int8))
    B8 = (np.array([f, t, t]), np.array([0, -3, 2], np.int8))
    p, v = um.ewise_union("plus", "INT8", A8, np.float64(np.nan), B8, np.float64(1e9))
    assert v.dtype == np.int8 and v.tolist() == [100 + 127 - 256, 0 - 3, 3]
    p, v = um.ewise_union("plus", "INT8", A8, np.float64(-1e9), B8, np.float64(2.9))
    assert v.tolist() == [102, -128 - 3 + 256, 3]
    # float operands cast into an integer operator as well, before the operator runs
    Af = (np.array([t, t]), np.array([2.9, -np.inf]))
    Bf = (np.array([f, t]), np.array([0.0, np.nan]))
    p, v = um.ewise_union("minus", "INT32", Af, 0, Bf, 1)
    assert v.dtype == np.int32 and v.tolist() == [2 - 1, -2 ** 31 - 0]
    # minus is not symmetric in "missing": a B-only entry is alpha - b, where eWiseAdd copies b
    p, v = um.ewise_union("minus", "FP64", (np.array([f]), np.array([0.0])), 0.0, (np.array([t]), np.array([6.0])), 0.0)
    assert v.tolist() == [-6.0] and dm.ewise("add", "minus", "FP64", (np.array([f]), np.array([0.0])),
                                              (np.array([t]), np.array([6.0])))[1].tolist() == [6.0]
    # div with defaults 1 keeps a one-sided entry's value or its reciprocal
    p, v = um.ewise_union("div", "FP64", (np.array([t, f]), np.array([8.0, 0.0])), 1, (np.array([f, t]), np.array([0.0, 4.0])), 1)
    assert v.tolist() == [8.0, 0.25]
    # both empty
    p, v = um.ewise_union("plus", "INT64", (np.zeros((2, 3), bool), np.zeros((2, 3), np.int64)), 5,
                          (np.zeros((2, 3), bool), np.zeros((2, 3), np.int64)), 6)
    assert not p.any() and not v.any()


def test_position_formulas_against_a_numpy_union():
    """the closed forms of csrc/gb_ewise_union.hip (S = B-only entries before an entry of B):
    orp[i] = arp[i] + S(brp[i]); an A entry p lands at p + S(lower_bound(B row, j)); a B-only
    entry q at lower_bound(A row, j) + S(q) -- on random structures with empty rows"""
    rng = np.random.default_rng(11)
    for trial in range(60):
        m, n = int(rng.integers(1, 9)), int(rng.integers(1, 70))
        ap, bp = rng.random((m, n)) < rng.random(), rng.random((m, n)) < rng.random()
        ap[rng.integers(0, m)] = False
        bp[rng.integers(0, m)] = False
        ar, ac = np.nonzero(ap)
        br, bc = np.nonzero(bp)
        arp = np.concatenate([[0], np.cumsum(np.bincount(ar, minlength=m))])
        brp = np.concatenate([[0], np.cumsum(np.bincount(br, minlength=m))])
        bonly = ~ap[br, bc]
        S = np.concatenate([[0], np.cumsum(bonly)])
        ur, uc = np.nonzero(ap | bp)
        want_rp = np.concatenate([[0], np.cumsum(np.bincount(ur, minlength=m))])
        assert np.array_equal(arp + S[brp], want_rp)
        out = np.full(ur.size, -1)
        for p in range(ar.size):
            i = ar[p]
            lb = brp[i] + np.searchsorted(bc[brp[i]:brp[i + 1]], ac[p], side="left")
            dst = p + S[lb]
            assert out[dst] == -1
            out[dst] = ac[p]
        for q in np.flatnonzero(bonly):
            i = br[q]
            la = arp[i] + np.searchsorted(ac[arp[i]:arp[i + 1]], bc[q], side="left")
            dst = la + S[q]
            assert out[dst] == -1
            out[dst] = bc[q]
        assert np.array_equal(out, uc)


# ---------------------------------------------------------------------- the front end, no device
def mstub(gb, dtype, nrows, ncols, name):
    from graphblas_amd.matrix import Matrix

    A = Matrix.__new__(Matrix)
    A.dtype, A.name, A._h, A._nrows, A._ncols = gb.dtypes.lookup_dtype(dtype), name, ctypes.c_void_p(), nrows, ncols
    return A


def vstub(gb, dtype, size, name):
    from graphblas_amd.vector import Vector

    v = Vector.__new__(Vector)
    v.dtype, v.name, v._h, v._size = gb.dtypes.lookup_dtype(dtype), name, ctypes.c_void_p(), size
    return v


def sstub(gb, dtype, value, name="s"):
    from graphblas_amd.scalar import Scalar

    s = Scalar.__new__(Scalar)
    s.dtype, s.name, s._h, s.stub_value = gb.dtypes.lookup_dtype(dtype), name, None, value
    return s


@pytest.fixture
def gb(monkeypatch):
    """the package, with Scalar.from_value making stubs (a real GrB_Scalar needs the device)"""
    import graphblas_amd
    from graphblas_amd.scalar import Scalar

    def from_value(value, dtype=None, *, name=None, **_):
        if dtype is None:
            dtype = np.asarray(value).dtype
        return sstub(graphblas_amd, dtype, value, name or "s")

    monkeypatch.setattr(Scalar, "from_value", staticmethod(from_value))
    return graphblas_amd


def test_methods_exist():
    import graphblas_amd as gb

    assert callable(gb.Matrix.ewise_union) and callable(gb.TransposedMatrix.ewise_union)
    assert callable(gb.Vector.ewise_union)


def test_expression_cfunc_arguments_and_transposes(gb):
    A, B = mstub(gb, "INT64", 3, 5, "A"), mstub(gb, "INT64", 3, 5, "B")
    Bt = mstub(gb, "INT64", 5, 3, "Bt")
    e = A.ewise_union(B, gb.binary.plus, 10, 20)
    assert e.method_name == "ewise_union" and e.cfunc_name == "GxB_Matrix_eWiseUnion"
    assert e.shape == (3, 5) and e.dtype == "INT64" and e.op.gb_name == "GrB_PLUS_INT64"
    assert not e.at and not e.bt and len(e.args) == 4
    a, ld, b, rd = e.args  # (add,) A, alpha, B, beta: the C argument order after the operator
    assert a is A and b is B
    assert (ld.dtype, ld.stub_value, rd.dtype, rd.stub_value) == ("INT64", 10, "INT64", 20)
    e = A.ewise_union(Bt.T, gb.binary.plus, 10, 20)
    assert e.shape == (3, 5) and e.bt and not e.at and e.args[0] is A and e.args[2] is Bt
    e = Bt.T.ewise_union(A, gb.binary.plus, 10, 20)
    assert e.shape == (3, 5) and e.at and not e.bt and e.args[0] is Bt and e.args[2] is A
    e = A.T.ewise_union(Bt, gb.binary.minus, 0, 0)
    assert e.shape == (5, 3) and e.at and not e.bt
    e = A.T.ewise_union(B.T, gb.binary.minus, 0, 0)
    assert e.shape == (5, 3) and e.at and e.bt
    # Scalars are passed through as they are
    s10, s20 = sstub(gb, "INT64", 10, "ten"), sstub(gb, "INT8", 20, "twenty")
    e = A.ewise_union(B, gb.binary.plus, s10, s20)
    assert e.args[1] is s10 and e.args[3] is s20 and e.op.gb_name == "GrB_PLUS_INT64"
    # vectors
    v, w = vstub(gb, "INT64", 7, "v"), vstub(gb, "INT32", 7, "w")
    e = v.ewise_union(w, gb.binary.minus, 0, 0)
    assert e.cfunc_name == "GxB_Vector_eWiseUnion" and e.method_name == "ewise_union" and e.size == 7
    assert e.args[0] is v and e.args[2] is w and e.dtype == "INT64" and e.op.gb_name == "GrB_MINUS_INT64"


def test_operator_dtype_rule(gb):
    A, B = mstub(gb, "INT64", 1, 3, "A"), mstub(gb, "INT64", 1, 3, "B")
    # float defaults upcast integer operands (reference tests/test_matrix.py:3581-3584)
    e = A.ewise_union(B, gb.monoid.plus, 10.1, 20.2)
    assert e.op.opclass == "BinaryOp" and e.op.gb_name == "GrB_PLUS_FP64" and e.dtype == "FP64"
    # the defaults unify with each other first
    e = A.ewise_union(B, gb.binary.plus, 1, 2.5)
    assert e.op.gb_name == "GrB_PLUS_FP64"
    # the operands unify with each other, then with the defaults' type
    C, D = mstub(gb, "FP32", 1, 3, "C"), mstub(gb, "INT8", 1, 3, "D")
    assert C.ewise_union(D, gb.binary.times, np.float32(1), np.float32(1)).op.gb_name == "GrB_TIMES_FP32"
    assert D.ewise_union(C, gb.binary.times, np.int8(1), np.int8(1)).op.gb_name == "GrB_TIMES_FP32"
    assert D.ewise_union(D, gb.binary.times, np.int8(1), np.int8(1)).op.gb_name == "GrB_TIMES_INT8"
    # a comparison returns BOOL; a typed operator is taken as it is
    e = A.ewise_union(B, gb.binary.lt, 0, 0)
    assert e.dtype == "BOOL" and e.op.gb_name == "GrB_LT_INT64"
    assert A.ewise_union(B, gb.binary.minus["FP32"], 0, 0).op.gb_name == "GrB_MINUS_FP32"
    # a Monoid becomes its BinaryOp, typed or not, and a string names a binary operator
    assert A.ewise_union(B, gb.monoid.min["INT64"], 0, 0).op.gb_name == "GrB_MIN_INT64"
    assert A.ewise_union(B, gb.monoid.max, 0, 0).op.opclass == "BinaryOp"
    assert A.ewise_union(B, "minus", 0, 0).op.gb_name == "GrB_MINUS_INT64"


def test_rejected_arguments(gb):
    A, B = mstub(gb, "INT64", 3, 5, "A"), mstub(gb, "INT64", 3, 5, "B")
    v, w = vstub(gb, "INT64", 5, "v"), vstub(gb, "INT64", 5, "w")
    # the four TypeErrors: a default that is no scalar (either side), one keyword only, no infix
    with pytest.raises(TypeError, match="Literal scalars also accepted."):
        A.ewise_union(B, gb.binary.plus, [1, 2], 0)
    with pytest.raises(TypeError, match="Literal scalars also accepted."):
        v.ewise_union(w, gb.binary.plus, 0, B)
    with pytest.raises(TypeError, match="Literal scalars also accepted."):
        A.ewise_union(B, gb.binary.plus, None, 0)
    for kw in ({"left_default": 0}, {"right_default": 0}):
        with pytest.raises(TypeError, match="left_default"):
            gb.binary.minus(A | B, **kw)
    with pytest.raises(TypeError, match="infix"):
        gb.binary.minus(A, B, left_default=0, right_default=0)
    with pytest.raises(TypeError, match="infix"):
        gb.binary.minus(A & B, left_default=0, right_default=0)
    with pytest.raises(TypeError, match="infix"):
        gb.binary.minus["INT64"](A, left_default=0, right_default=0)
    # operand kinds
    with pytest.raises(TypeError, match="other"):
        A.ewise_union(v, gb.binary.plus, 0, 0)  # broadcasting is out of scope
    with pytest.raises(TypeError, match="other"):
        v.ewise_union(A, gb.binary.plus, 0, 0)
    with pytest.raises(TypeError, match="op"):
        A.ewise_union(B, gb.semiring.plus_times, 0, 0)
    # shapes are checked when the expression is built
    with pytest.raises(gb.exceptions.DimensionMismatch):
        A.ewise_union(mstub(gb, "INT64", 1, 1, "bad"), gb.binary.plus, 0, 0)
    with pytest.raises(gb.exceptions.DimensionMismatch):
        A.ewise_union(B.T, gb.binary.plus, 0, 0)
    with pytest.raises(gb.exceptions.DimensionMismatch):
        v.ewise_union(vstub(gb, "INT64", 1, "bad"), gb.binary.plus, 0, 0)
    for name in POSITIONAL:
        with pytest.raises(NotImplementedError, match="positional"):
            A.ewise_union(B, getattr(gb.binary, name), 0, 0)
        with pytest.raises(NotImplementedError, match="positional"):
            v.ewise_union(w, getattr(gb.binary, name), 0, 0)


def same_expression(e, f):
    return (type(e) is type(f) and e.cfunc_name == f.cfunc_name and e.op is f.op and e.at == f.at and e.bt == f.bt
            and e.args[0] is f.args[0] and e.args[2] is f.args[2] and e.dtype == f.dtype
            and [(s.dtype, s.stub_value) for s in (e.args[1], e.args[3])]
            == [(s.dtype, s.stub_value) for s in (f.args[1], f.args[3])])


def test_functional_style_and_subtraction_build_the_same_expression(gb):
    A, B = mstub(gb, "INT64", 3, 5, "A"), mstub(gb, "FP32", 3, 5, "B")
    v, w = vstub(gb, "INT64", 5, "v"), vstub(gb, "INT64", 5, "w")
    for x, y in ((A, B), (v, w)):
        e = x.ewise_union(y, gb.binary.minus, 0, 0)
        assert same_expression(gb.binary.minus(x | y, left_default=0, right_default=0), e)
        assert same_expression(x - y, e)
        f = x.ewise_union(y, gb.binary.div, 1, 1.5)
        assert same_expression(gb.binary.div(x | y, left_default=1, right_default=1.5), f)
        assert f.op.type == "FP64"
        typed = gb.binary.minus["FP64"]
        assert same_expression(typed(x | y, left_default=0, right_default=0), x.ewise_union(y, typed, 0, 0))
    At = mstub(gb, "INT64", 5, 3, "At")
    assert same_expression(At.T - A, At.T.ewise_union(A, gb.binary.minus, 0, 0))
    assert same_expression(A - At.T, A.ewise_union(At.T, gb.binary.minus, 0, 0))
    # the functional style without the keywords is still eWiseAdd
    assert gb.binary.minus(A | B).cfunc_name == "GrB_Matrix_eWiseAdd_BinaryOp"
    # a scalar operand is not this change's business, nor a matrix with a vector
    assert A.__sub__(1) is NotImplemented and v.__sub__(2.5) is NotImplemented
    assert A.__sub__(v) is NotImplemented and v.__sub__(A) is NotImplemented
    with pytest.raises(TypeError):
        A - 1
