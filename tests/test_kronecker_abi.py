"""CPU checks of the kronecker surface: the three GrB_Matrix_kronecker_* entry points are exported,
declared in both headers and typed in _lib; Matrix.kronecker / TransposedMatrix.kronecker build
the expression python-graphblas builds (reference core/matrix.py:2253-2292); and the numpy model
the GPU tests compare with reproduces the two golden cases.  No compute calls (no GPU here)."""
import ctypes
import json
import os

import numpy as np
import pytest

import dense_model as dm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["GrB_Matrix_kronecker_BinaryOp", "GrB_Matrix_kronecker_Monoid", "GrB_Matrix_kronecker_Semiring"]


def kron_model(A_coo, B_coo, shapes, op, dtype):
    """kron(A, B) under binary.<op>[dtype] on COO triples: ((rows, cols, vals) in row-major order,
    the result's dtype name).  shapes = ((m, n), (p, q)); every pair of entries gives
    T(iA p + iB, jA q + jB) = op(cast(a), cast(b)); a stable sort by (row, col) orders them."""
    (ar, ac, av), (br, bc, bv) = A_coo, B_coo
    (m, n), (p, q) = shapes
    ar, ac, br, bc = (np.asarray(x, np.int64) for x in (ar, ac, br, bc))
    av, bv = dm.cast(np.asarray(av), dtype), dm.cast(np.asarray(bv), dtype)
    ia, ib = np.repeat(np.arange(ar.size), br.size), np.tile(np.arange(br.size), ar.size)
    rows, cols = ar[ia] * p + br[ib], ac[ia] * q + bc[ib]
    vals = dm.binop(op, dtype, av[ia], bv[ib])
    assert (rows < m * p).all() and (cols < n * q).all()
    order = np.lexsort((cols, rows))  # stable; (row, col) pairs are distinct when the inputs' are
    return (rows[order], cols[order], np.asarray(vals)[order]), dm.binop_return_dtype(op, dtype)


def golden_cases():
    with open(os.path.join(ROOT, "tests", "golden", "kronecker_golden.json")) as f:
        return json.load(f)["cases"]


def coo(d):
    return d["rows"], d["cols"], d["vals"]


@pytest.fixture(scope="module")
def dll():
    import graphblas_amd

    return ctypes.CDLL(graphblas_amd.LIB_PATH)


def stub(gb, dtype, nrows, ncols, name):
    """a Matrix object without a handle: enough for building expressions"""
    from graphblas_amd.matrix import Matrix

    A = Matrix.__new__(Matrix)
    A.dtype, A.name, A._h, A._nrows, A._ncols = gb.dtypes.lookup_dtype(dtype), name, ctypes.c_void_p(), nrows, ncols
    return A


def test_entry_points_are_exported_and_declared(dll):
    from graphblas_amd import _lib

    missing = [n for n in ENTRY_POINTS if not hasattr(dll, n)]
    assert not missing, missing
    header = open(os.path.join(ROOT, "include", "graphblas_amd.h")).read()
    cdef = open(os.path.join(ROOT, "include", "graphblas_amd_cdef.h")).read()
    for n in ENTRY_POINTS:
        assert f"GrB_Info {n}(GrB_Matrix C, const GrB_Matrix Mask, const GrB_BinaryOp accum," in header, n
        assert f"GrB_Info {n}(" in cdef, n
        assert _lib._SIGS[n] == [ctypes.c_void_p] * 7, n
        assert n in dir(_lib.lib)


def test_methods_exist():
    import graphblas_amd as gb

    assert callable(gb.Matrix.kronecker) and callable(gb.TransposedMatrix.kronecker)


def test_expression_shape_dtype_and_cfunc():
    import graphblas_amd as gb

    A = stub(gb, "INT64", 3, 5, "A")
    B = stub(gb, "FP64", 7, 2, "B")
    e = A.kronecker(B)  # times by default
    assert e.method_name == "kronecker" and e.cfunc_name == "GrB_Matrix_kronecker_BinaryOp"
    assert e.shape == (21, 10) and (e.nrows, e.ncols) == (21, 10)
    assert e.dtype == "FP64" and e.op.gb_name == "GrB_TIMES_FP64"
    assert e.args == [A, B] and not e.at and not e.bt
    e = A.kronecker(B, gb.binary.times)
    assert e.dtype == "FP64" and e.shape == (21, 10)
    e = A.kronecker(B, "eq")
    assert e.dtype == "BOOL" and e.op.gb_name == "GrB_EQ_FP64" and e.shape == (21, 10)
    e = A.kronecker(B, gb.monoid.plus)
    assert e.cfunc_name == "GrB_Matrix_kronecker_Monoid" and e.op.gb_name == "GrB_PLUS_MONOID_FP64"
    assert e.dtype == "FP64"
    # transposed operands: the descriptor carries the transposes, the shape is that of kron(A', B')
    e = A.T.kronecker(B)
    assert e.shape == (35, 6) and e.at and not e.bt and e.args == [A, B]
    e = A.kronecker(B.T)
    assert e.shape == (6, 35) and e.bt and not e.at
    e = A.T.kronecker(B.T, gb.binary.first["INT8"])
    assert e.shape == (10, 21) and e.at and e.bt and e.dtype == "INT8"


def test_rejected_arguments():
    import graphblas_amd as gb
    from graphblas_amd.vector import Vector

    A = stub(gb, "INT64", 3, 5, "A")
    B = stub(gb, "INT64", 7, 2, "B")
    with pytest.raises(TypeError, match="[Ss]emiring"):
        A.kronecker(B, gb.semiring.plus_times)
    with pytest.raises(TypeError, match="[Ss]emiring"):
        A.T.kronecker(B, gb.semiring.plus_times["INT64"])
    v = Vector.__new__(Vector)
    v.dtype, v.name, v._h, v._size = gb.dtypes.lookup_dtype("INT64"), "v", ctypes.c_void_p(), 5
    with pytest.raises(TypeError, match="other"):
        A.kronecker(v)
    with pytest.raises(TypeError, match="other"):
        A.kronecker(3)
    for name in ("firsti", "firsti1", "firstj", "firstj1", "secondi", "secondi1", "secondj", "secondj1"):
        with pytest.raises(NotImplementedError, match="positional"):
            A.kronecker(B, getattr(gb.binary, name))
        with pytest.raises(NotImplementedError, match="positional"):
            A.T.kronecker(B.T, getattr(gb.binary, name))


@pytest.mark.parametrize("case", golden_cases(), ids=lambda c: c["source"])
def test_model_reproduces_the_golden_cases(case):
    a, b, c = case["A"], case["B"], case["C"]
    (r, col, v), zt = kron_model(coo(a), coo(b), ((a["nrows"], a["ncols"]), (b["nrows"], b["ncols"])),
                                 case["op"], case["dtype"])
    assert zt == case["dtype"]
    assert len(c["rows"]) == len(a["rows"]) * len(b["rows"])
    assert np.array_equal(r, c["rows"]) and np.array_equal(col, c["cols"])
    assert v.dtype == dm.NP[case["dtype"]] and np.array_equal(v, np.asarray(c["vals"], v.dtype))


def test_model_row_pointer_closed_form():
    """the kernel's row pointer, rowptrT[iA p + iB] = rowptrA[iA] nvals(B) + lenA(iA) rowptrB[iB],
    and its within-row decomposition, against the sorted expansion (random inputs, empty rows)"""
    rng = np.random.default_rng(3)
    for (m, n, p, q) in [(5, 4, 3, 6), (9, 7, 8, 2), (1, 1, 1, 1), (6, 6, 6, 6)]:
        Ap, Bp = rng.random((m, n)) < 0.4, rng.random((p, q)) < 0.4
        Ap[rng.integers(0, m)] = False
        Bp[rng.integers(0, p)] = False
        ar, ac = np.nonzero(Ap)
        br, bc = np.nonzero(Bp)
        (rows, cols, _), _ = kron_model((ar, ac, np.ones(ar.size, np.int64)), (br, bc, np.ones(br.size, np.int64)),
                                        ((m, n), (p, q)), "times", "INT64")
        rpA = np.concatenate([[0], np.cumsum(np.bincount(ar, minlength=m))])
        rpB = np.concatenate([[0], np.cumsum(np.bincount(br, minlength=p))])
        want = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=m * p))])
        R = np.arange(m * p)
        iA, iB = R // p, R % p
        got = rpA[iA] * br.size + (rpA[iA + 1] - rpA[iA]) * rpB[iB]
        assert np.array_equal(np.concatenate([got, [ar.size * br.size]]), want)
        for t in range(rows.size):
            Rt = rows[t]
            e, lenB = t - want[Rt], rpB[Rt % p + 1] - rpB[Rt % p]
            a, b = rpA[Rt // p] + e // lenB, rpB[Rt % p] + e % lenB
            assert cols[t] == ac[a] * q + bc[b]
