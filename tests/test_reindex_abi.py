"""CPU checks of the diag / reshape / flatten surface: the six entry points are exported, declared
in both headers, typed in _lib and named in INTEGRATION.md; the numpy model the GPU tests compare
with (tests/reindex_model.py) reproduces the reference's own cases
(tests/golden/diag_reshape_golden.json); the layout formulas of csrc/gb_reindex.hip, restated in
numpy, hold on random structures; and the front end's shape normalisation and argument errors are
raised before any library call (reference core/ss/matrix.py:252-279, 3717-3815,
core/ss/vector.py:147-183, 1377-1405, ss/_core.py:24-70).  No compute calls: objects are stubs
without handles."""
import ctypes
import os
import re

import numpy as np
import pytest

import dense_model as dm
import reindex_model as rm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = {
    "GrB_Matrix_diag": "GrB_Matrix *C, const GrB_Vector v, int64_t k",
    "GxB_Matrix_diag": "GrB_Matrix C, const GrB_Vector v, int64_t k, const GrB_Descriptor desc",
    "GxB_Vector_diag": "GrB_Vector v, const GrB_Matrix A, int64_t k, const GrB_Descriptor desc",
    "GxB_Matrix_reshape": "GrB_Matrix C, bool by_col, GrB_Index nrows_new, GrB_Index ncols_new, "
                          "const GrB_Descriptor desc",
    "GxB_Matrix_reshapeDup": "GrB_Matrix *C, GrB_Matrix A, bool by_col, GrB_Index nrows_new, GrB_Index ncols_new, "
                             "const GrB_Descriptor desc",
    "GxB_Vector_flatten": "GrB_Vector w, const GrB_Matrix A, bool by_col, const GrB_Descriptor desc",
}
G = rm.golden()
EXC = {"TypeError": TypeError, "ValueError": ValueError}


def ident(case):
    return f"{case['src']}{'' if 'k' not in case else ' k=' + str(case['k'])}"


# ---------------------------------------------------------------------- the C ABI
def test_entry_points_are_exported_and_declared():
    import graphblas_amd
    from graphblas_amd import _lib

    dll = ctypes.CDLL(graphblas_amd.LIB_PATH)
    for path in ("graphblas_amd.h", "graphblas_amd_cdef.h"):
        text = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", path)).read())
        for name, args in ENTRY_POINTS.items():
            assert f"GrB_Info {name}({args});" in text, (path, name)
    P, I, L, B = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int64, ctypes.c_bool
    sigs = {"GrB_Matrix_diag": [P, P, L], "GxB_Matrix_diag": [P, P, L, P], "GxB_Vector_diag": [P, P, L, P],
            "GxB_Matrix_reshape": [P, B, I, I, P], "GxB_Matrix_reshapeDup": [P, P, B, I, I, P],
            "GxB_Vector_flatten": [P, P, B, P]}
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ENTRY_POINTS:
        assert hasattr(dll, name), name
        assert _lib._SIGS[name] == sigs[name], name
        assert name in dir(_lib.lib)
        assert name in text, name


def test_adapter_exposes_the_symbols():
    cdef = open(os.path.join(ROOT, "include", "graphblas_amd_cdef.h")).read()
    for name in ENTRY_POINTS:
        assert f"GrB_Info {name}(" in cdef


# ---------------------------------------------------------------------- the model
def same(got, want):
    assert got[0].shape == want[0].shape and np.array_equal(got[0], want[0])
    assert got[1].dtype == want[1].dtype and np.array_equal(np.where(got[0], got[1], 0), want[1])


@pytest.mark.parametrize("case", G["matrix_diag"], ids=ident)
def test_model_matrix_diag_reproduces_the_golden_cases(case):
    A, k = rm.golden_A(G), case["k"]
    want = rm.pair_of((case["size"],), (case["idx"],), case["vals"])
    same(rm.diag_vector(A, k), want)
    same(rm.diag_vector(dm.transpose(A), -k), want)


@pytest.mark.parametrize("case", G["vector_diag"], ids=ident)
def test_model_vector_diag_reproduces_the_golden_cases(case):
    v, k, n = rm.golden_v(G), case["k"], case["n"]
    want = rm.pair_of((n, n), (case["rows"], case["cols"]), case["vals"])
    D = rm.diag_matrix(v, k)
    same(D, want)
    same(rm.diag_vector(D, k), v)  # A.diag(k) gives v back, and A.T.diag(-k, dtype=float) as FP64
    same(rm.diag_vector(dm.transpose(D), -k, "FP64"), rm.cast(v, "FP64"))


@pytest.mark.parametrize("case", G["flatten"], ids=ident)
def test_model_flatten_reproduces_the_golden_cases(case):
    A = rm.golden_A(G)
    want = rm.pair_of((case["size"],), (case["idx"],), case["vals"])
    w = rm.flatten(A, case["order"])
    same(w, want)
    same(rm.reshape(w, A[0].shape, case["order"]), A)
    i, x = rm.flatten_coo(G["A"]["rows"], G["A"]["cols"], G["A"]["vals"], A[0].shape, case["order"])
    assert np.array_equal(i, np.flatnonzero(want[0])) and np.array_equal(x, want[1][want[0]])


@pytest.mark.parametrize("case", G["reshape"]["cases"], ids=ident)
def test_model_reshape_reproduces_the_golden_cases(case):
    shape = tuple(G["reshape"]["resize"])
    A = rm.golden_A(G, shape)
    new = (case["nrows"], case["ncols"])
    want = rm.pair_of(new, (case["rows"], case["cols"]), case["vals"])
    got = rm.reshape(A, new, case["order"])
    same(got, want)
    same(rm.reshape(got, shape, case["order"]), A)
    r, c, x = rm.reshape_coo(G["A"]["rows"], G["A"]["cols"], G["A"]["vals"], shape, new, case["order"])
    wr, wc = np.nonzero(want[0])
    assert np.array_equal(r, wr) and np.array_equal(c, wc) and np.array_equal(x, want[1][wr, wc])


def test_model_hand_worked_cases():
    t, f = True, False
    v = (np.array([t, f, t]), np.array([5, 0, -7], np.int8))
    p, x = rm.diag_matrix(v, -1)
    assert p.shape == (4, 4) and np.argwhere(p).tolist() == [[1, 0], [3, 2]] and x[3, 2] == -7
    assert rm.diag_matrix((np.zeros(0, bool), np.zeros(0)), 2)[0].shape == (2, 2)
    A = (np.arange(12).reshape(3, 4) % 2 == 1, np.arange(12).reshape(3, 4))
    assert [rm.diag_size(3, 4, k) for k in (-3, -2, 0, 1, 3, 4, 1000, -1000)] == [0, 1, 3, 3, 1, 0, 0, 0]
    assert rm.diag_vector(A, 1)[1].tolist() == [1, 6, 11] and rm.diag_vector(A, 1)[0].tolist() == [t, f, t]
    assert rm.diag_vector(A, 1000)[0].shape == (0,) and rm.diag_vector(A, -3)[0].shape == (0,)
    # the saturating cast into the output's type
    w = rm.diag_vector((np.ones((2, 2), bool), np.array([[np.nan, 0], [0, 1e9]])), 0, "INT8")
    assert w[1].dtype == np.int8 and w[1].tolist() == [0, 127]
    # (i, j) of 3 x 4 goes to divmod(4 i + j, 6) row-major, to ((i + 3 j) % 2, (i + 3 j) // 2) column-major
    assert rm.reshape(A, (2, 6))[1].tolist() == [[0, 1, 2, 3, 4, 5], [6, 7, 8, 9, 10, 11]]
    assert rm.reshape(A, (2, 6), "columnwise")[1].tolist() == [[0, 8, 5, 2, 10, 7], [4, 1, 9, 6, 3, 11]]
    assert rm.flatten(A, "columnwise")[1].tolist() == [0, 4, 8, 1, 5, 9, 2, 6, 10, 3, 7, 11]
    r, c, x = rm.reshape_coo([0, 2], [3, 0], [30, 80], (3, 4), (2, 6), "columnwise")
    assert (r.tolist(), c.tolist(), x.tolist()) == ([0, 1], [1, 4], [80, 30])


# ---------------------------------------------------------------------- the kernels' formulas
def csr_of(p):
    r, c = np.nonzero(p)
    return np.concatenate([[0], np.cumsum(np.bincount(r, minlength=p.shape[0]))]).astype(np.int64), c


def random_shapes(rng):
    total = int(rng.choice([1, 6, 12, 60, 64, 210, 360]))
    divs = [d for d in range(1, total + 1) if total % d == 0]
    nr, nr2 = int(rng.choice(divs)), int(rng.choice(divs))
    return (nr, total // nr), (nr2, total // nr2)


def test_reshape_row_pointer_closed_form():
    """k_reshape_rowptr / k_reshape_cols: in CSR order lin = i * ncols + j increases, so entry p
    keeps its storage position, gets column lin % ncols', and rowptr'[r'] = rowptr[i0] +
    lower_bound(columns of row i0, j0) with (i0, j0) = divmod(r' * ncols', ncols) -- which is
    searchsorted(lin of all entries, r' * ncols')"""
    rng = np.random.default_rng(11)
    for trial in range(60):
        (nr, nc), (nr2, nc2) = random_shapes(rng)
        p = rng.random((nr, nc)) < rng.random()
        if nr > 2:
            p[rng.integers(0, nr)] = False
        rp, ci = csr_of(p)
        rows = np.repeat(np.arange(nr), np.diff(rp))
        lin = rows * nc + ci
        assert np.all(np.diff(lin) > 0)
        got = np.empty(nr2 + 1, np.int64)
        for r2 in range(nr2):
            i0, j0 = divmod(r2 * nc2, nc)
            got[r2] = rp[i0] + np.searchsorted(ci[rp[i0]:rp[i0 + 1]], j0)
        got[nr2] = ci.size
        assert np.array_equal(got, np.searchsorted(lin, np.arange(nr2 + 1) * nc2))
        wrp, wci = csr_of(rm.reshape((p, p), (nr2, nc2))[0])
        assert np.array_equal(got, wrp) and np.array_equal(lin % nc2, wci)


def test_bitmap_rank_formulas():
    """k_bitmap_csr: rank(p) = word prefix + popcount of the lower bits is the storage position of
    v(p); a diagonal matrix's rowptr[r] = rank(clamp(r - r0, 0, size)) and a reshaped vector's
    rowptr[r] = rank(r * ncols), its columns p % ncols"""
    rng = np.random.default_rng(12)
    for trial in range(60):
        n = int(rng.choice([1, 5, 63, 64, 65, 130]))
        p = rng.random(n) < rng.random()
        words = np.packbits(np.pad(p, (0, -n % 64)), bitorder="little").view(np.uint64)
        woff = np.concatenate([[0], np.cumsum([bin(int(w)).count("1") for w in words])])

        def rank(q):
            if q >= n:
                return int(woff[-1])
            return int(woff[q >> 6]) + bin(int(words[q >> 6]) & ((1 << (q & 63)) - 1)).count("1")

        assert [rank(q) for q in range(n + 1)] == np.concatenate([[0], np.cumsum(p)]).tolist()
        k = int(rng.integers(-70, 71))
        r0, c0 = max(-k, 0), max(k, 0)
        wrp, wci = csr_of(rm.diag_matrix((p, p), k)[0])
        assert [rank(min(max(r - r0, 0), n)) for r in range(n + abs(k) + 1)] == wrp.tolist()
        assert (np.flatnonzero(p) + c0).tolist() == wci.tolist()
        divs = [d for d in range(1, n + 1) if n % d == 0]
        nc = int(rng.choice(divs))
        wrp, wci = csr_of(rm.reshape((p, p), (n // nc, nc))[0])
        assert [rank(r * nc) for r in range(n // nc + 1)] == wrp.tolist()
        assert (np.flatnonzero(p) % nc).tolist() == wci.tolist()


def test_column_major_is_the_transposed_row_major_reshape():
    """a column-major reshape into nr' x nc' = the transpose of the row-major reshape of A' into nc' x nr'"""
    rng = np.random.default_rng(13)
    for trial in range(40):
        (nr, nc), (nr2, nc2) = random_shapes(rng)
        A = (rng.random((nr, nc)) < 0.4, rng.integers(0, 99, (nr, nc)))
        via = dm.transpose(rm.reshape(dm.transpose(A), (nc2, nr2)))
        want = rm.reshape(A, (nr2, nc2), "columnwise")
        assert np.array_equal(via[0], want[0]) and np.array_equal(via[1], want[1])


# ---------------------------------------------------------------------- the front end, before any call
def stub(name, shape=(7, 7)):
    """a Matrix (A), its transpose (A.T) or a Vector (v) without a handle"""
    import graphblas_amd as gb

    if name == "v":
        v = gb.Vector.__new__(gb.Vector)
        v.dtype, v.name, v._size, v._h = gb.dtypes.INT64, "v", shape[0], None
        return v
    A = gb.Matrix.__new__(gb.Matrix)
    A.dtype, A.name, A._nrows, A._ncols, A._h = gb.dtypes.INT64, "A", shape[0], shape[1], None
    return A.T if name == "A.T" else A


def test_shape_normalisation():
    from graphblas_amd import ss

    f = ss._reshape_shape
    assert f((8, 8), 4, 16) == (4, 16) and f((8, 8), 4, -1) == (4, 16) and f((8, 8), (-1, 16), None) == (4, 16)
    assert f((8, 8), (4, 16), None) == (4, 16) and f((8, 8), [2, 32], None) == (2, 32)
    assert f((49, 1), 7, 7) == (7, 7) and f((0, 5), 5, 0) == (5, 0) and f((0, 5), 0, 7) == (0, 7)
    assert f((70000, 70000), 4900000, -1) == (4900000, 1000)
    assert all(type(x) is int for x in f((8, 8), np.int64(4), np.int32(16)))
    for order, want in [("rowwise", "rowwise"), ("row", "rowwise"), ("rows", "rowwise"), ("C", "rowwise"),
                        ("columnwise", "columnwise"), ("col", "columnwise"), ("cols", "columnwise"),
                        ("column", "columnwise"), ("columns", "columnwise"), ("F", "columnwise")]:
        assert ss._order(order) == want
    assert [ss._diag_size(7, 7, k) for k in (0, 1, 3, 10, -1, -3, -10)] == [c["size"] for c in G["matrix_diag"]]
    assert [ss._diag_size(3, 4, k) for k in (-3, -2, 0, 1, 3, 4)] == [rm.diag_size(3, 4, k) for k in (-3, -2, 0, 1, 3, 4)]


@pytest.mark.parametrize("case", G["errors"], ids=ident)
def test_golden_argument_errors(case):
    x = stub(case["of"], tuple(case["shape"]))
    args = [tuple(a) if isinstance(a, list) else a for a in case["args"]]
    with pytest.raises(EXC[case["raises"]], match=case["match"]):
        getattr(x.ss, case["method"])(*args, **case["kwargs"])


def test_argument_errors_of_the_methods():
    import graphblas_amd as gb

    A, At, v = stub("A"), stub("A.T"), stub("v")
    with pytest.raises(TypeError, match=r"Bad type for argument `vector` in Matrix.ss.build_diag\(...\)"):
        A.ss.build_diag(A)
    with pytest.raises(TypeError, match="Expected type: Vector"):
        A.ss.build_diag(At)
    with pytest.raises(TypeError, match=r"Bad type for argument `matrix` in Vector.ss.build_diag\(...\)"):
        v.ss.build_diag(v)
    with pytest.raises(TypeError, match="Expected type: Matrix, TransposedMatrix"):
        v.ss.build_diag(3)
    with pytest.raises(TypeError, match=r"Bad type for argument `x` in graphblas.ss.diag\(...\)"):
        gb.ss.diag([1, 2])
    for bad in (1.5, "1", None, True):
        with pytest.raises(TypeError, match="k must be an integer"):
            v.diag(bad)
        with pytest.raises(TypeError, match="k must be an integer"):
            A.diag(bad)
        with pytest.raises(TypeError, match="k must be an integer"):
            At.diag(bad)
        with pytest.raises(TypeError, match="k must be an integer"):
            A.ss.build_diag(v, bad)
    with pytest.raises(ValueError, match="Bad value for order"):
        v.ss.reshape(7, 1, order="bad")
    with pytest.raises(ValueError, match="cannot reshape array of size 7 into shape"):
        v.ss.reshape(2, 4)
    with pytest.raises(ValueError, match="cannot reshape array"):
        A.ss.reshape(-1, 5, inplace=True)
    assert (A._nrows, A._ncols) == (7, 7)  # a refused in-place reshape leaves the shape alone
    with pytest.raises(ValueError, match="Shape tuple must be of length 2, not 1"):
        A.ss.reshape((49,))
    with pytest.raises(ValueError, match="Extra descriptor options"):
        v.ss.build_diag(A, 0, bogus=1)
