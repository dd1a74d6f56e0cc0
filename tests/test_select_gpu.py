"""GrB_select on the device (gb_select.hip) against numpy models: every positional and value
operator, the structure edges of the entry-parallel compaction (word boundaries, empty-row
runs, rows spanning words), iso inputs, vectors, the output side (mask / replace / accum /
aliasing / typecast), the _Scalar entry points, recorder strings, and triangle counting."""
import ctypes
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POSITIONAL = ["tril", "triu", "diag", "offdiag", "colle", "colgt", "rowle", "rowgt"]
VALUE = ["valueeq", "valuene", "valuegt", "valuege", "valuelt", "valuele"]
THUNKS = [-1000, -3, -1, 0, 1, 2, 1000]
NP_CMP = {"valueeq": np.equal, "valuene": np.not_equal, "valuegt": np.greater,
          "valuege": np.greater_equal, "valuelt": np.less, "valuele": np.less_equal}


@pytest.fixture(scope="module")
def gb():
    import graphblas_amd

    return graphblas_amd


@pytest.fixture(scope="module")
def golden_select():
    with open(os.path.join(ROOT, "tests", "golden", "select_golden.json")) as f:
        return json.load(f)


def positional_keep(op, i, j, k):
    return {"tril": j <= i + k, "triu": j >= i + k, "diag": j == i + k, "offdiag": j != i + k,
            "colle": j <= k, "colgt": j > k, "rowle": i <= k, "rowgt": i > k}[op]


def coo_of(P, V):
    """row-major triples of a dense (present, values) pair"""
    r, c = np.nonzero(P)
    return r, c, V[r, c]


def from_dense(gb, P, V, dtype=None):
    r, c, v = coo_of(P, V)
    return gb.Matrix.from_coo(r, c, v, dtype=dtype, nrows=P.shape[0], ncols=P.shape[1])


def assert_triples(M, r, c, v, *, exact_nan=False):
    gr, gc, gv = M.to_coo()
    assert M.nvals == len(r)
    assert np.array_equal(gr.astype(np.int64), np.asarray(r, np.int64))
    assert np.array_equal(gc.astype(np.int64), np.asarray(c, np.int64))
    assert np.array_equal(gv, np.asarray(v, gv.dtype), equal_nan=exact_nan and gv.dtype.kind == "f")


def assert_dense(M, P, V):
    r, c, v = coo_of(P, V)
    assert_triples(M, r, c, v)


def random_dense(rng, shape, density, lo=-50, hi=50):
    if density >= 1.0:
        P = np.ones(shape, bool)
    elif density <= 0.0:
        P = np.zeros(shape, bool)
    else:
        P = rng.random(shape) < density
    V = rng.integers(lo, hi, shape).astype(np.int64)
    return P, V


# ------------------------------------------------------------------ golden cases
def test_golden_matrix_cases(gb, golden_select):
    g = golden_select["A"]
    A = gb.Matrix.from_coo(g["rows"], g["cols"], g["vals"], nrows=g["nrows"], ncols=g["ncols"])
    for case in golden_select["matrix_cases"]:
        want = gb.Matrix.from_coo(case["rows"], case["cols"], case["vals"], nrows=7, ncols=7)
        for form, name, thunk in case["forms"]:
            if form == "op":
                got = [A.select(getattr(gb.select, name), thunk).new(),
                       A.select(getattr(gb.indexunary, name), thunk).new()]
            elif form == "call":
                got = [getattr(gb.select, name)(A, thunk).new()]
            else:
                got = [(A.select(name) if thunk is None else A.select(name, thunk)).new()]
            for w in got:
                assert w.isequal(want), (case["name"], form, name)
                assert w.dtype == A.dtype
    with pytest.raises(TypeError, match="thunk"):
        A.select(gb.select.valueeq, object())
    with pytest.raises(TypeError, match="thunk"):
        A.select(A.S, 3)


def test_golden_vector_cases(gb, golden_select):
    g = golden_select["v"]
    v = gb.Vector.from_coo(g["idx"], g["vals"], size=g["size"])
    for case in golden_select["vector_cases"]:
        want = gb.Vector.from_coo(case["idx"], case["vals"], size=g["size"])
        for form, name, thunk in case["forms"]:
            if form == "op":
                w = v.select(getattr(gb.select, name), thunk).new()
            elif form == "call":
                w = getattr(gb.select, name)(v, thunk).new()
            else:
                w = (v.select(name) if thunk is None else v.select(name, thunk)).new()
            assert w.isequal(want), (case["name"], form, name)
    with pytest.raises(TypeError, match="thunk"):
        v.select(gb.select.valueeq, object())
    A = gb.Matrix.from_coo([0], [0], [1], nrows=7, ncols=1)
    with pytest.raises(TypeError):
        v.select(A.S)


# ------------------------------------------------------------------ positional operators
# nvals: 0 (density 0), 1, 300 (not multiples of 64), 64 and 128 exactly (full 1x64 and 2x64), random
SHAPES = [(1, 1), (1, 300), (300, 1), (37, 53), (130, 70)]
# 600x500: enough entries that a wave marks a run of several chunks, each starting its row search
# where the last one ended
POS_CASES = [(s, d) for s in SHAPES for d in (0.0, 0.05, 0.6, 1.0)] + [((1, 64), 1.0), ((2, 64), 1.0),
                                                                        ((600, 500), 0.3), ((3000, 40), 0.02)]


@pytest.mark.parametrize("shape,density", POS_CASES)
def test_positional_against_numpy(gb, shape, density):
    rng = np.random.default_rng(shape[0] * 1000 + shape[1] + int(density * 100))
    P, V = random_dense(rng, shape, density)
    if shape == (2, 64):
        assert P.sum() == 128
    if shape == (1, 64):
        assert P.sum() == 64
    A = from_dense(gb, P, V)
    I, J = np.indices(shape)
    It, Jt = np.indices(shape[::-1])
    for op in POSITIONAL:
        for k in THUNKS:
            got = A.select(op, k).new()
            assert_dense(got, P & positional_keep(op, I, J, k), V)
            got = A.T.select(getattr(gb.select, op), k).new()
            assert got.shape == shape[::-1]
            assert_dense(got, P.T & positional_keep(op, It, Jt, k), V.T)


# ------------------------------------------------------------------ structure edges
def edge_matrices():
    # first 70, a middle 70 and the last 70 rows empty: empty-row runs cross word boundaries and
    # rowptr[i] == nvals occurs for the trailing rows
    rows = np.concatenate([np.repeat(np.arange(70, 75), 30), np.repeat(np.arange(145, 150), 30)])
    cols = np.tile(np.arange(30), 10) * 3
    yield "empty_runs", rows, cols, 220, 100
    # one row of 200 entries (spans 4 words), then rows of length 1
    rows = np.concatenate([np.zeros(200, np.int64), np.arange(1, 41)])
    cols = np.concatenate([np.arange(200), np.arange(1, 41) * 3 % 200])
    yield "long_row", rows, cols, 41, 200
    # a row boundary exactly at entry 64, nvals = 128 (the word after the last is indexed)
    rows = np.concatenate([np.zeros(64, np.int64), np.full(40, 1), np.full(24, 3)])
    cols = np.concatenate([np.arange(64), np.arange(40), np.arange(24) * 2])
    yield "boundary_64", rows, cols, 5, 64


@pytest.mark.parametrize("name,rows,cols,nr,nc", list(edge_matrices()), ids=[e[0] for e in edge_matrices()])
def test_structure_edges(gb, name, rows, cols, nr, nc):
    rng = np.random.default_rng(5)
    vals = rng.integers(-9, 9, rows.size)
    A = gb.Matrix.from_coo(rows, cols, vals, nrows=nr, ncols=nc)
    order = np.lexsort((cols, rows))
    rows, cols, vals = rows[order], cols[order], vals[order]
    for op, k in [("tril", 0), ("tril", 60), ("triu", 1), ("offdiag", 0), ("colle", 17), ("colgt", 40),
                  ("rowle", 72), ("rowgt", 0), ("rowgt", 146), (">", 0), ("!=", 3), ("diag", -70)]:
        if op in POSITIONAL:
            keep = positional_keep(op, rows, cols, k)
        else:
            keep = vals > 0 if op == ">" else vals != 3
        got = A.select(op, k).new()
        assert got.nvals == int(keep.sum()), (name, op, k)
        assert_triples(got, rows[keep], cols[keep], vals[keep])  # in order: rowptr is right
        # a second select on the result reads the new rowptr
        again = got.select("triu", -5).new()
        keep2 = keep & (cols >= rows - 5)
        assert_triples(again, rows[keep2], cols[keep2], vals[keep2])
        csr = got.to_csr()[0]
        assert np.array_equal(csr, np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=nr))]))


# ------------------------------------------------------------------ value operators x dtypes
DTYPES = ["BOOL", "INT8", "UINT8", "INT16", "UINT16", "INT32", "UINT32", "INT64", "UINT64", "FP32", "FP64"]


def value_fixture(dtype):
    """(values array 37x53 of the numpy type, thunks): thunks that occur, that do not, and the
    extremes of the type"""
    rng = np.random.default_rng(DTYPES.index(dtype) + 100)
    shape = (37, 53)
    if dtype == "BOOL":
        return rng.random(shape) < 0.5, [True, False]
    npt = np.dtype({"FP32": "float32", "FP64": "float64"}.get(dtype, dtype.lower()))
    if npt.kind == "f":
        V = (rng.integers(-6, 6, shape) * 0.5).astype(npt)  # includes +0.0; 0.25 never occurs
        V[0, :5] = np.nan
        V[1, :5] = -0.0
        V[2, :5] = 0.0
        fi = np.finfo(npt)
        return V, [npt.type(0.0), npt.type(-0.0), npt.type(1.5), npt.type(0.25), fi.max, fi.min,
                   npt.type(np.inf), npt.type(-np.inf)]
    ii = np.iinfo(npt)
    V = rng.integers(max(ii.min, -20), min(ii.max, 20), shape).astype(npt)
    V[0, :4] = ii.max
    V[1, :4] = ii.min
    if dtype == "UINT64":
        V[2, :6] = np.uint64(2**63) + rng.integers(0, 1000, 6).astype(np.uint64)
        extra = [npt.type(2**63), npt.type(2**63 + 500)]
    else:
        extra = []
    return V, [npt.type(3), npt.type(0), npt.type(17 if ii.max > 17 else 1), npt.type(ii.max // 2 + 1),
               npt.type(ii.max), npt.type(ii.min)] + extra


@pytest.mark.parametrize("dtype", DTYPES)
def test_value_operators_every_dtype(gb, dtype):
    V, thunks = value_fixture(dtype)
    rng = np.random.default_rng(9)
    P = rng.random(V.shape) < 0.55
    P[:3, :6] = True  # the planted extremes / NaN / zeros are present
    A = from_dense(gb, P, V, dtype=dtype)
    assert A.dtype == dtype
    r, c, v = coo_of(P, V)
    for op in VALUE:
        for y in thunks:
            typed = getattr(gb.select, op)[dtype]
            assert typed.gb_name == f"GrB_{op.upper()}_{dtype}"
            got = A.select(typed, y).new()
            with np.errstate(invalid="ignore"):
                keep = NP_CMP[op](v, y)
            assert_triples(got, r[keep], c[keep], v[keep], exact_nan=True)
    if dtype in ("FP32", "FP64"):
        nan = np.isnan(v)
        assert nan.sum() == 5
        eq0 = A.select("==", V.dtype.type(0.0)).new().to_coo()[2]
        assert not np.isnan(eq0).any() and (eq0 == 0).all()
        assert np.signbit(eq0).sum() == 5 and eq0.size == int((v == 0).sum())  # both zeros kept
        for y in thunks:
            assert not np.isnan(A.select("==", y).new().to_coo()[2]).any()
            assert np.isnan(A.select("!=", y).new().to_coo()[2]).sum() == 5
    if dtype == "BOOL":
        got = A.select(gb.select.valueeq, True).new()
        assert got.nvals == int(v.sum()) and got.to_coo()[2].all()


def test_mixed_type_keeps_the_original_values(gb):
    # INT8 matrix, GrB_VALUEGT_FP64, thunk 2.5: the comparison is in FP64, T keeps A's INT8 values
    rng = np.random.default_rng(11)
    P, V = random_dense(rng, (37, 53), 0.5, -5, 6)
    A = from_dense(gb, P, V, dtype="INT8")
    C = gb.Matrix("INT8", 37, 53)
    lib = gb.lib
    assert lib.GrB_Matrix_select_FP64(C._h, None, None, lib.GrB_VALUEGT_FP64, A._h, 2.5, None) == 0
    assert_dense(C, P & (V > 2.5), V.astype(np.int8))
    assert C.to_coo()[2].dtype == np.int8
    # the front end unifies INT8 with the FP64 thunk the same way
    got = A.select(">", 2.5).new()
    assert got.dtype == "INT8" and got.isequal(C)


# ------------------------------------------------------------------ iso
def matrix_is_iso(gb, A):
    from graphblas_amd.device import matrix_view

    return bool(matrix_view(A._h).iso)


def test_iso_matrix(gb):
    rng = np.random.default_rng(13)
    P, _ = random_dense(rng, (37, 53), 0.6)
    r, c = np.nonzero(P)
    A = gb.Matrix.from_coo(r, c, 7, dtype="INT32", nrows=37, ncols=53)
    assert matrix_is_iso(gb, A)
    V = np.full(P.shape, 7, np.int32)
    I, J = np.indices(P.shape)
    L = A.select("tril", 2).new()
    assert matrix_is_iso(gb, L)
    assert_dense(L, P & (J <= I + 2), V)
    allkept = A.select("==", 7).new()
    assert matrix_is_iso(gb, allkept) and allkept.isequal(A)
    assert A.select("!=", 7).new().nvals == 0
    assert A.select(">", 7).new().nvals == 0


# ------------------------------------------------------------------ vectors
@pytest.mark.parametrize("n", [1, 63, 64, 65, 200])
@pytest.mark.parametrize("full", [False, True])
def test_vectors(gb, n, full):
    rng = np.random.default_rng(n * 2 + full)
    present = np.ones(n, bool) if full else rng.random(n) < 0.5
    vals = rng.integers(-4, 5, n)
    idx = np.nonzero(present)[0]
    v = gb.Vector.from_coo(idx, vals[idx], size=n)

    def check(w, keep):
        gi, gv = w.to_coo()
        assert w.nvals == int(keep.sum()) and w.size == n
        assert np.array_equal(gi.astype(np.int64), idx[keep]) and np.array_equal(gv, vals[idx][keep])

    for k in [-1, 0, 1, 62, 63, 64, 130, 1000]:
        check(v.select(gb.select.rowle, k).new(), idx <= k)
        check(v.select(gb.select.rowgt, k).new(), idx > k)
        check(v.select("index<=", k).new(), idx <= k)
        check(v.select("index>", k).new(), idx > k)
        check(v.select("tril", k).new(), 0 <= idx + k)  # j = 0
        check(v.select("col<=", k).new(), np.full(idx.size, 0 <= k))
    for op in VALUE:
        for y in [-9, -1, 0, 2, 9]:
            check(v.select(getattr(gb.select, op), y).new(), NP_CMP[op](vals[idx], y))
    # iso vector: stays iso, values right
    from graphblas_amd.device import vector_view

    u = gb.Vector.from_coo(idx, 3, dtype="INT16", size=n)
    w = u.select("index<=", n // 2).new()
    assert w.nvals == int((idx <= n // 2).sum())
    if w.nvals:
        assert (w.to_coo()[1] == 3).all()
        assert vector_view(u._h).iso and vector_view(w._h).iso
    assert u.select("==", 3).new().isequal(u)
    assert u.select("!=", 3).new().nvals == 0


# ------------------------------------------------------------------ output side
def model_write(Cp, Cv, Tp, Tv, Mp=None, Mv=None, *, comp=False, struct=False, replace=False, accum=False):
    """C<M, replace> = C accum T on dense (present, values) pairs"""
    allow = np.ones(Cp.shape, bool) if Mp is None else (Mp if struct else Mp & (Mv != 0))
    if comp:
        allow = ~allow
    if accum:
        Zp, Zv = Cp | Tp, np.where(Cp & Tp, Cv + Tv, np.where(Tp, Tv, Cv))
    else:
        Zp, Zv = Tp, Tv
    outp = np.where(allow, Zp, False if replace else Cp)
    return outp, np.where(allow, Zv, Cv)


@pytest.fixture(scope="module")
def outside(gb):
    rng = np.random.default_rng(17)
    Ap, Av = random_dense(rng, (37, 53), 0.5)
    Cp, Cv = random_dense(rng, (37, 53), 0.4)
    Mp, Mv = random_dense(rng, (37, 53), 0.5, 0, 2)  # values 0 / 1: explicit zeros
    I, J = np.indices((37, 53))
    Tp = Ap & (J <= I)
    return dict(Ap=Ap, Av=Av, Cp=Cp, Cv=Cv, Mp=Mp, Mv=Mv, Tp=Tp)


def test_output_mask_replace_accum(gb, outside):
    o = outside
    A = from_dense(gb, o["Ap"], o["Av"])
    M = from_dense(gb, o["Mp"], o["Mv"])
    expr = lambda: A.select("tril", 0)  # noqa: E731
    C = from_dense(gb, o["Cp"], o["Cv"])
    C(M.S) << expr()
    assert_dense(C, *model_write(o["Cp"], o["Cv"], o["Tp"], o["Av"], o["Mp"], o["Mv"], struct=True))
    C = from_dense(gb, o["Cp"], o["Cv"])
    C(~M.S, replace=True) << expr()
    assert_dense(C, *model_write(o["Cp"], o["Cv"], o["Tp"], o["Av"], o["Mp"], o["Mv"], struct=True, comp=True,
                                 replace=True))
    C = from_dense(gb, o["Cp"], o["Cv"])
    C(M.V) << expr()
    assert_dense(C, *model_write(o["Cp"], o["Cv"], o["Tp"], o["Av"], o["Mp"], o["Mv"]))
    C = from_dense(gb, o["Cp"], o["Cv"])
    C(accum=gb.binary.plus) << expr()
    assert_dense(C, *model_write(o["Cp"], o["Cv"], o["Tp"], o["Av"], accum=True))


def test_output_alias_and_typecast(gb, outside):
    o = outside
    A = from_dense(gb, o["Ap"], o["Av"])
    A << A.select("tril", 0)  # the output is the input
    assert_dense(A, o["Tp"], o["Av"])
    A = from_dense(gb, o["Ap"], o["Av"])
    A << A.select("==", 1000)  # nothing kept
    assert A.nvals == 0
    Q = from_dense(gb, o["Ap"][:37, :37], o["Av"][:37, :37])
    Q << Q.T.select("tril", -1)  # the output is the input of the transposed view
    assert_dense(Q, o["Ap"][:37, :37].T & np.tril(np.ones((37, 37), bool), -1), o["Av"][:37, :37].T)
    B = from_dense(gb, o["Ap"], o["Av"])
    assert B.dtype == "INT64"
    C = B.select("tril", 0).new(dtype="FP64")
    assert C.dtype == "FP64" and C.to_coo()[2].dtype == np.float64
    assert_dense(C, o["Tp"], o["Av"].astype(np.float64))
    B << B.select(">=", -1000)  # everything kept while aliased: T is a copy
    assert_dense(B, o["Ap"], o["Av"])


def test_mask_forms(gb, outside):
    o = outside
    A = from_dense(gb, o["Ap"], o["Av"])
    M = from_dense(gb, o["Mp"], o["Mv"])
    assert (o["Mp"] & (o["Mv"] == 0)).any()  # M holds explicit zeros
    assert_dense(A.select(M.S).new(), o["Ap"] & o["Mp"], o["Av"])
    assert_dense(A.select(M.V).new(), o["Ap"] & o["Mp"] & (o["Mv"] != 0), o["Av"])
    # under accum there is no replace: C keeps what the mask does not select
    C = from_dense(gb, o["Cp"], o["Cv"])
    C(accum=gb.binary.plus) << A.select(M.S)
    assert_dense(C, *model_write(o["Cp"], o["Cv"], o["Ap"], o["Av"], o["Mp"], o["Mv"], struct=True, accum=True))
    # with a mask on the updater: C<K> = A.dup(mask=M)
    K = from_dense(gb, o["Tp"], o["Av"])
    C = from_dense(gb, o["Cp"], o["Cv"])
    C(K.S) << A.select(M.V)
    assert_dense(C, *model_write(o["Cp"], o["Cv"], o["Ap"] & o["Mp"] & (o["Mv"] != 0), o["Av"], o["Tp"], o["Av"],
                                 struct=True))
    with pytest.raises(TypeError, match="thunk"):
        A.select(M.S, 1)
    v = gb.Vector.from_coo([1], [1], size=37)
    with pytest.raises(TypeError):
        A.select(v.S)
    # vectors
    u = gb.Vector.from_coo([0, 2, 5, 9], [4, 5, 6, 7], size=12)
    m = gb.Vector.from_coo([2, 5, 7], [1, 0, 1], size=12)
    got = u.select(m.S).new()
    assert np.array_equal(got.to_coo()[0], [2, 5]) and np.array_equal(got.to_coo()[1], [5, 6])
    got = u.select(m.V).new()
    assert np.array_equal(got.to_coo()[0], [2]) and np.array_equal(got.to_coo()[1], [5])


# ------------------------------------------------------------------ _Scalar entry points, errors
def test_scalar_entry_points(gb, outside):
    o = outside
    lib = gb.lib
    A = from_dense(gb, o["Ap"], o["Av"])
    typed = gb.Matrix("INT64", 37, 53)
    assert lib.GrB_Matrix_select_INT64(typed._h, None, None, lib.GrB_VALUEGT_INT64, A._h, 4, None) == 0
    s = gb.Scalar.from_value(4, "INT64")
    C = gb.Matrix("INT64", 37, 53)
    assert lib.GrB_Matrix_select_Scalar(C._h, None, None, lib.GrB_VALUEGT_INT64, A._h, s._h, None) == 0
    assert C.isequal(typed) and C.nvals == int((o["Ap"] & (o["Av"] > 4)).sum())
    # the front end takes the same route for a Scalar thunk
    with gb.Recorder() as rec:
        D = A.select(">", s).new(name="D")
    assert D.isequal(typed)
    assert rec.data[-1] == f"GrB_Matrix_select_Scalar(D, NULL, NULL, GrB_VALUEGT_INT64, {A.name}, {s.name}, NULL);"
    empty = gb.Scalar("INT64")
    assert lib.GrB_Matrix_select_Scalar(C._h, None, None, lib.GrB_VALUEGT_INT64, A._h, empty._h, None) \
        == lib.GrB_EMPTY_OBJECT
    assert C.isequal(typed)  # untouched
    # vectors
    u = gb.Vector.from_coo([0, 2, 5, 9], [4, 5, 6, 7], size=12)
    w = gb.Vector("INT64", 12)
    assert lib.GrB_Vector_select_Scalar(w._h, None, None, lib.GrB_VALUEGT_INT64, u._h, s._h, None) == 0
    assert np.array_equal(w.to_coo()[0], [2, 5, 9])
    assert lib.GrB_Vector_select_Scalar(w._h, None, None, lib.GrB_VALUEGT_INT64, u._h, empty._h, None) \
        == lib.GrB_EMPTY_OBJECT
    # dimension mismatch: reported on the output
    bad = gb.Matrix("INT64", 53, 37)
    assert lib.GrB_Matrix_select_INT64(bad._h, None, None, lib.GrB_TRIL, A._h, 0, None) \
        == lib.GrB_DIMENSION_MISMATCH
    msg = ctypes.c_char_p()
    assert lib.GrB_Matrix_error(ctypes.byref(msg), bad._h) == 0
    assert msg.value and b"dimension" in msg.value
    assert lib.GrB_Matrix_select_INT64(bad._h, None, None, lib.GrB_TRIL, A._h, 0, lib.GrB_DESC_T0) == 0
    assert bad.nvals == int((o["Ap"].T & np.tril(np.ones((53, 37), bool))).sum())
    with pytest.raises(gb.DimensionMismatch):
        bad << A.select("tril")
    # a null operator
    assert lib.GrB_Matrix_select_INT64(C._h, None, None, None, A._h, 0, None) == lib.GrB_NULL_POINTER


def test_recorder_strings(gb):
    A = gb.Matrix.from_coo([0, 1, 2], [1, 2, 0], [1, 2, 3], nrows=3, ncols=3, name="A")
    v = gb.Vector.from_coo([0, 2], [1.5, 2.5], size=3, name="v")
    C = gb.Matrix("INT64", 3, 3, name="C")
    w = gb.Vector("FP64", 3, name="w")
    with gb.Recorder() as rec:
        C << A.select(gb.select.tril, -1)
        C << A.T.select("triu", 1)
        w << v.select(">", 2.0)
    assert rec.data == [
        "GrB_Matrix_select_INT64(C, NULL, NULL, GrB_TRIL, A, -1, NULL);",
        "GrB_Matrix_select_INT64(C, NULL, NULL, GrB_TRIU, A, 1, GrB_DESC_T0);",
        "GrB_Vector_select_FP64(w, NULL, NULL, GrB_VALUEGT_FP64, v, 2.0, NULL);",
    ]


# ------------------------------------------------------------------ triangle counting
def count_triangles(gb, A):
    L = A.select("tril", -1).new()
    C = L.mxm(L.T, gb.semiring.plus_pair).new(mask=L.S)
    return C.reduce_scalar(gb.monoid.plus).new().value or 0


def test_triangle_count_dense_graph(gb):
    rng = np.random.default_rng(23)
    n = 200
    B = rng.random((n, n)) < 0.08
    loops = [3, 64, 65, 199]
    B[loops, loops] = True  # planted self-loops, stripped by offdiag
    r, c = np.nonzero(B)
    H = gb.Matrix.from_coo(r, c, np.ones(r.size, np.int64), nrows=n, ncols=n)
    S = H.ewise_add(H.T, gb.binary.max).new()  # A | A'
    A = S.select("offdiag").new()
    D = (B | B.T) & ~np.eye(n, dtype=bool)
    assert A.nvals == int(D.sum()) and S.nvals == int((B | B.T).sum())
    Di = D.astype(np.int64)
    want = int(np.trace(Di @ Di @ Di)) // 6
    assert want > 0
    assert count_triangles(gb, A) == want


def test_triangle_count_rmat(gb):
    import scipy.sparse as sp

    from graphblas_amd.matrix import Matrix

    scale = 12
    n = 1 << scale
    R = Matrix.__new__(Matrix)
    R.dtype, R.name, R._h, R._nrows, R._ncols = gb.INT64, "R", ctypes.c_void_p(), n, n
    assert gb.lib.GxB_Matrix_rmat(ctypes.byref(R._h), scale, 16, 42, 1, 2, 0, 0) == 0
    S = R.ewise_add(R.T, gb.binary.first).new()
    A = S.select("offdiag").new()
    r, c, _ = R.to_coo()
    G = sp.csr_matrix((np.ones(r.size, np.int64), (r.astype(np.int64), c.astype(np.int64))), shape=(n, n))
    G = ((G + G.T) > 0).astype(np.int64)
    G.setdiag(0)
    G.eliminate_zeros()
    assert A.nvals == G.nnz
    Ls = sp.tril(G, -1).tocsr()
    want = int((Ls @ Ls.T).multiply(Ls).sum())
    assert want > 0
    assert count_triangles(gb, A) == want
