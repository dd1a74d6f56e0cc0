"""GrB_apply with an index-unary operator on the device (gb_apply_index.hip) against the numpy
model of tests/index_apply_model.py, and GrB_select with the index-valued operators.  The results
are integers and booleans: every comparison is exact, through to_coo() (test_general_ops_gpu.check:
structure, order, nvals, dtype, values).

Shapes, and the path each one is for
  rows 70 x 300   rows of 0, 1, 63, 64, 65, 128, 129 and 300 entries: row boundaries on, before and
                  after a 64-entry wave step and a 256-entry chunk, one row across two chunks
  20000 x 70      0..3 entries per row: about 170 row boundaries per chunk, so every lane searches
                  its own row; a run of 300 empty rows that starts exactly on a chunk boundary, so the
                  bound carried from the chunk before is more than 64 rows short
  600 x 500       rows of about 150 entries: a wave owns a run of chunks whose few boundaries sit
                  one per lane and whose search starts where the last one ended
  3 x 300         nvals 0, 1, 63, 64, 65, 256, 257: the last wave step and the last chunk
  vectors         1, 63, 64, 65, 4097: a partial last bitmap word, more than one block
"""
import ctypes
import json
import os

import numpy as np
import pytest

import dense_model as dm
import index_apply_model as im
import indexing_cases as ic
from test_general_ops_gpu import check, to_gb
from test_indexing_gpu import bind, dev, is_iso

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THUNKS = [-1000, -3, 0, 2, 1000]
EMPTY_OBJECT, DIMENSION_MISMATCH, NULL_POINTER = -106, -6, -2


@pytest.fixture(scope="module")
def gb():
    import graphblas_amd

    return graphblas_amd


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "index_apply_golden.json")) as f:
        return json.load(f)


def chunks_per_wave(nvals):
    """the launch arithmetic of the matrix kernel: chunks of 4 x 64 entries, a block of 4 waves for
    every 16 chunks (at most 8192 blocks), the chunks dealt to the waves in contiguous runs"""
    chunks = -(-nvals // 256)
    blocks = min(max(-(-(-(-chunks // 4)) // 4), 1), 8192)
    return -(-chunks // (4 * blocks))


def typed(gb, op, optype):
    """the front-end operator of a model (name, type) pair"""
    if op in im.POSITIONAL:
        return getattr(gb.select, op)
    return getattr(gb.indexunary, op)[optype]


def run_both(gb, A, a, op, optype, y, what):
    """a.apply(op, y) and a.T.apply(op, y) against the model of A and of its transpose"""
    t, zt = typed(gb, op, optype), im.result_dtype(op, optype)
    check(a.apply(t, y).new(), im.index_apply(A, op, optype, y), zt, what=f"{what} {op}[{optype}] y={y}")
    check(a.T.apply(t, y).new(), im.index_apply(dm.transpose(A), op, optype, y), zt,
          what=f"{what} T0 {op}[{optype}] y={y}")


# ------------------------------------------------------------------ golden cases
def forms_of(gb, x, form, name, thunk):
    iu = gb.indexunary
    if form == "str":
        return x.apply(name) if thunk is None else x.apply(name, thunk)
    if form == "op":
        return x.apply(getattr(iu, name)) if thunk is None else x.apply(getattr(iu, name), thunk)
    if form == "call":
        return getattr(iu, name)(x)
    if form == "call_thunk_kw":
        return getattr(iu, name)(x, thunk=thunk)
    s = gb.Scalar.from_value(thunk, "INT64")
    if form == "op_scalar":
        return x.apply(getattr(iu, name), s)
    if form == "selectop_scalar":
        return x.apply(getattr(gb.select, name), s)
    if form == "str_scalar":
        return x.apply(name, s)
    assert form == "call_scalar"
    return getattr(iu, name)(x, s)


def test_golden_matrix_cases(gb, golden):
    g = golden["A"]
    A = gb.Matrix.from_coo(g["rows"], g["cols"], g["vals"], nrows=g["nrows"], ncols=g["ncols"])
    for case in golden["matrix_cases"]:
        want = gb.Matrix.from_coo(case["rows"], case["cols"], case["vals"], dtype=case["dtype"], nrows=7, ncols=7)
        assert want.nvals == A.nvals  # the structure of A, zeros and falses included
        for form, name, thunk in case["forms"]:
            w = forms_of(gb, A, form, name, thunk).new()
            assert w.dtype == case["dtype"], (case["name"], form)
            assert w.isequal(want, check_dtype=True), (case["name"], form, case["src"])
            assert np.array_equal(w.to_coo()[2], want.to_coo()[2]) and w.nvals == want.nvals
    with pytest.raises(TypeError, match="left"):
        A.apply(gb.select.valueeq, left=gb.Scalar.from_value(3, "INT64"))
    with pytest.raises(TypeError, match="left"):
        A.apply(gb.indexunary.rowindex, left=1)
    with pytest.raises(TypeError, match="left"):
        A.apply("colindex", left=1)


def test_golden_vector_cases(gb, golden):
    g = golden["v"]
    v = gb.Vector.from_coo(g["idx"], g["vals"], size=g["size"])
    for case in golden["vector_cases"]:
        want = gb.Vector.from_coo(case["idx"], case["vals"], dtype=case["dtype"], size=g["size"])
        for form, name, thunk in case["forms"]:
            w = forms_of(gb, v, form, name, thunk).new()
            assert w.dtype == case["dtype"], (case["name"], form)
            assert w.isequal(want, check_dtype=True), (case["name"], form, case["src"])
            assert np.array_equal(w.to_coo()[1], want.to_coo()[1]) and w.nvals == want.nvals
    with pytest.raises(TypeError, match="left"):
        v.apply(gb.indexunary.valueeq, left=gb.Scalar.from_value(2, "INT64"))


def test_unchanged_apply_forms(gb):
    A = gb.Matrix.from_coo([0, 1], [1, 0], [3, 4], nrows=2, ncols=2)
    with gb.Recorder() as rec:
        w = A.apply("==", 3).new(name="w")  # still the binary operator, bound second
    assert rec.data[-1] == f"GrB_Matrix_apply_BinaryOp2nd_INT64(w, NULL, NULL, GrB_EQ_INT64, {A.name}, 3, NULL);"
    assert w.dtype == "BOOL" and w.to_coo()[2].tolist() == [True, False]
    with pytest.raises(NotImplementedError):
        A.apply(gb.binary.firsti, right=1)


# ------------------------------------------------------------------ every operator
@pytest.mark.parametrize("optype", ["INT32", "INT64", None])
def test_positional_operators_on_rows(gb, optype):
    A = ic.matrix_named("rows", "INT32" if optype == "INT32" else "INT64")
    a = to_gb(gb, A)
    for op in (im.POSITIONAL if optype is None else im.INDEX):
        for y in THUNKS:
            run_both(gb, A, a, op, optype, y, "rows")
    if optype is not None:
        # the untyped operator resolves on the input: INT32 -> INT32, anything else -> INT64
        w = a.apply("diagindex", 7).new()
        check(w, im.index_apply(A, "diagindex", optype, 7), optype, what="untyped diagindex")


@pytest.mark.parametrize("dt", dm.ALL)
def test_value_operators_on_rows(gb, dt):
    A = ic.matrix_named("rows", dt)
    a = to_gb(gb, A)
    assert a.dtype == dt
    for op in im.VALUE:
        for y in THUNKS:
            run_both(gb, A, a, op, dt, y, "rows")
    # a thunk that occurs: the first stored value
    y = A[1][A[0]][0]
    if y == y:
        want = im.index_apply(A, "valueeq", dt, y)
        assert want[1].any()
        check(a.apply(gb.indexunary.valueeq[dt], y).new(), want, "BOOL", what=f"valueeq[{dt}] stored value")


def test_value_operator_of_another_type(gb):
    # INT8 entries under GrB_VALUEGT_FP64 with thunk 2.5: the entry and the thunk are cast to FP64
    A = ic.matrix_named("small", "INT8")
    a = to_gb(gb, A)
    C = gb.Matrix("BOOL", 70, 90)
    lib = gb.lib
    assert lib.GrB_Matrix_apply_IndexOp_FP64(C._h, None, None, lib.GrB_VALUEGT_FP64, a._h, 2.5, None) == 0
    check(C, im.index_apply(A, "valuegt", "FP64", 2.5), "BOOL", what="valuegt[FP64] on INT8")
    # the front end unifies INT8 with the FP64 thunk the same way
    assert a.apply(gb.indexunary.valuegt, 2.5).new().isequal(C, check_dtype=True)


# ------------------------------------------------------------------ per-lane search, carried bound
def ragged_with_gap():
    """20000 x 70, 0..3 entries per row, rows 9000..9299 and the last row empty, and the entries
    before row 9000 a multiple of 256: the chunk that follows them starts at row 9300, 301 row
    pointers past where the search of the chunk before ended (gb_wave_upper looks at 64).
    About 30000 entries are 118 chunks of 256; the launch takes ceil(ceil(118 / 4) / 4) = 8 blocks
    of 4 waves, so a wave owns ceil(118 / 32) = 4 chunks, and a chunk spans about 170 rows: more
    than the 63 boundaries a wave holds one per lane, so every lane searches for its own row."""
    p = ic._ragged(ic.rng_of("index_apply", "gap"), 20000, 70)
    p[9000:9300] = False
    p[-1] = False
    r, c = np.nonzero(p[:9000])
    extra = r.size % 256
    p[r[:extra], c[:extra]] = False
    assert p[:9000].sum() % 256 == 0 and p[:9000].sum() > 0 and p[9300:].sum() > 256
    assert chunks_per_wave(int(p.sum())) == 4 and p.sum() / 256 * 63 < p.any(axis=1).sum()
    return p


def test_per_lane_search_and_carried_bound(gb):
    p = ragged_with_gap()
    A = p, np.where(p, np.int64(1), np.int64(0))
    a = to_gb(gb, A)
    for op, y in [("rowindex", 0), ("diagindex", 5), ("rowindex", -9300), ("tril", 9000)]:
        optype = None if op == "tril" else "INT64"
        check(a.apply(typed(gb, op, optype), y).new(), im.index_apply(A, op, optype, y),
              im.result_dtype(op, optype), what=f"gap {op} y={y}")
    at = a.T.apply(gb.indexunary.rowindex).new()  # 70 hub rows of about 430 entries
    check(at, im.index_apply(dm.transpose(A), "rowindex", "INT64", 0), "INT64", what="gap T0 rowindex")


def test_run_of_chunks_with_boundaries_per_lane(gb):
    # 600 x 500 at density 0.3: about 90000 entries are 352 chunks; ceil(ceil(352 / 4) / 4) = 22
    # blocks of 4 waves, so a wave owns ceil(352 / 88) = 4 chunks, each with one or two row
    # boundaries (rows of about 150 entries), found where the chunk before stopped
    rng = ic.rng_of("index_apply", "run")
    p = rng.random((600, 500)) < 0.3
    p[100:103] = False  # three empty rows inside a wave's run
    assert chunks_per_wave(int(p.sum())) == 4
    A = p, np.where(p, rng.integers(-5, 5, p.shape), 0)
    a = to_gb(gb, A)
    for op, optype, y in [("rowindex", "INT64", 1), ("diagindex", "INT64", -2), ("offdiag", None, 3),
                          ("colindex", "INT64", 4), ("valuelt", "INT64", 0)]:
        run_both(gb, A, a, op, optype, y, "run")


# ------------------------------------------------------------------ edges
@pytest.mark.parametrize("nvals", [0, 1, 63, 64, 65, 256, 257])
def test_nvals_edges(gb, nvals):
    rng = ic.rng_of("index_apply", "edge", nvals)
    p = np.zeros((3, 300), bool)
    p.ravel()[rng.permutation(900)[:nvals]] = True
    A = p, np.where(p, rng.integers(-3, 4, p.shape), 0)
    a = to_gb(gb, A)
    assert a.nvals == nvals
    for op, optype, y in [("rowindex", "INT64", 2), ("colindex", "INT64", -1), ("diagindex", "INT64", 0),
                          ("triu", None, 1), ("valueeq", "INT64", 0)]:
        run_both(gb, A, a, op, optype, y, f"nvals={nvals}")


@pytest.mark.parametrize("name", ["one", "empty"])
def test_one_by_one_and_only_empty_rows(gb, name):
    A = ic.matrix_named(name, "INT64")
    a = to_gb(gb, A)
    for op, optype, y in [("rowindex", "INT64", 5), ("diagindex", "INT32", -5), ("diag", None, 0),
                          ("valuene", "INT64", 0)]:
        run_both(gb, A, a, op, optype, y, name)


# ------------------------------------------------------------------ vectors
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
@pytest.mark.parametrize("kind", ["sparse", "full", "empty", "iso"])
def test_vectors(gb, n, kind):
    U = ic.obj("INT16", (n,), ("index_apply", n), kind=kind)
    u = dev(gb, U, kind)
    iu = gb.indexunary
    for t, op, optype, y in [(iu.index, "rowindex", "INT64", 3), ("index", "rowindex", "INT64", 0),
                             (iu.colindex, "colindex", "INT64", 7),       # the constant y
                             (iu.diagindex, "diagindex", "INT64", 100),   # y - i
                             (iu.rowindex["INT32"], "rowindex", "INT32", 2**31 - 64),
                             (gb.select.rowle, "rowle", None, 63),
                             (iu.valuegt["INT16"], "valuegt", "INT16", 0),
                             (iu.valueeq, "valueeq", "INT16", ic.iso_value("INT16"))]:
        w = u.apply(t, y).new()
        check(w, im.index_apply(U, op, optype, y), im.result_dtype(op, optype), what=f"{kind} n={n} {op} y={y}")
        if kind == "iso" and U[0].any():
            assert is_iso(u)
            assert is_iso(w) == (op in im.VALUE), f"{op}: a value operator evaluates once, a positional one per entry"


# ------------------------------------------------------------------ iso matrices
def test_iso_matrix(gb):
    A = ic.matrix_named("rows", "INT32", kind="iso")
    a = dev(gb, A, "iso")
    assert is_iso(a)
    for op, optype, y in [("rowindex", "INT32", 1), ("colindex", "INT64", 0), ("diagindex", "INT64", 0),
                          ("tril", None, 0)]:
        w = a.apply(typed(gb, op, optype), y).new()
        assert not is_iso(w)
        check(w, im.index_apply(A, op, optype, y), im.result_dtype(op, optype), what=f"iso {op}")
    x = ic.iso_value("INT32")
    for op, y in [("valueeq", x), ("valuene", x), ("valuegt", 0), ("valuelt", 0)]:
        for obj, M in ((a, A), (a.T, dm.transpose(A))):
            w = obj.apply(typed(gb, op, "INT32"), y).new()
            assert is_iso(w)
            check(w, im.index_apply(M, op, "INT32", y), "BOOL", what=f"iso {op}")


# ------------------------------------------------------------------ output side
@pytest.mark.parametrize("ct", ["INT64", "FP32", "BOOL"])
def test_output_side_matrix(gb, ct):
    A = ic.matrix_named("small", "INT64")
    a = to_gb(gb, A)
    T = im.index_apply(A, "diagindex", "INT64", 0)  # negative, zero and positive results
    assert (T[1][T[0]] == 0).any() and (T[1] < 0).any()
    for wb in ic.WB_ALL:
        key = ("index_apply", "M", ct, wb)
        C, M = ic.obj(ct, (70, 90), key, 0.4), ic.mask_obj((70, 90), key)
        c = to_gb(gb, C)
        bind(gb, c, wb, to_gb(gb, M)) << a.apply(gb.indexunary.diagindex)
        check(c, dm.write_back(C, T, **ic.wb_kw(wb, M)), ct, what=f"C[{ct}] {wb}")


@pytest.mark.parametrize("ct", ["INT64", "FP32", "BOOL"])
def test_output_side_vector(gb, ct):
    U = ic.obj("INT64", (300,), ("index_apply", "u"))
    u = to_gb(gb, U)
    T = im.index_apply(U, "rowindex", "INT64", -100)
    assert (T[1][T[0]] == 0).any() or not U[0][100]
    for wb in ic.WB_ALL:
        key = ("index_apply", "w", ct, wb)
        W, M = ic.obj(ct, (300,), key, 0.4), ic.mask_obj((300,), key)
        w = to_gb(gb, W)
        bind(gb, w, wb, to_gb(gb, M)) << u.apply("index", -100)
        check(w, dm.write_back(W, T, **ic.wb_kw(wb, M)), ct, what=f"w[{ct}] {wb}")


def test_output_aliases(gb):
    A = ic.matrix_named("square", "INT64")
    T = im.index_apply(A, "colindex", "INT64", 1)
    Tt = im.index_apply(dm.transpose(A), "rowindex", "INT64", 1)
    for acc in (None, "plus"):
        a = to_gb(gb, A)  # C = A
        bind(gb, a, ("none", False, acc), None) << a.apply("colindex", 1)
        check(a, dm.write_back(A, T, accum=acc), "INT64", what=f"C=A accum={acc}")
        a = to_gb(gb, A)  # C = A, the transposed view
        bind(gb, a, ("none", False, acc), None) << a.T.apply("rowindex", 1)
        check(a, dm.write_back(A, Tt, accum=acc), "INT64", what=f"C=A T0 accum={acc}")
        for wb in [("V", True, acc), ("~S", False, acc)]:
            a = to_gb(gb, A)  # C = A and M = C
            bind(gb, a, wb, a) << a.apply("colindex", 1)
            check(a, dm.write_back(A, T, **ic.wb_kw(wb, A)), "INT64", what=f"C=A=M {wb}")
            a, C = to_gb(gb, A), ic.obj("INT64", (70, 70), ("index_apply", "alias", wb), 0.4)
            c = to_gb(gb, C)  # M = C
            bind(gb, c, wb, c) << a.apply("colindex", 1)
            check(c, dm.write_back(C, T, **ic.wb_kw(wb, C)), "INT64", what=f"M=C {wb}")
    U = ic.obj("INT32", (300,), ("index_apply", "alias"))
    u = to_gb(gb, U)
    u(u.V) << u.apply("index")  # w = u = mask
    check(u, dm.write_back(U, im.index_apply(U, "rowindex", "INT32", 0), mask=U), "INT32", what="w=u=mask")


# ------------------------------------------------------------------ thunk forms
def test_thunk_forms(gb):
    lib = gb.lib
    A = ic.matrix_named("small", "INT64")
    a = to_gb(gb, A)
    want = im.index_apply(A, "rowindex", "INT64", 5)
    s = gb.Scalar.from_value(5, "INT8")
    with gb.Recorder() as rec:
        r1 = a.apply(gb.indexunary.rowindex, s).new(name="r1")
        r2 = a.apply("rowindex", 5).new(name="r2")
        r3 = a.T.apply(gb.select.colle, 2.7).new(name="r3")
        r4 = a.apply(gb.indexunary.valuegt, 1.5).new(name="r4")
    assert [line for line in rec.data if "_apply_" in line] == [
        f"GrB_Matrix_apply_IndexOp_Scalar(r1, NULL, NULL, GrB_ROWINDEX_INT64, {a.name}, {s.name}, NULL);",
        f"GrB_Matrix_apply_IndexOp_INT64(r2, NULL, NULL, GrB_ROWINDEX_INT64, {a.name}, 5, NULL);",
        f"GrB_Matrix_apply_IndexOp_INT64(r3, NULL, NULL, GrB_COLLE, {a.name}, 2, GrB_DESC_T0);",
        f"GrB_Matrix_apply_IndexOp_FP64(r4, NULL, NULL, GrB_VALUEGT_FP64, {a.name}, 1.5, NULL);",
    ]
    check(r1, want, "INT64", what="Scalar thunk")
    check(r2, want, "INT64", what="literal thunk")
    check(r3, im.index_apply(dm.transpose(A), "colle", None, 2), "BOOL", what="2.7 on a positional operator")
    check(r4, im.index_apply(A, "valuegt", "FP64", 1.5), "BOOL", what="FP64 literal on a value operator")
    # the library's own cast of an FP64 thunk: 2.7 -> 2 for ROWINDEX_INT64 and for COLGT
    C = gb.Matrix("INT64", 70, 90)
    assert lib.GrB_Matrix_apply_IndexOp_FP64(C._h, None, None, lib.GrB_ROWINDEX_INT64, a._h, 2.7, None) == 0
    check(C, im.index_apply(A, "rowindex", "INT64", 2.7), "INT64", what="ROWINDEX_INT64 y=2.7")
    assert np.array_equal(C.to_coo()[2], C.to_coo()[0].astype(np.int64) + 2)
    B = gb.Matrix("BOOL", 70, 90)
    assert lib.GrB_Matrix_apply_IndexOp_FP64(B._h, None, None, lib.GrB_COLGT, a._h, 2.7, None) == 0
    check(B, im.index_apply(A, "colgt", None, 2.7), "BOOL", what="COLGT y=2.7")
    # an empty Scalar: GrB_EMPTY_OBJECT, and C stays as it was
    empty = gb.Scalar("INT64")
    before = C.dup()
    assert lib.GrB_Matrix_apply_IndexOp_Scalar(C._h, None, None, lib.GrB_COLINDEX_INT64, a._h, empty._h, None) \
        == EMPTY_OBJECT
    assert C.isequal(before, check_dtype=True)
    with pytest.raises(gb.EmptyObject):
        a.apply("colindex", empty).new()
    u = gb.Vector.from_coo([0, 2, 5, 9], [4, 5, 6, 7], size=12)
    w = gb.Vector("INT64", 12)
    assert lib.GrB_Vector_apply_IndexOp_Scalar(w._h, None, None, lib.GrB_ROWINDEX_INT64, u._h, s._h, None) == 0
    assert w.to_coo()[0].tolist() == [0, 2, 5, 9] and w.to_coo()[1].tolist() == [5, 7, 10, 14]
    assert lib.GrB_Vector_apply_IndexOp_Scalar(w._h, None, None, lib.GrB_ROWINDEX_INT64, u._h, empty._h, None) \
        == EMPTY_OBJECT
    assert w.to_coo()[1].tolist() == [5, 7, 10, 14]


def test_int32_wrap(gb):
    A = dm.to_dense((3, 2), ([0, 1, 1, 2], [0, 0, 1, 1]), np.array([1, 2, 3, 4], np.int32))
    a = to_gb(gb, A)
    y = 2**31 - 1
    want = im.index_apply(A, "rowindex", "INT32", y)
    assert want[1][want[0]].tolist() == [2**31 - 1, -2**31, -2**31, -2**31 + 1]
    w = a.apply("rowindex", y).new()  # an INT32 input takes GrB_ROWINDEX_INT32
    check(w, want, "INT32", what="rowindex[INT32] wrap")
    C = gb.Matrix("INT32", 3, 2)
    assert gb.lib.GrB_Matrix_apply_IndexOp_INT64(C._h, None, None, gb.lib.GrB_ROWINDEX_INT32, a._h, y, None) == 0
    check(C, want, "INT32", what="ROWINDEX_INT32 wrap, C ABI")
    # the thunk wraps in its own cast first: 2^32 + 1 is 1
    assert gb.lib.GrB_Matrix_apply_IndexOp_INT64(C._h, None, None, gb.lib.GrB_COLINDEX_INT32, a._h, 2**32 + 1,
                                                 None) == 0
    check(C, im.index_apply(A, "colindex", "INT32", 2**32 + 1), "INT32", what="COLINDEX_INT32 thunk wrap")
    # into an INT64 output the INT32 result is widened after it wrapped
    D = gb.Matrix("INT64", 3, 2)
    D << a.apply(gb.indexunary.rowindex["INT32"], y)
    assert D.to_coo()[2].tolist() == [2**31 - 1, -2**31, -2**31, -2**31 + 1]


# ------------------------------------------------------------------ select
@pytest.mark.parametrize("dt", ["INT32", "INT64"])
def test_select_with_index_valued_operators(gb, dt):
    A = ic.matrix_named("rows", dt)
    a = to_gb(gb, A)
    for op in im.INDEX:
        for y in THUNKS + [-7, -299]:
            z = im.index_apply(A, op, dt, y)
            keep = z[0] & (z[1] != 0)
            if y in (-3, -7):
                assert keep.sum() < A[0].sum(), (op, y)  # something is dropped
            want = keep, np.where(keep, A[1], A[1].dtype.type(0))
            check(a.select(getattr(gb.indexunary, op), y).new(), want, dt, what=f"select {op}[{dt}] y={y}")
            zt = im.index_apply(dm.transpose(A), op, dt, y)
            keep = zt[0] & (zt[1] != 0)
            want = keep, np.where(keep, A[1].T, A[1].dtype.type(0))
            check(a.T.select(getattr(gb.indexunary, op)[dt], y).new(), want, dt, what=f"select T0 {op}[{dt}] y={y}")
    # INT32: 2^32 is 0 after the thunk's cast, so ROWINDEX keeps every row but row 0
    if dt == "INT32":
        C = gb.Matrix("INT32", 70, 300)
        assert gb.lib.GrB_Matrix_select_INT64(C._h, None, None, gb.lib.GrB_ROWINDEX_INT32, a._h, 2**32, None) == 0
        keep = A[0].copy()
        keep[0] = False
        check(C, (keep, np.where(keep, A[1], np.int32(0))), "INT32", what="select ROWINDEX_INT32 y=2^32")
    u = gb.Vector.from_coo([0, 3, 5, 64, 65], [9, 8, 7, 6, 5], size=70)
    w = u.select(gb.indexunary.index, -64).new()
    assert w.to_coo()[0].tolist() == [0, 3, 5, 65] and w.to_coo()[1].tolist() == [9, 8, 7, 5]


# ------------------------------------------------------------------ errors
def test_errors(gb):
    lib = gb.lib
    A = ic.matrix_named("small", "INT64")
    a = to_gb(gb, A)
    bad = to_gb(gb, ic.obj("INT64", (90, 70), ("index_apply", "bad"), 0.3))
    before = bad.dup()
    assert lib.GrB_Matrix_apply_IndexOp_INT64(bad._h, None, None, lib.GrB_ROWINDEX_INT64, a._h, 0, None) \
        == DIMENSION_MISMATCH
    msg = ctypes.c_char_p()
    assert lib.GrB_Matrix_error(ctypes.byref(msg), bad._h) == 0
    assert msg.value and b"dimension" in msg.value
    assert bad.isequal(before, check_dtype=True)
    with pytest.raises(gb.DimensionMismatch):
        bad << a.apply("rowindex")
    assert lib.GrB_Matrix_apply_IndexOp_INT64(bad._h, None, None, lib.GrB_ROWINDEX_INT64, a._h, 0,
                                              lib.GrB_DESC_T0) == 0
    check(bad, im.index_apply(dm.transpose(A), "rowindex", "INT64", 0), "INT64", what="T0 into 90 x 70")
    C = to_gb(gb, A)
    assert lib.GrB_Matrix_apply_IndexOp_INT64(C._h, None, None, None, a._h, 0, None) == NULL_POINTER
    u = gb.Vector.from_coo([0, 2], [1, 2], size=5)
    w = gb.Vector("INT64", 7)
    assert lib.GrB_Vector_apply_IndexOp_INT64(w._h, None, None, lib.GrB_ROWINDEX_INT64, u._h, 0, None) \
        == DIMENSION_MISMATCH
    assert lib.GrB_Vector_apply_IndexOp_INT64(w._h, None, None, None, u._h, 0, None) == NULL_POINTER
    assert C.isequal(a, check_dtype=True) and w.nvals == 0
    with pytest.raises(TypeError, match="left"):
        a.apply(gb.indexunary.diagindex, left=2)
    with pytest.raises(TypeError, match="thunk"):
        a.apply(gb.indexunary.rowindex, object())


# ------------------------------------------------------------------ consumers
def test_parent_vector_from_index(gb):
    n = 4097
    v = gb.Vector.from_coo(np.arange(n), 1, dtype="BOOL", size=n)
    parent = gb.Vector("INT64", n)
    parent << v.apply("index")  # the first line of FastSV and of a parent BFS
    i, x = parent.to_coo()
    assert parent.nvals == n and np.array_equal(i.astype(np.int64), np.arange(n)) and np.array_equal(x, np.arange(n))


def test_argmin_per_row(gb):
    rng = ic.rng_of("index_apply", "argmin")
    p = rng.random((65, 70)) < 0.6
    p[:, 0] |= ~p.any(axis=1)
    vals = rng.permutation(65 * 70).reshape(65, 70).astype(np.float64)  # no ties
    a = to_gb(gb, (p, np.where(p, vals, 0.0)))
    rowmin = a.reduce_rowwise(gb.monoid.min).new()
    i, m = rowmin.to_coo()
    D = gb.Matrix.from_coo(i, i, m, nrows=65, ncols=65)
    B = D.mxm(a, gb.semiring.min_first).new()  # B(i, j) = min of row i, on the structure of A
    E = a.ewise_mult(B, gb.binary.eq).new()    # true at the minimum of each row
    J = gb.Matrix("INT64", 65, 70)
    J(E.V) << a.apply("colindex")
    got = J.reduce_rowwise(gb.monoid.min).new()
    gi, gx = got.to_coo()
    want = np.argmin(np.where(p, vals, np.inf), axis=1)
    assert J.nvals == 65 and np.array_equal(gi.astype(np.int64), np.arange(65)) and np.array_equal(gx, want)
