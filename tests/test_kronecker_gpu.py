"""GrB_kronecker on the device (csrc/gb_kron.hip) against the numpy model of test_kronecker_abi.py.

Every comparison goes through to_coo(): indices, their order, nvals, the dtype and the values by
bits (NaNs compare equal); isequal never judges.  Every structure case runs under kron_method 0
(the entry-parallel kernel) and 1 (one thread per output row).

Shapes, and the path each one is for (the kernel fills chunks of KRON_CHUNK = 512 positions, a
wave owns a run of chunks, lane l of a chunk owns the row of boundary l):
  1x1 (x) 1x1, empty operands       one entry; no fill launch at all
  3x5 (x) 7x2, 37x53 (x) 5x11       odd sizes at densities 0.05 / 0.3 / 1.0, several chunks per wave
  empty-row runs                    runs of >= 70 empty rows in A and in B: runs of empty output rows
                                    longer than a wave (the row search's binary-search branch)
  40x40 diagonal (x) one per row    1600 rows of one entry: 64 or more boundaries in a chunk, so
                                    every lane searches and divides for itself
  70-entry row (x) 50-entry row     one output row of 3500 entries across 7 chunks (64-bit-free
                                    stepping from the row's first position in the chunk), alone
                                    and next to short rows
  nvals(T) = 511, 512, 513          one chunk less one, exactly, plus one
  3x300 (x) 300x3                   a 290-entry row of A against 300 short rows of B
  R-MAT scale 7 squared             iso bool, about half a million entries; with the knob
                                    kron_grid = 2 eight waves run through ~120 chunks each

Tolerances: everything integer, bool, every cast and structure is exact, and so are the correctly
rounded float operators.  pow, atan2 and hypot are held to the ulp bounds of
test_general_ops_gpu.py ("General operations"), measured for the same device
functions.  Float min / max compare by value, not by bits: kronecker meets every pair of
operands, -0.0 against +0.0 among them, where IEEE fmin / fmax may return either zero.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import dense_model as dm
from test_general_ops_gpu import BINARY, INT_POW_EDGES, ULP_BOUND, _knobs, draw
from test_kronecker_abi import coo, golden_cases, kron_model

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
METHODS = [0, 1]


@pytest.fixture(scope="module")
def gb():
    import graphblas_amd

    return graphblas_amd


def kron_chunk():
    src = open(os.path.join(ROOT, "graph-python_amd", "csrc", "gb_kron.hip")).read()
    return int(re.search(r"#define KRON_CHUNK (\d+)", src).group(1))


def is_iso(A):
    from graphblas_amd.device import matrix_view

    return bool(matrix_view(A._h).iso)


def matrix(gb, triples, shape, dtype=None):
    r, c, v = triples
    if len(r) == 0:
        return gb.Matrix(dtype if dtype is not None else dm.name_of(np.asarray(v).dtype), *shape)
    return gb.Matrix.from_coo(r, c, v, dtype=dtype, nrows=shape[0], ncols=shape[1])


def bits(v):
    v = np.ascontiguousarray(v)
    return v.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[v.dtype.itemsize])


def assert_coo(C, want, zt, *, what="", by_value=False, ulps=None):
    """C's tuples against (rows, cols, vals): indices and order, nvals, dtype, values by bits with
    NaNs equal (by_value: ==, for float min / max; ulps: at most that many ulps apart)"""
    wr, wc, wv = want
    assert C.dtype == zt, f"{what}: dtype {C.dtype}, expected {zt}"
    gr, gc, gv = C.to_coo()
    assert C.nvals == len(wr) == gr.size, f"{what}: nvals {C.nvals}, expected {len(wr)}"
    assert np.array_equal(gr.astype(np.int64), wr), f"{what}: rows differ"
    assert np.array_equal(gc.astype(np.int64), wc), f"{what}: columns differ"
    wv = np.asarray(wv)
    assert gv.dtype == dm.NP[zt] == wv.dtype, f"{what}: value dtype {gv.dtype}"
    if ulps is not None:
        d = dm.ulp_distance(gv, wv)
        print(f"\nULP {what} {d}")
        assert d <= ulps, f"{what}: {d} ulps from the float64 reference, bound {ulps}"
        return
    if gv.dtype.kind == "f":
        both_nan = np.isnan(gv) & np.isnan(wv)
        same = both_nan | ((gv == wv) if by_value else (bits(gv) == bits(wv)))
    else:
        same = gv == wv
    if not same.all():
        q = np.flatnonzero(~same)[0]
        raise AssertionError(f"{what}: {(~same).sum()} of {gv.size} values differ; first at "
                             f"({gr[q]}, {gc[q]}): got {gv[q]!r}, expected {wv[q]!r}")


def random_coo(rng, shape, density, lo=-9, hi=10):
    P = np.ones(shape, bool) if density >= 1.0 else rng.random(shape) < density
    r, c = np.nonzero(P)
    return r, c, rng.integers(lo, hi, r.size).astype(np.int64)  # zeros among the values


def exact_nnz(rng, shape, nnz):
    flat = np.sort(rng.permutation(shape[0] * shape[1])[:nnz])
    return flat // shape[1], flat % shape[1], rng.integers(-9, 10, nnz).astype(np.int64)


def with_empty_runs(rng, ncols, per_row):
    """leading, interior and trailing runs of 70, 75 and 71 empty rows around two groups of 4 rows"""
    rows = np.concatenate([np.arange(70, 74), np.arange(149, 153)])
    r = np.repeat(rows, per_row)
    c = np.concatenate([np.sort(rng.permutation(ncols)[:per_row]) for _ in rows])
    return (r, c, rng.integers(-9, 10, r.size).astype(np.int64)), (224, ncols)


def one_row(n, cols, row=0, nrows=1):
    cols = np.asarray(cols)
    return np.full(cols.size, row), cols, np.arange(1, cols.size + 1, dtype=np.int64) * 3 - 50


def stack(*parts):
    return tuple(np.concatenate([p[i] for p in parts]) for i in range(3))


def structure_cases():
    rng = np.random.default_rng(2024)
    chunk = 512
    E = (np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int64))
    yield "1x1", ([0], [0], np.array([7])), (1, 1), ([0], [0], np.array([-3])), (1, 1)
    yield "A_empty", E, (3, 4), random_coo(rng, (5, 2), 0.5), (5, 2)
    yield "B_empty", random_coo(rng, (3, 4), 0.5), (3, 4), E, (5, 2)
    yield "both_empty", E, (3, 4), E, (5, 2)
    for d in (0.05, 0.3, 1.0):
        yield f"3x5_7x2_d{d}", random_coo(rng, (3, 5), d), (3, 5), random_coo(rng, (7, 2), d), (7, 2)
        yield f"37x53_5x11_d{d}", random_coo(rng, (37, 53), d), (37, 53), random_coo(rng, (5, 11), d), (5, 11)
    (a, ash), (b, bsh) = with_empty_runs(rng, 9, 3), with_empty_runs(rng, 6, 4)
    yield "empty_row_runs", a, ash, b, bsh
    d40 = np.arange(40)
    yield ("diag_x_one_per_row", (d40, d40, rng.integers(1, 9, 40)), (40, 40),
           (d40, rng.integers(0, 40, 40), rng.integers(1, 9, 40)), (40, 40))
    a70 = np.sort(rng.permutation(80)[:70])
    b50 = np.sort(rng.permutation(60)[:50])
    yield "row70_x_row50", one_row(80, a70), (1, 80), one_row(60, b50), (1, 60)
    yield ("row70_x_row50_among_short_rows",
           stack(one_row(80, [3, 9], 0), one_row(80, a70, 1), one_row(80, [79], 3)), (4, 80),
           stack(one_row(60, [5], 0), one_row(60, b50, 1), one_row(60, [0, 1, 59], 2)), (3, 60))
    # 511 = 7 x 73, 512 = 16 x 32, 513 = 27 x 19
    for nnz, na, nb in [(chunk - 1, 7, 73), (chunk, 16, 32), (chunk + 1, 27, 19)]:
        assert na * nb == nnz
        yield f"nvals_{nnz}", exact_nnz(rng, (4, 9), na), (4, 9), exact_nnz(rng, (21, 13), nb), (21, 13)
    a = stack(one_row(300, np.sort(rng.permutation(300)[:290]), 1), one_row(300, [0, 150, 299], 0),
              one_row(300, [7], 2))
    yield "3x300_x_300x3", a, (3, 300), random_coo(rng, (300, 3), 0.5), (300, 3)


STRUCTURE = list(structure_cases())


def test_chunk_constant():
    assert kron_chunk() == 512  # structure_cases() builds nvals(T) = 511 / 512 / 513 around it


@pytest.fixture(scope="module")
def structure_models():
    """the model results, computed once per (case, op)"""
    out = {}
    for name, a, ash, b, bsh in STRUCTURE:
        for op in ("times", "plus"):
            out[name, op] = kron_model(a, b, (ash, bsh), op, "INT64")[0]
    return out


# ------------------------------------------------------------------ 1. golden cases
@pytest.mark.parametrize("method", METHODS)
def test_golden(gb, method):
    lib = gb.lib
    with _knobs(gb, kron_method=method):
        for k, case in enumerate(golden_cases()):
            a, b, c = case["A"], case["B"], case["C"]
            dt = case["dtype"]
            A = matrix(gb, coo(a), (a["nrows"], a["ncols"]), dt)
            B = matrix(gb, coo(b), (b["nrows"], b["ncols"]), dt)
            want = (np.asarray(c["rows"]), np.asarray(c["cols"]), np.asarray(c["vals"], dm.NP[dt]))
            for C in (A.kronecker(B).new(), A.kronecker(B, "times").new(), A.kronecker(B, gb.binary.times).new(),
                      A.kronecker(B, gb.monoid.times).new()):
                assert C.shape == (c["nrows"], c["ncols"])
                assert_coo(C, want, dt, what=case["source"])
            if k == 0:  # the three entry points; the Semiring form exists at the C level only
                for fn, op in [(lib.GrB_Matrix_kronecker_BinaryOp, lib.GrB_TIMES_INT64),
                               (lib.GrB_Matrix_kronecker_Monoid, lib.GrB_TIMES_MONOID_INT64),
                               (lib.GrB_Matrix_kronecker_Semiring, lib.GrB_PLUS_TIMES_SEMIRING_INT64)]:
                    C = gb.Matrix(dt, c["nrows"], c["ncols"])
                    assert fn(C._h, None, None, op, A._h, B._h, None) == 0
                    assert_coo(C, want, dt, what=f"ctypes {case['source']}")
                C = gb.Matrix(dt, c["nrows"], c["ncols"])
                assert lib.GrB_Matrix_kronecker_BinaryOp(C._h, None, None, None, A._h, B._h, None) \
                    == lib.GrB_NULL_POINTER
                assert lib.GrB_Matrix_kronecker_BinaryOp(C._h, None, None, lib.GxB_FIRSTI_INT64, A._h, B._h, None) \
                    == lib.GrB_NOT_IMPLEMENTED
                assert C.nvals == 0


# ------------------------------------------------------------------ 2. structure edges
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("case", STRUCTURE, ids=[s[0] for s in STRUCTURE])
def test_structure(gb, structure_models, case, method):
    name, a, ash, b, bsh = case
    A, B = matrix(gb, a, ash, "INT64"), matrix(gb, b, bsh, "INT64")
    with _knobs(gb, kron_method=method):
        for op in ("times", "plus"):
            C = A.kronecker(B, op).new()
            assert C.shape == (ash[0] * bsh[0], ash[1] * bsh[1])
            want = structure_models[name, op]
            assert len(want[0]) == len(a[0]) * len(b[0])
            assert_coo(C, want, "INT64", what=f"{name} {op} method {method}")
            assert not is_iso(C) or C.nvals <= 1 or np.unique(want[2]).size == 1
            rp = C.to_csr()[0]
            assert np.array_equal(rp, np.concatenate([[0], np.cumsum(np.bincount(want[0], minlength=C.nrows))]))


@pytest.mark.parametrize("method,grid", [(0, 0), (0, 2), (1, 0)])
def test_rmat_square_is_iso(gb, method, grid):
    from graphblas_amd.matrix import Matrix

    scale, n = 7, 128
    R = Matrix.__new__(Matrix)
    R.dtype, R.name, R._h, R._nrows, R._ncols = gb.dtypes.BOOL, "R", ctypes.c_void_p(), n, n
    assert gb.lib.GxB_Matrix_rmat(ctypes.byref(R._h), scale, 8, 42, 0, 2, 0, 0) == 0
    assert is_iso(R) and R.dtype == "BOOL"
    r, c, v = R.to_coo()
    assert v.all() and 512 * 256 < r.size ** 2 <= 2_500_000  # many chunks per wave once the grid is 2 blocks
    with _knobs(gb, kron_method=method, kron_grid=grid):
        K = R.kronecker(R, "land").new()
    assert is_iso(K) and K.shape == (n * n, n * n)
    want, zt = kron_model((r, c, v), (r, c, v), ((n, n), (n, n)), "land", "BOOL")
    assert_coo(K, want, zt, what=f"R-MAT s7 squared, method {method}, grid {grid}")


# ------------------------------------------------------------------ 3. wide columns
@pytest.mark.parametrize("method", METHODS)
def test_wide_columns(gb, method):
    w = 46340
    A = gb.Matrix.from_coo([0, 0], [0, w - 1], [2, 3], nrows=1, ncols=w)
    with _knobs(gb, kron_method=method):
        C = A.kronecker(A).new()
        assert C.shape == (1, 2147395600) and C.ncols < 2**31
        assert_coo(C, (np.zeros(4, np.int64), np.array([0, w - 1, (w - 1) * w, 2147395599]),
                       np.array([4, 6, 6, 9])), "INT64", what="1x46340 squared")
        # one column more on each side: no such C can exist
        A2 = gb.Matrix.from_coo([0, 0], [0, w], [2, 3], nrows=1, ncols=w + 1)
        with pytest.raises(gb.OutOfMemory):
            A2.kronecker(A2).new()
        # a C of the wrong shape
        S = gb.Matrix.from_coo([0, 1], [1, 2], [1, 2], nrows=2, ncols=3)
        for shape in [(4, 6), (6, 4), (4, 10), (3, 9)]:
            bad = gb.Matrix("INT64", *shape)
            with pytest.raises(gb.DimensionMismatch):
                bad << S.kronecker(S)
            assert bad.nvals == 0
        good = gb.Matrix("INT64", 4, 9)
        good << S.kronecker(S)
        assert good.nvals == 4


# ------------------------------------------------------------------ 4. operators and types
def operand_values(op, dt, rng, n, second):
    """n values of dt from the pools of test_general_ops_gpu.py, with its restrictions for pow on
    integers (float64 pow exact or saturating without doubt) and ldexp (small exponents)"""
    t = dm.NP[dt]
    if op == "pow" and dm.is_int(dt):
        signed = dm.tmin(dt) < 0
        if second:
            v = rng.integers(0, 13, n).astype(t)
            edges = [b for _, b in INT_POW_EDGES if signed or b >= 0]
        else:
            v = rng.integers(-9 if signed else 0, 10, n).astype(t)
            edges = [a for a, _ in INT_POW_EDGES if signed or a >= 0]
        k = min(len(edges), n // 2)
        v[:k] = np.array(edges[:k], t)
        return v
    if op == "ldexp" and second:
        return rng.integers(-20, 21, n).astype(t)
    return draw(dt, rng, n)


@pytest.mark.parametrize("op", BINARY)
def test_every_binary_op_and_type(gb, op):
    opobj = getattr(gb.binary, op)
    ash, bsh = (6, 5), (4, 7)
    for dtobj in opobj.types:
        dt = dtobj.name
        rng = np.random.default_rng([BINARY.index(op), dm.ALL.index(dt)])
        Ap, Bp = rng.random(ash) < 0.5, rng.random(bsh) < 0.5
        Ap[0, 0] = Bp[0, 0] = True
        ar, ac = np.nonzero(Ap)
        br, bc = np.nonzero(Bp)
        a = (ar, ac, operand_values(op, dt, rng, ar.size, False))
        b = (br, bc, operand_values(op, dt, rng, br.size, True))
        want, zt = kron_model(a, b, (ash, bsh), op, dt)
        assert opobj[dt].return_type.name == zt
        C = matrix(gb, a, ash, dt).kronecker(matrix(gb, b, bsh, dt), opobj).new()
        what = f"kronecker {op}[{dt}]"
        if op in dm.TRANSCENDENTAL and dm.is_float(dt):
            assert_coo(C, want, zt, what=what, ulps=ULP_BOUND[op, dt])
        else:
            assert_coo(C, want, zt, what=what, by_value=op in ("min", "max"))


@pytest.mark.parametrize("adt,bdt,op,odt", [("INT8", "FP64", "times", "INT32"), ("BOOL", "INT64", "plus", "FP32")])
def test_mixed_inputs_are_cast_to_the_operator_type(gb, adt, bdt, op, odt):
    rng = np.random.default_rng(77)
    ash, bsh = (6, 5), (4, 7)
    Ap, Bp = rng.random(ash) < 0.5, rng.random(bsh) < 0.5
    ar, ac = np.nonzero(Ap)
    br, bc = np.nonzero(Bp)
    a = (ar, ac, draw(adt, rng, ar.size))
    bv = draw(bdt, rng, br.size)
    if bdt == "FP64":
        bv[:4] = [2.75, -3.5, 1e12, -1e12]  # truncation and saturation on the way to INT32
    b = (br, bc, bv)
    want, zt = kron_model(a, b, (ash, bsh), op, odt)
    assert zt == odt
    C = matrix(gb, a, ash, adt).kronecker(matrix(gb, b, bsh, bdt), getattr(gb.binary, op)[odt]).new()
    assert_coo(C, want, odt, what=f"{adt} (x) {bdt} under {op}[{odt}]")


# ------------------------------------------------------------------ 5. iso
@pytest.mark.parametrize("method", METHODS)
def test_iso_results(gb, method):
    rng = np.random.default_rng(5)
    ash, bsh = (9, 7), (6, 8)
    ar, ac, av = random_coo(rng, ash, 0.4, 1, 9)
    br, bc, bv = random_coo(rng, bsh, 0.4, 1, 9)
    assert np.unique(av).size > 1 and np.unique(bv).size > 1
    A, B = matrix(gb, (ar, ac, av), ash), matrix(gb, (br, bc, bv), bsh)
    Ai = gb.Matrix.from_coo(ar, ac, 6, dtype="INT64", nrows=ash[0], ncols=ash[1])
    Bi = gb.Matrix.from_coo(br, bc, -4, dtype="INT64", nrows=bsh[0], ncols=bsh[1])
    assert is_iso(Ai) and is_iso(Bi) and not is_iso(A) and not is_iso(B)
    ai, bi = (ar, ac, np.full(ar.size, 6)), (br, bc, np.full(br.size, -4))
    shapes = (ash, bsh)
    with _knobs(gb, kron_method=method):
        for op in ("times", "plus", "minus", "eq", "lt", "first", "second", "pair", "any", "min"):
            C = Ai.kronecker(Bi, op).new()
            want, zt = kron_model(ai, bi, shapes, op, "INT64")
            assert is_iso(C), op
            assert_coo(C, want, zt, what=f"iso (x) iso {op}")
        for X, Y, x, y, op in [(Ai, B, ai, (br, bc, bv), "first"), (A, Bi, (ar, ac, av), bi, "second"),
                               (A, Bi, (ar, ac, av), bi, "any"), (A, B, (ar, ac, av), (br, bc, bv), "pair")]:
            C = X.kronecker(Y, op).new()
            want, zt = kron_model(x, y, shapes, op, "INT64")
            assert is_iso(C), op
            assert_coo(C, want, zt, what=f"iso by operator {op}")
        for X, Y, x, y, op in [(Ai, B, ai, (br, bc, bv), "times"), (A, Bi, (ar, ac, av), bi, "times"),
                               (A, Bi, (ar, ac, av), bi, "first"), (Ai, B, ai, (br, bc, bv), "second"),
                               (A, B, (ar, ac, av), (br, bc, bv), "plus")]:
            C = X.kronecker(Y, op).new()
            want, zt = kron_model(x, y, shapes, op, "INT64")
            assert not is_iso(C), op
            assert_coo(C, want, zt, what=f"not iso {op}")


# ------------------------------------------------------------------ 6. output side
@pytest.fixture(scope="module")
def outside():
    rng = np.random.default_rng(17)
    ash, bsh = (12, 9), (5, 7)
    shape = (60, 63)
    a, b = random_coo(rng, ash, 0.4), random_coo(rng, bsh, 0.5)
    Cp = rng.random(shape) < 0.4
    Cv = np.where(Cp, rng.integers(-50, 50, shape), 0).astype(np.int64)
    Mp = rng.random(shape) < 0.5
    Mv = np.where(Mp, rng.integers(0, 2, shape), 0).astype(np.int64)  # stored false values
    assert (Mp & (Mv == 0)).any()
    return dict(a=a, b=b, ash=ash, bsh=bsh, shape=shape, C=(Cp, Cv), M=(Mp, Mv))


def dense_kron(a, b, shapes, op, dt, shape):
    (r, c, v), _ = kron_model(a, b, shapes, op, dt)
    return dm.to_dense(shape, (r, c), v)


def from_dense(gb, X, dt=None):
    p, v = X
    r, c = np.nonzero(p)
    return gb.Matrix.from_coo(r, c, v[r, c], dtype=dt, nrows=p.shape[0], ncols=p.shape[1])


def assert_dense(C, want, zt, what):
    p, v = want
    r, c = np.nonzero(p)
    assert_coo(C, (r, c, v[r, c]), zt, what=what)


@pytest.mark.parametrize("method", METHODS)
def test_output_masks_and_replace(gb, outside, method):
    o = outside
    A, B, M = matrix(gb, o["a"], o["ash"]), matrix(gb, o["b"], o["bsh"]), from_dense(gb, o["M"])
    T = dense_kron(o["a"], o["b"], (o["ash"], o["bsh"]), "times", "INT64", o["shape"])
    with _knobs(gb, kron_method=method):
        for tag, mask, kw in [("M.V", M.V, {}), ("M.S", M.S, dict(mask_struct=True)),
                              ("~M.V", ~M.V, dict(mask_comp=True)),
                              ("~M.S", ~M.S, dict(mask_comp=True, mask_struct=True))]:
            for replace in (False, True):
                C = from_dense(gb, o["C"])
                C(mask, replace=replace) << A.kronecker(B)
                want = dm.write_back(o["C"], T, mask=o["M"], replace=replace, **kw)
                assert_dense(C, want, "INT64", f"C({tag}, replace={replace})")
                C = from_dense(gb, o["C"])
                C(mask, gb.binary.plus, replace=replace) << A.kronecker(B)
                want = dm.write_back(o["C"], T, mask=o["M"], replace=replace, accum="plus", **kw)
                assert_dense(C, want, "INT64", f"C({tag}, plus, replace={replace})")
        # .new() with a dtype and a mask
        C = A.kronecker(B).new(dtype="FP32", mask=M.S)
        empty = (np.zeros(o["shape"], bool), np.zeros(o["shape"], np.float32))
        assert_dense(C, dm.write_back(empty, T, mask=o["M"], mask_struct=True), "FP32", "new(dtype, mask)")


def test_output_accum_into_another_type(gb, outside):
    o = outside
    shapes = (o["ash"], o["bsh"])
    A, B = matrix(gb, o["a"], o["ash"]), matrix(gb, o["b"], o["bsh"])
    # INT64 T into an FP64 C
    Cf = (o["C"][0], np.where(o["C"][0], o["C"][1] + 0.25, 0.0))
    C = from_dense(gb, Cf)
    C(accum=gb.binary.plus) << A.kronecker(B)
    T = dense_kron(o["a"], o["b"], shapes, "times", "INT64", o["shape"])
    assert_dense(C, dm.write_back(Cf, T, accum="plus"), "FP64", "FP64 C += INT64 T")
    # FP64 T into an INT64 C: the sum runs in INT64 on the truncated t
    af = (o["a"][0], o["a"][1], o["a"][2] + 0.5)
    bf = (o["b"][0], o["b"][1], o["b"][2] * 1.25)
    C = from_dense(gb, o["C"])
    C(accum=gb.binary.plus) << matrix(gb, af, o["ash"]).kronecker(matrix(gb, bf, o["bsh"]))
    T = dense_kron(af, bf, shapes, "times", "FP64", o["shape"])
    assert T[1].dtype == np.float64 and (T[1] != np.trunc(T[1])).any()
    assert_dense(C, dm.write_back(o["C"], T, accum="plus"), "INT64", "INT64 C += FP64 T")


def transposed(triples):
    r, c, v = triples
    order = np.lexsort((r, c))
    return np.asarray(c)[order], np.asarray(r)[order], np.asarray(v)[order]


@pytest.mark.parametrize("method", METHODS)
def test_transposed_operands(gb, outside, method):
    o = outside
    a, b, (m, n), (p, q) = o["a"], o["b"], o["ash"], o["bsh"]
    A, B = matrix(gb, a, (m, n)), matrix(gb, b, (p, q))
    at, bt = transposed(a), transposed(b)
    with _knobs(gb, kron_method=method):
        for X, Y, x, y, shapes in [(A.T, B, at, b, ((n, m), (p, q))), (A, B.T, a, bt, ((m, n), (q, p))),
                                   (A.T, B.T, at, bt, ((n, m), (q, p)))]:
            C = X.kronecker(Y, "minus").new()
            want, zt = kron_model(x, y, shapes, "minus", "INT64")
            assert C.shape == (shapes[0][0] * shapes[1][0], shapes[0][1] * shapes[1][1])
            assert_coo(C, want, zt, what=f"transposes {shapes}")


@pytest.mark.parametrize("method", METHODS)
def test_aliased_output(gb, outside, method):
    o = outside
    one = ([0], [0], np.array([3]))
    with _knobs(gb, kron_method=method):
        A = matrix(gb, o["a"], o["ash"])
        A << A.kronecker(matrix(gb, one, (1, 1)), "plus")  # C is A
        assert_coo(A, kron_model(o["a"], one, (o["ash"], (1, 1)), "plus", "INT64")[0], "INT64", what="C is A")
        B = matrix(gb, o["b"], o["bsh"])
        B << matrix(gb, one, (1, 1)).kronecker(B, "minus")  # C is B
        assert_coo(B, kron_model(one, o["b"], ((1, 1), o["bsh"]), "minus", "INT64")[0], "INT64", what="C is B")
        A = matrix(gb, o["a"], o["ash"])
        C = A.kronecker(A, "minus").new()  # A is B
        assert_coo(C, kron_model(o["a"], o["a"], (o["ash"], o["ash"]), "minus", "INT64")[0], "INT64", what="A is B")
        C = A.kronecker(A.T, "minus").new()
        assert_coo(C, kron_model(o["a"], transposed(o["a"]), (o["ash"], o["ash"][::-1]), "minus", "INT64")[0],
                   "INT64", what="A (x) A.T")
        I1 = matrix(gb, one, (1, 1))
        I1 << I1.kronecker(I1)  # C is A is B
        assert_coo(I1, ([0], [0], np.array([9])), "INT64", what="C is A is B")


# ------------------------------------------------------------------ 7. composition
def test_product_feeds_bfs_and_triangle_count(gb):
    import oracle as O

    rng = np.random.default_rng(31)
    k = 16
    U = np.triu(rng.random((k, k)) < 0.3, 1)
    U[np.arange(k - 1), np.arange(1, k)] = True  # a path: connected
    Sd = U | U.T
    Sd[0, 0] = Sd[5, 5] = True  # two self-loops: vertex (0, 0) of K has neighbours
    r, c = np.nonzero(Sd)
    S = gb.Matrix.from_coo(r, c, np.ones(r.size, bool), nrows=k, ncols=k)
    K = S.kronecker(S, "land").new()
    n = k * k
    assert K.dtype == "BOOL" and K.shape == (n, n) and K.nvals == r.size ** 2
    kr, kc, kv = K.to_coo()
    Kd = np.kron(Sd, Sd)
    assert kv.all() and np.array_equal(np.nonzero(Kd)[0], kr.astype(np.int64)) \
        and np.array_equal(np.nonzero(Kd)[1], kc.astype(np.int64))
    # BFS from vertex 0 with the notebook loop
    v = gb.Vector(gb.INT32, n)
    q = gb.Vector(bool, n)
    q[0] = True
    d = 0
    while True:
        d += 1
        v(mask=q.V)[:] = d
        q(~v.S, replace=True) << q.vxm(K, gb.semiring.lor_land)
        if q.nvals == 0:
            break
    idx, lv = v.to_coo()
    got = np.zeros(n, np.int32)
    got[idx.astype(np.int64)] = lv
    ref, _, _ = O.bfs_levels(O.Csr.from_coo(kr.astype(np.int64), kc.astype(np.int64), kv, nrows=n, ncols=n,
                                            dtype="BOOL"), 0)
    assert np.array_equal(got, ref) and got.max() > 2
    # triangles of K without its diagonal
    L = K.select("tril", -1).new()
    C = L.mxm(L.T, gb.semiring.plus_pair["INT64"]).new(mask=L.S)
    count = C.reduce_scalar(gb.monoid.plus).new().value or 0
    Di = (Kd & ~np.eye(n, dtype=bool)).astype(np.int64)
    want = int(np.trace(Di @ Di @ Di)) // 6
    assert want > 0 and count == want


# ------------------------------------------------------------------ 8. recorder
def test_recorder_strings(gb):
    A = gb.Matrix.from_coo([0, 1, 1], [0, 0, 1], [1, 2, 3], nrows=2, ncols=2, name="A")
    B = gb.Matrix.from_coo([0, 0, 1, 1], [1, 2, 0, 2], [2, 3, 8, 4], nrows=2, ncols=3, name="B")
    C = gb.Matrix("INT64", 4, 6, name="C")
    D = gb.Matrix("INT64", 4, 6, name="D")
    with gb.Recorder() as rec:
        C << A.kronecker(B, "times")
        C(accum=gb.binary.plus) << A.kronecker(B, gb.monoid.plus)
        D << A.T.kronecker(B.T.new(name="Bt").T, gb.binary.min)
    assert rec.data[0] == "GrB_Matrix_kronecker_BinaryOp(C, NULL, NULL, GrB_TIMES_INT64, A, B, NULL);"
    assert rec.data[1] == "GrB_Matrix_kronecker_Monoid(C, NULL, GrB_PLUS_INT64, GrB_PLUS_MONOID_INT64, A, B, NULL);"
    assert rec.data[-1] == "GrB_Matrix_kronecker_BinaryOp(D, NULL, NULL, GrB_MIN_INT64, A, Bt, GrB_DESC_T0T1);"
