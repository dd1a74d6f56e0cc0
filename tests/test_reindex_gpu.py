"""diag, reshape and flatten on the device (csrc/gb_reindex.hip) against the numpy model of
tests/reindex_model.py.  Every value is moved, never computed: every comparison is exact, through
to_coo() (test_general_ops_gpu.check: structure, order, nvals, dtype, values, NaN and the sign of
zero), and for vectors also through the exported bitmap words.

Shapes, and the path each one is for
  vectors 0 .. 1000    a bitmap without words, of one partial word, of exactly one word, one bit
                       into the second word, and of more than one block of positions; k = 64 and
                       -65 put the diagonal's first row / column on and past a word boundary
  rows 70 x 300        rows of 0, 1, 63, 64, 65, 128, 129 and 300 entries: the diagonal search ends
                       before, on and after every length; the k list has the diagonals of length
                       0, 1, 6, 7, 64 +- 1 and 70, and those outside the matrix
  heavy 301 x 6007     one row of 5200 entries: one search, not a walk
  400 x 40             runs of more than 64 empty rows: the row search of a chunk starts more than a
                       wave's width before its first row
  133125 x 64          about 2 * 10^5 entries, 0..3 per row: every lane of a chunk searches its own
                       row, and a wave owns many chunks
  70000 x 70000        4.9 * 10^9 positions: the 64-bit divisions ("stat_reshape_div64" = 1); every
                       other shape here takes the 32-bit path
"""
import ctypes
import time

import numpy as np
import pytest

import dense_model as dm
import reindex_model as rm
from test_ewise_union_gpu import bitmap_words
from test_general_ops_gpu import check, draw, heavy, iso_gb, ragged, to_gb

pytestmark = pytest.mark.gpu

G = rm.golden()
TYPES = ["BOOL", "INT8", "INT64", "FP32", "FP64"]
ORDERS = ["rowwise", "columnwise"]
DIMENSION_MISMATCH, OUT_OF_MEMORY, NULL_POINTER = -6, -102, -2


@pytest.fixture(scope="module")
def gb():
    import graphblas_amd

    return graphblas_amd


@pytest.fixture(scope="module", autouse=True)
def report_run_time():
    t0 = time.perf_counter()
    yield
    print(f"\ntest_reindex_gpu.py: {time.perf_counter() - t0:.1f} s")


def rng_of(*key):
    import zlib

    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def is_iso(obj):
    from graphblas_amd.device import matrix_view, vector_view

    return bool((vector_view if obj.ndim == 1 else matrix_view)(obj._h).iso)


def words_of(p):
    return np.packbits(np.pad(p, (0, -p.size % 64)), bitorder="little").view(np.uint64)


def check_vector(gb, w, want, dt, what):
    check(w, want, dt, what=what)
    assert np.array_equal(bitmap_words(gb, w), words_of(want[0])), f"{what}: bitmap words"


def vector_of(dt, n, density, key):
    rng = rng_of("vector", dt, n, density, key)
    p = rng.random(n) < density if 0 < density < 1 else np.full(n, bool(density))
    return p, np.where(p, draw(dt, rng, n), dm.NP[dt](0))


def rows_matrix(dt="INT64"):
    """70 x 300, rows of 0, 1, 63, 64, 65, 128, 129 and 300 entries in turn"""
    rng = rng_of("rows", dt)
    p = np.zeros((70, 300), bool)
    for i in range(70):
        p[i, rng.permutation(300)[:[0, 1, 63, 64, 65, 128, 129, 300][i % 8]]] = True
    return p, np.where(p, draw(dt, rng, p.size).reshape(p.shape), dm.NP[dt](0))


def gappy_matrix(dt="INT32"):
    """400 x 40 with rows 10..99 and 200..389 empty"""
    rng = rng_of("gappy", dt)
    p = rng.random((400, 40)) < 0.3
    p[10:100] = False
    p[200:390] = False
    return p, np.where(p, draw(dt, rng, p.size).reshape(p.shape), dm.NP[dt](0))


def transposes_cached(gb):
    return gb.get_knob("stat_transposes_cached")


# ---------------------------------------------------------------------- the reference's own cases
@pytest.mark.parametrize("case", G["matrix_diag"], ids=lambda c: f"k={c['k']}")
def test_golden_matrix_diag(gb, case):
    A, k = to_gb(gb, rm.golden_A(G)), case["k"]
    want = rm.pair_of((case["size"],), (case["idx"],), case["vals"])
    check_vector(gb, A.diag(k), want, "INT64", "A.diag(k)")
    check_vector(gb, A.T.diag(-k), want, "INT64", "A.T.diag(-k)")
    v = gb.ss.diag(A, k=k)
    check_vector(gb, v, want, "INT64", "ss.diag(A, k=k)")
    v[:] = 0
    v.ss.build_diag(A, k=k)
    check_vector(gb, v, want, "INT64", "build_diag(A, k=k)")
    check_vector(gb, gb.ss.diag(A.T, k=-k), want, "INT64", "ss.diag(A.T, k=-k)")
    v[:] = 0
    v.ss.build_diag(A.T, -k)
    check_vector(gb, v, want, "INT64", "build_diag(A.T, -k)")


@pytest.mark.parametrize("case", G["vector_diag"], ids=lambda c: f"k={c['k']}")
def test_golden_vector_diag(gb, case):
    V = rm.golden_v(G)
    v, k, n = to_gb(gb, V), case["k"], case["n"]
    want = rm.pair_of((n, n), (case["rows"], case["cols"]), case["vals"])
    check(gb.ss.diag(v, k=k, nthreads=2), want, "INT64", what="ss.diag(v, k=k)")
    A = v.diag(k)
    check(A, want, "INT64", what="v.diag(k)")
    check_vector(gb, gb.ss.diag(A, gb.Scalar.from_value(k), nthreads=2), V, "INT64", "ss.diag(A, Scalar k)")
    check_vector(gb, gb.ss.diag(A.T, -k, dtype=float), rm.cast(V, "FP64"), "FP64", "ss.diag(A.T, -k, float)")
    check_vector(gb, A.diag(gb.Scalar.from_value(k)), V, "INT64", "A.diag(Scalar k)")
    check_vector(gb, A.T.diag(-k, dtype=float), rm.cast(V, "FP64"), "FP64", "A.T.diag(-k, float)")


def call_form(method, form):
    return method(*[tuple(a) if isinstance(a, list) else a for a in form["args"]], **form["kwargs"])


@pytest.mark.parametrize("case", G["flatten"], ids=lambda c: c["order"])
def test_golden_flatten(gb, case):
    A = rm.golden_A(G)
    a = to_gb(gb, A)
    want = rm.pair_of((case["size"],), (case["idx"],), case["vals"])
    assert case["flatten_forms"] and case["reshape_forms"]
    for form in case["flatten_forms"]:
        v = call_form(a.ss.flatten, form)
        check_vector(gb, v, want, "INT64", f"flatten {form}")
        for back in case["reshape_forms"]:
            check(call_form(v.ss.reshape, back), A, "INT64", what=f"reshape {back}")


def test_golden_reshape(gb):
    shape = tuple(G["reshape"]["resize"])
    A = rm.golden_A(G, shape)
    a = to_gb(gb, rm.golden_A(G))
    a.resize(*shape)
    rv = None
    for case in G["reshape"]["cases"]:
        want = rm.pair_of((case["nrows"], case["ncols"]), (case["rows"], case["cols"]), case["vals"])
        for form in case["forms"]:
            got = call_form(a.ss.reshape, form)
            check(got, want, "INT64", what=f"reshape {form}")
            rv = got if case["order"] == "rowwise" else rv
    back = G["reshape"]["inplace_back"]
    assert call_form(rv.ss.reshape, back) is None
    check(rv, A, "INT64", what="in place, back")
    check(a, A, "INT64", what="the operand is unchanged")


@pytest.mark.parametrize("case", G["errors"], ids=lambda c: c["src"])
def test_golden_errors(gb, case):
    a = to_gb(gb, rm.golden_A(G))
    if case["shape"] == G["reshape"]["resize"]:
        a.resize(*case["shape"])
    x = a.ss.flatten() if case["of"] == "v" else a
    with pytest.raises(ValueError, match=case["match"]):
        call_form(getattr(x.ss, case["method"]), case)


# ---------------------------------------------------------------------- diagonal matrix from a vector
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 129, 1000])
def test_vector_diag_sizes(gb, n):
    for density in (0, 0.5, 1):
        V = vector_of("INT64", n, density, "sizes")
        v = to_gb(gb, V)
        for k in (0, 1, -1, 64, -65, 200):
            check(v.diag(k), rm.diag_matrix(V, k), "INT64", what=f"n={n} density={density} k={k}")
    never = gb.Vector("INT64", n)  # no entry was ever written
    check(never.diag(-1), rm.diag_matrix(vector_of("INT64", n, 0, ""), -1), "INT64", what="never written")


@pytest.mark.parametrize("dt", TYPES)
def test_vector_diag_types_and_iso(gb, dt):
    for n in (1, 65, 1000):
        for k in (0, 1, -65):
            V = vector_of(dt, n, 0.5 if n > 1 else 1, "types")
            D = to_gb(gb, V).diag(k)
            check(D, rm.diag_matrix(V, k), dt, what=f"{dt} n={n} k={k}")
            assert not is_iso(D) or V[0].sum() <= 1
            value = draw(dt, rng_of("iso", dt, n, k), 1)[0]
            u, U = iso_gb(gb, V[0], value, dt)
            assert is_iso(u)
            D = u.diag(k)
            check(D, rm.diag_matrix(U, k), dt, what=f"iso {dt} n={n} k={k}")
            assert is_iso(D), "an iso vector gives an iso matrix"
            C = gb.Matrix(dt, n + abs(k), n + abs(k))
            C.ss.build_diag(u, k)
            check(C, rm.diag_matrix(U, k), dt, what=f"iso build_diag {dt} n={n} k={k}")
            assert is_iso(C)


def test_matrix_build_diag_casts_and_refuses(gb):
    V = vector_of("INT64", 129, 0.5, "cast")
    v = to_gb(gb, V)
    old = ragged(131, 131, "FP64", "old")
    for k in (2, -2):
        C = to_gb(gb, old)
        C.ss.build_diag(v, k)  # the old contents are discarded
        check(C, rm.diag_matrix(V, k, "FP64"), "FP64", what=f"INT64 into FP64, k={k}")
    small = vector_of("FP64", 70, 0.5, "sat")  # the saturating cast: NaN -> 0, inf -> 127
    C = gb.Matrix("INT8", 70, 70)
    C.ss.build_diag(to_gb(gb, small))
    check(C, rm.diag_matrix(small, 0, "INT8"), "INT8", what="FP64 into INT8")
    check(gb.ss.diag(v, 3, dtype="FP32"), rm.diag_matrix(V, 3, "FP32"), "FP32", what="ss.diag dtype")
    for shape, k in (((129, 129), 1), ((130, 131), 1), ((131, 131), 0)):
        C = to_gb(gb, ragged(*shape, "FP64", "refused"))
        with pytest.raises(gb.DimensionMismatch):
            C.ss.build_diag(v, k)
        check(C, ragged(*shape, "FP64", "refused"), "FP64", what=f"refused {shape} k={k}")
    lib = gb.lib
    assert lib.GrB_Matrix_diag(None, v._h, 0) == NULL_POINTER
    h = ctypes.c_void_p()
    assert lib.GrB_Matrix_diag(ctypes.byref(h), None, 0) == NULL_POINTER and not h.value
    assert lib.GxB_Matrix_diag(None, v._h, 0, None) == NULL_POINTER
    assert lib.GxB_Matrix_diag(C._h, None, 0, None) == NULL_POINTER


# ---------------------------------------------------------------------- diagonal of a matrix
KS = [0, 1, -1, 63, 64, -64, 229, 230, 299, 300, -69, -70, 1000, -1000]


@pytest.mark.parametrize("transposed", [False, True], ids=["70x300", "300x70"])
def test_matrix_diag_rows(gb, transposed):
    A = rows_matrix()
    A = dm.transpose(A) if transposed else A
    a = to_gb(gb, A)
    before = transposes_cached(gb)
    for k in KS:
        want = rm.diag_vector(A, k)
        check_vector(gb, a.diag(k), want, "INT64", f"k={k}")
        check_vector(gb, a.T.diag(-k), want, "INT64", f"A.T.diag({-k})")
        w = gb.Vector("INT64", want[0].size)
        assert gb.lib.GxB_Vector_diag(w._h, a._h, -k, gb.lib.GrB_DESC_T0) == 0  # A' through the descriptor
        check_vector(gb, w, want, "INT64", f"T0, k={-k}")
    assert transposes_cached(gb) == before, "a diagonal of A' must not build the transpose"
    assert gb.lib.GxB_Matrix_prepare_transpose(a._h) == 0
    assert transposes_cached(gb) == before + 1  # the counter does see one that is built


@pytest.mark.parametrize("dt", TYPES)
def test_matrix_diag_types_iso_and_casts(gb, dt):
    A = rows_matrix(dt)
    a = to_gb(gb, A)
    for k in (0, -5):
        check_vector(gb, a.diag(k), rm.diag_vector(A, k), dt, f"{dt} k={k}")
        check_vector(gb, a.diag(k, dtype="FP64"), rm.diag_vector(A, k, "FP64"), "FP64", f"{dt} -> FP64 k={k}")
        check_vector(gb, a.diag(k, dtype="INT8"), rm.diag_vector(A, k, "INT8"), "INT8", f"{dt} -> INT8 k={k}")
    value = draw(dt, rng_of("iso", dt), 1)[0]
    u, U = iso_gb(gb, A[0], value, dt)
    w = u.diag(1)
    check_vector(gb, w, rm.diag_vector(U, 1), dt, f"iso {dt}")
    assert is_iso(w)
    w = gb.Vector(dt, 70)
    w[:] = 1  # the old contents are discarded
    w.ss.build_diag(u, 0)
    check_vector(gb, w, rm.diag_vector(U, 0), dt, f"iso {dt} build_diag")


def test_matrix_diag_hub_and_refusals(gb):
    H = heavy("INT32", "diag")
    h = to_gb(gb, H)
    for k in (0, 5000):
        check_vector(gb, h.diag(k), rm.diag_vector(H, k), "INT32", f"heavy k={k}")
    a = to_gb(gb, rows_matrix())
    for size, k in ((69, 0), (71, 0), (70, 231), (0, 0), (1, 300)):
        w = to_gb(gb, vector_of("INT64", size, 0.5, "refused"))
        with pytest.raises(gb.DimensionMismatch):
            w.ss.build_diag(a, k)
        check_vector(gb, w, vector_of("INT64", size, 0.5, "refused"), "INT64", f"refused size={size} k={k}")
    empty = gb.Matrix("FP32", 5, 0)
    check_vector(gb, empty.diag(0), (np.zeros(0, bool), np.zeros(0, np.float32)), "FP32", "5 x 0")
    check_vector(gb, gb.Matrix("FP32", 5, 9).diag(2), (np.zeros(5, bool), np.zeros(5, np.float32)), "FP32", "no entries")
    lib = gb.lib
    w = gb.Vector("INT64", 70)
    assert lib.GxB_Vector_diag(None, a._h, 0, None) == NULL_POINTER
    assert lib.GxB_Vector_diag(w._h, None, 0, None) == NULL_POINTER
    for k, size in ((2 ** 63 - 1, 0), (-2 ** 63, 0)):  # any k is legal
        w = gb.Vector("INT64", size)
        assert lib.GxB_Vector_diag(w._h, a._h, k, None) == 0 and w.nvals == 0
        assert lib.GxB_Vector_diag(w._h, a._h, k, lib.GrB_DESC_T0) == 0 and w.nvals == 0


# ---------------------------------------------------------------------- reshape
def reshape_all_ways(gb, A, a, new, dt, what):
    """both orders, into a new matrix and in place, and back again"""
    for order in ORDERS:
        want = rm.reshape(A, new, order)
        got = a.ss.reshape(new, order=order)
        check(got, want, dt, what=f"{what} -> {new} {order}")
        assert gb.get_knob("stat_reshape_div64") == 0
        check(a, A, dt, what=f"{what}: the operand is unchanged")
        b = a.dup()
        assert b.ss.reshape(*new, order=order, inplace=True) is None
        assert b.shape == new
        check(b, want, dt, what=f"{what} -> {new} {order} in place")
        b.ss.reshape(A[0].shape, order=order, inplace=True)
        check(b, A, dt, what=f"{what} -> {new} -> back, {order} in place")
        check(got.ss.reshape(A[0].shape, order=order), A, dt, what=f"{what} -> {new} -> back, {order}")


@pytest.mark.parametrize("new", [(300, 70), (140, 150), (7, 3000), (3000, 7), (21000, 1), (1, 21000)])
def test_reshape_rows(gb, new):
    A = rows_matrix("FP64")
    reshape_all_ways(gb, A, to_gb(gb, A), new, "FP64", "rows")


@pytest.mark.parametrize("new", [(40, 400), (16000, 1)])
def test_reshape_empty_row_runs(gb, new):
    A = gappy_matrix()
    reshape_all_ways(gb, A, to_gb(gb, A), new, "INT32", "gappy")


def test_reshape_without_entries_or_positions(gb):
    E = np.zeros((70, 300), bool), np.zeros((70, 300), np.int8)
    reshape_all_ways(gb, E, gb.Matrix("INT8", 70, 300), (140, 150), "INT8", "empty")
    for new in ((5, 0), (0, 7)):
        Z = np.zeros((0, 5), bool), np.zeros((0, 5), np.float32)
        reshape_all_ways(gb, Z, gb.Matrix("FP32", 0, 5), new, "FP32", "0 x 5")


@pytest.mark.parametrize("dt", TYPES)
def test_reshape_types_and_iso(gb, dt):
    A = gappy_matrix(dt)
    reshape_all_ways(gb, A, to_gb(gb, A), (100, 160), dt, dt)
    value = draw(dt, rng_of("iso", dt), 1)[0]
    u, U = iso_gb(gb, A[0], value, dt)
    for order in ORDERS:
        got = u.ss.reshape(100, 160, order=order)
        check(got, rm.reshape(U, (100, 160), order), dt, what=f"iso {dt} {order}")
        assert is_iso(got), "iso stays iso"
        b = u.dup()
        b.ss.reshape(-1, 160, order=order, inplace=True)
        check(b, rm.reshape(U, (100, 160), order), dt, what=f"iso {dt} {order} in place")
        assert is_iso(b)


def test_inplace_row_major_keeps_the_values_and_drops_the_transpose(gb):
    from graphblas_amd.device import matrix_view

    rng = rng_of("stale")
    p = rows_matrix()[0]
    A = p, np.where(p, rng.integers(1, 100, p.shape), 0)
    a = to_gb(gb, A)
    assert gb.lib.GxB_Matrix_prepare_transpose(a._h) == 0  # the cached transpose of the 70 x 300 shape
    values = matrix_view(a._h).values
    a.ss.reshape(140, 150, inplace=True)
    assert matrix_view(a._h).values == values, "the in-place row-major reshape must not copy the values"
    R = rm.reshape(A, (140, 150))
    check(a.T.new(), dm.transpose(R), "INT64", what="A.T after the reshape")  # not the stale 300 x 70
    for obj, M, n in ((a, R[1], 150), (a.T, R[1].T, 140)):
        xs = rng.integers(1, 100, n)
        y = obj.mxv(gb.Vector.from_coo(np.arange(n), xs, size=n), gb.semiring.plus_times).new()
        want = M @ xs
        rows = np.flatnonzero((M != 0).any(axis=1))
        idx, vals = y.to_coo()
        assert np.array_equal(idx.astype(np.int64), rows) and np.array_equal(vals, want[rows]), n


@pytest.mark.parametrize("new", [(26625, 320), (2130000, 4)])
def test_reshape_many_chunks_per_wave(gb, new):
    A = ragged(133125, 64, "INT32", "reshape")
    a = to_gb(gb, A)
    assert a.nvals > 190000
    r, c = np.nonzero(A[0])
    for order in ORDERS:
        wr, wc, wx = rm.reshape_coo(r, c, A[1][r, c], A[0].shape, new, order)
        for inplace in (False, True):
            got = a.dup() if inplace else a.ss.reshape(new, order=order)
            if inplace:
                got.ss.reshape(new, order=order, inplace=True)
            gr, gc, gx = got.to_coo()
            assert got.shape == new and got.dtype == "INT32"
            assert np.array_equal(gr.astype(np.int64), wr) and np.array_equal(gc.astype(np.int64), wc), (order, inplace)
            assert np.array_equal(gx, wx), (order, inplace)
            assert gb.get_knob("stat_reshape_div64") == 0
    if new[1] == 320:
        check(a.ss.reshape(new).ss.reshape(133125, 64), A, "INT32", what="and back")


def big_matrix(gb):
    rng = rng_of("big")
    lin = np.sort(rng.choice(70000 * 70000, 1000, replace=False))
    lin[:3] = [0, 69999, 70000]
    lin[-1] = 70000 * 70000 - 1
    lin = np.unique(lin)
    r, c = np.divmod(lin, 70000)
    x = rng.integers(-10 ** 12, 10 ** 12, lin.size)
    return gb.Matrix.from_coo(r, c, x, nrows=70000, ncols=70000), r, c, x


@pytest.mark.parametrize("new", [(4900000, 1000), (100, 49000000)])
def test_reshape_64_bit_divisions(gb, new):
    a, r, c, x = big_matrix(gb)
    for order in ORDERS:
        wr, wc, wx = rm.reshape_coo(r, c, x, (70000, 70000), new, order)
        got = a.ss.reshape(new, order=order)
        assert gb.get_knob("stat_reshape_div64") == 1
        gr, gc, gx = got.to_coo()
        assert got.shape == new
        assert np.array_equal(gr.astype(np.int64), wr) and np.array_equal(gc.astype(np.int64), wc), order
        assert np.array_equal(gx, wx), order
        got.ss.reshape(70000, 70000, order=order, inplace=True)
        assert gb.get_knob("stat_reshape_div64") == 1
        gr, gc, gx = got.to_coo()
        assert np.array_equal(gr.astype(np.int64), r) and np.array_equal(gc.astype(np.int64), c), order
        assert np.array_equal(gx, x), order
    small = to_gb(gb, gappy_matrix())
    small.ss.reshape(40, 400)
    assert gb.get_knob("stat_reshape_div64") == 0


def test_reshape_refusals_leave_the_object_unchanged(gb):
    lib = gb.lib
    a, r, c, x = big_matrix(gb)

    def unchanged():
        gr, gc, gx = a.to_coo()
        n1, n2 = ctypes.c_uint64(), ctypes.c_uint64()
        lib.GrB_Matrix_nrows(ctypes.byref(n1), a._h)
        lib.GrB_Matrix_ncols(ctypes.byref(n2), a._h)
        return (n1.value, n2.value) == (70000, 70000) and np.array_equal(gr.astype(np.int64), r) \
            and np.array_equal(gc.astype(np.int64), c) and np.array_equal(gx, x)

    h = ctypes.c_void_p()
    for by_col in (False, True):
        for nr, nc, code in ((1, 4900000000, OUT_OF_MEMORY),        # the columns do not fit the device index
                             (4900000, 1001, DIMENSION_MISMATCH),   # another number of positions
                             (2 ** 40, 2 ** 40, DIMENSION_MISMATCH),  # a product beyond 64 bits
                             (2 ** 63, 2 ** 63, DIMENSION_MISMATCH),
                             (4900000000 + 2 ** 32, 2 ** 32 + 1, DIMENSION_MISMATCH)):
            assert lib.GxB_Matrix_reshape(a._h, by_col, nr, nc, None) == code, (by_col, nr, nc)
            assert unchanged(), (by_col, nr, nc)
            assert lib.GxB_Matrix_reshapeDup(ctypes.byref(h), a._h, by_col, nr, nc, None) == code
            assert not h.value
    with pytest.raises(gb.OutOfMemory):
        a.ss.reshape(1, -1)
    with pytest.raises(gb.OutOfMemory):
        a.ss.reshape(1, -1, inplace=True)
    assert a.shape == (70000, 70000) and unchanged()
    assert lib.GxB_Matrix_reshape(None, False, 1, 1, None) == NULL_POINTER
    assert lib.GxB_Matrix_reshapeDup(None, a._h, False, 70000, 70000, None) == NULL_POINTER
    assert lib.GxB_Matrix_reshapeDup(ctypes.byref(h), None, False, 1, 1, None) == NULL_POINTER


# ---------------------------------------------------------------------- flatten and Vector.ss.reshape
@pytest.mark.parametrize("which", ["rows", "gappy", "7x9", "3x64", "5x13"])
def test_flatten_and_back(gb, which):
    if which == "rows":
        A, dt = rows_matrix("FP64"), "FP64"
    elif which == "gappy":
        A, dt = gappy_matrix(), "INT32"
    else:
        shape = {"7x9": (7, 9), "3x64": (3, 64), "5x13": (5, 13)}[which]
        rng, dt = rng_of("flat", which), "INT64"
        p = rng.random(shape) < 0.5 if which == "7x9" else np.ones(shape, bool)  # full: entries share and straddle words
        A = p, np.where(p, draw(dt, rng, p.size).reshape(shape), 0)
    a = to_gb(gb, A)
    for order in ORDERS:
        v = a.ss.flatten(order)
        check_vector(gb, v, rm.flatten(A, order), dt, f"{which} {order}")
        check(v.ss.reshape(*A[0].shape, order), A, dt, what=f"{which} {order} back")
        check(v.ss.reshape(A[0].shape[::-1], order=order), rm.reshape(rm.flatten(A, order), A[0].shape[::-1], order),
              dt, what=f"{which} {order} other shape")
    check(a, A, dt, what="the operand is unchanged")


@pytest.mark.parametrize("dt", TYPES)
def test_flatten_types_iso_and_casts(gb, dt):
    A = gappy_matrix(dt)
    a = to_gb(gb, A)
    lib = gb.lib
    for order in ORDERS:
        check_vector(gb, a.ss.flatten(order), rm.flatten(A, order), dt, f"{dt} {order}")
        w = gb.Vector("FP32", 16000)
        w[:] = 1  # the old contents are discarded
        assert lib.GxB_Vector_flatten(w._h, a._h, order == "columnwise", None) == 0
        check_vector(gb, w, rm.flatten(A, order, "FP32"), "FP32", f"{dt} -> FP32 {order}")
    value = draw(dt, rng_of("iso", dt), 1)[0]
    u, U = iso_gb(gb, A[0], value, dt)
    v = u.ss.flatten("F")
    check_vector(gb, v, rm.flatten(U, "columnwise"), dt, f"iso {dt}")
    assert is_iso(v)
    got = v.ss.reshape(400, 40, "F")
    check(got, U, dt, what=f"iso {dt} back")
    assert is_iso(got)
    never = gb.Vector(dt, 600)
    check(never.ss.reshape(20, 30), (np.zeros((20, 30), bool), np.zeros((20, 30), dm.NP[dt])), dt, what="never written")


def test_flatten_refusals(gb):
    lib = gb.lib
    a = to_gb(gb, rows_matrix())
    for size in (20999, 21001, 0):
        W = vector_of("INT64", size, 0.5, "refused")
        w = to_gb(gb, W)
        assert lib.GxB_Vector_flatten(w._h, a._h, False, None) == DIMENSION_MISMATCH
        check_vector(gb, w, W, "INT64", f"refused {size}")
    w = gb.Vector("INT64", 21000)
    assert lib.GxB_Vector_flatten(None, a._h, False, None) == NULL_POINTER
    assert lib.GxB_Vector_flatten(w._h, None, False, None) == NULL_POINTER
    v = a.ss.flatten()
    with pytest.raises(ValueError, match="cannot reshape array of size 21000"):
        v.ss.reshape(7, 7)
    assert lib.GxB_Matrix_reshape(v._h, False, 21000, 1, None) == 0  # a vector keeps its one column
    assert lib.GxB_Matrix_reshape(v._h, False, 1, 21000, None) == -3
    check_vector(gb, v, rm.flatten(rows_matrix()), "INT64", "a vector handle in place")


# ---------------------------------------------------------------------- aggregators over the new diag
def test_argmin_argmax_rows(gb):
    rng = rng_of("agg")
    p = rng.random((70, 300)) < 0.2
    p[::9] = False
    x = rng.integers(-50, 50, p.shape)  # ties: the first column wins
    a = to_gb(gb, (p, np.where(p, x, 0)))
    for name, fn, fill in (("argmin", np.argmin, 10 ** 6), ("argmax", np.argmax, -10 ** 6)):
        got = a.reduce_rowwise(getattr(gb.agg.ss, name)).new()
        rows = np.flatnonzero(p.any(axis=1))
        want = fn(np.where(p, x, fill), axis=1)[rows]
        idx, vals = got.to_coo()
        assert np.array_equal(idx.astype(np.int64), rows), name
        assert np.array_equal(vals.astype(np.int64), want), name
