"""Dense import and export on the device (csrc/gb_reindex.hip: k_dense_flags, k_dense_fill,
k_dense_scatter, k_bitmap_dense behind GxB_{Matrix,Vector}_{import,export}_dense and from_dense /
to_dense) against the numpy model of tests/dense_io_model.py.  Every value is moved, never
computed: device objects are compared through test_general_ops_gpu.check (structure, order, nvals,
dtype, values, NaN, the sign of zero) and their values bit for bit, vectors also through their
bitmap words, exported arrays bit for bit as unsigned integers.

Shapes, and what each one is for
  vectors 0, 1, 63, 64, 65, 127, 1000   no word, a partial word, exactly one word, one bit into the
                       next, and more than one chunk of positions
  0 x 5, 5 x 0, 1 x 1  no positions (no array is touched), one position
  7 x 7                the reference's fixture
  5 x 3                several rows inside one 64-position word
  3 x 64, 3 x 65       rows ending on and one past a word
  1 x 1000, 1000 x 1   one long row, one entry per row
  rows 70 x 300        rows of 0, 1, 63, 64, 65, 128, 129 and 300 entries
  gappy 400 x 40       runs of more than 64 empty rows: gb_chunk_rows across empty runs in the export,
                       equal row pointers over a run in the import
  301 x 6007           one full row among sparse ones
  65537 x 65536        2^32 + 65536 positions of one byte: the 64-bit division of k_bitmap_csr
                       ("stat_reshape_div64" = 1); every other shape takes the 32-bit path
  1300 x 700, 70001    the grid-sweep suite's shapes, under grid_cap 1, 3, 33 and 0
"""
import ctypes
import os
import time

import numpy as np
import pytest

import dense_io_model as dio
import dense_model as dm
import reindex_model as rm
from test_general_ops_gpu import check, coo_of, draw, iso_gb, to_gb
from test_reindex_gpu import check_vector, gappy_matrix, rng_of, rows_matrix

pytestmark = pytest.mark.gpu

G = dio.golden()
TYPES = ["BOOL", "INT8", "INT64", "FP32", "FP64"]
TORCH_TYPES = ["BOOL", "INT8", "UINT8", "INT16", "INT32", "INT64", "FP32", "FP64"]
VECTORS = [0, 1, 63, 64, 65, 127, 1000]
MATRICES = [(0, 5), (5, 0), (1, 1), (7, 7), (5, 3), (3, 64), (3, 65), (1, 1000), (1000, 1)]
NULL_POINTER, INVALID_VALUE, OUT_OF_MEMORY = -2, -3, -102
BITMAP_BYTES = np.array([0, 1, 2, -1], np.int8)


@pytest.fixture(scope="module")
def gb():
    import graphblas_amd

    yield graphblas_amd
    graphblas_amd.set_knob("grid_cap", 0)


@pytest.fixture(scope="module", autouse=True)
def report_run_time():
    t0 = time.perf_counter()
    yield
    print(f"\ntest_dense_io_gpu.py: {time.perf_counter() - t0:.1f} s")


# ---------------------------------------------------------------------- arrays, host and device
def placed(x, order, device):
    """the numpy array x in C or F order, on the host or as a torch CUDA tensor of the same strides"""
    if x is None:
        return None
    if not device:
        return np.asfortranarray(x) if order == "F" else np.ascontiguousarray(x)
    import torch

    if order == "F" and x.ndim == 2:
        return torch.from_numpy(np.ascontiguousarray(x.T)).cuda().T
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def empty_out(shape, np_type, order, device):
    """an output array with every byte 0x5a (BOOL: true), so that an untouched position shows"""
    size = np.dtype(np_type).itemsize
    x = np.ones(shape, np.bool_) if np_type == np.bool_ \
        else np.full(tuple(shape) + (size,), 0x5a, np.uint8).view(np_type).reshape(shape)
    return placed(x, order, device)


def to_host(x):
    if isinstance(x, np.ndarray):
        return x
    import torch

    torch.cuda.synchronize()
    return x.cpu().numpy()


def do_import(gb, X, missing=None, bitmap=None, *, order="C", device=False, **kw):
    cls = gb.Vector if X.ndim == 1 else gb.Matrix
    x, b = placed(X, order, device), placed(bitmap, order, device)
    if device:
        import torch

        torch.cuda.synchronize()
    A = cls.from_dense(x, missing, bitmap=b, **kw)
    if device:
        A.wait()
    return A


def check_object(gb, obj, want, dt, what):
    """the model's structure and values: check(), the values bit for bit, a vector's bitmap words"""
    if obj.ndim == 1:
        check_vector(gb, obj, want, dt, what)
    else:
        check(obj, want, dt, what=what)
    assert np.array_equal(dio.bits(coo_of(obj)[1]), dio.bits(want[1][want[0]])), f"{what}: value bits"


def absent_value(A):
    """a value of A's type that none of its entries holds (and no zero: both zeros compare equal);
    None when a one-byte type has them all"""
    p, v = A
    t = v.dtype.type
    if t == np.bool_:
        return None if (v[p].any() and not v[p].all()) else t(not v[p].any())
    have = set(v[p].tolist())
    return next((t(c) for c in (77, 99, 101, 33, 12, 55, 66, 111, 123, *range(1, 128)) if t(c).item() not in have), None)


def import_configs(X, key):
    """(name, missing value, bitmap) for the array X: none; 0; a value that occurs; a bitmap of the
    bytes 0, 1, 2, -1 of density about 0.3, alone, as bool, as uint8 and with a missing value; an
    empty bitmap"""
    rng = rng_of("import", X.shape, X.dtype.name, key)
    t = X.dtype.type
    occurs = X.ravel()[rng.integers(X.size)] if X.size else t(1)
    bm = rng.choice(BITMAP_BYTES, X.shape, p=[0.7, 0.1, 0.1, 0.1])
    return [("dense", None, None), ("missing 0", t(0), None), ("missing that occurs", occurs, None),
            ("bitmap", None, bm), ("bool bitmap", None, bm != 0), ("uint8 bitmap", None, bm.view(np.uint8)),
            ("bitmap and missing", occurs, bm), ("empty bitmap", None, np.zeros(X.shape, np.int8))]


def check_export(gb, a, A, fill=None, dtype=None, *, order="C", out=False, bitmap=False, device=False, what=""):
    """a.to_dense(...) against the model, bit for bit; returns the array"""
    want, wab = dio.export_dense(A, fill, dtype, upcast=a.ndim == 2, bitmap=bitmap)
    o = empty_out(want.shape, want.dtype.type, order, device) if out or device else None
    b = empty_out(want.shape, np.int8, order if o is not None else "C", device) if bitmap else None
    if device:
        import torch

        torch.cuda.synchronize()
    got = a.to_dense(fill, dtype, out=o, bitmap=b)
    if device:
        a.wait()
    if o is not None:
        assert got is o, what
    got = to_host(got)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype)
    assert np.array_equal(dio.bits(got), dio.bits(want)), f"{what}: exported values"
    if bitmap:
        assert np.array_equal(to_host(b), wab), f"{what}: exported bitmap"
    return got


def run_all(gb, X, key, *, device=False, orders=("C",)):
    """every import configuration of X, and the exports of each imported object"""
    dt = dm.name_of(X.dtype)
    results = []
    for name, missing, bm in import_configs(X, key):
        for order in orders:
            what = f"{dt} {X.shape} {name} {order}{' device' if device else ''}"
            want = dio.import_dense(X, missing, bm)
            a = do_import(gb, X, missing, bm, order=order, device=device)
            check_object(gb, a, want, dt, what)
            results.append(coo_of(a))
            if not X.size:
                assert a.to_dense().shape == X.shape
                continue
            f = absent_value(want)
            if f is not None:
                check_export(gb, a, want, f, order=order, out=order == "F", device=device, what=what + " export")
                check_export(gb, a, want, f, order=order, out=True, bitmap=True, device=device,
                             what=what + " export with bitmap")
            check_export(gb, a, want, None, bitmap=True, device=device, what=what + " export without fill")
            if want[0].all():
                check_export(gb, a, want, None, order=order, device=device, what=what + " full, no fill")
    return results


def random_array(dt, shape, key):
    rng = rng_of("array", dt, shape, key)
    return draw(dt, rng, int(np.prod(shape))).reshape(shape)


# ---------------------------------------------------------------------- the reference's own cases
def golden_device_object(gb, desc):
    cls = getattr(gb, desc["kind"])
    if desc["how"] == "from_dense":
        a = cls.from_dense(*desc["args"], **desc["kwargs"])
    else:
        a = cls.from_coo(*desc["args"], **desc["kwargs"])
    for step, arg in desc["steps"]:
        if step == "del":
            del a[tuple(arg)]
        else:
            a.resize(*arg)
    return a


@pytest.mark.parametrize("case", [c for c in G if c["check"] != "raises" or c["method"] == "to_dense"],
                         ids=lambda c: c["src"])
def test_golden_cases(gb, case):
    if case["check"] == "isequal":
        a, b = golden_device_object(gb, case["left"]), golden_device_object(gb, case["right"])
        want = dio.golden_object(case["right"])
        check_object(gb, a, want, dm.name_of(want[1].dtype), case["src"])
        assert a.isequal(b, check_dtype=True)
        return
    a = golden_device_object(gb, case["of"])
    if case["check"] == "raises":
        from test_dense_io_abi import argument

        with pytest.raises(TypeError, match=case["match"]):
            a.to_dense(*[argument(x) for x in case["args"]])
        return
    fill, dtype = dio.golden_call(case)
    got = (a.T if case["T"] else a).to_dense(fill, dtype)
    want = np.asarray(case["expect"])
    assert got.shape == want.shape and np.array_equal(got, want) and got.dtype.kind == want.dtype.kind
    model = dio.golden_object(case["of"])
    model = dm.transpose(model) if case["T"] else model
    if a.ndim == 2:
        assert got.dtype == dio.export_dense(model, fill, dtype)[0].dtype


def test_golden_fixture(gb):
    """the 7 x 7 of the reference's tests, through from_dense(A.to_dense(f), f)"""
    A = rm.golden_A(rm.golden())
    a = to_gb(gb, A)
    f = absent_value(A)
    dense = check_export(gb, a, A, f, what="7 x 7")
    check_object(gb, gb.Matrix.from_dense(dense, f), A, "INT64", "7 x 7 round trip")
    check_export(gb, a.T, dm.transpose(A), f, what="7 x 7 transposed")


# ---------------------------------------------------------------------- shapes x types
@pytest.mark.parametrize("dt", TYPES)
@pytest.mark.parametrize("n", VECTORS)
def test_vectors(gb, n, dt):
    run_all(gb, random_array(dt, (n,), "v"), "v")
    assert gb.get_knob("stat_reshape_div64") == 0


@pytest.mark.parametrize("dt", TYPES)
@pytest.mark.parametrize("shape", MATRICES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_matrices(gb, shape, dt):
    run_all(gb, random_array(dt, shape, "m"), "m", orders=("C", "F"))
    assert gb.get_knob("stat_reshape_div64") == 0


@pytest.mark.parametrize("dt", dm.ALL)
def test_every_type(gb, dt):
    run_all(gb, random_array(dt, (37, 53), "t"), "t")
    run_all(gb, random_array(dt, (129,), "t"), "t")


def full_row_matrix(dt):
    """301 x 6007 of density 0.01 with row 7 full"""
    rng = rng_of("full row", dt)
    p = rng.random((301, 6007)) < 0.01
    p[7] = True
    return p, np.where(p, draw(dt, rng, p.size).reshape(p.shape), dm.NP[dt](0))


@pytest.mark.parametrize("name,dt", [("rows", "INT64"), ("rows", "FP32"), ("gappy", "INT32"), ("gappy", "BOOL"),
                                     ("full row", "INT8"), ("full row", "FP64")])
def test_structured_matrices(gb, name, dt):
    """a given structure in and out: as a bitmap of the bytes 1, 2 and -1, and as a missing value"""
    A = {"rows": rows_matrix, "gappy": gappy_matrix, "full row": full_row_matrix}[name](dt)
    p, v = A
    rng = rng_of("structured", name, dt)
    bm = np.where(p, rng.choice(BITMAP_BYTES[1:], p.shape), np.int8(0))
    noise = random_array(dt, p.shape, name)  # what a position without an entry holds is never read as a value
    for order in ("C", "F"):
        a = do_import(gb, np.where(p, v, noise), None, bm, order=order)
        check_object(gb, a, A, dt, f"{name} {dt} bitmap {order}")
    f = absent_value(A)
    if f is not None:
        X = np.where(p, v, f)
        for order in ("C", "F"):
            check_object(gb, do_import(gb, X, f, order=order), A, dt, f"{name} {dt} missing {order}")
            got = check_export(gb, a, A, f, order=order, out=True, bitmap=True, what=f"{name} {dt} export {order}")
            assert np.array_equal(dio.bits(got), dio.bits(X))
        check_export(gb, a.T, dm.transpose(A), f, what=f"{name} {dt} transposed export")
        check_object(gb, gb.Matrix.from_dense(a.to_dense(f), f), A, dt, f"{name} {dt} round trip")
    check_export(gb, a, A, None, bitmap=True, what=f"{name} {dt} export without fill")


# ---------------------------------------------------------------------- the missing value
def test_missing_value_semantics(gb):
    nan = np.nan
    for t, dt in ((np.float64, "FP64"), (np.float32, "FP32")):
        X = np.array([[0.0, -0.0, nan, 1.5], [-nan, np.inf, -0.0, 0.0]], t)
        for missing in (None, t(nan), t(0.0), t(-0.0), t(1.5), 0, False, 1.5):
            want = dio.import_dense(X, missing)
            check_object(gb, gb.Matrix.from_dense(X, missing), want, dt, f"{dt} missing {missing!r}")
            check_object(gb, gb.Vector.from_dense(X[0], missing), dio.import_dense(X[0], missing), dt,
                         f"{dt} vector missing {missing!r}")
        assert gb.Matrix.from_dense(X, t(nan)).nvals == 8 and gb.Matrix.from_dense(X, 0.0).nvals == 4
    B = np.array([True, False, False, True, True])
    check_object(gb, gb.Vector.from_dense(B, False), dio.import_dense(B, False), "BOOL", "BOOL missing False")
    check_object(gb, gb.Vector.from_dense(B, True), dio.import_dense(B, True), "BOOL", "BOOL missing True")
    # an INT64 missing value given to an INT8 array is cast: 300 is 44
    X8 = np.array([[44, 3, -1], [0, 44, 127]], np.int8)
    for missing in (300, np.int64(300), np.int64(-1), 44):
        check_object(gb, gb.Matrix.from_dense(X8, missing), dio.import_dense(X8, missing), "INT8",
                     f"INT8 missing {missing!r}")
    assert gb.Matrix.from_dense(X8, 300).nvals == 4
    s = gb.Scalar.from_value(44, "INT64")
    check_object(gb, gb.Matrix.from_dense(X8, s), dio.import_dense(X8, 44), "INT8", "a Scalar")
    check_object(gb, gb.Matrix.from_dense(X8, gb.Scalar("INT64")), dio.import_dense(X8), "INT8", "an empty Scalar")
    # lists, and dtype= as from_coo converts values
    check_object(gb, gb.Matrix.from_dense([[1, 2], [3, 4]], 3, dtype="FP32"),
                 dio.import_dense(np.array([[1, 2], [3, 4]], np.float32), 3), "FP32", "a list with dtype")
    # an array in neither order goes through a contiguous copy
    X = random_array("INT64", (12, 10), "strided")[::2, ::3]
    check_object(gb, gb.Matrix.from_dense(X, X[0, 0]), dio.import_dense(X, X[0, 0]), "INT64", "strided")
    check_object(gb, gb.Vector.from_dense(X[:, 1], bitmap=X[:, 2] > 0), dio.import_dense(X[:, 1], None, X[:, 2] > 0),
                 "INT64", "strided vector")


# ---------------------------------------------------------------------- residence
@pytest.mark.parametrize("dt", TORCH_TYPES)
def test_device_arrays_give_what_host_arrays_give(gb, dt):
    for shape, orders in (((3, 65), ("C", "F")), ((65,), ("C",))):
        X = random_array(dt, shape, "residence")
        host = run_all(gb, X, "residence", orders=orders)
        dev = run_all(gb, X, "residence", orders=orders, device=True)
        assert len(host) == len(dev)
        for (hi, hv), (di, dv) in zip(host, dev):
            assert all(np.array_equal(a, b) for a, b in zip(hi, di)) and np.array_equal(dio.bits(hv), dio.bits(dv))


def test_device_arrays_of_another_type_and_bad_strides(gb):
    import torch

    X = random_array("INT32", (5, 3), "dup")
    a = do_import(gb, X, X[0, 0], device=True, dtype="FP64")
    p, v = dio.import_dense(X, X[0, 0])
    check_object(gb, a, (p, v.astype(np.float64)), "FP64", "imported in its own type, then dup(dtype)")
    t = torch.zeros((8, 6), dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError, match="C- or F-contiguous"):
        gb.Matrix.from_dense(t[::2, ::2])
    with pytest.raises(ValueError, match="must live where the values do"):
        gb.Matrix.from_dense(t, bitmap=np.ones((8, 6), bool))
    with pytest.raises(ValueError, match="must live where the values do"):
        gb.Matrix.from_dense(np.zeros((8, 6)), bitmap=t.to(torch.int8))
    with pytest.raises(ValueError, match="same order"):
        gb.Matrix.from_dense(t, bitmap=torch.ones((6, 8), dtype=torch.bool, device="cuda").T)


# ---------------------------------------------------------------------- export
def test_export_fill_rules(gb):
    A = (np.array([[True, False, True], [True, True, False]]), np.array([[7, 0, -2], [3, 4, 0]], np.int64))
    a = to_gb(gb, A)
    assert check_export(gb, a, A, 6.5).dtype == np.float64          # the fill upcasts
    assert check_export(gb, a, A, 6.5, "INT64").tolist() == [[7, 6, -2], [3, 4, 6]]
    assert a.to_dense(6.5, int).dtype == np.int64 and a.to_dense(6.5, int).tolist() == [[7, 6, -2], [3, 4, 6]]
    assert check_export(gb, a, A, gb.Scalar.from_value(6.5).value, "FP32").dtype == np.float32
    assert a.to_dense(gb.Scalar.from_value(6.5)).tolist() == [[7, 6.5, -2], [3, 4, 6.5]]
    assert check_export(gb, a, A, np.nan, "INT8", out=True).tolist() == [[7, 0, -2], [3, 4, 0]]   # NaN casts to 0
    assert check_export(gb, a, A, -1, "UINT8", out=True, bitmap=True)[0, 1] == 255
    assert check_export(gb, a, A, 300, "INT8", out=True)[0, 1] == 44
    assert check_export(gb, a.T, dm.transpose(A), 9, order="F", out=True).shape == (3, 2)
    v = to_gb(gb, (A[0][0], A[1][0]))
    # a Vector's out= / bitmap= path keeps its type unless out says otherwise; the plain path is as it was
    assert check_export(gb, v, (A[0][0], A[1][0]), 6.5, bitmap=True).tolist() == [7, 6, -2]
    assert check_export(gb, v, (A[0][0], A[1][0]), 6.5, out=True).dtype == np.int64
    out = np.zeros(3)
    assert v.to_dense(6.5, out=out) is out and out.tolist() == [7, 6.5, -2]
    assert v.to_dense(6.5).tolist() == [7, 6, -2] and v.to_dense(6.5).dtype == np.int64
    assert v.to_dense(6.5, dtype=float).tolist() == [7, 6.5, -2]


def test_export_without_fill(gb):
    lib = gb.lib
    full = (np.ones((3, 5), bool), random_array("FP32", (3, 5), "full"))
    f = to_gb(gb, full)
    assert np.array_equal(dio.bits(f.to_dense()), dio.bits(full[1]))
    assert np.array_equal(dio.bits(f.T.to_dense()), dio.bits(np.ascontiguousarray(full[1].T)))
    assert f.to_dense(4.5).dtype == np.float32 and f.to_dense(dtype="FP64").dtype == np.float64
    fv = to_gb(gb, (full[0][1], full[1][1]))
    assert np.array_equal(dio.bits(fv.to_dense(out=np.zeros(5, np.float32))), dio.bits(full[1][1]))
    A = (full[0].copy(), full[1])
    A[0][1, 2] = False
    for a, shape in ((to_gb(gb, A), (3, 5)), (to_gb(gb, A).T, (5, 3)), (to_gb(gb, (A[0][1], A[1][1])), (5,))):
        out = np.full(shape, 42, np.float32)
        with pytest.raises(TypeError, match="fill_value must be given in `to_dense` when there are missing values"):
            a.to_dense(out=out)
        with pytest.raises(TypeError, match="fill_value must be given"):
            a.to_dense()
        assert (out == 42).all()
        h = (a._matrix if a.ndim == 2 and hasattr(a, "_matrix") else a)._h
        X = ctypes.c_void_p(out.ctypes.data)
        if a.ndim == 2:
            assert lib.GxB_Matrix_export_dense(X, None, h, None, False, False) == INVALID_VALUE
            assert lib.GxB_Matrix_export_dense(X, None, h, gb.Scalar("FP32")._h, True, False) == INVALID_VALUE
        else:
            assert lib.GxB_Vector_export_dense(X, None, h, None, False) == INVALID_VALUE
        assert (out == 42).all()


@pytest.mark.parametrize("dt", ["BOOL", "INT8", "INT64", "FP32", "FP64"])
def test_export_iso_objects(gb, dt):
    value = {"BOOL": True, "FP32": -0.0}.get(dt, 3)
    for shape in ((70, 300), (127,), (3, 64)):
        rng = rng_of("iso", dt, shape)
        for density in (0.3, 1.0):
            a, A = iso_gb(gb, rng.random(shape) < density, value, dt)
            f = absent_value(A)
            for order in ("C", "F"):
                if f is not None:
                    check_export(gb, a, A, f, order=order, out=True, bitmap=True, what=f"iso {dt} {shape}")
                check_export(gb, a, A, None, order=order, out=True, bitmap=True, what=f"iso {dt} {shape} no fill")
            if a.ndim == 2 and f is not None:
                check_export(gb, a.T, dm.transpose(A), f, what=f"iso {dt} {shape} transposed")
    m, M = gb.Matrix.from_scalar(value, 5, 66, dt), (np.ones((5, 66), bool), np.full((5, 66), value, dm.NP[dt]))
    check_object(gb, m, M, dt, "Matrix.from_scalar")
    check_export(gb, m, M, None, what="from_scalar export")
    v = gb.Vector.from_scalar(gb.Scalar.from_value(value, dt), 65)
    check_object(gb, v, (np.ones(65, bool), np.full(65, value, dm.NP[dt])), dt, "Vector.from_scalar")
    assert gb.Vector.from_scalar(2.5, 3).dtype == "FP64" and gb.Matrix.from_scalar(2, 0, 4).shape == (0, 4)


def test_export_a_column_word_matrix(gb):
    """the result of a masked scalar assign under the colbits knob (held as column words when the
    library chooses to) exports like any other"""
    rng = rng_of("colwords")
    p = rng.random((4, 300)) < 0.3
    A = (p, p.copy())
    gb.set_knob("colbits", 1)
    try:
        V = gb.Matrix(bool, 4, 300)
        V(mask=to_gb(gb, A).V)[:, :] = True
        check_export(gb, V, A, False, out=True, bitmap=True, what="column words")
        check_export(gb, V.T, dm.transpose(A), False, what="column words, transposed")
    finally:
        gb.set_knob("colbits", 0)


# ---------------------------------------------------------------------- the C errors
def test_c_errors(gb):
    lib = gb.lib
    h = ctypes.c_void_p()
    X = np.arange(6, dtype=np.int64)
    px = ctypes.c_void_p(X.ctypes.data)
    T = gb.dtypes.INT64._carg
    im, iv = lib.GxB_Matrix_import_dense, lib.GxB_Vector_import_dense
    assert im(None, T, 2, 3, px, None, None, False, False) == NULL_POINTER
    assert iv(None, T, 6, px, None, None, False) == NULL_POINTER
    assert im(ctypes.byref(h), T, 2, 3, None, None, None, False, False) == NULL_POINTER and not h.value
    assert iv(ctypes.byref(h), T, 6, None, None, None, False) == NULL_POINTER and not h.value
    # what GrB_Matrix_new refuses, with its code; by_col builds the transpose, so either dimension is a column once
    big = ctypes.c_void_p()
    for nr, nc in ((1, 2 ** 31), (2 ** 61, 1), (1, 2 ** 61)):
        code = lib.GrB_Matrix_new(ctypes.byref(big), T, nr, nc)
        assert code != 0 and not big.value
        for by_col in (False, True):
            assert im(ctypes.byref(h), T, nr, nc, px, None, None, by_col, False) == code and not h.value
    assert lib.GrB_Matrix_new(ctypes.byref(big), T, 2 ** 31, 1) == 0
    lib.GrB_Matrix_free(ctypes.byref(big))
    assert im(ctypes.byref(h), T, 2 ** 31, 1, px, None, None, True, False) == OUT_OF_MEMORY and not h.value
    assert iv(ctypes.byref(h), T, 2 ** 61, px, None, None, False) == lib.GrB_Vector_new(ctypes.byref(big), T, 2 ** 61)
    assert not h.value and not big.value
    # nrows * ncols must fit 63 bits
    for by_col in (False, True):
        assert im(ctypes.byref(h), T, 2 ** 33, 2 ** 30, px, None, None, by_col, False) == OUT_OF_MEMORY and not h.value
    assert X.tolist() == list(range(6))
    # zero positions is a valid call and touches no array
    for nr, nc in ((0, 5), (5, 0), (0, 0)):
        for by_col in (False, True):
            assert im(ctypes.byref(h), T, nr, nc, None, None, None, by_col, False) == 0 and h.value
            n = ctypes.c_uint64(7)
            assert lib.GrB_Matrix_nvals(ctypes.byref(n), h) == 0 and n.value == 0
            assert lib.GxB_Matrix_export_dense(None, None, h, None, by_col, False) == 0
            lib.GrB_Matrix_free(ctypes.byref(h))
    assert iv(ctypes.byref(h), T, 0, None, None, None, False) == 0 and h.value
    assert lib.GxB_Vector_export_dense(None, None, h, None, False) == 0
    lib.GrB_Vector_free(ctypes.byref(h))
    a = gb.Matrix.from_dense(X.reshape(2, 3))
    assert lib.GxB_Matrix_export_dense(None, None, a._h, None, False, False) == NULL_POINTER
    assert lib.GxB_Matrix_export_dense(px, None, None, None, False, False) == NULL_POINTER
    assert lib.GxB_Vector_export_dense(px, None, None, None, False) == NULL_POINTER
    assert X.tolist() == list(range(6))


# ---------------------------------------------------------------------- 64-bit positions
def test_positions_past_2_to_the_32(gb):
    """65537 x 65536 bytes on the device (4.3 GB; nothing of that size on the host): the position
    arithmetic of k_dense_flags and the 64-bit division of k_bitmap_csr"""
    import torch

    nr, nc = 65537, 65536
    rng = rng_of("wide")
    rows = np.concatenate([[0, 0, 65535, 65535, 65536, 65536, 1, 65534], rng.integers(0, nr, 300)])
    cols = np.concatenate([[0, nc - 1, 0, nc - 1, 0, nc - 1, 63, 64], rng.integers(0, nc, 300)])
    t = torch.zeros((nr, nc), dtype=torch.bool, device="cuda")
    t[torch.from_numpy(rows).cuda(), torch.from_numpy(cols).cuda()] = True
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a = gb.Matrix.from_dense(t, False)
    a.wait()
    r, c, x = a.to_coo()
    print(f"\n65537 x 65536 BOOL import: {time.perf_counter() - t0:.2f} s")
    assert gb.get_knob("stat_reshape_div64") == 1
    del t
    lin = np.unique(rows.astype(np.int64) * nc + cols)
    assert a.shape == (nr, nc) and a.dtype == "BOOL" and a.nvals == lin.size
    assert np.array_equal(r.astype(np.int64) * nc + c.astype(np.int64), lin) and x.all()
    small = gb.Matrix.from_dense(np.ones((3, 3)))
    assert gb.get_knob("stat_reshape_div64") == 0 and small.nvals == 9


# ---------------------------------------------------------------------- grid sweeps
def chunk_grid_site():
    """stat_grid_clamped's key of the gb_grid( call of chunk_grid() in csrc/gb_reindex.hip"""
    import test_grid_sweeps_gpu as sweeps

    with open(os.path.join(sweeps.CSRC, "gb_reindex.hip")) as f:
        lines = f.read().split("\n")
    start = next(i for i, text in enumerate(lines) if text.startswith("unsigned chunk_grid("))
    line = next(i for i in range(start, start + 6) if "gb_grid(" in lines[i])
    return f"stat_grid_clamped:gb_reindex.hip:{line + 1}"


def test_grid_sweeps(gb):
    """import and export of the sweep suite's shapes under grid_cap 1, 3, 33 and 0: equal results,
    and chunk_grid()'s clamp bites at cap 1"""
    import test_grid_sweeps_gpu as sweeps

    A, u = sweeps.mat("INT64", sweeps.SHAPE, "dense io"), sweeps.vec("FP64", sweeps.NVEC, "half", "dense io")
    fA, fu = absent_value(A), absent_value(u)
    XA, Xu = np.where(A[0], A[1], fA), np.where(u[0], u[1], fu)
    site = chunk_grid_site()
    seen = []
    try:
        for cap in (1, 3, 33, 0):
            before = gb.get_knob(site)
            gb.set_knob("grid_cap", cap)
            what = f"grid_cap={cap}"
            outs = []
            for order in ("C", "F"):
                a = do_import(gb, XA, fA, order=order)
                check_object(gb, a, A, "INT64", what)
                outs.append(check_export(gb, a, A, fA, order=order, out=True, bitmap=True, what=what))
                outs.append(check_export(gb, a.T, dm.transpose(A), fA, order=order, out=True, what=what))
            a = do_import(gb, A[1], None, A[0])
            check_object(gb, a, A, "INT64", what + " bitmap")
            w = do_import(gb, Xu, fu)
            check_object(gb, w, u, "FP64", what + " vector")
            outs.append(check_export(gb, w, u, fu, out=True, bitmap=True, what=what + " vector"))
            outs.append(check_export(gb, do_import(gb, A[1]), (np.ones_like(A[0]), A[1]), None, what=what + " full"))
            gb.set_knob("grid_cap", 0)
            if cap == 1:
                assert gb.get_knob(site) > before, f"{site} was not clamped at cap 1"
            if cap == 0:
                assert gb.get_knob(site) == before
            seen.append(outs)
    finally:
        gb.set_knob("grid_cap", 0)
    for outs in seen[1:]:
        assert all(np.array_equal(dio.bits(x), dio.bits(y)) for x, y in zip(outs, seen[0]))
