"""Sparse import and export from device arrays (csrc/gb_sparse_io.hip: k_sio_keys, k_sio_ptr,
k_sio_rows, k_sio_convert, k_sio_fill around the build's device core, behind
GxB_{Matrix,Vector}_{import,export}_sparse and from_coo / build / from_csr / from_csc / to_coo /
to_csr / to_csc) against the numpy model of tests/sparse_io_model.py and against the host-array
path given the same arrays, which is the code the library had before.  Objects are compared through
test_general_ops_gpu.check (structure, order, nvals, dtype, values) and their values bit for bit;
the two paths must also agree in iso-ness; exported arrays are compared bit for bit.

Shapes, and what each one is for
  COO of 0, 1, 63, 64, 65, 257, 5000 tuples   nothing, one lane, around one wave, two blocks' worth of
                       16-byte groups with a tail, many blocks
  on 7 x 7, 70 x 300, 0 x 5, 5 x 0            few keys (long runs of duplicates), many keys, no positions
  orders               strictly increasing (path 0), sorted with duplicates, reversed, shuffled, one
                       key n times (path 1)
  edge_index [2, E], E odd   the second slice starts 8 bytes past a 16-byte boundary
  rows 70 x 300        rows of 0, 1, 63, 64, 65, 128, 129 and 300 entries: the wave-per-row pass
  gappy 400 x 40       runs of empty rows: equal pointers
  1 x 1000, 1000 x 1   one long row, one entry per row (and the other way round as CSC)
  vectors 0, 1, 63, 64, 65, 127, 1000         no word, a partial word, one word, one bit more, many
  1300 x 700, 70001    the grid-sweep suite's shapes, under grid_cap 1, 3, 33 and 0

One documented difference between the paths: a Python scalar with device indices imports as iso
(one value is read); the host `from_csr` / `from_csc` broadcast it, and a host `from_coo` of one
tuple is iso where the device one holds its single value.  Iso-ness is compared everywhere else.
"""
import ctypes
import time

import numpy as np
import pytest

import dense_model as dm
import sparse_io_model as sm
from test_general_ops_gpu import check, coo_of, draw
from test_reindex_gpu import gappy_matrix, is_iso, rng_of, rows_matrix

pytestmark = pytest.mark.gpu

G = sm.golden()
INVALID_VALUE, INSUFFICIENT_SPACE, INDEX_OUT_OF_BOUNDS, DOMAIN_MISMATCH = -3, -103, -105, -5
COO_SIZES = [0, 1, 63, 64, 65, 257, 5000]
ORDERS = ["increasing", "sorted_dups", "reversed", "shuffled", "one_key"]
VECTORS = [0, 1, 63, 64, 65, 127, 1000]
FORMATS = {"coo": 2, "csr": 0, "csc": 1}


@pytest.fixture(scope="module")
def gb():
    import graphblas_amd

    yield graphblas_amd
    graphblas_amd.set_knob("grid_cap", 0)


@pytest.fixture(scope="module", autouse=True)
def report_run_time():
    t0 = time.perf_counter()
    yield
    print(f"\ntest_sparse_io_gpu.py: {time.perf_counter() - t0:.1f} s")


# ---------------------------------------------------------------------- arrays
def dev(x):
    """a numpy array as a torch CUDA tensor (None and scalars as they are)"""
    if x is None or np.ndim(x) == 0:
        return x
    import torch

    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def host(x):
    if x is None or isinstance(x, np.ndarray):
        return x
    import torch

    torch.cuda.synchronize()
    return x.cpu().numpy()


def path(gb):
    return gb.get_knob("stat_sparse_import_path")


def tuples(shape, n, order, key):
    """(rows, columns) of n tuples on `shape` in the given order (fewer when the order needs unique keys)"""
    rng = rng_of("tuples", shape, n, order, key)
    npos = shape[0] * shape[1]
    if order in ("increasing", "reversed"):
        flat = np.sort(rng.choice(npos, min(n, npos), replace=False))
        flat = flat[::-1] if order == "reversed" else flat
    elif order == "one_key":
        flat = np.full(n, rng.integers(0, npos))
    else:
        flat = rng.integers(0, npos, n)
        flat = np.sort(flat) if order == "sorted_dups" else flat
    flat = np.ascontiguousarray(flat, np.int64)
    return flat // shape[1], flat % shape[1]


def tame(vals):
    """FP32 values whose sums stay finite: inf - inf would make the payload of a NaN the subject"""
    return np.clip(np.where(np.isfinite(vals), vals, np.float32(1.5)), -1e6, 1e6).astype(np.float32)


def same_objects(gb, got, ref, what, iso=True):
    """the device import against the host import of the same arrays: structure, dtype, value bits, iso-ness"""
    assert got.dtype == ref.dtype and got.shape == ref.shape and got.nvals == ref.nvals, what
    gi, gv = coo_of(got)
    ri, rv = coo_of(ref)
    for a, b in zip(gi, ri):
        assert np.array_equal(a, b), f"{what}: indices differ from the host path"
    assert np.array_equal(sm.bits(gv), sm.bits(rv)), f"{what}: value bits differ from the host path"
    if iso:
        assert is_iso(got) == is_iso(ref), f"{what}: iso-ness differs from the host path"


def check_import(gb, got, want, dt, what):
    check(got, want, dt, what=what)
    assert np.array_equal(sm.bits(coo_of(got)[1]), sm.bits(want[1][want[0]])), f"{what}: value bits"


def still_works(gb):
    """after a refusal: a small import and export still give the right answer"""
    import torch

    i = torch.tensor([1, 0], dtype=torch.int64, device="cuda")
    A = gb.Matrix.from_coo(i, i, torch.tensor([5, 6], dtype=torch.int64, device="cuda"), nrows=2, ncols=2)
    r, c, v = (host(x) for x in A.to_coo(device=True))
    assert r.tolist() == [0, 1] and c.tolist() == [0, 1] and v.tolist() == [6, 5]


# ---------------------------------------------------------------------- COO import
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("n", COO_SIZES)
@pytest.mark.parametrize("shape", [(7, 7), (70, 300)], ids=str)
def test_coo_import_sizes_and_orders(gb, shape, n, order):
    r, c = tuples(shape, n, order, 0)
    vals = draw("INT64", rng_of("coo-values", shape, n, order), r.size)
    want = sm.from_coo(shape, (r, c), vals, "plus", "INT64")
    got = gb.Matrix.from_coo(dev(r), dev(c), dev(vals), nrows=shape[0], ncols=shape[1], dup_op=gb.binary.plus)
    assert path(gb) == sm.path_of_coo((r, c), shape), f"{order}: path"
    check_import(gb, got, want, "INT64", f"from_coo {shape} {n} {order}")
    ref = gb.Matrix.from_coo(r, c, vals, nrows=shape[0], ncols=shape[1], dup_op=gb.binary.plus)
    same_objects(gb, got, ref, f"from_coo {shape} {n} {order}")


@pytest.mark.parametrize("shape", [(0, 5), (5, 0), (7, 7)], ids=str)
def test_coo_import_of_nothing(gb, shape):
    import torch

    e = torch.empty(0, dtype=torch.int64, device="cuda")
    got = gb.Matrix.from_coo(e, e, torch.empty(0, dtype=torch.float64, device="cuda"), nrows=shape[0], ncols=shape[1])
    check_import(gb, got, (np.zeros(shape, bool), np.zeros(shape)), "FP64", f"empty {shape}")
    got = gb.Matrix.from_coo(e, e, 3, nrows=shape[0], ncols=shape[1])
    assert got.nvals == 0 and got.dtype == "INT64" and path(gb) == 0


@pytest.mark.parametrize("n", [257, 5000])
@pytest.mark.parametrize("dup", [None, "plus", "min", "first", "second"])
def test_coo_import_dup_operators(gb, dup, n):
    """FP32: the plus fold's result depends on its order, which is the input's"""
    shape = (70, 300) if n == 5000 else (7, 7)
    r, c = tuples(shape, n, "shuffled", dup)
    vals = tame(draw("FP32", rng_of("dup-values", dup, n), n))
    if dup == "min":  # IEEE 754 minNum may return either of +0 and -0: one zero only
        vals = np.where(vals == 0, np.float32(0), vals)
    op = None if dup is None else getattr(gb.binary, dup)
    kw = dict(nrows=shape[0], ncols=shape[1], dup_op=op)
    if dup is None:
        assert sm.has_duplicates((r, c), shape)
        for arrays in ((dev(r), dev(c), dev(vals)), (r, c, vals)):
            with pytest.raises(ValueError, match="Duplicate indices found"):
                gb.Matrix.from_coo(*arrays, **kw)
        return
    got = gb.Matrix.from_coo(dev(r), dev(c), dev(vals), **kw)
    assert path(gb) == 1
    check_import(gb, got, sm.from_coo(shape, (r, c), vals, dup, "FP32"), "FP32", f"dup {dup}")
    same_objects(gb, got, gb.Matrix.from_coo(r, c, vals, **kw), f"dup {dup}")


@pytest.mark.parametrize("dt", dm.ALL)
def test_coo_import_value_types(gb, dt):
    shape, n = (70, 300), 257
    r, c = tuples(shape, n, "shuffled", dt)
    vals = draw(dt, rng_of("type-values", dt), n)
    got = gb.Matrix.from_coo(dev(r), dev(c), dev(vals), nrows=70, ncols=300, dup_op=gb.binary.second)
    check_import(gb, got, sm.from_coo(shape, (r, c), vals, "second", dt), dt, f"values {dt}")
    same_objects(gb, got, gb.Matrix.from_coo(r, c, vals, nrows=70, ncols=300, dup_op=gb.binary.second), dt)
    r, c = tuples(shape, n, "increasing", dt)
    got = gb.Matrix.from_coo(dev(r), dev(c), dev(vals), nrows=70, ncols=300)
    assert path(gb) == 0
    check_import(gb, got, sm.from_coo(shape, (r, c), vals, None, dt), dt, f"values {dt}, direct")


@pytest.mark.parametrize("src,dst", [("FP64", "INT8"), ("INT64", "FP32"), ("INT32", "BOOL")])
@pytest.mark.parametrize("order", ["increasing", "shuffled"])
def test_coo_import_casts(gb, src, dst, order):
    shape, n = (70, 300), 257
    r, c = tuples(shape, n, order, (src, dst))
    vals = draw(src, rng_of("cast-values", src, dst), n)
    kw = dict(dtype=dst, nrows=70, ncols=300, dup_op=gb.binary.plus)
    got = gb.Matrix.from_coo(dev(r), dev(c), dev(vals), **kw)
    check_import(gb, got, sm.from_coo(shape, (r, c), vals, "plus", dst), dst, f"{src} -> {dst} {order}")
    if src == "FP64":
        # the host front end casts host values with numpy before the call, which neither saturates
        # nor maps NaN to 0 as the library's cast does: the two paths are compared on values that
        # INT8 holds (fractions included: both truncate), the model above on all of them
        vals = np.clip(np.where(np.isfinite(vals), vals, 3.75), -128, 127)
        got = gb.Matrix.from_coo(dev(r), dev(c), dev(vals), **kw)
    same_objects(gb, got, gb.Matrix.from_coo(r, c, vals, **kw), f"{src} -> {dst} {order}")


@pytest.mark.parametrize("n", [1, 64, 257])
@pytest.mark.parametrize("order", ["increasing", "shuffled"])
def test_coo_import_scalar_is_iso(gb, n, order):
    shape = (70, 300)
    r, c = tuples(shape, n, order, "scalar")
    got = gb.Matrix.from_coo(dev(r), dev(c), 7, nrows=70, ncols=300)
    check_import(gb, got, sm.from_coo(shape, (r, c), 7), "INT64", f"scalar {n} {order}")
    ref = gb.Matrix.from_coo(r, c, 7, nrows=70, ncols=300)
    same_objects(gb, got, ref, f"scalar {n} {order}", iso=n > 1)
    assert is_iso(got) == (n > 1)
    got = gb.Matrix.from_coo(dev(r), dev(c), 2.5, dtype="FP32", nrows=70, ncols=300)
    check_import(gb, got, sm.from_coo(shape, (r, c), np.float32(2.5)), "FP32", "scalar FP32")


@pytest.mark.parametrize("index", ["INT32", "INT64", "UINT64"])
@pytest.mark.parametrize("order", ["increasing", "shuffled"])
def test_coo_import_index_types(gb, index, order):
    from graphblas_amd.sparse import DeviceArray

    shape, n = (70, 300), 257
    r, c = tuples(shape, n, order, index)
    vals = draw("INT32", rng_of("index-values", index), n)
    if index == "UINT64":  # an int64 tensor re-described
        keep = [dev(r), dev(c)]
        I, J = (DeviceArray(t, np.uint64) for t in keep)
    else:
        I, J = dev(r.astype(sm.INDEX[index])), dev(c.astype(sm.INDEX[index]))
    got = gb.Matrix.from_coo(I, J, dev(vals), nrows=70, ncols=300, dup_op=gb.binary.plus)
    assert path(gb) == sm.path_of_coo((r, c), shape)
    check_import(gb, got, sm.from_coo(shape, (r, c), vals, "plus", "INT32"), "INT32", f"index {index} {order}")


@pytest.mark.parametrize("index", ["INT32", "INT64"])
@pytest.mark.parametrize("order", ["increasing", "shuffled"])
def test_coo_import_edge_index_slices(gb, index, order):
    """rows and columns as the two rows of one [2, E] tensor with odd E: edge_index[1] is not 16-byte aligned"""
    shape, E = (70, 300), 1001
    r, c = tuples(shape, E, order, "edge_index")
    ei = dev(np.stack([r, c]).astype(sm.INDEX[index]))
    assert ei[0].data_ptr() % 16 == 0 and ei[1].data_ptr() % 16 == (8 if index == "INT64" else 4)
    got = gb.Matrix.from_coo(ei[0], ei[1], 1.0, nrows=70, ncols=300)
    check_import(gb, got, sm.from_coo(shape, (r, c), 1.0), "FP64", f"edge_index {index}")
    got = gb.Matrix.from_coo(ei[1], ei[0], 1.0, nrows=300, ncols=70)  # the unaligned slice leads
    check_import(gb, got, sm.from_coo((300, 70), (c, r), 1.0), "FP64", f"edge_index {index}, swapped")


def test_matrix_build_from_device_arrays(gb):
    shape, n = (70, 300), 257
    r, c = tuples(shape, n, "shuffled", "build")
    vals = draw("INT32", rng_of("build-values"), n)
    A = gb.Matrix("INT32", 70, 300)
    A.build(dev(r), dev(c), dev(vals), dup_op=gb.binary.max)
    check_import(gb, A, sm.from_coo(shape, (r, c), vals, "max", "INT32"), "INT32", "build")
    with pytest.raises(gb.exceptions.OutputNotEmpty):
        A.build(dev(r), dev(c), dev(vals), dup_op=gb.binary.max)
    A.build(dev(r), dev(c), dev(vals), dup_op=gb.binary.min, clear=True, nrows=80)
    check_import(gb, A, sm.from_coo((80, 300), (r, c), vals, "min", "INT32"), "INT32", "build, clear and resize")
    v = gb.Vector("INT64", 70)
    v.build(dev(r), dev(np.arange(n)), dup_op=gb.binary.plus)
    check_import(gb, v, sm.from_coo((70,), (r,), np.arange(n), "plus", "INT64"), "INT64", "Vector.build")


# ---------------------------------------------------------------------- CSR and CSC import
def compressed_matrices():
    rng = rng_of("compressed")
    p1, p2 = rng.random((1, 1000)) < 0.3, rng.random((1000, 1)) < 0.3
    return {"rows": rows_matrix("INT64"), "gappy": gappy_matrix("INT32"),
            "1x1000": (p1, np.where(p1, draw("FP64", rng, 1000).reshape(p1.shape), 0.0)),
            "1000x1": (p2, np.where(p2, draw("FP64", rng, 1000).reshape(p2.shape), 0.0))}


COMPRESSED = compressed_matrices()


def variant(indptr, indices, values, how, key):
    """the arrays with one row jumbled (two neighbours swapped) or one column duplicated in its row;
    None when no row has two entries"""
    if how == "sorted":
        return indptr, indices, values
    rows = np.flatnonzero(np.diff(indptr) >= 2)
    if rows.size == 0:
        return None
    i = rows[rng_of("variant", how, key).integers(0, rows.size)]
    a = int(indptr[i])
    indices, values = indices.copy(), values.copy()
    if how == "jumbled":
        indices[[a, a + 1]] = indices[[a + 1, a]]
        values[[a, a + 1]] = values[[a + 1, a]]
    else:
        indices[a + 1] = indices[a]
    return indptr, indices, values


def compressed_arrays(name, by_col, index, how):
    return variant(*(sm.to_csc if by_col else sm.to_csr)(COMPRESSED[name], index), how, (name, by_col))


# every variant a shape has: a shape without a row of two entries (1000 x 1 as CSR, 1 x 1000 as CSC)
# has no jumbled or duplicated one
COMPRESSED_CASES = [(name, by_col, index, how) for name in COMPRESSED for by_col in (False, True)
                    for index in ("INT32", "INT64") for how in ("sorted", "jumbled", "duplicated")
                    if compressed_arrays(name, by_col, index, how) is not None]


@pytest.mark.parametrize("name,by_col,index,how", COMPRESSED_CASES,
                         ids=[f"{n}-{'csc' if b else 'csr'}-{i}-{h}" for n, b, i, h in COMPRESSED_CASES])
def test_compressed_import(gb, name, by_col, index, how):
    A = COMPRESSED[name]
    dt = dm.name_of(A[1].dtype)
    arrays = compressed_arrays(name, by_col, index, how)
    ptr, idx, vals = arrays
    shape = A[0].shape
    want = sm.from_csx(shape, ptr, idx, vals, dt, by_col)
    if by_col:
        got = gb.Matrix.from_csc(dev(ptr), dev(idx), dev(vals), nrows=shape[0])
        ref = gb.Matrix.from_csc(ptr, idx, vals, nrows=shape[0])
    else:
        got = gb.Matrix.from_csr(dev(ptr), dev(idx), dev(vals), ncols=shape[1])
        ref = gb.Matrix.from_csr(ptr, idx, vals, ncols=shape[1])
    assert path(gb) == (0 if how == "sorted" else 2) == sm.path_of_csx(ptr, idx)
    check_import(gb, got, want, dt, f"{name} {how}")
    if by_col and how == "duplicated":
        # the typed host import installs the CSC result with Ap[last] entries although the fold
        # dropped one: its nvals is one too many.  The host entry points are not this suite's
        # subject and stay as they are; the device path is held to the model above, and the host
        # path to what it is known to give, so that a later fix of it is noticed here.
        assert ref.nvals == int(ptr[-1]) == got.nvals + 1
        return
    same_objects(gb, got, ref, f"{name} {how}")


def test_compressed_import_scalar_cast_and_short_pointer(gb):
    A = COMPRESSED["rows"]
    ptr, idx, vals = sm.to_csr(A)
    got = gb.Matrix.from_csr(dev(ptr), dev(idx), 7, ncols=300)
    check_import(gb, got, sm.from_csx((70, 300), ptr, idx, 7), "INT64", "from_csr scalar")
    assert is_iso(got)
    got = gb.Matrix.from_csc(*(dev(x) for x in sm.to_csc(A)[:2]), 2.5, nrows=70)
    check_import(gb, got, (A[0], np.where(A[0], 2.5, 0.0)), "FP64", "from_csc scalar")
    got = gb.Matrix.from_csr(dev(ptr), dev(idx), dev(vals), dtype="FP32", ncols=300)
    check_import(gb, got, sm.from_csx((70, 300), ptr, idx, vals, "FP32"), "FP32", "from_csr cast")
    # Ap[last] below len(Ai), values of the short length: accepted, the tail is not read
    long_idx = np.concatenate([idx, np.full(9, 299, idx.dtype)])
    got = gb.Matrix.from_csr(dev(ptr), dev(long_idx), dev(vals), ncols=300)
    check_import(gb, got, A, "INT64", "from_csr, indices longer than the pointer says")
    with pytest.raises(ValueError, match="nrows must"):
        gb.Matrix.from_csr(dev(ptr), dev(idx), dev(vals), nrows=8, ncols=300)


def test_host_csc_round_trips(gb):
    """from_csc / to_csc on host arrays: GrB_Matrix_import / export with GrB_CSC_FORMAT"""
    for A in COMPRESSED.values():
        dt = dm.name_of(A[1].dtype)
        ptr, idx, vals = sm.to_csc(A)
        B = gb.Matrix.from_csc(ptr, idx, vals, nrows=A[0].shape[0])
        check_import(gb, B, A, dt, "host from_csc")
        for got, want in zip(B.to_csc(), (ptr, idx, vals)):
            assert got.dtype == want.dtype and np.array_equal(sm.bits(got), sm.bits(want))
        for got, want in zip(B.T.to_csr(), (ptr, idx, vals)):
            assert np.array_equal(sm.bits(got), sm.bits(want))
        for got, want in zip(B.T.to_csc(), sm.to_csr(A)):
            assert np.array_equal(sm.bits(got), sm.bits(want))


# ---------------------------------------------------------------------- the reference's own cases
def golden_arguments(G, desc, place):
    args = []
    for a in desc["args"]:
        if isinstance(a, dict) and "star" in a:
            args += [place(x) for x in sm._export(G, a["star"])]
        elif np.ndim(a) == 0:
            args.append(a)
        else:
            args.append(place(np.asarray(a, np.int64 if len(args) < len(desc["args"]) - 1 else None)))
    kw = {k: (v["dtype"] if isinstance(v, dict) and "dtype" in v else v) for k, v in desc["kwargs"].items()}
    return args, kw


GOLDEN_OBJECTS = {}
for _c in G["cases"]:
    for _d in ([_c["of"]] if "of" in _c else [_c["left"], _c["right"]] if "left" in _c else []):
        if _d.get("how") in ("from_coo", "from_csr", "from_csc"):
            GOLDEN_OBJECTS[_d["src"]] = _d


@pytest.mark.parametrize("src", sorted(GOLDEN_OBJECTS))
def test_golden_objects_from_device_arrays(gb, src):
    """every object the reference's tests construct, from device arrays (the dimensions the
    reference infers are given: they are the model's)"""
    desc = GOLDEN_OBJECTS[src]
    want = sm.golden_object(G, desc)
    dt = dm.name_of(want[1].dtype)
    args, kw = golden_arguments(G, desc, dev)
    if "dup_op" in kw:
        kw["dup_op"] = getattr(getattr(gb, kw["dup_op"]["op"].split(".")[0]), kw["dup_op"]["op"].split(".")[1])
    if desc["kind"] == "Vector":
        kw["size"] = want[0].shape[0]
    else:
        kw["nrows"], kw["ncols"] = want[0].shape
    if desc["how"] == "from_csr":
        kw.pop("nrows")
    if desc["how"] == "from_csc":
        kw.pop("ncols")
    assert any(hasattr(a, "__cuda_array_interface__") for a in args), "every constructor has an index array"
    got = getattr(getattr(gb, desc["kind"]), desc["how"])(*args, **kw)
    check_import(gb, got, want, dt, src)


def test_golden_refusals_from_device_arrays(gb):
    import torch

    t = lambda x, dt=torch.int64: torch.tensor(x, dtype=dt, device="cuda")  # noqa: E731
    with pytest.raises(ValueError, match="Duplicate indices found"):
        gb.Matrix.from_coo(t([0, 1, 1]), t([2, 1, 1]), t([True, True, True], torch.bool), nrows=2, ncols=3)
    with pytest.raises(gb.exceptions.IndexOutOfBound):
        gb.Matrix.from_coo(t([0, 1, 3]), t([1, 1, 2]), t([12.3, 12.4, 12.5], torch.float64), nrows=17, ncols=2)
    with pytest.raises(gb.exceptions.InvalidValue):  # a pointer of four entries for two rows' worth of indices
        gb.Matrix.from_csr(t([0, 1, 2, 3]), t([1, 0, 0]), t([10, 20]), ncols=3)
    with pytest.raises(ValueError, match="Duplicate indices found"):
        gb.Vector.from_coo(t([0, 1, 1]), t([True, True, True], torch.bool), size=2)
    still_works(gb)


# ---------------------------------------------------------------------- vectors
@pytest.mark.parametrize("dups", [False, True], ids=["unique", "dups"])
@pytest.mark.parametrize("n", VECTORS)
def test_vector_import(gb, n, dups):
    rng = rng_of("vector", n, dups)
    for dt, index in (("INT64", "INT64"), ("FP32", "INT32"), ("BOOL", "INT64")):
        m = n // 2 if not dups else 2 * n
        idx = rng.integers(0, n, m) if (dups and n) else rng.permutation(n)[:m]
        idx = idx.astype(sm.INDEX[index])
        vals = draw(dt, rng, idx.size)
        if dt == "FP32":
            vals = tame(vals)
        kw = dict(size=n, dup_op=gb.binary.plus)
        got = gb.Vector.from_coo(dev(idx), dev(vals), **kw)
        assert path(gb) == sm.path_of_coo((idx,), (n,))
        check_import(gb, got, sm.from_coo((n,), (idx,), vals, "plus", dt), dt, f"vector {n} {dt}")
        same_objects(gb, got, gb.Vector.from_coo(idx, vals, **kw), f"vector {n} {dt}")
        srt = np.sort(rng.permutation(n)[:n // 2 + n % 2]).astype(sm.INDEX[index])
        svals = draw(dt, rng, srt.size)
        got = gb.Vector.from_coo(dev(srt), dev(svals), size=n)
        assert path(gb) == 0
        check_import(gb, got, sm.from_coo((n,), (srt,), svals, None, dt), dt, f"vector {n} {dt} sorted")
        got = gb.Vector.from_coo(dev(srt), 3, size=n)
        check_import(gb, got, sm.from_coo((n,), (srt,), 3), "INT64", f"vector {n} scalar")
        assert is_iso(got) == (srt.size > 1)


@pytest.mark.parametrize("n", VECTORS)
def test_vector_export(gb, n):
    rng = rng_of("vector-export", n)
    p = rng.random(n) < 0.4
    for dt in ("INT64", "FP32", "INT8"):
        A = (p, np.where(p, draw(dt, rng, n), dm.NP[dt](0)))
        v = gb.Vector.from_coo(np.flatnonzero(p), A[1][p], dtype=dt, size=n)
        for index, cast in (("INT64", None), ("INT32", None), ("INT64", "FP64"), ("INT32", "INT16")):
            want = sm.to_coo(A, index, cast)
            got = v.to_coo(cast, device=True, index_dtype=sm.INDEX[index])
            for g, w in zip(got, want):
                g = host(g)
                assert g.dtype == w.dtype and np.array_equal(sm.bits(g), sm.bits(w)), f"vector export {n} {dt}"
        i, x = v.to_coo(device=True, values=False)
        assert x is None and np.array_equal(host(i), np.flatnonzero(p))
        i, x = v.to_coo(device=True, indices=False)
        assert i is None and np.array_equal(sm.bits(host(x)), sm.bits(A[1][p]))
    iso = gb.Vector.from_coo(np.flatnonzero(p), 9, size=n)
    i, x = iso.to_coo("FP32", device=True, index_dtype="int32")
    assert np.array_equal(host(i), np.flatnonzero(p).astype(np.int32))
    assert host(x).dtype == np.float32 and np.array_equal(host(x), np.full(int(p.sum()), 9, np.float32))


# ---------------------------------------------------------------------- export
def guarded(n, np_type):
    """a device tensor of n + 1 elements, every byte 0x5a (BOOL: true): a stray write shows"""
    size = np.dtype(np_type).itemsize
    x = np.ones(n + 1, np.bool_) if np_type == np.bool_ else np.full((n + 1, size), 0x5a, np.uint8).view(np_type).ravel()
    return dev(x), x[0]


def raw_export(gb, A, fmt, index, dt, want=(True, True, True)):
    """GxB_Matrix_export_sparse into guarded tensors; the arrays cut to the lengths returned"""
    it = sm.INDEX[index]
    nz = A.nvals
    np_len = {"coo": nz, "csr": A.nrows + 1, "csc": A.ncols + 1}[fmt]
    bufs = [guarded(np_len, it), guarded(nz, it), guarded(nz, dm.NP[dt])]
    lens = [ctypes.c_uint64(np_len + 1), ctypes.c_uint64(nz + 1), ctypes.c_uint64(nz + 1)]
    ptrs = [ctypes.c_void_p(b[0].data_ptr()) if w else None for b, w in zip(bufs, want)]
    rc = gb.lib.GxB_Matrix_export_sparse(*ptrs, getattr(gb.lib, f"GrB_{index}"), getattr(gb.lib, f"GrB_{dt}"),
                                         *[ctypes.byref(x) for x in lens], FORMATS[fmt], A._h, True)
    assert rc == 0, rc
    A.wait()
    assert [x.value for x in lens] == [np_len, nz, nz if want[2] else 0]
    out = []
    for (t, fill), w, n in zip(bufs, want, (np_len, nz, nz)):
        h = host(t)
        assert np.array_equal(sm.bits(h[n if w else 0:]), sm.bits(np.full(1 if w else n + 1, fill))), "a stray write"
        out.append(h[:n] if w else None)
    return out


def export_subjects(gb):
    """(name, Matrix, model): plain matrices, an iso matrix, a select result, a column-word matrix"""
    from graphblas_amd import device as gdev

    out = []
    for name, A in COMPRESSED.items():
        out.append((name, to_matrix(gb, A), A))
    f = G["fixture_A"]
    A = sm.from_coo((7, 7), (f["rows"], f["columns"]), np.asarray(f["values"]))
    out.append(("fixture", to_matrix(gb, A), A))
    p = COMPRESSED["gappy"][0]
    iso = gb.Matrix.from_coo(*np.nonzero(p), 7, nrows=400, ncols=40)
    assert is_iso(iso)
    out.append(("iso", iso, (p, np.where(p, 7, 0))))
    R = COMPRESSED["rows"]
    sel = to_matrix(gb, R).select(gb.select.triu).new()
    keep = np.triu(np.ones(R[0].shape, bool))
    out.append(("select", sel, (R[0] & keep, np.where(R[0] & keep, R[1], 0))))
    rng = rng_of("colwords")
    p = rng.random((5, 900)) < 0.2
    Q = gb.Matrix.from_coo(*np.nonzero(p), True, nrows=5, ncols=900)
    gdev.colwords_view(Q._h)  # from here on Q is held as column words
    out.append(("colwords", Q, (p, p.copy())))
    empty = gb.Matrix("FP32", 0, 5)
    out.append(("0x5", empty, (np.zeros((0, 5), bool), np.zeros((0, 5), np.float32))))
    return out


def to_matrix(gb, A):
    p, v = A
    r, c = np.nonzero(p)
    return gb.Matrix.from_coo(r, c, v[p], dtype=dm.name_of(v.dtype), nrows=p.shape[0], ncols=p.shape[1])


@pytest.fixture(scope="module")
def subjects(gb):
    return export_subjects(gb)


@pytest.mark.parametrize("fmt", ["coo", "csr", "csc"])
@pytest.mark.parametrize("index", ["INT32", "INT64"])
def test_matrix_export(gb, subjects, fmt, index):
    model = {"coo": sm.to_coo, "csr": sm.to_csr, "csc": sm.to_csc}[fmt]
    for name, M, A in subjects:
        own = dm.name_of(A[1].dtype)
        for dt in (own, "FP32" if own != "FP32" else "INT16"):
            want = model(A, index, None if dt == own else dt)
            if name == "colwords":
                from graphblas_amd import device as gdev

                gdev.colwords_view(M._h)  # an export converts it back: put it into column words again
            got = raw_export(gb, M, fmt, index, dt)
            for g, w in zip(got, want):
                assert g.dtype == w.dtype and np.array_equal(sm.bits(g), sm.bits(w)), f"{name} {fmt} {index} {dt}"
        got = raw_export(gb, M, fmt, index, own, (True, True, False))  # the structure only
        assert got[2] is None and all(np.array_equal(g, w) for g, w in zip(got[:2], want[:2]))
        got = raw_export(gb, M, fmt, index, own, (False, False, True))
        assert got[0] is None and got[1] is None and np.array_equal(sm.bits(got[2]), sm.bits(model(A, index)[2]))


def test_front_end_exports(gb, subjects):
    for name, M, A in subjects:
        for method, model in (("to_coo", sm.to_coo), ("to_csr", sm.to_csr), ("to_csc", sm.to_csc)):
            for kw, index, cast in (({}, "INT64", None), ({"index_dtype": "int32"}, "INT32", None),
                                    ({"dtype": "FP64"}, "INT64", "FP64")):
                got = getattr(M, method)(device=True, **kw)
                for g, w in zip(got, model(A, index, cast)):
                    g = host(g)
                    assert g.dtype == w.dtype and np.array_equal(sm.bits(g), sm.bits(w)), f"{name} {method} {kw}"
        r, c, x = M.to_coo(device=True, rows=False)
        assert r is None and np.array_equal(host(c), sm.to_coo(A)[1])
        r, c, x = M.to_coo(device=True, columns=False, values=False)
        assert c is None and x is None and np.array_equal(host(r), sm.to_coo(A)[0])
        for got, want in zip(M.T.to_coo(device=True), sm.to_coo(dm.transpose(A))):
            assert np.array_equal(sm.bits(host(got)), sm.bits(want)), f"{name} T.to_coo"
        for a, b in zip(M.T.to_csr(device=True), M.to_csc(device=True)):
            assert np.array_equal(sm.bits(host(a)), sm.bits(host(b))), f"{name} T.to_csr"
        for a, b in zip(M.T.to_csr(), M.to_csc()):
            assert np.array_equal(sm.bits(a), sm.bits(b))


def test_round_trips(gb, subjects):
    for name, M, A in subjects:
        dt = dm.name_of(A[1].dtype)
        nr, nc = A[0].shape
        for B in (gb.Matrix.from_csr(*M.to_csr(device=True), ncols=nc), gb.Matrix.from_csc(*M.to_csc(device=True), nrows=nr),
                  gb.Matrix.from_coo(*M.to_coo(device=True), nrows=nr, ncols=nc),
                  gb.Matrix.from_csc(*M.T.to_csr(device=True), nrows=nr),
                  gb.Matrix.from_csr(*M.to_csr(device=True, index_dtype="int32"), ncols=nc)):
            assert path(gb) == 0, name
            check_import(gb, B, A, dt, f"round trip of {name}")
    for src in ("graphblas/tests/test_matrix.py:3955", "graphblas/tests/test_matrix.py:3959"):
        case = next(c for c in G["cases"] if c["src"] == src)
        assert sm.same_object(sm.golden_object(G, case["left"]), sm.golden_object(G, case["right"]), True)


# ---------------------------------------------------------------------- grid sweeps
@pytest.mark.parametrize("cap", [1, 3, 33, 0])
def test_grid_sweeps(gb, cap):
    """the sweep suite's shapes: every new kernel runs its later grid sweeps at cap 1, 3 and 33"""
    shape, nvec = (1300, 700), 70001
    rng = rng_of("sweeps")
    p = rng.random(shape) < 0.05
    A = (p, np.where(p, draw("INT64", rng, p.size).reshape(shape), 0))
    r, c = np.nonzero(p)
    o = rng.permutation(r.size)
    extra = rng.integers(0, r.size, 5000)
    sr, sc = np.concatenate([r[o], r[extra]]), np.concatenate([c[o], c[extra]])
    svals = draw("INT64", rng, sr.size)
    pv = rng.random(nvec) < 0.3
    V = (pv, np.where(pv, draw("FP64", rng, nvec), 0.0))
    try:
        gb.set_knob("grid_cap", cap)
        got = gb.Matrix.from_coo(dev(r), dev(c), dev(A[1][p]), nrows=shape[0], ncols=shape[1])
        assert path(gb) == 0
        check_import(gb, got, A, "INT64", f"cap {cap}: sorted COO")
        got = gb.Matrix.from_coo(dev(sr), dev(sc), dev(svals), nrows=shape[0], ncols=shape[1], dup_op=gb.binary.plus)
        assert path(gb) == 1
        check_import(gb, got, sm.from_coo(shape, (sr, sc), svals, "plus", "INT64"), "INT64", f"cap {cap}: shuffled COO")
        got = gb.Matrix.from_coo(dev(r.astype(np.int32)), dev(c.astype(np.int32)), 4, nrows=shape[0], ncols=shape[1])
        check_import(gb, got, (p, np.where(p, 4, 0)), "INT64", f"cap {cap}: iso COO")
        M = got
        for by_col, to in ((False, sm.to_csr), (True, sm.to_csc)):
            for how in ("sorted", "jumbled"):
                ptr, idx, vals = variant(*to(A, "INT32"), how, cap)
                kw = {"nrows": shape[0]} if by_col else {"ncols": shape[1]}
                got = (gb.Matrix.from_csc if by_col else gb.Matrix.from_csr)(dev(ptr), dev(idx), dev(vals), **kw)
                assert path(gb) == (0 if how == "sorted" else 2)
                check_import(gb, got, A, "INT64", f"cap {cap}: {'csc' if by_col else 'csr'} {how}")
        for fmt, model in (("coo", sm.to_coo), ("csr", sm.to_csr), ("csc", sm.to_csc)):
            for index, dt in (("INT32", "INT64"), ("INT64", "FP32")):
                for g, w in zip(raw_export(gb, got, fmt, index, dt), model(A, index, None if dt == "INT64" else dt)):
                    assert np.array_equal(sm.bits(g), sm.bits(w)), f"cap {cap}: export {fmt} {index}"
            for g, w in zip(raw_export(gb, M, fmt, "INT64", "INT16"), model((p, np.where(p, 4, 0)), "INT64", "INT16")):
                assert np.array_equal(sm.bits(g), sm.bits(w)), f"cap {cap}: iso export {fmt}"
        iv = np.flatnonzero(pv)
        ov = rng.permutation(iv.size)
        v = gb.Vector.from_coo(dev(iv), dev(V[1][pv]), size=nvec)
        assert path(gb) == 0
        check_import(gb, v, V, "FP64", f"cap {cap}: sorted vector")
        v = gb.Vector.from_coo(dev(iv[ov].astype(np.int32)), dev(V[1][pv][ov]), size=nvec)
        assert path(gb) == 1
        check_import(gb, v, V, "FP64", f"cap {cap}: shuffled vector")
        for index, cast in (("INT64", None), ("INT32", "FP32")):
            for g, w in zip(v.to_coo(cast, device=True, index_dtype=sm.INDEX[index]), sm.to_coo(V, index, cast)):
                assert np.array_equal(sm.bits(host(g)), sm.bits(w)), f"cap {cap}: vector export"
    finally:
        gb.set_knob("grid_cap", 0)
    assert gb.get_knob("grid_cap") == 0


# ---------------------------------------------------------------------- refusals
def test_front_end_refusals(gb):
    """every value read stays inside the tensors of the call, even were a check missing"""
    import torch

    t = lambda x, dt=torch.int64: torch.tensor(x, dtype=dt, device="cuda")  # noqa: E731
    x4 = t([1.0, 2.0, 3.0, 4.0], torch.float64)
    E = gb.exceptions
    for dt in (torch.int64, torch.int32):
        with pytest.raises(E.IndexOutOfBound):  # an index equal to the dimension
            gb.Matrix.from_coo(t([0, 1, 2, 3], dt), t([0, 1, 5, 3], dt), x4, nrows=4, ncols=5)
        with pytest.raises(E.IndexOutOfBound):
            gb.Matrix.from_coo(t([0, 4, 2, 3], dt), t([0, 1, 2, 3], dt), x4, nrows=4, ncols=5)
        with pytest.raises(E.IndexOutOfBound):  # -1 does not wrap
            gb.Matrix.from_coo(t([0, 1, -1, 3], dt), t([0, 1, 2, 3], dt), x4, nrows=4, ncols=5)
        with pytest.raises(E.IndexOutOfBound):
            gb.Vector.from_coo(t([0, 9, 2, 3], dt), x4, size=9)
        with pytest.raises(E.IndexOutOfBound):
            gb.Vector.from_coo(t([0, -1, 2, 3], dt), x4, size=9)
        with pytest.raises(E.IndexOutOfBound):
            gb.Matrix.from_csr(t([0, 2, 4], dt), t([0, 1, 2, 5], dt), x4, ncols=5)
        with pytest.raises(E.IndexOutOfBound):
            gb.Matrix.from_csc(t([0, 2, 4], dt), t([0, 1, -1, 3], dt), x4, nrows=5)
        with pytest.raises(E.InvalidValue):  # the pointer does not start at 0
            gb.Matrix.from_csr(t([1, 2, 4], dt), t([0, 1, 2, 3], dt), x4, ncols=5)
        with pytest.raises(E.InvalidValue):  # it decreases
            gb.Matrix.from_csr(t([0, 3, 2, 4], dt), t([0, 1, 2, 3], dt), x4, ncols=5)
        with pytest.raises(E.InvalidValue):
            gb.Matrix.from_csc(t([0, 3, 2, 4], dt), t([0, 1, 2, 3], dt), x4, nrows=5)
        with pytest.raises(E.InvalidValue):  # fewer values than the pointer says, and more than one
            gb.Matrix.from_csr(t([0, 2, 4], dt), t([0, 1, 2, 3], dt), x4[:3], ncols=5)
        still_works(gb)
    # Ap[last] below len(Ai) with values of the short length is no refusal
    A = gb.Matrix.from_csr(t([0, 1, 2]), t([0, 1, 4, 4]), x4[:2], ncols=5)
    check_import(gb, A, sm.from_csx((2, 5), [0, 1, 2], [0, 1, 4, 4], np.array([1.0, 2.0])), "FP64", "short pointer")


def test_entry_point_refusals(gb):
    import torch

    lib = gb.lib
    ptr = torch.tensor([0, 2, 6], dtype=torch.int64, device="cuda")
    idx = torch.zeros(8, dtype=torch.int64, device="cuda")  # 8 long: Ap[last] = 6 stays inside it
    val = torch.ones(8, dtype=torch.float64, device="cuda")
    h = ctypes.c_void_p()
    P = lambda x: ctypes.c_void_p(x.data_ptr())  # noqa: E731
    args = lambda ai_len, it=lib.GrB_INT64: (ctypes.byref(h), lib.GrB_FP64, 2, 5, P(ptr), P(idx), P(val), it,  # noqa: E731
                                            lib.GrB_FP64, 3, ai_len, 8, FORMATS["csr"], None, True)
    assert lib.GxB_Matrix_import_sparse(*args(4)) == INVALID_VALUE and h.value is None  # Ap[last] = 6 > Ai_len = 4
    assert lib.GxB_Matrix_import_sparse(*args(8, lib.GrB_FP64)) == DOMAIN_MISMATCH and h.value is None
    assert lib.GxB_Matrix_import_sparse(*args(8, lib.GrB_UINT32)) == DOMAIN_MISMATCH and h.value is None
    assert lib.GxB_Matrix_import_sparse(*args(8)) == 0 and h.value  # rows {0, 0} and {0, 0, 0, 0}: jumbled, kept last
    assert gb.get_knob("stat_sparse_import_path") == 2
    n = ctypes.c_uint64()
    assert lib.GrB_Matrix_nvals(ctypes.byref(n), h) == 0 and n.value == 2
    # a too-small export capacity: nothing is written
    for fmt, short in (("csr", 0), ("csr", 1), ("coo", 0), ("csc", 2)):
        bufs = [guarded(8, np.int64), guarded(8, np.int64), guarded(8, np.float64)]
        caps = [8, 8, 8]
        caps[short] = 1
        lens = [ctypes.c_uint64(c) for c in caps]
        rc = lib.GxB_Matrix_export_sparse(*[P(b[0]) for b in bufs], lib.GrB_INT64, lib.GrB_FP64,
                                          *[ctypes.byref(x) for x in lens], FORMATS[fmt], h, True)
        assert rc == INSUFFICIENT_SPACE, (fmt, short)
        for t, fill in bufs:
            assert (sm.bits(host(t)) == sm.bits(np.full(1, fill))[0]).all(), "written despite the refusal"
    lens = [ctypes.c_uint64(0), ctypes.c_uint64(0)]
    v = gb.Vector.from_coo(idx[:1], val[:1], size=3)
    out = guarded(4, np.int64)
    rc = lib.GxB_Vector_export_sparse(P(out[0]), None, lib.GrB_INT64, lib.GrB_FP64, *[ctypes.byref(x) for x in lens],
                                      v._h, True)
    assert rc == INSUFFICIENT_SPACE and (host(out[0]) == out[1]).all()
    assert lib.GrB_Matrix_free(ctypes.byref(h)) == 0
    still_works(gb)


# ---------------------------------------------------------------------- host pointers, unaligned outputs
def host_import(gb, kind, fmt, dims, arrays, index, vdt, dt, dup=None):
    """GxB_{Matrix,Vector}_import_sparse with on_device false: numpy arrays, staged by one copy each"""
    lib, h = gb.lib, ctypes.c_void_p()
    P = lambda a: ctypes.c_void_p(a.ctypes.data) if a.size else None  # noqa: E731
    T = lambda name: getattr(lib, f"GrB_{name}")  # noqa: E731
    dup = None if dup is None else getattr(lib, f"GrB_{dup.upper()}_{dt}")
    if kind == "Vector":
        i, x = arrays
        rc = lib.GxB_Vector_import_sparse(ctypes.byref(h), T(dt), dims[0], P(i), P(x), T(index), T(vdt), i.size, x.size,
                                          dup, False)
        obj = gb.Vector.__new__(gb.Vector)
        obj._size = dims[0]
    else:
        p, i, x = arrays
        rc = lib.GxB_Matrix_import_sparse(ctypes.byref(h), T(dt), dims[0], dims[1], P(p), P(i), P(x), T(index), T(vdt),
                                          p.size, i.size, x.size, FORMATS[fmt], dup, False)
        obj = gb.Matrix.__new__(gb.Matrix)
        obj._nrows, obj._ncols = dims
    if rc != 0:
        assert h.value is None
        return rc
    obj._h, obj.dtype, obj.name = h, gb.dtypes.lookup_dtype(dt), "host_import"
    return obj


def test_host_pointer_imports(gb):
    """the on_device == false half of the imports: every format, both paths, a cast, an iso value"""
    shape, n = (70, 300), 257
    for order in ("increasing", "shuffled"):
        for index in ("INT32", "INT64", "UINT64"):
            r, c = (x.astype(sm.INDEX[index]) for x in tuples(shape, n, order, ("host", index)))
            vals = draw("INT32", rng_of("host-values", order, index), n)
            got = host_import(gb, "Matrix", "coo", shape, (r, c, vals), index, "INT32", "INT64", "plus")
            assert path(gb) == sm.path_of_coo((r, c), shape)
            check_import(gb, got, sm.from_coo(shape, (r, c), vals, "plus", "INT64"), "INT64", f"host COO {order} {index}")
            one = np.array([2.5], np.float32)
            got = host_import(gb, "Matrix", "coo", shape, (r, c, one), index, "FP32", "FP32")
            check_import(gb, got, sm.from_coo(shape, (r, c), np.float32(2.5)), "FP32", f"host COO iso {order} {index}")
            assert is_iso(got)
            got = host_import(gb, "Vector", None, (70,), (r, vals), index, "INT32", "INT32", "plus")
            check_import(gb, got, sm.from_coo((70,), (r,), vals, "plus", "INT32"), "INT32", f"host vector {order} {index}")
    A = COMPRESSED["rows"]
    for by_col, fmt, to in ((False, "csr", sm.to_csr), (True, "csc", sm.to_csc)):
        for how in ("sorted", "jumbled", "duplicated"):
            ptr, idx, vals = variant(*to(A, "INT32"), how, ("host", by_col))
            got = host_import(gb, "Matrix", fmt, (70, 300), (ptr, idx, vals), "INT32", "INT64", "FP64")
            assert path(gb) == (0 if how == "sorted" else 2)
            check_import(gb, got, sm.from_csx((70, 300), ptr, idx, vals, "FP64", by_col), "FP64", f"host {fmt} {how}")
    bad = np.array([0, 70], np.int64)
    assert host_import(gb, "Matrix", "coo", shape, (bad, bad, np.ones(2)), "INT64", "FP64", "FP64") == INDEX_OUT_OF_BOUNDS
    ptr = np.array([0, 3, 2, 4], np.int64)
    assert host_import(gb, "Matrix", "csr", (3, 5), (ptr, np.arange(4), np.ones(4)), "INT64", "FP64", "FP64") == INVALID_VALUE
    still_works(gb)


def test_host_pointer_exports(gb, subjects):
    """the on_device == false half of the exports, into guarded numpy arrays"""
    lib = gb.lib
    for name, M, A in subjects:
        own = dm.name_of(A[1].dtype)
        for fmt, model in (("coo", sm.to_coo), ("csr", sm.to_csr), ("csc", sm.to_csc)):
            for index, dt in (("INT64", own), ("INT32", "FP32" if own != "FP32" else "INT16")):
                want = model(A, index, None if dt == own else dt)
                bufs = [np.full(w.size + 1, 0x5a, np.uint8).repeat(w.dtype.itemsize).view(w.dtype)
                        if w.dtype != np.bool_ else np.ones(w.size + 1, np.bool_) for w in want]
                lens = [ctypes.c_uint64(b.size) for b in bufs]
                rc = lib.GxB_Matrix_export_sparse(*[ctypes.c_void_p(b.ctypes.data) for b in bufs],
                                                  getattr(lib, f"GrB_{index}"), getattr(lib, f"GrB_{dt}"),
                                                  *[ctypes.byref(x) for x in lens], FORMATS[fmt], M._h, False)
                assert rc == 0 and [x.value for x in lens] == [w.size for w in want], f"{name} {fmt} {index}"
                for b, w in zip(bufs, want):
                    assert np.array_equal(sm.bits(b[:-1]), sm.bits(w)), f"host export {name} {fmt} {index} {dt}"
                    assert sm.bits(b[-1:])[0] == (1 if w.dtype == np.bool_ else sm.bits(np.full(1, 0x5a, np.uint8).repeat(
                        w.dtype.itemsize).view(w.dtype))[0]), "a stray write"
    for n in (0, 65, 1000):
        p = rng_of("host-vector-export", n).random(n) < 0.4
        for v, vals in ((gb.Vector.from_coo(np.flatnonzero(p), np.flatnonzero(p) * 3, size=n), np.flatnonzero(p) * 3),
                        (gb.Vector.from_coo(np.flatnonzero(p), 9, size=n), np.full(int(p.sum()), 9))):
            for index, dt in (("INT64", "INT64"), ("INT32", "FP32")):
                i = np.full(int(p.sum()) + 1, -7, sm.INDEX[index])
                x = np.full(int(p.sum()) + 1, -7, dm.NP[dt])
                lens = [ctypes.c_uint64(i.size), ctypes.c_uint64(x.size)]
                rc = lib.GxB_Vector_export_sparse(ctypes.c_void_p(i.ctypes.data), ctypes.c_void_p(x.ctypes.data),
                                                  getattr(lib, f"GrB_{index}"), getattr(lib, f"GrB_{dt}"),
                                                  *[ctypes.byref(t) for t in lens], v._h, False)
                assert rc == 0 and lens[0].value == lens[1].value == int(p.sum())
                assert np.array_equal(i[:-1], np.flatnonzero(p)) and i[-1] == -7
                assert np.array_equal(x[:-1], vals.astype(dm.NP[dt])) and x[-1] == -7


@pytest.mark.parametrize("offset", [1, 2, 3])
def test_exports_into_unaligned_slices(gb, subjects, offset):
    """outputs that start 1, 2 or 3 elements past a 16-byte boundary: the scalar head of
    k_sio_convert and k_sio_fill, and the groups whose stores are not aligned"""
    import torch

    for name, M, A in subjects:
        own = dm.name_of(A[1].dtype)
        for fmt, model in (("coo", sm.to_coo), ("csr", sm.to_csr), ("csc", sm.to_csc)):
            for index, dt in (("INT64", "INT16"), ("INT32", own), ("INT32", "FP64")):
                want = model(A, index, None if dt == own else dt)
                bufs = [torch.full((w.size + offset + 1,), 0x5a, dtype=torch.uint8, device="cuda").repeat_interleave(
                    w.dtype.itemsize).view(getattr(torch, str(w.dtype)) if w.dtype != np.bool_ else torch.uint8)
                    for w in want]
                assert all(b.data_ptr() % 16 == 0 for b in bufs)
                lens = [ctypes.c_uint64(w.size) for w in want]
                ptrs = [ctypes.c_void_p(b.data_ptr() + offset * w.dtype.itemsize) for b, w in zip(bufs, want)]
                rc = gb.lib.GxB_Matrix_export_sparse(*ptrs, getattr(gb.lib, f"GrB_{index}"), getattr(gb.lib, f"GrB_{dt}"),
                                                     *[ctypes.byref(x) for x in lens], FORMATS[fmt], M._h, True)
                assert rc == 0, rc
                M.wait()
                for b, w in zip(bufs, want):
                    h = host(b).view(np.uint8).reshape(-1, w.dtype.itemsize)
                    what = f"{name} {fmt} {index} {dt} +{offset}"
                    assert (h[:offset] == 0x5a).all() and (h[offset + w.size:] == 0x5a).all(), f"{what}: a stray write"
                    assert np.array_equal(h[offset:offset + w.size].ravel(), w.view(np.uint8).ravel()), what
