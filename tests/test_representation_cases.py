"""The tables of representation_cases.py checked without a GPU: both tables against the header
(every entry point that takes a vector has a consumer or an exclusion, every one that writes a
matrix or a vector has a producer or an exclusion), the stated properties of the operands, the
CPU side of the poison, and every consumer's and producer's model half run against a stand-in
for the device objects.  The stand-in answers every question with itself: that run shows only
that each row's model half executes and yields well-formed expectations (and, for the producers,
a model of the stated shape and type); whether a result matches its expectation is the GPU
file's business."""
import os

import numpy as np
import pytest

import dense_model as dm
import representation_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "graphblas_amd.h")


@pytest.fixture(scope="module")
def header():
    with open(HDR) as f:
        return rc.header_functions(f.read())


# ---------------------------------------------------------------------- the header guard
def test_header_parser(header):
    assert len(header) > 150
    for name in ("GrB_mxv", "GrB_Vector_assign_T", "GxB_Vector_eWiseUnion", "GrB_Matrix_diag", "GxB_Matrix_split",
                 "GrB_Vector_extractElement_T", "GxB_Vector_export_dense", "GrB_Matrix_reduce_BinaryOp"):
        assert name in header, name
    assert "GrB_Vector_assign_FP64" not in header  # a typed family is one name
    assert rc.takes_vector(header["GrB_mxv"]) and rc.takes_vector(header["GrB_Row_assign"])
    assert rc.takes_vector(header["GrB_Vector_nvals"]) and rc.takes_vector(header["GrB_Vector_resize"])
    assert not rc.takes_vector(header["GrB_mxm"]) and not rc.takes_vector(header["GrB_Vector_new"])
    assert rc.writes_object(header["GrB_mxm"]) and rc.writes_object(header["GrB_Vector_new"])
    assert rc.writes_object(header["GxB_Matrix_split"]) and rc.writes_object(header["GxB_Vector_sort"])
    assert not rc.writes_object(header["GrB_Matrix_nvals"]) and not rc.writes_object(header["GxB_Matrix_device_view"])
    assert not rc.writes_object(header["GrB_Vector_extractTuples_T"])


def _check(header, wanted, rows, excluded, what):
    need = {k for k, p in header.items() if wanted(p)}
    have = {e for r in rows.values() for e in r.entries}
    assert len(need) > 40
    missing = sorted(need - have - set(excluded))
    assert not missing, f"{what} without a row or an exclusion: {missing}"
    gone = sorted((have | set(excluded)) - set(header))
    assert not gone, f"the table names entry points that the header lacks: {gone}"
    both = sorted(have & set(excluded))
    assert not both, f"excluded although a row names them: {both}"
    for k, reason in excluded.items():
        assert k in need, f"{k} is excluded but is not {what}"
        assert isinstance(reason, str) and len(reason) > 10 and "\n" not in reason, k


def test_every_vector_input_has_a_consumer(header):
    _check(header, rc.takes_vector, rc.CONSUMERS, rc.VECTOR_INPUT_EXCLUDED, "an entry point that takes a GrB_Vector")


def test_every_object_output_has_a_producer(header):
    _check(header, rc.writes_object, rc.PRODUCERS, rc.OBJECT_OUTPUT_EXCLUDED,
           "an entry point that writes a GrB_Matrix or GrB_Vector")


# ---------------------------------------------------------------------- the operands
@pytest.mark.parametrize("dt", rc.TYPES)
@pytest.mark.parametrize("n", rc.SIZES)
def test_vector_model(n, dt):
    p, v = rc.vec_model(n, dt)
    assert p.shape == (n,) and v.dtype == dm.NP[dt] and not v[~p].any()
    w = rc.words_of(p)
    assert w.size == (n + 63) // 64 == (2 if n == 65 else 11)
    assert w[0] == np.uint64(2 ** 64 - 1) and p[0] and not p[n - 1]      # word 0 full, bit n - 1 clear
    assert (w == 0).any()                                                # one whole word clear
    assert int((~p).sum()) >= 1                                          # something to poison
    if n == 700:
        assert not p[64 * rc.CLEAR_WORD:64 * (rc.CLEAR_WORD + 1)].any() and n % 64 == 60
        assert 0.4 < p.mean() < 0.6
        assert len(np.unique(v[p])) == (2 if dt == "BOOL" else 4)
    assert v[p].max() <= 3 and (v[p] == 0).any() and (v[p] != 0).any()   # a value mask is not the structure
    for pattern in rc.PATTERNS:  # no stored value can be taken for the pattern
        assert not (v[p].view(np.uint8) == pattern).reshape(-1, v.itemsize).all(axis=1).any()
    o = rc.other_model(n, dt)
    assert (p & o[0]).any() and (p & ~o[0]).any() and (~p & o[0]).any() and (n == 65 or (~p & ~o[0]).any())


def test_types_patterns_sizes_and_mask_kinds():
    assert set(rc.TYPES) == {"FP64", "FP32", "INT32", "UINT8", "BOOL"} and rc.SIZES == (65, 700)
    assert rc.PATTERNS == (0x5A, 0xFF)
    for dt in ("FP64", "FP32"):
        t = dm.NP[dt]
        big = np.frombuffer(bytes([0x5A]) * t().itemsize, t)[0]
        assert np.isfinite(big) and big > 1e10 and np.isnan(np.frombuffer(bytes([0xFF]) * t().itemsize, t)[0])
    assert np.frombuffer(bytes([0xFF]) * 4, np.int32)[0] == -1 and np.frombuffer(bytes([0xFF]), np.uint8)[0] == 255
    assert 0x5A not in (0, 1)
    assert rc.MASK_KINDS == ("V", "S", "~V", "~S")
    for kind in rc.MASK_KINDS:
        assert f"mxv_mask_{kind}" in rc.CONSUMERS and f"mxv_mask_{kind}_replace" in rc.CONSUMERS
    for c in rc.CONSUMERS.values():
        assert set(c.types) == set(rc.TYPES), c.name  # every consumer runs in every type
    assert set(rc.EWISE_OPS) == {"plus", "min", "first", "second", "lor"}
    for dt in rc.TYPES:
        names = {f"{a}_{b}" for a, b, _ in rc.semirings(dt)}
        assert {"any_pair", "lor_land"} <= names and (dt == "BOOL" or {"plus_times", "min_plus"} <= names)
    A = rc.mat_model(90, 700, "FP64")
    assert A[0].sum(1).max() > 128 and not A[0][1].any() and A[0][:, 3].sum() == 89  # a long row, an empty one, a hot column
    assert rc.mat_model(40, 65, "FP64")[0].sum(1).max() <= 65


def test_required_consumers_and_producers_are_there():
    for name in ("mxv_u", "vxm_u", "mxv_u_merge_path", "mxv_u_rows", "mxv_u_hot", "vxm_u_pull", "vxm_u_push",
                 "mxv_w_accum", "inner_outer", "ewise_add_left", "ewise_add_right", "ewise_mult_left",
                 "ewise_mult_right", "ewise_union_left", "ewise_union_right", "apply_unary", "apply_bound",
                 "apply_rowindex", "select", "reduce", "isequal", "assign_u", "assign_w", "assign_mask", "subassign",
                 "line_assign", "extract", "scalar_assign", "extract_element", "remove_then_set", "resize", "dup",
                 "sort", "selectk_compactify", "scan", "diag", "reshape", "concat_split", "to_dense", "to_coo"):
        assert name in rc.CONSUMERS, name
    for name in ("mxm_dot", "mxm_hash", "mxm_esc", "mxm_colbits", "mxm_any_pair", "mxm_plus_pair_iso",
                 "mxv_general_65", "vxm_general_700", "vxm_iso_bfs", "mxv_iso_bfs_pull", "matrix_ewise_add",
                 "matrix_ewise_mult", "matrix_ewise_union", "matrix_apply_unary", "matrix_apply_right",
                 "matrix_select", "kronecker_binaryop", "transpose", "extract_matrix", "extract_column", "extract_vector",
                 "assign_matrix", "assign_matrix_scalar", "assign_vector", "assign_vector_scalar", "deferred_stamp",
                 "reduce_vector", "matrix_sort_values", "matrix_sort_permutation", "matrix_selectk",
                 "matrix_compactify", "matrix_scan", "concat_matrix", "split_matrix", "diag_new", "diag_matrix",
                 "diag_vector", "reshape_inplace", "reshape_dup", "flatten", "import_dense_matrix",
                 "import_sparse_coo", "import_sparse_csr", "import_sparse_csc", "import_device", "dup_matrix",
                 "resize_matrix", "clear_build_matrix", "elements_matrix", "elements_vector"):
        assert name in rc.PRODUCERS, name
    for p in rc.PRODUCERS.values():
        assert set(p.types) <= set(rc.BTYPES) and p.types, p.name
    for dt in rc.BTYPES:
        A = rc.big_model(dt)
        assert A[0].shape == (70, 300) and tuple(A[0].sum(1)[:6]) == rc.ROW_LENGTHS
    for name in ("transpose", "mxm_left", "mxm_right", "dot", "mask_S", "mask_V", "mask_cS_replace", "mask_cV_replace",
                 "mxv", "vxm", "ewise_add", "apply", "select", "reduce_rowwise", "reduce_columnwise", "reduce_scalar",
                 "extract", "sort", "dup_set", "concat", "to_csr"):
        assert name in rc.MATRIX_BATTERY, name
    for name in ("mxv", "mask_V", "mask_S", "mask_cS", "ewise_mult", "reduce", "assign", "extract", "diag", "to_dense"):
        assert name in rc.VECTOR_BATTERY, name


# ---------------------------------------------------------------------- the poison, CPU side
@pytest.mark.parametrize("n", [1, 63, 64, 65, 700])
def test_byte_mask(n):
    rng = np.random.default_rng(n)
    for p in (rng.random(n) < 0.5, np.zeros(n, bool), np.ones(n, bool), np.arange(n) == n - 1, np.arange(n) != n - 1):
        w = rc.words_of(p)
        assert w.dtype == np.uint64 and w.size == (n + 63) // 64
        if n % 64:
            assert int(w[-1]) >> (n % 64) == 0  # no bit past the size
        clear = rc.clear_slots(w, n)
        assert clear.shape == (n,) and np.array_equal(clear, ~p)
        assert np.array_equal(rc.clear_slots(w.view(np.int64), n), ~p)  # the words as torch hands them back
        for size in (1, 4, 8):
            m = rc.byte_mask(w, n, size)
            assert m.shape == (n * size,) and np.array_equal(m.reshape(n, size), np.repeat((~p)[:, None], size, 1))
            vals = np.arange(n * size, dtype=np.int64).astype(np.uint8) % 50  # never a pattern byte
            for pattern in rc.PATTERNS:
                x = vals.copy()
                x[m] = pattern
                held = (x.reshape(n, size) == pattern).all(axis=1)
                assert np.array_equal(held, ~p) and np.array_equal(x[~m], vals[~m])


def test_same_compares_bits():
    a = np.array([1.0, np.nan, 0.0])
    assert rc.same((a, 3, None), (a.copy(), 3, None)) is None
    assert rc.same((a,), (np.array([1.0, np.nan, -0.0]),)) is not None  # the sign of a zero is a bit
    assert rc.same(a, a.astype(np.float32)) is not None and rc.same(a, a[:2]) is not None
    assert rc.same(np.array([0x5A], np.uint8).view(bool), np.array([True])) is not None  # a bool byte that is not 1
    assert rc.same(None, 1) is not None and rc.same((1, 2), (1,)) is not None and rc.same(True, False) is not None


# ---------------------------------------------------------------------- the model halves
class Stub:
    """stands in for the library and its objects: the model half of a row runs without a GPU"""

    def __getattr__(self, k):
        if k.startswith("__"):
            raise AttributeError(k)
        return Stub()

    def __call__(self, *a, **k):
        return Stub()

    def __getitem__(self, k):
        return Stub()

    def __setitem__(self, k, v):
        pass

    def __delitem__(self, k):
        pass

    def __lshift__(self, o):
        return None

    def __invert__(self):
        return Stub()

    def __and__(self, o):
        return Stub()

    def __iter__(self):
        return iter([Stub(), Stub()])

    def __eq__(self, o):
        return True

    def __hash__(self):
        return 0

    def __int__(self):
        return 0

    def __array__(self, dtype=None, copy=None):
        return np.zeros((), dtype or np.float64)


@pytest.fixture()
def stubbed(monkeypatch):
    for name in ("vc", "mc"):
        monkeypatch.setattr(rc, name, lambda x: None)
    monkeypatch.setattr(rc.dc, "vec_coo", lambda x: None)
    monkeypatch.setattr(rc.dc, "coo", lambda x: None)
    return Stub()


def _well_formed(e, what):
    """an expectation: nested tuples of arrays, numbers and None, nothing of the stand-in's"""
    if isinstance(e, (tuple, list)):
        for k, x in enumerate(e):
            _well_formed(x, f"{what}[{k}]")
        return
    assert e is None or isinstance(e, (bool, int, float, np.generic, np.ndarray)), (what, type(e))


@pytest.mark.parametrize("dt", rc.TYPES)
@pytest.mark.parametrize("n", rc.SIZES)
def test_consumer_models_run(stubbed, n, dt):
    ran = 0
    for c in rc.CONSUMERS.values():
        if c.device:
            continue
        got, exp = c.fn(rc.Case(stubbed, n, dt, None))
        assert isinstance(exp, tuple) and (got is None or len(got) == len(exp)), c.name
        _well_formed(exp, c.name)
        ran += 1
    assert ran == len(rc.CONSUMERS) - 3  # to_dense, to_coo and as_replaced_output allocate device arrays


def test_producer_models_run(stubbed):
    ran = 0
    for p in rc.PRODUCERS.values():
        if p.device:
            continue
        for dt in p.types:
            _, m = p.fn(stubbed, dt)
            assert m[0].dtype == bool and m[0].shape == m[1].shape and m[0].ndim in (1, 2), p.name
            assert not m[1][~m[0]].any(), p.name  # the model convention: zero where absent
            assert max(m[0].shape) <= 700 and m[0].size <= 70 * 300 * 2, p.name  # the largest shapes of the file
            ran += 1
    assert ran > 150
