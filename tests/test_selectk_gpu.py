"""GxB_{Matrix,Vector}_selectk / _compactify on the device against tests/selectk_model.py.

Every comparison is exact and goes through to_coo(): shape, dtype, nvals, indices in order and value
bits.  (key, position) and (hash, position) are total orders, so the sub-wave class, the workgroup
class and the segmented radix sort must all choose the same entries.

Shapes and what they reach (class bounds read from the knobs' defaults, 64 and 2048):
  LENGTHS     rows of 0 .. 4 and 62 .. 66 entries (k-1, k, k+1 for every k below), 511 .. 513 (the
              workgroup class's one-wave rows end at 512), 2047 .. 2049, 6000, and 48 short rows
              packed between them, in 6000 columns; its transpose for the columnwise runs, so that
              columns reach the long classes too
  K           0, 1, 2, 3, 64, 65 and 10^9.  compactify to 10^9 columns is run rowwise only: the
              columnwise result has 10^9 rows, whose row pointer alone is 8 GB
  lowered     selectk_wave_max = 8, selectk_block_max = 64: every class just above its bound
  vectors     0, 1, 64, 65 and 70001 positions; k = 10^9 for selectk only (a compactified vector
              of 10^9 positions is 8 GB of dense values)
The four stat counters are checked against the row lengths wherever a value or random mode ran.
"""
import json
import os

import numpy as np
import pytest

import dense_model as dm
import selectk_model as km
from test_general_ops_gpu import _knobs, _rng, draw, iso_gb, to_gb

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = (0, 1, 2, 3, 64, 65, 10 ** 9)
SEED = 0x5EED5EED12345
VALUE_HOWS = ("smallest", "largest")


@pytest.fixture(scope="module")
def gb():
    import graphblas_amd

    return graphblas_amd


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "selectk_golden.json")) as f:
        return json.load(f)


def lengths():
    base = [0, 1, 2, 3, 4, 62, 63, 64, 65, 66, 511, 512, 513, 2047, 2048, 2049, 6000]
    rng = _rng("selectk lengths")
    more = list(rng.integers(0, 70, 48))  # short rows packed beside the long ones
    return [int(x) for x in rng.permutation(base + more + [2, 2, 3, 0])]


def values(dt, rng, n):
    """draw()'s mix of specials (type min / max, +-0.0, +-inf, denormals) and random values, no NaN"""
    v = draw(dt, rng, n)
    if dm.is_float(dt):
        v = np.where(np.isnan(v), dm.NP[dt](0.25), v).astype(dm.NP[dt])
    return v


_MODELS = {}


def ragged(dt, key="base", ties=False):
    """the LENGTHS matrix of type dt (shared: never written to)"""
    if (dt, key, ties) not in _MODELS:
        rng = _rng("selectk", dt, key)
        lens = lengths()
        p = np.zeros((len(lens), 6000), bool)
        for i, n in enumerate(lens):
            p[i, rng.choice(6000, n, replace=False)] = True
        if ties:  # three values: many ties in every row
            v = rng.choice(np.array([0, 1, 1, 2]).astype(dm.NP[dt]), p.size).reshape(p.shape)
        else:
            v = values(dt, rng, p.size).reshape(p.shape)
        _MODELS[dt, key, ties] = (p, np.where(p, v, dm.NP[dt](0)))
    return _MODELS[dt, key, ties]


def transposed(A):
    return np.ascontiguousarray(A[0].T), np.ascontiguousarray(A[1].T)


def is_iso(A):
    from graphblas_amd.device import matrix_view, vector_view

    return bool((vector_view if A.ndim == 1 else matrix_view)(A._h).iso)


def expect_stats(gb, A, k, columnwise, ranked_all, wave_max=64, block_max=2048):
    """rows kept whole, and rows of two or more entries ranked per class (ranked_all: compactify by
    value ranks every row, selectk and "random" only those of more than k entries)"""
    d = A[0].sum(axis=0 if columnwise else 1)
    r = d[(d >= 2) & ((d > k) | ranked_all)]
    want = (int((d <= k).sum()), int((r <= wave_max).sum()), int(((r > wave_max) & (r <= block_max)).sum()),
            int((r > block_max).sum()))
    got = tuple(gb.get_knob(f"stat_selectk_rows_{c}") for c in ("all", "wave", "block", "long"))
    assert got == want, f"rows per class {got}, expected {want}"
    return got


def run_matrix(gb, a, A, dt, how, k, order, *, iso=False, compact_too=True, stats=None):
    """selectk and the four compactify variants of one (how, k, order) against the model"""
    col = order == "columnwise"
    what = f"{dt} {how} k={k} {order}"
    C = a.ss.selectk(how, k, order, seed=SEED)
    km.same(C, km.selectk(A, how, k, columnwise=col, seed=SEED, iso=iso), dt, "selectk " + what)
    if C.nvals:
        assert is_iso(C) == iso
    ranked = how in VALUE_HOWS + ("random",) and not (iso and how in VALUE_HOWS)
    if stats is not None and ranked and k > 0:
        expect_stats(gb, A, k, col, False, **stats)
    if not compact_too or (col and k == 10 ** 9):
        return
    for reverse in (False, True):
        for asindex in (False, True):
            C = a.ss.compactify(how, k, order, reverse=reverse, asindex=asindex, seed=SEED)
            want = km.compactify(A, how, k, columnwise=col, reverse=reverse, asindex=asindex, seed=SEED, iso=iso)
            km.same(C, want, "UINT64" if asindex else dt, f"compactify {what} reverse={reverse} asindex={asindex}")
            if C.nvals:
                assert is_iso(C) == (iso and not asindex)
            if stats is not None and k > 0 and not iso and how in VALUE_HOWS:
                expect_stats(gb, A, k, col, True, **stats)


# ---------------------------------------------------------------------- golden, errors, front end
def golden_obj(gb, g, name):
    base, iso = (name[:-4], True) if name.endswith("_iso") else (name, False)
    a = g[base]
    vals = 1 if iso else a["vals"]
    if base == "A":
        return gb.Matrix.from_coo(a["rows"], a["cols"], vals, dtype=a["dtype"], nrows=a["nrows"], ncols=a["ncols"])
    return gb.Vector.from_coo(a["idx"], vals, dtype=a["dtype"], size=a["size"])


def test_golden_cases(gb, golden):
    from test_selectk_abi import accepted

    objs = {}
    for case in golden["matrix_cases"] + golden["vector_cases"]:
        x = objs.setdefault(case["input"], golden_obj(gb, golden, case["input"]))
        args = [case["order"]] if "order" in case else []
        if case["op"] == "selectk":
            got = x.ss.selectk(case["how"], case["k"], *args)
        else:
            got = x.ss.compactify(case["how"], case["k"], *args, reverse=case["reverse"], asindex=case["asindex"])
        out = got.to_coo()
        idx = tuple(np.asarray(i).astype(np.int64) for i in out[:-1])
        assert got.nvals == out[-1].size
        if "count_range" in case:
            lo, hi = case["count_range"]
            counts = np.bincount(idx[1 if case["order"] == "columnwise" else 0], minlength=7)
            assert counts.min() == lo and counts.max() == hi and got.shape == x.shape, case
            continue
        assert got.dtype == ("UINT64" if case.get("asindex") else "INT64"), case
        assert accepted(golden, case, (got.shape, idx, out[-1])), (case, out)
        if case["op"] == "compactify" and case["k"] is not None:
            want = (case["k"],) if x.ndim == 1 else (x.nrows, case["k"]) if case["order"] == "rowwise" \
                else (case["k"], x.ncols)
            assert tuple(got.shape) == want, case


def test_error_returns_leave_the_outputs_untouched(gb, golden):
    from test_sort_gpu import same_coo

    lib = gb.lib
    A = golden_obj(gb, golden, "A")
    v = golden_obj(gb, golden, "v")
    C = gb.Matrix.from_coo([1, 2], [3, 4], [5, 6], dtype="INT64", nrows=7, ncols=7)
    C3 = gb.Matrix.from_coo([1, 2], [0, 2], [5, 6], dtype="INT64", nrows=7, ncols=3)
    C37 = gb.Matrix.from_coo([1, 2], [0, 2], [5, 6], dtype="INT64", nrows=3, ncols=7)
    CF = gb.Matrix.from_coo([1, 2], [0, 2], [5.0, 6.0], dtype="FP64", nrows=7, ncols=3)
    CF7 = gb.Matrix.from_coo([1, 2], [0, 2], [5.0, 6.0], dtype="FP64", nrows=7, ncols=7)
    CU = gb.Matrix.from_coo([1, 2], [0, 2], [5, 6], dtype="UINT64", nrows=7, ncols=3)
    FIRST, T0 = lib.GxB_SELECTK_FIRST, lib.GrB_DESC_T0
    sel = [(lib.GrB_INVALID_VALUE, (C._h, A._h, 5, 1, 0, None)),
           (lib.GrB_INVALID_VALUE, (C._h, A._h, -1, 1, 0, None)),
           (lib.GrB_NULL_POINTER, (C._h, None, FIRST, 1, 0, None)),
           (lib.GrB_NULL_POINTER, (None, A._h, FIRST, 1, 0, None)),
           (lib.GrB_DIMENSION_MISMATCH, (C3._h, A._h, FIRST, 1, 0, None)),
           (lib.GrB_DIMENSION_MISMATCH, (C37._h, A._h, FIRST, 1, 0, T0)),
           (lib.GrB_DOMAIN_MISMATCH, (CF7._h, A._h, FIRST, 1, 0, None))]
    for want, args in sel:
        assert lib.GxB_Matrix_selectk(*args) == want, (want, args)
    cmp_ = [(lib.GrB_INVALID_VALUE, (C3._h, A._h, 7, 3, False, False, 0, None)),
            (lib.GrB_DIMENSION_MISMATCH, (C3._h, A._h, FIRST, 2, False, False, 0, None)),
            (lib.GrB_DIMENSION_MISMATCH, (C3._h, A._h, FIRST, 3, False, False, 0, T0)),
            (lib.GrB_DIMENSION_MISMATCH, (C37._h, A._h, FIRST, 3, False, False, 0, None)),
            (lib.GrB_DIMENSION_MISMATCH, (C._h, A._h, FIRST, 3, False, False, 0, None)),
            (lib.GrB_DOMAIN_MISMATCH, (CF._h, A._h, FIRST, 3, False, False, 0, None)),
            (lib.GrB_DOMAIN_MISMATCH, (CF._h, A._h, FIRST, 3, False, True, 0, None)),
            (lib.GrB_DOMAIN_MISMATCH, (CU._h, A._h, FIRST, 3, False, False, 0, None))]
    for want, args in cmp_:
        assert lib.GxB_Matrix_compactify(*args) == want, (want, args)
    same_coo(C, ([1, 2], [3, 4]), [5, 6], "INT64", "C after a refusal")
    same_coo(C3, ([1, 2], [0, 2]), [5, 6], "INT64", "C3 after a refusal")
    same_coo(C37, ([1, 2], [0, 2]), [5, 6], "INT64", "C37 after a refusal")
    same_coo(CF, ([1, 2], [0, 2]), [5.0, 6.0], "FP64", "CF after a refusal")
    same_coo(CU, ([1, 2], [0, 2]), [5, 6], "UINT64", "CU after a refusal")
    w = gb.Vector.from_coo([2], [5], dtype="INT64", size=7)
    w3 = gb.Vector.from_coo([2], [5], dtype="INT64", size=3)
    wf = gb.Vector.from_coo([2], [5.0], dtype="FP32", size=7)
    assert lib.GxB_Vector_selectk(w._h, v._h, 9, 1, 0, None) == lib.GrB_INVALID_VALUE
    assert lib.GxB_Vector_selectk(w3._h, v._h, FIRST, 1, 0, None) == lib.GrB_DIMENSION_MISMATCH
    assert lib.GxB_Vector_selectk(wf._h, v._h, FIRST, 1, 0, None) == lib.GrB_DOMAIN_MISMATCH
    assert lib.GxB_Vector_selectk(w._h, None, FIRST, 1, 0, None) == lib.GrB_NULL_POINTER
    assert lib.GxB_Vector_compactify(w._h, v._h, FIRST, 3, False, False, 0, None) == lib.GrB_DIMENSION_MISMATCH
    assert lib.GxB_Vector_compactify(w3._h, v._h, 5, 3, False, False, 0, None) == lib.GrB_INVALID_VALUE
    assert lib.GxB_Vector_compactify(wf._h, v._h, FIRST, 7, False, True, 0, None) == lib.GrB_DOMAIN_MISMATCH
    same_coo(w, ([2],), [5], "INT64", "w after a refusal")
    same_coo(w3, ([2],), [5], "INT64", "w3 after a refusal")
    same_coo(wf, ([2],), [5.0], "FP32", "wf after a refusal")
    with pytest.raises(ValueError, match="negative k is not allowed"):
        A.ss.compactify("first", -2)
    with pytest.raises(ValueError, match="Bad value for order"):
        A.ss.selectk("first", 1, "diagonal")


def test_aliasing_prefilled_outputs_and_index_type(gb):
    A = ragged("INT64")
    lib = gb.lib
    for how, name in ((lib.GxB_SELECTK_LARGEST, "largest"), (lib.GxB_SELECTK_RANDOM, "random")):
        a = to_gb(gb, A)
        assert lib.GxB_Matrix_selectk(a._h, a._h, how, 3, SEED, None) == 0  # C == A
        km.same(a, km.selectk(A, name, 3, seed=SEED), "INT64", f"C == A {name}")
        a = to_gb(gb, A)
        assert lib.GxB_Matrix_selectk(a._h, a._h, how, 3, SEED, lib.GrB_DESC_T0) == 0
        km.same(a, km.selectk(A, name, 3, columnwise=True, seed=SEED), "INT64", f"C == A {name} T0")
    # a prefilled (iso) output is replaced; an INT64 A may take its own indices as INT64
    a = to_gb(gb, A)
    other, _ = iso_gb(gb, ragged("INT64", "other")[0][:, :5], 3, "INT64")
    assert lib.GxB_Matrix_compactify(other._h, a._h, lib.GxB_SELECTK_SMALLEST, 5, True, True, 0, None) == 0
    shape, idx, x = km.compactify(A, "smallest", 5, reverse=True, asindex=True)
    km.same(other, (shape, idx, x.astype(np.int64)), "INT64", "indices into an INT64 C")
    u = (A[0][7], A[1][7])
    w = to_gb(gb, u)
    assert lib.GxB_Vector_selectk(w._h, w._h, lib.GxB_SELECTK_SMALLEST, 4, 0, None) == 0
    km.same(w, km.selectk_vector(u, "smallest", 4), "INT64", "w == u")


def test_seeds(gb):
    A = ragged("INT32")
    a = to_gb(gb, A)
    one = a.ss.selectk("random", 3, seed=77)
    two = a.ss.selectk("random", 3, seed=77)
    assert all(np.array_equal(x, y) for x, y in zip(one.to_coo(), two.to_coo()))
    km.same(one, km.selectk(A, "random", 3, seed=77), "INT32", "seed 77")
    other = a.ss.selectk("random", 3, seed=78)
    assert not np.array_equal(one.to_coo()[1], other.to_coo()[1])
    km.same(a.ss.selectk("random", 3, seed=2 ** 64 - 1), km.selectk(A, "random", 3, seed=2 ** 64 - 1), "INT32",
            "seed 2^64 - 1")
    # seed=None draws from numpy.random: np.random.seed governs it
    np.random.seed(5)
    x = a.ss.compactify("random", 2, asindex=True)
    y = a.ss.selectk("random", 2)
    np.random.seed(5)
    x2 = a.ss.compactify("random", 2, asindex=True)
    y2 = a.ss.selectk("random", 2)
    assert np.array_equal(x.to_coo()[2], x2.to_coo()[2]) and np.array_equal(y.to_coo()[1], y2.to_coo()[1])
    v = to_gb(gb, (A[0][3], A[1][3]))
    km.same(v.ss.selectk("random", 5, seed=9), km.selectk_vector((A[0][3], A[1][3]), "random", 5, seed=9), "INT32",
            "vector seed")


# ---------------------------------------------------------------------- every mode, every k, both orders
@pytest.mark.parametrize("order", ["rowwise", "columnwise"])
@pytest.mark.parametrize("how", km.HOWS)
def test_every_mode_and_k(gb, how, order):
    A = ragged("FP64")
    if order == "columnwise":
        A = transposed(A)
    a = to_gb(gb, A)
    for k in K:
        run_matrix(gb, a, A, "FP64", how, k, order, stats={})
    # no k: the longest row (column)
    C = a.ss.compactify(how, None, order, asindex=True, seed=SEED)
    km.same(C, km.compactify(A, how, None, columnwise=order == "columnwise", asindex=True, seed=SEED), "UINT64",
            f"{how} {order} default k")
    assert 6000 in C.shape


@pytest.mark.parametrize("how", km.HOWS)
def test_short_columns(gb, how):
    """columnwise on the wide matrix: 6000 columns of at most 65 entries"""
    A = ragged("INT16")
    a = to_gb(gb, A)
    for k in (1, 3, 64):
        run_matrix(gb, a, A, "INT16", how, k, "columnwise", stats={})


@pytest.mark.parametrize("how", ["smallest", "largest", "random"])
def test_lowered_class_bounds(gb, how):
    assert (gb.get_knob("selectk_wave_max"), gb.get_knob("selectk_block_max")) == (64, 2048)
    A = ragged("FP32")
    a = to_gb(gb, A)
    with _knobs(gb, selectk_wave_max=8, selectk_block_max=64):
        assert (gb.get_knob("selectk_wave_max"), gb.get_knob("selectk_block_max")) == (8, 64)
        for k in (1, 3, 65):
            run_matrix(gb, a, A, "FP32", how, k, "rowwise", stats=dict(wave_max=8, block_max=64))
            got = tuple(gb.get_knob(f"stat_selectk_rows_{c}") for c in ("wave", "block", "long"))
            assert all(got[1:]) or k > 64, got  # rows of more than 65 entries are all long under these bounds
    run_matrix(gb, a, A, "FP32", how, 3, "rowwise", stats={})
    got = tuple(gb.get_knob(f"stat_selectk_rows_{c}") for c in ("all", "wave", "block", "long"))
    assert all(got), got  # the shape reaches every class at the default bounds


@pytest.mark.parametrize("dt", dm.ALL)
def test_value_modes_every_type(gb, dt):
    A = ragged(dt)
    a = to_gb(gb, A)
    for how in VALUE_HOWS:
        for k in (2, 65):
            run_matrix(gb, a, A, dt, how, k, "rowwise", stats={})


@pytest.mark.parametrize("dt", ["INT8", "FP32", "FP64", "BOOL"])
def test_many_ties(gb, dt):
    A = ragged(dt, "ties", ties=True)
    At = transposed(A)
    a, at = to_gb(gb, A), to_gb(gb, At)
    for how in VALUE_HOWS:
        for k in (1, 3, 64):
            run_matrix(gb, a, A, dt, how, k, "rowwise")
        run_matrix(gb, at, At, dt, how, 65, "columnwise")


def test_signed_zeros_and_extremes(gb):
    for dt in ("FP32", "FP64"):
        t = dm.NP[dt]
        f = np.finfo(t)
        pool = np.array([np.inf, -np.inf, f.smallest_subnormal, -f.smallest_subnormal, f.max, -f.max, 0.0, -0.0, 0.0,
                         -0.0, 1.0], t)
        p = ragged(dt)[0]
        rng = _rng("selectk zeros", dt)
        A = (p, np.where(p, rng.choice(pool, p.size).reshape(p.shape), t(0)))
        a = to_gb(gb, A)
        for how in VALUE_HOWS:
            for k in (2, 64):
                run_matrix(gb, a, A, dt, how, k, "rowwise")


@pytest.mark.parametrize("how", km.HOWS)
def test_iso_input(gb, how):
    p = ragged("INT16")[0]
    a, A = iso_gb(gb, p, -7, "INT16")
    assert is_iso(a)
    for k in (0, 2, 65):
        run_matrix(gb, a, A, "INT16", how, k, "rowwise", iso=True)
    at, At = iso_gb(gb, np.ascontiguousarray(p.T), -7, "INT16")
    run_matrix(gb, at, At, "INT16", how, 3, "columnwise", iso=True)


@pytest.mark.parametrize("shape", [(1, 1), (0, 5), (5, 0), (9, 11)])
def test_degenerate_shapes(gb, shape):
    p = np.zeros(shape, bool)
    if shape == (1, 1):
        p[0, 0] = True
    A = (p, np.where(p, np.int16(-3), np.int16(0)))
    a = to_gb(gb, A)
    for how in km.HOWS:
        for order in ("rowwise", "columnwise"):
            for k in (0, 1, 2):
                run_matrix(gb, a, A, "INT16", how, k, order)
            C = a.ss.compactify(how, None, order)
            assert C.nvals == int(p.sum()) and set(C.shape) <= {0, 1, 5, 9, 11}


# ---------------------------------------------------------------------- grid sweeps
@pytest.mark.parametrize("cap", [1, 3, 33, 0])
def test_matrix_cases_under_grid_cap(gb, cap):
    A = ragged("INT32")
    At = transposed(A)
    a, at = to_gb(gb, A), to_gb(gb, At)
    gb.set_knob("grid_cap", cap)
    try:
        for how in km.HOWS:
            for k in (3, 65):
                run_matrix(gb, a, A, "INT32", how, k, "rowwise", stats={})
            run_matrix(gb, at, At, "INT32", how, 3, "columnwise", stats={})
            run_matrix(gb, a, A, "INT32", how, 2, "columnwise")
        with _knobs(gb, selectk_wave_max=8, selectk_block_max=64):
            run_matrix(gb, a, A, "INT32", "largest", 3, "rowwise", stats=dict(wave_max=8, block_max=64))
    finally:
        gb.set_knob("grid_cap", 0)


# ---------------------------------------------------------------------- vectors
@pytest.mark.parametrize("fill", ["sparse", "full", "empty"])
@pytest.mark.parametrize("n", [0, 1, 64, 65, 70001])
def test_vectors(gb, n, fill):
    dt = "FP64" if n != 65 else "INT8"
    rng = _rng("selectk vec", n, fill)
    p = {"sparse": rng.random(n) < 0.4, "full": np.ones(n, bool), "empty": np.zeros(n, bool)}[fill]
    um = (p, np.where(p, values(dt, rng, n), dm.NP[dt](0)))
    u = to_gb(gb, um)
    nv = int(p.sum())
    for how in km.HOWS:
        for k in ((0, 3, 65, 10 ** 9) if n > 65 else K):
            w = u.ss.selectk(how, k, seed=SEED)
            km.same(w, km.selectk_vector(um, how, k, seed=SEED), dt, f"vector selectk {n} {fill} {how} {k}")
            assert w.dup().nvals == min(k, nv)  # the device count is current
            if k == 10 ** 9:
                continue
            for reverse, asindex in ((False, False), (True, False), (False, True), (True, True)):
                w = u.ss.compactify(how, k, reverse=reverse, asindex=asindex, seed=SEED)
                want = km.compactify_vector(um, how, k, reverse=reverse, asindex=asindex, seed=SEED)
                km.same(w, want, "UINT64" if asindex else dt,
                        f"vector compactify {n} {fill} {how} {k} reverse={reverse} asindex={asindex}")
                assert w.dup().nvals == min(k, nv)
        w = u.ss.compactify(how, asindex=True, seed=SEED)
        km.same(w, km.compactify_vector(um, how, None, asindex=True, seed=SEED), "UINT64", f"default size {how}")
        assert w.size == nv


@pytest.mark.parametrize("how", km.HOWS)
def test_iso_vectors(gb, how):
    pv = np.zeros(70, bool)
    pv[[3, 9, 64, 69]] = True
    u, um = iso_gb(gb, pv, 2.5, "FP32")
    for k in (0, 1, 3, 9):
        w = u.ss.selectk(how, k, seed=SEED)
        km.same(w, km.selectk_vector(um, how, k, seed=SEED, iso=True), "FP32", f"iso vector selectk {how} {k}")
        assert is_iso(w) or w.nvals == 0
        for reverse in (False, True):
            for asindex in (False, True):
                w = u.ss.compactify(how, k, reverse=reverse, asindex=asindex, seed=SEED)
                want = km.compactify_vector(um, how, k, reverse=reverse, asindex=asindex, seed=SEED, iso=True)
                km.same(w, want, "UINT64" if asindex else "FP32", f"iso vector compactify {how} {k}")
