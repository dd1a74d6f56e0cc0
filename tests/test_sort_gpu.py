"""GxB_Matrix_sort / GxB_Vector_sort on the device against tests/sort_model.py.

Every comparison is exact and goes through to_coo(): indices, order, nvals, dtype and value bits
(the sign of zero included).  (key, original index) is a total order, so the sub-wave class, the
workgroup class, the segmented radix sort and sort_method = 1 must all give the same bits.

Shapes and what they reach (class bounds read from the knobs' defaults, 64 and 2048):
  LENGTHS        rows of 0, 1, 2 .. 129 and 6000 entries, and cap - 1, cap, cap + 1 for both bounds
                 and for the 512 entries up to which the workgroup class sorts a row in one wave
                 (SORT_SMALL_CAP, read from the source): every sub-wave group size, both
                 workgroup sizes, hipCUB
  lowered        sort_wave_max = 8, sort_block_max = 64: every class sorts rows just above the
                 lowered bounds; sort_method = 1: everything through hipCUB
  140000 x 70    runs of one-entry rows, alternating empty and 64-entry rows; with sort_grid = 2
                 every stride loop runs many times
The three stat counters are checked against the row lengths in every one of these.
"""
import json
import os
import re

import numpy as np
import pytest

import dense_model as dm
import sort_model as sm
from test_general_ops_gpu import _knobs, _rng, check, draw, iso_gb, to_gb
from test_indexing_gpu import bitmap_words

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPS = ["lt", "gt"]


@pytest.fixture(scope="module")
def gb():
    import graphblas_amd

    return graphblas_amd


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "sort_golden.json")) as f:
        return json.load(f)


def caps(gb):
    return gb.get_knob("sort_wave_max"), gb.get_knob("sort_block_max")


def small_cap():
    src = open(os.path.join(ROOT, "graph-python_amd", "csrc", "gb_sort.hip")).read()
    return int(re.search(r"#define SORT_SMALL_CAP (\d+)", src).group(1))


def values(dt, rng, n):
    """draw()'s mix of specials (type min / max, +-0.0, +-inf, denormals) and random values, no NaN"""
    v = draw(dt, rng, n)
    if dm.is_float(dt):
        v = np.where(np.isnan(v), dm.NP[dt](0.25), v).astype(dm.NP[dt])
    return v


def ragged(lengths, ncols, dt, key, vals=None):
    """a model matrix whose row i has lengths[i] entries at random columns"""
    rng = _rng("sort", dt, key)
    p = np.zeros((len(lengths), ncols), bool)
    for i, n in enumerate(lengths):
        p[i, rng.choice(ncols, n, replace=False)] = True
    v = values(dt, rng, p.size).reshape(p.shape) if vals is None else vals(rng, p.shape)
    return p, np.where(p, v, dm.NP[dt](0))


def sort_both(gb, A, op, **kw):
    return A.ss.sort(getattr(gb.binary, op), **kw)


def check_sorted(gb, A, model, op, dt, what, *, columnwise=False, op_dtype=None):
    C, P = A.ss.sort(getattr(gb.binary, op)[op_dtype or dt], "columnwise" if columnwise else "rowwise")
    wc, wp = sm.sort_matrix(model, op, op_dtype, columnwise)
    check(C, wc, dt, what=what + " C")
    check(P, wp, "UINT64", what=what + " P")
    return C, P


def expect_stats(gb, lengths, wave_max, block_max, method=0):
    n = np.asarray(lengths)
    n = n[n >= 2]
    if method == 1:
        want = (0, 0, n.size)
    else:
        want = (int((n <= wave_max).sum()), int(((n > wave_max) & (n <= block_max)).sum()), int((n > block_max).sum()))
    got = tuple(gb.get_knob(f"stat_sort_rows_{c}") for c in ("wave", "block", "long"))
    assert got == want, f"rows per class {got}, expected {want}"
    assert sum(got) == n.size
    return got


def lengths_for(gb):
    wm, bm = caps(gb)
    assert (wm, bm) == (64, 2048)
    base = [0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 128, 129, 6000]
    sc = small_cap()
    assert wm < sc < bm
    edge = [wm - 1, wm, wm + 1, sc - 1, sc, sc + 1, bm - 1, bm, bm + 1]
    rng = _rng("lengths")
    more = list(rng.integers(0, 70, 48))  # short rows packed next to the long ones
    out = base + edge + more + [2, 2, 2, 3, 0]
    return [int(x) for x in rng.permutation(out)]


CONFIGS = {"default": {}, "method1": {"sort_method": 1}, "lowered": {"sort_wave_max": 8, "sort_block_max": 64},
           "grid2": {"sort_grid": 2}}


# ---------------------------------------------------------------------- golden
def golden_A(gb, g):
    a = g["A"]
    return gb.Matrix.from_coo(a["rows"], a["cols"], a["vals"], dtype=a["dtype"], nrows=a["nrows"], ncols=a["ncols"])


def same_coo(obj, idx, vals, dt, what):
    """obj against expected triples given in any order (to_coo() is row-major)"""
    got = obj.to_coo()
    assert obj.dtype == dt and obj.nvals == len(vals), what
    idx = [np.asarray(x, np.int64) for x in idx]
    order = np.lexsort(idx[::-1])
    for a, b in zip(got[:-1], idx):
        assert np.array_equal(np.asarray(a).astype(np.int64), b[order]), what
    assert got[-1].dtype == dm.NP[dt] and np.array_equal(got[-1], np.asarray(vals, dm.NP[dt])[order]), what


@pytest.mark.parametrize("values_,permutation", [(True, True), (True, False), (False, True), (False, False)])
def test_golden_front_end(gb, golden, values_, permutation):
    A = golden_A(gb, golden)
    for case in golden["matrix_cases"]:
        C, P = A.ss.sort(case["op"], case["order"], values=values_, permutation=permutation, nthreads=4)
        idx = (case["rows"], case["cols"])
        assert (C is None) == (not values_) and (P is None) == (not permutation)
        if values_:
            assert C.name == "Values" and (C.nrows, C.ncols) == (7, 7)
            same_coo(C, idx, case["C"], "INT64", case["source"])
        if permutation:
            assert P.name == "Permutation"
            same_coo(P, idx, case["P"], "UINT64", case["source"])
    u = golden["v"]
    v = gb.Vector.from_coo(u["idx"], u["vals"], dtype=u["dtype"], size=u["size"])
    for case in golden["vector_cases"]:
        w, p = v.ss.sort(case["op"], values=values_, permutation=permutation, nthreads=None)
        assert (w is None) == (not values_) and (p is None) == (not permutation)
        if values_:
            assert w.name == "Values" and w.size == 7
            same_coo(w, (case["idx"],), case["w"], "INT64", case["source"])
        if permutation and case["p"] is not None:
            assert p.name == "Permutation"
            same_coo(p, (case["idx"],), case["p"], "UINT64", case["source"])


def test_golden_operator_forms(gb, golden):
    A = golden_A(gb, golden)
    case = golden["matrix_cases"][2]
    for op in (">", gb.binary.gt, gb.binary.gt["INT64"]):
        for order in ("columnwise", "col", "F"):
            C, P = A.ss.sort(op, order)
            same_coo(C, (case["rows"], case["cols"]), case["C"], "INT64", repr(op))
            same_coo(P, (case["rows"], case["cols"]), case["P"], "UINT64", repr(op))
    with pytest.raises(ValueError):
        A.ss.sort("<", "diagonal")


@pytest.mark.parametrize("with_c,with_p", [(True, True), (True, False), (False, True)])
def test_golden_through_ctypes(gb, golden, with_c, with_p):
    lib = gb.lib
    A = golden_A(gb, golden)
    for case in golden["matrix_cases"]:
        C, P = gb.Matrix("INT64", 7, 7), gb.Matrix("INT64", 7, 7)  # INT64 is allowed for P
        op = getattr(lib, f"GrB_{case['op'].upper()}_INT64")
        desc = lib.GrB_DESC_T0 if case["order"] == "columnwise" else None
        assert lib.GxB_Matrix_sort(C._h if with_c else None, P._h if with_p else None, op, A._h, desc) == 0
        idx = (case["rows"], case["cols"])
        if with_c:
            same_coo(C, idx, case["C"], "INT64", case["source"])
        else:
            assert C.nvals == 0
        if with_p:
            same_coo(P, idx, case["P"], "INT64", case["source"])
        else:
            assert P.nvals == 0


def test_error_codes_leave_outputs_untouched(gb, golden):
    from graphblas_amd.exceptions import DomainMismatch, NotImplementedException

    lib = gb.lib
    A = golden_A(gb, golden)
    v = gb.Vector.from_coo(golden["v"]["idx"], golden["v"]["vals"], size=7)
    with pytest.raises(DomainMismatch):
        A.ss.sort("+")
    with pytest.raises(DomainMismatch):
        v.ss.sort(gb.binary.plus)
    for op in ("le", "ge", "eq", "ne", "pair", "lxor"):
        with pytest.raises(NotImplementedException):
            A.ss.sort(getattr(gb.binary, op)["BOOL"] if op in ("pair", "lxor") else getattr(gb.binary, op))
        with pytest.raises(NotImplementedException):
            v.ss.sort(getattr(gb.binary, op)["BOOL"] if op in ("pair", "lxor") else getattr(gb.binary, op))
    with pytest.raises(NotImplementedException):
        A.ss.sort(gb.monoid.lxnor)  # a Monoid gives its binary operator, which is no order
    C = gb.Matrix.from_coo([1, 2], [3, 4], [5, 6], dtype="INT64", nrows=7, ncols=7)
    P = gb.Matrix.from_coo([0], [6], [9], dtype="UINT64", nrows=7, ncols=7)
    LT, NULL = lib.GrB_LT_INT64, None
    P32, PF, C78, P67 = gb.Matrix("INT32", 7, 7), gb.Matrix("FP64", 7, 7), gb.Matrix("INT64", 7, 8), gb.Matrix("UINT64", 6, 7)
    codes = [
        (lib.GrB_NULL_POINTER, (NULL, NULL, LT, A._h, NULL)),
        (lib.GrB_NULL_POINTER, (C._h, P._h, NULL, A._h, NULL)),
        (lib.GrB_NULL_POINTER, (C._h, P._h, LT, NULL, NULL)),
        (lib.GrB_DOMAIN_MISMATCH, (C._h, P._h, lib.GrB_PLUS_INT64, A._h, NULL)),
        (lib.GrB_DOMAIN_MISMATCH, (C._h, P._h, lib.GxB_FIRSTI_INT64, A._h, NULL)),
        (lib.GrB_NOT_IMPLEMENTED, (C._h, P._h, lib.GrB_LE_INT64, A._h, NULL)),
        (lib.GrB_NOT_IMPLEMENTED, (C._h, P._h, lib.GrB_EQ_INT64, A._h, NULL)),
        (lib.GrB_NOT_IMPLEMENTED, (C._h, P._h, lib.GxB_PAIR_BOOL, A._h, NULL)),
        (lib.GrB_NOT_IMPLEMENTED, (C._h, P._h, lib.GrB_LXOR, A._h, NULL)),
        (lib.GrB_NOT_IMPLEMENTED, (C._h, C._h, LT, A._h, NULL)),
        (lib.GrB_DOMAIN_MISMATCH, (C._h, P32._h, LT, A._h, NULL)),
        (lib.GrB_DOMAIN_MISMATCH, (C._h, PF._h, LT, A._h, NULL)),
        (lib.GrB_DIMENSION_MISMATCH, (C78._h, P._h, LT, A._h, NULL)),
        (lib.GrB_DIMENSION_MISMATCH, (C._h, P67._h, LT, A._h, NULL)),
    ]
    for want, args in codes:
        assert lib.GxB_Matrix_sort(*args) == want, (want, args)
        same_coo(C, ([1, 2], [3, 4]), [5, 6], "INT64", "C after a refusal")
        same_coo(P, ([0], [6]), [9], "UINT64", "P after a refusal")
    w = gb.Vector.from_coo([2], [5], dtype="INT64", size=7)
    p = gb.Vector.from_coo([3], [1], dtype="UINT64", size=7)
    p8, w8 = gb.Vector("INT8", 7), gb.Vector("INT64", 8)
    vcodes = [
        (lib.GrB_NULL_POINTER, (NULL, NULL, LT, v._h, NULL)),
        (lib.GrB_NULL_POINTER, (w._h, p._h, NULL, v._h, NULL)),
        (lib.GrB_NULL_POINTER, (w._h, p._h, LT, NULL, NULL)),
        (lib.GrB_DOMAIN_MISMATCH, (w._h, p._h, lib.GrB_PLUS_INT64, v._h, NULL)),
        (lib.GrB_NOT_IMPLEMENTED, (w._h, p._h, lib.GrB_GE_INT64, v._h, NULL)),
        (lib.GrB_NOT_IMPLEMENTED, (w._h, w._h, LT, v._h, NULL)),
        (lib.GrB_DOMAIN_MISMATCH, (w._h, p8._h, LT, v._h, NULL)),
        (lib.GrB_DIMENSION_MISMATCH, (w8._h, p._h, LT, v._h, NULL)),
    ]
    for want, args in vcodes:
        assert lib.GxB_Vector_sort(*args) == want, (want, args)
        same_coo(w, ([2],), [5], "INT64", "w after a refusal")
        same_coo(p, ([3],), [1], "UINT64", "p after a refusal")


# ---------------------------------------------------------------------- row lengths, every class
@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("dt", dm.ALL)
def test_row_lengths_every_type(gb, dt, op, config):
    lengths = lengths_for(gb)
    model = ragged(lengths, 6000, dt, "lengths")
    A = to_gb(gb, model)
    kv = CONFIGS[config]
    with _knobs(gb, **kv):
        check_sorted(gb, A, model, op, dt, f"{dt} {op} {config}")
        got = expect_stats(gb, lengths, kv.get("sort_wave_max", 64), kv.get("sort_block_max", 2048),
                           kv.get("sort_method", 0))
    if config != "method1":
        assert all(got), got  # the shape reaches every class


def test_values_or_permutation_alone_match_both(gb):
    lengths = lengths_for(gb)
    model = ragged(lengths, 6000, "FP32", "alone")
    A = to_gb(gb, model)
    wc, wp = sm.sort_matrix(model, "gt")
    C, none = A.ss.sort(">", permutation=False)
    assert none is None
    check(C, wc, "FP32", what="values only")
    none, P = A.ss.sort(">", values=False)
    assert none is None
    check(P, wp, "UINT64", what="permutation only")


# ---------------------------------------------------------------------- row packing
@pytest.fixture(scope="module")
def packed_case():
    """140000 x 70, 133125 non-empty rows: runs of one-entry rows between stretches of
    alternating empty and 64-entry rows"""
    nrows, ncols = 140000, 70
    lens = np.ones(nrows, np.int64)
    pair = np.tile([0, 64], 625)  # 1250 rows
    for k in range(11):
        s = 3000 + k * 12000
        lens[s:s + pair.size] = pair
    assert (lens > 0).sum() == 133125
    rng = _rng("packed")
    p = rng.random((nrows, ncols)).argsort(axis=1).argsort(axis=1) < lens[:, None]
    v = np.where(p, rng.integers(-50, 50, p.shape, dtype=np.int32), np.int32(0))
    model = (p, v)
    return lens, model, {op: sm.sort_matrix(model, op) for op in OPS}


@pytest.mark.parametrize("config", ["default", "grid2", "method1"])
@pytest.mark.parametrize("op", OPS)
def test_row_packing(gb, packed_case, op, config):
    lens, model, want = packed_case
    A = to_gb(gb, model)
    with _knobs(gb, **CONFIGS[config]):
        C, P = sort_both(gb, A, op)
        expect_stats(gb, lens, 64, 2048, CONFIGS[config].get("sort_method", 0))
    check(C, want[op][0], "INT32", what=f"packed {op} {config} C")
    check(P, want[op][1], "UINT64", what=f"packed {op} {config} P")


@pytest.mark.parametrize("shape", [(1, 1), (0, 5), (5, 0), (9, 11)])
def test_degenerate_shapes(gb, shape):
    p = np.zeros(shape, bool)
    if shape == (1, 1):
        p[0, 0] = True
    model = (p, np.where(p, np.int16(-3), np.int16(0)))
    A = to_gb(gb, model)
    for op in OPS:
        for columnwise in (False, True):
            check_sorted(gb, A, model, op, "INT16", f"{shape} {op}", columnwise=columnwise)


# ---------------------------------------------------------------------- value pools
def pool(kind, dt):
    t = dm.NP[dt]
    f = np.finfo(t)

    def make(rng, shape):
        n = int(np.prod(shape))
        if kind == "three":
            v = rng.choice(np.array([-1.5, 0.0, 7.0], t), n)
        elif kind == "equal":
            v = np.full(n, 2.5, t)
        elif kind == "sorted":
            v = np.arange(n, dtype=t)
        elif kind == "reverse":
            v = -np.arange(n, dtype=t)
        elif kind == "zeros":  # +0.0 and -0.0 interleaved by column
            v = np.where(np.arange(n) % 2 == 0, t(0.0), t(-0.0))
        else:  # +-inf, denormals, min / max
            v = rng.choice(np.array([np.inf, -np.inf, f.smallest_subnormal, -f.smallest_subnormal, f.max, -f.max,
                                     f.smallest_normal, 0.0, -0.0, 1.0], t), n)
        return v.reshape(shape)

    return make


@pytest.mark.parametrize("kind", ["three", "equal", "sorted", "reverse", "zeros", "extremes"])
@pytest.mark.parametrize("dt", ["FP32", "FP64"])
def test_value_pools(gb, dt, kind):
    lengths = [6000, 0, 1, 2, 5, 33, 64, 65, 512, 513, 700, 2048, 2049, 3]
    model = ragged(lengths, 6000, dt, kind, vals=pool(kind, dt))
    A = to_gb(gb, model)
    for config in ("default", "lowered", "method1"):
        with _knobs(gb, **CONFIGS[config]):
            for op in OPS:
                check_sorted(gb, A, model, op, dt, f"{kind} {dt} {op} {config}")


def test_casts(gb):
    lengths = [0, 1, 2, 9, 40, 64, 65, 300, 2500]
    # INT8 values compared as FP64, into an INT32 C
    model = ragged(lengths, 3000, "INT8", "cast8")
    A = to_gb(gb, model)
    C, P = gb.Matrix("INT32", len(lengths), 3000), gb.Matrix("UINT64", len(lengths), 3000)
    assert gb.lib.GxB_Matrix_sort(C._h, P._h, gb.lib.GrB_LT_FP64, A._h, None) == 0
    wc, wp = sm.sort_matrix(model, "lt", "FP64", out_dtype="INT32")
    check(C, wc, "INT32", what="INT8 under LT_FP64 into INT32")
    check(P, wp, "UINT64", what="INT8 under LT_FP64 P")
    # UINT8 compared as INT8: values above 127 sort as negative; C keeps A's own values
    model = ragged(lengths, 3000, "UINT8", "castu8")
    check_sorted(gb, to_gb(gb, model), model, "gt", "UINT8", "UINT8 under GT_INT8", op_dtype="INT8")
    # an FP64 C for an INT64 A (values beyond 2^53 round in the cast, after the sort)
    model = ragged(lengths, 3000, "INT64", "cast64")
    A = to_gb(gb, model)
    C = gb.Matrix("FP64", len(lengths), 3000)
    assert gb.lib.GxB_Matrix_sort(C._h, None, gb.lib.GrB_GT_INT64, A._h, None) == 0
    wc, _ = sm.sort_matrix(model, "gt", out_dtype="FP64")
    check(C, wc, "FP64", what="INT64 into FP64")


@pytest.mark.parametrize("dt", ["FP32", "FP64"])
def test_nan_rows_are_permutations_with_the_rest_in_order(gb, dt):
    lengths = [0, 1, 2, 5, 33, 64, 65, 700, 2049, 6000]
    rng = _rng("nan", dt)
    p, v = ragged(lengths, 6000, dt, "nan")
    v = np.where(p & (rng.random(p.shape) < 0.2), dm.NP[dt](np.nan), v)
    v[3, np.nonzero(p[3])[0]] = np.nan  # a row of NaNs only
    A = to_gb(gb, (p, v))
    bits = {"FP32": np.uint32, "FP64": np.uint64}[dt]
    for config in ("default", "lowered", "method1"):
        with _knobs(gb, **CONFIGS[config]):
            for op in OPS:
                C, P = sort_both(gb, A, op)
                cr, cc, cv = C.to_coo()
                pr, pc, pv = P.to_coo()
                assert np.array_equal(cr, pr) and np.array_equal(cc, pc)
                cr, cc, pv = cr.astype(np.int64), cc.astype(np.int64), pv.astype(np.int64)
                for i, n in enumerate(lengths):
                    sel = cr == i
                    assert np.array_equal(cc[sel], np.arange(n)), (i, config)
                    cols = np.nonzero(p[i])[0]
                    assert np.array_equal(np.sort(pv[sel]), cols), "P's row is not a permutation of the columns"
                    assert np.array_equal(cv[sel].view(bits), v[i, pv[sel]].view(bits)), "C is not A at P"
                    ok = ~np.isnan(cv[sel])
                    want = sm.sort_vector((p[i] & ~np.isnan(v[i]), np.where(np.isnan(v[i]), 0, v[i])), op)
                    k = int(ok.sum())
                    assert np.array_equal(pv[sel][ok], want[1][1][:k].astype(np.int64)), "non-NaN entries out of order"


# ---------------------------------------------------------------------- iso, columnwise, aliasing
def is_iso(A):
    from graphblas_amd.device import matrix_view, vector_view

    return bool((vector_view if A.ndim == 1 else matrix_view)(A._h).iso)


def test_iso_input(gb):
    lengths = [0, 1, 2, 40, 65, 300, 2500]
    p, _ = ragged(lengths, 3000, "INT16", "iso")
    A, model = iso_gb(gb, p, -7, "INT16")
    assert is_iso(A)
    for op in OPS:
        for columnwise in (False, True):
            C, P = check_sorted(gb, A, model, op, "INT16", f"iso {op}", columnwise=columnwise)
            assert is_iso(C) and not is_iso(P)
    pv = np.zeros(70, bool)
    pv[[3, 9, 64, 69]] = True
    u, um = iso_gb(gb, pv, 2.5, "FP32")
    w, q = u.ss.sort(">")
    ww, wq = sm.sort_vector(um, "gt")
    check(w, ww, "FP32", what="iso vector w")
    check(q, wq, "UINT64", what="iso vector p")
    assert is_iso(w) and not is_iso(q)


@pytest.mark.parametrize("shape", [(37, 53), (300, 3), (3, 300)])
@pytest.mark.parametrize("dt", ["INT32", "FP64", "BOOL"])
def test_columnwise(gb, shape, dt):
    rng = _rng("col", shape, dt)
    p = rng.random(shape) < 0.6
    model = (p, np.where(p, values(dt, rng, p.size).reshape(shape), dm.NP[dt](0)))
    A = to_gb(gb, model)
    for op in OPS:
        C, P = check_sorted(gb, A, model, op, dt, f"columnwise {shape} {op}", columnwise=True)
        assert (C.nrows, C.ncols) == shape and (P.nrows, P.ncols) == shape
        check_sorted(gb, A, model, op, dt, f"rowwise {shape} {op}")


def test_columnwise_after_a_mutation(gb):
    rng = _rng("stale")
    p = rng.random((37, 53)) < 0.5
    p[5, 7] = False
    v = np.where(p, rng.integers(-9, 9, p.shape), 0).astype(np.int64)
    A = to_gb(gb, (p, v))
    check_sorted(gb, A, (p, v), "lt", "INT64", "before", columnwise=True)  # the CSC is cached now
    A[5, 7] = -100
    p[5, 7], v[5, 7] = True, -100
    C, P = check_sorted(gb, A, (p, v), "lt", "INT64", "after setElement", columnwise=True)
    assert C[0, 7].new().value == -100 and P[0, 7].new().value == 5
    # and a sorted matrix's own cached transpose does not survive being sorted into again
    B = C.T.new()
    assert gb.lib.GxB_Matrix_sort(C._h, None, gb.lib.GrB_GT_INT64, A._h, None) == 0
    check(C, sm.sort_matrix((p, v), "gt")[0], "INT64", what="C reused")
    check(C.T.new(), tuple(x.T for x in sm.sort_matrix((p, v), "gt")[0]), "INT64", what="C.T after reuse")
    assert B.nvals == C.nvals


def test_aliasing_and_prefilled_outputs(gb):
    lengths = [0, 1, 2, 9, 40, 64, 65, 300, 2500]
    model = ragged(lengths, 3000, "INT64", "alias")
    wc, wp = sm.sort_matrix(model, "gt")
    lib, GT = gb.lib, gb.lib.GrB_GT_INT64
    # C == A
    A = to_gb(gb, model)
    P = gb.Matrix("UINT64", *model[0].shape)
    assert lib.GxB_Matrix_sort(A._h, P._h, GT, A._h, None) == 0
    check(A, wc, "INT64", what="C == A")
    check(P, wp, "UINT64", what="P with C == A")
    # P == A (INT64 is a permitted permutation type)
    A = to_gb(gb, model)
    C = gb.Matrix("INT64", *model[0].shape)
    assert lib.GxB_Matrix_sort(C._h, A._h, GT, A._h, None) == 0
    check(C, wc, "INT64", what="C with P == A")
    check(A, (wp[0], wp[1].astype(np.int64)), "INT64", what="P == A")
    # C == A columnwise
    A = to_gb(gb, model)
    assert lib.GxB_Matrix_sort(A._h, None, GT, A._h, lib.GrB_DESC_T0) == 0
    check(A, sm.sort_matrix(model, "gt", columnwise=True)[0], "INT64", what="C == A, T0")
    # outputs that hold other entries (and an iso one) are replaced, not merged
    A = to_gb(gb, model)
    other = ragged([5] * len(lengths), 3000, "INT64", "other")
    C = to_gb(gb, other)
    P, _ = iso_gb(gb, other[0], 3, "UINT64")
    assert lib.GxB_Matrix_sort(C._h, P._h, GT, A._h, None) == 0
    check(C, wc, "INT64", what="prefilled C")
    check(P, wp, "UINT64", what="prefilled iso P")
    # vectors: w == u, p == u
    um = (model[0][7], model[1][7])
    ww, wq = sm.sort_vector(um, "lt")
    u = to_gb(gb, um)
    q = gb.Vector("UINT64", 3000)
    assert lib.GxB_Vector_sort(u._h, q._h, lib.GrB_LT_INT64, u._h, None) == 0
    check(u, ww, "INT64", what="w == u")
    check(q, wq, "UINT64", what="p with w == u")
    u = to_gb(gb, um)
    assert lib.GxB_Vector_sort(None, u._h, lib.GrB_LT_INT64, u._h, None) == 0
    check(u, (wq[0], wq[1].astype(np.int64)), "INT64", what="p == u")


# ---------------------------------------------------------------------- vectors
def check_tail(gb, w, want, what):
    n = w.size
    bits = np.zeros(((n + 63) // 64) * 64, bool)
    bits[:n] = want[0]
    packed = np.packbits(bits, bitorder="little").view(np.uint64) if n else np.zeros(0, np.uint64)
    assert np.array_equal(bitmap_words(gb, w), packed), f"{what}: bitmap words"


@pytest.mark.parametrize("fill", ["sparse", "full", "empty"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 70001, 262245])
def test_vectors(gb, n, fill):
    for dt in (["INT32", "FP64", "UINT8"] if n < 70001 else ["INT64", "FP32"]):
        rng = _rng("vec", n, fill, dt)
        p = {"sparse": rng.random(n) < 0.4, "full": np.ones(n, bool), "empty": np.zeros(n, bool)}[fill]
        um = (p, np.where(p, values(dt, rng, n), dm.NP[dt](0)))
        u = to_gb(gb, um)
        for op in OPS:
            w, q = u.ss.sort(op)
            ww, wq = sm.sort_vector(um, op)
            check(w, ww, dt, what=f"w {n} {fill} {dt} {op}")
            check(q, wq, "UINT64", what=f"p {n} {fill} {dt} {op}")
            check_tail(gb, w, ww, f"w {n} {fill}")
            check_tail(gb, q, wq, f"p {n} {fill}")
            # the device count is current: a later operation that trusts it sees the same entries
            assert w.dup().nvals == int(p.sum()) and q.dup().nvals == int(p.sum())


def test_vector_outputs_alone_and_casts(gb):
    rng = _rng("vec-cast")
    n = 300
    p = rng.random(n) < 0.5
    um = (p, np.where(p, values("INT8", rng, n), np.int8(0)))
    u = to_gb(gb, um)
    w, none = u.ss.sort("<", permutation=False)
    assert none is None
    check(w, sm.sort_vector(um, "lt")[0], "INT8", what="w alone")
    none, q = u.ss.sort(">", values=False)
    assert none is None
    check(q, sm.sort_vector(um, "gt")[1], "UINT64", what="p alone")
    w = gb.Vector("FP32", n)
    q = gb.Vector("INT64", n)
    assert gb.lib.GxB_Vector_sort(w._h, q._h, gb.lib.GrB_GT_UINT8, u._h, None) == 0
    ww, wq = sm.sort_vector(um, "gt", "UINT8", out_dtype="FP32")
    check(w, ww, "FP32", what="INT8 under GT_UINT8 into FP32")
    check(q, (wq[0], wq[1].astype(np.int64)), "INT64", what="INT64 p")


# ---------------------------------------------------------------------- top-k
def test_top_k_of_an_rmat(gb):
    import oracle as O

    G = O.rmat(10, 16, 5, values="FP64", value_seed=9)
    r, c, v = G.to_coo()
    A = gb.Matrix.from_coo(r, c, v, nrows=G.nrows, ncols=G.ncols)
    C, P = A.ss.sort(">")
    expect_stats(gb, np.diff(G.indptr), 64, 2048)
    r, c = np.asarray(r, np.int64), np.asarray(c, np.int64)
    order = np.lexsort((c, -v, r))  # per row: descending value, ties by ascending column
    rs, cs, vs = r[order], c[order], v[order]
    rank = np.arange(rs.size) - np.asarray(G.indptr, np.int64)[rs]
    for k in (1, 4, 64):
        Ck = C.select("col<=", k - 1).new()
        Pk = P.select("col<=", k - 1).new()
        keep = rank < k
        same_coo(Ck, (rs[keep], rank[keep]), vs[keep], "FP64", f"top-{k} values")
        same_coo(Pk, (rs[keep], rank[keep]), cs[keep], "UINT64", f"top-{k} columns")
