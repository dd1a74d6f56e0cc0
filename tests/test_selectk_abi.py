"""CPU checks of the selectk / compactify surface: the entry points are exported, declared in both
headers and typed in _lib; ``ss.selectk`` / ``ss.compactify`` have the reference's argument order
(core/ss/matrix.py:3815, 3877, core/ss/vector.py:1407, 1456) and its ValueError texts; the numpy
model the GPU tests compare with (tests/selectk_model.py) reproduces every case of the reference's
own tests (tests/golden/selectk_golden.json), agrees with itself between selectk and compactify,
and its random order is uniform.  No compute calls (no GPU here)."""
import ctypes
import inspect
import json
import os

import numpy as np
import pytest

import dense_model as dm
import selectk_model as km

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, E, I, U, B = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_bool
ENTRY_POINTS = {
    "GxB_Matrix_selectk": ("GrB_Info GxB_Matrix_selectk(GrB_Matrix C, const GrB_Matrix A, int how, GrB_Index k,\n"
                           "                            uint64_t seed, const GrB_Descriptor desc);", [P, P, E, I, U, P]),
    "GxB_Vector_selectk": ("GrB_Info GxB_Vector_selectk(GrB_Vector w, const GrB_Vector u, int how, GrB_Index k,\n"
                           "                            uint64_t seed, const GrB_Descriptor desc);", [P, P, E, I, U, P]),
    "GxB_Matrix_compactify": ("GrB_Info GxB_Matrix_compactify(GrB_Matrix C, const GrB_Matrix A, int how, GrB_Index k,\n"
                              "                               bool reverse, bool asindex, uint64_t seed,\n"
                              "                               const GrB_Descriptor desc);", [P, P, E, I, B, B, U, P]),
    "GxB_Vector_compactify": ("GrB_Info GxB_Vector_compactify(GrB_Vector w, const GrB_Vector u, int how, GrB_Index k,\n"
                              "                               bool reverse, bool asindex, uint64_t seed,\n"
                              "                               const GrB_Descriptor desc);", [P, P, E, I, B, B, U, P]),
    "GxB_Matrix_compactify_width": ("GrB_Info GxB_Matrix_compactify_width(GrB_Index *k, const GrB_Matrix A, "
                                    "const GrB_Descriptor desc);", [P, P, P]),
}
ENUM = ("typedef enum { GxB_SELECTK_FIRST, GxB_SELECTK_LAST, GxB_SELECTK_SMALLEST,\n"
        "               GxB_SELECTK_LARGEST, GxB_SELECTK_RANDOM } GxB_SelectK_How;")


def golden():
    with open(os.path.join(ROOT, "tests", "golden", "selectk_golden.json")) as f:
        return json.load(f)


def golden_input(g, name):
    """(model pair, iso) of the golden input ``name``: A, A_iso, v, v_iso, vc, vc_iso"""
    base, iso = (name[:-4], True) if name.endswith("_iso") else (name, False)
    a = g[base]
    t = dm.NP[a["dtype"]]
    if base == "A":
        idx, shape = (np.asarray(a["rows"]), np.asarray(a["cols"])), (a["nrows"], a["ncols"])
    else:
        idx, shape = (np.asarray(a["idx"]),), (a["size"],)
    p = np.zeros(shape, bool)
    v = np.zeros(shape, t)
    p[idx] = True
    v[idx] = 1 if iso else a["vals"]
    return (p, v), iso


def accepted(g, case, got):
    """whether the COO result ``got`` is one of the case's accepted results"""
    shape, idx, vals = got
    for acc in case["accept"]:
        if acc == "input":
            (p, v), _ = golden_input(g, case["input"])
            widx = np.nonzero(p)
            wv = v[widx]
        elif "rows" in acc:
            widx = (np.asarray(acc["rows"], np.int64), np.asarray(acc["cols"], np.int64))
            wv = np.asarray(acc["vals"])
        else:
            widx = (np.asarray(acc["idx"], np.int64),)
            wv = np.asarray(acc["vals"])
        o = np.lexsort(widx[::-1]) if wv.size else np.zeros(0, np.int64)
        if wv.size == vals.size and all(np.array_equal(a, b[o]) for a, b in zip(idx, widx)) \
                and np.array_equal(vals.astype(np.int64), wv[o].astype(np.int64)):
            return True
    return False


def model_of(g, case, seed=0):
    A, iso = golden_input(g, case["input"])
    vector = A[0].ndim == 1
    if case["op"] == "selectk":
        if vector:
            return km.selectk_vector(A, case["how"], case["k"], seed=seed, iso=iso)
        return km.selectk(A, case["how"], case["k"], columnwise=case["order"] == "columnwise", seed=seed, iso=iso)
    kw = dict(reverse=case["reverse"], asindex=case["asindex"], seed=seed, iso=iso)
    if vector:
        return km.compactify_vector(A, case["how"], case["k"], **kw)
    return km.compactify(A, case["how"], case["k"], columnwise=case["order"] == "columnwise", **kw)


def case_id(c):
    return "-".join(str(c.get(k)) for k in ("input", "op", "how", "k", "order", "reverse", "asindex"))


def test_entry_points_are_exported_and_declared():
    import graphblas_amd
    from graphblas_amd import _lib

    dll = ctypes.CDLL(graphblas_amd.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "graphblas_amd.h")).read()
    cdef = open(os.path.join(ROOT, "include", "graphblas_amd_cdef.h")).read()
    assert ENUM in header and ENUM in cdef
    for n, (decl, sig) in ENTRY_POINTS.items():
        getattr(dll, n)  # AttributeError: not exported
        assert decl in header, n
        assert decl in cdef, n
        assert _lib._SIGS[n] == sig, n
        assert n in dir(_lib.lib)
    for i, n in enumerate(("FIRST", "LAST", "SMALLEST", "LARGEST", "RANDOM")):
        assert getattr(_lib.lib, f"GxB_SELECTK_{n}") == i


def test_front_end_signatures_and_error_texts():
    import graphblas_amd as gb
    from graphblas_amd.ss import MatrixSS, VectorSS

    KW = inspect.Parameter.KEYWORD_ONLY
    ps = inspect.signature(MatrixSS.selectk).parameters
    assert list(ps) == ["self", "how", "k", "order", "seed", "name"]
    assert ps["order"].default == "rowwise" and ps["seed"].kind is KW and ps["seed"].default is None
    ps = inspect.signature(MatrixSS.compactify).parameters
    assert list(ps) == ["self", "how", "k", "order", "reverse", "asindex", "seed", "name"]
    assert (ps["how"].default, ps["k"].default, ps["order"].default) == ("first", None, "rowwise")
    assert ps["reverse"].kind is KW and ps["reverse"].default is False and ps["asindex"].default is False
    ps = inspect.signature(VectorSS.selectk).parameters
    assert list(ps) == ["self", "how", "k", "seed", "name"] and ps["seed"].kind is KW
    ps = inspect.signature(VectorSS.compactify).parameters
    assert list(ps) == ["self", "how", "size", "reverse", "asindex", "seed", "name"]
    assert (ps["how"].default, ps["size"].default) == ("first", None) and ps["reverse"].kind is KW
    # the argument checks come before any library call: no GPU is needed to see them
    A, v = gb.Matrix.__new__(gb.Matrix), gb.Vector.__new__(gb.Vector)
    for obj in (A, v):
        with pytest.raises(ValueError, match="`how` argument must be one of: "):
            obj.ss.selectk("bad", 1)
        with pytest.raises(ValueError, match='`how` argument must be one of: "first", "last", "smallest", "largest", '
                                             '"random"'):
            obj.ss.compactify("bad_how")
        with pytest.raises(ValueError, match="negative k is not allowed"):
            obj.ss.selectk("first", -1)
    with pytest.raises(ValueError, match="negative k is not allowed"):
        A.ss.selectk("random", -1, order="columnwise")
    with pytest.raises(ValueError, match="`how` argument must be one of:"):
        A.ss.selectk("bad", 1, order="col")


@pytest.mark.parametrize("case", golden()["matrix_cases"] + golden()["vector_cases"], ids=case_id)
def test_model_reproduces_the_golden_cases(case):
    g = golden()
    if "count_range" in case:  # the reference's random test: entries per row (column)
        lo, hi = case["count_range"]
        (p, _), _ = golden_input(g, case["input"])
        for seed in range(20):
            shape, idx, _ = model_of(g, case, seed)
            axis = 1 if case["order"] == "columnwise" else 0
            counts = np.bincount(idx[axis], minlength=shape[axis])
            assert counts.min() == lo and counts.max() == hi and p[idx].all()
        return
    assert accepted(g, case, model_of(g, case)), case


def ragged_model(nrows, ncols, dt, seed, ties=False):
    rng = np.random.default_rng(seed)
    p = rng.random((nrows, ncols)) < rng.random((nrows, 1))
    p[0] = False
    v = rng.integers(0, 4 if ties else 1000, p.shape).astype(dm.NP[dt])
    return p, np.where(p, v, dm.NP[dt](0))


@pytest.mark.parametrize("how", km.HOWS)
@pytest.mark.parametrize("columnwise", [False, True])
def test_model_selectk_keeps_what_compactify_lists(how, columnwise):
    A = ragged_model(23, 17, "INT32", 5, ties=True)
    for k in (0, 1, 2, 5, 40):
        shape, (r, c), x = km.selectk(A, how, k, columnwise=columnwise, seed=11)
        assert shape == A[0].shape and A[0][r, c].all() and np.array_equal(x, A[1][r, c])
        _, (cr, cc), ci = km.compactify(A, how, k, columnwise=columnwise, asindex=True, seed=11)
        _, _, cv = km.compactify(A, how, k, columnwise=columnwise, seed=11)
        # compactify's indices name the kept entries (row, index) or (index, column); its values are theirs
        kept = set(zip(r.tolist(), c.tolist()))
        named = zip(ci.tolist(), cc.tolist()) if columnwise else zip(cr.tolist(), ci.tolist())
        named = list(named)
        assert len(named) == len(kept) and set(named) == kept
        assert np.array_equal(cv, A[1][tuple(np.asarray(named, np.int64).reshape(-1, 2).T)])
        # and under reverse every row comes out backwards
        if how != "random":
            _, (rr, rc), ri = km.compactify(A, how, k, columnwise=columnwise, asindex=True, reverse=True, seed=11)
            line, slot, rline, rslot = (cc, cr, rc, rr) if columnwise else (cr, cc, rr, rc)
            m = np.bincount(line, minlength=max(A[0].shape))[line]
            fwd = dict(zip(zip(line.tolist(), slot.tolist()), ci.tolist()))
            bwd = dict(zip(zip(rline.tolist(), rslot.tolist()), ri.tolist()))
            assert all(bwd[(i, int(mm) - 1 - t)] == x_ for ((i, t), x_), mm in zip(fwd.items(), m))


def test_model_orders_by_hand():
    # row 0: values 3 3 1 3 at columns 1 2 4 6; -0.0 ties with +0.0 in row 1
    p = np.zeros((2, 8), bool)
    v = np.zeros((2, 8))
    p[0, [1, 2, 4, 6]] = True
    v[0, [1, 2, 4, 6]] = [3, 3, 1, 3]
    p[1, [0, 3, 5]] = True
    v[1, [0, 3, 5]] = [0.0, -0.0, -1.0]
    A = (p, v)
    _, (r, c), x = km.compactify(A, "smallest", asindex=True)
    assert c.tolist() == [0, 1, 2, 3, 0, 1, 2] and x.tolist() == [4, 1, 2, 6, 5, 0, 3] and x.dtype == np.uint64
    _, _, x = km.compactify(A, "largest", asindex=True)  # the value order reversed: ties in descending position
    assert x.tolist() == [6, 2, 1, 4, 3, 0, 5]
    _, _, x = km.compactify(A, "largest", 2, asindex=True, reverse=True)
    assert x.tolist() == [2, 6, 0, 3]
    _, (r, c), x = km.selectk(A, "largest", 2)
    assert c.tolist() == [2, 6, 0, 3] and np.signbit(x[3])
    _, (r, c), _ = km.selectk(A, "smallest", 2)
    assert c.tolist() == [1, 4, 0, 5]
    _, (r, c), _ = km.selectk(A, "last", 1)
    assert c.tolist() == [6, 5]
    # iso: smallest and largest are first
    for how in ("smallest", "largest"):
        _, (r, c), _ = km.selectk(A, how, 1, iso=True)
        assert c.tolist() == [1, 0]
        _, _, x = km.compactify(A, how, 2, asindex=True, reverse=True, iso=True)
        assert x.tolist() == [1, 2, 0, 3]
    u = (p[0], v[0])
    assert km.compactify_vector(u, "last", 3, asindex=True)[2].tolist() == [6, 4, 2]
    assert km.compactify_vector((np.zeros(5, bool), np.zeros(5)), "first")[0] == (0,)


def test_hash_is_the_documented_one():
    # splitmix64's finaliser of 1 and of 0, and the composition of include/graphblas_amd.h's order
    assert int(km.mix64(0)) == 0
    assert int(km.mix64(1)) == 0x5692161D100B05E5
    g = 0x9E3779B97F4A7C15
    want = int(km.mix64((int(km.mix64((7 + g * 4) & km.M64)) + g * 10) & km.M64))
    assert int(km.hash3(7, 3, 9)) == want
    assert km.hash3(2 ** 64 - 1, np.arange(5), 2 ** 40).dtype == np.uint64


@pytest.mark.parametrize("seed", [0, 1, 0xDEADBEEFCAFEF00D])
def test_random_order_is_uniform(seed):
    """20 000 rows of 10 entries, k = 3: each position is kept Binomial(20000, 0.3) times, and
    5 standard deviations of that are 5 sqrt(20000 0.3 0.7) = 324"""
    n, d, k = 20000, 10, 3
    A = (np.ones((n, d), bool), np.ones((n, d), np.int8))
    _, (r, c), _ = km.selectk(A, "random", k, seed=seed)
    assert np.array_equal(np.bincount(r, minlength=n), np.full(n, k))
    counts = np.bincount(c, minlength=d)
    bound = 5 * np.sqrt(n * 0.3 * 0.7)
    print(f"seed {seed:#x}: inclusion counts {counts.tolist()}, bound 6000 +- {bound:.0f}")
    assert (np.abs(counts - n * k / d) <= bound).all(), counts
    _, (r2, c2), _ = km.selectk(A, "random", k, seed=seed + 1)
    assert not np.array_equal(c, c2)
