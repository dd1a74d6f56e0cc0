"""CPU checks of the subassign surface: the eight entry points are declared in both headers,
exported, typed in _lib and named in INTEGRATION.md; the two formulations of the numpy model the
GPU tests compare with (tests/subassign_model.py) reproduce the reference's own cases
(tests/golden/subassign_golden.json) and agree with each other on random small cases; and the front
end raises its TypeError / DimensionMismatch / NotImplementedError before any library call
(reference core/matrix.py:2905-3316).  No compute calls: objects are stubs without handles."""
import ctypes
import os
import re

import numpy as np
import pytest

import dense_model as dm
import subassign_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAT = "const GrB_Index *I, GrB_Index ni, const GrB_Index *J, GrB_Index nj, const GrB_Descriptor desc"
ROW = "const GrB_Vector u, GrB_Index i, const GrB_Index *J, GrB_Index nj, const GrB_Descriptor desc"
COL = "const GrB_Vector u, const GrB_Index *I, GrB_Index ni, GrB_Index j, const GrB_Descriptor desc"
ENTRY_POINTS = {
    "GxB_Matrix_subassign": f"GrB_Matrix C, const GrB_Matrix Mask, const GrB_BinaryOp accum, const GrB_Matrix A, {MAT}",
    "GxB_Vector_subassign": "GrB_Vector w, const GrB_Vector mask, const GrB_BinaryOp accum, const GrB_Vector u, "
                            "const GrB_Index *I, GrB_Index ni, const GrB_Descriptor desc",
    "GxB_Row_subassign": f"GrB_Matrix C, const GrB_Vector mask, const GrB_BinaryOp accum, {ROW}",
    "GxB_Col_subassign": f"GrB_Matrix C, const GrB_Vector mask, const GrB_BinaryOp accum, {COL}",
    "GrB_Row_assign": f"GrB_Matrix C, const GrB_Vector mask, const GrB_BinaryOp accum, {ROW}",
    "GrB_Col_assign": f"GrB_Matrix C, const GrB_Vector mask, const GrB_BinaryOp accum, {COL}",
    "GxB_Matrix_subassign_Scalar": f"GrB_Matrix C, const GrB_Matrix Mask, const GrB_BinaryOp accum, "
                                   f"const GrB_Scalar x, {MAT}",
    "GxB_Vector_subassign_Scalar": "GrB_Vector w, const GrB_Vector mask, const GrB_BinaryOp accum, "
                                   "const GrB_Scalar x, const GrB_Index *I, GrB_Index ni, const GrB_Descriptor desc",
}
G = sm.golden()


# ---------------------------------------------------------------------- the C ABI
def test_entry_points_are_exported_and_declared():
    import graphblas_amd
    from graphblas_amd import _lib

    dll = ctypes.CDLL(graphblas_amd.LIB_PATH)
    for path in ("graphblas_amd.h", "graphblas_amd_cdef.h"):
        text = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", path)).read())
        for name, args in ENTRY_POINTS.items():
            assert f"GrB_Info {name}({args});" in text, (path, name)
    P, I = ctypes.c_void_p, ctypes.c_uint64
    sigs = {"GxB_Matrix_subassign": [P, P, P, P, P, I, P, I, P], "GxB_Vector_subassign": [P, P, P, P, P, I, P],
            "GxB_Row_subassign": [P, P, P, P, I, P, I, P], "GxB_Col_subassign": [P, P, P, P, P, I, I, P],
            "GrB_Row_assign": [P, P, P, P, I, P, I, P], "GrB_Col_assign": [P, P, P, P, P, I, I, P],
            "GxB_Matrix_subassign_Scalar": [P, P, P, P, P, I, P, I, P],
            "GxB_Vector_subassign_Scalar": [P, P, P, P, P, I, P]}
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ENTRY_POINTS:
        assert hasattr(dll, name), name
        assert _lib._SIGS[name] == sigs[name], name
        assert name in dir(_lib.lib)
        assert name in text, name


def test_adapter_exposes_the_symbols():
    cdef = open(os.path.join(ROOT, "include", "graphblas_amd_cdef.h")).read()
    for name in ENTRY_POINTS:
        assert f"GrB_Info {name}(" in cdef


# ---------------------------------------------------------------------- the model and the golden steps
def same(got, want, what=""):
    assert got[0].shape == want[0].shape and np.array_equal(got[0], want[0]), what
    assert got[1].dtype == want[1].dtype and np.array_equal(np.where(got[0], got[1], 0), want[1]), what


@pytest.mark.parametrize("name", sm.CHAINS)
def test_both_formulations_reproduce_the_golden_chains(name):
    case = G[name]
    objs = sm.golden_objects(G, case)
    results = [sm.pair_of(r) for r in case["results"]]
    for direct in (False, True):
        state = {}
        done = 0
        for step in case["steps"]:
            base = objs[step["target"]]
            C = base if step["fresh"] or step["target"] not in state else state[step["target"]]
            if "raises" in step["expect"]:
                continue
            want = results[step["expect"]["result"]]
            if want[0].shape != C[0].shape:  # from_coo infers the shape from the largest index
                want = dm.resize(want, C[0].shape)
            got = sm.model_step(C, step, objs, direct)
            same(got, want, f"{step['src']} direct={direct}")
            state[step["target"]] = got
            done += 1
        assert done >= len(case["results"])


@pytest.mark.parametrize("case", sm.combo_cases(G), ids=lambda c: c["id"])
def test_both_formulations_reproduce_the_combos(case):
    struct, comp = sm.MASK_KINDS[case["mask_kind"]]
    kw = dict(accum=case["accum"], replace=case["replace"], mask_struct=struct, mask_comp=comp)
    I = list(range(12))
    for sub in (sm.subassign, sm.subassign_direct):
        if case["shape"] == "vector":
            got = sub(case["self"], case["val"], I, None, mask=case["mask"], **kw)
            same(got, case["want"], case["src"])
        elif case["shape"] in ("row", "matrix"):
            got = sub(sm.as_row(case["self"]), sm.as_row(case["val"]), [0], I, mask=sm.as_row(case["mask"]), **kw)
            same(got, sm.as_row(case["want"]), case["src"])
        else:
            got = sub(sm.as_col(case["self"]), sm.as_col(case["val"]), I, [0], mask=sm.as_col(case["mask"]), **kw)
            same(got, sm.as_col(case["want"]), case["src"])


def random_object(rng, shape, dt, density):
    p = rng.random(shape) < density
    if dt == "BOOL":
        v = rng.random(shape) < 0.5
    elif dm.is_int(dt):
        v = rng.integers(-5, 6, shape).astype(dm.NP[dt]) if dm.tmin(dt) < 0 else rng.integers(0, 6, shape).astype(dm.NP[dt])
    else:
        v = rng.choice(np.array([0.0, -0.0, 1.5, -2.5, np.inf, np.nan, 3.0]), shape).astype(dm.NP[dt])
    return p, np.where(p, v, dm.NP[dt](0))


def random_list(rng, n):
    kind = rng.choice(["all", "empty", "one", "perm", "subset"])
    if kind == "all":
        return None
    if kind == "empty" or n == 0:
        return []
    if kind == "one":
        return [int(rng.integers(0, n))]
    if kind == "perm":
        return rng.permutation(n).tolist()
    return rng.permutation(n)[:int(rng.integers(1, n + 1))].tolist()


def test_the_two_formulations_agree_on_random_cases():
    rng = np.random.default_rng(20240611)
    kinds = [None, "S", "V", "CS", "CV"]
    seen = set()
    for trial in range(400):
        nr, nc = int(rng.integers(1, 10)), int(rng.integers(1, 12))
        ct, at = rng.choice(["INT64", "FP64", "INT8", "BOOL", "FP32"]), rng.choice(["INT64", "FP64", "INT8", "BOOL"])
        C = random_object(rng, (nr, nc), ct, rng.choice([0.0, 0.4, 1.0]))
        I, J = random_list(rng, nr), random_list(rng, nc)
        ni, nj = (nr if I is None else len(I)), (nc if J is None else len(J))
        kind = kinds[trial % 5]
        replace = bool(rng.integers(0, 2)) and kind is not None
        accum = rng.choice([None, "plus", "min", "second"])
        adt = rng.choice([None, "FP64", "INT8"]) if accum is not None else None
        kw = dict(replace=replace, accum=accum, accum_dtype=adt)
        if kind is not None:
            kw["mask_struct"], kw["mask_comp"] = sm.MASK_KINDS[kind]
        seen.add((kind, replace, accum is not None))
        form = trial % 4
        if form == 0:  # matrix
            A = random_object(rng, (ni, nj), at, rng.choice([0.0, 0.5, 1.0]))
            M = None if kind is None else random_object(rng, (ni, nj), "INT8", rng.choice([0.0, 0.3, 1.0]))
            got, want = sm.subassign(C, A, I, J, mask=M, **kw), sm.subassign_direct(C, A, I, J, mask=M, **kw)
        elif form == 1:  # scalar, a value or the empty scalar
            A = None if rng.random() < 0.3 else dm.NP[at](3)
            M = None if kind is None else random_object(rng, (ni, nj), "INT8", rng.choice([0.0, 0.3, 1.0]))
            got, want = sm.subassign(C, A, I, J, mask=M, **kw), sm.subassign_direct(C, A, I, J, mask=M, **kw)
        elif form == 2:  # row assign: the mask spans the row
            i = int(rng.integers(0, nr))
            u = random_object(rng, (nj,), at, rng.choice([0.0, 0.5, 1.0]))
            m = None if kind is None else random_object(rng, (nc,), "INT8", rng.choice([0.0, 0.3, 1.0]))
            got = sm.row_assign(C, u, i, J, mask=m, **kw)
            want = sm.line_assign_direct(C, u, i, J, col=False, mask=m, **kw)
        else:  # column assign, and the vector subassign on column 0 alone
            j = int(rng.integers(0, nc))
            u = random_object(rng, (ni,), at, rng.choice([0.0, 0.5, 1.0]))
            m = None if kind is None else random_object(rng, (nr,), "INT8", rng.choice([0.0, 0.3, 1.0]))
            got = sm.col_assign(C, u, I, j, mask=m, **kw)
            want = sm.line_assign_direct(C, u, j, I, col=True, mask=m, **kw)
            w = (C[0][:, 0].copy(), C[1][:, 0].copy())
            ms = None if kind is None else random_object(rng, (ni,), "INT8", 0.5)
            a, b = sm.subassign(w, u, I, None, mask=ms, **kw), sm.subassign_direct(w, u, I, None, mask=ms, **kw)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1], equal_nan=True), trial
        assert got[1].dtype == want[1].dtype == C[1].dtype
        assert np.array_equal(got[0], want[0]), trial
        assert np.array_equal(np.where(got[0], got[1], 0), np.where(want[0], want[1], 0), equal_nan=True), trial
    assert len(seen) >= 14  # every mask kind with and without replace and accum


def test_model_hand_worked_cases():
    t, f = True, False
    C = (np.array([[t, t, f], [f, t, t]]), np.array([[1, 2, 0], [0, 5, 6]], np.int64))
    A = (np.array([[t, f]]), np.array([[10, 0]], np.int64))
    # no mask, no accum: the region becomes A, entries A lacks are deleted, nothing else moves
    p, v = sm.subassign(C, A, [1], [2, 1])
    assert p.tolist() == [[t, t, f], [f, f, t]] and v.tolist() == [[1, 2, 0], [0, 0, 10]]
    # replace outside the region: a subassign leaves row 0, a row assign with the mask over the row deletes (1, 1)
    m = (np.array([t, f]), np.array([1, 0], np.int8))
    u = (np.array([t, t]), np.array([7, 8], np.int64))
    p, v = sm.row_subassign(C, u, 1, [2, 0], mask=m, mask_struct=True, replace=True)
    assert p.tolist() == [[t, t, f], [f, t, t]] and v[1].tolist() == [0, 5, 7]
    m3 = (np.array([t, f, t]), np.array([1, 0, 1], np.int8))
    p, v = sm.row_assign(C, u, 1, [2, 0], mask=m3, mask_struct=True, replace=True)
    assert p[1].tolist() == [t, f, t] and v[1].tolist() == [8, 0, 7] and p[0].tolist() == [t, t, f]
    d = sm.line_assign_direct(C, u, 1, [2, 0], mask=m3, mask_struct=True, replace=True)
    assert np.array_equal(d[0], p) and np.array_equal(d[1], v)


# ---------------------------------------------------------------------- the front end, before any call
def stub(kind, shape, dt="INT64"):
    import graphblas_amd as gb

    if kind == "v":
        v = gb.Vector.__new__(gb.Vector)
        v.dtype, v.name, v._size, v._h = gb.dtypes.lookup_dtype(dt), "v", shape, None
        return v
    A = gb.Matrix.__new__(gb.Matrix)
    A.dtype, A.name, A._nrows, A._ncols, A._h = gb.dtypes.lookup_dtype(dt), "A", shape[0], shape[1], None
    return A


def test_argument_errors_are_raised_before_any_call():
    import graphblas_amd as gb
    from graphblas_amd.exceptions import DimensionMismatch

    C, B, M22, A22 = stub("A", (3, 3)), stub("A", (2, 2)), stub("A", (2, 1)), stub("A", (2, 2))
    v2, v3, m2 = stub("v", 2), stub("v", 3), stub("v", 2)
    vec_submask = "Indices for subassign imply Vector submask, but got Matrix mask instead"
    for value in (v3, 100):
        with pytest.raises(TypeError, match=vec_submask):
            C[0, :](C.S) << value
        with pytest.raises(TypeError, match=vec_submask):
            C[:, 0](C.S) << value
    with pytest.raises(TypeError, match="Unable to use Vector mask on Matrix assignment to a Matrix"):
        C[:, :](v3.S) << 1
    with pytest.raises(TypeError, match="Unable to use Vector mask on Matrix assignment to a Matrix"):
        C[[0, 1], [0, 1]](v2.S) << B
    with pytest.raises(TypeError, match="Unable to use Vector mask on Matrix assignment to a Matrix"):
        C(v3.S)[[0, 1], [0, 1]] << B
    with pytest.raises(TypeError, match="Unable to use Vector mask on single element assignment to a Matrix"):
        C[0, 0](v3.S) << 1
    with pytest.raises(TypeError, match="Single element assign does not accept a submask"):
        C[0, 0](C.S) << 100
    with pytest.raises(TypeError, match="Single element assign does not accept a submask"):
        v3[0](v3.S) << 1
    v3[0](v3.S, replace=True)  # building it is allowed, as in the reference
    for bad in (C, C.T):
        with pytest.raises(TypeError, match="Bad type for argument `value`"):
            C[0, :] = bad
        with pytest.raises(TypeError, match="Bad type for argument `value`"):
            C[0, [0, 1]](v2.S) << bad
    with pytest.raises(TypeError, match="Bad type for argument `value`"):
        C[[0, 1], [0, 1]] = v2
    with pytest.raises(TypeError, match="Bad type for argument `value`"):
        C[[0, 1], [0, 1]](B.S) << v2
    with pytest.raises(TypeError, match="Mask object must be type Vector"):
        v3[[0, 1]](C.S) << 88
    with pytest.raises(TypeError, match="Mask object must be type Vector"):
        v3[[0, 1]](C.S) << v2
    # shapes
    with pytest.raises(DimensionMismatch):
        C[[0, 1, 2], [0, 1]] = B
    with pytest.raises(DimensionMismatch):
        C[[0, 1], [0, 1]](M22.S) << B
    with pytest.raises(DimensionMismatch):
        C[[0, 1], [0, 1]](B.S) << C
    with pytest.raises(DimensionMismatch):
        C[0, [0, 1]] = v3
    with pytest.raises(DimensionMismatch):
        C[[0, 1], 0](m2.S) << v3
    with pytest.raises(DimensionMismatch):
        C(m2.S)[[0, 1], 0] << v2  # the mask of an assign spans the whole column
    with pytest.raises(DimensionMismatch):
        C(M22.S)[[0, 1], [0]] << M22  # reference test_subassign_matrix
    with pytest.raises(DimensionMismatch):
        C(M22.S)[0, [0, 1]] << v2
    with pytest.raises(DimensionMismatch):
        v3[[0, 1]](v3.S) << v2
    with pytest.raises(DimensionMismatch):
        v3[[0, 1]](m2.S) << v3
    with pytest.raises(DimensionMismatch):
        v3[[0, 1]](v3.S) << 99
    # a Matrix mask of C's shape with index lists is the one form left out
    with pytest.raises(NotImplementedError, match="GrB_Matrix_assign with index lists"):
        C(C.S)[[0, 1], [0, 1]] << A22
    with pytest.raises(NotImplementedError, match="GrB_Matrix_assign with index lists"):
        C(C.S)[0, :] << v3
    with pytest.raises(NotImplementedError, match="GrB_Matrix_assign with index lists"):
        C(C.S, accum=gb.binary.plus)[:, 1] = v3
    with pytest.raises(TypeError, match="is not an assignment target"):
        C.mxm(C) << C


@pytest.mark.parametrize("name", sm.CHAINS)
def test_golden_steps_that_raise_do_so_without_a_library_call(name):
    """the steps of the reference's tests that end in pytest.raises, and those that need the refused
    GrB_Matrix_assign, on stubs of the recorded shapes"""
    from graphblas_amd.exceptions import DimensionMismatch

    import graphblas_amd as gb

    case = G[name]
    objs = sm.golden_objects(G, case)

    def st(x):
        return stub("v", x[0].shape[0], dm.name_of(x[1].dtype)) if x[0].ndim == 1 else \
            stub("A", x[0].shape, dm.name_of(x[1].dtype))

    stubs = {k: st(x) for k, x in objs.items()}
    exc = {"DimensionMismatch": DimensionMismatch, "TypeError": TypeError}
    for step in case["steps"]:
        if "raises" in step["expect"]:
            err, match = exc[step["expect"]["raises"]], step["expect"]["match"]
        elif step.get("needs_matrix_assign"):
            err, match = NotImplementedError, "GrB_Matrix_assign with index lists"
        else:
            continue
        with pytest.raises(err, match=match):
            apply_step(gb, stubs[step["target"]], step, stubs)


def apply_step(gb, C, step, objs):
    """a golden step through the Python syntax (the GPU tests use it too)"""
    v = step["value"]
    value = v["scalar"] if isinstance(v, dict) else (objs[v[:-2]].T if v.endswith(".T") else objs[v])
    keys = sm.key_of(step["I"]) if step["J"] is None else (sm.key_of(step["I"]), sm.key_of(step["J"]))
    args = []
    if step["mask"] is not None:
        m = objs[step["mask"]]
        args.append({"S": m.S, "V": m.V, "CS": ~m.S, "CV": ~m.V}[step["mask_kind"]])
    kw = {"replace": step["replace"]}
    if step["accum"] is not None:
        kw["accum"] = getattr(gb.binary, step["accum"])
    if step["form"] == "assign":
        C(*args, **kw)[keys] << value
    else:
        C[keys](*args, **kw) << value
