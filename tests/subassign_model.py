"""numpy model of GxB_subassign and of GrB_Row_assign / GrB_Col_assign on (present, values) pairs,
the objects of tests/dense_model.py.  Two formulations of each, which the CPU tests hold against
each other and against the reference's own cases (tests/golden/subassign_golden.json):

composed   subassign = dm.extract, dm.write_back on the submatrix, stored back at np.ix_(I, J);
           row_assign = dm.assign_vec on row i (GrB_assign semantics on that one row).
direct     one loop over the positions of the region (or of the row) that applies the
           mask / replace / accum truth table of the SuiteSparse user guide (GxB_subassign) and of
           the C API 2.0 (4.3.7.3 / 4.3.7.4) position by position.

A is a model object of the region's shape, a numpy scalar (every position of the region), or None:
the empty scalar, an A without entries.  Index lists are duplicate-free; None is GrB_ALL."""
import json
import os

import numpy as np

import dense_model as dm

HERE = os.path.dirname(os.path.abspath(__file__))


def golden():
    with open(os.path.join(HERE, "golden", "subassign_golden.json")) as f:
        return json.load(f)


def _lists(C, I, J):
    cp = C[0]
    lists = [dm._index(I, cp.shape[0])] + ([dm._index(J, cp.shape[1])] if cp.ndim == 2 else [])
    assert all(np.unique(l).size == l.size for l in lists), "a repeated index is refused"
    return lists


def _region_A(A, shape, ct):
    """A as a (present, values) pair of the region's shape"""
    if A is None:
        return np.zeros(shape, bool), np.zeros(shape, dm.NP[ct])
    if dm.is_scalar(A):
        x = np.asarray(A)
        return np.ones(shape, bool), np.full(shape, x, x.dtype)
    assert A[0].shape == tuple(shape), "A must have the shape of the region"
    return A


# ---------------------------------------------------------------------- composed
def subassign(C, A, I=None, J=None, **kw):
    """C(I, J)<M, replace> = accum(C(I, J), A); M has the region's shape; for a vector J is None"""
    cp, cv = C[0].copy(), C[1].copy()
    ct = dm.name_of(cv.dtype)
    lists = _lists(C, I, J)
    sel = np.ix_(*lists)
    S = (cp[sel].copy(), cv[sel].copy())
    sp, sv = dm.write_back(S, _region_A(A, S[0].shape, ct), **kw)
    cp[sel], cv[sel] = sp, sv
    return cp, cv


def row_subassign(C, u, i, J=None, mask=None, **kw):
    m = None if mask is None else (mask[0][None, :], mask[1][None, :])
    A = u if u is None or dm.is_scalar(u) else (u[0][None, :], u[1][None, :])
    return subassign(C, A, [i], J, mask=m, **kw)


def col_subassign(C, u, I, j, mask=None, **kw):
    m = None if mask is None else (mask[0][:, None], mask[1][:, None])
    A = u if u is None or dm.is_scalar(u) else (u[0][:, None], u[1][:, None])
    return subassign(C, A, I, [j], mask=m, **kw)


def row_assign(C, u, i, J=None, **kw):
    """C(i, :)<mask, replace> = z, z(J) = accum(z(J), u): the mask has ncols entries"""
    cp, cv = C[0].copy(), C[1].copy()
    cp[i], cv[i] = dm.assign_vec((cp[i].copy(), cv[i].copy()), u, J, **kw)
    return cp, cv


def col_assign(C, u, I, j, **kw):
    cp, cv = C[0].copy(), C[1].copy()
    cp[:, j], cv[:, j] = dm.assign_vec((cp[:, j].copy(), cv[:, j].copy()), u, I, **kw)
    return cp, cv


# ---------------------------------------------------------------------- direct
def _one(x, t):
    return dm.cast(np.asarray(x).reshape(1), t)


def _z(c_has, c_val, a_has, a_val, ct, accum, adt):
    """Z at one position: (present, value of C's type)"""
    if accum is None:
        return (True, _one(a_val, ct)[0]) if a_has else (False, dm.NP[ct](0))
    if c_has and a_has:
        t = ct if adt is None else adt
        return True, dm.cast(dm.binop(accum, t, _one(c_val, t), _one(a_val, t)), ct)[0]
    if c_has:
        return True, c_val
    if a_has:
        return True, _one(a_val, ct)[0]
    return False, dm.NP[ct](0)


def _mask_at(mask, pos, comp, struct):
    if mask is None:
        m = True
    else:
        m = bool(mask[0][pos]) and (struct or bool(dm.cast(np.asarray(mask[1][pos]).reshape(1), "BOOL")[0]))
    return m != comp


def _a_at(A, pos):
    if A is None:
        return False, 0
    if dm.is_scalar(A):
        return True, np.asarray(A)
    return bool(A[0][pos]), A[1][pos]


def subassign_direct(C, A, I=None, J=None, mask=None, mask_comp=False, mask_struct=False, replace=False,
                     accum=None, accum_dtype=None):
    cp, cv = C[0].copy(), C[1].copy()
    ct = dm.name_of(cv.dtype)
    lists = _lists(C, I, J)
    for pos in np.ndindex(*[l.size for l in lists]):
        at = tuple(int(l[k]) for l, k in zip(lists, pos))
        c_has, c_val = bool(C[0][at]), C[1][at]
        if _mask_at(mask, pos, mask_comp, mask_struct):
            a_has, a_val = _a_at(A, pos)
            cp[at], cv[at] = _z(c_has, c_val, a_has, a_val, ct, accum, accum_dtype)
        elif replace:
            cp[at], cv[at] = False, 0
    return cp, cv


def line_assign_direct(C, u, index, L=None, col=False, mask=None, mask_comp=False, mask_struct=False,
                       replace=False, accum=None, accum_dtype=None):
    """GrB_Row_assign (col False: index is the row, L the columns) or GrB_Col_assign"""
    cp, cv = C[0].copy(), C[1].copy()
    ct = dm.name_of(cv.dtype)
    n = cp.shape[0] if col else cp.shape[1]
    L = dm._index(L, n)
    assert np.unique(L).size == L.size
    where = {int(c): k for k, c in enumerate(L)}
    for c in range(n):
        at = (c, index) if col else (index, c)
        c_has, c_val = bool(C[0][at]), C[1][at]
        if c in where:
            a_has, a_val = _a_at(u, where[c])
            z = _z(c_has, c_val, a_has, a_val, ct, accum, accum_dtype)
        else:
            z = (c_has, c_val)
        if _mask_at(mask, c, mask_comp, mask_struct):
            cp[at], cv[at] = z
        elif replace:
            cp[at], cv[at] = False, 0
    cv[~cp] = 0
    return cp, cv


# ---------------------------------------------------------------------- the golden steps
CHAINS = ["test_assign", "test_assign_row", "test_assign_column", "test_subassign_row_col", "test_subassign_matrix",
          "test_assign_row_col_matrix_mask", "test_vector_subassign"]
MASK_KINDS = {"S": (True, False), "V": (False, False), "CS": (True, True), "CV": (False, True)}  # struct, comp


def pair_of(o):
    """the model object of a recorded from_coo: BOOL for bool literals, else INT64"""
    vals = np.asarray(o["vals"])
    vals = vals.astype(np.bool_ if vals.dtype == np.bool_ else np.int64)
    if "rows" in o:
        return dm.to_dense((o["nrows"], o["ncols"]), (o["rows"], o["cols"]), vals)
    return dm.to_dense((o["size"],), (o["idx"],), vals)


def golden_objects(G, case):
    """name -> model object of a chain: its own from_coo objects, the fixtures, and mT = m.T.new()"""
    objs = {o["name"]: pair_of(o) for o in case["objects"]}
    for f in case["fixtures"]:
        objs[f] = pair_of(G["v"] if f == "v" else G["A"])
    if "m" in objs and objs["m"][0].ndim == 2:
        objs["mT"] = dm.transpose(objs["m"])
    return objs


def key_of(x):
    """an index of a step as the Python syntax takes it"""
    if isinstance(x, dict):
        return slice(*x["slice"])
    return slice(None) if x == "all" else x


def list_of(x, n):
    """the same index as the model's list (None: all)"""
    if isinstance(x, dict):
        return list(range(n))[slice(*x["slice"])]
    if x == "all":
        return None
    return [x] if isinstance(x, int) else list(x)


def value_of(step, objs):
    v = step["value"]
    if isinstance(v, dict):
        return np.int64(v["scalar"])
    return dm.transpose(objs[v[:-2]]) if v.endswith(".T") else objs[v]


def model_step(C, step, objs, direct=False):
    """the state after a (non-raising) step, by the composed or the direct formulation"""
    kw = {"accum": step["accum"], "replace": step["replace"]}
    mask = None
    if step["mask"] is not None:
        mask = objs[step["mask"]]
        kw["mask_struct"], kw["mask_comp"] = MASK_KINDS[step["mask_kind"]]
    A = value_of(step, objs)
    sub = subassign_direct if direct else subassign
    if C[0].ndim == 1:
        return sub(C, A, list_of(step["I"], C[0].shape[0]), None, mask=mask, **kw)
    I, J = list_of(step["I"], C[0].shape[0]), list_of(step["J"], C[0].shape[1])
    row, col = isinstance(step["I"], int), isinstance(step["J"], int)

    def as2d(x):  # a vector as the 1 x n or n x 1 object of the region
        if x is None or dm.is_scalar(x) or x[0].ndim == 2:
            return x
        return (x[0][None, :], x[1][None, :]) if row else (x[0][:, None], x[1][:, None])

    if mask is not None and mask[0].ndim == 2 and step["form"] == "assign":
        return dm.assign(C, as2d(A), I, J, mask=mask, **kw)  # a mask of C's shape: GrB_Matrix_assign
    if step["form"] == "subassign" or mask is None:
        return sub(C, as2d(A), I, J, mask=as2d(mask), **kw)
    if direct:
        return line_assign_direct(C, A, step["J"] if col else step["I"], I if col else J, col=col, mask=mask, **kw)
    return col_assign(C, A, I, step["J"], mask=mask, **kw) if col else row_assign(C, A, step["I"], J, mask=mask, **kw)


def combo_cases(G):
    """test_subassign_combos as (id, C, index, mask, mask kind, replace, value, expected): the four
    shapes times the eight parameter rows; index is slice(12) or list(range(12))"""
    g = G["test_subassign_combos"]
    base = {k: pair_of(g[k]) for k in ("mask", "val", "self")}
    n = g["n"]
    out = []
    for index in g["index"]:
        for shape in g["shapes"]:
            for p in g["params"]:
                want = dm.to_dense((g["self"]["size"],), (p["idx"],), np.asarray(p["vals"], np.int64))
                out.append({"id": f"{shape['shape']}-{index}-{p['mask_kind']}-{p['replace']}", "shape": shape["shape"],
                            "index": slice(n) if index == "slice" else list(range(n)), "mask_kind": p["mask_kind"],
                            "replace": p["replace"], "accum": g["accum"], "self": base["self"], "mask": base["mask"],
                            "val": base["val"], "want": want, "src": p["src"]})
    return out


def as_row(x):
    return x[0][None, :].copy(), x[1][None, :].copy()


def as_col(x):
    return x[0][:, None].copy(), x[1][:, None].copy()
