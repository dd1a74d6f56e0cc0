"""A numpy model of the dense import and export (GxB_{Matrix,Vector}_{import,export}_dense and the
front end's from_dense / to_dense) on dense_model's ``(present, values)`` pairs, written from the
rules the C header states, not from the kernels:

  import  position p holds an entry iff (no bitmap or bitmap[p] != 0) and (no missing value or
          X[p] != m), m the missing value cast to the array's type by the library's typecast
          (dense_model.cast), != C's: a NaN m drops nothing, m = 0.0 drops both zeros.  Values are
          kept bit for bit.
  export  the result type is `dtype` if given, else unify(fill type, object type) with the fill as
          the scalar when a fill is given, the object is not full and the caller upcasts (Matrix;
          a plain Vector.to_dense keeps its type), else the object's own; the object is cast to it
          (dense_model.cast), positions without an entry get the fill cast to it, or zero bytes
          when there is no fill but a bitmap is asked for; no fill, no bitmap and a missing entry
          is a TypeError.

golden() / golden_object() / golden_call() read tests/golden/dense_io_golden.json, the reference's
own cases."""
import json
import os

import numpy as np

import dense_model as dm

HERE = os.path.dirname(os.path.abspath(__file__))
PY_TYPES = {"int": "INT64", "float": "FP64"}


def golden():
    with open(os.path.join(HERE, "golden", "dense_io_golden.json")) as f:
        return json.load(f)["cases"]


def scalar_type(x):
    """the GraphBLAS type of a literal: its numpy type (a Python int is INT64, a float FP64)"""
    return dm.name_of(np.asarray(x).dtype)


def import_dense(X, missing=None, bitmap=None):
    """(present, values) of the dense array X (already of the object's type)"""
    X = np.asarray(X)
    present = np.ones(X.shape, bool)
    if bitmap is not None:
        bitmap = np.asarray(bitmap)
        assert bitmap.shape == X.shape
        present &= bitmap != 0
    if missing is not None:
        m = dm.cast(np.asarray(missing), dm.name_of(X.dtype))[()]
        with np.errstate(invalid="ignore"):
            present &= X != m
    return present, X.copy()


def result_type(obj_type, fill=None, dtype=None, *, full=False, upcast=True):
    if dtype is not None:
        return dtype
    if fill is not None and not full and upcast:
        return dm.name_of(np.result_type(np.array(0, dm.NP[scalar_type(fill)]), dm.NP[obj_type]))
    return obj_type


def export_dense(A, fill=None, dtype=None, *, upcast=True, bitmap=False):
    """-> (array, bitmap bytes): the dense array of A = (present, values)"""
    p, v = A
    full = bool(p.all())
    rt = result_type(dm.name_of(v.dtype), fill, dtype, full=full, upcast=upcast)
    if fill is None and not bitmap and not full:
        raise TypeError("fill_value must be given in `to_dense` when there are missing values")
    vals = dm.cast(v, rt)
    f = dm.NP[rt](0) if fill is None else dm.cast(np.asarray(fill), rt)[()]
    return np.where(p, vals, f).astype(dm.NP[rt]), p.astype(np.int8)


def bits(x):
    """an array viewed as unsigned integers of its item size: the bit-for-bit comparison"""
    x = np.ascontiguousarray(x)
    return x.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[x.dtype.itemsize])


# ---------------------------------------------------------------------- the golden cases
def _literal(x):
    """a recorded argument: {"scalar": x} is Scalar.from_value(x), {"type": "int"} the Python type"""
    if isinstance(x, dict) and "scalar" in x:
        return x["scalar"]
    if isinstance(x, dict) and "type" in x:
        return PY_TYPES[x["type"]]
    return x


def golden_object(desc):
    """the model pair of a recorded `from_dense(...)` / `from_coo(...)` object after its steps"""
    args, kw = desc["args"], desc["kwargs"]
    if desc["how"] == "from_dense":
        A = import_dense(np.asarray(args[0]), args[1] if len(args) > 1 else None)
    else:
        *idx, vals = args
        vals = np.asarray(vals)
        idx = [np.asarray(i, np.int64) for i in idx]
        shape = tuple(int(i.max()) + 1 for i in idx)
        if "size" in kw:
            shape = (kw["size"],)
        p, v = np.zeros(shape, bool), np.zeros(shape, vals.dtype)
        p[tuple(idx)] = True
        v[tuple(idx)] = vals
        A = (p, v)
    for step, arg in desc["steps"]:
        if step == "del":
            A[0][tuple(arg)] = False
            A[1][tuple(arg)] = 0
        else:
            A = dm.resize(A, tuple(arg))
    return A


def golden_call(case):
    """(fill, dtype) of a recorded to_dense call"""
    args = [_literal(a) for a in case["args"]]
    fill = args[0] if args else _literal(case["kwargs"].get("fill_value"))
    dtype = args[1] if len(args) > 1 else _literal(case["kwargs"].get("dtype"))
    return fill, dtype


def same_object(A, B):
    """isequal(check_dtype=True)"""
    return A[0].shape == B[0].shape and np.array_equal(A[0], B[0]) and A[1].dtype == B[1].dtype \
        and np.array_equal(A[1][A[0]], B[1][B[0]])
