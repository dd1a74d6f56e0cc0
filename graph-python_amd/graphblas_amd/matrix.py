"""Matrix collection and its delayed expressions (mirrors the hot-path parts of
reference core/matrix.py: new/free :178-213, build :643-697, from_coo
:885-960, to_coo :543-611, _from_csx :1057-1133, _to_csx :1658-1702,
isequal :357-398, mxv :2163-2204, mxm :2206-2251, power :2754-2806,
MatrixExpression :3371-3412, TransposedMatrix :3614-3778)."""
import ctypes

import numpy as np

from . import operator as _op
from ._lib import lib
from .base import (BaseExpression, BaseType, ComplementedStructuralMask, StructuralMask, ValueMask,
                   _autoname, _check_mask, _Pointer, call, descriptor_lookup)
from .dtypes import BOOL, FP64, INT64, UINT64, lookup_dtype, unify
from .exceptions import DimensionMismatch, NoValue, check_status_carg


class _CArray:
    __slots__ = "array", "name"

    def __init__(self, array, name="array"):
        self.array = np.ascontiguousarray(array)
        self.name = name

    @property
    def _carg(self):
        return ctypes.c_void_p(self.array.ctypes.data)


def _values_dtype(values, dtype):
    if dtype is not None:
        return lookup_dtype(dtype)
    a = np.asarray(values)
    if a.dtype == object:  # reference core/utils.py values_to_numpy_buffer
        raise ValueError("object dtype for values is not allowed")
    if a.dtype == np.bool_:
        return lookup_dtype(BOOL)
    if np.issubdtype(a.dtype, np.integer) or np.issubdtype(a.dtype, np.floating):
        return lookup_dtype(a.dtype)
    raise TypeError(f"Cannot infer a GraphBLAS dtype from {a.dtype}")


def _index_array(x, name):
    a = np.asarray(x)
    if a.size and not (np.issubdtype(a.dtype, np.integer) or a.dtype == np.bool_):
        raise ValueError(f"{name} must be integers, not {a.dtype.name}")
    if a.size and a.min() < 0:
        raise ValueError(f"{name} must be non-negative")
    return np.ascontiguousarray(a, np.uint64)


class Matrix(BaseType):
    ndim = 2

    def __init__(self, dtype=FP64, nrows=0, ncols=0, *, name=None):
        self.dtype = lookup_dtype(dtype)
        self.name = _autoname("M") if name is None else name
        self._h = ctypes.c_void_p()
        self._nrows = int(nrows)
        self._ncols = int(ncols)
        call("GrB_Matrix_new", [_Pointer(self), self.dtype, self._nrows, self._ncols])

    def __del__(self):
        h = getattr(self, "_h", None)
        if getattr(self, "_parent", None) is not None:
            return  # a cast view (Vector._as_matrix) does not own the handle
        if h is not None and h.value:
            try:
                lib.GrB_Matrix_free(ctypes.byref(h))
            except Exception:
                pass

    # ---------------------------------------------------------------- properties
    @property
    def nrows(self):
        return self._nrows

    @property
    def ncols(self):
        return self._ncols

    @property
    def shape(self):
        return (self._nrows, self._ncols)

    @property
    def nvals(self):
        n = ctypes.c_uint64()
        check_status_carg(lib.GrB_Matrix_nvals(ctypes.byref(n), self._h), "Matrix", self._h)
        return n.value

    _nvals = nvals

    @property
    def T(self):
        return TransposedMatrix(self)

    @property
    def ss(self):
        from .ss import MatrixSS

        return MatrixSS(self)

    @property
    def S(self):
        return StructuralMask(self)

    @property
    def V(self):
        return ValueMask(self)

    def __repr__(self):
        return f"<Matrix {self.name}: {self._nrows}x{self._ncols}, nvals={self.nvals}, {self.dtype}>"

    # ---------------------------------------------------------------- construction
    @classmethod
    def from_coo(cls, rows, columns, values=1.0, dtype=None, *, nrows=None, ncols=None, dup_op=None,
                 name=None):
        from . import sparse

        if sparse.any_device(rows, columns, values):  # device arrays never leave the device
            return sparse.matrix_from_coo(cls, rows, columns, values, dtype, nrows, ncols, dup_op, name)
        rows = _index_array(rows, "row indices")
        columns = _index_array(columns, "column indices")
        if nrows is None:
            nrows = int(rows.max()) + 1 if rows.size else 0
        if ncols is None:
            ncols = int(columns.max()) + 1 if columns.size else 0
        if np.ndim(values) == 0 and not isinstance(values, np.ndarray):
            if dup_op is not None:  # reference core/matrix.py:947-951
                raise ValueError("dup_op must be None if values is a scalar so that all "
                                 "values can be identical.  Duplicate indices will be ignored.")
            dt = _values_dtype(values, dtype)
            C = cls(dt, nrows, ncols, name=name)
            n = rows.size
            if rows.size != columns.size:
                raise ValueError("`rows` and `columns` lengths must match")
            if n:
                x = np.asarray(values, dt.np_type).item()
                call(f"GxB_Matrix_build_Scalar_{dt.name}",
                     [C, _CArray(rows, "rows"), _CArray(columns, "cols"), x, n])
            return C
        vals = np.asarray(values)
        dt = _values_dtype(vals, dtype)
        C = cls(dt, nrows, ncols, name=name)
        C.build(rows, columns, vals, dup_op=dup_op)
        return C

    def build(self, rows, columns, values, *, dup_op=None, clear=False, nrows=None, ncols=None):
        from . import sparse

        if sparse.any_device(rows, columns, values):
            nr, nc = self._nrows if nrows is None else int(nrows), self._ncols if ncols is None else int(ncols)
            sparse.matrix_from_coo(Matrix, rows, columns, values, self.dtype, nr, nc, dup_op, None, "build",
                                   into=self, clear=clear)
            return
        rows = _index_array(rows, "row indices")
        columns = _index_array(columns, "column indices")
        values = np.ascontiguousarray(np.broadcast_to(np.asarray(values, self.dtype.np_type), rows.shape))
        n = values.shape[0]
        if rows.size != n or columns.size != n:
            raise ValueError("`rows` and `columns` and `values` lengths must match: "
                             f"{rows.size}, {columns.size}, {values.size}")
        if clear:
            self.clear()
        if nrows is not None or ncols is not None:
            self.resize(self._nrows if nrows is None else nrows, self._ncols if ncols is None else ncols)
        if n == 0:
            return
        dup = None if dup_op is None else _binary_for(dup_op, self.dtype)
        call(f"GrB_Matrix_build_{self.dtype.name}",
             [self, _CArray(rows, "rows"), _CArray(columns, "cols"), _CArray(values, "values"), n, dup])
        if dup_op is None and self.nvals < n:
            raise ValueError("Duplicate indices found, must provide `dup_op` BinaryOp")

    @classmethod
    def from_csr(cls, indptr, col_indices, values=1.0, dtype=None, *, nrows=None, ncols=None, name=None):
        from . import sparse

        if sparse.any_device(indptr, col_indices, values):
            return sparse.matrix_from_csx(cls, indptr, col_indices, values, dtype, nrows, ncols, name, by_col=False)
        indptr = np.ascontiguousarray(indptr, np.uint64)
        col_indices = np.ascontiguousarray(col_indices, np.uint64)
        if nrows is not None and int(nrows) != indptr.size - 1:  # reference core/matrix.py:1073-1077
            raise ValueError(f"nrows must be None or equal to len(indptr) - 1; expected {indptr.size - 1}, got {nrows}")
        nrows = indptr.size - 1
        if ncols is None:
            ncols = int(col_indices.max()) + 1 if col_indices.size else 0
        vals = np.asarray(values)
        dt = _values_dtype(vals, dtype)
        vals = np.ascontiguousarray(np.broadcast_to(np.asarray(vals, dt.np_type), col_indices.shape))
        C = cls.__new__(cls)
        C.dtype = dt
        C.name = _autoname("M") if name is None else name
        C._h = ctypes.c_void_p()
        C._nrows, C._ncols = int(nrows), int(ncols)
        call(f"GrB_Matrix_import_{dt.name}",
             [_Pointer(C), dt, nrows, ncols, _CArray(indptr, "indptr"), _CArray(col_indices, "col"),
              _CArray(vals, "values"), indptr.size, col_indices.size, vals.size, lib.GrB_CSR_FORMAT])
        return C

    @classmethod
    def from_csc(cls, indptr, row_indices, values=1.0, dtype=None, *, nrows=None, ncols=None, name=None):
        """The Matrix of a CSC triple (reference core/matrix.py:1180-1222): host arrays through
        GrB_Matrix_import with GrB_CSC_FORMAT, device arrays through GxB_Matrix_import_sparse."""
        from . import sparse

        if sparse.any_device(indptr, row_indices, values):
            return sparse.matrix_from_csx(cls, indptr, row_indices, values, dtype, nrows, ncols, name, by_col=True)
        indptr = np.ascontiguousarray(indptr, np.uint64)
        row_indices = np.ascontiguousarray(row_indices, np.uint64)
        if ncols is not None and int(ncols) != indptr.size - 1:  # reference core/matrix.py:1081-1085
            raise ValueError(f"ncols must be None or equal to len(indptr) - 1; expected {indptr.size - 1}, got {ncols}")
        ncols = indptr.size - 1
        if nrows is None:
            nrows = int(row_indices.max()) + 1 if row_indices.size else 0
        vals = np.asarray(values)
        dt = _values_dtype(vals, dtype)
        vals = np.ascontiguousarray(np.broadcast_to(np.asarray(vals, dt.np_type), row_indices.shape))
        C = cls.__new__(cls)
        C.dtype = dt
        C.name = _autoname("M") if name is None else name
        C._h = ctypes.c_void_p()
        C._nrows, C._ncols = int(nrows), int(ncols)
        call(f"GrB_Matrix_import_{dt.name}",
             [_Pointer(C), dt, nrows, ncols, _CArray(indptr, "indptr"), _CArray(row_indices, "row"),
              _CArray(vals, "values"), indptr.size, row_indices.size, vals.size, lib.GrB_CSC_FORMAT])
        return C

    @classmethod
    def from_dense(cls, values, missing_value=None, *, dtype=None, name=None, bitmap=None):
        """The Matrix of a 2-d list, numpy array or device array (GxB_Matrix_import_dense; reference
        core/matrix.py:1457-1518): every position holds an entry, but those equal to
        ``missing_value`` and those whose byte of ``bitmap`` (same shape, order and residence) is 0."""
        from .dense import from_dense

        return from_dense(cls, values, missing_value, dtype, name, bitmap)

    @classmethod
    def from_scalar(cls, value, nrows, ncols, dtype=None, *, name=None):
        """The full nrows x ncols Matrix of one value (reference core/matrix.py:1393-1455)."""
        from .dense import from_scalar

        return from_scalar(cls, value, (nrows, ncols), dtype, name)

    def to_dense(self, fill_value=None, dtype=None, *, out=None, bitmap=None):
        """The numpy array of this shape with ``fill_value`` where there is no entry
        (GxB_Matrix_export_dense; reference core/matrix.py:1520-1574).  ``out``: a numpy or device
        array in C or F order to fill in place (its dtype is the result's); ``bitmap``: an array of
        the same shape, order and residence that receives 1 / 0 per position."""
        from .dense import to_dense

        return to_dense(self, fill_value, dtype, out, bitmap, upcast=True)

    def to_csr(self, dtype=None, *, sort=True, device=False, index_dtype="int64"):
        """(indptr, col_indices, values).  ``device=True``: torch CUDA tensors written on the device
        (GxB_Matrix_export_sparse), indices int64 or, with ``index_dtype="int32"``, int32; the library
        stream is waited on, so the tensors are complete on any stream."""
        if device:
            from .sparse import matrix_export

            return matrix_export(self, "csr", dtype, index_dtype, (True, True, True))
        return self._to_csx(dtype, lib.GrB_CSR_FORMAT, self._nrows + 1)

    def to_csc(self, dtype=None, *, sort=True, device=False, index_dtype="int64"):
        """(indptr, row_indices, values) (reference core/matrix.py:1704-1727); ``device`` as in to_csr."""
        if device:
            from .sparse import matrix_export

            return matrix_export(self, "csc", dtype, index_dtype, (True, True, True))
        return self._to_csx(dtype, lib.GrB_CSC_FORMAT, self._ncols + 1)

    def _to_csx(self, dtype, fmt, np_len):
        dt = self.dtype if dtype is None else lookup_dtype(dtype)
        n = self.nvals
        ap = np.empty(np_len, np.uint64)
        ai = np.empty(n, np.uint64)
        ax = np.empty(n, dt.np_type)
        lens = [ctypes.c_uint64(ap.size), ctypes.c_uint64(ai.size), ctypes.c_uint64(ax.size)]
        rc = getattr(lib, f"GrB_Matrix_export_{dt.name}")(
            ctypes.c_void_p(ap.ctypes.data), ctypes.c_void_p(ai.ctypes.data),
            ctypes.c_void_p(ax.ctypes.data), *[ctypes.byref(x) for x in lens], fmt, self._h)
        check_status_carg(rc, "Matrix", self._h)
        return ap.astype(np.int64), ai.astype(np.int64), ax

    def to_coo(self, dtype=None, *, rows=True, columns=True, values=True, sort=True, device=False,
               index_dtype="int64"):
        if device:  # torch CUDA tensors written on the device; an array that is not wanted is not exported
            from .sparse import matrix_export

            return matrix_export(self, "coo", dtype, index_dtype, (rows, columns, values))
        dt = self.dtype if dtype is None else lookup_dtype(dtype)
        n = self.nvals
        r = np.empty(n, np.uint64)
        c = np.empty(n, np.uint64)
        v = np.empty(n, dt.np_type)
        nv = ctypes.c_uint64(n)
        rc = getattr(lib, f"GrB_Matrix_extractTuples_{dt.name}")(
            ctypes.c_void_p(r.ctypes.data), ctypes.c_void_p(c.ctypes.data), ctypes.c_void_p(v.ctypes.data),
            ctypes.byref(nv), self._h)
        check_status_carg(rc, "Matrix", self._h)
        return (r if rows else None, c if columns else None, v if values else None)

    def to_dict(self):
        r, c, v = self.to_coo()
        return {(int(a), int(b)): x.item() for a, b, x in zip(r, c, v)}

    def dup(self, dtype=None, *, clear=False, mask=None, name=None):
        if dtype is None and not clear and mask is None:
            C = Matrix.__new__(Matrix)
            C.dtype = self.dtype
            C.name = _autoname("M") if name is None else name
            C._h = ctypes.c_void_p()
            C._nrows, C._ncols = self._nrows, self._ncols
            call("GrB_Matrix_dup", [_Pointer(C), self])
            return C
        C = Matrix(self.dtype if dtype is None else dtype, self._nrows, self._ncols, name=name)
        if not clear:
            if mask is None:
                C << self
            else:
                C(mask=mask) << self
        return C

    def clear(self):
        call("GrB_Matrix_clear", [self])

    def resize(self, nrows, ncols):
        call("GrB_Matrix_resize", [self, nrows, ncols])
        self._nrows, self._ncols = int(nrows), int(ncols)

    def wait(self):
        call("GrB_Matrix_wait", [self, lib.GrB_MATERIALIZE])

    # ---------------------------------------------------------------- elements
    def __getitem__(self, keys):
        """A[i, j] element; A[I, J] -> GrB_Matrix_extract; A[I, j] / A[i, J] -> GrB_Col_extract
        (the row form with INP0 transposed), reference core/matrix.py:2860-2920."""
        if not isinstance(keys, tuple) or len(keys) != 2:
            raise TypeError("Matrix indexing requires a (rows, columns) pair")
        rk, rc, rn = _axis_index(keys[0], self._nrows)
        ck, cc, cn = _axis_index(keys[1], self._ncols)
        if rk == "scalar" and ck == "scalar":
            return _MatrixElement(self, rc, cc)
        from .vector import VectorExpression

        if rk == "scalar":
            expr = VectorExpression("extract", "GrB_Col_extract", [self, cc, cn, rc], at=True, dtype=self.dtype,
                                    size=cn)
        elif ck == "scalar":
            expr = VectorExpression("extract", "GrB_Col_extract", [self, rc, rn, cc], dtype=self.dtype, size=rn)
        else:
            expr = MatrixExpression("extract", "GrB_Matrix_extract", [self, rc, rn, cc, cn], dtype=self.dtype,
                                    nrows=rn, ncols=cn)
        expr._target = (self, keys)  # C[I, J] << A and C[I, J](M) << A (BaseExpression)
        return expr

    def __setitem__(self, keys, value):
        if keys is Ellipsis or (isinstance(keys, tuple) and all(_is_full_slice(k) for k in keys)):
            self._assign(Ellipsis, value, None, None, False)
            return
        if not (isinstance(keys, tuple) and len(keys) == 2 and all(_is_int(k) for k in keys)):
            self._assign(keys, value, None, None, False)
            return
        i, j = _scalar_keys(keys, 2)
        from .scalar import Scalar

        if isinstance(value, Scalar):
            value = value.value
            if value is None:
                del self[i, j]
                return
        call(f"GrB_Matrix_setElement_{self.dtype.name}", [self, value, i, j])

    def __delitem__(self, keys):
        i, j = _scalar_keys(keys, 2)
        call("GrB_Matrix_removeElement", [self, i, j])

    def _assign(self, keys, value, mask, accum, replace):
        """C(mask, accum, replace)[keys] << value: which call each form becomes follows the reference's
        _prep_for_assign (core/matrix.py:2905-3316).  Without a mask, assign and subassign are one operation,
        so C[I, J] << A is GxB_Matrix_subassign; a mask of C's shape with index lists needs
        GrB_Matrix_assign with lists, which the library does not implement."""
        from .scalar import Scalar
        from .vector import Vector

        if keys is Ellipsis or (isinstance(keys, tuple) and all(_is_full_slice(k) for k in keys)) \
                or _is_full_slice(keys):
            desc = _mask_desc(mask, replace, isinstance(value, TransposedMatrix))
            if isinstance(value, TransposedMatrix):
                value = value._matrix
            if isinstance(value, Matrix):
                call("GrB_Matrix_assign", [self, mask, accum, value, lib.GrB_ALL, self._nrows, lib.GrB_ALL,
                                           self._ncols, desc])
                return
            if isinstance(value, Scalar):
                value = value.value
            call(f"GrB_Matrix_assign_{self.dtype.name}",
                 [self, mask, accum, value, lib.GrB_ALL, self._nrows, lib.GrB_ALL, self._ncols, desc])
            return
        (rk, rc, rn), (ck, cc, cn) = self._region(keys)
        vmask = mask is not None and mask.parent.ndim == 1
        if isinstance(value, Vector):
            if rk == ck:
                _bad_value(value, "Scalar" if rk == "scalar" else "Scalar, Matrix, TransposedMatrix")
            if mask is not None and not vmask:  # C(M)[i, J] << v
                self._matrix_mask_with_lists(mask)
            n = cn if rk == "scalar" else rn
            if value._size != n:
                raise DimensionMismatch(f"value of size {value._size} does not match the {n} selected positions")
            line = self._ncols if rk == "scalar" else self._nrows
            if mask is not None and mask.parent._size != line:  # the mask of an assign spans the whole row / column
                raise DimensionMismatch(f"mask of size {mask.parent._size} does not match the "
                                        f"{'row' if rk == 'scalar' else 'column'} of size {line}")
            desc = _mask_desc(mask, replace)
            if rk == "scalar":
                call("GrB_Row_assign", [self, mask, accum, value, rc, cc, cn, desc])
            else:
                call("GrB_Col_assign", [self, mask, accum, value, rc, rn, cc, desc])
            return
        if isinstance(value, (Matrix, TransposedMatrix)):
            if rk == "scalar" or ck == "scalar":
                _bad_value(value, "Scalar" if rk == ck else "Scalar, Vector")
            if vmask:
                raise TypeError("Unable to use Vector mask on Matrix assignment to a Matrix")
            if mask is not None:  # C(M)[I, J] << A
                self._matrix_mask_with_lists(mask)
            if value.shape != (rn, cn):
                raise DimensionMismatch(f"value of shape {value.shape} does not match the region {(rn, cn)}")
            desc = _mask_desc(None, False, isinstance(value, TransposedMatrix))
            if isinstance(value, TransposedMatrix):
                value = value._matrix
            call("GxB_Matrix_subassign", [self, None, accum, value, rc, rn, cc, cn, desc])
            return
        # a scalar
        if vmask:
            if rk == ck:
                raise TypeError("Unable to use Vector mask on single element assignment to a Matrix"
                                if rk == "scalar" else "Unable to use Vector mask on Matrix assignment to a Matrix")
            expanded = self._expand_scalar(value, cn if rk == "scalar" else rn)
            self._assign(keys, expanded, mask, accum, replace)
            return
        if isinstance(value, Scalar):
            value = value.value
        if rk == "scalar":
            rc, rn = _CArray(np.array([rc], np.uint64), "I"), 1
        if ck == "scalar":
            cc, cn = _CArray(np.array([cc], np.uint64), "J"), 1
        call(f"GrB_Matrix_assign_{self.dtype.name}", [self, mask, accum, value, rc, rn, cc, cn,
                                                      _mask_desc(mask, replace)])

    def _subassign(self, keys, value, mask, accum, replace):
        """C[keys](mask, accum, replace) << value: the mask has the region's shape (GxB_*_subassign)."""
        from .scalar import Scalar
        from .vector import Vector

        if mask is None:  # C[I, J](accum=op) << A: assign and subassign coincide
            self._assign(keys, value, None, accum, False)
            return
        if keys is Ellipsis or _is_full_slice(keys):
            keys = (slice(None), slice(None))
        (rk, rc, rn), (ck, cc, cn) = self._region(keys)
        vmask = mask.parent.ndim == 1
        if rk == "scalar" and ck == "scalar":
            if vmask:
                raise TypeError("Unable to use Vector mask on single element assignment to a Matrix")
            raise TypeError("Single element assign does not accept a submask")
        desc = _mask_desc(mask, replace, isinstance(value, TransposedMatrix))
        if rk == "scalar" or ck == "scalar":
            if isinstance(value, (Matrix, TransposedMatrix)):
                _bad_value(value, "Scalar, Vector")
            if not vmask:
                raise TypeError("Indices for subassign imply Vector submask, but got Matrix mask instead")
            n = cn if rk == "scalar" else rn
            if not isinstance(value, Vector):  # the scalar as a value vector of the mask's size
                value = self._expand_scalar(value, mask.parent._size)
            if value._size != n or mask.parent._size != n:
                raise DimensionMismatch(f"value of size {value._size} and mask of size {mask.parent._size} "
                                        f"must match the {n} selected positions")
            if rk == "scalar":
                call("GxB_Row_subassign", [self, mask, accum, value, rc, cc, cn, desc])
            else:
                call("GxB_Col_subassign", [self, mask, accum, value, rc, rn, cc, desc])
            return
        if isinstance(value, Vector):
            _bad_value(value, "Scalar, Matrix, TransposedMatrix")
        if vmask:
            raise TypeError("Unable to use Vector mask on Matrix assignment to a Matrix")
        if mask.parent.shape != (rn, cn):
            raise DimensionMismatch(f"mask of shape {mask.parent.shape} does not match the region {(rn, cn)}")
        if isinstance(value, (Matrix, TransposedMatrix)):
            if value.shape != (rn, cn):
                raise DimensionMismatch(f"value of shape {value.shape} does not match the region {(rn, cn)}")
            if isinstance(value, TransposedMatrix):
                value = value._matrix
            call("GxB_Matrix_subassign", [self, mask, accum, value, rc, rn, cc, cn, desc])
            return
        if not isinstance(value, Scalar):
            value = Scalar.from_value(value, self.dtype)
        call("GxB_Matrix_subassign_Scalar", [self, mask, accum, value, rc, rn, cc, cn, desc])

    def _region(self, keys):
        if not isinstance(keys, tuple) or len(keys) != 2:
            raise TypeError("Matrix indexing requires a (rows, columns) pair")
        return _axis_index(keys[0], self._nrows), _axis_index(keys[1], self._ncols)

    def _matrix_mask_with_lists(self, mask):
        if mask.parent.shape != self.shape:
            raise DimensionMismatch(f"mask of shape {mask.parent.shape} does not match the output {self.shape}")
        raise NotImplementedError("C(M)[I, J] << A with a Matrix mask of C's shape needs GrB_Matrix_assign with "
                                  "index lists, which is not implemented; use the submask form C[I, J](M) << A")

    def _expand_scalar(self, value, n):
        from .scalar import Scalar
        from .vector import Vector

        dtype = value.dtype if isinstance(value, Scalar) else self.dtype
        v = Vector(dtype, n, name="v_temp")
        v[:] = value
        return v

    # ---------------------------------------------------------------- operations
    def mxm(self, other, op=None):
        return _mxm(self, other, op)

    def mxv(self, other, op=None):
        return _mxv(self, other, op)

    def ewise_mult(self, other, op=None):
        return _ewise(self, other, op if op is not None else _op.binary.times, "mult")

    def ewise_add(self, other, op=None):
        return _ewise(self, other, op if op is not None else _op.monoid.plus, "add")

    def ewise_union(self, other, op, left_default, right_default):
        return _ewise_union(self, other, op, left_default, right_default)

    def reduce_scalar(self, op=None, *, allow_empty=True):
        return _reduce_scalar(self, op, allow_empty)

    def reduce_rowwise(self, op=None):
        return _reduce_rows(self, op, columnwise=False)

    def reduce_columnwise(self, op=None):
        return _reduce_rows(self, op, columnwise=True)

    def apply(self, op, right=None, *, left=None):
        return _apply_expr(self, op, right, left)

    def select(self, op, thunk=None):
        return _select_expr(self, op, thunk)

    def kronecker(self, other, op=None):
        return _kronecker(self, other, op)

    def diag(self, k=0, dtype=None, *, name=None, **opts):
        """Diagonal ``k`` as a new Vector (GxB_Vector_diag; reference core/matrix.py:735-754)."""
        from .ss import diag

        return diag(self, k=k, dtype=dtype, name=name, **opts)

    def isequal(self, other, *, check_dtype=False):
        """reference core/matrix.py:357-398"""
        if isinstance(other, TransposedMatrix):
            other = other.new()
        if not isinstance(other, Matrix):
            raise TypeError(f"Expected Matrix, got {type(other)}")
        if check_dtype and self.dtype != other.dtype:
            return False
        if self.shape != other.shape or self.nvals != other.nvals:
            return False
        opr = _op.binary.eq[self.dtype] if check_dtype else _op.get_typed_op(_op.binary.eq, self.dtype,
                                                                             other.dtype)
        matches = Matrix(BOOL, self._nrows, self._ncols, name="M_isequal")
        matches << self.ewise_mult(other, opr)
        if matches.nvals != self.nvals:
            return False
        return matches.reduce_scalar(_op.monoid.land, allow_empty=False).new().value

    def isclose(self, other, *, rel_tol=1e-7, abs_tol=0.0, check_dtype=False):
        if isinstance(other, TransposedMatrix):
            other = other.new()
        if check_dtype and self.dtype != other.dtype:
            return False
        if self.shape != other.shape or self.nvals != other.nvals:
            return False
        r1, c1, v1 = self.to_coo()
        r2, c2, v2 = other.to_coo()
        if not (np.array_equal(r1, r2) and np.array_equal(c1, c2)):
            return False
        return bool(np.all(np.isclose(v1, v2, rtol=rel_tol, atol=abs_tol, equal_nan=True)))

    def power(self, n, op=None):
        """A^n by repeated squaring with GrB_mxm (reference core/matrix.py:95-154, 2754-2806)."""
        if isinstance(n, bool) or not isinstance(n, (int, np.integer)):
            raise TypeError(f"n must be a positive integer; got bad type: {type(n)}")
        if n <= 0:
            raise ValueError(f"n must be a positive integer; got: {n}")
        if self._nrows != self._ncols:
            raise DimensionMismatch(f"power only works for square Matrix; shape is {self.shape}")
        op = _op.get_typed_op(op if op is not None else _op.semiring.plus_times, self.dtype,
                              kind="semiring")
        return MatrixExpression("power", None, [self, _power, (self, n, op)], op=op, nrows=self._nrows,
                                ncols=self._ncols, dtype=op.return_type)


def _power(updater, A, n, op):
    result = None
    base = A
    while True:
        if n & 1:
            result = base if result is None else result.mxm(base, op).new()
        n >>= 1
        if not n:
            break
        base = base.mxm(base, op).new()
    updater << result


def _is_int(k):
    return isinstance(k, (int, np.integer)) and not isinstance(k, bool)


def _is_full_slice(k):
    return isinstance(k, slice) and k == slice(None)


def _mask_desc(mask, replace, transpose_first=False):
    return descriptor_lookup(mask_complement=mask.complement if mask is not None else False,
                             mask_structure=mask.structure if mask is not None else False,
                             output_replace=replace, transpose_first=transpose_first)


def _bad_value(value, expected):
    raise TypeError(f"Bad type for argument `value` in Matrix.__setitem__(...): expected {expected}; "
                    f"got {type(value).__name__}")


def _axis_index(key, size):
    """One axis of an index: ("scalar", i, 1), or ("list", GrB_ALL | _CArray, length).  Slices
    other than ':' become explicit index arrays (the reference's non-SuiteSparse path,
    core/slice.py:26-33)."""
    if isinstance(key, (int, np.integer)) and not isinstance(key, bool):
        i = int(key)
        if i < 0:
            i += size
        if not 0 <= i < size:
            raise IndexError(f"index {int(key)} out of range for size {size}")
        return "scalar", i, 1
    if isinstance(key, slice):
        start, stop, step = key.indices(size)
        n = len(range(start, stop, step))
        if n == size and step == 1:
            return "list", lib.GrB_ALL, size
        return "list", _CArray(np.arange(start, stop, step, dtype=np.uint64), "I"), n
    arr = np.asarray(key)
    if arr.dtype == np.bool_:
        raise TypeError("boolean index arrays are not supported")
    arr = np.where(arr < 0, arr + size, arr) if arr.size else arr
    arr = _index_array(np.atleast_1d(arr), "indices")
    if arr.size and int(arr.max()) >= size:
        raise IndexError(f"index {int(arr.max())} out of range for size {size}")
    return "list", _CArray(arr, "I"), int(arr.size)


def _scalar_keys(keys, nd):
    if not isinstance(keys, tuple) or len(keys) != nd:
        raise TypeError(f"Expected {nd} integer indices")
    out = []
    for k in keys:
        if isinstance(k, (int, np.integer)) and not isinstance(k, bool):
            out.append(int(k))
        else:
            raise NotImplementedError("only scalar element indexing is supported")
    return out


class _MatrixElement:
    __slots__ = "parent", "i", "j"

    def __init__(self, parent, i, j):
        self.parent, self.i, self.j = parent, i, j

    def new(self, dtype=None, *, name=None):
        from .scalar import Scalar

        s = Scalar(self.parent.dtype if dtype is None else dtype, name=name)
        s.value = self.value
        return s

    @property
    def value(self):
        A = self.parent
        out = np.empty(1, A.dtype.np_type)
        rc = getattr(lib, f"GrB_Matrix_extractElement_{A.dtype.name}")(
            ctypes.c_void_p(out.ctypes.data), A._h, self.i, self.j)
        if check_status_carg(rc, "Matrix", A._h) is NoValue:
            return None
        return out[0].item()

    def __lshift__(self, value):
        self.parent[self.i, self.j] = value

    update = __lshift__

    def __call__(self, *args, **kwargs):
        upd = self.parent(*args, **kwargs)
        if upd.mask is not None and upd.mask.parent.ndim == 1:
            return _NoSubmask("Unable to use Vector mask on single element assignment to a Matrix")
        return _NoSubmask()

    def __eq__(self, other):
        return self.value == other


class _NoSubmask:
    """C[i, j](...) or w[i](...): building it is allowed (as in the reference), assigning through it is not"""

    __slots__ = ("message",)

    def __init__(self, message="Single element assign does not accept a submask"):
        self.message = message

    def __lshift__(self, value):
        raise TypeError(self.message)

    update = __lshift__


class TransposedMatrix:
    ndim = 2
    _is_transposed = True
    _is_scalar = False

    def __init__(self, matrix):
        self._matrix = matrix

    @property
    def _carg(self):
        return self._matrix._carg

    @property
    def name(self):
        return self._matrix.name

    @property
    def dtype(self):
        return self._matrix.dtype

    @property
    def nrows(self):
        return self._matrix._ncols

    @property
    def ncols(self):
        return self._matrix._nrows

    _nrows = property(lambda self: self._matrix._ncols)
    _ncols = property(lambda self: self._matrix._nrows)

    @property
    def shape(self):
        return (self.nrows, self.ncols)

    @property
    def nvals(self):
        return self._matrix.nvals

    @property
    def T(self):
        return self._matrix

    def new(self, dtype=None, *, mask=None, name=None):
        C = Matrix(self.dtype if dtype is None else dtype, self.nrows, self.ncols, name=name)
        expr = MatrixExpression("transpose", "GrB_transpose", [self._matrix], dtype=self.dtype,
                                nrows=self.nrows, ncols=self.ncols)
        if mask is None:
            C << expr
        else:
            C(mask=_check_mask(mask)) << expr
        return C

    def mxm(self, other, op=None):
        return _mxm(self, other, op)

    def mxv(self, other, op=None):
        return _mxv(self, other, op)

    def ewise_mult(self, other, op=None):
        return _ewise(self, other, op if op is not None else _op.binary.times, "mult")

    def ewise_add(self, other, op=None):
        return _ewise(self, other, op if op is not None else _op.monoid.plus, "add")

    def ewise_union(self, other, op, left_default, right_default):
        return _ewise_union(self, other, op, left_default, right_default)

    def power(self, n, op=None):
        return self.new().power(n, op)

    def diag(self, k=0, dtype=None, *, name=None, **opts):
        """Diagonal ``k`` of the transpose: diagonal ``-k`` of the matrix, nothing is transposed
        (reference core/matrix.py:3677-3679)."""
        from .ss import _diag_k

        return self._matrix.diag(-_diag_k(k), dtype, name=name, **opts)

    def reduce_rowwise(self, op=None):
        return _reduce_rows(self, op, columnwise=False)

    def reduce_columnwise(self, op=None):
        return _reduce_rows(self, op, columnwise=True)

    def reduce_scalar(self, op=None, *, allow_empty=True):
        return self._matrix.reduce_scalar(op, allow_empty=allow_empty)

    def apply(self, op, right=None, *, left=None):
        return _apply_expr(self, op, right, left)

    def select(self, op, thunk=None):
        return _select_expr(self, op, thunk)

    def kronecker(self, other, op=None):
        return _kronecker(self, other, op)

    def to_coo(self, *args, device=False, index_dtype="int64", **kw):
        if device:  # the transpose is built on the device (GrB_transpose) and exported row-major
            return self.new().to_coo(*args, device=True, index_dtype=index_dtype, **kw)
        r, c, v = self._matrix.to_coo(*args, **kw)
        o = np.lexsort((r, c))
        return c[o], r[o], v[o]

    def to_csr(self, dtype=None, *, sort=True, device=False, index_dtype="int64"):
        """The CSR of the transpose is the matrix' CSC: nothing is transposed."""
        return self._matrix.to_csc(dtype, sort=sort, device=device, index_dtype=index_dtype)

    def to_csc(self, dtype=None, *, sort=True, device=False, index_dtype="int64"):
        return self._matrix.to_csr(dtype, sort=sort, device=device, index_dtype=index_dtype)

    def to_dense(self, fill_value=None, dtype=None, *, out=None, bitmap=None):
        """As Matrix.to_dense: the column-major export of the matrix, nothing is transposed."""
        from .dense import to_dense

        return to_dense(self, fill_value, dtype, out, bitmap, upcast=True)

    def isequal(self, other, **kw):
        return self.new().isequal(other, **kw)

    def __matmul__(self, other):
        from .infix import _matmul_infix_expr

        return _matmul_infix_expr(self, other)

    def __rmatmul__(self, other):
        from .infix import _matmul_infix_expr

        return _matmul_infix_expr(other, self)

    def __sub__(self, other):
        from .infix import _sub_infix_expr

        return _sub_infix_expr(self, other)


def _is_agg(op):
    return getattr(op, "opclass", None) == "Aggregator"


def _reduce_rows(A, op, *, columnwise):
    """A.reduce_rowwise / reduce_columnwise (reference core/matrix.py:2556-2623): a monoid (or a
    BinaryOp that is one) -> GrB_Matrix_reduce_Monoid (desc INP0=TRAN for columns of A, rows of
    A.T); an Aggregator -> its semiring lowering (agg.py)."""
    from .vector import VectorExpression

    if op is None:
        op = _op.monoid.plus
    size = A.ncols if columnwise else A.nrows
    if _is_agg(op):
        from .agg import reduce_rowwise_recipe

        typed = op[A.dtype] if op.opclass == "Aggregator" and not hasattr(op, "parent") else op
        return VectorExpression("reduce_columnwise" if columnwise else "reduce_rowwise", None,
                                [A, reduce_rowwise_recipe, (A, typed, columnwise)],
                                dtype=typed.return_type, size=size)
    t = _op.get_typed_op(op, A.dtype, kind="monoid")
    if t.opclass == "BinaryOp":
        mon = getattr(_op.monoid, t.parent.name, None)
        if mon is None or t.type not in mon._typed:
            raise TypeError(f"{op!r} is not a monoid; reduce needs a Monoid")
        t = mon[t.type]
    if t.opclass != "Monoid":
        raise TypeError(f"Expected a Monoid or Aggregator, got {t.opclass}")
    a, at = _unwrap(A)
    return VectorExpression("reduce_columnwise" if columnwise else "reduce_rowwise", "GrB_Matrix_reduce_Monoid",
                            [a], op=t, at=(at != columnwise), size=size)


def _reduce_scalar(x, op, allow_empty):
    """Vector.reduce / Matrix.reduce_scalar: monoids -> GrB_*_reduce_Monoid_Scalar; Aggregators ->
    the two-SpMV lowering of reference core/operator/agg.py:229-276."""
    from .scalar import ScalarExpression

    if op is None:
        op = _op.monoid.plus
    if _is_agg(op):
        from .agg import matrix_scalar_forbidden, reduce_scalar_recipe

        typed = op[x.dtype] if not hasattr(op, "parent") else op
        bad = matrix_scalar_forbidden(typed.parent) if x.ndim == 2 else None
        if bad:
            raise ValueError(f"Aggregator {bad} may not be used with Matrix.reduce_scalar.")
        if not allow_empty:
            if typed.parent._monoid is None:
                raise ValueError("allow_empty=False not allowed when using Aggregators")
            return _reduce_scalar(x, typed.parent._monoid[typed.type], allow_empty)
        return ScalarExpression("reduce", None, [x, reduce_scalar_recipe, (x, typed)],
                                dtype=typed.return_type)
    op = _op.get_typed_op(op, x.dtype, kind="monoid")
    if op.opclass == "BinaryOp":
        op = getattr(_op.monoid, op.parent.name)[op.type]
    kind = "Matrix" if x.ndim == 2 else "Vector"
    return ScalarExpression("reduce_scalar" if kind == "Matrix" else "reduce",
                            f"GrB_{kind}_reduce_Monoid_Scalar", [x], op=op, allow_empty=allow_empty)


def _apply_expr(x, op, right, left):
    """x.apply(op[, right= | left=]) (reference core/vector.py:1311-1460, core/matrix.py:2297-2447):
    a UnaryOp -> GrB_*_apply; a BinaryOp with a bound scalar -> GrB_*_apply_BinaryOp{1st,2nd}_<T>;
    an index-unary or select operator (or "rowindex" / "colindex" / "diagindex" / "index") with the
    thunk in `right` -> GrB_*_apply_IndexOp_<T>."""
    from .scalar import Scalar
    from .vector import VectorExpression

    kind = "Vector" if x.ndim == 1 else "Matrix"
    src, at = _unwrap(x) if kind == "Matrix" else (x, False)
    if _is_index_unary(op):
        return _apply_index_expr(x, kind, src, at, op, right, left)

    def mk(cf, args, t):
        if kind == "Vector":
            return VectorExpression("apply", cf, args, op=t, size=x.size)
        return MatrixExpression("apply", cf, args, op=t, at=at, nrows=x.nrows, ncols=x.ncols)

    if left is None and right is None:
        t = _op.get_typed_op(op, x.dtype, kind="unary")
        if t.opclass != "UnaryOp":
            raise TypeError(f"Bad type for argument `op`: expected UnaryOp, got {t.opclass}")
        return mk(f"GrB_{kind}_apply", [src], t)
    if left is not None and right is not None:
        raise TypeError("Cannot provide both `left` and `right` to apply")
    val = left if right is None else right
    sc = val if isinstance(val, Scalar) else Scalar.from_value(val)
    if right is None:
        t = _op.get_typed_op(op, sc.dtype, x.dtype, kind="binary", is_left_scalar=True)
    else:
        t = _op.get_typed_op(op, x.dtype, sc.dtype, kind="binary", is_right_scalar=True)
    if t.opclass == "Monoid":
        t = getattr(_op.binary, t.parent.name)[t.type]
    elif t.opclass != "BinaryOp":
        raise TypeError(f"Bad type for argument `op`: expected BinaryOp, got {t.opclass}")
    if t.is_positional:
        raise NotImplementedError("positional operators in apply")
    cv = sc.value
    if right is None:
        return mk(f"GrB_{kind}_apply_BinaryOp1st_{sc.dtype.name}", [cv, src], t)
    return mk(f"GrB_{kind}_apply_BinaryOp2nd_{sc.dtype.name}", [src, cv], t)


def _is_index_unary(op):
    """An index-unary or select operator, typed or not, or one of the names only `indexunary` has
    (any other string in apply, "==" included, names a unary or binary operator)."""
    if isinstance(op, str):
        return op.strip().lower() in _op._INDEXUNARY_STRINGS
    return getattr(op, "opclass", None) in ("IndexUnaryOp", "SelectOp")


def _thunk_arg(thunk, kind, method, cname):
    """-> (thunk dtype, C function, argument): a Scalar goes to GrB_<kind>_<cname>_Scalar, a literal
    as a C scalar of its numpy type to the typed entry point (no GrB_Scalar)."""
    from .scalar import Scalar

    if isinstance(thunk, Scalar):
        return thunk.dtype, f"GrB_{kind}_{cname}_Scalar", thunk
    try:
        a = np.asarray(thunk)
        if a.ndim != 0:
            raise TypeError("not a scalar")
        tdtype = lookup_dtype(a.dtype)
    except (TypeError, ValueError) as exc:
        raise TypeError(f"Bad type for keyword argument `thunk` in {method}: {type(thunk)}; expected a "
                        "Scalar or a literal scalar") from exc
    return tdtype, f"GrB_{kind}_{cname}_{tdtype.name}", a.item()


def _apply_index_expr(x, kind, src, at, op, right, left):
    """x.apply(indexunary op, thunk) (reference core/matrix.py:2337-2437, core/vector.py, same
    method): f(x(i, j), i, j, thunk) on the structure of x -> GrB_*_apply_IndexOp_<T> (a Scalar
    thunk: GrB_*_apply_IndexOp_Scalar)."""
    from .scalar import Scalar
    from .vector import VectorExpression

    if left is not None:
        raise TypeError("Do not use `left` with an IndexUnaryOp or SelectOp in apply; "
                        "the thunk goes to `right`")
    thunk = right
    if thunk is None:
        thunk = False  # the most basic form of 0 when unifying dtypes
    tdtype, cf, arg = _thunk_arg(thunk, kind, "apply", "apply_IndexOp")
    if isinstance(op, str):
        op = _op.indexunary.from_string(op)
    if op.is_positional:
        # typed by the input alone: INT32 -> the INT32 operator, anything else -> INT64
        t = _op.get_typed_op(op, x.dtype, kind="indexunary")
        if not isinstance(thunk, Scalar):
            # the library casts the thunk of a positional operator to an integer
            arg, cf = int(arg), f"GrB_{kind}_apply_IndexOp_INT64"
    else:
        t = _op.get_typed_op(op, x.dtype, tdtype, kind="indexunary", is_right_scalar=True)
    if kind == "Vector":
        return VectorExpression("apply", cf, [src, arg], op=t, size=x.size)
    return MatrixExpression("apply", cf, [src, arg], op=t, at=at, nrows=x.nrows, ncols=x.ncols)


def _select_mask(updater, obj, mask):
    """x.select(mask): the entries of x the mask selects (reference core/vector.py:80-93)."""
    from .base import Updater

    if updater.mask is None:
        Updater(updater.parent, mask=mask, accum=updater.accum, replace=updater.accum is None,
                opts=updater.opts) << obj
    else:
        updater << obj.dup(mask=mask)


def _select_expr(x, op, thunk):
    """x.select(op, thunk) (reference core/vector.py:1463-1560, core/matrix.py:2452-2551): the
    entries a SelectOp keeps -> GrB_*_select_<T> (a Scalar thunk: GrB_*_select_Scalar); a mask in
    place of the operator -> the entries it selects."""
    from .base import Mask
    from .scalar import Scalar
    from .vector import Vector, VectorExpression

    kind = "Vector" if x.ndim == 1 else "Matrix"
    src, at = _unwrap(x) if kind == "Matrix" else (x, False)

    def mk(cf, args, t=None):
        if kind == "Vector":
            return VectorExpression("select", cf, args, op=t, size=x.size, dtype=x.dtype)
        return MatrixExpression("select", cf, args, op=t, at=at if cf else False, nrows=x.nrows, ncols=x.ncols,
                                dtype=x.dtype)

    if isinstance(op, (Mask, Matrix, Vector)):
        if thunk is not None:
            raise TypeError("thunk argument not None when calling select with mask or boolean object")
        mask = _check_mask(op)
        if type(mask.parent) is not (Vector if kind == "Vector" else Matrix):
            raise TypeError(f"Bad type for argument `op` in select: expected a {kind} mask, got "
                            f"{type(mask.parent).__name__}")
        obj = x.new() if at else x
        return mk(None, [obj, mask, _select_mask, (obj, mask)])
    if thunk is None:
        thunk = False  # the most basic form of 0 when unifying dtypes
    tdtype, cf, arg = _thunk_arg(thunk, kind, "select", "select")
    if getattr(op, "opclass", None) == "IndexUnaryOp" and op.is_positional:
        t = _op.get_typed_op(op, x.dtype)  # rowindex / colindex / diagindex: typed by the input alone
    else:
        t = _op.get_typed_op(op, x.dtype, tdtype, kind="select", is_right_scalar=True)
    if t.opclass not in ("SelectOp", "IndexUnaryOp"):
        raise TypeError(f"Bad type for argument `op` in select: expected SelectOp, got {t.opclass}")
    if t.is_positional and not isinstance(thunk, Scalar):
        # the library casts the thunk of a positional operator to INT64
        arg, cf = int(arg), f"GrB_{kind}_select_INT64"
    return mk(cf, [src, arg], t)


def _unwrap(x):
    if isinstance(x, TransposedMatrix):
        return x._matrix, True
    return x, False


def _binary_for(opobj, dtype):
    t = _op.get_typed_op(opobj, dtype, kind="binary")
    if t.opclass == "Monoid":
        t = getattr(_op.binary, t.parent.name)[t.type]
    return t


def _mxm(left, right, op):
    from .vector import Vector

    if isinstance(right, Vector):
        raise TypeError("mxm requires a Matrix on the right; use mxv for vectors")
    if op is None:
        op = _op.semiring.plus_times
    op = _op.get_typed_op(op, left.dtype, right.dtype, kind="semiring")
    if op.opclass != "Semiring":
        raise TypeError(f"Expected a Semiring, got {op.opclass}")
    a, at = _unwrap(left)
    b, bt = _unwrap(right)
    if left.ncols != right.nrows:
        raise DimensionMismatch(f"Dimensions not compatible for mxm: {left.shape} and {right.shape}")
    return MatrixExpression("mxm", "GrB_mxm", [a, b], op=op, at=at, bt=bt, nrows=left.nrows,
                            ncols=right.ncols)


def _mxv(left, v, op):
    from .vector import Vector, VectorExpression

    if not isinstance(v, Vector):
        raise TypeError(f"mxv requires a Vector, got {type(v)}")
    if op is None:
        op = _op.semiring.plus_times
    op = _op.get_typed_op(op, left.dtype, v.dtype, kind="semiring")
    if op.opclass != "Semiring":
        raise TypeError(f"Expected a Semiring, got {op.opclass}")
    a, at = _unwrap(left)
    if left.ncols != v.size:
        raise DimensionMismatch(f"Dimensions not compatible for mxv: {left.shape} and {v.size}")
    return VectorExpression("mxv", "GrB_mxv", [a, v], op=op, at=at, size=left.nrows)


def _ewise(left, right, opobj, kind):
    a, at = _unwrap(left)
    b, bt = _unwrap(right)
    op = _op.get_typed_op(opobj, left.dtype, right.dtype, kind="binary")
    if op.opclass == "Monoid":
        op = getattr(_op.binary, op.parent.name if op.parent.name != "eq" else "lxnor")[op.type]
    if left.shape != right.shape:
        raise DimensionMismatch(f"Dimensions do not match: {left.shape} and {right.shape}")
    cf = "GrB_Matrix_eWiseMult_BinaryOp" if kind == "mult" else "GrB_Matrix_eWiseAdd_BinaryOp"
    return MatrixExpression(f"ewise_{kind}", cf, [a, b], op=op, at=at, bt=bt, nrows=left.nrows,
                            ncols=left.ncols)


def _union_default(value, keyword):
    """A default of ewise_union as a Scalar: a Scalar as it is, a literal through Scalar.from_value."""
    from .scalar import Scalar

    if isinstance(value, Scalar):
        return value
    try:
        a = np.asarray(value)
        if a.ndim != 0 or a.dtype == object:
            raise TypeError("not a scalar")
        dtype = lookup_dtype(a.dtype)
    except (TypeError, ValueError) as exc:
        raise TypeError(f"Bad type for keyword argument `{keyword}` in ewise_union: expected Scalar, got "
                        f"{type(value).__name__}.  Literal scalars also accepted.") from exc
    return Scalar.from_value(a.item(), dtype)


def _ewise_union(left, right, op, left_default, right_default):
    """x.ewise_union(y, op, left_default, right_default) (reference core/matrix.py:2044-2161,
    core/vector.py:1141-1260) -> GxB_{Matrix,Vector}_eWiseUnion: op(x, y) where both are stored,
    op(x, right_default) where only x is, op(left_default, y) where only y is.  The operator is
    typed from the defaults unified with the operands, so float defaults upcast integer operands."""
    from .vector import Vector, VectorExpression

    kind = "Vector" if left.ndim == 1 else "Matrix"
    want = (Vector,) if kind == "Vector" else (Matrix, TransposedMatrix)
    if not isinstance(right, want):
        raise TypeError(f"Bad type for argument `other` in ewise_union: expected {kind}, got "
                        f"{type(right).__name__}")
    ld = _union_default(left_default, "left_default")
    rd = _union_default(right_default, "right_default")
    t = _op.get_typed_op(op, unify(ld.dtype, rd.dtype), unify(left.dtype, right.dtype), kind="binary",
                         is_left_scalar=True)
    if t.opclass == "Monoid":
        t = getattr(_op.binary, t.parent.name if t.parent.name != "eq" else "lxnor")[t.type]
    elif t.opclass != "BinaryOp":
        raise TypeError(f"Bad type for argument `op` in ewise_union: expected BinaryOp or Monoid, got {t.opclass}")
    if t.is_positional:
        raise NotImplementedError("positional operators in ewise_union")
    if left.shape != right.shape:
        raise DimensionMismatch(f"Dimensions do not match: {left.shape} and {right.shape}")
    if kind == "Vector":
        return VectorExpression("ewise_union", "GxB_Vector_eWiseUnion", [left, ld, right, rd], op=t, size=left.size)
    a, at = _unwrap(left)
    b, bt = _unwrap(right)
    return MatrixExpression("ewise_union", "GxB_Matrix_eWiseUnion", [a, ld, b, rd], op=t, at=at, bt=bt,
                            nrows=left.nrows, ncols=left.ncols)


def _kronecker(left, right, op):
    """A.kronecker(B, op) (reference core/matrix.py:2253-2292): a BinaryOp or a Monoid ->
    GrB_Matrix_kronecker_{BinaryOp,Monoid}; the result is (m p) x (n q)."""
    if not isinstance(right, (Matrix, TransposedMatrix)):
        raise TypeError(f"Bad type for argument `other` in kronecker: expected Matrix or TransposedMatrix, got "
                        f"{type(right).__name__}")
    if op is None:
        op = _op.binary.times
    op = _op.get_typed_op(op, left.dtype, right.dtype, kind="binary")
    # Per the spec, op may be a semiring, but this is weird, so don't.
    if op.opclass not in ("BinaryOp", "Monoid"):
        raise TypeError(f"Bad type for argument `op` in kronecker: expected BinaryOp or Monoid, got {op.opclass}")
    if getattr(op, "is_positional", False):
        raise NotImplementedError("positional operators in kronecker")
    a, at = _unwrap(left)
    b, bt = _unwrap(right)
    return MatrixExpression("kronecker", f"GrB_Matrix_kronecker_{op.opclass}", [a, b], op=op, at=at, bt=bt,
                            nrows=left.nrows * right.nrows, ncols=left.ncols * right.ncols)


class MatrixExpression(BaseExpression):
    output_type = Matrix
    ndim = 2

    def __init__(self, method_name, cfunc_name, args, *, at=False, bt=False, op=None, dtype=None,
                 nrows=None, ncols=None, expr_repr=None):
        super().__init__(method_name, cfunc_name, args, at=at, bt=bt, op=op, dtype=dtype,
                         expr_repr=expr_repr)
        self._nrows = nrows
        self._ncols = ncols

    @property
    def nrows(self):
        return self._nrows

    @property
    def ncols(self):
        return self._ncols

    @property
    def shape(self):
        return (self._nrows, self._ncols)

    def construct_output(self, dtype=None, *, name=None):
        return Matrix(self.dtype if dtype is None else dtype, self._nrows, self._ncols, name=name)

    def __repr__(self):
        return f"<MatrixExpression {self.method_name} {self._nrows}x{self._ncols} {self.dtype}>"
