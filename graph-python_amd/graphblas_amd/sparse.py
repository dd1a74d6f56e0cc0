"""Sparse import and export from device arrays: COO, CSR and CSC of a Matrix, indices plus values of
a Vector, over GxB_{Matrix,Vector}_{import,export}_sparse (reference core/matrix.py:885-960 from_coo,
:1057-1133 _from_csx, :543-611 to_coo, :1658-1702 _to_csx; core/vector.py:731, :482).  A device
array is any object with ``__cuda_array_interface__`` such as a torch CUDA tensor; it is read or
written on the library stream in its own index width and value type and never leaves the device.
Host arrays do not come here: they keep the typed entry points.  Argument errors are raised before
the first library call.

Streams: the library runs on its own stream (``set_stream`` makes it torch's).  Input arrays must
be complete on the device before the call.  An import waits on the new object before it returns, so
the arrays, temporaries included, may be dropped at once; an export drains torch's current stream
before the library writes the tensors torch allocated and waits before it returns them, so they are
complete on any stream.  (The C entry points wait for nothing: there the caller does.)"""
import ctypes

import numpy as np

from ._lib import lib
from .base import _autoname, _Pointer, call
from .dense import _Array
from .dtypes import lookup_dtype

_INDEX_TYPES = (np.dtype(np.int32), np.dtype(np.int64), np.dtype(np.uint64))


class DeviceArray:
    """A device allocation described as a 1-d array of ``np_type``: what ``__cuda_array_interface__``
    needs.  Re-describes a tensor's bytes, e.g. an int64 tensor as uint64 indices."""

    def __init__(self, owner, np_type, size=None, ptr=None):
        self.owner = owner
        np_type = np.dtype(np_type)
        if ptr is None:
            ptr = owner.data_ptr()
        if size is None:
            size = owner.numel() * owner.element_size() // np_type.itemsize
        self.__cuda_array_interface__ = {"shape": (int(size),), "typestr": np_type.str, "data": (int(ptr), False),
                                         "version": 3, "strides": None}


def is_device(x):
    return hasattr(x, "__cuda_array_interface__")


def _is_scalar(values):
    """a Python or numpy scalar, a 0-d numpy array included"""
    return not is_device(values) and np.ndim(values) == 0


def any_device(*arrays):
    """True when the call takes the device path: some array lives on the device.  Mixing raises."""
    if not any(is_device(a) for a in arrays):  # a host call: nothing else is looked at
        return False
    if not all(is_device(a) for a in arrays if not _is_scalar(a)):
        raise ValueError("host and device arrays cannot be mixed: every index and value array must live on "
                         "the device (a Python scalar is accepted for the values)")
    return True


def _index(x, argname):
    a = _Array(x, argname)
    if len(a.shape) != 1:
        raise ValueError(f"`{argname}` must be one-dimensional")
    if a.np_type not in _INDEX_TYPES:
        raise TypeError(f"`{argname}` on the device must be int32, int64 or uint64, not {a.np_type}")
    return a


def _same_index_type(a, b, names):
    if a.np_type != b.np_type:
        raise TypeError(f"{names} must have the same dtype, not {a.np_type} and {b.np_type}")


def _values(values, dtype):
    """(the values as an _Array or None for a Python scalar, their DataType)"""
    from .matrix import _values_dtype

    if _is_scalar(values):
        return None, _values_dtype(values, dtype)
    a = _Array(values, "values")
    if len(a.shape) != 1:
        raise ValueError("`values` must be one-dimensional")
    return a, lookup_dtype(a.np_type)


def _scalar_array(value, dt, like):
    """a Python scalar as a one-element device array of type dt next to ``like``: it imports as iso"""
    import torch

    device = getattr(like.obj, "device", None)
    if not isinstance(device, torch.device):
        device = getattr(getattr(like.obj, "owner", None), "device", "cuda")
    one = torch.from_numpy(np.asarray(value, dt.np_type).reshape(1)).to(device)
    torch.cuda.current_stream(one.device).synchronize()  # produced before the library stream reads it
    return _Array(DeviceArray(one, dt.np_type, 1), "values")


def _imported(obj, *arrays):
    """The library stream may still be reading the arrays when the call returns, and a temporary
    such as ``torch.ones(E)``, or the one-element array of a scalar, is freed as soon as the caller
    lets go of it: the object is waited on first, with the arrays still referenced here."""
    obj.wait()


def _required(value, argname, method):
    if value is None:
        raise ValueError(f"`{argname}` must be given in {method} with device arrays: a dimension is not "
                         "inferred from indices on the device")
    return int(value)


def _new(cls, dt, name):
    C = cls.__new__(cls)
    C.dtype = dt
    C.name = _autoname("M" if cls.ndim == 2 else "v") if name is None else name
    C._h = ctypes.c_void_p()
    return C


def _dup_arg(dup_op, dt):
    from .matrix import _binary_for

    return None if dup_op is None else _binary_for(dup_op, dt)


_DUP_SCALAR = ("dup_op must be None if values is a scalar so that all values can be identical.  "
               "Duplicate indices will be ignored.")
_DUP_NEEDED = "Duplicate indices found, must provide `dup_op` BinaryOp"


# ---------------------------------------------------------------------- import
def matrix_from_coo(cls, rows, columns, values, dtype, nrows, ncols, dup_op, name, method="from_coo", *, into=None,
                    clear=False):
    """``into``: the Matrix whose ``build`` this is; it takes the storage of the imported object"""
    I, J = _index(rows, "rows"), _index(columns, "columns")
    _same_index_type(I, J, "`rows` and `columns`")
    nrows, ncols = _required(nrows, "nrows", method), _required(ncols, "ncols", method)
    X, xdt = _values(values, dtype)
    scalar = X is None
    if scalar and dup_op is not None:
        raise ValueError(_DUP_SCALAR)
    n = I.shape[0]
    if J.shape[0] != n or (not scalar and X.shape[0] != n):
        raise ValueError("`rows` and `columns` and `values` lengths must match: "
                         f"{n}, {J.shape[0]}, {n if scalar else X.shape[0]}")
    dt = xdt if dtype is None else lookup_dtype(dtype)
    dup = _dup_arg(dup_op, dt)
    if scalar:
        X = _scalar_array(values, xdt, I)
    C = _new(cls, dt, name)
    C._nrows, C._ncols = nrows, ncols
    if into is not None:
        ready_to_build(into, clear, (nrows, ncols))
    call("GxB_Matrix_import_sparse",
         [_Pointer(C), dt, nrows, ncols, I.address("rows"), J.address("columns"), X.address("values"),
          lookup_dtype(I.np_type), xdt, n, n, X.shape[0], lib.GrB_COO_FORMAT, dup, True])
    if into is not None:
        take_storage(into, C)
        C = into
    _imported(C, I, J, X)
    if dup_op is None and not scalar and C.nvals < n:
        raise ValueError(_DUP_NEEDED)
    return C


def matrix_from_csx(cls, indptr, indices, values, dtype, nrows, ncols, name, *, by_col):
    method, iname = ("from_csc", "row_indices") if by_col else ("from_csr", "col_indices")
    P, J = _index(indptr, "indptr"), _index(indices, iname)
    _same_index_type(P, J, f"`indptr` and `{iname}`")
    if P.shape[0] < 1:
        raise ValueError("`indptr` must hold at least one entry")
    major = P.shape[0] - 1
    if by_col:
        if ncols is not None and int(ncols) != major:
            raise ValueError(f"ncols must be None or equal to len(indptr) - 1; expected {major}, got {ncols}")
        nrows, ncols = _required(nrows, "nrows", method), major
    else:
        if nrows is not None and int(nrows) != major:
            raise ValueError(f"nrows must be None or equal to len(indptr) - 1; expected {major}, got {nrows}")
        nrows, ncols = major, _required(ncols, "ncols", method)
    X, xdt = _values(values, dtype)
    dt = xdt if dtype is None else lookup_dtype(dtype)
    scalar = X is None
    if scalar:
        X = _scalar_array(values, xdt, P)
    C = _new(cls, dt, name)
    C._nrows, C._ncols = nrows, ncols
    call("GxB_Matrix_import_sparse",
         [_Pointer(C), dt, nrows, ncols, P.address("indptr"), J.address(iname), X.address("values"),
          lookup_dtype(P.np_type), xdt, P.shape[0], J.shape[0], X.shape[0],
          lib.GrB_CSC_FORMAT if by_col else lib.GrB_CSR_FORMAT, None, True])
    _imported(C, P, J, X)
    return C


def vector_from_coo(cls, indices, values, dtype, size, dup_op, name, method="from_coo", *, into=None, clear=False):
    I = _index(indices, "indices")
    size = _required(size, "size", method)
    X, xdt = _values(values, dtype)
    scalar = X is None
    if scalar and dup_op is not None:
        raise ValueError(_DUP_SCALAR)
    n = I.shape[0]
    if not scalar and X.shape[0] != n:
        raise ValueError(f"`indices` and `values` lengths must match: {n}, {X.shape[0]}")
    dt = xdt if dtype is None else lookup_dtype(dtype)
    dup = _dup_arg(dup_op, dt)
    if scalar:
        X = _scalar_array(values, xdt, I)
    v = _new(cls, dt, name)
    v._size = size
    if into is not None:
        ready_to_build(into, clear, (size,))
    call("GxB_Vector_import_sparse",
         [_Pointer(v), dt, size, I.address("indices"), X.address("values"), lookup_dtype(I.np_type), xdt, n,
          X.shape[0], dup, True])
    if into is not None:
        take_storage(into, v)
        v = into
    _imported(v, I, X)
    if dup_op is None and not scalar and v.nvals < n:
        raise ValueError(_DUP_NEEDED)
    return v


def ready_to_build(obj, clear, shape):
    """what ``obj.build`` does before it builds, once the arguments are known to be good"""
    from .exceptions import OutputNotEmpty

    if clear:
        obj.clear()
    if shape != obj.shape:
        obj.resize(*shape)
    if obj.nvals:
        raise OutputNotEmpty("output is not empty")


def take_storage(obj, T):
    """``obj.build`` from device arrays: the import made T, of obj's type and shape, and obj takes its
    storage (a build needs an empty output, so nothing of obj is lost; T frees what obj had)"""
    obj._h, T._h = T._h, obj._h


# ---------------------------------------------------------------------- export
def _torch_dtype(np_type):
    import torch

    return getattr(torch, np.dtype(np_type).name if np.dtype(np_type) != np.bool_ else "bool")


def _index_dtype(index_dtype):
    t = np.dtype(index_dtype)
    if t not in (np.dtype(np.int32), np.dtype(np.int64)):
        raise TypeError(f"index_dtype must be int64 or int32, not {index_dtype}")
    return t


class _Out:
    """a torch tensor to be written (or none: NULL) as a C argument"""

    def __init__(self, n, np_type, want, exc_arg):
        import torch

        self.tensor = torch.empty(n, dtype=_torch_dtype(np_type), device="cuda") if want else None
        self._exc_arg = exc_arg
        self.name = "out"

    @property
    def _carg(self):
        return ctypes.c_void_p(self.tensor.data_ptr() if self.tensor is not None and self.tensor.numel() else None)


def _before_export():
    """The output tensors come from torch's allocator on torch's current stream, which may still be
    using the blocks it hands out: that stream is drained before the library stream writes them."""
    import torch

    torch.cuda.current_stream().synchronize()


def matrix_export(A, fmt, dtype, index_dtype, want):
    """(pointer or rows, indices, values) of Matrix A as torch CUDA tensors; want: which of the three.
    The tensors are complete when this returns: the library stream is waited on, so they can be used
    on any stream."""
    it = _index_dtype(index_dtype)
    dt = A.dtype if dtype is None else lookup_dtype(dtype)
    nz = A.nvals
    np_len = {"coo": nz, "csr": A._nrows + 1, "csc": A._ncols + 1}[fmt]
    outs = [_Out(np_len, it, want[0], A), _Out(nz, it, want[1], A), _Out(nz, dt.np_type, want[2], A)]
    lens = [ctypes.c_uint64(np_len), ctypes.c_uint64(nz), ctypes.c_uint64(nz)]
    _before_export()
    call("GxB_Matrix_export_sparse",
         outs + [lookup_dtype(it), dt] + [ctypes.byref(x) for x in lens] +
         [{"coo": lib.GrB_COO_FORMAT, "csr": lib.GrB_CSR_FORMAT, "csc": lib.GrB_CSC_FORMAT}[fmt], A, True])
    A.wait()
    return tuple(o.tensor for o in outs)


def vector_export(v, dtype, index_dtype, want):
    it = _index_dtype(index_dtype)
    dt = v.dtype if dtype is None else lookup_dtype(dtype)
    nz = v.nvals
    outs = [_Out(nz, it, want[0], v), _Out(nz, dt.np_type, want[1], v)]
    lens = [ctypes.c_uint64(nz), ctypes.c_uint64(nz)]
    _before_export()
    call("GxB_Vector_export_sparse",
         outs + [lookup_dtype(it), dt] + [ctypes.byref(x) for x in lens] + [v, True])
    v.wait()
    return tuple(o.tensor for o in outs)
