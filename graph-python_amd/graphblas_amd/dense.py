"""Dense import and export: ``from_dense`` / ``to_dense`` of Matrix and Vector over
GxB_{Matrix,Vector}_{import,export}_dense (reference core/matrix.py:1457-1574,
core/vector.py:894-999).  An array is a numpy array (host) or any object with
``__cuda_array_interface__`` such as a torch CUDA tensor (device, read or written on the library
stream); a C-ordered array goes in as it is and an F-ordered one with ``by_col``, so neither is
copied on the host.  Argument errors are raised before the first library call."""
import ctypes

import numpy as np

from .base import _autoname, _Pointer, call
from .dtypes import lookup_dtype, unify

_BITMAP_TYPES = (np.dtype(np.bool_), np.dtype(np.int8), np.dtype(np.uint8))


class _Address:
    """A host or device address as a C argument (0 -> NULL); errors are read from ``exc_arg``."""

    __slots__ = "ptr", "name", "keep", "_exc_arg"

    def __init__(self, ptr, name, keep, exc_arg=None):
        self.ptr, self.name, self.keep, self._exc_arg = ptr, name, keep, exc_arg

    @property
    def _carg(self):
        return ctypes.c_void_p(self.ptr or None)


class _Array:
    """What the C entry points need to know of a host or device array"""

    __slots__ = "ptr", "shape", "order", "np_type", "on_device", "obj"

    def __init__(self, x, argname):
        self.obj = x
        self.on_device = hasattr(x, "__cuda_array_interface__")
        if self.on_device:
            d = x.__cuda_array_interface__
            self.np_type = np.dtype(d["typestr"])
            self.shape = tuple(int(n) for n in d["shape"])
            self.ptr = int(d["data"][0] or 0)
            strides = d.get("strides")
        elif isinstance(x, np.ndarray):
            self.np_type, self.shape, self.ptr, strides = x.dtype, x.shape, x.ctypes.data, x.strides
        else:
            raise TypeError(f"Bad type for argument `{argname}`: expected a numpy array or a device array "
                            f"(__cuda_array_interface__), got {type(x).__name__}")
        self.order = _strides_order(self.shape, strides, self.np_type.itemsize)
        if self.order is None:
            raise ValueError(f"`{argname}` must be C- or F-contiguous")

    def address(self, name, exc_arg=None):
        return _Address(self.ptr, name, self.obj, exc_arg)


def _strides_order(shape, strides, itemsize):
    """"C", "F" (an array that is both counts as "C") or None for strides in bytes"""
    if strides is None or 0 in shape:
        return "C"

    def contiguous(dims):
        expected = itemsize
        for n, stride in dims:
            if n != 1 and stride != expected:
                return False
            expected *= n
        return True

    if contiguous(zip(shape[::-1], strides[::-1])):
        return "C"
    return "F" if contiguous(zip(shape, strides)) else None


def _check_ndim(kind, ndim, dtype_name):
    """the reference's argument errors (core/matrix.py:1486-1496, core/vector.py:924-932)"""
    want = 2 if kind == "Matrix" else 1
    if ndim == 0:
        raise TypeError("values must be an array or list, not a scalar. "
                        f"To create a dense {kind} from a scalar, use `{kind}.from_scalar`.")
    if kind == "Matrix" and ndim == 1:
        raise ValueError("A 2d array or scalar is required to create a dense Matrix")
    if ndim > want:
        raise ValueError(f"values array must be {want}d to create dense {kind} with dtype {dtype_name}")


def _scalar_arg(value, keyword, within):
    """None, a Scalar as it is, or a literal as a Scalar of its own type"""
    from .scalar import Scalar

    if value is None or isinstance(value, Scalar):
        return value
    try:
        a = np.asarray(value)
        if a.ndim != 0 or a.dtype == object:
            raise TypeError("not a scalar")
        dtype = lookup_dtype(a.dtype)
    except (TypeError, ValueError) as exc:
        raise TypeError(f"Bad type for keyword argument `{keyword}` in {within}: expected Scalar, got "
                        f"{type(value).__name__}.  Literal scalars also accepted.") from exc
    return Scalar.from_value(a.item(), dtype)


def _scalar_dtype(value, keyword, within):
    """the type `_scalar_arg` gives the value, without building the Scalar"""
    from .scalar import Scalar

    if isinstance(value, Scalar):
        return value.dtype
    try:
        a = np.asarray(value)
        if a.ndim != 0 or a.dtype == object:
            raise TypeError("not a scalar")
        return lookup_dtype(a.dtype)
    except (TypeError, ValueError) as exc:
        raise TypeError(f"Bad type for keyword argument `{keyword}` in {within}: expected Scalar, got "
                        f"{type(value).__name__}.  Literal scalars also accepted.") from exc


def _bitmap_array(bitmap, like, argname="bitmap"):
    """`bitmap` as an _Array of `like`'s shape, order and residence (a host array is converted)"""
    if bitmap is None:
        return None
    if not hasattr(bitmap, "__cuda_array_interface__"):
        if like.on_device:
            raise ValueError(f"`{argname}` must live where the values do: on the device")
        bitmap = np.asarray(bitmap)
        if bitmap.dtype not in _BITMAP_TYPES:
            raise TypeError(f"`{argname}` must be bool, int8 or uint8, not {bitmap.dtype}")
        if bitmap.shape == like.shape:
            bitmap = np.asfortranarray(bitmap) if like.order == "F" else np.ascontiguousarray(bitmap)
    elif not like.on_device:
        raise ValueError(f"`{argname}` must live where the values do: on the host")
    b = _Array(bitmap, argname)
    if b.np_type not in _BITMAP_TYPES:
        raise TypeError(f"`{argname}` must be bool, int8 or uint8, not {b.np_type}")
    if b.shape != like.shape:
        raise ValueError(f"`{argname}` of shape {b.shape} does not match the values' shape {like.shape}")
    if b.order != like.order:
        raise ValueError(f"`{argname}` must be in the same order ({like.order}) as the values")
    return b


def _both_orders(shape):
    """a shape whose C and F layouts are the same memory"""
    return sum(n != 1 for n in shape) <= 1 or 0 in shape


def from_dense(cls, values, missing_value, dtype, name, bitmap):
    from .matrix import _values_dtype

    kind = "Matrix" if cls.ndim == 2 else "Vector"
    if hasattr(values, "__cuda_array_interface__"):
        ndim = len(values.__cuda_array_interface__["shape"])
        _check_ndim(kind, ndim, dtype if dtype is not None else "of the array")
        X = _Array(values, "values")
        dt = lookup_dtype(X.np_type)
    else:
        a = values if isinstance(values, np.ndarray) else np.asarray(values)
        dt = _values_dtype(a, dtype)
        _check_ndim(kind, a.ndim, dt)
        a = np.asarray(a, dt.np_type)
        if not (a.flags.c_contiguous or a.flags.f_contiguous):
            a = np.ascontiguousarray(a)
        X = _Array(a, "values")
    Ab = _bitmap_array(bitmap, X)
    m = _scalar_arg(missing_value, "missing_value", "from_dense")
    by_col = X.order == "F"
    C = cls.__new__(cls)
    C.dtype = dt
    C.name = _autoname("M" if cls.ndim == 2 else "v") if name is None else name
    C._h = ctypes.c_void_p()
    ab = None if Ab is None else Ab.address("bitmap")
    if cls.ndim == 2:
        C._nrows, C._ncols = X.shape
        call("GxB_Matrix_import_dense", [_Pointer(C), dt, C._nrows, C._ncols, X.address("values"), ab, m, by_col,
                                         X.on_device])
    else:
        C._size = X.shape[0]
        call("GxB_Vector_import_dense", [_Pointer(C), dt, C._size, X.address("values"), ab, m, X.on_device])
    if dtype is not None and lookup_dtype(dtype) != dt:  # a device array is imported in its own type
        C = C.dup(dtype, name=name)
    return C


def to_dense(x, fill_value, dtype, out, bitmap, *, upcast):
    """x: Matrix, TransposedMatrix or Vector.  upcast: a fill value's type can widen the result type."""
    src = x._matrix if getattr(x, "_is_transposed", False) else x
    transposed = src is not x
    shape = x.shape
    want = None if dtype is None else lookup_dtype(dtype)
    O = None
    if out is not None:
        O = _Array(out, "out")
        if O.shape != shape:
            raise ValueError(f"`out` of shape {O.shape} does not match the shape {shape}")
        out_dt = lookup_dtype(O.np_type)
        if want is not None and want != out_dt:
            raise TypeError(f"dtype={want} conflicts with the dtype of `out`, {out_dt}")
        want = out_dt
    fill_dt = None if fill_value is None else _scalar_dtype(fill_value, "fill_value", "to_dense")
    B = None
    if bitmap is not None:
        if not hasattr(bitmap, "__cuda_array_interface__") and not isinstance(bitmap, np.ndarray):
            raise TypeError("`bitmap` must be a numpy array or a device array to write into")
        B = _Array(bitmap, "bitmap")
        if B.np_type not in _BITMAP_TYPES:
            raise TypeError(f"`bitmap` must be bool, int8 or uint8, not {B.np_type}")
        if B.shape != shape:
            raise ValueError(f"`bitmap` of shape {B.shape} does not match the shape {shape}")
        if B.on_device != (O is not None and O.on_device):
            raise ValueError("`bitmap` must live where `out` does (the host, without `out`)")
        if B.order != (O.order if O is not None else "C") and not _both_orders(shape):
            raise ValueError("`bitmap` must be in the same order as `out` (C, without `out`)")
    # ---- from here on, library calls
    npos = int(np.prod(shape, dtype=object)) if shape else 1
    full = src.nvals == npos
    if fill_value is None and B is None and not full:
        raise TypeError("fill_value must be given in `to_dense` when there are missing values")
    if want is None:  # as the reference: the fill of a full object is never used
        want = unify(fill_dt, src.dtype, is_left_scalar=True) if upcast and fill_dt is not None and not full \
            else src.dtype
    if O is None:
        result = np.empty(shape, want.np_type)
        O = _Array(result, "out")
    else:
        result = out
    if want != src.dtype:
        src = src.dup(want)
    fill = _scalar_arg(fill_value, "fill_value", "to_dense")
    ab = None if B is None else B.address("bitmap")
    X = O.address("out", src)
    if x.ndim == 2:
        by_col = transposed != (O.order == "F")
        call("GxB_Matrix_export_dense", [X, ab, src, fill, by_col, O.on_device])
    else:
        call("GxB_Vector_export_dense", [X, ab, src, fill, O.on_device])
    return result


def from_scalar(cls, value, dims, dtype, name):
    """an iso-full object by the scalar assign (reference core/matrix.py:1432-1455, core/vector.py:871-892)"""
    from .scalar import Scalar

    if not isinstance(value, Scalar):
        dt = _scalar_dtype(value, "value", "from_scalar") if dtype is None else lookup_dtype(dtype)
        value = np.asarray(value, dt.np_type).item()
    else:
        dt = value.dtype if dtype is None else lookup_dtype(dtype)
    C = cls(dt, *dims, name=name)
    C[...] = value
    return C
