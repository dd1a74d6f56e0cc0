"""A dense numpy model of GrB_apply with a builtin index-unary operator, written from the
GraphBLAS C API 2.0 text (GrB_apply, the index-unary operator variants, and the table of the
predefined index-unary operators), not from the kernels:

    T(i, j) = f(A(i, j), i, j, s)   for every stored A(i, j) -- also where the result is 0 / false

    ROWINDEX_<T>   z = i + s            T in INT32, INT64; s is cast to T, the sum is taken in
    COLINDEX_<T>   z = j + s            64 bits and cast to T as C casts (INT32 wraps)
    DIAGINDEX_<T>  z = j - i + s
    TRIL  j <= i + s    TRIU  j >= i + s    DIAG  j == i + s    OFFDIAG  j != i + s
    COLLE j <= s        COLGT j > s         ROWLE i <= s        ROWGT    i > s      (s cast to INT64)
    VALUEEQ_<T> .. VALUELE_<T>   the entry and s cast to T, compared (a NaN compares false, except NE)

The predicates give BOOL.  A vector entry is at (i, 0).  An object is the ``(present, values)``
pair of tests/dense_model.py; the output side is dense_model.write_back's business.
"""
import numpy as np

import dense_model as dm

INDEX = ("rowindex", "colindex", "diagindex")
POSITIONAL = ("tril", "triu", "diag", "offdiag", "colle", "colgt", "rowle", "rowgt")
VALUE = {"valueeq": np.equal, "valuene": np.not_equal, "valuegt": np.greater, "valuege": np.greater_equal,
         "valuelt": np.less, "valuele": np.less_equal}


def thunk_as(y, dtype):
    """the scalar y (a numpy scalar or a Python number, typed as numpy types it) cast to dtype"""
    return dm.cast(np.atleast_1d(np.asarray(y)), dtype)[0]


def index_apply(A, op, optype, y):
    """-> (present, result): op is the operator's lower-case name, optype its type suffix ("INT32" /
    "INT64" for the index-valued operators, the value type for VALUE*, None for TRIL .. ROWGT)"""
    p, v = A
    if p.ndim == 1:
        I, J = np.arange(p.shape[0], dtype=np.int64), np.zeros(p.shape[0], np.int64)
    else:
        I, J = (a.astype(np.int64) for a in np.indices(p.shape))
    if op in INDEX:
        assert optype in ("INT32", "INT64")
        s = np.int64(thunk_as(y, optype))
        base = {"rowindex": I, "colindex": J, "diagindex": J - I}[op]
        with np.errstate(over="ignore"):
            z = dm.cast(base + s, optype)  # the int64 sum wraps; int64 -> int32 keeps the low bits
        zero = dm.NP[optype](0)
    elif op in POSITIONAL:
        assert optype is None
        # indices are below 2^60: beyond +-2^61 every thunk decides alike, and i + s cannot overflow
        s = np.int64(min(max(int(thunk_as(y, "INT64")), -2**61), 2**61))
        z = {"tril": lambda: J <= I + s, "triu": lambda: J >= I + s, "diag": lambda: J == I + s,
             "offdiag": lambda: J != I + s, "colle": lambda: J <= s, "colgt": lambda: J > s,
             "rowle": lambda: I <= s, "rowgt": lambda: I > s}[op]()
        zero = False
    else:
        x, s = dm.cast(v, optype), thunk_as(y, optype)
        with np.errstate(invalid="ignore"):
            z = VALUE[op](x, s)
        zero = False
    return p.copy(), np.where(p, z, zero)


def result_dtype(op, optype):
    return optype if op in INDEX else "BOOL"
