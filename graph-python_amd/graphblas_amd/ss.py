"""``Vector.ss`` / ``Matrix.ss`` extension namespaces: the prefix scan, sort, split and concat.

``scan`` is one call of GxB_Matrix_scan / GxB_Vector_scan (csrc/gb_scan.hip): a segmented
inclusive scan of every row (column, vector) under a monoid, in the monoid's type; nothing goes
through the host.  Its association order (include/graphblas_amd.h) is that of ``prefix_scan``
below, so both return the same bits, floats included.

``prefix_scan`` is the recipe ``scan`` replaced, kept as a public function and as the parity
check of the device call.  It restates reference core/ss/prefix_scan.py:12-172: a
Blelloch up-sweep / down-sweep expressed entirely as masked, accumulated
``mxm`` / ``vxm`` calls with the semiring ``<monoid>_first`` against small
iso selection matrices (one per level, log2(N) levels), on the entries of
each row compacted to positions 0..deg-1.  Every level is one library call;
compaction / de-compaction of the index space goes through to_coo / from_coo
(the reference uses the ss export / import of the same arrays).

``sort`` is one call of GxB_Matrix_sort / GxB_Vector_sort (csrc/gb_sort.hip): a
segmented sort on the device, nothing goes through the host.  The k largest
entries of every row are ``C, P = A.ss.sort(">")`` followed by
``C.select("col<=", k - 1)`` (and the same select of ``P`` for where they came from).

``selectk`` / ``compactify`` are one call of GxB_*_selectk / GxB_*_compactify (csrc/gb_selectk.hip):
up to k entries of every row, chosen by position, by value or at random, kept in place or moved to
the left; the k largest of every row with their columns are ``A.ss.compactify("largest", k)`` and
``A.ss.compactify("largest", k, asindex=True)``, without sorting or writing the rest of the row.

``split`` / ``concat`` are one call of GxB_Matrix_split / GxB_Matrix_concat (csrc/gb_tile.hip)
whatever the number of tiles; vectors go through the same two entry points as N x 1 objects, as
in the reference (core/ss/matrix.py:281-381, core/ss/vector.py:185-265, ss/_core.py:73-107).

``diag`` / ``build_diag`` / ``reshape`` / ``flatten`` are one call each of GxB_Matrix_diag,
GxB_Vector_diag, GxB_Matrix_reshape[Dup] and GxB_Vector_flatten (csrc/gb_reindex.hip): the values
stay on the device and only their indices change (reference ss/_core.py:24-70,
core/ss/matrix.py:252-279, 3717-3815, core/ss/vector.py:147-183, 1377-1405).
"""
import ctypes
from math import ceil, log2

import numpy as np

from . import operator as _op
from .base import call, descriptor_lookup
from .dtypes import INT8, UINT64, lookup_dtype, unify


def _scan_monoid(x, op):
    t = _op.get_typed_op(op, x.dtype, kind="monoid")
    if t.opclass == "BinaryOp":
        mon = getattr(_op.monoid, t.parent.name, None)
        if mon is None or t.type not in mon._typed:
            raise TypeError(f"Bad type for argument `op` in scan: {op!r} is a BinaryOp with no Monoid")
        t = mon[t.type]
    if t.opclass != "Monoid":
        raise TypeError(f"Bad type for argument `op` in scan: expected Monoid, got {t.opclass}")
    return t


def _iso_pattern(rows, cols, nrows, ncols, name):
    from .matrix import Matrix

    return Matrix.from_coo(np.asarray(rows, np.uint64), np.asarray(cols, np.uint64), 1, dtype=INT8,
                           nrows=nrows, ncols=ncols, name=name)


def prefix_scan(A, op, *, name=None):
    from .matrix import Matrix, TransposedMatrix
    from .vector import Vector

    mon = _scan_monoid(A, op)
    mname = mon.parent.name
    semiring = getattr(_op.semiring, f"{'lxnor' if mname == 'eq' else mname}_first")[mon.type]
    accum = getattr(_op.binary, "lxnor" if mname == "eq" else mname)[mon.type]
    is_vector = A.ndim == 1
    is_transposed = isinstance(A, TransposedMatrix)
    if A.shape[-1] < 2:
        return A.T.dup(name=name) if is_transposed else A.dup(name=name)

    # compact every row to positions 0..deg-1 (reference prefix_scan.py:36-63)
    if is_vector:
        idx, vals = A.to_coo()
        n_cols = len(idx)
        Ac = Vector.from_coo(np.arange(n_cols, dtype=np.uint64), vals, dtype=A.dtype, size=n_cols)
    else:
        rows, cols, vals = A.to_coo()
        nr = A.nrows
        rows64 = rows.astype(np.int64)
        deg = np.bincount(rows64, minlength=nr)
        start = np.zeros(nr + 1, np.int64)
        np.cumsum(deg, out=start[1:])
        pos = np.arange(len(rows64), dtype=np.int64) - start[rows64]
        n_cols = int(deg.max()) if len(deg) else 0
        Ac = Matrix.from_coo(rows, pos.astype(np.uint64), vals, dtype=A.dtype, nrows=nr, ncols=max(n_cols, 1))
    if n_cols < 2:
        return A.T.dup(name=name) if is_transposed else A.dup(name=name)
    n_half = n_cols // 2

    def mul(X, S):
        return X.vxm(S, semiring) if is_vector else X.mxm(S, semiring)

    # first iteration: pairwise sums (reference :75-92)
    j = np.arange(n_half)
    S = _iso_pattern(np.stack([2 * j, 2 * j + 1], 1).ravel(), np.repeat(j, 2), n_cols, n_half, "Up_0")
    B = mul(Ac, S).new(name="B")
    mask = None if is_vector else B.S

    # up-sweep (reference :94-116)
    stride, stride2 = 1, 2
    while stride2 <= n_half:
        c = np.arange(stride2 - 1, n_half, stride2)
        S = _iso_pattern(c - stride, c, n_half, n_half, "Up")
        B(accum, mask=mask) << mul(B, S)
        stride, stride2 = stride2, stride2 * 2

    # down-sweep (reference :118-146)
    if n_half > 2:
        stride2 = max(2, 2 ** ceil(log2(n_half // 2)))
        stride = stride2 // 2
        while stride > 0:
            c = np.arange(stride2 + stride - 1, n_half, stride2)
            if c.size == 0:
                stride2 = stride
                stride //= 2
                continue
            S = _iso_pattern(c - stride, c, n_half, n_half, "Down")
            B(accum, mask=mask) << mul(B, S)
            stride2 = stride
            stride //= 2

    # last iteration: spread to odd positions, then add the even originals (reference :148-170)
    indptr = np.arange(0, 2 * n_half + 2, 2)
    indptr[-1] = n_cols - 1
    lr = np.repeat(np.arange(n_half), np.diff(indptr))
    S = _iso_pattern(lr, np.arange(1, n_cols), n_half, n_cols, "Down_last")
    RV = mul(B, S).new(mask=Ac.S, name="RV")
    ev = np.arange(0, n_cols, 2)
    D = _iso_pattern(ev, ev, n_cols, n_cols, "D")
    RV(accum) << mul(Ac, D)

    # de-compact into the input's index space
    if is_vector:
        _, rv = RV.to_coo()
        return Vector.from_coo(idx, rv, dtype=RV.dtype, size=A.size, name=name)
    _, _, rv = RV.to_coo()
    if is_transposed:
        M = A.T
        return Matrix.from_coo(cols, rows, rv, dtype=RV.dtype, nrows=M.nrows, ncols=M.ncols, name=name)
    return Matrix.from_coo(rows, cols, rv, dtype=RV.dtype, nrows=A.nrows, ncols=A.ncols, name=name)


# ---------------------------------------------------------------- split / concat
def _integral(x):
    """``x`` as an int when it is a whole number (int, numpy integer, float without fraction)."""
    if isinstance(x, (int, np.integer)):
        return int(x)
    if isinstance(x, (float, np.floating)) and float(x).is_integer():
        return int(x)
    return None


def _positive(c):
    if c < 0:
        raise ValueError(f"Chunksize must be greater than 0; got: {c}")
    return c


def _dimension_chunks(size, chunk, chunks):
    """The chunk sizes of one dimension of length ``size``."""
    if chunk is None:
        return [size]
    c = _integral(chunk)
    if c is not None:
        _positive(c)
        full, rest = divmod(size, c)
        return [c] * full + ([rest] if rest else [])
    if isinstance(chunk, np.ndarray):
        if not np.issubdtype(chunk.dtype, np.integer):
            raise TypeError(f"numpy array for chunks must be integer dtype; got {chunk.dtype}")
        if chunk.ndim != 1:
            raise TypeError(f"numpy array for chunks must be 1-dimension; got ndim={chunk.ndim}")
        if (chunk < 0).any():
            raise ValueError(f"Chunksize must be greater than 0; got: {chunk[chunk < 0]}")
        return chunk.tolist()
    if not isinstance(chunk, (list, tuple)):
        raise TypeError("Chunks for a dimension must be an integer, a list or tuple of integers, or None."
                        f"  Got: {type(chunk)}")
    sizes, rest_at = [], None
    for item in chunk:
        if item is None:
            if rest_at is not None:
                raise TypeError('None value in chunks for "the rest" can only appear once per dimension')
            rest_at = len(sizes)
            sizes.append(0)
            continue
        c = _integral(item)
        if c is None:
            raise TypeError(f"Bad type for element in chunks; expected int or None, but got: {type(chunks)}")
        sizes.append(_positive(c))
    if rest_at is not None:
        rest = size - sum(sizes)
        if rest < 0:
            raise ValueError("Chunks are too large; None value in chunks would need to be negative "
                             "to match size of input")
        sizes[rest_at] = rest
    return sizes


def normalize_chunks(chunks, shape):
    """The ``chunks`` argument of ``split`` as one list of sizes per dimension of ``shape``
    (behaviour of reference core/utils.py:172-258).  Per dimension: an integer (equal chunks, the
    last one smaller), a list or tuple of sizes with at most one ``None`` for "the rest", ``None``
    (one chunk) or a 1-D integer numpy array; a single integer stands for every dimension.
    Whether the sizes add up to the dimension is the library's check (DimensionMismatch)."""
    whole = _integral(chunks)
    if whole is not None:
        chunks = (whole,) * len(shape)
    elif isinstance(chunks, np.ndarray):
        chunks = chunks.tolist()
    elif not isinstance(chunks, (list, tuple)):
        raise TypeError(f"chunks argument must be a list, tuple, or numpy array; got: {type(chunks)}")
    if len(chunks) != len(shape):
        kind = "Vector" if len(shape) == 1 else "Matrix"
        raise ValueError(f"chunks argument must be of length {len(shape)} (one for each dimension of a {kind})")
    return [_dimension_chunks(size, chunk, chunks) for size, chunk in zip(shape, chunks)]


class _HandleArray:
    """A ``GrB_Matrix[]`` argument; errors of the call are read from ``exc_arg`` when given."""

    def __init__(self, count, name="tiles", exc_arg=None):
        self.array = (ctypes.c_void_p * count)()
        self.name = name
        if exc_arg is not None:
            self._exc_arg = exc_arg

    @property
    def _carg(self):
        return ctypes.cast(self.array, ctypes.c_void_p)


class _IndexArray:
    def __init__(self, values, name):
        self.array = (ctypes.c_uint64 * len(values))(*values)
        self.name = name

    @property
    def _carg(self):
        return ctypes.cast(self.array, ctypes.c_void_p)


def _tile_kind(tile):
    """2 for a Matrix or TransposedMatrix, 1 for a Vector or Scalar, 0 for anything else."""
    from .matrix import Matrix, TransposedMatrix
    from .scalar import Scalar
    from .vector import Vector

    if isinstance(tile, (Matrix, TransposedMatrix)):
        return 2
    return 1 if isinstance(tile, (Vector, Scalar)) else 0


def _tile_shape(tile):
    if _tile_kind(tile) == 2:
        return tile._nrows, tile._ncols
    return getattr(tile, "_size", 1), 1


def _concat_tiles(tiles, is_matrix=None):
    """Check the ``tiles`` argument of a concat: ``(rows of tiles, m, n, is_matrix)``.  A flat
    list of vectors is a vector concat (unless ``is_matrix`` asks for a Matrix), a list of lists
    a matrix concat in which vectors count as N x 1."""
    if not isinstance(tiles, (list, tuple)):
        raise TypeError(f"tiles argument must be list or tuple; got: {type(tiles)}")
    if not tiles:
        raise ValueError("tiles argument must not be empty")
    rows, n = [], None
    for i, row in enumerate(tiles):
        if not isinstance(row, (list, tuple)):
            if is_matrix or _tile_kind(row) != 1:
                raise TypeError(f"tiles must be lists or tuples; got: {type(row)}")
            is_matrix, n = False, 1
            rows.append([row])
            continue
        if is_matrix is False:
            raise TypeError(f"Bad tile type for concat at position {i}")
        is_matrix = True
        if n is None:
            n = len(row)
            if n == 0:
                raise ValueError("tiles must not be empty")
        elif len(row) != n:
            raise ValueError(f"tiles must all be the same length; got tiles of length {n} and {len(row)}")
        for j, tile in enumerate(row):
            if _tile_kind(tile) == 0:
                raise TypeError(f"Bad tile type for concat at position [{i}, {j}]; got: {type(tile)}")
        rows.append(list(row))
    return rows, len(rows), n, is_matrix


def _concat_into(out, rows, m, n):
    """GxB_Matrix_concat of the checked tiles into ``out`` (a Matrix or a Vector)."""
    from .matrix import TransposedMatrix

    ctiles = _HandleArray(m * n)
    keep = []  # materialised transposes live until the call is over
    for i, row in enumerate(rows):
        for j, tile in enumerate(row):
            if isinstance(tile, TransposedMatrix):
                tile = tile.new()
                keep.append(tile)
            ctiles.array[i * n + j] = tile._h.value
    call("GxB_Matrix_concat", [out, ctiles, m, n, None])


def concat(tiles, dtype=None, *, name=None):
    """GxB_Matrix_concat into a new object (reference ss/_core.py:73-107): a list of lists of
    tiles gives a Matrix (vectors inside count as N x 1), a flat list of vectors a Vector.
    ``dtype`` defaults to the type that holds every tile's."""
    from .matrix import Matrix
    from .vector import Vector

    rows, m, n, is_matrix = _concat_tiles(tiles)
    if dtype is None:
        dtype = rows[0][0].dtype
        for row in rows:
            for tile in row:
                dtype = unify(dtype, tile.dtype)
    dtype = lookup_dtype(dtype)
    nrows = sum(_tile_shape(row[0])[0] for row in rows)
    if is_matrix:
        ncols = sum(_tile_shape(tile)[1] for tile in rows[0])
        out = Matrix(dtype, nrows, ncols, name=name)
    else:
        out = Vector(dtype, nrows, name=name)
    _concat_into(out, rows, m, n)
    return out


_ORDERS = {"rowwise": "rowwise", "row": "rowwise", "rows": "rowwise", "c": "rowwise",
           "columnwise": "columnwise", "col": "columnwise", "cols": "columnwise", "column": "columnwise",
           "columns": "columnwise", "f": "columnwise"}


class _NewHandle:
    """``&C`` of an object the call creates; errors of the call are read from ``exc_arg``."""

    def __init__(self, obj, exc_arg):
        self.obj = obj
        self._exc_arg = exc_arg

    @property
    def _carg(self):
        return ctypes.byref(self.obj._h)

    @property
    def name(self):
        return f"&{self.obj.name}"


def _order(order):
    """"rowwise" or "columnwise" for any alias in ``_ORDERS`` (reference core/ss/matrix.py get_order)."""
    key = order.lower() if isinstance(order, str) else order
    if key not in _ORDERS:
        raise ValueError(f"Bad value for order: {order!r}")
    return _ORDERS[key]


def _expect_type(self, x, types, *, within, argname):
    """``x`` if its type is one of ``types``, else the reference's TypeError (core/base.py:57-110)."""
    if not isinstance(types, tuple):
        types = (types,)
    if type(x) in types:
        return x
    owner = self if isinstance(self, str) else type(self).__name__
    raise TypeError(f"Bad type for argument `{argname}` in {owner}.{within}(...).\n"
                    f"    - Expected type: {', '.join(t.__name__ for t in types)}.\n"
                    f"    - Got: {type(x)}.")


def _diag_k(k):
    """The diagonal ``k`` as an int: an integer or a Scalar that holds one (cast as INT64)."""
    from .scalar import Scalar

    if isinstance(k, Scalar):
        k = k.value
        if k is None:
            raise TypeError("k must not be an empty Scalar")
    if isinstance(k, bool) or _integral(k) is None:
        raise TypeError(f"k must be an integer; got: {type(k)}")
    return _integral(k)


def _diag_size(nrows, ncols, k):
    """Length of diagonal ``k`` of an nrows x ncols matrix (reference ss/_core.py:64-67)."""
    if k < 0:
        return max(0, min(nrows + k, ncols))
    return max(0, min(ncols - k, nrows))


def _reshape_shape(shape, nrows, ncols):
    """The (nrows, ncols) a reshape of an object of ``shape`` is asked for: ``-1`` for one of them,
    a tuple as ``nrows``; numpy's own ValueError "cannot reshape array" when the sizes do not fit
    (reference core/ss/matrix.py:3779-3786: the reshape of a broadcast view, which moves nothing)."""
    array = np.broadcast_to(False, shape)
    array = array.reshape(nrows) if ncols is None else array.reshape(nrows, ncols)
    if array.ndim != 2:
        raise ValueError(f"Shape tuple must be of length 2, not {array.ndim}")
    return int(array.shape[0]), int(array.shape[1])


def _reshape_dup(parent, shape, nrows, ncols, order, name):
    """GxB_Matrix_reshapeDup of a Matrix, or of a Vector as size x 1, into a new Matrix."""
    from .base import _autoname
    from .matrix import Matrix

    columnwise = _order(order) == "columnwise"
    nrows, ncols = _reshape_shape(shape, nrows, ncols)
    C = Matrix.__new__(Matrix)
    C.dtype, C.name = parent.dtype, _autoname("M") if name is None else name
    C._h = ctypes.c_void_p()
    C._nrows, C._ncols = nrows, ncols
    call("GxB_Matrix_reshapeDup", [_NewHandle(C, parent), parent, columnwise, nrows, ncols, None])
    return C


def diag(x, k=0, dtype=None, *, name=None, **opts):
    """GxB_Matrix_diag / GxB_Vector_diag into a new object (reference ss/_core.py:24-70): the
    diagonal Matrix of a Vector, or diagonal ``k`` of a Matrix or TransposedMatrix as a Vector."""
    from .matrix import Matrix, TransposedMatrix
    from .vector import Vector

    x = _expect_type("graphblas.ss", x, (Matrix, TransposedMatrix, Vector), within="diag", argname="x")
    k = _diag_k(k)
    descriptor_lookup(**_sort_opts(opts))  # accepted as in the reference, and unused
    dtype = x.dtype if dtype is None else lookup_dtype(dtype)
    if type(x) is Vector:
        size = x._size + abs(k)
        rv = Matrix(dtype, size, size, name=name)
    else:
        rv = Vector(dtype, _diag_size(x._nrows, x._ncols, k), name=name)
    rv.ss.build_diag(x, k)
    return rv


def _sort_op(parent, op):
    """The typed BinaryOp of a sort (reference core/ss/matrix.py:4029-4033): a Monoid gives its
    binary operator; whether it is an order is the library's decision."""
    t = _op.get_typed_op(op, parent.dtype, kind="binary")
    if t.opclass == "Monoid":
        t = t.binaryop[t.type]
    if t.opclass != "BinaryOp":
        raise TypeError(f"Bad type for argument `op` in sort: expected BinaryOp, got {t.opclass}")
    return t


def _sort_opts(opts):
    opts.pop("nthreads", None)  # accepted as in the reference; the device has no thread count
    return opts


_HOWS = {"first": 0, "last": 1, "smallest": 2, "largest": 3, "random": 4}  # GxB_SelectK_How
_SELECTK_HOWS = '`how` argument must be one of: "random", "first", "last", "largest", "smallest"'
_COMPACTIFY_HOWS = '`how` argument must be one of: "first", "last", "smallest", "largest", "random"'


def _how(how, message):
    key = how.lower() if isinstance(how, str) else how
    if key not in _HOWS:
        raise ValueError(message)
    return _HOWS[key]


def _count(k):
    if k < 0:
        raise ValueError("negative k is not allowed")
    return int(k)


def _seed(seed):
    """The 64 bits of the random order: ``seed``, or a draw from ``numpy.random``'s global state
    (so that ``np.random.seed`` governs a run, as it does for the reference)."""
    if seed is None:
        return int(np.random.randint(0, 1 << 64, dtype=np.uint64))
    return int(seed) & ((1 << 64) - 1)


class _IndexOut:
    """A ``GrB_Index *`` result."""

    def __init__(self, name):
        self.value = ctypes.c_uint64()
        self.name = name

    @property
    def _carg(self):
        return ctypes.byref(self.value)


def _scan(parent, op, columnwise, name):
    """GxB_Matrix_scan / GxB_Vector_scan of ``parent`` into a new object of the monoid's type."""
    from .matrix import Matrix
    from .vector import Vector

    mon = _scan_monoid(parent, _op.monoid.plus if op is None else op)
    dtype = lookup_dtype(mon.type)
    is_vector = parent.ndim == 1
    desc = None if is_vector else descriptor_lookup(transpose_first=columnwise)
    if dtype != parent.dtype:
        # prefix_scan returns a dup, in the input's type, when nothing is folded: fewer than two
        # positions along the scan, or no row with two entries.  Only here can that type show.
        along = parent._size if is_vector else parent._nrows if columnwise else parent._ncols
        longest = 0
        if along >= 2:
            if is_vector:
                longest = parent.nvals
            else:
                width = _IndexOut("&k")
                call("GxB_Matrix_compactify_width", [width, parent, desc])
                longest = width.value.value
        if longest < 2:
            return parent.dup(name=name)
    if is_vector:
        out = Vector(dtype, parent._size, name=name)
        call("GxB_Vector_scan", [out, mon, parent, desc])
    else:
        out = Matrix(dtype, parent._nrows, parent._ncols, name=name)
        call("GxB_Matrix_scan", [out, mon, parent, desc])
    return out


class VectorSS:
    def __init__(self, parent):
        self._parent = parent

    def scan(self, op=None, *, name=None):
        """GxB_Vector_scan (reference core/ss/vector.py:1365-1375): the inclusive prefix scan of the
        entries in index order under a monoid (default plus), in the monoid's type."""
        return _scan(self._parent, op, False, name)

    def sort(self, op=_op.binary.lt, *, values=True, permutation=True, **opts):
        """GxB_Vector_sort (reference core/ss/vector.py:1562-1617): ``(w, p)``, the values in
        the order of ``op`` (ties by ascending index) at positions 0 .. nvals-1 and the indices
        they came from; an output that was not requested is ``None``."""
        from .vector import Vector

        parent = self._parent
        op = _sort_op(parent, op)
        desc = descriptor_lookup(**_sort_opts(opts))
        if not values and not permutation:
            return None, None
        w = Vector(parent.dtype, parent.size, name="Values") if values else None
        p = Vector(UINT64, parent.size, name="Permutation") if permutation else None
        call("GxB_Vector_sort", [w, p, op, parent, desc])
        return w, p

    def selectk(self, how, k, *, seed=None, name=None):
        """GxB_Vector_selectk (reference core/ss/vector.py:1407-1454): up to ``k`` entries, each at
        its own index.  ``how``: "first", "last", "smallest", "largest" (ties by position, see
        include/graphblas_amd.h) or "random" (a uniform k-subset; ``seed`` reproduces it)."""
        from .vector import Vector

        parent = self._parent
        how = _how(how, _SELECTK_HOWS)
        k = _count(k)
        w = Vector(parent.dtype, parent._size, name=name)
        call("GxB_Vector_selectk", [w, parent, how, k, _seed(seed), None])
        return w

    def compactify(self, how="first", size=None, *, reverse=False, asindex=False, seed=None, name=None):
        """GxB_Vector_compactify (reference core/ss/vector.py:1456-1560): the entries moved to
        positions 0 .. in the order of ``how`` (reversed if ``reverse``), as values or, with
        ``asindex``, as the indices they came from (UINT64), in a new Vector of ``size`` positions
        (default: nvals).  "random" emits its choice in ascending index and ignores ``reverse``."""
        from .vector import Vector

        parent = self._parent
        how = _how(how, _COMPACTIFY_HOWS)
        dtype = UINT64 if asindex else parent.dtype
        if size is None:
            size = parent.nvals
        size = _count(size)
        w = Vector(dtype, size, name=name)
        if size:
            call("GxB_Vector_compactify", [w, parent, how, size, bool(reverse), bool(asindex), _seed(seed), None])
        return w

    def split(self, chunks, *, name=None):
        """GxB_Matrix_split of the vector as N x 1 (reference core/ss/vector.py:185-234): a list
        of Vectors named ``f"{name}_{i}"``.  ``chunks``: see ``normalize_chunks``."""
        from .vector import Vector

        parent = self._parent
        sizes, _ = normalize_chunks([chunks, None], (parent._size, 1))
        m = len(sizes)
        tiles = _HandleArray(m, exc_arg=parent)
        call("GxB_Matrix_split", [tiles, m, 1, _IndexArray(sizes, "Tile_nrows"), _IndexArray([1], "Tile_ncols"),
                                  parent, None])
        name = parent.name if name is None else name
        out = []
        for i, size in enumerate(sizes):
            w = Vector.__new__(Vector)
            w.dtype, w.name, w._size = parent.dtype, f"{name}_{i}", size
            w._h = ctypes.c_void_p(tiles.array[i])
            out.append(w)
        return out

    def concat(self, tiles):
        """GxB_Matrix_concat of a flat list of Vectors into this Vector, whose old contents are
        discarded (reference core/ss/vector.py:251-267)."""
        rows, m, n, _ = _concat_tiles(tiles, is_matrix=False)
        _concat_into(self._parent, rows, m, n)

    def build_diag(self, matrix, k=0, **opts):
        """GxB_Vector_diag (reference core/ss/vector.py:147-183): diagonal ``k`` of a Matrix or
        TransposedMatrix into this Vector, whose old contents are discarded.  ``A.T`` is read as
        ``A`` with ``-k``: nothing is transposed."""
        from .matrix import Matrix, TransposedMatrix

        matrix = _expect_type(self._parent, matrix, (Matrix, TransposedMatrix), within="ss.build_diag",
                              argname="matrix")
        k = _diag_k(k)
        desc = descriptor_lookup(**_sort_opts(opts))
        if type(matrix) is TransposedMatrix:
            k = -k
            matrix = matrix._matrix
        call("GxB_Vector_diag", [self._parent, matrix, k, desc])

    def reshape(self, nrows, ncols=None, order="rowwise", *, name=None):
        """The Vector as a Matrix of the given shape (reference core/ss/vector.py:1377-1405):
        GxB_Matrix_reshapeDup of the vector as size x 1, from the bitmap straight to CSR."""
        parent = self._parent
        return _reshape_dup(parent, (parent._size, 1), nrows, ncols, order, name)


class MatrixSS:
    def __init__(self, parent):
        self._parent = parent

    def scan(self, op=None, order="rowwise", *, name=None):
        """GxB_Matrix_scan (reference core/ss/matrix.py:3701-3715): the inclusive prefix scan of
        every row (column, if columnwise) under a monoid (default plus), in the monoid's type."""
        return _scan(self._parent, op, _order(order) == "columnwise", name)

    def sort(self, op=_op.binary.lt, order="rowwise", *, values=True, permutation=True, **opts):
        """GxB_Matrix_sort (reference core/ss/matrix.py:3991-4055): ``(C, P)``, the values of
        every row (column, if columnwise) in the order of ``op`` (ties by ascending index) moved
        to the left (top), and the column (row) indices they came from; both have the parent's
        shape, an output that was not requested is ``None``."""
        from .matrix import Matrix

        columnwise = _order(order) == "columnwise"
        parent = self._parent
        op = _sort_op(parent, op)
        desc = descriptor_lookup(transpose_first=columnwise, **_sort_opts(opts))
        if not values and not permutation:
            return None, None
        C = Matrix(parent.dtype, parent.nrows, parent.ncols, name="Values") if values else None
        P = Matrix(UINT64, parent.nrows, parent.ncols, name="Permutation") if permutation else None
        call("GxB_Matrix_sort", [C, P, op, parent, desc])
        return C, P

    def selectk(self, how, k, order="rowwise", *, seed=None, name=None):
        """GxB_Matrix_selectk (reference core/ss/matrix.py:3815-3875): up to ``k`` entries of every
        row (column, if columnwise), each where it was.  ``how``: "first", "last", "smallest",
        "largest" (ties by position, see include/graphblas_amd.h) or "random" (a uniform k-subset of
        every row; ``seed`` reproduces it)."""
        from .matrix import Matrix

        parent = self._parent
        columnwise = _order(order) == "columnwise"
        how = _how(how, _SELECTK_HOWS)
        k = _count(k)
        C = Matrix(parent.dtype, parent._nrows, parent._ncols, name=name)
        call("GxB_Matrix_selectk", [C, parent, how, k, _seed(seed), descriptor_lookup(transpose_first=columnwise)])
        return C

    def compactify(self, how="first", k=None, order="rowwise", *, reverse=False, asindex=False, seed=None, name=None):
        """GxB_Matrix_compactify (reference core/ss/matrix.py:3877-3989): every row's entries moved
        to columns 0 .. (every column's to rows 0 .., if columnwise) in the order of ``how``
        (reversed if ``reverse``), as values or, with ``asindex``, as the column (row) indices they
        came from (UINT64).  The new Matrix is nrows x k (k x ncols); ``k`` defaults to the longest
        row (column).  "random" emits its choice in ascending position and ignores ``reverse``."""
        from .matrix import Matrix

        parent = self._parent
        columnwise = _order(order) == "columnwise"
        how = _how(how, _COMPACTIFY_HOWS)
        desc = descriptor_lookup(transpose_first=columnwise)
        if k is None:
            width = _IndexOut("&k")
            call("GxB_Matrix_compactify_width", [width, parent, desc])
            k = width.value.value
        k = _count(k)
        dtype = UINT64 if asindex else parent.dtype
        C = Matrix(dtype, k, parent._ncols, name=name) if columnwise else Matrix(dtype, parent._nrows, k, name=name)
        call("GxB_Matrix_compactify", [C, parent, how, k, bool(reverse), bool(asindex), _seed(seed), desc])
        return C

    def split(self, chunks, *, name=None):
        """GxB_Matrix_split (reference core/ss/matrix.py:281-339): a list of lists of Matrix
        tiles named ``f"{name}_{i}x{j}"``.  ``chunks``: see ``normalize_chunks``."""
        from .matrix import Matrix

        parent = self._parent
        tile_nrows, tile_ncols = normalize_chunks(chunks, parent.shape)
        m, n = len(tile_nrows), len(tile_ncols)
        tiles = _HandleArray(m * n, exc_arg=parent)
        call("GxB_Matrix_split", [tiles, m, n, _IndexArray(tile_nrows, "Tile_nrows"),
                                  _IndexArray(tile_ncols, "Tile_ncols"), parent, None])
        name = parent.name if name is None else name
        out = []
        for i, nrows in enumerate(tile_nrows):
            row = []
            for j, ncols in enumerate(tile_ncols):
                T = Matrix.__new__(Matrix)
                T.dtype, T.name, T._nrows, T._ncols = parent.dtype, f"{name}_{i}x{j}", nrows, ncols
                T._h = ctypes.c_void_p(tiles.array[i * n + j])
                row.append(T)
            out.append(row)
        return out

    def concat(self, tiles):
        """GxB_Matrix_concat of a list of lists of tiles into this Matrix, whose old contents are
        discarded; Vectors count as N x 1 (reference core/ss/matrix.py:363-381)."""
        rows, m, n, _ = _concat_tiles(tiles, is_matrix=True)
        _concat_into(self._parent, rows, m, n)

    def build_diag(self, vector, k=0, **opts):
        """GxB_Matrix_diag (reference core/ss/matrix.py:252-279): the diagonal matrix of
        ``vector`` on diagonal ``k`` into this Matrix, whose old contents are discarded."""
        from .vector import Vector

        vector = _expect_type(self._parent, vector, Vector, within="ss.build_diag", argname="vector")
        k = _diag_k(k)
        call("GxB_Matrix_diag", [self._parent, vector, k, descriptor_lookup(**_sort_opts(opts))])

    def reshape(self, nrows, ncols=None, order="rowwise", *, inplace=False, name=None):
        """GxB_Matrix_reshape / GxB_Matrix_reshapeDup (reference core/ss/matrix.py:3742-3815): the
        Matrix with a new shape of as many positions, filled in row-major ("rowwise") or
        column-major order.  One dimension may be ``-1``; ``nrows`` may be the shape tuple.
        ``inplace=True`` reshapes this Matrix (row-major: its values do not move) and returns None."""
        parent = self._parent
        if not inplace:
            return _reshape_dup(parent, parent.shape, nrows, ncols, order, name)
        columnwise = _order(order) == "columnwise"
        nrows, ncols = _reshape_shape(parent.shape, nrows, ncols)
        call("GxB_Matrix_reshape", [parent, columnwise, nrows, ncols, None])
        parent._nrows, parent._ncols = nrows, ncols

    def flatten(self, order="rowwise", *, name=None):
        """The Matrix as a Vector of nrows * ncols positions, row-major or column-major (reference
        core/ss/matrix.py:3717-3740): one call of GxB_Vector_flatten."""
        from .vector import Vector

        parent = self._parent
        columnwise = _order(order) == "columnwise"
        w = Vector(parent.dtype, parent._nrows * parent._ncols, name=name)
        call("GxB_Vector_flatten", [w, parent, columnwise, None])
        return w
