"""A dense numpy model of the general GraphBLAS operations (eWise, apply, reduce,
transpose, build, the output write-back, and the indexing operations extract, assign,
setElement, removeElement and resize), written from the GraphBLAS C API
rules and the SuiteSparse:GraphBLAS 7.4 builtin definitions, not from the
kernels.  A sparse object is a ``(present, values)`` pair of arrays of the
object's shape; dtypes are the GraphBLAS names ("INT8", "FP64", ...).

The tests compare the device results with this model through ``to_coo()``;
``test_dense_model.py`` checks the model itself against hand-worked values.
"""
import math

import numpy as np

NP = {"BOOL": np.bool_, "INT8": np.int8, "UINT8": np.uint8, "INT16": np.int16, "UINT16": np.uint16,
      "INT32": np.int32, "UINT32": np.uint32, "INT64": np.int64, "UINT64": np.uint64,
      "FP32": np.float32, "FP64": np.float64}
NAME = {np.dtype(v): k for k, v in NP.items()}
INTS = ["INT8", "UINT8", "INT16", "UINT16", "INT32", "UINT32", "INT64", "UINT64"]
FLOATS = ["FP32", "FP64"]
ALL = ["BOOL"] + INTS + FLOATS

COMPARE = {"eq", "ne", "gt", "lt", "ge", "le"}
# exp, log, ...: compared in ulps against float64 (see the tolerance table of the GPU tests)
TRANSCENDENTAL = {"exp", "exp2", "log", "log2", "log10", "sin", "cos", "tan", "pow", "atan2", "hypot"}


def name_of(dtype):
    return dtype if isinstance(dtype, str) else NAME[np.dtype(dtype)]


def is_int(dtype):
    return dtype in INTS


def is_float(dtype):
    return dtype in FLOATS


def tmin(dtype):
    return np.iinfo(NP[dtype]).min


def tmax(dtype):
    return np.iinfo(NP[dtype]).max


# ---------------------------------------------------------------------- cast
def cast(values, dtype):
    """SuiteSparse typecasting: anything -> bool is ``!= 0``; float -> integer is NaN -> 0,
    saturating, else truncation; integer -> integer is the value modulo 2^bits."""
    x = np.asarray(values)
    src = name_of(x.dtype)
    if src == dtype:
        return x.copy()
    if dtype == "BOOL":
        return x != 0
    if is_float(src) and is_int(dtype):
        lo, hi = tmin(dtype), tmax(dtype)
        xd = x.astype(np.float64)
        # float(hi) rounds up to 2^63 / 2^64 for the 64-bit types: >= still saturates correctly
        low, high, nan = xd <= float(lo), xd >= float(hi), np.isnan(xd)
        safe = np.where(low | high | nan, 0.0, np.trunc(xd))
        out = safe.astype(NP[dtype])
        out[low] = lo
        out[high] = hi
        out[nan] = 0
        return out
    with np.errstate(over="ignore", invalid="ignore"):
        return x.astype(NP[dtype])  # int -> int wraps (sign-extending); the rest is exact or rounds


# ---------------------------------------------------------------------- operators
def _idiv(x, y, dtype):
    """integer x / y: x/0 is 0, type max or (signed x < 0) type min; x/-1 the wrapped negation;
    otherwise truncation toward zero"""
    t = NP[dtype]
    x, y = np.asarray(x, t), np.asarray(y, t)
    x, y = np.broadcast_arrays(x, y)
    signed = np.issubdtype(t, np.signedinteger)
    zero = y == 0
    special = zero | (y == -1) if signed else zero
    ys = np.where(special, t(1), y)
    q = x // ys  # floor
    if signed:
        q = q + (((x % ys) != 0) & ((x < 0) != (ys < 0))).astype(t)
        q = np.where(y == -1, (-x.astype(np.uint64 if t == np.int64 else np.int64)).astype(t), q)
        byzero = np.where(x == 0, t(0), np.where(x < 0, t(tmin(dtype)), t(tmax(dtype))))
    else:
        byzero = np.where(x == 0, t(0), t(tmax(dtype)))
    return np.where(zero, byzero, q).astype(t)


def _round_half_away(x):
    r = np.trunc(x)
    with np.errstate(invalid="ignore"):
        up = np.abs(x - r) >= 0.5  # x - trunc(x) is exact
    return np.copysign(np.where(up, np.abs(r) + 1, np.abs(r)), x).astype(x.dtype)


def _ieee_remainder(x, y):
    out = np.empty(np.broadcast(x, y).shape, np.float64)
    xb, yb = np.broadcast_arrays(np.asarray(x, np.float64), np.asarray(y, np.float64))
    for k in np.ndindex(out.shape):
        try:
            out[k] = math.remainder(float(xb[k]), float(yb[k]))
        except ValueError:  # x infinite or y zero
            out[k] = math.nan
    return out


def _via64(fn, t, *args):
    """float64 evaluation rounded once to the operand type"""
    with np.errstate(all="ignore"):
        return np.asarray(fn(*[np.asarray(a, np.float64) for a in args])).astype(t)


def binop(name, dtype, x, y):
    """z = name(x, y) with x, y of `dtype`; z is bool for eq..le, else `dtype`"""
    t = NP[dtype]
    x, y = np.broadcast_arrays(np.asarray(x, t), np.asarray(y, t))
    one = np.ones(x.shape, t)
    if dtype == "BOOL":
        name = {"plus": "lor", "max": "lor", "times": "land", "min": "land", "minus": "lxor",
                "rminus": "lxor", "ne": "lxor", "isne": "lxor", "div": "first", "rdiv": "second",
                "eq": "lxnor", "iseq": "lxnor", "isgt": "gt", "islt": "lt", "isge": "ge", "isle": "le",
                "bor": "lor", "band": "land", "bxor": "lxor", "bxnor": "lxnor"}.get(name, name)
        table = {"first": lambda: x, "second": lambda: y, "any": lambda: y, "pair": lambda: one,
                 "lor": lambda: x | y, "land": lambda: x & y, "lxor": lambda: x ^ y, "lxnor": lambda: ~(x ^ y),
                 "gt": lambda: x & ~y, "lt": lambda: ~x & y, "ge": lambda: x | ~y, "le": lambda: ~x | y,
                 "pow": lambda: x | ~y}
        return table[name]().copy()
    xb, yb = x != 0, y != 0
    with np.errstate(all="ignore"):
        if name == "first":
            return x.copy()
        if name in ("second", "any"):  # ANY picks one of its arguments; the library documents the second
            return y.copy()
        if name == "pair":
            return one
        if name in COMPARE or name in ("iseq", "isne", "isgt", "islt", "isge", "isle"):
            fn = {"eq": np.equal, "ne": np.not_equal, "gt": np.greater, "lt": np.less,
                  "ge": np.greater_equal, "le": np.less_equal}[name[-2:]]
            r = fn(x, y)
            return r if name in COMPARE else r.astype(t)
        if name in ("lor", "land", "lxor", "lxnor"):
            r = {"lor": xb | yb, "land": xb & yb, "lxor": xb ^ yb, "lxnor": ~(xb ^ yb)}[name]
            return r.astype(t)
        if name == "min":
            return np.fmin(x, y) if is_float(dtype) else np.minimum(x, y)
        if name == "max":
            return np.fmax(x, y) if is_float(dtype) else np.maximum(x, y)
        if name == "plus":
            return x + y
        if name == "minus":
            return x - y
        if name == "rminus":
            return y - x
        if name == "times":
            return x * y
        if name in ("div", "rdiv"):
            a, b = (x, y) if name == "div" else (y, x)
            return _idiv(a, b, dtype) if is_int(dtype) else a / b
        if name == "pow":
            if is_int(dtype):  # the saturating cast of a float64 pow
                return cast(np.power(x.astype(np.float64), y.astype(np.float64)), dtype)
            return _via64(np.power, t, x, y)
        if is_int(dtype):
            if name == "bor":
                return x | y
            if name == "band":
                return x & y
            if name == "bxor":
                return x ^ y
            if name == "bxnor":
                return ~(x ^ y)
        else:
            if name == "atan2":
                return _via64(np.arctan2, t, x, y)
            if name == "hypot":
                return _via64(np.hypot, t, x, y)
            if name == "fmod":
                return _via64(np.fmod, t, x, y)
            if name == "remainder":
                return _via64(_ieee_remainder, t, x, y)
            if name == "ldexp":
                return np.ldexp(x, np.trunc(y).astype(np.int32)).astype(t)
            if name == "copysign":
                return np.copysign(x, y)
    raise KeyError(f"binary.{name}[{dtype}]")


def binop_return_dtype(name, dtype):
    return "BOOL" if name in COMPARE else dtype


def unop(name, dtype, x):
    t = NP[dtype]
    x = np.asarray(x, t)
    if dtype == "BOOL":
        if name in ("lnot", "bnot"):
            return ~x
        if name in ("one", "minv"):
            return np.ones(x.shape, t)
        return x.copy()  # identity, ainv, abs
    with np.errstate(all="ignore"):
        if name == "identity":
            return x.copy()
        if name == "ainv":
            return np.negative(x)  # wraps on integers; -x (not 0 - x) on floats
        if name == "minv":
            return _idiv(np.ones(x.shape, t), x, dtype) if is_int(dtype) else t(1) / x
        if name == "abs":
            return np.abs(x)  # wraps at the signed minimum
        if name == "lnot":
            return (x == 0).astype(t)
        if name == "one":
            return np.ones(x.shape, t)
        if name == "bnot" and is_int(dtype):
            return ~x
        if is_float(dtype):
            if name == "round":
                return _round_half_away(x)
            fn = {"sqrt": np.sqrt, "log": np.log, "log2": np.log2, "log10": np.log10, "exp": np.exp,
                  "exp2": np.exp2, "floor": np.floor, "ceil": np.ceil, "trunc": np.trunc, "sin": np.sin,
                  "cos": np.cos, "tan": np.tan}.get(name)
            if fn is not None:
                return _via64(fn, t, x)
    raise KeyError(f"unary.{name}[{dtype}]")


# ---------------------------------------------------------------------- monoids
def monoid_identity(name, dtype):
    t = NP[dtype]
    if name in ("plus", "lor", "lxor", "bor", "bxor", "any"):
        return t(0)
    if name in ("times", "land", "lxnor"):
        return t(1)
    if name == "min":
        return t(np.inf) if is_float(dtype) else t(tmax(dtype))
    if name == "max":
        return t(-np.inf) if is_float(dtype) else t(tmin(dtype))
    if name in ("band", "bxnor"):
        return t(tmax(dtype))  # all ones (unsigned types only)
    raise KeyError(name)


def monoid_fold(name, dtype, vals):
    """left-to-right fold of a non-empty 1-d array with the monoid's binary operator
    (exact monoids only: the caller bounds float plus / times separately)"""
    vals = np.asarray(vals, NP[dtype])
    if name == "plus":
        return np.add.reduce(vals, dtype=NP[dtype])
    if name == "times":
        return np.multiply.reduce(vals, dtype=NP[dtype])
    if name == "min":
        return np.fmin.reduce(vals) if is_float(dtype) else vals.min()
    if name == "max":
        return np.fmax.reduce(vals) if is_float(dtype) else vals.max()
    if name == "any":
        return vals[0]  # any one of them: callers check membership, not this value
    if name in ("lor", "land", "lxor", "lxnor"):
        b = vals != 0
        r = {"lor": b.any(), "land": b.all(), "lxor": bool(b.sum() & 1),
             "lxnor": not ((~b).sum() & 1)}[name]  # a chain of == is true iff the falses pair up
        return NP[dtype](r)
    if name in ("bor", "band", "bxor"):
        return {"bor": np.bitwise_or, "band": np.bitwise_and, "bxor": np.bitwise_xor}[name].reduce(vals)
    if name == "bxnor":  # ~(a ^ b) = a ^ b ^ ones: n values carry n - 1 complements
        r = np.bitwise_xor.reduce(vals)
        return r if vals.size & 1 else ~r
    raise KeyError(name)


def monoid_fold_sequential(name, dtype, vals):
    """the same by the definition, one binary operator call per value (checks the closed forms)"""
    vals = np.asarray(vals, NP[dtype])
    acc = vals[:1]
    for k in range(1, vals.size):
        acc = binop(name, dtype, acc, vals[k:k + 1])
    return acc[0]


# ---------------------------------------------------------------------- operations
def ewise(kind, op, dtype, A, B):
    """C = A (+) B (kind "add") or A (*) B ("mult") with the typed operator op[dtype]: both
    operands are cast to `dtype`; an entry present on one side only (add) carries the cast of
    that side's value to the operator's return type"""
    (ap, av), (bp, bv) = A, B
    zt = binop_return_dtype(op, dtype)
    ax, bx = cast(av, dtype), cast(bv, dtype)
    both = ap & bp
    z = cast(binop(op, dtype, ax, bx), zt)
    if kind == "mult":
        return both, np.where(both, z, NP[zt](0))
    out = np.where(both, z, np.where(ap, cast(ax, zt), cast(bx, zt)))
    present = ap | bp
    return present, np.where(present, out, NP[zt](0))


def apply(op, dtype, A, left=None, right=None):
    """unary op[dtype](A), or binary op[dtype](left, A) / op[dtype](A, right) with a bound scalar"""
    p, v = A
    x = cast(v, dtype)
    if left is None and right is None:
        z, zt = unop(op, dtype, x), dtype
    else:
        zt = binop_return_dtype(op, dtype)
        s = cast(np.atleast_1d(np.asarray(left if right is None else right)), dtype)
        z = binop(op, dtype, s, x) if right is None else binop(op, dtype, x, s)
    return p.copy(), np.where(p, z, NP[zt](0))


def reduce_scalar(monoid, dtype, A):
    """None for an empty object, else the fold of its entries (row-major) cast to `dtype`"""
    p, v = A
    vals = cast(v[p], dtype)
    return None if vals.size == 0 else monoid_fold(monoid, dtype, vals)


def reduce_rows(monoid, dtype, A):
    p, v = A
    out = np.zeros(p.shape[0], NP[dtype])
    present = p.any(axis=1)
    for i in np.flatnonzero(present):
        out[i] = monoid_fold(monoid, dtype, cast(v[i][p[i]], dtype))
    return present, out


def reduce_cols(monoid, dtype, A):
    return reduce_rows(monoid, dtype, transpose(A))


def transpose(A):
    p, v = A
    return np.ascontiguousarray(p.T), np.ascontiguousarray(v.T)


def build(shape, indices, values, dup_op, dtype):
    """COO ingest: `indices` is a tuple of index arrays (one per dimension); the values are cast
    to `dtype` first, then duplicates fold in input order, z = dup_op(z, next)"""
    vals = cast(np.asarray(values), dtype)
    present = np.zeros(shape, bool)
    out = np.zeros(shape, NP[dtype])
    flat = np.ravel_multi_index(tuple(np.asarray(i, np.int64) for i in indices), shape)
    order = np.argsort(flat, kind="stable")
    flat, vals = flat[order], vals[order]
    starts = np.flatnonzero(np.r_[True, flat[1:] != flat[:-1]])
    ends = np.r_[starts[1:], flat.size]
    acc = vals[starts].copy()
    # fold the k-th duplicate of every key at once
    k = 1
    live = np.flatnonzero(ends - starts > 1)
    while live.size:
        acc[live] = cast(binop(dup_op, dtype, acc[live], vals[starts[live] + k]), dtype)
        k += 1
        live = live[ends[live] - starts[live] > k]
    present.ravel()[flat[starts]] = True
    out.ravel()[flat[starts]] = acc
    return present, out


def write_back(C, T, mask=None, mask_comp=False, mask_struct=False, replace=False, accum=None,
               accum_dtype=None):
    """C<M, replace> = accum(C, T) (C API 2.0 section 3.5, with SuiteSparse's typing of Z):
    Z has C's type; an entry only in C is taken unchanged, an entry only in T is cast to C's
    type, and where both exist the accumulator runs in its own type on the casts of c and t and
    its result is cast to C's type.  Then C = Z where the mask is true; elsewhere C keeps its
    entry, or loses it under `replace`."""
    (cp, cv), (tp, tv) = C, T
    ct = name_of(cv.dtype)
    t_c = cast(tv, ct)
    if accum is None:
        zp, zv = tp, t_c
    else:
        adt = ct if accum_dtype is None else accum_dtype
        both = cast(binop(accum, adt, cast(cv, adt), cast(tv, adt)), ct)
        zp = cp | tp
        zv = np.where(cp & tp, both, np.where(cp, cv, t_c))
    if mask is None:
        m = np.ones(cp.shape, bool)
    else:
        mp, mv = mask
        m = mp if mask_struct else mp & cast(mv, "BOOL")
    if mask_comp:
        m = ~m
    present = np.where(m, zp, cp & (not replace))
    values = np.where(m, zv, cv)
    return present, np.where(present, values, NP[ct](0))


# ---------------------------------------------------------------------- conversions
def to_dense(shape, indices, values):
    """(present, values) from COO arrays without duplicates"""
    values = np.asarray(values)
    present = np.zeros(shape, bool)
    out = np.zeros(shape, values.dtype)
    idx = tuple(np.asarray(i, np.int64) for i in indices)
    present[idx] = True
    out[idx] = values
    return present, out


def to_coo(A):
    """indices (row-major order, as the library exports them) and values of a model object"""
    p, v = A
    idx = np.nonzero(p)
    return idx + (v[idx],)


def ulp_distance(got, ref):
    """largest distance in units in the last place between two float arrays of one dtype; NaNs
    and infinities must coincide (returns inf where they do not)"""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.dtype == ref.dtype and got.shape == ref.shape
    special = ~np.isfinite(ref)
    same = np.where(np.isnan(ref), np.isnan(got), got == ref)
    if not same[special].all() or not np.isfinite(got[~special]).all():
        return math.inf
    it = np.int32 if got.dtype == np.float32 else np.int64
    lowest = int(np.iinfo(it).min)

    def key(a):  # an integer that grows with the float: adjacent floats differ by one
        b = a.view(it).astype(np.int64)
        return np.where(b < 0, lowest - b, b)

    g, r = key(got[~special]), key(ref[~special])
    return int(np.max(np.abs(g - r))) if g.size else 0


# ---------------------------------------------------------------------- mxm, mxv, vxm
POSITIONAL = {"firsti": ("i", 0), "firsti1": ("i", 1), "firstj": ("k", 0), "firstj1": ("k", 1),
              "secondi": ("k", 0), "secondi1": ("k", 1), "secondj": ("j", 0), "secondj1": ("j", 1)}


class Products:
    """Every product of T = A (+).(x) B, grouped by output entry.  Entry e is T(rows[e], cols[e]);
    its products are z[start[e]:end[e]] with the inner indices k[start[e]:end[e]] ascending."""

    def __init__(self, shape, dtype, rows, cols, start, end, z, k, clash=None):
        self.shape, self.dtype = shape, dtype
        self.rows, self.cols, self.start, self.end, self.z, self.k = rows, cols, start, end, z, k
        # per product: a float min / max multiplier met +0.0 and -0.0, and may return either
        self.clash = np.zeros(z.size, bool) if clash is None else clash

    @property
    def segment(self):
        """the entry number of every product"""
        return np.repeat(np.arange(self.rows.size), self.end - self.start)

    def lists(self):
        """{(i, j): the products of that entry in ascending k}"""
        return {(int(i), int(j)): self.z[s:e] for i, j, s, e in zip(self.rows, self.cols, self.start, self.end)}

    def reordered(self, order):
        """the products with every list reversed ("descending") or shuffled (a numpy Generator)"""
        seg = self.segment
        if isinstance(order, str):
            assert order == "descending"
            key = -np.arange(seg.size)
        else:
            key = order.permutation(seg.size)
        return self.z[np.lexsort((key, seg))]

    def fold(self, monoid, z=None):
        """every list folded left to right, one call of the monoid's binary operator per product
        (monoid_fold_sequential, run on all the lists at once)"""
        z = self.z if z is None else z
        acc = z[self.start].copy()
        live = np.flatnonzero(self.end - self.start > 1)
        t = 1
        while live.size:
            acc[live] = binop(monoid, self.dtype, acc[live], z[self.start[live] + t])
            t += 1
            live = live[self.end[live] - self.start[live] > t]
        return acc

    def dense(self, per_entry, fill=0):
        """a per-entry array scattered to the shape of T"""
        per_entry = np.asarray(per_entry)
        out = np.full(self.shape, fill, per_entry.dtype)
        out[self.rows, self.cols] = per_entry
        return out

    def member(self, rows, cols, values):
        """for each (rows[q], cols[q]), an entry asked about once: is values[q] one of that entry's
        products, compared by bits"""
        lookup = self.dense(np.arange(self.rows.size), -1)
        e = lookup[rows, cols]
        assert (e >= 0).all()
        want = np.full(self.rows.size, 0, self.z.dtype)
        want[e] = values
        u = np.dtype(f"u{self.z.dtype.itemsize}")
        asked = want[self.segment]
        hit = self.z.view(u) == asked.view(u)
        if self.z.dtype.kind == "f":  # any NaN is the NaN; a clash product is a zero of either sign
            hit |= (np.isnan(self.z) & np.isnan(asked)) | (self.clash & (self.z == asked))
        ok = np.logical_or.reduceat(hit, self.start) if hit.size else np.zeros(0, bool)
        return ok[e]


def mxm_products(mul, dtype, A, B, tran0=False, tran1=False):
    """The products of A (x) B.  `dtype` is the multiplier's input type: both operands are cast to
    it first and z has binop_return_dtype(mul, dtype) (BOOL for the comparators).  A positional
    multiplier ignores the values and `dtype` is its result type; the indices are those of the
    operands as multiplied, after any transpose: A(i,k) . B(k,j) gives FIRSTI = i, FIRSTJ =
    SECONDI = k, SECONDJ = j, and the `1` forms one more (the GxB positional operators; the same
    reading as oracle/gb_oracle.c binop())."""
    if tran0:
        A = transpose(A)
    if tran1:
        B = transpose(B)
    (ap, av), (bp, bv) = A, B
    assert ap.shape[1] == bp.shape[0]
    clash = None
    n, m = ap.shape[0], bp.shape[1]
    ai, ak = np.nonzero(ap)  # row-major: ascending k within a row
    brow = bp.sum(axis=1)
    bptr = np.r_[0, np.cumsum(brow)]
    bj = np.nonzero(bp)[1]
    cnt = brow[ak]
    total = int(cnt.sum())
    src = np.repeat(np.arange(ai.size), cnt)
    within = np.arange(total) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    I, K = ai[src], ak[src]
    J = bj[bptr[K] + within] if total else np.zeros(0, np.int64)
    if mul in POSITIONAL:
        which, plus = POSITIONAL[mul]
        with np.errstate(over="ignore"):
            z = ({"i": I, "k": K, "j": J}[which] + plus).astype(NP[dtype])
        zt = dtype
    else:
        zt = binop_return_dtype(mul, dtype)
        ax, bx = cast(av, dtype), cast(bv, dtype)
        x, y = ax[I, K], bx[K, J]
        z = cast(binop(mul, dtype, x, y), zt)
        if mul in ("min", "max") and is_float(dtype):
            clash = (x == 0) & (y == 0) & (np.signbit(x) != np.signbit(y))
    order = np.argsort(I * m + J, kind="stable")  # keeps k ascending inside an entry
    I, J, K, z = I[order], J[order], K[order], z[order]
    clash = None if clash is None else clash[order]
    key = I * m + J
    start = np.flatnonzero(np.r_[True, key[1:] != key[:-1]]) if total else np.zeros(0, np.int64)
    end = np.r_[start[1:], total] if total else np.zeros(0, np.int64)
    return Products((n, m), zt, I[start], J[start], start, end, z, K, clash)


def mxm(monoid, mul, dtype, A, B, tran0=False, tran1=False, products=False):
    """T = A (+).(x) B as (present, values) in the monoid's type, every entry folded in ascending
    k; with products=True also the Products the fold ran on.  Masks, accumulators and replace
    are write_back's business."""
    P = mxm_products(mul, dtype, A, B, tran0, tran1)
    monoid = {"eq": "lxnor"}.get(monoid, monoid)
    vals = P.fold(monoid) if P.rows.size else np.zeros(0, NP[P.dtype])
    T = P.dense(np.ones(P.rows.size, bool), False), P.dense(vals)
    return (T, P) if products else T


def _column(u):
    return u[0][:, None], u[1][:, None]


def _row(u):
    return u[0][None, :], u[1][None, :]


def mxv(monoid, mul, dtype, A, u, tran0=False, products=False):
    """w = A (+).(x) u with u an n x 1 matrix (SECONDJ = 0): the C API's definition of GrB_mxv,
    reference docs/user_guide/operations.rst:17-22"""
    T, P = mxm(monoid, mul, dtype, A, _column(u), tran0=tran0, products=True)
    w = T[0][:, 0], T[1][:, 0]
    return (w, P) if products else w


def vxm(monoid, mul, dtype, u, A, tran1=False, products=False):
    """w = u (+).(x) A with u a 1 x n matrix (FIRSTI = 0)"""
    T, P = mxm(monoid, mul, dtype, _row(u), A, tran1=tran1, products=True)
    w = T[0][0, :], T[1][0, :]
    return (w, P) if products else w


def order_dependent(monoid, P, seed=0):
    """Per entry: does the fold of its products depend on their order?  Folds ascending k,
    descending k and one seeded shuffle and compares the bits (NaNs count as equal).  Float
    min / max return either zero when a list holds both: those entries are compared with ==."""
    monoid = {"eq": "lxnor"}.get(monoid, monoid)
    if P.rows.size == 0:
        return np.zeros(0, bool)
    a = P.fold(monoid)
    bad = np.zeros(P.rows.size, bool)
    loose = both_zeros(P) if monoid in ("min", "max") else bad
    for order in ("descending", np.random.default_rng(seed)):
        b = P.fold(monoid, P.reordered(order))
        u = np.dtype(f"u{a.dtype.itemsize}")
        same = a.view(u) == b.view(u)
        if a.dtype.kind == "f":
            same |= np.isnan(a) & np.isnan(b)
            same |= loose & (a == b)
        bad |= ~same
    return bad


def both_zeros(P):
    """per entry of a float product: does its list hold +0.0 and -0.0?"""
    if P.z.dtype.kind != "f" or P.rows.size == 0:
        return np.zeros(P.rows.size, bool)
    zero, neg = P.z == 0, np.signbit(P.z)
    return np.logical_or.reduceat(zero & neg, P.start) & np.logical_or.reduceat(zero & ~neg, P.start)


def zero_sign_free(monoid, P):
    """Per entry of a float product: may a zero result carry either sign?  True where a min / max
    monoid folds a list that holds both zeros, and where the list holds a product of a min / max
    multiplier on +0.0 and -0.0 (C's fmin / fmax may return either; such a term can only change
    the sign of a zero sum, product, minimum or maximum).  These entries are compared with ==."""
    if P.z.dtype.kind != "f" or P.rows.size == 0:
        return np.zeros(P.rows.size, bool)
    free = np.logical_or.reduceat(P.clash, P.start)
    return free | both_zeros(P) if monoid in ("min", "max") else free


# ---------------------------------------------------------------------- indexing operations
# Written from the GraphBLAS C API 2.0 text: GrB_extract (section 4.3.6), GrB_assign (4.3.7),
# setElement / removeElement (4.2.x) and resize.  Index lists are int arrays; None is GrB_ALL.
def _index(I, n):
    return np.arange(n, dtype=np.int64) if I is None else np.asarray(I, np.int64).reshape(-1)


def extract(A, I=None, J=None):
    """T(r, c) = A(I[r], J[c]); the lists may repeat and come in any order"""
    p, v = A
    sel = np.ix_(_index(I, p.shape[0]), _index(J, p.shape[1]))
    return p[sel].copy(), v[sel].copy()


def extract_vec(u, I=None):
    """t(k) = u(I[k])"""
    p, v = u
    I = _index(I, p.shape[0])
    return p[I].copy(), v[I].copy()


def is_scalar(A):
    return not isinstance(A, tuple)


def assign(C, A, I=None, J=None, mask=None, mask_comp=False, mask_struct=False, replace=False, accum=None,
           accum_dtype=None):
    """GrB_assign (not subassign) C<M, replace>(I, J) = accum(C(I, J), A) for a matrix or, with
    J None, a vector.  A is a model object of the region's shape (duplicate-free lists), a numpy
    scalar assigned to every position of the region (lists may repeat), or None: the empty scalar.
    Z = C; inside the region Z = accum(C, A) on the union, or without accum Z = A there (entries
    of C that A lacks are deleted).  Then C<M, replace> = Z over the whole of C: the mask has C's
    shape and `replace` deletes outside the region too."""
    cp, cv = C
    ct = name_of(cv.dtype)
    lists = [_index(I, cp.shape[0])] + ([_index(J, cp.shape[1])] if cp.ndim == 2 else [])
    sel = np.ix_(*lists)
    region = np.zeros(cp.shape, bool)
    region[sel] = True
    if A is None:
        tp, tv = np.zeros(cp.shape, bool), np.zeros(cp.shape, NP[ct])
    elif is_scalar(A):
        x = np.asarray(A)
        tp, tv = region, np.where(region, x, x.dtype.type(0))
    else:
        ap, av = A
        assert ap.shape == tuple(l.size for l in lists), "A must have the shape of the region"
        assert all(np.unique(l).size == l.size for l in lists), "duplicates are undefined for object assign"
        tp, tv = np.zeros(cp.shape, bool), np.zeros(cp.shape, av.dtype)
        tp[sel], tv[sel] = ap, av
    if accum is None:
        zp, zv = np.where(region, tp, cp), np.where(region, cast(tv, ct), cv)
    else:  # outside the region T is empty and C is kept
        zp, zv = write_back(C, (tp, tv), accum=accum, accum_dtype=accum_dtype)
    zv = np.where(zp, zv, NP[ct](0))
    return write_back(C, (zp, zv), mask=mask, mask_comp=mask_comp, mask_struct=mask_struct, replace=replace)


def assign_vec(w, u, I=None, **kw):
    assert w[0].ndim == 1
    return assign(w, u, I, None, **kw)


def set_element(A, index, x):
    """A(index) = x cast to A's type; index is an int (vector) or an (i, j) pair"""
    p, v = A[0].copy(), A[1].copy()
    p[index] = True
    v[index] = cast(np.asarray(x).reshape(1), name_of(v.dtype))[0]
    return p, v


def remove_element(A, index):
    p, v = A[0].copy(), A[1].copy()
    p[index] = False
    v[index] = 0
    return p, v


def resize(A, shape):
    """shrinking drops the entries outside the new shape; growing adds none"""
    p, v = A
    shape = (shape,) if np.ndim(shape) == 0 else tuple(shape)
    np_, nv = np.zeros(shape, bool), np.zeros(shape, v.dtype)
    keep = tuple(slice(0, min(a, b)) for a, b in zip(shape, p.shape))
    np_[keep], nv[keep] = p[keep], v[keep]
    return np_, nv
