"""The tables of test_representation_gpu.py (no GPU needed to import).

A consumer's result is a function of (shape, type, pattern, values at the pattern) of its operands
and of nothing else.  Two tables test that:

CONSUMERS (part A): every operation that takes a vector, run on a vector whose don't-care slots --
the elements of its value array under a clear bit, which no producer writes (gb_new_vec_result
does not clear them) -- were overwritten with a byte pattern through GxB_Vector_device_view.  A
consumer is `fn(c) -> (got, expected)`; `c` (a Case) hands out freshly poisoned copies of the
vector (`c.vec()`), its model (`c.m`) and clean operands; the expectation is the dense model's
(dense_model.py and its companions), computed from the unpoisoned content.

PRODUCERS (part B): every operation that writes a matrix or a vector, as `fn(gb, dt) -> (P,
model)`.  P goes as it was left -- iso, in column words, with a count the host has not read, a
hint, a pooled bitmap, a pending deferred assign -- through MATRIX_BATTERY / VECTOR_BATTERY, next
to R = from_coo(*P.to_coo()); the two results must be equal bit for bit.

Every value is a small integer, so every expectation is exact.  test_representation_cases.py
checks both tables against include/graphblas_amd.h: an entry point that takes a vector, or writes
a matrix or vector, has a row or a one-line exclusion."""
import ctypes
import re

import numpy as np

import dense_model as dm
import derived_state_cases as dc

knobs = dc.knobs
SIZES = (65, 700)            # two words with a one-bit tail; eleven words with a 60-bit tail (dc.N)
TYPES = ("FP64", "FP32", "INT32", "UINT8", "BOOL")
PATTERNS = (0x5A, 0xFF)      # a large finite number (BOOL: neither 0 nor 1); NaN / -1 / the maximum
CLEAR_WORD = 5               # n = 700: bits 320..383 are all clear
MASK_KINDS = ("V", "S", "~V", "~S")


# ---------------------------------------------------------------------- comparison
def _leaf(x):
    a = np.ascontiguousarray(np.asarray(x))
    if a.dtype.kind in "fb":  # bits, not values: NaNs equal, -0.0 != 0.0, a bool byte of 0x5a != 1
        a = a.reshape(-1).view(f"u{a.dtype.itemsize}")
    return a


def same(got, exp):
    """bit-exact comparison of two (nested) tuples of arrays, numbers or None: None, or what differs"""
    if isinstance(exp, (tuple, list)):
        if not isinstance(got, (tuple, list)) or len(got) != len(exp):
            return f"length {len(got) if isinstance(got, (tuple, list)) else got!r} != {len(exp)}"
        for k, (g, e) in enumerate(zip(got, exp)):
            d = same(g, e)
            if d:
                return f"[{k}] {d}"
        return None
    if exp is None or got is None:
        return None if exp is None and got is None else f"{got!r} != {exp!r}"
    g, e = np.asarray(got), np.asarray(exp)
    if g.shape != e.shape:
        return f"shape {g.shape} != {e.shape}"
    if g.dtype != e.dtype:
        return f"dtype {g.dtype} != {e.dtype}"
    gb_, eb = _leaf(g), _leaf(e)
    if not np.array_equal(gb_, eb):
        bad = np.flatnonzero(gb_.ravel() != eb.ravel())
        return f"{bad.size} of {g.size} differ, first at {bad[0]}: {g.ravel()[bad[0]]!r} != {e.ravel()[bad[0]]!r}"
    return None


# ---------------------------------------------------------------------- the poison (CPU side)
def words_of(p):
    """the bitmap words of a presence array, as uint64"""
    return dc._words(np.asarray(p, bool)).astype(np.int64).view(np.uint64)


def clear_slots(words, n):
    """per element of an n-vector: is its bit clear in the bitmap words"""
    w = np.ascontiguousarray(np.asarray(words)).view(np.uint64)
    assert w.size == (n + 63) // 64
    bits = np.unpackbits(w.view(np.uint8), bitorder="little")[:n]
    return bits == 0


def byte_mask(words, n, itemsize):
    """per byte of the value array of an n-vector: does it belong to a don't-care slot"""
    return np.repeat(clear_slots(words, n), itemsize)


def poison(v, pattern):
    """overwrite every byte of every element of v's value array whose bit is clear; returns the
    number of slots written (never 0: the caller has no case without one)"""
    import torch
    from graphblas_amd import device as gdev

    torch.cuda.synchronize()
    before = dc.vec_coo(v)
    view = gdev.vector_view(v._h)
    assert not view.iso and view.values and view.bitmap, "an iso vector has no don't-care slots: not a case"
    n, size = int(view.nrows), dm.NP[v.dtype.name]().itemsize
    bits = gdev.device_tensor(torch, view.bitmap, (n + 63) // 64).cpu().numpy()
    vals = gdev.device_tensor(torch, view.values, n * size, "|u1")
    clear = clear_slots(bits, n)
    stored = vals.cpu().numpy().reshape(n, size).copy()
    vals[torch.from_numpy(byte_mask(bits, n, size)).cuda()] = pattern
    torch.cuda.synchronize()
    now = vals.cpu().numpy().reshape(n, size)
    held = (now == pattern).all(axis=1)
    assert int(clear.sum()) == n - before[0].size, "the bitmap and the count disagree"
    # exactly the n - nvals don't-care slots hold the pattern, next to the entries whose own value is
    # the pattern's (-1 under 0xff), and no stored value changed
    own = ~clear & (stored == pattern).all(axis=1)
    assert np.array_equal(held, clear | own) and int(held.sum()) == n - before[0].size + int(own.sum()), \
        f"{int(held.sum())} elements hold the pattern, {int(clear.sum())} bits are clear"
    assert np.array_equal(now[~clear], stored[~clear]), "a stored value changed"
    assert clear.any(), "no don't-care slot was written"
    diff = same(dc.vec_coo(v), before)
    assert diff is None, f"to_coo changed under the poison: {diff}"
    return int(clear.sum())


# ---------------------------------------------------------------------- models of the operands
def val(dt, x):
    return dm.NP[dt](x)


def item(dt, x):
    return dm.NP[dt](x).item()


def _vals(dt, k, mod):
    """0 .. mod-1 by position (BOOL: false at every third)"""
    return (k % 3 != 0) if dt == "BOOL" else (k % mod).astype(dm.NP[dt])


def pv_of(p, v, dt):
    p = np.asarray(p, bool)
    return p, np.where(p, v, dm.NP[dt](0)).astype(dm.NP[dt])


def vec_model(n, dt):
    """about half the bits set; word 0 full, bit n - 1 clear, and for n = 700 one whole word clear;
    values 0..3 (a value mask differs from a structural one)"""
    rng = np.random.default_rng(100 + n)
    p = rng.random(n) < 0.5
    p[:min(n, 64)] = True
    if n > 64 * (CLEAR_WORD + 1):
        p[64 * CLEAR_WORD:64 * (CLEAR_WORD + 1)] = False
    p[n - 1] = False
    return pv_of(p, _vals(dt, np.arange(n), 4), dt)


def other_model(n, dt, seed=7):
    """a clean second operand: another half of the bits (both, either and neither occur), values 0..4"""
    rng = np.random.default_rng(seed * 1000 + n)
    p = rng.random(n) < 0.5
    p[[1, n - 1]] = True
    p[0] = False
    return pv_of(p, _vals(dt, np.arange(n) * 7 + 1, 5), dt)


LONG_ROW = 300  # entries of row 0 of the product matrix over 700 columns: past SPMV_LONG (128)


def mat_model(nr, nc, dt, seed=3, density=0.15):
    """row 1 and column 2 empty, column 3 full, row 0 long where the width allows; values 1..3
    (BOOL: false at every third)"""
    rng = np.random.default_rng(seed * 100003 + nr * 1009 + nc)
    p = rng.random((nr, nc)) < density
    if nc > LONG_ROW:
        p[0, :LONG_ROW] = True
    if nr > 1:
        p[1, :] = False
    if nc > 3:
        p[:, 2] = False
        p[:, 3] = True
        if nr > 1:
            p[1, 3] = False
    k = np.add.outer(np.arange(nr), np.arange(nc))
    return pv_of(p, (k % 3 != 0) if dt == "BOOL" else (k % 3 + 1), dt)


def gvec(gb, pv, dt):
    i, v = dc.model_vec_coo(pv)
    return gb.Vector.from_coo(i, v, dtype=dt, size=len(pv[0]))


def gmat(gb, pv, dt):
    r, c, v = dm.to_coo(pv)
    return gb.Matrix.from_coo(r, c, v, dtype=dt, nrows=pv[0].shape[0], ncols=pv[0].shape[1])


def vc(w):
    return dc.vec_coo(w)


def mvc(pv):
    return dc.model_vec_coo(pv)


def mc(A):
    return dc.coo(A)


def mmc(pv):
    r, c, v = dm.to_coo(pv)
    return r.astype(np.int64), c.astype(np.int64), v


def zero_of(shape, dt):
    return np.zeros(shape, bool), np.zeros(shape, dm.NP[dt])


def mask_kw(kind):
    return dict(mask_struct="S" in kind, mask_comp=kind.startswith("~"))


def mask_of(k, kind):
    m = k.S if "S" in kind else k.V
    return ~m if kind.startswith("~") else m


def bool_names(dt):
    """(plus, times, min) of the type: BOOL has no plus / times / min monoid of its own"""
    return ("lor", "land", "land") if dt == "BOOL" else ("plus", "times", "min")


def semirings(dt):
    """(monoid, multiplier, the model's type) of the products a vector of this type enters"""
    if dt == "BOOL":
        return [("any", "pair", "BOOL"), ("lor", "land", "BOOL")]
    return [("plus", "times", dt), ("min", "plus", dt), ("any", "pair", dt), ("lor", "land", "BOOL")]


def sr_of(gb, mon, mul, dt):
    return getattr(gb.semiring, f"{mon}_{mul}")[dt]


class OutPtr:
    """a typed `ctype *` result of a direct C call"""

    def __init__(self, dt, name="&x"):
        self.array = np.zeros(1, dm.NP[dt])
        self.name = name

    @property
    def _carg(self):
        return ctypes.c_void_p(self.array.ctypes.data)


class Case:
    """one (size, type, pattern) of part A; pattern None: nothing is poisoned (the same consumers
    on clean storage, to tell a wrong expectation from a dependence on the slots)"""

    def __init__(self, gb, n, dt, pattern):
        self.gb, self.n, self.dt, self.pattern = gb, n, dt, pattern
        self.m = vec_model(n, dt)
        self.o = other_model(n, dt)
        self.written = []

    def poison(self, v):
        if self.pattern is not None:
            self.written.append(poison(v, self.pattern))
        return v

    def vec(self):
        return self.poison(gvec(self.gb, self.m, self.dt))

    def other(self, dt=None):
        dt = dt or self.dt
        o = other_model(self.n, dt)
        return gvec(self.gb, o, dt), o

    def rows(self):
        return 40 if self.n < 128 else 90


# ====================================================================== part A: the consumers
class Consumer:
    """device: the row's function needs device memory of its own (it cannot run against a stand-in)"""

    def __init__(self, name, entries, fn, types=TYPES, device=False):
        self.name, self.entries, self.fn, self.types, self.device = name, tuple(entries), fn, tuple(types), device


CONSUMERS = {}


def consumer(*entries, types=TYPES, name=None, device=False):
    def wrap(fn):
        k = name or fn.__name__[2:]
        assert k not in CONSUMERS, k
        CONSUMERS[k] = Consumer(k, entries, fn, types, device)
        return fn
    return wrap


# ---------------------------------------------------------------------- products
def _mxv_all(c, **kw):
    gb, dt = c.gb, c.dt
    A = mat_model(c.rows(), c.n, dt)
    got, exp = [], []
    for mon, mul, mt in semirings(dt):
        with knobs(gb, **kw):
            w = gmat(gb, A, dt).mxv(c.vec(), sr_of(gb, mon, mul, dt)).new()
        got.append(vc(w))
        exp.append(mvc(dm.mxv(mon, mul, mt, A, c.m)))
    return tuple(got), tuple(exp)


def _vxm_all(c, **kw):
    gb, dt = c.gb, c.dt
    B = dm.transpose(mat_model(c.rows(), c.n, dt))
    got, exp = [], []
    for mon, mul, mt in semirings(dt):
        with knobs(gb, **kw):
            w = c.vec().vxm(gmat(gb, B, dt), sr_of(gb, mon, mul, dt)).new()
        got.append(vc(w))
        exp.append(mvc(dm.vxm(mon, mul, mt, c.m, B)))
    return tuple(got), tuple(exp)


@consumer("GrB_mxv")
def c_mxv_u(c):
    """u of w = A u under plus_times, min_plus, any_pair and lor_land"""
    return _mxv_all(c)


@consumer("GrB_vxm")
def c_vxm_u(c):
    return _vxm_all(c)


@consumer("GrB_mxv")
def c_mxv_u_merge_path(c):
    """the general SpMV's merge-path mode"""
    return _mxv_all(c, spmv_words=2)


@consumer("GrB_mxv")
def c_mxv_u_rows(c):
    """the general SpMV without the long-row table: lanes per row"""
    return _mxv_all(c, spmv_general=1)


@consumer("GrB_mxv")
def c_mxv_u_hot(c):
    """the hot-column relabel forced: a sparse u must not take it"""
    return _mxv_all(c, xhot=2, xhot_cols=16)


@consumer("GrB_vxm")
def c_vxm_u_pull(c):
    """the iso-result SpMV (any_pair) pulling, and the rest on its way"""
    return _vxm_all(c, spmv_direction=1)


@consumer("GrB_vxm")
def c_vxm_u_push(c):
    return _vxm_all(c, spmv_direction=2)


@consumer("GrB_mxv", "GrB_Vector_removeElement")
def c_mxv_u_full_minus_one(c):
    """a full u consumed through the hot-column relabel (the host now believes it full), one entry
    removed, that slot and no other poisoned, consumed again"""
    gb, dt = c.gb, c.dt
    mon, mul, mt = semirings(dt)[0] if dt != "BOOL" else semirings(dt)[1]
    A = mat_model(c.rows(), c.n, dt)
    u = np.ones(c.n, bool), (_vals(dt, np.arange(c.n), 4) if dt == "BOOL" else _vals(dt, np.arange(c.n), 4) + val(dt, 1))
    u = pv_of(*u, dt)
    x, a = gvec(gb, u, dt), gmat(gb, A, dt)
    sr = sr_of(gb, mon, mul, dt)
    with knobs(gb, xhot=2, xhot_cols=16):
        w0 = a.mxv(x, sr).new()
        del x[3]  # column 3 is full: a hot column
        u1 = dm.remove_element(u, 3)
        c.poison(x)
        w1 = a.mxv(x, sr).new()
    return (vc(w0), vc(w1)), (mvc(dm.mxv(mon, mul, mt, A, u)), mvc(dm.mxv(mon, mul, mt, A, u1)))


def _mask_product(c):
    """T = A2 u2 (INT32 plus_times) of size n, and the output's old content"""
    A2 = mat_model(c.n, 50, "INT32", seed=5, density=0.1)
    u2 = other_model(50, "INT32", seed=8)
    w0 = other_model(c.n, "INT32", seed=9)
    return A2, u2, w0, dm.mxv("plus", "times", "INT32", A2, u2)


def _c_mxv_mask(kind, replace):
    def fn(c):
        gb = c.gb
        A2, u2, w0, T = _mask_product(c)
        w = gvec(gb, w0, "INT32")
        w(mask_of(c.vec(), kind), replace=replace) << gmat(gb, A2, "INT32").mxv(gvec(gb, u2, "INT32"),
                                                                               gb.semiring.plus_times["INT32"])
        return vc(w), mvc(dm.write_back(w0, T, mask=c.m, replace=replace, **mask_kw(kind)))
    fn.__doc__ = f"the mask {kind} of an mxv, replace={replace}"
    return fn


for _k in MASK_KINDS:
    for _r in (False, True):
        consumer("GrB_mxv", name=f"mxv_mask_{_k}{'_replace' if _r else ''}")(_c_mxv_mask(_k, _r))


@consumer("GrB_vxm")
def c_vxm_mask(c):
    """the mask of a vxm, every kind, with replace"""
    gb = c.gb
    A2, u2, w0, T = _mask_product(c)
    got, exp = [], []
    for kind in MASK_KINDS:
        w = gvec(gb, w0, "INT32")
        w(mask_of(c.vec(), kind), replace=True) << gvec(gb, u2, "INT32").vxm(gmat(gb, dm.transpose(A2), "INT32"),
                                                                             gb.semiring.plus_times["INT32"])
        got.append(vc(w))
        exp.append(mvc(dm.write_back(w0, T, mask=c.m, replace=True, **mask_kw(kind))))
    return tuple(got), tuple(exp)


@consumer("GrB_mxv", "GrB_vxm")
def c_mxv_w_accum(c):
    """the output w of w += A u and w += u A, no mask, no replace: w's old values are read only
    where w has them, and positions neither w nor T holds stay absent"""
    gb, dt = c.gb, c.dt
    plus, times, _ = bool_names(dt)
    u2 = other_model(50, dt, seed=8)
    sr, acc = sr_of(gb, plus, times, dt), getattr(gb.binary, plus)[dt]
    got, exp = [], []
    for last in (False, True):  # the last position, clear in w: T holds it, or nobody does
        A2 = mat_model(c.n, 50, dt, seed=5, density=0.05)
        A2[0][:, 3] = False
        A2[0][c.n - 1, :] = False
        A2[0][c.n - 1, np.flatnonzero(u2[0])[:2]] = last
        A2 = pv_of(A2[0], A2[1], dt)
        T = dm.mxv(plus, times, dt, A2, u2)
        assert T[0][c.n - 1] == last and not c.m[0][c.n - 1] and (T[0] & c.m[0]).any() and (~T[0] & c.m[0]).any()
        w = c.vec()
        w(acc) << gmat(gb, A2, dt).mxv(gvec(gb, u2, dt), sr)
        w2 = c.vec()
        w2(acc) << gvec(gb, u2, dt).vxm(gmat(gb, dm.transpose(A2), dt), sr)
        got += [vc(w), vc(w2)]
        exp += [mvc(dm.write_back(c.m, T, accum=plus))] * 2
    return tuple(got), tuple(exp)


@consumer("GrB_vxm", "GrB_mxm")
def c_inner_outer(c):
    """u' v and u v' through vxm / mxm, the poisoned vector on either side"""
    gb, dt = c.gb, c.dt
    plus, times, _ = bool_names(dt)
    o, om = c.other()
    sr = sr_of(gb, plus, times, dt)
    mul = getattr(gb.binary, times)[dt]
    got = [c.vec().inner(o, sr).new().value, o.inner(c.vec(), sr).new().value,
           mc(c.vec().outer(o, mul).new()), mc(o.outer(c.vec(), mul).new())]
    s = dm.vxm(plus, times, dt, c.m, dm._column(om))
    s2 = dm.vxm(plus, times, dt, om, dm._column(c.m))
    exp = [s[1][0].item() if s[0][0] else None, s2[1][0].item() if s2[0][0] else None,
           mmc(dm.mxm("any", times, dt, dm._column(c.m), dm._row(om))),
           mmc(dm.mxm("any", times, dt, dm._column(om), dm._row(c.m)))]
    return tuple(got), tuple(exp)


# ---------------------------------------------------------------------- element-wise and unary
EWISE_OPS = ("plus", "min", "first", "second", "lor")


def _c_ewise(kind, side):
    def fn(c):
        import union_model as um

        gb, dt = c.gb, c.dt
        got, exp = [], []
        for op in EWISE_OPS:
            o, om = c.other()
            x = c.vec()
            a, b = (x, o) if side == "left" else (o, x)
            am, bm = (c.m, om) if side == "left" else (om, c.m)
            bop = getattr(gb.binary, op)[dt]
            if kind == "union":
                w = a.ewise_union(b, bop, item(dt, 2), item(dt, 3)).new()
                e = um.ewise_union(op, dt, am, val(dt, 2), bm, val(dt, 3))
            else:
                w = getattr(a, f"ewise_{kind}")(b, bop).new()
                e = dm.ewise(kind, op, dt, am, bm)
            got.append(vc(w))
            exp.append(mvc(e))
        return tuple(got), tuple(exp)
    fn.__doc__ = f"ewise_{kind}, the poisoned vector on the {side}, with plus, min, first, second and lor"
    return fn


for _kind, _entry in (("add", "GrB_Vector_eWiseAdd_BinaryOp"), ("mult", "GrB_Vector_eWiseMult_BinaryOp"),
                      ("union", "GxB_Vector_eWiseUnion")):
    for _side in ("left", "right"):
        consumer(_entry, name=f"ewise_{_kind}_{_side}")(_c_ewise(_kind, _side))


@consumer("GrB_Vector_apply")
def c_apply_unary(c):
    gb, dt = c.gb, c.dt
    op = "lnot" if dt == "BOOL" else "ainv"
    return vc(c.vec().apply(getattr(gb.unary, op)[dt]).new()), mvc(dm.apply(op, dt, c.m))


@consumer("GrB_Vector_apply_BinaryOp1st_T", "GrB_Vector_apply_BinaryOp2nd_T")
def c_apply_bound(c):
    gb, dt = c.gb, c.dt
    op = "lxor" if dt == "BOOL" else "minus"
    bop = getattr(gb.binary, op)[dt]
    s = gb.Scalar.from_value(item(dt, 3 if dt != "BOOL" else 1), dt)
    got = vc(c.vec().apply(bop, left=s).new()), vc(c.vec().apply(bop, right=s).new())
    sv = val(dt, 3 if dt != "BOOL" else 1)
    return got, (mvc(dm.apply(op, dt, c.m, left=sv)), mvc(dm.apply(op, dt, c.m, right=sv)))


def _index_type(dt):
    return "INT32" if dt == "INT32" else "INT64"


@consumer("GrB_Vector_apply_IndexOp_T", "GrB_Vector_apply_IndexOp_Scalar")
def c_apply_rowindex(c):
    import index_apply_model as im

    gb, dt = c.gb, c.dt
    it = _index_type(dt)
    got = (vc(c.vec().apply("rowindex", 1).new()),
           vc(c.vec().apply("rowindex", gb.Scalar.from_value(1, "INT64")).new()))
    e = mvc(im.index_apply(c.m, "rowindex", it, 1))
    assert e[1].dtype == dm.NP[it]
    return got, (e, e)


@consumer("GrB_Vector_select_T", "GrB_Vector_select_Scalar")
def c_select(c):
    """value>, value== and row<=: the kept entries carry the vector's own values"""
    import index_apply_model as im

    gb, dt = c.gb, c.dt
    got, exp = [], []
    cases = [("valuegt", val(dt, 0 if dt == "BOOL" else 1), dt), ("valueeq", val(dt, 1 if dt == "BOOL" else 2), dt),
             ("rowle", np.int64(c.n // 2), None)]
    for op, y, ot in cases:
        keep = im.index_apply(c.m, op, ot, y)
        e = mvc(pv_of(keep[0] & keep[1], c.m[1], dt))
        got.append(vc(c.vec().select(getattr(gb.select, op), y).new()))
        exp.append(e)
        got.append(vc(c.vec().select(getattr(gb.select, op), gb.Scalar.from_value(y.item(), ot or "INT64")).new()))
        exp.append(e)
    return tuple(got), tuple(exp)


def _reduce_cases(dt):
    return [(m, mt) for m, mt in (("plus", dt), ("min", dt), ("lor", "BOOL"), ("any", dt))
            if not (dt == "BOOL" and m == "plus")]


@consumer("GrB_Vector_reduce_Monoid_Scalar", "GrB_Vector_reduce_T")
def c_reduce(c):
    """plus, min, lor and any to a GrB_Scalar and to a C scalar (any: one of the stored values)"""
    gb, dt = c.gb, c.dt
    got, exp = [], []
    stored = c.m[1][c.m[0]]
    for mon, mt in _reduce_cases(dt):
        op = getattr(gb.monoid, mon)[dt]
        s = c.vec().reduce(op).new()
        out = OutPtr(mt)
        gb.base.call(f"GrB_Vector_reduce_{mt}", [out, None, op, c.vec(), None])
        for g in (np.asarray(s.value, dm.NP[mt]), out.array[0]):
            if mon == "any":
                got.append(bool((_leaf(stored) == _leaf(g)).any()))
                exp.append(True)
            else:
                got.append(np.asarray(g))
                exp.append(np.asarray(dm.reduce_scalar(mon, mt, c.m)))
    return tuple(got), tuple(exp)


@consumer("GrB_Vector_eWiseMult_BinaryOp", "GrB_Vector_nvals")
def c_isequal(c):
    """against a clean copy, either way round, and against one that differs in one value"""
    gb, dt = c.gb, c.dt
    clean = gvec(gb, c.m, dt)
    k = int(np.flatnonzero(c.m[0])[-1])
    other = dm.set_element(c.m, k, val(dt, 1) if c.m[1][k] != 1 else val(dt, 0))
    got = (c.vec().isequal(clean), clean.isequal(c.vec()), c.vec().isequal(c.vec()), c.vec().isequal(gvec(gb, other, dt)),
           int(c.vec().nvals))
    return got, (True, True, True, False, int(c.m[0].sum()))


# ---------------------------------------------------------------------- indexing
def _perm(n, seed=1):
    return np.random.default_rng(seed).permutation(n)


def _sub(n):
    """a duplicate-free list that reaches the first, the last and a word boundary"""
    return np.unique(np.r_[0, 63, 64, n - 1, _perm(n, 2)[:n // 3]])[::-1].copy()


@consumer("GrB_Vector_assign")
def c_assign_u(c):
    """u of w[I] << u (I a permutation) and of w << u"""
    gb, dt = c.gb, c.dt
    I = _perm(c.n)
    w0 = other_model(c.n, dt, seed=9)
    w = gvec(gb, w0, dt)
    w[I] << c.vec()
    w2 = gvec(gb, w0, dt)
    w2 << c.vec()
    w3 = gvec(gb, w0, dt)
    plus = bool_names(dt)[0]
    w3(getattr(gb.binary, plus)[dt]) << c.vec()
    return (vc(w), vc(w2), vc(w3)), (mvc(dm.assign_vec(w0, c.m, I)), mvc(dm.assign_vec(w0, c.m)),
                                     mvc(dm.assign_vec(w0, c.m, accum=plus)))


@consumer("GrB_Vector_assign")
def c_assign_w(c):
    """w of w[I] << u, plain and accumulated"""
    gb, dt = c.gb, c.dt
    I = _sub(c.n)
    u = other_model(len(I), dt, seed=4)
    plus = bool_names(dt)[0]
    w = c.vec()
    w[I] << gvec(gb, u, dt)
    w2 = c.vec()
    w2(getattr(gb.binary, plus)[dt])[I] << gvec(gb, u, dt)
    return (vc(w), vc(w2)), (mvc(dm.assign_vec(c.m, u, I)), mvc(dm.assign_vec(c.m, u, I, accum=plus)))


@consumer("GrB_Vector_assign")
def c_assign_mask(c):
    """the mask of w(k)[:] << u, every kind, with and without replace"""
    gb, dt = c.gb, c.dt
    w0 = other_model(c.n, dt, seed=9)
    u = other_model(c.n, dt, seed=4)
    got, exp = [], []
    for kind in MASK_KINDS:
        for replace in (False, True):
            w = gvec(gb, w0, dt)
            w(mask_of(c.vec(), kind), replace=replace) << gvec(gb, u, dt)
            got.append(vc(w))
            exp.append(mvc(dm.assign_vec(w0, u, mask=c.m, replace=replace, **mask_kw(kind))))
    return tuple(got), tuple(exp)


@consumer("GxB_Vector_subassign")
def c_subassign(c):
    """u, w and the mask of w[I](k) << u"""
    import subassign_model as sm

    gb, dt = c.gb, c.dt
    P = _perm(c.n, 3)
    I = _sub(c.n)
    w0 = other_model(c.n, dt, seed=9)
    u = other_model(len(I), dt, seed=4)
    un = other_model(c.n, dt, seed=6)
    k = other_model(c.n, "BOOL", seed=5)
    kI = other_model(len(I), "BOOL", seed=5)
    got, exp = [], []
    w = gvec(gb, w0, dt)
    w[P](gvec(gb, k, "BOOL").V) << c.vec()
    got.append(vc(w))
    exp.append(mvc(sm.subassign(w0, c.m, P, mask=k)))
    w = c.vec()
    w[I](gvec(gb, kI, "BOOL").S, replace=True) << gvec(gb, u, dt)
    got.append(vc(w))
    exp.append(mvc(sm.subassign(c.m, u, I, mask=kI, mask_struct=True, replace=True)))
    for kind in MASK_KINDS:
        w = gvec(gb, w0, dt)
        w[P](mask_of(c.vec(), kind), replace=True) << gvec(gb, un, dt)
        got.append(vc(w))
        exp.append(mvc(sm.subassign(w0, un, P, mask=c.m, replace=True, **mask_kw(kind))))
    return tuple(got), tuple(exp)


@consumer("GrB_Row_assign", "GrB_Col_assign")
def c_line_assign(c):
    """u and the mask of C[i, :] << u and C[:, j] << u"""
    import subassign_model as sm

    gb, dt = c.gb, c.dt
    R = mat_model(5, c.n, dt, seed=11, density=0.4)
    Cc = dm.transpose(R)
    u = other_model(c.n, dt, seed=4)
    got, exp = [], []
    C = gmat(gb, R, dt)
    C[2, :] << c.vec()
    got.append(mc(C))
    exp.append(mmc(sm.row_assign(R, c.m, 2)))
    C = gmat(gb, Cc, dt)
    C[:, 2] << c.vec()
    got.append(mc(C))
    exp.append(mmc(sm.col_assign(Cc, c.m, None, 2)))
    for kind in MASK_KINDS:
        C = gmat(gb, R, dt)
        C(mask_of(c.vec(), kind), replace=True)[2, :] << gvec(gb, u, dt)
        got.append(mc(C))
        exp.append(mmc(sm.row_assign(R, u, 2, mask=c.m, replace=True, **mask_kw(kind))))
        C = gmat(gb, Cc, dt)
        C(mask_of(c.vec(), kind))[:, 2] << gvec(gb, u, dt)
        got.append(mc(C))
        exp.append(mmc(sm.col_assign(Cc, u, None, 2, mask=c.m, **mask_kw(kind))))
    return tuple(got), tuple(exp)


@consumer("GxB_Row_subassign", "GxB_Col_subassign")
def c_line_subassign(c):
    """u and the mask of C[i, :](k) << u and C[:, j](k) << u"""
    import subassign_model as sm

    gb, dt = c.gb, c.dt
    R = mat_model(5, c.n, dt, seed=11, density=0.4)
    Cc = dm.transpose(R)
    u = other_model(c.n, dt, seed=4)
    k = other_model(c.n, "BOOL", seed=5)
    got, exp = [], []
    C = gmat(gb, R, dt)
    C[2, :](gvec(gb, k, "BOOL").S) << c.vec()
    got.append(mc(C))
    exp.append(mmc(sm.row_subassign(R, c.m, 2, mask=k, mask_struct=True)))
    C = gmat(gb, Cc, dt)
    C[:, 2](gvec(gb, k, "BOOL").V, replace=True) << c.vec()
    got.append(mc(C))
    exp.append(mmc(sm.col_subassign(Cc, c.m, None, 2, mask=k, replace=True)))
    for kind in ("V", "~S"):
        C = gmat(gb, R, dt)
        C[2, :](mask_of(c.vec(), kind), replace=True) << gvec(gb, u, dt)
        got.append(mc(C))
        exp.append(mmc(sm.row_subassign(R, u, 2, mask=c.m, replace=True, **mask_kw(kind))))
        C = gmat(gb, Cc, dt)
        C[:, 2](mask_of(c.vec(), kind)) << gvec(gb, u, dt)
        got.append(mc(C))
        exp.append(mmc(sm.col_subassign(Cc, u, None, 2, mask=c.m, **mask_kw(kind))))
    return tuple(got), tuple(exp)


@consumer("GrB_Vector_extract")
def c_extract(c):
    """w = u[I] with a permuted and a repeated list, and u as the mask and the accumulated output"""
    gb, dt = c.gb, c.dt
    plus = bool_names(dt)[0]
    P = _perm(c.n, 3)
    rep = np.r_[np.arange(c.n - 1, -1, -3), [0, 0, c.n - 1, 64, 64, 63]]
    src = other_model(c.n, dt, seed=6)
    got = [vc(c.vec()[P].new()), vc(c.vec()[rep].new())]
    exp = [mvc(dm.extract_vec(c.m, P)), mvc(dm.extract_vec(c.m, rep))]
    w = c.vec()
    w(getattr(gb.binary, plus)[dt]) << gvec(gb, src, dt)[P]
    got.append(vc(w))
    exp.append(mvc(dm.write_back(c.m, dm.extract_vec(src, P), accum=plus)))
    w = gvec(gb, c.o, dt)
    w(c.vec().V, replace=True) << gvec(gb, src, dt)[P]
    got.append(vc(w))
    exp.append(mvc(dm.write_back(c.o, dm.extract_vec(src, P), mask=c.m, replace=True)))
    return tuple(got), tuple(exp)


@consumer("GrB_Col_extract", "GrB_Matrix_reduce_Monoid", "GrB_Matrix_reduce_BinaryOp")
def c_matrix_to_vector(c):
    """the mask and the accumulated output of A[:, j] and of the row reductions"""
    gb, dt = c.gb, c.dt
    plus = bool_names(dt)[0]
    A = mat_model(c.n, 6, dt, seed=12, density=0.5)
    col = A[0][:, 4], A[1][:, 4]
    rr = dm.reduce_rows(plus, dt, A)
    acc = getattr(gb.binary, plus)[dt]
    mon = getattr(gb.monoid, plus)[dt]
    got, exp = [], []
    for T, expr in ((col, lambda a: a[:, 4]), (rr, lambda a: a.reduce_rowwise(mon))):
        w = gvec(gb, c.o, dt)
        w(c.vec().V, replace=True) << expr(gmat(gb, A, dt))
        got.append(vc(w))
        exp.append(mvc(dm.write_back(c.o, T, mask=c.m, replace=True)))
        w = c.vec()
        w(acc) << expr(gmat(gb, A, dt))
        got.append(vc(w))
        exp.append(mvc(dm.write_back(c.m, T, accum=plus)))
    w = c.vec()
    gb.base.call("GrB_Matrix_reduce_BinaryOp", [w, None, acc, acc, gmat(gb, A, dt), None])
    got.append(vc(w))
    exp.append(mvc(dm.write_back(c.m, rr, accum=plus)))
    return tuple(got), tuple(exp)


@consumer("GrB_Vector_assign_T", "GxB_Vector_subassign_Scalar")
def c_scalar_assign(c):
    """w(k)[:] << s and w[I](k) << s with the poisoned vector as the mask, and as w"""
    import subassign_model as sm

    gb, dt = c.gb, c.dt
    w0 = other_model(c.n, dt, seed=9)
    s, sv = item(dt, 1), val(dt, 1)
    I, P = _sub(c.n), _perm(c.n, 3)
    k = other_model(c.n, "BOOL", seed=5)
    got, exp = [], []
    for kind in MASK_KINDS:
        w = gvec(gb, w0, dt)
        w(mask_of(c.vec(), kind))[:] << s
        got.append(vc(w))
        exp.append(mvc(dm.assign_vec(w0, sv, mask=c.m, **mask_kw(kind))))
        w = gvec(gb, w0, dt)
        w[P](mask_of(c.vec(), kind), replace=True) << s
        got.append(vc(w))
        exp.append(mvc(sm.subassign(w0, sv, P, mask=c.m, replace=True, **mask_kw(kind))))
    w = c.vec()
    w[I] << s
    got.append(vc(w))
    exp.append(mvc(dm.assign_vec(c.m, sv, I)))
    w = c.vec()
    w(gvec(gb, k, "BOOL").S)[:] << s
    got.append(vc(w))
    exp.append(mvc(dm.assign_vec(c.m, sv, mask=k, mask_struct=True)))
    plus = bool_names(dt)[0]
    w = c.vec()
    w(getattr(gb.binary, plus)[dt])[I] << s
    got.append(vc(w))
    exp.append(mvc(dm.assign_vec(c.m, sv, I, accum=plus)))
    return tuple(got), tuple(exp)


@consumer("GrB_Vector_extractElement_T", "GrB_Vector_extractTuples_T")
def c_extract_element(c):
    """no value at a clear bit -- the last one, one inside the clear word, every fifth -- and the
    stored value at a set one"""
    x = c.vec()
    at = sorted({0, 63, 64 % c.n, c.n - 1, c.n - 2} | set(range(0, c.n, 5)))
    got = tuple(x[i].value for i in at)
    exp = tuple(c.m[1][i].item() if c.m[0][i] else None for i in at)
    assert None in exp and any(e is not None for e in exp)
    return (got, vc(x)), (exp, mvc(c.m))


@consumer("GrB_Vector_removeElement", "GrB_Vector_setElement_T")
def c_remove_then_set(c):
    """removeElement, then setElement at slots that were clear"""
    dt = c.dt
    x, m = c.vec(), c.m
    clear = np.flatnonzero(~m[0])
    for i in (0, int(np.flatnonzero(m[0])[-1])):
        del x[i]
        m = dm.remove_element(m, i)
    del x[int(clear[0])]  # not there
    for i in (int(clear[-1]), int(clear[0])):
        x[i] = item(dt, 1)
        m = dm.set_element(m, i, val(dt, 1))
    return (vc(x), int(x.nvals)), (mvc(m), int(m[0].sum()))


@consumer("GrB_Vector_resize")
def c_resize(c):
    """down below a word boundary and up again, twice: the regrown tail is empty"""
    gb, dt = c.gb, c.dt
    plus = bool_names(dt)[0]
    got, exp = [], []
    for small in (c.n - 3, 40):
        x, m = c.vec(), c.m
        for k in (small, c.n + 70):
            x.resize(k)
            m = dm.resize(m, k)
        got += [vc(x), int(x.nvals), np.asarray(x.reduce(getattr(gb.monoid, plus)[dt]).new().value, dm.NP[dt])]
        exp += [mvc(m), int(m[0].sum()), np.asarray(dm.reduce_scalar(plus, dt, m))]
    return tuple(got), tuple(exp)


@consumer("GrB_Vector_dup")
def c_dup(c):
    """the dup itself, and the dup as an operand"""
    gb, dt = c.gb, c.dt
    o, om = c.other()
    d = c.vec().dup()
    w = c.vec().dup().ewise_add(o, gb.binary.second[dt]).new()
    return (vc(d), int(d.nvals), vc(w)), (mvc(c.m), int(c.m[0].sum()), mvc(dm.ewise("add", "second", dt, c.m, om)))


@consumer("GrB_Vector_clear", "GrB_Vector_wait")
def c_clear_then_set(c):
    """clear keeps the value array: one setElement later only that entry exists"""
    dt = c.dt
    x = c.vec()
    x.wait()
    x.clear()
    n0 = int(x.nvals)
    k = int(np.flatnonzero(~c.m[0])[0])
    x[k] = item(dt, 1)
    return (n0, vc(x)), (0, mvc(dm.set_element(zero_of(c.n, dt), k, val(dt, 1))))


# ---------------------------------------------------------------------- re-forming
@consumer("GxB_Vector_sort")
def c_sort(c):
    import sort_model as som

    gb = c.gb
    got, exp = [], []
    for op in ("lt", "gt"):
        w, p = c.vec().ss.sort(getattr(gb.binary, op))
        W, Pm = som.sort_vector(c.m, op)
        got += [vc(w), vc(p)]
        exp += [mvc(W), mvc(Pm)]
    return tuple(got), tuple(exp)


def _skv(res):
    (n,), (i,), x = res
    return i.astype(np.int64), np.asarray(x)


@consumer("GxB_Vector_selectk", "GxB_Vector_compactify")
def c_selectk_compactify(c):
    import selectk_model as skm

    k = max(3, int(c.m[0].sum()) // 3)
    got, exp = [], []
    for how in ("largest", "first", "smallest", "last"):
        got.append(vc(c.vec().ss.selectk(how, k)))
        exp.append(_skv(skm.selectk_vector(c.m, how, k)))
    for kw in (dict(how="first"), dict(how="largest", size=k), dict(how="smallest", size=k, reverse=True),
               dict(how="last", asindex=True)):
        got.append(vc(c.vec().ss.compactify(**kw)))
        exp.append(_skv(skm.compactify_vector(c.m, **kw)))
    return tuple(got), tuple(exp)


@consumer("GxB_Vector_scan")
def c_scan(c):
    import scan_model as scm

    gb, dt = c.gb, c.dt
    got, exp = [], []
    for mon in ("lor", "land") if dt == "BOOL" else ("plus", "min"):
        got.append(vc(c.vec().ss.scan(getattr(gb.monoid, mon)[dt])))
        exp.append(mvc(scm.scan_vector(c.m, mon, dt)))
    return tuple(got), tuple(exp)


@consumer("GrB_Matrix_diag", "GxB_Matrix_diag")
def c_diag(c):
    import reindex_model as rm

    gb, dt = c.gb, c.dt
    got, exp = [mc(c.vec().diag())], [mmc(rm.diag_matrix(c.m))]
    for k in (1, -2):
        C = gb.Matrix(dt, c.n + abs(k), c.n + abs(k))
        C.ss.build_diag(c.vec(), k)
        got.append(mc(C))
        exp.append(mmc(rm.diag_matrix(c.m, k)))
    return tuple(got), tuple(exp)


@consumer("GxB_Matrix_reshapeDup")
def c_reshape(c):
    import reindex_model as rm

    nr = 5 if c.n == 65 else 28
    assert c.n % nr == 0
    col = c.m[0][:, None], c.m[1][:, None]
    got, exp = [], []
    for order in ("rowwise", "columnwise"):
        got.append(mc(c.vec().ss.reshape(nr, c.n // nr, order=order)))
        exp.append(mmc(rm.reshape(col, (nr, c.n // nr), order)))
    return tuple(got), tuple(exp)


@consumer("GxB_Matrix_concat", "GxB_Matrix_split")
def c_concat_split(c):
    """a tile of a vector concat, first and last; the source of a split"""
    import tile_model as tm

    gb, dt = c.gb, c.dt
    o, om = c.other()
    w = gb.Vector(dt, 2 * c.n)
    w.ss.concat([c.vec(), o])
    w2 = gb.Vector(dt, 2 * c.n)
    w2.ss.concat([o, c.vec()])
    sizes = [33, c.n - 33 - 7, 7]
    tiles = c.vec().ss.split(sizes)
    got = [vc(w), vc(w2)] + [vc(tiles[k]) for k in range(len(sizes))]
    exp = [mvc(tm.concat([c.m, om], dt)), mvc(tm.concat([om, c.m], dt))] + [mvc(t) for t in tm.split(c.m, [sizes])]
    return tuple(got), tuple(exp)


@consumer("GxB_Vector_diag", "GxB_Vector_flatten", "GxB_Vector_bitmap_import", device=True)
def c_as_replaced_output(c):
    """the poisoned vector as an output that is replaced whole: nothing of it may survive"""
    import reindex_model as rm
    import torch

    gb, dt = c.gb, c.dt
    A = mat_model(c.n, c.n + 1, dt, seed=13, density=0.3)
    x = c.vec()
    x.ss.build_diag(gmat(gb, A, dt), 1)
    nr = 5 if c.n == 65 else 28
    F = mat_model(nr, c.n // nr, dt, seed=14, density=0.4)
    y = c.vec()
    gb.base.call("GxB_Vector_flatten", [y, gmat(gb, F, dt), False, None])
    z = c.vec()
    p = other_model(c.n, "BOOL", seed=15)[0]
    words = torch.from_numpy(dc._words(p)).cuda()
    torch.cuda.synchronize()
    assert gb.lib.GxB_Vector_bitmap_import(z._h, ctypes.c_void_p(words.data_ptr()), len(words)) == 0
    return (vc(x), vc(y), vc(z)), (mvc(rm.diag_vector(A, 1)), mvc(rm.flatten(F)), mvc(pv_of(p, val(dt, 1), dt)))


# ---------------------------------------------------------------------- export
@consumer("GxB_Vector_export_dense", device=True)
def c_to_dense(c):
    """the fill value, not the poison, stands at clear bits: host and device, with and without bitmap="""
    import torch

    dt = c.dt
    t = dm.NP[dt]
    fill = item(dt, 1)
    want = np.where(c.m[0], c.m[1], t(fill))
    got, exp = [], []
    out = np.zeros(c.n, t)
    c.vec().to_dense(fill, out=out)
    got.append(out)
    exp.append(want)
    out, bm = np.zeros(c.n, t), np.full(c.n, 7, np.int8)
    c.vec().to_dense(fill, out=out, bitmap=bm)
    got += [out, bm]
    exp += [want, c.m[0].astype(np.int8)]
    out, bm = np.full(c.n, 1, t), np.full(c.n, 7, np.int8)
    c.vec().to_dense(out=out, bitmap=bm)  # no fill: zero bytes where there is no entry
    got += [out, bm]
    exp += [c.m[1], c.m[0].astype(np.int8)]
    dev = torch.zeros(c.n, dtype=getattr(torch, np.dtype(t).name if dt != "BOOL" else "bool"), device="cuda")
    dbm = torch.full((c.n,), 7, dtype=torch.int8, device="cuda")
    c.vec().to_dense(fill, out=dev, bitmap=dbm)
    torch.cuda.synchronize()
    got += [dev.cpu().numpy(), dbm.cpu().numpy()]
    exp += [want, c.m[0].astype(np.int8)]
    return tuple(got), tuple(exp)


@consumer("GrB_Vector_extractTuples_T", "GxB_Vector_export_sparse", "GxB_Vector_bitmap_export", device=True)
def c_to_coo(c):
    import torch

    gb = c.gb
    i, v = c.vec().to_coo(device=True)
    torch.cuda.synchronize()
    nw = (c.n + 63) // 64
    words = torch.zeros(nw, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    x = c.vec()
    assert gb.lib.GxB_Vector_bitmap_export(x._h, ctypes.c_void_p(words.data_ptr()), nw) == 0
    torch.cuda.synchronize()
    e = mvc(c.m)
    return (vc(c.vec()), (i.cpu().numpy(), v.cpu().numpy()), words.cpu().numpy()), (e, e, dc._words(c.m[0]))


# entry points that take a GrB_Vector and have no row, each with the reason
VECTOR_INPUT_EXCLUDED = {
    "GrB_Vector_build_T": "the output of a build must hold no entry: it is a producer (part B)",
    "GxB_Vector_build_Scalar_T": "the output of a build must hold no entry: it is a producer (part B)",
    "GrB_Vector_size": "reads the dimension only",
    "GrB_Vector_error": "reads the error string only",
    "GxB_Vector_type": "reads the type only",
    "GrB_Vector_extractElement_Scalar": "a host wrapper of the typed form, which has a row",
    "GrB_Vector_setElement_Scalar": "a host wrapper of the typed form and of removeElement, which have rows",
    "GrB_Vector_assign_Scalar": "reads the GrB_Scalar on the host and runs the typed form, which has a row",
    "GrB_Vector_apply_BinaryOp1st_Scalar": "reads the GrB_Scalar on the host and runs the typed form, which has a row",
    "GrB_Vector_apply_BinaryOp2nd_Scalar": "reads the GrB_Scalar on the host and runs the typed form, which has a row",
    "GxB_Vector_device_view": "the poison itself goes through it",
    "GxB_Vector_device_touch": "declares that stored content changed: the poison changes none, and the touch "
                               "would reset the host's beliefs",
    "GxB_Vector_publish_ticket": "reads the count mailbox's ticket only",
    "GxB_Vector_wait_ticket": "reads the count mailbox only",
    "GxB_PeerWindow_put": "needs a window shared between ranks; moves bitmap words only (test_peer_exchange.py)",
    "GxB_PeerWindow_wait": "needs a window shared between ranks; its output is an iso vector (test_peer_exchange.py)",
}


# ---------------------------------------------------------------------- the header
def header_functions(text):
    """{name: [parameter declarations]} of every entry point; a typed family is one name, `..._T`"""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = text.replace("\\\n", " ")
    out = {}
    for m in re.finditer(r"GrB_Info\s+(\w+?)(_##T)?\s*\(([^)]*)\)", text):
        name = m.group(1) + ("_T" if m.group(2) else "")
        out[name] = [re.sub(r"\s+", " ", p.strip()) for p in m.group(3).split(",")]
    return out


def takes_vector(params):
    return any(re.match(r"(const )?GrB_Vector \w+$", p) for p in params)


def writes_object(params):
    """a GrB_Matrix / GrB_Vector parameter that is not const, or a pointer to one"""
    return any(re.match(r"GrB_(Matrix|Vector) ?\*? ?\w+$", p) for p in params)


# ====================================================================== part B: the producers
BTYPES = ("INT32", "FP64", "BOOL")
ROW_LENGTHS = (0, 1, 63, 64, 65, 129)  # rows 0..5 of the 70 x 300 matrices (indexing table)
SHAPE = (70, 300)


def big_model(dt, shape=SHAPE, seed=21, density=0.04):
    """70 x 300 with one row each of 0, 1, 63, 64, 65 and 129 entries; values 1..3"""
    rng = np.random.default_rng(seed * 7919 + shape[0] * 31 + shape[1])
    p = rng.random(shape) < density
    for r, k in enumerate(ROW_LENGTHS):
        if r < shape[0] and k <= shape[1]:
            p[r] = False
            p[r, rng.choice(shape[1], k, replace=False)] = True
    k = np.add.outer(np.arange(shape[0]) * 2, np.arange(shape[1]))
    return pv_of(p, (k % 3 != 0) if dt == "BOOL" else (k % 3 + 1), dt)


def iso_model(dt, shape=SHAPE, seed=22):
    p = big_model(dt, shape, seed)[0]
    return pv_of(p, val(dt, 1), dt)


def giso(gb, pv, dt):
    r, c, _ = dm.to_coo(pv)
    return gb.Matrix.from_coo(r, c, item(dt, 1), dtype=dt, nrows=pv[0].shape[0], ncols=pv[0].shape[1])


class Producer:
    def __init__(self, name, entries, fn, types, device=False):
        self.name, self.entries, self.fn, self.types, self.device = name, tuple(entries), fn, tuple(types), device


PRODUCERS = {}


def producer(*entries, types=BTYPES, name=None, device=False):
    def wrap(fn):
        k = name or fn.__name__[2:]
        assert k not in PRODUCERS, k
        PRODUCERS[k] = Producer(k, entries, fn, types, device)
        return fn
    return wrap


def _square_mask(n, seed=23, density=0.15):
    rng = np.random.default_rng(seed + n)
    p = rng.random((n, n)) < density
    p[0, :] = True
    return p, p.copy()


# ---------------------------------------------------------------------- products
@producer("GrB_mxm")
def p_mxm_dot(gb, dt):
    """C<M.S> = A A' through the masked dot: the write-back keeps within_mask"""
    plus, times, _ = bool_names(dt)
    A, M = big_model(dt), _square_mask(SHAPE[0])
    a, m = gmat(gb, A, dt), gmat(gb, M, "BOOL")
    C = gb.Matrix(dt, SHAPE[0], SHAPE[0])
    with knobs(gb, mxm_method=1):
        C(m.S) << a.mxm(a.T, sr_of(gb, plus, times, dt))
    T = dm.mxm(plus, times, dt, A, A, tran1=True)
    return C, dm.write_back(zero_of(T[0].shape, dt), T, mask=M, mask_struct=True)


def _p_mxm(method):
    def fn(gb, dt):
        plus, times, _ = bool_names(dt)
        A, B = big_model(dt), big_model(dt, (SHAPE[1], 60), seed=24, density=0.03)
        with knobs(gb, spgemm_method=method):
            C = gmat(gb, A, dt).mxm(gmat(gb, B, dt), sr_of(gb, plus, times, dt)).new()
        return C, dm.mxm(plus, times, dt, A, B)
    return fn


producer("GrB_mxm", name="mxm_hash")(_p_mxm(0))
producer("GrB_mxm", name="mxm_esc")(_p_mxm(1))


def _frontiers(k, n, seed=25):
    p = np.zeros((k, n), bool)
    p[np.arange(n) % k, np.arange(n)] = np.random.default_rng(seed).random(n) < 0.1
    p[0, 0] = True
    return p, p.copy()


@producer("GrB_mxm", types=("BOOL",))
def p_mxm_colbits(gb, dt):
    """7 x 300 = Q0 any.pair A with the colbits knob: the result is resident in column words"""
    Q0, A = _frontiers(7, SHAPE[1]), iso_model("BOOL", (SHAPE[1], SHAPE[1]), seed=26)
    q, a = giso(gb, Q0, "BOOL"), giso(gb, A, "BOOL")
    with knobs(gb, colbits=1):
        q << q.mxm(a, gb.semiring.any_pair["BOOL"])
    return q, dm.mxm("any", "pair", "BOOL", Q0, A)


@producer("GrB_Matrix_assign_T", types=("INT32",))
def p_colbits_stamp(gb, dt):
    """V<Q.V> = 2 on a 7 x 300 matrix held in column words: the stamp is a pending layer"""
    Q0, A = _frontiers(7, SHAPE[1]), iso_model("BOOL", (SHAPE[1], SHAPE[1]), seed=26)
    q, a = giso(gb, Q0, "BOOL"), giso(gb, A, "BOOL")
    V = gb.Matrix(dt, 7, SHAPE[1])
    with knobs(gb, colbits=1):
        V(mask=q.V)[:, :] = 1
        q << q.mxm(a, gb.semiring.any_pair["BOOL"])
        V(mask=q.V)[:, :] = 2
    Q1 = dm.mxm("any", "pair", "BOOL", Q0, A)
    m = dm.assign(zero_of(Q0[0].shape, dt), val(dt, 1), mask=Q0)
    return V, dm.assign(m, val(dt, 2), mask=Q1)


@producer("GrB_mxm")
def p_mxm_any_pair(gb, dt):
    """an iso result set by the producer (gb_spgemm: T.iso)"""
    A, B = big_model(dt), big_model(dt, (SHAPE[1], 60), seed=24, density=0.03)
    C = gmat(gb, A, dt).mxm(gmat(gb, B, dt), gb.semiring.any_pair[dt]).new()
    return C, dm.mxm("any", "pair", dt, A, B)


@producer("GrB_mxm", types=("INT32", "FP64"))
def p_mxm_plus_pair_iso(gb, dt):
    A, B = iso_model(dt), iso_model(dt, (SHAPE[1], 60), seed=24)
    C = giso(gb, A, dt).mxm(giso(gb, B, dt), gb.semiring.plus_pair[dt]).new()
    return C, dm.mxm("plus", "pair", dt, A, B)


@producer("GrB_mxv", name="mxv_general_65")
def p_mxv_65(gb, dt):
    plus, times, _ = bool_names(dt)
    A, u = mat_model(65, 40, dt, seed=27), other_model(40, dt)
    return gmat(gb, A, dt).mxv(gvec(gb, u, dt), sr_of(gb, plus, times, dt)).new(), dm.mxv(plus, times, dt, A, u)


@producer("GrB_vxm", name="vxm_general_700")
def p_vxm_700(gb, dt):
    plus, times, _ = bool_names(dt)
    A, u = mat_model(60, 700, dt, seed=28, density=0.02), other_model(60, dt)
    return gvec(gb, u, dt).vxm(gmat(gb, A, dt), sr_of(gb, plus, times, dt)).new(), dm.vxm(plus, times, dt, u, A)


def _bfs(gb, mxv, **kw):
    """three levels of the BFS loop: q is the iso frontier of level 4, with its hint, its mailbox
    and a pooled bitmap live"""
    m = dc.make("G")
    A = dc.to_gb(gb, m)
    n = m.shape[0]
    v, q = gb.Vector(gb.INT32, n), gb.Vector(bool, n)
    q[dc.SRC] = True
    with knobs(gb, **kw):
        for d in (1, 2, 3):
            v(mask=q.V)[:] = d
            if mxv:
                q(~v.S, replace=True) << A.mxv(q, gb.semiring.any_pair)
            else:
                q(~v.S, replace=True) << q.vxm(A, gb.semiring.any_pair)
    lev, _ = dc.ref_bfs(m.pv[0], dc.SRC)
    return (q, v), (pv_of(lev == 4, True, "BOOL"), pv_of((lev > 0) & (lev <= 3), lev, "INT32"))


@producer("GrB_vxm", types=("BOOL",))
def p_vxm_iso_bfs(gb, dt):
    (q, _), (qm, _) = _bfs(gb, False)
    return q, qm


@producer("GrB_vxm", types=("BOOL",))
def p_vxm_iso_bfs_push(gb, dt):
    (q, _), (qm, _) = _bfs(gb, False, spmv_direction=2, push_heavy=dc.PUSH_HEAVY)
    return q, qm


@producer("GrB_mxv", types=("BOOL",))
def p_mxv_iso_bfs_pull(gb, dt):
    (q, _), (qm, _) = _bfs(gb, True, spmv_direction=1)
    return q, qm


@producer("GrB_Vector_assign_T", types=("INT32",))
def p_bfs_levels(gb, dt):
    """the level vector of the same loop: stamped by the fused masked scalar assigns"""
    (_, v), (_, vm) = _bfs(gb, False)
    return v, vm


@producer("GrB_Vector_assign_T", types=("INT32",))
def p_deferred_stamp(gb, dt):
    """v<q> = d recorded by the loop's deferral.  The library promises that no call observes a
    deferral: the first unrelated call (here the free of q) carries it out, so this row covers
    that resolve and what it leaves; test_live_deferral_meets_its_consumer has the live state"""
    n = dc.N
    v, q = gb.Vector(dt, n), gb.Vector(bool, n)
    v[5] = 7
    q[dc.SRC] = True
    v(mask=q.V)[:] = 1
    m = dm.set_element(dm.set_element(zero_of(n, dt), 5, val(dt, 7)), dc.SRC, val(dt, 1))
    return v, m


@producer("GrB_Vector_setElement_T", types=("BOOL",))
def p_pending_root(gb, dt):
    """q[src] = true on an empty BOOL vector, recorded as the loop's pending root and carried out
    by the next unrelated call: this row covers that resolve (the live state: see p_deferred_stamp)"""
    q = gb.Vector(bool, dc.N)
    q[dc.SRC] = True
    return q, dm.set_element(zero_of(dc.N, "BOOL"), dc.SRC, True)


def _pair(dt, vector, n=700):
    if vector:
        return vec_model(n, dt), other_model(n, dt)
    return big_model(dt), big_model(dt, seed=29, density=0.1)


def _g(gb, pv, dt):
    return gvec(gb, pv, dt) if pv[0].ndim == 1 else gmat(gb, pv, dt)


def _p_ewise(kind, vector):
    def fn(gb, dt):
        import union_model as um

        plus = bool_names(dt)[0]
        A, B = _pair(dt, vector, 65 if kind == "mult" else 700)
        a, b, op = _g(gb, A, dt), _g(gb, B, dt), getattr(gb.binary, plus)[dt]
        if kind == "union":
            return a.ewise_union(b, op, item(dt, 1), item(dt, 1)).new(), um.ewise_union(plus, dt, A, val(dt, 1), B, val(dt, 1))
        return getattr(a, f"ewise_{kind}")(b, op).new(), dm.ewise(kind, plus, dt, A, B)
    return fn


for _kind, _e in (("add", "eWiseAdd_BinaryOp"), ("mult", "eWiseMult_BinaryOp"), ("union", "eWiseUnion")):
    _pre = "GxB" if _kind == "union" else "GrB"
    producer(f"{_pre}_Matrix_{_e}", name=f"matrix_ewise_{_kind}")(_p_ewise(_kind, False))
    producer(f"{_pre}_Vector_{_e}", name=f"vector_ewise_{_kind}")(_p_ewise(_kind, True))


def _p_apply(form, vector):
    def fn(gb, dt):
        import index_apply_model as im

        A = _pair(dt, vector, 65 if form == "left" else 700)[0]
        a = _g(gb, A, dt)
        if form == "unary":
            op = "lnot" if dt == "BOOL" else "ainv"
            return a.apply(getattr(gb.unary, op)[dt]).new(), dm.apply(op, dt, A)
        if form == "index":
            return a.apply("rowindex", 1).new(), im.index_apply(A, "rowindex", _index_type(dt), 1)
        op = "lxor" if dt == "BOOL" else "plus"
        s = gb.Scalar.from_value(item(dt, 1), dt)
        kw = {form: s}
        return a.apply(getattr(gb.binary, op)[dt], **kw).new(), dm.apply(op, dt, A, **{form: val(dt, 1)})
    return fn


for _form, _e in (("unary", "apply"), ("left", "apply_BinaryOp1st_T"), ("right", "apply_BinaryOp2nd_T"),
                  ("index", "apply_IndexOp_T")):
    producer(f"GrB_Matrix_{_e}", name=f"matrix_apply_{_form}")(_p_apply(_form, False))
    producer(f"GrB_Vector_{_e}", name=f"vector_apply_{_form}")(_p_apply(_form, True))


@producer("GrB_Matrix_select_T")
def p_matrix_select(gb, dt):
    A = big_model(dt)
    keep = np.triu(A[0], 3)
    C = gmat(gb, A, dt).select("triu", 3).new()
    return C, pv_of(keep, A[1], dt)


@producer("GrB_Vector_select_T")
def p_vector_select(gb, dt):
    u = vec_model(700, dt)
    y = val(dt, 0 if dt == "BOOL" else 1)
    keep = u[0] & (u[1] > y)
    return gvec(gb, u, dt).select(gb.select.valuegt, y).new(), pv_of(keep, u[1], dt)


def _p_kronecker(form):
    def fn(gb, dt):
        """(2 x 3) (x) (35 x 100)"""
        plus, times, _ = bool_names(dt)
        K, L = mat_model(2, 3, dt, seed=30, density=0.7), big_model(dt, (35, 100), seed=31)
        k, l = gmat(gb, K, dt), gmat(gb, L, dt)
        if form == "Semiring":
            C = gb.Matrix(dt, 70, 300)
            gb.base.call("GrB_Matrix_kronecker_Semiring", [C, None, None, sr_of(gb, plus, times, dt), k, l, None])
        else:
            C = k.kronecker(l, getattr(gb.binary if form == "BinaryOp" else gb.monoid, times)[dt]).new()
        return C, pv_of(np.kron(K[0], L[0]), np.kron(K[1], L[1]), dt)
    return fn


for _form in ("BinaryOp", "Monoid", "Semiring"):
    producer(f"GrB_Matrix_kronecker_{_form}", name=f"kronecker_{_form.lower()}")(_p_kronecker(_form))


@producer("GrB_transpose")
def p_transpose(gb, dt):
    A = big_model(dt)
    return gmat(gb, A, dt).T.new(), dm.transpose(A)


# ---------------------------------------------------------------------- indexing and re-forming
EX_I = np.r_[np.arange(0, 70, 2), [5, 5, 3]]
EX_J = np.r_[np.arange(299, -1, -3), [0, 64, 64]]


@producer("GrB_Matrix_extract")
def p_extract_matrix(gb, dt):
    A = big_model(dt)
    return gmat(gb, A, dt)[EX_I, EX_J].new(), dm.extract(A, EX_I, EX_J)


@producer("GrB_Col_extract")
def p_extract_column(gb, dt):
    A = mat_model(700, 6, dt, seed=12, density=0.5)
    return gmat(gb, A, dt)[:, 4].new(), (A[0][:, 4].copy(), A[1][:, 4].copy())


@producer("GrB_Vector_extract")
def p_extract_vector(gb, dt):
    u, I = vec_model(700, dt), _perm(700, 3)[:65]
    return gvec(gb, u, dt)[I].new(), dm.extract_vec(u, I)


AS_I = np.array([64, 0, 5, 33, 69])
AS_J = np.array([7, 64, 129, 299, 0, 63])


@producer("GrB_Matrix_assign_T")
def p_assign_matrix_scalar(gb, dt):
    A = big_model(dt)
    a = gmat(gb, A, dt)
    a[AS_I, AS_J] << item(dt, 1)
    return a, dm.assign(A, val(dt, 1), AS_I, AS_J)


@producer("GxB_Matrix_subassign", "GrB_Matrix_assign")
def p_assign_matrix(gb, dt):
    """C[I, J] << B, then C(M.S) << D over the whole of C"""
    A, B = big_model(dt), mat_model(len(AS_I), len(AS_J), dt, seed=32, density=0.5)
    D, M = big_model(dt, seed=29, density=0.1), big_model("BOOL", seed=33, density=0.3)
    a = gmat(gb, A, dt)
    a[AS_I, AS_J] << gmat(gb, B, dt)
    a(gmat(gb, M, "BOOL").S) << gmat(gb, D, dt)
    return a, dm.assign(dm.assign(A, B, AS_I, AS_J), D, mask=M, mask_struct=True)


@producer("GxB_Matrix_subassign_Scalar")
def p_subassign_matrix_scalar(gb, dt):
    import subassign_model as sm

    A, M = big_model(dt), mat_model(len(AS_I), len(AS_J), "BOOL", seed=32, density=0.5)
    a = gmat(gb, A, dt)
    a[AS_I, AS_J](gmat(gb, M, "BOOL").S) << item(dt, 1)
    return a, sm.subassign(A, val(dt, 1), AS_I, AS_J, mask=M, mask_struct=True)


@producer("GrB_Row_assign", "GrB_Col_assign", "GxB_Row_subassign", "GxB_Col_subassign")
def p_line_assign(gb, dt):
    import subassign_model as sm

    A = big_model(dt)
    u, w = other_model(SHAPE[1], dt), other_model(SHAPE[0], dt)
    k, kc = other_model(SHAPE[1], "BOOL", seed=5), other_model(SHAPE[0], "BOOL", seed=5)
    a = gmat(gb, A, dt)
    a[0, :] << gvec(gb, u, dt)
    a[:, 64] << gvec(gb, w, dt)
    a[4, :](gvec(gb, k, "BOOL").S) << gvec(gb, u, dt)
    a[:, 7](gvec(gb, kc, "BOOL").S) << gvec(gb, w, dt)
    m = sm.col_assign(sm.row_assign(A, u, 0), w, None, 64)
    m = sm.col_subassign(sm.row_subassign(m, u, 4, mask=k, mask_struct=True), w, None, 7, mask=kc, mask_struct=True)
    return a, m


@producer("GrB_Vector_assign", "GxB_Vector_subassign")
def p_assign_vector(gb, dt):
    import subassign_model as sm

    w0, I = vec_model(700, dt), _sub(700)
    u, k = other_model(len(I), dt, seed=4), other_model(len(I), "BOOL", seed=5)
    w = gvec(gb, w0, dt)
    w[I] << gvec(gb, u, dt)
    w[I](gvec(gb, k, "BOOL").V, replace=True) << gvec(gb, u, dt)
    return w, sm.subassign(dm.assign_vec(w0, u, I), u, I, mask=k, replace=True)


@producer("GrB_Vector_assign_T", "GxB_Vector_subassign_Scalar")
def p_assign_vector_scalar(gb, dt):
    import subassign_model as sm

    w0, I = vec_model(65, dt), _sub(65)
    k = other_model(len(I), "BOOL", seed=5)
    w = gvec(gb, w0, dt)
    w[I] << item(dt, 1)
    w[I](gvec(gb, k, "BOOL").S) << item(dt, 0)
    return w, sm.subassign(dm.assign_vec(w0, val(dt, 1), I), val(dt, 0), I, mask=k, mask_struct=True)


@producer("GrB_Matrix_reduce_BinaryOp")
def p_reduce_binaryop(gb, dt):
    plus = bool_names(dt)[0]
    A = big_model(dt)
    w = gb.Vector(dt, SHAPE[0])
    gb.base.call("GrB_Matrix_reduce_BinaryOp", [w, None, None, getattr(gb.binary, plus)[dt], gmat(gb, A, dt), None])
    return w, dm.reduce_rows(plus, dt, A)


@producer("GrB_Matrix_reduce_Monoid")
def p_reduce_vector(gb, dt):
    plus = bool_names(dt)[0]
    A = big_model(dt)
    return gmat(gb, A, dt).reduce_rowwise(getattr(gb.monoid, plus)[dt]).new(), dm.reduce_rows(plus, dt, A)


@producer("GrB_Matrix_reduce_Monoid")
def p_reduce_columns(gb, dt):
    mn = bool_names(dt)[2]
    A = big_model(dt)
    return gmat(gb, A, dt).reduce_columnwise(getattr(gb.monoid, mn)[dt]).new(), dm.reduce_cols(mn, dt, A)


def _p_sort(which, vector):
    def fn(gb, dt):
        import sort_model as som

        A = vec_model(700, dt) if vector else big_model(dt)
        out = _g(gb, A, dt).ss.sort()
        model = som.sort_vector(A) if vector else som.sort_matrix(A)
        return out[which], model[which]
    return fn


producer("GxB_Matrix_sort", name="matrix_sort_values")(_p_sort(0, False))
producer("GxB_Matrix_sort", name="matrix_sort_permutation")(_p_sort(1, False))
producer("GxB_Vector_sort", name="vector_sort_values")(_p_sort(0, True))
producer("GxB_Vector_sort", name="vector_sort_permutation")(_p_sort(1, True))


def _from_sk(res, dt, shape):
    _, idx, x = res
    P = np.zeros(shape, bool)
    V = np.zeros(shape, np.asarray(x).dtype)
    P[idx], V[idx] = True, x
    return P, V


@producer("GxB_Matrix_selectk")
def p_matrix_selectk(gb, dt):
    import selectk_model as skm

    A = big_model(dt)
    return gmat(gb, A, dt).ss.selectk("largest", 3), _from_sk(skm.selectk(A, "largest", 3), dt, SHAPE)


@producer("GxB_Vector_selectk")
def p_vector_selectk(gb, dt):
    import selectk_model as skm

    u = vec_model(700, dt)
    return gvec(gb, u, dt).ss.selectk("smallest", 200), _from_sk(skm.selectk_vector(u, "smallest", 200), dt, (700,))


@producer("GxB_Matrix_compactify")
def p_matrix_compactify(gb, dt):
    import selectk_model as skm

    A = big_model(dt)
    return gmat(gb, A, dt).ss.compactify("first", 70), _from_sk(skm.compactify(A, "first", 70), dt, (SHAPE[0], 70))


@producer("GxB_Vector_compactify")
def p_vector_compactify(gb, dt):
    import selectk_model as skm

    u = vec_model(700, dt)
    return (gvec(gb, u, dt).ss.compactify("last", 400),
            _from_sk(skm.compactify_vector(u, "last", 400), dt, (400,)))


def _p_scan(vector):
    def fn(gb, dt):
        import scan_model as scm

        mon = bool_names(dt)[0]
        A = vec_model(65, dt) if vector else big_model(dt)
        out = _g(gb, A, dt).ss.scan(getattr(gb.monoid, mon)[dt])
        return out, (scm.scan_vector if vector else scm.scan_matrix)(A, mon, dt)
    return fn


producer("GxB_Matrix_scan", name="matrix_scan")(_p_scan(False))
producer("GxB_Vector_scan", name="vector_scan")(_p_scan(True))


@producer("GxB_Matrix_concat")
def p_concat_matrix(gb, dt):
    import tile_model as tm

    A, B = big_model(dt, (35, 300), seed=34), big_model(dt, (35, 300), seed=35)
    C = gb.Matrix(dt, 70, 300)
    C.ss.concat([[gmat(gb, A, dt)], [gmat(gb, B, dt)]])
    return C, tm.concat([[A], [B]], dt)


@producer("GxB_Matrix_concat")
def p_concat_vector(gb, dt):
    import tile_model as tm

    a, b = vec_model(65, dt), other_model(635, dt)
    w = gb.Vector(dt, 700)
    w.ss.concat([gvec(gb, a, dt), gvec(gb, b, dt)])
    return w, tm.concat([a, b], dt)


@producer("GxB_Matrix_split")
def p_split_matrix(gb, dt):
    """one tile of a split: rows 3.., columns 60.."""
    A = big_model(dt, (73, 360), seed=36)
    tile = gmat(gb, A, dt).ss.split([[3, 70], [60, 300]])[1][1]
    return tile, (A[0][3:, 60:].copy(), A[1][3:, 60:].copy())


@producer("GxB_Matrix_split")
def p_split_vector(gb, dt):
    u = vec_model(700, dt)
    tile = gvec(gb, u, dt).ss.split([635, 65])[1]
    return tile, (u[0][635:].copy(), u[1][635:].copy())


@producer("GrB_Matrix_diag")
def p_diag_new(gb, dt):
    import reindex_model as rm

    u = vec_model(65, dt)
    return gvec(gb, u, dt).diag(2), rm.diag_matrix(u, 2)


@producer("GxB_Matrix_diag")
def p_diag_matrix(gb, dt):
    import reindex_model as rm

    u = vec_model(65, dt)
    C = gmat(gb, big_model(dt, (66, 66), seed=37), dt)
    C.ss.build_diag(gvec(gb, u, dt), -1)
    return C, rm.diag_matrix(u, -1)


@producer("GxB_Vector_diag")
def p_diag_vector(gb, dt):
    import reindex_model as rm

    A = big_model(dt, (70, 70), seed=38, density=0.5)
    w = gb.Vector(dt, 65)
    w.ss.build_diag(gmat(gb, A, dt), 5)
    return w, rm.diag_vector(A, 5)


@producer("GxB_Matrix_reshape")
def p_reshape_inplace(gb, dt):
    import reindex_model as rm

    A = big_model(dt)
    a = gmat(gb, A, dt)
    a.ss.reshape(140, 150, inplace=True)
    return a, rm.reshape(A, (140, 150))


@producer("GxB_Matrix_reshapeDup")
def p_reshape_dup(gb, dt):
    import reindex_model as rm

    A = big_model(dt)
    return gmat(gb, A, dt).ss.reshape(100, 210, order="columnwise"), rm.reshape(A, (100, 210), "columnwise")


@producer("GxB_Matrix_reshapeDup")
def p_reshape_vector(gb, dt):
    import reindex_model as rm

    u = vec_model(700, dt)
    return gvec(gb, u, dt).ss.reshape(28, 25), rm.reshape((u[0][:, None], u[1][:, None]), (28, 25))


@producer("GxB_Vector_flatten")
def p_flatten(gb, dt):
    import reindex_model as rm

    A = big_model(dt, (28, 25), seed=39, density=0.4)
    return gmat(gb, A, dt).ss.flatten(), rm.flatten(A)


# ---------------------------------------------------------------------- import and lifecycle
def _torch_of(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@producer("GxB_Matrix_import_dense", device=True)
def p_import_dense_matrix(gb, dt):
    A = big_model(dt)
    X = np.where(A[0], A[1], val(dt, 0))
    a = gb.Matrix.from_dense(_torch_of(X), bitmap=_torch_of(A[0].astype(np.int8)))
    return a, A


@producer("GxB_Vector_import_dense")
def p_import_dense_vector(gb, dt):
    u = vec_model(700, dt)
    return gb.Vector.from_dense(np.where(u[0], u[1], val(dt, 0)), bitmap=u[0].astype(np.int8), dtype=dt), u


def _p_import_sparse(fmt):
    def fn(gb, dt):
        A = big_model(dt)
        r, c, v = dm.to_coo(A)
        if fmt == "coo":
            o = np.random.default_rng(40).permutation(r.size)  # unsorted: the sort-and-fold path
            a = gb.Matrix.from_coo(_torch_of(r[o]), _torch_of(c[o]), _torch_of(v[o]), dtype=dt, nrows=SHAPE[0],
                                   ncols=SHAPE[1])
        elif fmt == "csr":
            ptr = np.r_[0, np.cumsum(A[0].sum(1))].astype(np.int64)
            a = gb.Matrix.from_csr(_torch_of(ptr), _torch_of(c), _torch_of(v), dtype=dt, nrows=SHAPE[0], ncols=SHAPE[1])
        else:
            rt, ct, vt = dm.to_coo(dm.transpose(A))
            ptr = np.r_[0, np.cumsum(A[0].sum(0))].astype(np.int64)
            a = gb.Matrix.from_csc(_torch_of(ptr), _torch_of(ct), _torch_of(vt), dtype=dt, nrows=SHAPE[0],
                                   ncols=SHAPE[1])
        return a, A
    return fn


for _fmt in ("coo", "csr", "csc"):
    producer("GxB_Matrix_import_sparse", name=f"import_sparse_{_fmt}", device=True)(_p_import_sparse(_fmt))


@producer("GxB_Vector_import_sparse", device=True)
def p_import_sparse_vector(gb, dt):
    u = vec_model(700, dt)
    i, v = mvc(u)
    return gb.Vector.from_coo(_torch_of(i), _torch_of(v), dtype=dt, size=700), u


@producer("GrB_Matrix_import_T")
def p_import_host_csr(gb, dt):
    A = big_model(dt)
    _, c, v = dm.to_coo(A)
    ptr = np.r_[0, np.cumsum(A[0].sum(1))].astype(np.int64)
    return gb.Matrix.from_csr(ptr, c, v, dtype=dt, nrows=SHAPE[0], ncols=SHAPE[1]), A


@producer("GxB_Matrix_import_device", device=True)
def p_import_device(gb, dt):
    import torch

    A = big_model(dt)
    _, c, v = dm.to_coo(A)
    ptr = _torch_of(np.r_[0, np.cumsum(A[0].sum(1))].astype(np.int64))
    ci, vx = _torch_of(c.astype(np.int32)), _torch_of(v)
    torch.cuda.synchronize()
    from graphblas_amd import device as gdev

    a = gdev.matrix_from_csr(dt, SHAPE[0], SHAPE[1], ptr.data_ptr(), ci.data_ptr(), vx.data_ptr(), int(c.size))
    torch.cuda.synchronize()
    return a, A


@producer("GrB_Matrix_dup")
def p_dup_matrix(gb, dt):
    """the dup of a matrix whose transpose is cached"""
    A = big_model(dt)
    a = gmat(gb, A, dt)
    a.T.new()
    return a.dup(), A


@producer("GrB_Vector_dup")
def p_dup_vector(gb, dt):
    u = vec_model(700, dt)
    return gvec(gb, u, dt).dup(), u


@producer("GrB_Matrix_resize")
def p_resize_matrix(gb, dt):
    A = big_model(dt, (90, 330), seed=41)
    a = gmat(gb, A, dt)
    a.resize(60, 200)
    a.resize(*SHAPE)
    return a, dm.resize(dm.resize(A, (60, 200)), SHAPE)


@producer("GrB_Vector_resize")
def p_resize_vector(gb, dt):
    u = vec_model(700, dt)
    w = gvec(gb, u, dt)
    w.resize(50)
    w.resize(65)
    return w, dm.resize(dm.resize(u, 50), 65)


@producer("GrB_Matrix_clear", "GrB_Matrix_build_T")
def p_clear_build_matrix(gb, dt):
    A, B = big_model(dt), big_model(dt, seed=42)
    a = gmat(gb, A, dt)
    a.T.new()
    a.clear()
    r, c, v = dm.to_coo(B)
    a.build(r, c, v)
    return a, B


@producer("GrB_Vector_clear", "GrB_Vector_build_T")
def p_clear_build_vector(gb, dt):
    u, o = vec_model(700, dt), other_model(700, dt)
    w = gvec(gb, u, dt)
    w.clear()
    i, v = mvc(o)
    w.build(i, v)
    return w, o


@producer("GxB_Matrix_build_Scalar_T")
def p_build_scalar_matrix(gb, dt):
    A = iso_model(dt)
    return giso(gb, A, dt), A


@producer("GxB_Vector_build_Scalar_T")
def p_build_scalar_vector(gb, dt):
    u = pv_of(vec_model(700, dt)[0], val(dt, 1), dt)
    i, _ = mvc(u)
    return gb.Vector.from_coo(i, item(dt, 1), dtype=dt, size=700), u


@producer("GrB_Matrix_new", "GrB_Matrix_setElement_T", "GrB_Matrix_removeElement")
def p_elements_matrix(gb, dt):
    """setElement / removeElement on a new matrix, an element at a time"""
    a = gb.Matrix(dt, *SHAPE)
    m = zero_of(SHAPE, dt)
    rng = np.random.default_rng(43)
    for k in range(60):
        i, j = int(rng.integers(SHAPE[0])), int(rng.integers(SHAPE[1]))
        a[i, j] = item(dt, k % 3 + 1)
        m = dm.set_element(m, (i, j), val(dt, k % 3 + 1))
        if k % 4 == 3:
            r, c, _ = dm.to_coo(m)
            del a[int(r[0]), int(c[0])]
            m = dm.remove_element(m, (int(r[0]), int(c[0])))
            del a[int(r[-1]), int(c[-1])]
            m = dm.remove_element(m, (int(r[-1]), int(c[-1])))
    return a, m


@producer("GrB_Vector_new", "GrB_Vector_setElement_T", "GrB_Vector_removeElement")
def p_elements_vector(gb, dt):
    w = gb.Vector(dt, 65)
    m = zero_of(65, dt)
    for k, i in enumerate([64, 0, 63, 5, 5, 31, 64, 17]):
        w[i] = item(dt, k % 3 + 1)
        m = dm.set_element(m, i, val(dt, k % 3 + 1))
    del w[63]
    del w[0]
    m = dm.remove_element(dm.remove_element(m, 63), 0)
    return w, m


@producer("GrB_Matrix_new")
def p_new_matrix(gb, dt):
    return gb.Matrix(dt, *SHAPE), zero_of(SHAPE, dt)


@producer("GrB_Vector_new")
def p_new_vector(gb, dt):
    return gb.Vector(dt, 700), zero_of(700, dt)


@producer("GxB_Matrix_prepare_transpose")
def p_prepared(gb, dt):
    """a matrix with its CSC and narrow copies built ahead"""
    A = big_model(dt)
    a = gmat(gb, A, dt)
    assert gb.lib.GxB_Matrix_prepare_transpose(a._h) == 0
    return a, A


@producer("GxB_Vector_device_touch", "GxB_Vector_bitmap_import", device=True)
def p_device_written(gb, dt):
    """bits imported from device words (iso true), then half of them cleared through the view"""
    import torch
    from graphblas_amd import device as gdev

    p, keep = vec_model(700, "BOOL")[0], np.arange(700) % 2 == 0
    w = gb.Vector(dt, 700)
    words = _torch_of(dc._words(p))
    torch.cuda.synchronize()
    assert gb.lib.GxB_Vector_bitmap_import(w._h, ctypes.c_void_p(words.data_ptr()), len(words)) == 0
    torch.cuda.synchronize()
    bits = gdev.device_tensor(torch, gdev.vector_view(w._h).bitmap, len(words))
    bits &= _torch_of(dc._words(keep))
    torch.cuda.synchronize()
    assert gb.lib.GxB_Vector_device_touch(w._h) == 0
    return w, pv_of(p & keep, val(dt, 1), dt)


# entry points that write a matrix or a vector and have no row, each with the reason
OBJECT_OUTPUT_EXCLUDED = {
    "GrB_Matrix_free": "destroys the object",
    "GrB_Vector_free": "destroys the object",
    "GrB_Matrix_wait": "completes pending work: the object keeps the form its producer gave it",
    "GrB_Vector_wait": "completes pending work: the object keeps the form its producer gave it",
    "GrB_Matrix_exportSize": "reads the object; the C API declares the parameter without const",
    "GrB_Matrix_exportHint": "reads the object; the C API declares the parameter without const",
    "GrB_Matrix_export_T": "reads the object; the C API declares the parameter without const",
    "GrB_Matrix_apply_BinaryOp1st_Scalar": "reads the GrB_Scalar on the host and runs the typed form, which has a row",
    "GrB_Matrix_apply_BinaryOp2nd_Scalar": "reads the GrB_Scalar on the host and runs the typed form, which has a row",
    "GrB_Vector_apply_BinaryOp1st_Scalar": "reads the GrB_Scalar on the host and runs the typed form, which has a row",
    "GrB_Vector_apply_BinaryOp2nd_Scalar": "reads the GrB_Scalar on the host and runs the typed form, which has a row",
    "GrB_Matrix_apply_IndexOp_Scalar": "reads the GrB_Scalar on the host and runs the typed form, which has a row",
    "GrB_Vector_apply_IndexOp_Scalar": "reads the GrB_Scalar on the host and runs the typed form, which has a row",
    "GrB_Matrix_select_Scalar": "reads the GrB_Scalar on the host and runs the typed form, which has a row",
    "GrB_Vector_select_Scalar": "reads the GrB_Scalar on the host and runs the typed form, which has a row",
    "GrB_Matrix_assign_Scalar": "reads the GrB_Scalar on the host and runs the typed form, which has a row",
    "GrB_Vector_assign_Scalar": "reads the GrB_Scalar on the host and runs the typed form, which has a row",
    "GrB_Matrix_setElement_Scalar": "a host wrapper of the typed form and of removeElement, which have rows",
    "GrB_Vector_setElement_Scalar": "a host wrapper of the typed form and of removeElement, which have rows",
    "GxB_Vector_publish_ticket": "reads the count mailbox's ticket only",
    "GxB_Vector_wait_ticket": "reads the count mailbox only",
    "GxB_Vector_bitmap_export": "reads the bitmap; declared without const",
    "GxB_Matrix_colwords_view": "hands out the column words for a collective to rewrite; needs the exchange of "
                                "test_colbits.py to change anything",
    "GxB_Matrix_colwords_touch": "a recount after such a rewrite: without one it changes nothing",
    "GxB_PeerWindow_wait": "needs a window shared between ranks (test_peer_exchange.py)",
    "GxB_Matrix_rmat": "a generator, not an operation on stored objects: its output is a build of generated tuples, "
                       "checked against the oracle's generator in test_io.py",
}


# ---------------------------------------------------------------------- the batteries
def _fresh_matrix(gb, nr, nc, dt, seed, density=0.1):
    return gmat(gb, mat_model(nr, nc, dt, seed=seed, density=density), dt)


def _mask_call(kind, replace):
    def fn(gb, X, dt):
        nr, nc = X.shape
        C = _fresh_matrix(gb, nr, nc, "INT32", 51, 0.05)
        C(mask_of(X, kind), replace=replace) << _fresh_matrix(gb, nr, 6, "INT32", 52, 0.5).mxm(
            _fresh_matrix(gb, 6, nc, "INT32", 53, 0.5), gb.semiring.plus_times["INT32"])
        return mc(C)
    return fn


def _b_dot(gb, X, dt):
    plus, times, _ = bool_names(dt)
    nr = X.shape[0]
    M = _square_mask(nr, seed=54, density=0.05)
    C = gb.Matrix(dt, nr, nr)
    with knobs(gb, mxm_method=1):
        C(gmat(gb, M, "BOOL").S) << X.mxm(X.T, sr_of(gb, plus, times, dt))
    return mc(C)


def _b_sort(gb, X, dt):
    C, P = X.ss.sort()
    return mc(C), mc(P)


def _b_dup_set(gb, X, dt):
    Y = X.dup()
    Y[X.shape[0] - 1, X.shape[1] - 1] = item(dt, 1)
    Y[0, 0] = item(dt, 0)
    return mc(Y), int(Y.nvals)


def _b_concat(gb, X, dt):
    nr, nc = X.shape
    C = gb.Matrix(dt, nr, 2 * nc)
    C.ss.concat([[X, X]])
    return mc(C)


def _b_csr(gb, X, dt):
    import torch

    out = X.to_csr(device=True)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


def _b_extract(gb, X, dt):
    nr, nc = X.shape
    I = np.r_[np.arange(nr - 1, -1, -2), [0, 0]]
    J = np.r_[np.arange(0, nc, 3), [nc - 1, nc - 1]]
    return mc(X[I, J].new())


def _pt(dt):
    plus, times, _ = bool_names(dt)
    return plus, times


MATRIX_BATTERY = {
    "transpose": lambda gb, X, dt: mc(X.T.new()),
    "mxm_left": lambda gb, X, dt: mc(X.mxm(_fresh_matrix(gb, X.shape[1], 9, dt, 55), sr_of(gb, *_pt(dt), dt)).new()),
    "mxm_right": lambda gb, X, dt: mc(_fresh_matrix(gb, 8, X.shape[0], dt, 56).mxm(X, sr_of(gb, *_pt(dt), dt)).new()),
    "dot": _b_dot,
    "mask_S": _mask_call("S", False),
    "mask_V": _mask_call("V", False),
    "mask_cS_replace": _mask_call("~S", True),
    "mask_cV_replace": _mask_call("~V", True),
    "mxv": lambda gb, X, dt: vc(X.mxv(gvec(gb, other_model(X.shape[1], dt), dt), sr_of(gb, *_pt(dt), dt)).new()),
    "vxm": lambda gb, X, dt: vc(gvec(gb, other_model(X.shape[0], dt), dt).vxm(X, sr_of(gb, *_pt(dt), dt)).new()),
    "ewise_add": lambda gb, X, dt: mc(X.ewise_add(_fresh_matrix(gb, *X.shape, dt, 57), getattr(gb.binary, _pt(dt)[0])[dt]).new()),
    "apply": lambda gb, X, dt: mc(X.apply(getattr(gb.unary, "lnot" if dt == "BOOL" else "ainv")[dt]).new()),
    "select": lambda gb, X, dt: mc(X.select("tril").new()),
    "reduce_rowwise": lambda gb, X, dt: vc(X.reduce_rowwise(getattr(gb.monoid, _pt(dt)[0])[dt]).new()),
    "reduce_columnwise": lambda gb, X, dt: vc(X.reduce_columnwise(getattr(gb.monoid, _pt(dt)[0])[dt]).new()),
    "reduce_scalar": lambda gb, X, dt: X.reduce_scalar(getattr(gb.monoid, _pt(dt)[0])[dt]).new().value,
    "extract": _b_extract,
    "sort": _b_sort,
    "dup_set": _b_dup_set,
    "concat": _b_concat,
    "to_csr": _b_csr,
}


def _vmask_call(kind):
    def fn(gb, X, dt):
        n = X.size
        w = gvec(gb, other_model(n, "INT32", seed=9), "INT32")
        w(mask_of(X, kind), replace=True) << _fresh_matrix(gb, n, 50, "INT32", 58).mxv(
            gvec(gb, other_model(50, "INT32", seed=8), "INT32"), gb.semiring.plus_times["INT32"])
        return vc(w)
    return fn


def _b_vassign(gb, X, dt):
    n = X.size
    w = gvec(gb, other_model(n + 9, dt, seed=9), dt)
    w[_perm(n + 9, 5)[:n]] << X
    return vc(w)


def _b_vdense(gb, X, dt):
    out, bm = np.zeros(X.size, dm.NP[dt]), np.full(X.size, 7, np.int8)
    X.to_dense(item(dt, 1), out=out, bitmap=bm)
    return out, bm


VECTOR_BATTERY = {
    "mxv": lambda gb, X, dt: vc(_fresh_matrix(gb, 40, X.size, dt, 59).mxv(X, sr_of(gb, *_pt(dt), dt)).new()),
    "mask_V": _vmask_call("V"),
    "mask_S": _vmask_call("S"),
    "mask_cS": _vmask_call("~S"),
    "ewise_mult": lambda gb, X, dt: vc(X.ewise_mult(gvec(gb, other_model(X.size, dt), dt), getattr(gb.binary, _pt(dt)[0])[dt]).new()),
    "reduce": lambda gb, X, dt: X.reduce(getattr(gb.monoid, _pt(dt)[0])[dt]).new().value,
    "assign": _b_vassign,
    "extract": lambda gb, X, dt: vc(X[_perm(X.size, 6)].new()),
    "diag": lambda gb, X, dt: mc(X.diag()),
    "to_dense": _b_vdense,
}


def rebuilt(gb, P):
    """R = from_coo(*P.to_coo()): the same content in the tidy storage of a build"""
    dt = P.dtype.name
    if P.ndim == 1:
        i, v = P.to_coo()
        return gb.Vector.from_coo(i, v, dtype=dt, size=P.size)
    r, c, v = P.to_coo()
    return gb.Matrix.from_coo(r, c, v, dtype=dt, nrows=P.nrows, ncols=P.ncols)
