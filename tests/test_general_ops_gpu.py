"""GPU parity of eWise, apply, reduce, transpose, build and the output write-back with the dense
numpy model of tests/dense_model.py (checked on its own by tests/test_dense_model.py).

Every comparison goes through to_coo() and numpy: indices, their order, nvals, the dtype of the
result and the values.  isequal never judges here (it is itself eWiseMult + reduce); the last
tests check isequal against numpy instead.  Inputs are seeded by zlib.crc32 of the parameters.

Shapes, and the path each one is for
  vectors  1, 63, 64, 65   one bitmap word: empty tail lanes, a full word, one bit in a second word
           70001           above 256 x 256 values: the stride loop of k_reduce_partial (256 blocks)
           262245          1024 x 256 + 64 + 37: a second grid sweep of k_ewise_vec / k_vec_merge
                           (both capped at 1024 blocks of 256 threads) ending in a partial word
  matrices 1 x 1, 37 x 53  one block, odd sizes
           3 x 300, 300 x 3  at most 64 rows on one side (the column-word formats' limit)
           301 x 6007      "301 x 257 widened": a third of the rows empty, row 7 holds 5200 entries
           133125 x 64     131072 + 2048 + 5 rows of 0..3 entries: the row pointers of k_ewise_mat,
                           of build and of the transpose come from the wave-tile scan (scanw,
                           gb_prim.hip, from 131072 items up) with a ragged last tile; run again
                           with the knob scan_u8 = 1, which sends the same scans to hipCUB
           131071 x 64     one row short of the threshold: hipCUB
  build    200000 tuples over 300 x 300 with one key 5000 times (a run of k_fold_runs that spans
           blocks of k_heads), and 140000 distinct rows (the build's scans on the wave-tile path)

Tolerances
  Exact (np.array_equal, NaNs position-wise, the sign of zero asserted except for min / max):
  everything integer and bool, all casts and structure, all comparisons, and float plus, minus,
  rminus, times, div, rdiv, min, max, abs, ainv, minv, sqrt, floor, ceil, round, trunc, copysign,
  ldexp, fmod, remainder (numpy in the same type; FP32 sqrt, fmod, remainder: float64 rounded).
  exp .. hypot are compared in ulps with numpy float64 (FP32: float64 rounded to float32).  The
  table holds the largest distance measured on an MI355X over the inputs of these tests; each
  bound is twice that, rounded up to a power of two (0 stays 0):

      op      FP32 measured/bound   FP64 measured/bound
      exp     0 / 0                 1 / 2
      exp2    0 / 0                 1 / 2
      log     0 / 0                 1 / 2
      log2    0 / 0                 1 / 2
      log10   0 / 0                 1 / 2
      sin     0 / 0                 1 / 2
      cos     0 / 0                 1 / 2
      tan     0 / 0                 1 / 2
      atan2   0 / 0                 1 / 2
      hypot   0 / 0                 1 / 2
      pow     1 / 2                 1 / 2

  (FP32 operands are evaluated in double on the device and rounded once, hence 0; pow[FP32] is
  powf.  The float-only unary operators on integer / bool inputs compute in FP32 or FP64 and
  stay within the same bounds.  2 ulps are 2.4e-7 relative in FP32 and 4.4e-16 in FP64, inside
  the project's 1e-6 relative budget.)

  Float plus / times reductions of n values: |got - ref| <= n eps sum|x| (plus, ref math.fsum)
  and n eps |prod| (times, values in [0.5, 2], ref the float64 product), eps = 2^-53 or 2^-24.
"""
import math
import zlib

import numpy as np
import pytest

import dense_model as dm

pytestmark = pytest.mark.gpu

BINARY = ["first", "second", "plus", "minus", "times", "div", "min", "max", "pow", "rminus", "rdiv", "pair",
          "any", "iseq", "isne", "isgt", "islt", "isge", "isle", "lor", "land", "lxor", "lxnor", "eq", "ne",
          "gt", "lt", "ge", "le", "bor", "band", "bxor", "bxnor", "atan2", "hypot", "fmod", "remainder",
          "ldexp", "copysign"]
POSITIONAL = ["firsti", "firsti1", "firstj", "firstj1", "secondi", "secondi1", "secondj", "secondj1"]
UNARY = ["identity", "ainv", "minv", "abs", "lnot", "one", "bnot", "sqrt", "log", "log2", "log10", "exp",
         "exp2", "floor", "ceil", "round", "trunc", "sin", "cos", "tan"]
MONOIDS = ["min", "max", "plus", "times", "lor", "land", "lxor", "lxnor", "eq", "any", "bor", "band", "bxor",
           "bxnor"]

# (op, dtype) -> bound in ulps; see the table above
ULP_BOUND = {("exp", "FP32"): 0, ("exp", "FP64"): 2, ("exp2", "FP32"): 0, ("exp2", "FP64"): 2, ("log", "FP32"): 0, ("log", "FP64"): 2, ("log2", "FP32"): 0, ("log2", "FP64"): 2, ("log10", "FP32"): 0, ("log10", "FP64"): 2, ("sin", "FP32"): 0, ("sin", "FP64"): 2, ("cos", "FP32"): 0, ("cos", "FP64"): 2, ("tan", "FP32"): 0, ("tan", "FP64"): 2, ("atan2", "FP32"): 0, ("atan2", "FP64"): 2, ("hypot", "FP32"): 0, ("hypot", "FP64"): 2, ("pow", "FP32"): 2, ("pow", "FP64"): 2}

SMALL_VEC = [(1,), (63,), (64,), (65,)]
SMALL_MAT = [(1, 1), (37, 53), (3, 300), (300, 3)]


@pytest.fixture(scope="module")
def gb():
    import graphblas_amd

    return graphblas_amd


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


class _knobs:
    def __init__(self, gb, **kv):
        self.gb, self.kv = gb, kv

    def __enter__(self):
        for k, v in self.kv.items():
            self.gb.set_knob(k, v)

    def __exit__(self, *a):
        for k in self.kv:
            self.gb.set_knob(k, 0)


# ---------------------------------------------------------------------- value pools
def specials(dt):
    t = dm.NP[dt]
    if dt == "BOOL":
        return np.array([False, True])
    if dm.is_int(dt):
        lo, hi = dm.tmin(dt), dm.tmax(dt)
        s = [0, 1, 2, 3, 5, 7, hi, hi - 1, hi // 2 + 1]
        if lo < 0:
            s += [-1, -2, -5, lo, lo + 1]
        return np.array(s, t)
    f = np.finfo(t)
    return np.array([0.0, -0.0, np.inf, -np.inf, np.nan, f.smallest_subnormal, -f.smallest_subnormal,
                     f.smallest_normal / 4, f.smallest_normal, 1.0, -1.0, 0.5, -0.5, 1.5, 2.5, -2.5, 3.0,
                     f.max, -f.max], t)


def draw(dt, rng, n, positive=False):
    """n values of dt: half of them specials, the others random (integers over the whole range
    and near zero, floats normal with mixed scales)"""
    t = dm.NP[dt]
    if dt == "BOOL":
        return rng.random(n) < 0.5
    if dm.is_int(dt):
        wide = rng.integers(dm.tmin(dt), dm.tmax(dt), n, dtype=t, endpoint=True)
        near = rng.integers(0 if dm.tmin(dt) == 0 else -9, 10, n).astype(t)
        out = np.where(rng.random(n) < 0.5, wide, near)
    else:
        out = (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, n)).astype(t)
        if positive:
            out = np.abs(out)
    sp = specials(dt)
    pick = rng.random(n) < 0.5
    return np.where(pick, sp[rng.integers(0, sp.size, n)], out).astype(t)


INT_POW_EDGES = [(3, 5), (-2, 63), (2, 63), (0, -1), (2, -1), (0, 0), (-1, 11), (9, 12), (-9, 11)]


def binary_inputs(op, dt, shape, key):
    """two model operands of `shape` for op[dt]: the cross product of the specials first (as
    many pairs as fit in half the cells, both entries present), random values and structure after"""
    rng = _rng("binary", op, dt, shape, key)
    t = dm.NP[dt]
    total = int(np.prod(shape))
    x, y = draw(dt, rng, total), draw(dt, rng, total)
    sp = specials(dt)
    cx, cy = [a.ravel() for a in np.meshgrid(sp, sp, indexing="ij")]
    if op == "pow" and dm.is_int(dt):
        # float64 pow exact or saturating without doubt: |base| <= 9, exponent 0..12, plus edges
        x = rng.integers(0 if dm.tmin(dt) == 0 else -9, 10, total).astype(t)
        y = rng.integers(0, 13, total).astype(t)
        edges = [(a, b) for a, b in INT_POW_EDGES if dm.tmin(dt) < 0 or (a >= 0 and b >= 0)]
        cx, cy = np.array([e[0] for e in edges], t), np.array([e[1] for e in edges], t)
    elif op == "ldexp":
        y = rng.integers(-20, 21, total).astype(t)
        cy = rng.integers(-20, 21, cx.size).astype(t)
    k = min(cx.size, total // 2)
    sel = rng.permutation(cx.size)[:k]
    x[:k], y[:k] = cx[sel], cy[sel]
    if op in ("min", "max") and dm.is_float(dt):  # never -0.0 against +0.0: either answer is right
        clash = (x == 0) & (y == 0) & (np.signbit(x) != np.signbit(y))
        y[clash] = x[clash]
    px, py = rng.random(total) < 0.7, rng.random(total) < 0.7
    px[:k] = py[:k] = True
    if total == 1:
        px[:] = py[:] = True
    return (px.reshape(shape), np.where(px, x, t(0)).reshape(shape)), \
           (py.reshape(shape), np.where(py, y, t(0)).reshape(shape))


def unary_input(op, dt, shape, key):
    rng = _rng("unary", op, dt, shape, key)
    total = int(np.prod(shape))
    x = draw(dt, rng, total, positive=op in ("sqrt", "log", "log2", "log10"))
    sp = specials(dt)
    k = min(sp.size, total)
    x[:k] = sp[:k]
    p = rng.random(total) < 0.7
    p[:k] = True
    return p.reshape(shape), np.where(p, x, dm.NP[dt](0)).reshape(shape)


# ---------------------------------------------------------------------- device <-> model
def to_gb(gb, A, dt=None):
    p, v = A
    dt = dm.name_of(v.dtype) if dt is None else dt
    idx = np.nonzero(p)
    if p.ndim == 1:
        return gb.Vector.from_coo(idx[0], v[idx], dtype=dt, size=p.shape[0])
    return gb.Matrix.from_coo(idx[0], idx[1], v[idx], dtype=dt, nrows=p.shape[0], ncols=p.shape[1])


def iso_gb(gb, p, value, dt):
    """an iso object of structure p (from_coo with a scalar), and its model"""
    idx = np.nonzero(p)
    v = np.where(p, dm.NP[dt](value), dm.NP[dt](0))
    if p.ndim == 1:
        return gb.Vector.from_coo(idx[0], dm.NP[dt](value).item(), dtype=dt, size=p.shape[0]), (p, v)
    return gb.Matrix.from_coo(idx[0], idx[1], dm.NP[dt](value).item(), dtype=dt, nrows=p.shape[0],
                              ncols=p.shape[1]), (p, v)


def coo_of(obj):
    out = obj.to_coo()
    return tuple(np.asarray(i).astype(np.int64) for i in out[:-1]), out[-1]


def check(obj, want, dt, *, ulps=False, zero_sign=True, what=""):
    """structure exactly; values exactly, or (ulps=True) returns their largest ulp distance"""
    wp, wv = want
    assert obj.dtype == dt, f"{what}: dtype {obj.dtype}, expected {dt}"
    assert tuple(obj.shape) == tuple(wp.shape), what
    idx, vals = coo_of(obj)
    widx = np.nonzero(wp)
    assert obj.nvals == widx[0].size, f"{what}: nvals {obj.nvals}, expected {widx[0].size}"
    for a, b in zip(idx, widx):
        assert np.array_equal(a, b), f"{what}: indices differ"
    assert vals.dtype == dm.NP[dt], what
    wvals = wv[widx]
    assert wvals.dtype == dm.NP[dt], f"{what}: model dtype {wvals.dtype}"
    if ulps:
        return dm.ulp_distance(vals, wvals)
    isf = dm.is_float(dt)
    if not np.array_equal(vals, wvals, equal_nan=isf):
        same = (vals == wvals) | ((vals != vals) & (wvals != wvals))
        bad = np.flatnonzero(~same)
        q = bad[0]
        raise AssertionError(f"{what}: {bad.size} of {vals.size} values differ; first at "
                             f"{[int(i[q]) for i in idx]}: got {vals[q]!r}, expected {wvals[q]!r}")
    if isf and zero_sign:
        z = wvals == 0
        assert np.array_equal(np.signbit(vals[z]), np.signbit(wvals[z])), f"{what}: sign of zero"
    return 0


def ulp_report(measured):
    """print every (op, computing dtype, note, worst ulps) figure, then hold each to its bound"""
    for op, ct, note, worst in measured:
        print(f"\nULP {op} {ct} {worst} {note}")
    for op, ct, note, worst in measured:
        bound = ULP_BOUND.get((op, ct), 0)
        assert worst <= bound, f"{op}[{ct}] {note}: {worst} ulps from the float64 reference, bound {bound}"


def typed_info(typed):
    """(model operator name, dtype it computes in, dtype it returns) of a typed operator"""
    name = {"eq": "lxnor"}.get(typed.name, typed.name) if typed.opclass == "Monoid" else typed.name
    return name, typed.type.name, typed.return_type.name


# ---------------------------------------------------------------------- the operator lists
def test_operator_lists_are_complete(gb):
    assert set(vars(gb.binary)) == set(BINARY) | set(POSITIONAL)
    assert set(vars(gb.unary)) == set(UNARY)
    assert set(vars(gb.monoid)) == set(MONOIDS)


# ---------------------------------------------------------------------- eWise sweep
@pytest.mark.parametrize("op", BINARY)
def test_ewise_every_binary_op(gb, op):
    opobj = getattr(gb.binary, op)
    exact = op not in dm.TRANSCENDENTAL
    measured = []
    for dtobj in opobj.types:
        dt = dtobj.name
        zt = dm.binop_return_dtype(op, dt)
        assert opobj[dt].type.name == dt and opobj[dt].return_type.name == zt
        worst = 0
        for shape in SMALL_VEC + SMALL_MAT:
            A, B = binary_inputs(op, dt, shape, "ewise")
            a, b = to_gb(gb, A), to_gb(gb, B)
            for kind in ("mult", "add"):
                got = getattr(a, f"ewise_{kind}")(b, opobj).new()
                want = dm.ewise(kind, op, dt, A, B)
                what = f"ewise_{kind} {op}[{dt}] {shape}"
                if exact or not dm.is_float(dt):
                    check(got, want, zt, zero_sign=op not in ("min", "max"), what=what)
                    continue
                # transcendental: one-sided entries of ewise_add are plain casts and stay exact
                both = A[0] & B[0]
                worst = max(worst, check(got, want, zt, ulps=True, what=what))
                if kind == "add":
                    only = want[0] & ~both
                    gi, gv = coo_of(got)
                    sel = only[gi]
                    assert np.array_equal(gv[sel], want[1][only], equal_nan=True), what
        if not exact and dm.is_float(dt):
            measured.append((op, dt, "ewise", worst))
    ulp_report(measured)


@pytest.mark.parametrize("op", POSITIONAL)
def test_positional_binaries_are_rejected(gb, op):
    opobj = getattr(gb.binary, op)
    A, B = binary_inputs("plus", "INT64", (65,), "positional")
    a, b = to_gb(gb, A), to_gb(gb, B)
    M, N = binary_inputs("plus", "INT64", (37, 53), "positional")
    m, n = to_gb(gb, M), to_gb(gb, N)
    for x, y in ((a, b), (m, n)):
        for kind in ("ewise_mult", "ewise_add"):
            with pytest.raises(gb.exceptions.NotImplementedException):
                getattr(x, kind)(y, opobj).new()
        with pytest.raises(NotImplementedError):
            x.apply(opobj, right=1)
        with pytest.raises(NotImplementedError):
            x.apply(opobj, left=1)


MIXED = [("INT8", "UINT8", "INT16"), ("INT64", "UINT64", "FP64"), ("INT32", "FP32", "FP64"),
         ("BOOL", "INT8", "INT8"), ("UINT16", "FP32", "FP32"), ("FP64", "INT64", "FP64")]


@pytest.mark.parametrize("op", ["plus", "div", "min", "pow", "eq", "lor", "first", "second", "bxor"])
def test_ewise_mixed_dtypes(gb, op):
    """operands of different dtypes: the front end picks op[unified type], both sides are cast to it"""
    opobj = getattr(gb.binary, op)
    for da, db, dz in MIXED:
        if dz not in [t.name for t in opobj.types]:
            continue
        for shape in [(65,), (37, 53)]:
            rng = _rng("mixed", op, da, db, shape)
            n = int(np.prod(shape))
            pa, pb = rng.random(shape) < 0.7, rng.random(shape) < 0.7
            if op == "pow":  # keep the float64 pow exact (see binary_inputs)
                va = rng.integers(0, 10, n).astype(dm.NP[da]).reshape(shape)
                vb = rng.integers(0, 13, n).astype(dm.NP[db]).reshape(shape)
            else:
                va, vb = draw(da, rng, n).reshape(shape), draw(db, rng, n).reshape(shape)
            if op == "min":
                va, vb = np.where(va == 0, dm.NP[da](1), va), np.where(vb == 0, dm.NP[db](1), vb)
            A, B = (pa, np.where(pa, va, dm.NP[da](0))), (pb, np.where(pb, vb, dm.NP[db](0)))
            a, b = to_gb(gb, A), to_gb(gb, B)
            for kind in ("mult", "add"):
                expr = getattr(a, f"ewise_{kind}")(b, opobj)
                assert expr.op.type.name == dz, (op, da, db)
                zt = dm.binop_return_dtype(op, dz)
                what = f"ewise_{kind} {op} {da} x {db} {shape}"
                if op == "pow" and dm.is_float(dz):
                    d = check(expr.new(), dm.ewise(kind, op, dz, A, B), zt, ulps=True, what=what)
                    print(f"\nULP pow {dz} {d} {what}")
                    assert d <= ULP_BOUND.get(("pow", dz), 0), f"{what}: {d} ulps"
                else:
                    check(expr.new(), dm.ewise(kind, op, dz, A, B), zt, what=what)


@pytest.mark.parametrize("dt", ["INT32", "FP64", "BOOL", "UINT8"])
def test_ewise_iso_operands(gb, dt):
    ops = ["plus", "times", "max", "eq", "lor", "minus", "second"]
    for shape in [(65,), (37, 53), (3, 300)]:
        rng = _rng("iso", dt, shape)
        pa, pb = rng.random(shape) < 0.6, rng.random(shape) < 0.6
        sa, sb = (True, True) if dt == "BOOL" else (3, 2)
        a_iso, A_iso = iso_gb(gb, pa, sa, dt)
        b_iso, B_iso = iso_gb(gb, pb, sb, dt)
        B = (pb, np.where(pb, draw(dt, rng, pb.size).reshape(shape), dm.NP[dt](0)))
        if dt == "FP64":
            B = (pb, np.where(pb & ~np.isnan(B[1]) & (B[1] != 0), B[1], 1.0 * pb))
        b = to_gb(gb, B)
        for op in ops:
            for kind in ("mult", "add"):
                zt = dm.binop_return_dtype(op, dt)
                for (x, X), (y, Y), tag in (((a_iso, A_iso), (b, B), "iso,full"), ((b, B), (a_iso, A_iso), "full,iso"),
                                            ((a_iso, A_iso), (b_iso, B_iso), "iso,iso")):
                    got = getattr(x, f"ewise_{kind}")(y, getattr(gb.binary, op)).new()
                    check(got, dm.ewise(kind, op, dt, X, Y), zt, zero_sign=op != "max",
                          what=f"ewise_{kind} {op}[{dt}] {shape} {tag}")


@pytest.mark.parametrize("dt", ["INT16", "FP32"])
def test_ewise_transposed_operands(gb, dt):
    A, B = binary_inputs("minus", dt, (37, 53), "T")
    At, Bt = dm.transpose(A), dm.transpose(B)  # 53 x 37 objects whose .T are A and B
    a, b, at, bt = to_gb(gb, A), to_gb(gb, B), to_gb(gb, At), to_gb(gb, Bt)
    for op in ("minus", "div", "gt", "first"):
        opobj = getattr(gb.binary, op)
        zt = dm.binop_return_dtype(op, dt)
        for kind in ("mult", "add"):
            want = dm.ewise(kind, op, dt, A, B)
            for x, y, tag in ((at.T, b, "A.T,B"), (a, bt.T, "A,B.T"), (at.T, bt.T, "A.T,B.T")):
                got = getattr(x, f"ewise_{kind}")(y, opobj).new()
                check(got, want, zt, what=f"ewise_{kind} {op}[{dt}] {tag}")
    # an iso operand behind a transpose
    p = A[0]
    c_iso, C_iso = iso_gb(gb, np.ascontiguousarray(p.T), 3, dt)
    got = c_iso.T.ewise_add(b, gb.binary.minus).new()
    check(got, dm.ewise("add", "minus", dt, dm.transpose(C_iso), B), dt, what="iso.T")


# ---------------------------------------------------------------------- big shapes
def ragged(nrows, ncols, dt, key, maxrow=3):
    """0..maxrow entries per row, random distinct columns, random values"""
    rng = _rng("ragged", nrows, ncols, dt, key)
    cnt = rng.integers(0, maxrow + 1, nrows)
    rows = np.repeat(np.arange(nrows), cnt)
    k = np.arange(rows.size) - np.repeat(np.cumsum(cnt) - cnt, cnt)  # position within the row
    cols = (np.repeat(rng.integers(0, ncols, nrows), cnt) + 17 * k) % ncols  # 0, 17, 34: distinct mod 64
    p = np.zeros((nrows, ncols), bool)
    p[rows, cols] = True
    v = np.zeros((nrows, ncols), dm.NP[dt])
    v[rows, cols] = draw(dt, rng, rows.size)
    return p, v


def heavy(dt, key, nrows=301, ncols=6007, hub=7, hub_entries=5200):
    """a third of the rows empty, one row of hub_entries entries, the rest about 1% full"""
    rng = _rng("heavy", dt, key)
    p = rng.random((nrows, ncols)) < 0.01
    p[np.arange(nrows) % 3 == 1] = False
    p[hub] = False
    p[hub, rng.permutation(ncols)[:hub_entries]] = True
    v = np.where(p, draw(dt, rng, p.size).reshape(p.shape), dm.NP[dt](0))
    return p, v


@pytest.mark.parametrize("n", [70001, 262245])
@pytest.mark.parametrize("dt", ["INT32", "FP64"])
def test_ewise_apply_big_vectors(gb, n, dt):
    A, B = binary_inputs("plus", dt, (n,), "big")
    a, b = to_gb(gb, A), to_gb(gb, B)
    for op in ("plus", "lt"):
        zt = dm.binop_return_dtype(op, dt)
        for kind in ("mult", "add"):
            got = getattr(a, f"ewise_{kind}")(b, getattr(gb.binary, op)).new()
            check(got, dm.ewise(kind, op, dt, A, B), zt, what=f"ewise_{kind} {op}[{dt}] {n}")
    check(a.apply(gb.unary.ainv).new(), dm.apply("ainv", dt, A), dt, what=f"apply ainv {n}")
    three = dm.NP[dt](3)  # a scalar of the operand's type keeps the operator in that type
    check(a.apply(gb.binary.minus, right=three).new(), dm.apply("minus", dt, A, right=three), dt,
          what=f"apply minus right {n}")


@pytest.mark.parametrize("shape,scan_u8", [((133125, 64), 0), ((133125, 64), 1), ((131071, 64), 0),
                                           ((301, 6007), 0)])
def test_ewise_apply_transpose_big_matrices(gb, shape, scan_u8):
    dt = "INT32"
    A = heavy(dt, "a") if shape[0] == 301 else ragged(*shape, dt, "a")
    B = heavy(dt, "b", hub=7) if shape[0] == 301 else ragged(*shape, dt, "b")
    with _knobs(gb, scan_u8=scan_u8):
        a, b = to_gb(gb, A), to_gb(gb, B)  # the build: its scans run over the tuples and the rows
        check(a, A, dt, what=f"build {shape}")
        for kind in ("mult", "add"):
            got = getattr(a, f"ewise_{kind}")(b, gb.binary.plus).new()
            check(got, dm.ewise(kind, "plus", dt, A, B), dt, what=f"ewise_{kind} {shape} scan_u8={scan_u8}")
        check(a.apply(gb.unary.abs).new(), dm.apply("abs", dt, A), dt, what=f"apply {shape}")
        at = a.T.new()
        check(at, dm.transpose(A), dt, what=f"A.T.new() {shape}")
        check(at.T.new(), A, dt, what=f"transpose back {shape}")  # 64 x n -> n rows: scan over n
        c = gb.Matrix(dt, shape[1], shape[0])
        c << a.T
        check(c, dm.transpose(A), dt, what=f"C << A.T {shape}")
        got = at.T.ewise_mult(b, gb.binary.times).new()
        check(got, dm.ewise("mult", "times", dt, A, B), dt, what=f"(A.T).T * B {shape}")


# ---------------------------------------------------------------------- apply
@pytest.mark.parametrize("op", UNARY)
def test_apply_every_unary_op(gb, op):
    opobj = getattr(gb.unary, op)
    measured = []
    for dtobj in opobj.types:  # includes the integer / bool inputs the float-only operators accept
        dt = dtobj.name
        name, ct, zt = typed_info(opobj[dt])
        assert name == op
        exact = op not in dm.TRANSCENDENTAL
        worst = 0
        for shape in SMALL_VEC + SMALL_MAT:
            A = unary_input(op, dt, shape, "apply")
            got = to_gb(gb, A).apply(opobj).new()
            want = dm.apply(op, ct, A)
            what = f"apply {op}[{dt}] {shape}"
            if exact:
                check(got, want, zt, what=what)
            else:
                worst = max(worst, check(got, want, zt, ulps=True, what=what))
        if not exact:
            measured.append((op, ct, "apply" if ct == dt else f"apply, input {dt}", worst))
    ulp_report(measured)


def test_apply_unary_iso_and_transposed(gb):
    p = _rng("apply-iso").random((37, 53)) < 0.5
    a_iso, A_iso = iso_gb(gb, p, -3, "INT8")
    check(a_iso.apply(gb.unary.ainv).new(), dm.apply("ainv", "INT8", A_iso), "INT8", what="iso ainv")
    check(a_iso.T.apply(gb.unary.abs).new(), dm.apply("abs", "INT8", dm.transpose(A_iso)), "INT8", what="iso.T abs")
    A = unary_input("round", "FP64", (37, 53), "T")
    check(to_gb(gb, A).T.apply(gb.unary.round).new(), dm.apply("round", "FP64", dm.transpose(A)), "FP64",
          what="A.T round")
    v_iso, V_iso = iso_gb(gb, p[0], 2.5, "FP32")
    check(v_iso.apply(gb.unary.round).new(), dm.apply("round", "FP32", V_iso), "FP32", what="iso round")
    check(v_iso.apply(gb.binary.minus, left=np.float32(1)).new(),
          dm.apply("minus", "FP32", V_iso, left=np.float32(1)), "FP32", what="iso minus left")


@pytest.mark.parametrize("op", BINARY)
def test_apply_every_binary_op_with_a_bound_scalar(gb, op):
    opobj = getattr(gb.binary, op)
    exact = op not in dm.TRANSCENDENTAL
    measured = []
    for dtobj in opobj.types:
        dt = dtobj.name
        t = dm.NP[dt]
        zt = dm.binop_return_dtype(op, dt)
        sp = specials(dt)
        rng = _rng("bound", op, dt)
        scalars = list(sp[rng.permutation(sp.size)[:4]]) + [draw(dt, rng, 1)[0]]
        if op == "pow" and dm.is_int(dt):
            scalars = [t(0), t(2), t(3), t(9)]
        if op == "ldexp":
            scalars = [t(-20), t(0), t(7)]
        worst = 0
        for shape in [(65,), (37, 53)]:
            A, B = binary_inputs(op, dt, shape, "bound")
            a, b = to_gb(gb, A), to_gb(gb, B)
            for s in scalars:
                if op in ("min", "max") and dm.is_float(dt) and s == 0:
                    continue  # -0.0 against +0.0
                for side in ("right", "left"):
                    if op == "ldexp" and side == "left":
                        continue  # the operand would be the exponent: out of the -20..20 domain
                    X, x = (A, a) if side == "right" else (B, b)  # B holds the second-argument domain
                    got = x.apply(opobj, **{side: s}).new()
                    want = dm.apply(op, dt, X, **{side: s})
                    what = f"apply {op}[{dt}] {side}={s!r} {shape}"
                    if exact or not dm.is_float(dt):
                        check(got, want, zt, zero_sign=op not in ("min", "max"), what=what)
                    else:
                        worst = max(worst, check(got, want, zt, ulps=True, what=what))
        if not exact and dm.is_float(dt):
            measured.append((op, dt, "bound scalar", worst))
    ulp_report(measured)


@pytest.mark.parametrize("op", ["plus", "minus", "div", "max", "lt", "lor", "second", "first"])
def test_apply_scalar_of_another_dtype(gb, op):
    """the operator's type comes from operand and scalar together; both are cast to it"""
    opobj = getattr(gb.binary, op)
    cases = [("FP32", np.int64(3)), ("INT16", np.float32(2.5)), ("UINT8", np.int8(-3)), ("INT64", np.float64(-0.75)),
             ("BOOL", np.int32(7)), ("FP64", np.uint64(2**63 + 2048)), ("INT8", np.int64(1000))]
    for dt, s in cases:
        for shape in [(65,), (37, 53)]:
            A = unary_input("identity", dt, shape, ("other", op))
            a = to_gb(gb, A)
            for side in ("right", "left"):
                expr = a.apply(opobj, **{side: s})
                ct = expr.op.type.name
                zt = dm.binop_return_dtype(op, ct)
                want = dm.apply(op, ct, A, **{side: s})
                check(expr.new(), want, zt, zero_sign=op != "max",
                      what=f"apply {op} {dt} {side}={s!r} ({s.dtype}) -> {ct} {shape}")
    # a Scalar object of another dtype
    A = unary_input("identity", "INT32", (65,), "scalar-object")
    s = gb.Scalar.from_value(2.5, "FP32")
    expr = to_gb(gb, A).apply(gb.binary.times, right=s)
    ct = expr.op.type.name
    check(expr.new(), dm.apply("times", ct, A, right=np.float32(2.5)), ct, what="Scalar FP32")


# ---------------------------------------------------------------------- reduce
def reduce_input(mon, dt, shape, key, density=0.6):
    """values for a reduction by `mon`: anything where the monoid is exact; normals for float
    plus, [0.5, 2] for float times (nothing overflows)"""
    rng = _rng("reduce", mon, dt, shape, key)
    total = int(np.prod(shape))
    if dm.is_float(dt) and mon == "plus":
        x = (rng.standard_normal(total) * 100).astype(dm.NP[dt])
    elif dm.is_float(dt) and mon == "times":
        x = np.exp(rng.uniform(-math.log(2), math.log(2), total)).astype(dm.NP[dt])
    else:
        x = draw(dt, rng, total)
        if dm.is_float(dt):  # min / max: keep one sign of zero
            x = np.where(x == 0, dm.NP[dt](0), x)
    p = rng.random(total) < density
    if total <= 64:
        p[:] = True
    return p.reshape(shape), np.where(p, x, dm.NP[dt](0)).reshape(shape)


def check_reduced(got, vals, name, ct, what, verbose=False):
    """one reduced value against the fold of `vals` (already of type ct)"""
    t = dm.NP[ct]
    got = np.asarray(got, t)[()]
    if name == "any":
        assert np.isin(got, vals) or (got != got and np.isnan(vals).any()), f"{what}: {got!r} is no input"
        return
    if dm.is_float(ct) and name in ("plus", "times"):
        eps = 2.0 ** -53 if ct == "FP64" else 2.0 ** -24
        v64 = vals.astype(np.float64)
        if name == "plus":
            ref, bound = math.fsum(v64), vals.size * eps * float(np.abs(v64).sum())
        else:
            ref = float(np.multiply.reduce(v64))
            bound = vals.size * eps * abs(ref)
        err = abs(float(got) - ref)
        if verbose:
            print(f"REDUCE {what}: n={vals.size} err={err:.3e} bound={bound:.3e}")
        assert err <= bound, f"{what}: |{got!r} - {ref!r}| = {err} > {bound}"
        return
    want = dm.monoid_fold(name, ct, vals)
    assert np.array_equal(got, want, equal_nan=dm.is_float(ct)), f"{what}: got {got!r}, expected {want!r}"


def scalar_value(s, zt):
    assert s.dtype == zt
    return s.value


@pytest.mark.parametrize("mon", MONOIDS)
def test_reduce_scalar_every_monoid(gb, mon):
    monobj = getattr(gb.monoid, mon)
    for dtobj in monobj.types:
        dt = dtobj.name
        name, ct, zt = typed_info(monobj[dt])
        assert zt == ct
        for shape in SMALL_VEC + [(1, 1), (37, 53), (3, 300)]:
            A = reduce_input(name, dt, shape, "scalar")
            a = to_gb(gb, A)
            red = a.reduce if len(shape) == 1 else a.reduce_scalar
            vals = dm.cast(A[1][A[0]], ct)
            what = f"reduce {mon}[{dt}] {shape}"
            for allow_empty in (True, False):
                check_reduced(scalar_value(red(monobj, allow_empty=allow_empty).new(), zt), vals, name, ct, what)
            if len(shape) == 2 and shape[0] > 1:
                got = scalar_value(a.T.reduce_scalar(monobj).new(), zt)
                check_reduced(got, vals, name, ct, what + " .T")
        # iso inputs: n copies of one value
        p = _rng("reduce-iso", mon, dt).random((37, 53)) < 0.5
        sval = True if dt == "BOOL" else 3
        for pp in (p[0], p):
            x_iso, X_iso = iso_gb(gb, pp, sval, dt)
            red = x_iso.reduce if pp.ndim == 1 else x_iso.reduce_scalar
            vals = dm.cast(X_iso[1][pp], ct)
            if not (dm.is_float(ct) and name in ("plus", "times")):
                check_reduced(scalar_value(red(monobj).new(), zt), vals, name, ct, f"reduce {mon}[{dt}] iso")
        # empty inputs: no value, or the monoid's identity
        for empty in (gb.Vector(dt, 65), gb.Matrix(dt, 37, 53)):
            red = empty.reduce if empty.ndim == 1 else empty.reduce_scalar
            s = red(monobj, allow_empty=True).new()
            assert s.dtype == zt and s.is_empty and s.value is None, f"{mon}[{dt}] empty"
            s = red(monobj, allow_empty=False).new()
            ident = dm.monoid_identity(name, ct)
            assert s.dtype == zt and not s.is_empty, f"{mon}[{dt}] identity"
            assert np.asarray(s.value, dm.NP[ct])[()] == ident, f"{mon}[{dt}]: identity {s.value!r}, expected {ident!r}"


BIG_REDUCE = [("plus", "INT64"), ("plus", "FP64"), ("plus", "FP32"), ("times", "FP64"), ("times", "UINT32"),
              ("min", "INT32"), ("max", "FP32"), ("lor", "BOOL"), ("land", "BOOL"), ("lxor", "BOOL"),
              ("lxnor", "BOOL"), ("any", "INT16"), ("bor", "UINT64"), ("band", "UINT8"), ("bxor", "UINT16"),
              ("bxnor", "UINT32")]


@pytest.mark.parametrize("n", [70001, 262245])
def test_reduce_scalar_big(gb, n):
    """the stride loop and the second level of k_reduce_partial, on vectors and matrices"""
    for mon, dt in BIG_REDUCE:
        monobj = getattr(gb.monoid, mon)
        name, ct, zt = typed_info(monobj[dt])
        density = 0.97 if mon in ("land", "band") else 0.5
        A = reduce_input(name, dt, (n,), "big", density)
        if mon == "land":
            A = (A[0], A[0].copy())  # all true: a single false lane must not be what decides
        vals = dm.cast(A[1][A[0]], ct)
        check_reduced(scalar_value(to_gb(gb, A).reduce(monobj).new(), zt), vals, name, ct, f"reduce {mon}[{dt}] {n}",
                      verbose=True)
        if mon == "land":
            B = (A[0], A[1].copy())
            B[1][np.flatnonzero(A[0])[-3]] = False  # one false near the end
            check_reduced(scalar_value(to_gb(gb, B).reduce(monobj).new(), zt), B[1][B[0]], name, ct,
                          f"reduce land one false {n}")
    # a matrix with that many entries (values reduce in storage order)
    rows = n // 64 + 1
    M = reduce_input("plus", "INT64", (rows, 64), "bigmat", 0.99)
    for mon in ("plus", "min", "bxor"):
        dt = "INT64" if mon != "bxor" else "UINT64"
        Md = (M[0], dm.cast(M[1], dt))
        got = scalar_value(to_gb(gb, Md).reduce_scalar(getattr(gb.monoid, mon)).new(), dt)
        check_reduced(got, Md[1][Md[0]], mon, dt, f"reduce_scalar {mon} {rows}x64")


ROW_REDUCE = {"min": ["INT32", "FP64"], "max": ["INT32", "FP64"], "plus": ["INT32", "FP64"],
              "times": ["INT32", "FP64"], "lor": ["BOOL"], "land": ["BOOL"], "lxor": ["BOOL"], "lxnor": ["BOOL"],
              "eq": ["BOOL"], "any": ["INT32"], "bor": ["UINT16"], "band": ["UINT16"], "bxor": ["UINT16"],
              "bxnor": ["UINT16"]}


def check_reduced_vector(got, A, name, ct, what):
    """a row reduction of model matrix A (values already of type ct) against per-row folds"""
    p, v = A
    assert got.dtype == ct and got.size == p.shape[0], what
    idx, vals = got.to_coo()
    idx = idx.astype(np.int64)
    want = np.flatnonzero(p.any(axis=1))
    assert got.nvals == want.size and np.array_equal(idx, want), f"{what}: structure"
    assert vals.dtype == dm.NP[ct]
    for i, g in zip(idx, vals):
        check_reduced(g, v[i][p[i]], name, ct, f"{what} row {i}")


@pytest.mark.parametrize("mon", MONOIDS)
@pytest.mark.parametrize("shape", [(301, 6007), (3, 300)])
def test_reduce_rowwise_columnwise(gb, mon, shape):
    monobj = getattr(gb.monoid, mon)
    for dt in ROW_REDUCE[mon]:
        name, ct, zt = typed_info(monobj[dt])
        if shape[0] == 301:
            p = heavy("BOOL", (mon, dt))[0]
        else:
            p = _rng("rows", mon, dt).random(shape) < 0.5
        A = (p, np.where(p, reduce_input(name, dt, shape, "rows", 1.0)[1], dm.NP[dt](0)))
        At = dm.transpose(A)
        a = to_gb(gb, A)
        Ac, Atc = (A[0], dm.cast(A[1], ct)), (At[0], dm.cast(At[1], ct))
        what = f"{mon}[{dt}] {shape}"
        check_reduced_vector(a.reduce_rowwise(monobj).new(), Ac, name, ct, "reduce_rowwise " + what)
        check_reduced_vector(a.reduce_columnwise(monobj).new(), Atc, name, ct, "reduce_columnwise " + what)
        check_reduced_vector(a.T.reduce_rowwise(monobj).new(), Atc, name, ct, "A.T.reduce_rowwise " + what)
        check_reduced_vector(a.T.reduce_columnwise(monobj).new(), Ac, name, ct, "A.T.reduce_columnwise " + what)
        if name == "any" or (dm.is_float(ct) and name in ("plus", "times")):
            continue  # no single expected value to accumulate into
        # mask + accum into a non-empty w
        rng = _rng("rows-w", mon, dt, shape)
        for X, expr, tag in ((Ac, a.reduce_rowwise(monobj), "rowwise"), (Atc, a.reduce_columnwise(monobj), "columnwise")):
            n = X[0].shape[0]
            W = (rng.random(n) < 0.5, None)
            W = (W[0], np.where(W[0], draw(ct, rng, n), dm.NP[ct](0)))
            if dm.is_float(ct):
                W = (W[0], np.where(np.isfinite(W[1]), W[1], dm.NP[ct](1)) * W[0])
            M = (rng.random(n) < 0.5, np.ones(n, bool))
            T = dm.reduce_rows(name, ct, X)
            acc = "max" if dm.is_float(ct) else "plus"
            w = to_gb(gb, W)
            w(to_gb(gb, M).S, getattr(gb.binary, acc)) << expr
            check(w, dm.write_back(W, T, mask=M, mask_struct=True, accum=acc), ct, zero_sign=False,
                  what=f"w(M.S, {acc}) << reduce_{tag} {what}")


# ---------------------------------------------------------------------- transpose
@pytest.mark.parametrize("shape", SMALL_MAT + [(301, 6007)])
@pytest.mark.parametrize("dt", ["INT8", "FP64", "BOOL"])
def test_transpose(gb, shape, dt):
    if shape[0] == 301:
        A = heavy(dt, "transpose")
    else:
        A = unary_input("identity", dt, shape, "transpose")
    At = dm.transpose(A)
    a = to_gb(gb, A)
    sval = True if dt == "BOOL" else -7
    a_iso, A_iso = iso_gb(gb, A[0], sval, dt)
    for x, X, tag in ((a, A, "full"), (a_iso, A_iso, "iso")):
        Xt = dm.transpose(X)
        check(x.T.new(), Xt, dt, what=f"A.T.new() {shape} {tag}")
        c = gb.Matrix(dt, shape[1], shape[0])
        c << x.T
        check(c, Xt, dt, what=f"C << A.T {shape} {tag}")
        assert x.T.T is x
        check(x.T.new().T.new(), X, dt, what=f"transpose of the transpose {shape} {tag}")
        check(x.T.new(dtype="FP32"), (Xt[0], dm.cast(Xt[1], "FP32")), "FP32", what=f"A.T.new(FP32) {shape} {tag}")
    # into a non-empty C: structural mask, complemented mask with replace, accum
    rng = _rng("transpose-into", shape, dt)
    tshape = (shape[1], shape[0])
    n = int(np.prod(tshape))
    cp, mp = rng.random(tshape) < 0.5, rng.random(tshape) < 0.5
    C = (cp, np.where(cp, draw(dt, rng, n).reshape(tshape), dm.NP[dt](0)))
    M = (mp, rng.random(tshape) < 0.5)
    m = to_gb(gb, M)
    for kw, mk in ((dict(mask_struct=True), lambda: dict(mask=m.S)),
                   (dict(mask_struct=True, mask_comp=True, replace=True), lambda: dict(mask=~m.S, replace=True)),
                   (dict(mask_comp=True, replace=True), lambda: dict(mask=~m.V, replace=True)),
                   (dict(accum="plus"), lambda: dict(accum=gb.binary.plus)),
                   (dict(mask_struct=True, accum="minus"), lambda: dict(mask=m.S, accum=gb.binary.minus))):
        c = to_gb(gb, C)
        c(**mk()) << a.T
        want = dm.write_back(C, At, mask=M if ("mask_struct" in kw or "mask_comp" in kw) else None, **kw)
        check(c, want, dt, what=f"C({kw}) << A.T {shape}")


# ---------------------------------------------------------------------- build
DUP_OPS = ["plus", "times", "min", "max", "first", "second", "any", "lor", "land", "lxor", "bor", "band", "bxor",
           "minus"]
_build_tuples = {}


def build_tuples():
    """200000 tuples over 300 x 300, unsorted, heavy duplication, one key 5000 times (shared)"""
    if not _build_tuples:
        rng = _rng("build")
        n = 200000
        r, c = rng.integers(0, 300, n), rng.integers(0, 300, n)
        hot = rng.permutation(n)[:5000]
        r[hot], c[hot] = 123, 45
        _build_tuples.update(r=r, c=c)
    return _build_tuples["r"], _build_tuples["c"]


@pytest.mark.parametrize("dt", ["INT8", "UINT64", "FP64", "BOOL"])
def test_build_with_dup_op(gb, dt):
    r, c = build_tuples()
    rng = _rng("build-values", dt)
    if dt == "FP64":  # small integers: every fold is exact, so the order shows only where it should
        vals = rng.integers(-3, 4, r.size).astype(np.float64)
    else:
        vals = draw(dt, rng, r.size)
    for op in DUP_OPS:
        if op in ("bor", "band", "bxor") and not dm.is_int(dt):
            continue
        v = vals
        if op == "times" and dt == "FP64":
            v = np.where(rng.random(r.size) < 0.5, 1.0, rng.choice([-1.0, 2.0, 0.5], r.size))
        opobj = getattr(gb.binary, op)
        got = gb.Matrix.from_coo(r, c, v, dtype=dt, nrows=300, ncols=300, dup_op=opobj)
        check(got, dm.build((300, 300), (r, c), v, op, dt), dt, what=f"Matrix.from_coo dup_op={op}[{dt}]")
        flat = (r * 300 + c) % 7001  # a vector with even more duplicates
        got = gb.Vector.from_coo(flat, v, dtype=dt, size=7001, dup_op=opobj)
        check(got, dm.build((7001,), (flat,), v, op, dt), dt, what=f"Vector.from_coo dup_op={op}[{dt}]")


def test_build_casts_before_the_fold(gb):
    """values of another type than the target.  from_coo converts on the host (numpy), so only
    conversions numpy and GraphBLAS agree on go through it; GrB_*_build_FP64 into an INT8 / UINT8 /
    BOOL object is called directly for the device's saturating cast."""
    from graphblas_amd.base import call
    from graphblas_amd.matrix import _CArray

    r, c = build_tuples()
    rng = _rng("build-cast")
    ivals = rng.integers(-1000, 1000, r.size)
    got = gb.Vector.from_coo(r, ivals, dtype="UINT8", size=300, dup_op=gb.binary.plus)
    check(got, dm.build((300,), (r,), ivals, "plus", "UINT8"), "UINT8", what="build INT64 -> UINT8 plus")
    fvals = rng.uniform(-100, 100, r.size)
    for dt, op in (("INT8", "plus"), ("BOOL", "lxor"), ("FP32", "min"), ("INT64", "second")):
        got = gb.Matrix.from_coo(r, c, fvals, dtype=dt, nrows=300, ncols=300, dup_op=getattr(gb.binary, op))
        check(got, dm.build((300, 300), (r, c), fvals, op, dt), dt, what=f"from_coo FP64 -> {dt} {op}")
    vals = rng.uniform(-300, 300, r.size)  # FP64 into INT8: saturate first, then wrap in the sum
    vals[rng.random(r.size) < 0.01] = np.nan
    ru, cu = np.ascontiguousarray(r, np.uint64), np.ascontiguousarray(c, np.uint64)
    for dt, op in (("INT8", "plus"), ("UINT8", "max"), ("UINT8", "plus"), ("BOOL", "lxor"), ("INT16", "minus")):
        m = gb.Matrix(dt, 300, 300)
        call("GrB_Matrix_build_FP64", [m, _CArray(ru), _CArray(cu), _CArray(vals), r.size, getattr(gb.binary, op)[dt]])
        check(m, dm.build((300, 300), (r, c), vals, op, dt), dt, what=f"GrB_Matrix_build_FP64 -> {dt} {op}")
        v = gb.Vector(dt, 300)
        call("GrB_Vector_build_FP64", [v, _CArray(ru), _CArray(vals), r.size, getattr(gb.binary, op)[dt]])
        check(v, dm.build((300,), (r,), vals, op, dt), dt, what=f"GrB_Vector_build_FP64 -> {dt} {op}")


def test_build_scalar_value(gb):
    r, c = build_tuples()
    # an iso build ignores duplicates: every entry is the scalar
    got = gb.Matrix.from_coo(r, c, 3, dtype="INT32", nrows=300, ncols=300)
    want = dm.build((300, 300), (r, c), np.full(r.size, 3), "first", "INT32")
    check(got, want, "INT32", what="from_coo scalar")
    got = gb.Vector.from_coo(r, 2.5, dtype="FP32", size=300)
    check(got, dm.build((300,), (r,), np.full(r.size, 2.5), "second", "FP32"), "FP32", what="Vector.from_coo scalar")
    # as in the reference, from_coo refuses a dup_op next to a scalar (it would be ignored) ...
    with pytest.raises(ValueError, match="dup_op must be None"):
        gb.Matrix.from_coo(r, c, 3, nrows=300, ncols=300, dup_op=gb.binary.plus)
    with pytest.raises(ValueError, match="dup_op must be None"):
        gb.Vector.from_coo(r, 3, size=300, dup_op=gb.binary.plus)
    # ... and build() folds the broadcast scalar: under plus the result is no longer one value
    for op in ("plus", "min", "first", "times", "lxor", "minus"):
        m = gb.Matrix("INT32", 300, 300)
        m.build(r, c, 3, dup_op=getattr(gb.binary, op))
        want = dm.build((300, 300), (r, c), np.full(r.size, 3), op, "INT32")
        check(m, want, "INT32", what=f"build scalar dup_op={op}")
        if op == "plus":
            assert np.unique(m.to_coo()[2]).size > 1 and m[123, 45].value >= 5000 * 3
        v = gb.Vector("INT32", 300)
        v.build(r, 3, dup_op=getattr(gb.binary, op))
        check(v, dm.build((300,), (r,), np.full(r.size, 3), op, "INT32"), "INT32", what=f"Vector.build scalar {op}")


@pytest.mark.parametrize("scan_u8", [0, 1])
def test_build_many_rows(gb, scan_u8):
    """140000 distinct rows, 300000 tuples: the scans over the tuples and over the rows take the
    wave-tile path (scan_u8 = 1: the same through hipCUB)"""
    rng = _rng("build-rows")
    nrows, n = 140000, 300000
    r = np.r_[rng.permutation(nrows), rng.integers(0, nrows, n - nrows)]
    c = rng.integers(0, 5, n)
    vals = rng.integers(-100, 100, n)
    order = rng.permutation(n)
    r, c, vals = r[order], c[order], vals[order]
    with _knobs(gb, scan_u8=scan_u8):
        got = gb.Matrix.from_coo(r, c, vals, dtype="INT64", nrows=nrows, ncols=5, dup_op=gb.binary.minus)
        check(got, dm.build((nrows, 5), (r, c), vals, "minus", "INT64"), "INT64", what="build 140000 rows")
        got = gb.Vector.from_coo(r, vals, dtype="INT32", size=nrows, dup_op=gb.binary.plus)
        check(got, dm.build((nrows,), (r,), vals, "plus", "INT32"), "INT32", what="build 140000-vector")


# ---------------------------------------------------------------------- write-back, typed accumulator
def accum_case(ctype, shape, key):
    """C, T (FP64), a mask: about a third of C's entries have no T entry, a third of the
    positions lie outside the mask"""
    rng = _rng("accum", ctype, shape, key)
    n = int(np.prod(shape))
    cp, tp, mp = rng.random(n) < 0.7, rng.random(n) < 0.6, rng.random(n) < 0.6
    if ctype == "INT64":
        pool = np.array([2**53 + 1, -(2**62) - 3, 2**63 - 1, -(2**63), 2**53 + 3, 1, -7, 0, 12345], np.int64)
        cv = pool[rng.integers(0, pool.size, n)]
        tv = np.where(rng.random(n) < 0.5, rng.integers(-50, 50, n) + 0.5, rng.standard_normal(n) * 1e17)
    elif ctype == "FP64":  # values FP32 cannot hold
        cv = rng.standard_normal(n) * 1e3 + rng.standard_normal(n) * 1e-9
        tv = rng.standard_normal(n) * 1e3 + rng.standard_normal(n) * 1e-9
        tv[rng.random(n) < 0.05] = 1e300  # infinite in FP32
    else:  # UINT8 with max evaluated in INT64
        cv = rng.integers(0, 256, n).astype(np.uint8)
        tv = rng.choice([300.0, -4.0, 1e9, 17.5, 200.25, np.nan, -1e30, 255.0, 256.0], n)
    cv, tv = np.asarray(cv, dm.NP[ctype]), np.asarray(tv, np.float64)
    C = (cp.reshape(shape), np.where(cp, cv, dm.NP[ctype](0)).reshape(shape))
    T = (tp.reshape(shape), np.where(tp, tv, 0.0).reshape(shape))
    M = (mp.reshape(shape), rng.random(n).reshape(shape) < 0.5)
    return C, T, M


@pytest.mark.parametrize("shape", [(200,), (37, 53)])
@pytest.mark.parametrize("ctype,accum,adt", [("INT64", "plus", None), ("INT64", "plus", "FP64"),
                                             ("FP64", "plus", "FP32"), ("UINT8", "max", "INT64")])
def test_write_back_typed_accumulator(gb, shape, ctype, accum, adt):
    """Z = accum(C, T) has C's type: entries of C that T does not touch come back bit-identical
    (outside the mask, and under accum with no T entry); entries only in T are cast to C's type;
    entries in both are the accumulator's result, computed in its type, cast to C's type."""
    C, T, M = accum_case(ctype, shape, (accum, adt))
    u, m = to_gb(gb, T), to_gb(gb, M)
    op = getattr(gb.binary, accum)
    op = op if adt is None else op[adt]
    variants = [("unmasked", {}, {}),
                ("M.S", dict(mask=M, mask_struct=True), dict(mask=m.S)),
                ("~M.S, replace", dict(mask=M, mask_struct=True, mask_comp=True, replace=True),
                 dict(mask=~m.S, replace=True)),
                ("M.V", dict(mask=M), dict(mask=m.V))]
    for tag, mkw, gkw in variants:
        c = to_gb(gb, C)
        c(accum=op, **gkw) << u.apply(gb.unary.identity)
        want = dm.write_back(C, T, accum=accum, accum_dtype=adt, **mkw)
        what = f"C[{ctype}]({tag}, accum={accum}[{adt or ctype}]) << FP64 {shape}"
        check(c, want, ctype, what=what)
        # said again without the model: what T does not touch keeps its bits
        mask = np.ones(shape, bool)
        if mkw:
            mask = M[0] if mkw.get("mask_struct") else M[0] & M[1]
            mask = ~mask if mkw.get("mask_comp") else mask
        untouched = C[0] & ~(mask & T[0]) & (mask | (not mkw.get("replace", False)))
        gi, gv = coo_of(c)
        dense = np.zeros(shape, dm.NP[ctype])
        dense[gi] = gv
        assert untouched.any() and np.array_equal(dense[untouched].view(np.uint8), C[1][untouched].view(np.uint8)), what
        if ctype == "INT64" and adt == "FP64":
            both = C[0] & T[0] & mask
            ref = dm.cast(C[1][both].astype(np.float64) + T[1][both], "INT64")
            assert both.any() and np.array_equal(dense[both], ref), what


def test_write_back_typed_accumulator_other_producers(gb):
    """the same rule behind eWise, transpose and assign (every operation shares the write-back)"""
    C, T, M = accum_case("INT64", (37, 53), "producers")
    m = to_gb(gb, M)
    acc = gb.binary.plus["FP64"]
    want = dm.write_back(C, T, mask=M, mask_struct=True, accum="plus", accum_dtype="FP64")
    c = to_gb(gb, C)
    c(m.S, acc) << to_gb(gb, dm.transpose(T)).T
    check(c, want, "INT64", what="C(M.S, plus[FP64]) << U.T")
    c = to_gb(gb, C)
    z = gb.Matrix("FP64", 37, 53)
    c(m.S, acc) << to_gb(gb, T).ewise_add(z, gb.binary.plus)
    check(c, want, "INT64", what="C(M.S, plus[FP64]) << U + empty")
    c = to_gb(gb, C)
    c(m.S, acc) << to_gb(gb, T)
    check(c, want, "INT64", what="C(M.S, plus[FP64]) << U (assign)")
    Cv, Tv, Mv = accum_case("INT64", (262245,), "producers")  # a second grid sweep of k_vec_merge
    c = to_gb(gb, Cv)
    c(~to_gb(gb, Mv).S, acc) << to_gb(gb, Tv).apply(gb.unary.identity)
    check(c, dm.write_back(Cv, Tv, mask=Mv, mask_struct=True, mask_comp=True, accum="plus", accum_dtype="FP64"),
          "INT64", what="262245-vector")


# ---------------------------------------------------------------------- column-word resident inputs
def colbits_q(gb, n=700, nq=5):
    """Q (nq x n, BOOL) = Q0 any.pair P computed with the colbits knob on, so the result is held
    as column words; and its model"""
    rng = _rng("colbits", n, nq)
    P = rng.random((n, n)) < 0.01
    Q0 = np.zeros((nq, n), bool)
    Q0[np.arange(nq), rng.permutation(n)[:nq]] = True
    Q0[0, rng.permutation(n)[:3]] = True
    pr, pc = np.nonzero(P)
    qr, qc = np.nonzero(Q0)
    p = gb.Matrix.from_coo(pr, pc, True, nrows=n, ncols=n)
    q = gb.Matrix.from_coo(qr, qc, True, nrows=nq, ncols=n)
    with _knobs(gb, colbits=1):
        q << q.mxm(p, gb.semiring.any_pair)
    present = (Q0.astype(np.int64) @ P.astype(np.int64)) > 0
    return q, (present, present.copy())


def test_colbits_resident_inputs(gb):
    q, Q = colbits_q(gb)
    assert Q[0].sum() > 20
    check(q, Q, "BOOL", what="colbits Q itself")
    rng = _rng("colbits-d")
    D = (rng.random(Q[0].shape) < 0.5, rng.random(Q[0].shape) < 0.5)
    d = to_gb(gb, D)
    q, _ = colbits_q(gb)
    check(q.ewise_mult(d, gb.binary.lxor).new(), dm.ewise("mult", "lxor", "BOOL", Q, D), "BOOL", what="colbits ewise_mult")
    q, _ = colbits_q(gb)
    check(d.ewise_add(q, gb.binary.land).new(), dm.ewise("add", "land", "BOOL", D, Q), "BOOL", what="colbits ewise_add")
    q, _ = colbits_q(gb)
    check(q.apply(gb.unary.lnot).new(), dm.apply("lnot", "BOOL", Q), "BOOL", what="colbits apply lnot")
    q, _ = colbits_q(gb)
    check(q.apply(gb.binary.plus["INT32"], right=41).new(), dm.apply("plus", "INT32", Q, right=np.int32(41)), "INT32",
          what="colbits apply plus")
    q, _ = colbits_q(gb)
    s = q.reduce_scalar(gb.monoid.plus["INT64"]).new()
    assert s.dtype == "INT64" and s.value == int(Q[0].sum())
    q, _ = colbits_q(gb)
    assert q.reduce_scalar(gb.monoid.land).new().value is True
    q, _ = colbits_q(gb)
    got = q.reduce_columnwise(gb.monoid.plus["INT32"]).new()
    check(got, dm.reduce_cols("plus", "INT32", Q), "INT32", what="colbits reduce_columnwise")
    q, _ = colbits_q(gb)
    check(q.reduce_rowwise(gb.monoid.lor).new(), dm.reduce_rows("lor", "BOOL", Q), "BOOL", what="colbits reduce_rowwise")
    q, _ = colbits_q(gb)
    check(q.T.new(), dm.transpose(Q), "BOOL", what="colbits .T")
    q, _ = colbits_q(gb)
    check(q.T.ewise_mult(to_gb(gb, dm.transpose(D)), gb.binary.lor).new(),
          dm.ewise("mult", "lor", "BOOL", dm.transpose(Q), dm.transpose(D)), "BOOL", what="colbits .T ewise")


# ---------------------------------------------------------------------- the comparator itself
def test_isequal_sees_one_value(gb):
    """isequal is eWiseMult(eq) + reduce(land): one differing value in the second grid sweep of a
    262245-vector must make it False"""
    for dt in ("INT64", "FP32"):
        A = reduce_input("min", dt, (262245,), "isequal", 0.9)
        if dt == "FP32":
            A = (A[0], np.where(np.isnan(A[1]), np.float32(1), A[1]))
        A[0][262200] = True
        a = to_gb(gb, A)
        assert a.isequal(a.dup()) is True and a.isequal(to_gb(gb, A)) is True
        B = (A[0], A[1].copy())
        B[1][262200] = B[1][262200] + dm.NP[dt](1) if B[1][262200] < 100 else dm.NP[dt](0)
        assert B[1][262200] != A[1][262200]
        b = to_gb(gb, B)
        assert b.nvals == a.nvals and a.isequal(b) is False and b.isequal(a) is False
        Cc = (A[0].copy(), A[1])
        Cc[0][262200] = False
        Cc[0][np.flatnonzero(~A[0])[-1]] = True  # same nvals, one index moved
        c = to_gb(gb, Cc)
        assert c.nvals == a.nvals and a.isequal(c) is False


def test_isequal_sees_one_moved_column(gb):
    for shape in [(37, 53), (300, 3)]:
        A = unary_input("identity", "INT32", shape, "isequal")
        v = np.where(A[0], np.int32(5), np.int32(0))  # equal values everywhere
        A = (A[0], v)
        a = to_gb(gb, A)
        assert a.isequal(a.dup()) is True and a.isequal(to_gb(gb, A)) is True
        r, c = np.nonzero(A[0])
        k = next(i for i in range(r.size) if not A[0][r[i], (c[i] + 1) % shape[1]])
        p = A[0].copy()
        p[r[k], c[k]] = False
        p[r[k], (c[k] + 1) % shape[1]] = True
        b = to_gb(gb, (p, np.where(p, np.int32(5), np.int32(0))))
        assert b.nvals == a.nvals and a.isequal(b) is False and b.isequal(a) is False
        assert a.isequal(to_gb(gb, (A[0], v * 1)), check_dtype=True) is True
        assert a.isequal(to_gb(gb, (A[0], v.astype(np.int64))), check_dtype=True) is False
