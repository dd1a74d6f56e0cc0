"""GxB_Matrix_scan / GxB_Vector_scan on the device against tests/scan_model.py and against the
recipe they replaced (``ss.prefix_scan``).

Every comparison goes through to_coo(): shape, dtype, nvals, indices in order and value bits.  NaNs
compare as NaN; float MIN / MAX compare +-0.0 as equal (the shared functor does not pin the sign);
ANY is checked as "each output is a value of its row at a column <= its own".

Shapes and what they reach (class bounds read from the knobs' defaults: 64, 4096, chunk 4096):
  LENGTHS     rows of 0 .. 4 and 62 .. 66 entries (the sub-wave class ends at 64), 511 .. 513,
              2047 .. 2049, 4095 .. 4097 (the workgroup class ends at 4096) and 6000 (a long row of
              two chunks), and 48 short rows packed between them, in 6000 columns; its transpose
              for the columnwise runs, so that columns reach the long class too
  lowered     scan_wave_max = 8, scan_block_max = 64, scan_chunk = 64: every class just above its
              bound, and single rows of 64^2 + 1 and 64^3 + 1 entries: chunk levels 2 and 3
  vectors     0, 1, 64, 65 and 70001 positions
The three stat counters are checked against the row lengths wherever a kernel over the entries ran.
"""
import numpy as np
import pytest

import dense_model as dm
import scan_model as sm
from test_general_ops_gpu import _knobs, _rng, coo_of, draw, iso_gb, to_gb

pytestmark = pytest.mark.gpu

NUMERIC = ("any", "plus", "times", "min", "max")
BITWISE = ("bor", "band", "bxor", "bxnor")
LOGICAL = ("lor", "land", "lxor", "lxnor")
UNSIGNED = ("UINT8", "UINT16", "UINT32", "UINT64")
LOWERED = dict(scan_wave_max=8, scan_block_max=64, scan_chunk=64)


@pytest.fixture(scope="module")
def gb():
    import graphblas_amd

    return graphblas_amd


def monoids_of(dt):
    """(front-end monoid name, the model's name) of every builtin monoid on dt"""
    if dt == "BOOL":
        return [(m, m) for m in LOGICAL] + [("any", "any"), ("eq", "lxnor")]
    return [(m, m) for m in NUMERIC + (BITWISE if dt in UNSIGNED else ())]


def lengths():
    base = [0, 1, 2, 3, 4, 62, 63, 64, 65, 66, 511, 512, 513, 2047, 2048, 2049, 4095, 4096, 4097, 6000]
    rng = _rng("scan lengths")
    more = list(rng.integers(0, 70, 48))  # short rows packed beside the long ones
    return [int(x) for x in rng.permutation(base + more)]


_MODELS = {}


def ragged(dt):
    """the LENGTHS matrix of type dt (shared: never written to)"""
    if dt not in _MODELS:
        rng = _rng("scan", dt)
        lens = lengths()
        p = np.zeros((len(lens), 6000), bool)
        for i, n in enumerate(lens):
            p[i, rng.choice(6000, n, replace=False)] = True
        v = draw(dt, rng, p.size).reshape(p.shape)
        _MODELS[dt] = (p, np.where(p, v, dm.NP[dt](0)))
    return _MODELS[dt]


def transposed(A):
    return np.ascontiguousarray(A[0].T), np.ascontiguousarray(A[1].T)


def is_iso(A):
    from graphblas_amd.device import matrix_view, vector_view

    return bool((vector_view if A.ndim == 1 else matrix_view)(A._h).iso)


def same_values(got, want, dt, what, zero_sign=True):
    assert got.dtype == want.dtype == dm.NP[dt], f"{what}: dtype {got.dtype}"
    assert got.shape == want.shape, what
    if not dm.is_float(dt):
        bad = got != want
    else:
        u = np.uint32 if dt == "FP32" else np.uint64
        bad = got.view(u) != want.view(u)
        bad &= ~(np.isnan(got) & np.isnan(want))
        if not zero_sign:
            bad &= ~((got == 0) & (want == 0))
    assert not bad.any(), f"{what}: {int(bad.sum())} values differ, first at {int(np.argmax(bad))}: " \
                          f"{got[bad][:4]} expected {want[bad][:4]}"


def same(obj, want, dt, what, zero_sign=True):
    """obj against the model pair ``want``: structure exactly, values by their bits"""
    wp, wv = want
    assert obj.dtype == dt, f"{what}: dtype {obj.dtype}, expected {dt}"
    assert tuple(obj.shape) == tuple(wp.shape), what
    idx, vals = coo_of(obj)
    widx = np.nonzero(wp)
    assert obj.nvals == widx[0].size == vals.size, f"{what}: nvals {obj.nvals}, expected {widx[0].size}"
    for a, b in zip(idx, widx):
        assert np.array_equal(a, b), f"{what}: indices differ"
    same_values(vals, wv[widx], dt, what, zero_sign)


def same_objects(a, b, what):
    """two library objects, bit for bit"""
    assert a.dtype == b.dtype and tuple(a.shape) == tuple(b.shape) and a.nvals == b.nvals, what
    ia, va = coo_of(a)
    ib, vb = coo_of(b)
    for x, y in zip(ia, ib):
        assert np.array_equal(x, y), f"{what}: indices differ"
    same_values(va, vb, dm.name_of(va.dtype), what)


def any_is_valid(obj, A, dt, columnwise, what):
    """every output of an ANY scan is a value of its row (column) at a column (row) <= its own"""
    p, v = A
    assert obj.dtype == dt and tuple(obj.shape) == p.shape and obj.nvals == int(p.sum()), what
    idx, vals = coo_of(obj)
    widx = np.nonzero(p)
    for a, b in zip(idx, widx):
        assert np.array_equal(a, b), f"{what}: indices differ"
    out = np.zeros(p.shape, dm.NP[dt])
    out[widx] = vals
    if columnwise:
        p, v, out = p.T, v.T, out.T
    for i in range(p.shape[0]):
        x, y = v[i][p[i]], out[i][p[i]]
        eq = (x == y) | ((x != x) & (y != y))
        for k in np.nonzero(~eq)[0]:
            assert np.isin(y[k], x[:k + 1]), f"{what}: row {i} position {k}"


def expect_stats(gb, A, columnwise, wave_max=64, block_max=4096, ran=True):
    d = A[0].sum(axis=0 if columnwise else 1)
    want = (int(((d >= 2) & (d <= wave_max)).sum()), int(((d > wave_max) & (d <= block_max)).sum()),
            int((d > max(block_max, 1)).sum())) if ran else (0, 0, 0)
    got = tuple(gb.get_knob(f"stat_scan_rows_{c}") for c in ("wave", "block", "long"))
    assert got == want, f"rows per class {got}, expected {want}"
    return got


def run(gb, a, A, dt, monoid, model, order, stats=None, what=""):
    col = order == "columnwise"
    mdt = "BOOL" if model in LOGICAL else dt
    what = f"{what}{dt} {monoid} {order}"
    C = a.ss.scan(getattr(gb.monoid, monoid), order)
    if model == "any":
        any_is_valid(C, A, mdt, col, what)
    else:
        same(C, sm.scan_matrix(A, model, mdt, columnwise=col), mdt, what,
             zero_sign=not (dm.is_float(dt) and model in ("min", "max")))
    if stats is not None:
        expect_stats(gb, A, col, ran=model != "any", **stats)
    return C


# ---------------------------------------------------------------------- 1. every (monoid, type) pair
@pytest.mark.parametrize("dt", dm.ALL)
def test_every_monoid_of_the_type(gb, dt):
    assert (gb.get_knob("scan_wave_max"), gb.get_knob("scan_block_max"), gb.get_knob("scan_chunk")) == (64, 4096, 4096)
    A = ragged(dt)
    At = transposed(A)
    a, at = to_gb(gb, A), to_gb(gb, At)
    for monoid, model in monoids_of(dt):
        run(gb, a, A, dt, monoid, model, "rowwise", stats={})
        got = run(gb, at, At, dt, monoid, model, "columnwise", stats={})
        assert tuple(got.shape) == At[0].shape
    assert all(expect_stats(gb, At, True))  # the shape reaches every class


@pytest.mark.parametrize("dt", ["INT16", "FP64"])
def test_logical_monoids_cast_their_input_to_bool(gb, dt):
    A = ragged(dt)
    a = to_gb(gb, A)
    for monoid in LOGICAL:
        run(gb, a, A, dt, monoid, monoid, "rowwise", stats={})
    run(gb, a, A, dt, "lxor", "lxor", "columnwise", stats={})


# ---------------------------------------------------------------------- 2. parity with the recipe
def parity_matrix():
    rng = _rng("scan parity")
    lens = rng.permutation(301)
    p = np.zeros((301, 400), bool)
    for i, n in enumerate(lens):
        p[i, rng.choice(400, n, replace=False)] = True
    return p


@pytest.mark.parametrize("dt,monoid", [("INT64", "plus"), ("FP64", "plus"), ("FP64", "times"), ("FP32", "plus"),
                                       ("FP64", "max")])
def test_same_bits_as_prefix_scan(gb, dt, monoid):
    """the test that shows floats did not change: ``A.ss.scan(op)`` is ``ss.prefix_scan(A, op)``"""
    from graphblas_amd.ss import prefix_scan

    p = parity_matrix()
    rng = _rng("scan parity values", dt, monoid)
    v = draw(dt, rng, p.size).reshape(p.shape)
    if dm.is_float(dt):  # finite values of mixed scales: every rounding shows, nothing turns to NaN
        v = np.where(np.isfinite(v), v, dm.NP[dt](1.25)).astype(dm.NP[dt])
    A = (p, np.where(p, v, dm.NP[dt](0)))
    op = getattr(gb.monoid, monoid)
    a = to_gb(gb, A)
    same_objects(a.ss.scan(op), prefix_scan(a, op), f"{dt} {monoid} rowwise")
    at = to_gb(gb, transposed(A))
    same_objects(at.ss.scan(op, order="col"), prefix_scan(at.T, op), f"{dt} {monoid} columnwise")
    # and the model is that order too
    same(a.ss.scan(op), sm.scan_matrix(A, monoid, dt), dt, f"{dt} {monoid} model", zero_sign=monoid != "max")
    pv = np.zeros(3000, bool)
    pv[rng.choice(3000, 1000, replace=False)] = True
    vv = draw(dt, rng, 3000)
    if dm.is_float(dt):
        vv = np.where(np.isfinite(vv), vv, dm.NP[dt](1.25)).astype(dm.NP[dt])
    u = to_gb(gb, (pv, np.where(pv, vv, dm.NP[dt](0))))
    same_objects(u.ss.scan(op), prefix_scan(u, op), f"{dt} {monoid} vector")


# ---------------------------------------------------------------------- 3. classes do not change bits
@pytest.mark.parametrize("dt,monoid", [("FP64", "plus"), ("INT64", "times")])
def test_lowered_class_bounds_keep_every_bit(gb, dt, monoid):
    A = ragged(dt)
    a = to_gb(gb, A)
    op = getattr(gb.monoid, monoid)
    default = a.ss.scan(op)
    expect_stats(gb, A, False)
    with _knobs(gb, **LOWERED):
        assert (gb.get_knob("scan_wave_max"), gb.get_knob("scan_block_max"), gb.get_knob("scan_chunk")) == (8, 64, 64)
        low = a.ss.scan(op)
        got = expect_stats(gb, A, False, wave_max=8, block_max=64)
        assert all(got), got
        same_objects(low, default, f"{dt} {monoid} lowered bounds")
        lowc = a.ss.scan(op, "columnwise")
        expect_stats(gb, A, True, wave_max=8, block_max=64)
    same_objects(lowc, a.ss.scan(op, "columnwise"), f"{dt} {monoid} lowered bounds, columnwise")
    same(default, sm.scan_matrix(A, monoid, dt), dt, f"{dt} {monoid} default bounds")


@pytest.mark.parametrize("n", [64 ** 2 + 1, 64 ** 3 + 1])
def test_single_long_rows_through_every_chunk_level(gb, n):
    rng = _rng("scan long row", n)
    x = (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, n)).astype(np.float64)
    A = (np.ones((1, n), bool), x[None, :])
    a = gb.Matrix.from_coo(np.zeros(n, np.int64), np.arange(n), x, dtype="FP64", nrows=1, ncols=n)
    want = sm.scan_matrix(A, "plus", "FP64")
    default = a.ss.scan(gb.monoid.plus)
    assert tuple(gb.get_knob(f"stat_scan_rows_{c}") for c in ("wave", "block", "long")) == (0, 0, 1)
    same(default, want, "FP64", f"one row of {n}, default chunk")
    with _knobs(gb, **LOWERED):
        low = a.ss.scan(gb.monoid.plus)
        assert tuple(gb.get_knob(f"stat_scan_rows_{c}") for c in ("wave", "block", "long")) == (0, 0, 1)
    same(low, want, "FP64", f"one row of {n}, chunk 64")
    with _knobs(gb, scan_chunk=256, scan_block_max=100):
        assert gb.get_knob("scan_chunk") == 256
        same(a.ss.scan(gb.monoid.plus), want, "FP64", f"one row of {n}, chunk 256")


# ---------------------------------------------------------------------- 4. vectors
@pytest.mark.parametrize("fill", ["half", "full", "empty"])
@pytest.mark.parametrize("n", [0, 1, 64, 65, 70001])
def test_vectors_equal_the_one_row_matrix(gb, n, fill):
    rng = _rng("scan vec", n, fill)
    p = {"half": rng.random(n) < 0.5, "full": np.ones(n, bool), "empty": np.zeros(n, bool)}[fill]
    for dt, monoid in (("FP64", "plus"), ("INT8", "times"), ("FP32", "min")):
        um = (p, np.where(p, draw(dt, rng, n), dm.NP[dt](0)))
        u = to_gb(gb, um)
        op = getattr(gb.monoid, monoid)
        w = u.ss.scan(op)
        what = f"vector {n} {fill} {dt} {monoid}"
        assert w.dup().nvals == int(p.sum()), what  # the device count is current
        same(w, sm.scan_vector(um, monoid, dt), dt, what, zero_sign=monoid != "min")
        if n:
            row = to_gb(gb, (p[None, :], um[1][None, :])).ss.scan(op)
            (_, rc), rv = coo_of(row)
            (wi,), wv = coo_of(w)
            assert np.array_equal(wi, rc) and np.array_equal(wi, np.nonzero(p)[0]), what  # u's bitmap
            same_values(wv, rv, dt, what + " against the 1 x n matrix")
    with _knobs(gb, **LOWERED):
        same_objects(u.ss.scan(op), w, f"vector {n} {fill} lowered bounds")


# ---------------------------------------------------------------------- 5. iso inputs
def test_iso_inputs(gb):
    p = ragged("INT16")[0]
    a, A = iso_gb(gb, p, -7, "INT16")
    at, At = iso_gb(gb, np.ascontiguousarray(p.T), -7, "INT16")
    assert is_iso(a)
    for monoid in ("min", "max", "any"):
        C = a.ss.scan(getattr(gb.monoid, monoid))
        assert is_iso(C), monoid
        same(C, A, "INT16", f"iso {monoid}")
        expect_stats(gb, A, False, ran=False)  # no kernel over the entries
        C = at.ss.scan(getattr(gb.monoid, monoid), "columnwise")
        assert is_iso(C), monoid
        same(C, At, "INT16", f"iso {monoid} columnwise")
    for monoid in ("lor", "land"):
        C = a.ss.scan(getattr(gb.monoid, monoid))
        assert is_iso(C), monoid
        same(C, (p, p.copy()), "BOOL", f"iso {monoid}")
    b, B = iso_gb(gb, p, 0x5A, "UINT8")
    for monoid in ("bor", "band"):
        C = b.ss.scan(getattr(gb.monoid, monoid))
        assert is_iso(C), monoid
        same(C, B, "UINT8", f"iso {monoid}")
    for monoid in ("plus", "times"):
        C = run(gb, a, A, "INT16", monoid, monoid, "rowwise", stats={}, what="iso ")
        assert not is_iso(C), monoid
        C = run(gb, at, At, "INT16", monoid, monoid, "columnwise", stats={}, what="iso ")
        assert not is_iso(C), monoid
    C = run(gb, a, A, "INT16", "lxor", "lxor", "rowwise", stats={}, what="iso ")
    assert not is_iso(C)
    f, F = iso_gb(gb, p, 0.1, "FP64")
    assert not is_iso(run(gb, f, F, "FP64", "plus", "plus", "rowwise", stats={}, what="iso "))
    # vectors
    pv = np.zeros(300, bool)
    pv[_rng("scan iso vec").choice(300, 170, replace=False)] = True
    u, um = iso_gb(gb, pv, 2.5, "FP32")
    w = u.ss.scan(gb.monoid.max)
    assert is_iso(w)
    same(w, um, "FP32", "iso vector max")
    w = u.ss.scan(gb.monoid.plus)
    assert not is_iso(w)
    same(w, sm.scan_vector(um, "plus", "FP32"), "FP32", "iso vector plus")


# ---------------------------------------------------------------------- 6. the ABI itself
def test_direct_calls_aliasing_typecast_and_errors(gb):
    lib = gb.lib
    A = ragged("INT64")
    plus, fplus = lib.GrB_PLUS_MONOID_INT64, lib.GrB_PLUS_MONOID_FP64
    want = sm.scan_matrix(A, "plus", "INT64")
    a = to_gb(gb, A)
    assert lib.GxB_Matrix_scan(a._h, plus, a._h, None) == 0  # C == A
    same(a, want, "INT64", "C == A")
    a = to_gb(gb, A)
    assert lib.GxB_Matrix_scan(a._h, plus, a._h, lib.GrB_DESC_T0) == 0
    same(a, sm.scan_matrix(A, "plus", "INT64", columnwise=True), "INT64", "C == A under T0")
    # C of another type takes the result cast to it; a prefilled (iso) C is replaced
    a = to_gb(gb, A)
    c32, _ = iso_gb(gb, ragged("INT16")[0], 3, "INT32")
    assert lib.GxB_Matrix_scan(c32._h, plus, a._h, None) == 0
    same(c32, (want[0], dm.cast(want[1], "INT32")), "INT32", "INT32 C from an INT64 monoid")
    F = ragged("FP64")
    f = to_gb(gb, F)
    c = gb.Matrix("FP32", *F[0].shape)
    assert lib.GxB_Matrix_scan(c._h, fplus, f._h, None) == 0
    wf = sm.scan_matrix(F, "plus", "FP64")
    same(c, (wf[0], dm.cast(wf[1], "FP32")), "FP32", "FP32 C from an FP64 monoid")
    # an INT64 A under an FP64 monoid: cast first, arithmetic in FP64
    c = gb.Matrix("FP64", *A[0].shape)
    assert lib.GxB_Matrix_scan(c._h, fplus, a._h, None) == 0
    same(c, sm.scan_matrix(A, "plus", "FP64"), "FP64", "INT64 A under an FP64 monoid")
    u = to_gb(gb, (A[0][5], A[1][5]))
    assert lib.GxB_Vector_scan(u._h, plus, u._h, None) == 0  # w == u
    same(u, sm.scan_vector((A[0][5], A[1][5]), "plus", "INT64"), "INT64", "w == u")
    # nothing stored, and no rows or no columns
    for shape in ((9, 11), (0, 5), (5, 0)):
        e = gb.Matrix("INT64", *shape)
        for desc in (None, lib.GrB_DESC_T0):
            c = gb.Matrix.from_coo([0], [0], [7], dtype="INT64", nrows=shape[0], ncols=shape[1]) if min(shape) \
                else gb.Matrix("INT64", *shape)
            assert lib.GxB_Matrix_scan(c._h, plus, e._h, desc) == 0
            assert c.nvals == 0 and tuple(c.shape) == shape
            assert e.ss.scan(gb.monoid.plus, "columnwise" if desc else "rowwise").nvals == 0
    # refusals leave C as it was
    C = gb.Matrix.from_coo([1, 2], [3, 4], [5, 6], dtype="INT64", nrows=A[0].shape[0], ncols=A[0].shape[1])
    Cs = gb.Matrix.from_coo([1, 2], [0, 2], [5, 6], dtype="INT64", nrows=7, ncols=3)
    Ct = gb.Matrix.from_coo([1, 2], [0, 2], [5, 6], dtype="INT64", nrows=A[0].shape[1], ncols=A[0].shape[0])
    w = gb.Vector.from_coo([2], [5], dtype="INT64", size=7)
    a = to_gb(gb, A)
    for wanted, args in [(lib.GrB_NULL_POINTER, (None, plus, a._h, None)),
                         (lib.GrB_NULL_POINTER, (C._h, None, a._h, None)),
                         (lib.GrB_NULL_POINTER, (C._h, plus, None, None)),
                         (lib.GrB_DIMENSION_MISMATCH, (Cs._h, plus, a._h, None)),
                         (lib.GrB_DIMENSION_MISMATCH, (Ct._h, plus, a._h, None)),
                         (lib.GrB_DIMENSION_MISMATCH, (Ct._h, plus, a._h, lib.GrB_DESC_T0)),
                         (lib.GrB_INVALID_OBJECT, (C._h, plus, u._h, None)),
                         (lib.GrB_INVALID_OBJECT, (w._h, plus, a._h, None))]:
        assert lib.GxB_Matrix_scan(*args) == wanted, (wanted, args)
    for wanted, args in [(lib.GrB_NULL_POINTER, (None, plus, u._h, None)),
                         (lib.GrB_NULL_POINTER, (w._h, None, u._h, None)),
                         (lib.GrB_NULL_POINTER, (w._h, plus, None, None)),
                         (lib.GrB_DIMENSION_MISMATCH, (w._h, plus, u._h, None)),
                         (lib.GrB_DIMENSION_MISMATCH, (w._h, plus, a._h, None))]:
        assert lib.GxB_Vector_scan(*args) == wanted, (wanted, args)
    for obj, idx, vals in ((C, ([1, 2], [3, 4]), [5, 6]), (Cs, ([1, 2], [0, 2]), [5, 6]), (Ct, ([1, 2], [0, 2]), [5, 6]),
                           (w, ([2],), [5])):
        got_idx, got = coo_of(obj)
        assert all(np.array_equal(x, y) for x, y in zip(got_idx, idx)) and np.array_equal(got, vals)


def test_front_end_is_one_call(gb):
    A = gb.Matrix.from_coo([0, 0, 2], [1, 2, 0], [1, 2, 3], nrows=3, ncols=3, dtype="INT64", name="A")
    v = gb.Vector.from_coo([0, 2], [1.5, 2.5], size=3, name="v")
    with gb.Recorder() as rec:
        C = A.ss.scan(gb.monoid.plus, name="C")
        D = A.ss.scan(gb.binary.times, order="columnwise", name="D")
        w = v.ss.scan(name="w")
    assert [line for line in rec.data if "_new(" not in line] == [
        "GxB_Matrix_scan(C, GrB_PLUS_MONOID_INT64, A, NULL);",
        "GxB_Matrix_scan(D, GrB_TIMES_MONOID_INT64, A, GrB_DESC_T0);",
        "GxB_Vector_scan(w, GrB_PLUS_MONOID_FP64, v, NULL);",
    ]
    assert len(rec.data) == 6  # and the three outputs' GrB_*_new: nothing is read back
    assert np.array_equal(coo_of(C)[1], [1, 3, 3]) and np.array_equal(coo_of(D)[1], [1, 2, 3])
    assert np.array_equal(coo_of(w)[1], [1.5, 4.0])
    with pytest.raises(TypeError, match="Bad type for argument `op`"):
        A.ss.scan(gb.binary.first)
    # the recipe's early exits return a dup in the input's type: they show under a logical monoid
    one = gb.Matrix.from_coo([0, 2], [1, 0], [4, 5], nrows=3, ncols=3, dtype="INT64")
    from graphblas_amd.ss import prefix_scan

    for x in (one, gb.Matrix.from_coo([0, 1], [0, 0], [4, 5], nrows=2, ncols=1, dtype="INT64"),
              gb.Vector.from_coo([1], [4], size=3, dtype="INT64")):
        same_objects(x.ss.scan(gb.monoid.lor), prefix_scan(x, gb.monoid.lor), "early exit")
        assert x.ss.scan(gb.monoid.lor).dtype == "INT64"
    assert A.ss.scan(gb.monoid.lor).dtype == "BOOL"
    same_objects(A.ss.scan(gb.monoid.lor), prefix_scan(A, gb.monoid.lor), "lor of INT64")


# ---------------------------------------------------------------------- 7. later grid sweeps
@pytest.mark.parametrize("cap", [1, 3, 33])
def test_under_grid_cap(gb, cap):
    A = ragged("INT64")
    a = to_gb(gb, A)
    rng = _rng("scan grid vec")
    p = rng.random(70001) < 0.5
    um = (p, np.where(p, draw("INT64", rng, 70001), np.int64(0)))
    u = to_gb(gb, um)
    wm, wmt, wv = a.ss.scan(gb.monoid.plus), a.ss.scan(gb.monoid.plus, "columnwise"), u.ss.scan(gb.monoid.plus)
    gb.set_knob("grid_cap", cap)
    try:
        same_objects(a.ss.scan(gb.monoid.plus), wm, f"grid_cap {cap}")
        expect_stats(gb, A, False)
        same_objects(a.ss.scan(gb.monoid.plus, "columnwise"), wmt, f"grid_cap {cap} columnwise")
        same_objects(u.ss.scan(gb.monoid.plus), wv, f"grid_cap {cap} vector")
        with _knobs(gb, **LOWERED):
            same_objects(a.ss.scan(gb.monoid.plus), wm, f"grid_cap {cap} lowered bounds")
            same_objects(u.ss.scan(gb.monoid.plus), wv, f"grid_cap {cap} vector, lowered bounds")
    finally:
        gb.set_knob("grid_cap", 0)
    same(wm, sm.scan_matrix(A, "plus", "INT64"), "INT64", "matrix")
    same(wv, sm.scan_vector(um, "plus", "INT64"), "INT64", "vector")
