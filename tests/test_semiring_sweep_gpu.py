"""Every builtin semiring through every mxm / mxv / vxm kernel, against tests/dense_model.py.

Breadth (test_every_semiring): the 1499 semirings of _builtins.SEMIRINGS, one case per (monoid,
multiplier) with the dtypes looped inside, on 24 x 17 x 29 operands (semiring_cases.py) through
hash, expand-sort-compress and window SpGEMM, the masked dot in its three forms, a complemented
mask with replace, both transposes, and the four SpMV forms with a sparse and a full u under the
default kernels, the general pull and the merge path.

Depth (the other tests): a representative list (REP: every monoid, multiplier class and dtype)
at the shapes where a kernel changes path: long SpMV rows, the hot-column relabel, iso operands,
long masked-dot lists over the narrowing boundaries, the hash bins of an R-MAT and operands of a
type other than the semiring's.

Every expectation is folded by the model in ascending, descending and shuffled order first and
must not depend on it (semiring_cases.Case, dm.order_dependent), so every comparison is exact:
indices, their order, nvals, dtype and the values by bits (NaNs equal).  Two exceptions: an
ANY result must be one of its entry's products, and a float entry is compared with == where the
sign of a zero is not defined (dm.zero_sign_free): a min / max monoid over a list with both
zeros, or a min / max multiplier that met +0.0 and -0.0, for which fmin / fmax may return either.
"""
import numpy as np
import pytest

import dense_model as dm
import semiring_cases as sc

pytestmark = pytest.mark.gpu

TABLE = sc.table()
PAIRS = sorted(TABLE)
RAN = {}  # library name -> the forms it ran through


@pytest.fixture(scope="module")
def gb():
    import graphblas_amd

    return graphblas_amd


class _knobs:
    def __init__(self, gb, **kv):
        self.gb, self.kv = gb, kv

    def __enter__(self):
        for k, v in self.kv.items():
            self.gb.set_knob(k, v)

    def __exit__(self, *a):
        for k in self.kv:
            self.gb.set_knob(k, 0)


def to_gb(gb, X, dt=None):
    p, v = X
    dt = dm.name_of(v.dtype) if dt is None else dt
    idx = np.nonzero(p)
    if p.ndim == 1:
        return gb.Vector.from_coo(idx[0], v[idx], dtype=dt, size=p.shape[0])
    return gb.Matrix.from_coo(idx[0], idx[1], v[idx], dtype=dt, nrows=p.shape[0], ncols=p.shape[1])


def iso_gb(gb, p, value, dt):
    idx = np.nonzero(p)
    x = dm.NP[dt](value).item()
    v = np.where(p, dm.NP[dt](value), dm.NP[dt](0))
    if p.ndim == 1:
        return gb.Vector.from_coo(idx[0], x, dtype=dt, size=p.shape[0]), (p, v)
    return gb.Matrix.from_coo(idx[0], idx[1], x, dtype=dt, nrows=p.shape[0], ncols=p.shape[1]), (p, v)


def is_iso(obj):
    from graphblas_amd.device import matrix_view, vector_view

    return bool((vector_view if obj.ndim == 1 else matrix_view)(obj._h).iso)


def _bits(a):
    return np.ascontiguousarray(a).view(np.dtype(f"u{a.dtype.itemsize}"))


def check(obj, want, zt, what, loose=None, anyof=None):
    """structure exactly; values by bits (NaNs equal), == where `loose`, members of their
    product list for the ANY monoid (anyof: the Products)"""
    wp, wv = want
    assert obj.dtype == zt, f"{what}: dtype {obj.dtype}, expected {zt}"
    assert tuple(obj.shape) == tuple(wp.shape), f"{what}: shape {obj.shape}, expected {wp.shape}"
    out = obj.to_coo()
    idx, vals = tuple(np.asarray(i).astype(np.int64) for i in out[:-1]), out[-1]
    widx = np.nonzero(wp)
    assert obj.nvals == widx[0].size, f"{what}: nvals {obj.nvals}, expected {widx[0].size}"
    for a, b in zip(idx, widx):
        assert np.array_equal(a, b), f"{what}: indices differ"
    assert vals.dtype == dm.NP[zt] and wv.dtype == dm.NP[zt], f"{what}: value dtype {vals.dtype} / {wv.dtype}"
    wvals = wv[widx]
    if anyof is not None:
        if len(idx) == 2:
            rows, cols = idx
        else:
            zero = np.zeros_like(idx[0])
            rows, cols = (idx[0], zero) if anyof.shape[1] == 1 else (zero, idx[0])
        ok = anyof.member(rows, cols, vals)
        assert ok.all(), f"{what}: {int((~ok).sum())} ANY values are none of their entry's products"
        return
    same = _bits(vals) == _bits(wvals)
    if vals.dtype.kind == "f":
        same |= np.isnan(vals) & np.isnan(wvals)
        if loose is not None:
            same |= loose[widx] & (vals == wvals)
    if not same.all():
        bad = np.flatnonzero(~same)
        q = bad[0]
        raise AssertionError(f"{what}: {bad.size} of {vals.size} values differ; first at "
                             f"{[int(i[q]) for i in idx]}: got {vals[q]!r}, expected {wvals[q]!r}")


# ---------------------------------------------------------------------- breadth
def run_forms(gb, case, sr, tag):
    """every form of the sweep for one semiring; returns (forms run, failures)"""
    zt, want = case.zt, case.want
    A, B = to_gb(gb, case.A), to_gb(gb, case.B)
    At, Bt = to_gb(gb, dm.transpose(case.A)), to_gb(gb, dm.transpose(case.B))
    Mg = to_gb(gb, case.mask)
    u = {k: to_gb(gb, v) for k, v in case.u.items()}
    ran, failed = [], []

    def chk(label, key, make):
        ran.append(label)
        name, T = want[key]
        try:
            check(make(), T, zt, f"{tag} {label}", loose=case.loose(key),
                  anyof=case.products[name] if case.monoid == "any" else None)
        except AssertionError as e:
            failed.append(str(e).splitlines()[0])

    def comp_replace():
        C = to_gb(gb, case.C0)
        C(~Mg.S, replace=True) << A.mxm(B, sr)
        return C

    chk("mxm", "mxm", lambda: A.mxm(B, sr).new())
    with _knobs(gb, spgemm_method=1):
        chk("mxm esc", "mxm", lambda: A.mxm(B, sr).new())
    with _knobs(gb, hash_window=1):
        chk("mxm window", "mxm", lambda: A.mxm(B, sr).new())
    chk("mxm struct", "mxm_struct", lambda: A.mxm(B, sr).new(mask=Mg.S))
    with _knobs(gb, dot_method=1):
        chk("mxm struct dot_method=1", "mxm_struct", lambda: A.mxm(B, sr).new(mask=Mg.S))
    with _knobs(gb, dot_group=8):
        chk("mxm struct dot_group=8", "mxm_struct", lambda: A.mxm(B, sr).new(mask=Mg.S))
    chk("mxm comp replace", "mxm_comp_replace", comp_replace)
    chk("mxm A.T", "mxm_AtB", lambda: At.T.mxm(B, sr).new())
    chk("mxm A.T struct", "mxm_AtB_struct", lambda: At.T.mxm(B, sr).new(mask=Mg.S))
    chk("mxm B.T", "mxm_ABt", lambda: A.mxm(Bt.T, sr).new())
    chk("mxm B.T struct", "mxm_ABt_struct", lambda: A.mxm(Bt.T, sr).new(mask=Mg.S))
    for kn in ({}, {"spmv_general": 1}, {"spmv_words": 2}):
        ktag = "".join(f" {k}={v}" for k, v in kn.items())
        with _knobs(gb, **kn):
            for fill in ("sparse", "full"):
                uk, un = u[("k", fill)], u[("n", fill)]
                chk(f"mxv {fill}{ktag}", f"mxv_{fill}", lambda: A.mxv(uk, sr).new())
                chk(f"vxm {fill}{ktag}", f"vxm_{fill}", lambda: un.vxm(A, sr).new())
                chk(f"A.T.mxv {fill}{ktag}", f"mxv_T_{fill}", lambda: A.T.mxv(un, sr).new())
                chk(f"vxm A.T {fill}{ktag}", f"vxm_T_{fill}", lambda: uk.vxm(A.T, sr).new())
    return ran, failed


N_FORMS = 11 + 3 * 8


@pytest.mark.parametrize("mon,mul", PAIRS, ids=[f"{a}_{b}" for a, b in PAIRS])
def test_every_semiring(gb, mon, mul):
    failures = []
    for pyname, dt, zt, names in TABLE[(mon, mul)]:
        sr = getattr(gb.semiring, pyname)[dt]
        assert sr.gb_name in names and sr.type.name == dt and sr.return_type.name == zt, (pyname, dt, sr.gb_name)
        case = sc.Case(mon, mul, dt, zt)
        ran, failed = run_forms(gb, case, sr, f"{pyname}[{dt}]")
        failures += failed
        for name in names:
            RAN[name] = ran
    assert not failures, f"{len(failures)} forms differ from the model:\n" + "\n".join(failures[:40])


def test_the_sweep_reaches_all_1499_semirings(gb):
    """every table name resolves through the front end to itself or its alias; every pair is a
    case of the sweep; whatever part of the sweep ran in this session ran all 35 forms"""
    names = set()
    for (mon, mul), entries in TABLE.items():
        for pyname, dt, zt, lib_names in entries:
            sr = getattr(gb.semiring, pyname)[dt]
            assert sr.gb_name in lib_names, (pyname, dt, sr.gb_name)
            names |= lib_names
    import graphblas_amd._builtins as b

    assert len(b.SEMIRINGS) == 1499 and names >= set(b.SEMIRINGS) and len(PAIRS) == 210
    assert sum(len(v) for v in TABLE.values()) == 1499
    for name, ran in RAN.items():
        assert len(ran) == N_FORMS and len(set(ran)) == N_FORMS, (name, ran)
    if RAN:  # the sweep ran in this session (it stands above this test): it must have been whole
        swept = set(RAN) & set(b.SEMIRINGS)
        assert len(swept) == 1499, f"the sweep ran {len(swept)} of 1499 semirings"


# ---------------------------------------------------------------------- depth
# (monoid, multiplier, dtype): every monoid, every multiplier class, every dtype
REP = [
    ("plus", "times", "INT8"), ("plus", "times", "FP32"), ("times", "plus", "UINT16"), ("plus", "plus", "FP64"),
    ("min", "minus", "INT16"), ("max", "rminus", "INT32"), ("min", "div", "FP64"), ("max", "rdiv", "UINT32"),
    ("plus", "div", "INT64"), ("plus", "minus", "UINT64"),
    ("min", "first", "UINT64"), ("max", "second", "INT16"), ("any", "pair", "BOOL"), ("any", "first", "INT32"),
    ("plus", "pair", "UINT8"),
    ("max", "isgt", "INT8"), ("plus", "isle", "FP32"), ("times", "isgt", "UINT32"),
    ("lor", "eq", "INT8"), ("land", "gt", "UINT64"), ("lxor", "le", "FP32"), ("lxnor", "gt", "INT8"),
    ("any", "le", "UINT64"), ("lor", "gt", "FP32"),
    ("lor", "land", "BOOL"), ("lxor", "land", "BOOL"), ("land", "lxor", "BOOL"), ("lxnor", "lor", "BOOL"),
    ("max", "land", "INT32"), ("plus", "lxor", "FP64"),
    ("bor", "band", "UINT8"), ("band", "bor", "UINT16"), ("bxor", "bxnor", "UINT32"), ("bxnor", "band", "UINT64"),
    ("bxnor", "bxnor", "UINT8"),
    ("min", "firsti", "INT64"), ("plus", "firstj1", "INT32"), ("max", "secondi", "INT32"),
    ("any", "secondj1", "INT64"), ("times", "secondj1", "INT32"),
]
CLASSES = {
    "commutative arithmetic": {"plus", "times"}, "ordered": {"minus", "rminus", "div", "rdiv"},
    "selection": {"first", "second", "pair"}, "is": {"isgt", "isle"}, "comparator": {"eq", "gt", "le"},
    "logical and bitwise": {"land", "lxor", "band", "bxnor"},
    "positional": {"firsti", "firstj1", "secondi", "secondj1"},
}


def _rep_id(s):
    return f"{s[0]}_{s[1]}-{s[2]}"


def lookup(gb, mon, mul, dt):
    """(typed semiring, result dtype) of a REP-style triple, through the table"""
    for pyname, key, zt, names in TABLE[(mon, mul)]:
        if key == dt:
            return getattr(gb.semiring, pyname)[dt], zt
    raise KeyError((mon, mul, dt))


def test_the_representative_list_covers_monoids_classes_and_types():
    assert {s[0] for s in REP} == {m for m, _ in PAIRS} and len({m for m, _ in PAIRS}) == 13
    muls = {s[1] for s in REP}
    for cls, members in CLASSES.items():
        assert members <= muls, cls
    assert {s[2] for s in REP} == set(dm.ALL)
    for mon, mul, dt in REP:
        assert any(key == dt for _, key, _, _ in TABLE[(mon, mul)]), (mon, mul, dt)
    comparators = {(s[1], s[2]) for s in REP if s[1] in dm.COMPARE}
    assert {dt for _, dt in comparators} >= {"INT8", "UINT64", "FP32"}


def expect(mon, mul, dt, fn, *args, what="", **kw):
    """the model's result and products, held to the order-independence condition"""
    T, P = fn(mon, mul, dt, *args, products=True, **kw)
    if mon != "any":
        bad = dm.order_dependent(mon, P)
        assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} expected entries depend on the fold order"
    loose = None
    if T[1].dtype.kind == "f":
        loose = P.dense(dm.zero_sign_free(mon, P), False).reshape(T[0].shape)
    return T, P, loose


def check_T(obj, exp, zt, mon, what):
    T, P, loose = exp
    check(obj, T, zt, what, loose=loose, anyof=P if mon == "any" else None)


def _vt(mul, dt):
    return "INT64" if mul in dm.POSITIONAL else dt


def _terminal_pair(mon, mul, dt, zt):
    """pool values (x, y) whose product is the monoid's terminal value, or None"""
    if mon not in sc.TERMINAL or mul in dm.POSITIONAL or dm.is_float(dt):
        return None
    p = sc.pool(dt)
    x, y = [a.ravel() for a in np.meshgrid(p, p, indexing="ij")]
    hit = np.flatnonzero(dm.cast(dm.binop(mul, dt, x, y), zt) == sc.named(zt, sc.TERMINAL[mon]))
    return (x[hit[0]], y[hit[0]]) if hit.size else None


# ---- SpMV long rows
LONG_SHAPE = (700, 1300)


def _long_rows(rng):
    """rows 0, 3, 4: 1100 entries (above the 1024 chunk); row 1: 130 (above the 128 long-row
    threshold); row 2 full; every fifth row empty; the others 0..6 entries"""
    n, m = LONG_SHAPE
    p = np.zeros((n, m), bool)
    for i in range(n):
        L = {0: 1100, 3: 1100, 4: 1100, 1: 130, 2: m}.get(i, 0 if i % 5 == 0 else int(rng.integers(0, 7)))
        p[i, rng.choice(m, L, replace=False)] = True
    return p


@pytest.mark.parametrize("sr3", [s for s in REP if not (s[0] == "times" and dm.is_float(s[2]))], ids=_rep_id)
def test_spmv_long_rows(gb, sr3):
    """k_spmv_words with lchunks and k_spmv_fold: the long rows as rows of the stored matrix (mxv
    and A.T's vxm) and, stored transposed, as its columns (vxm and A.T's mxv); the monoid's
    terminal value sits first in row 0, in the middle of row 3 and last in row 4"""
    mon, mul, dt = sr3
    sr, zt = lookup(gb, mon, mul, dt)
    rng = sc.rng_of("long", sr3)
    vt = _vt(mul, dt)
    n, m = LONG_SHAPE
    p = _long_rows(rng)
    av = sc.draw(vt, rng, (n, m), mon, mul)
    um = {"sparse": rng.random(m) < 0.5, "full": np.ones(m, bool)}
    un = {"sparse": rng.random(n) < 0.5, "full": np.ones(n, bool)}
    uvm, uvn = sc.draw(vt, rng, m, mon, mul), sc.draw(vt, rng, n, mon, mul)
    pair = _terminal_pair(mon, mul, dt, zt)
    if pair is not None:
        for row, where in ((0, 0), (3, 550), (4, -1)):
            c = np.flatnonzero(p[row])[where]
            av[row, c], uvm[c] = pair
            um["sparse"][c] = True
    A = p, np.where(p, av, dm.NP[vt](0))
    At = dm.transpose(A)
    Ag, Atg = to_gb(gb, A), to_gb(gb, At)
    for fill in ("sparse", "full"):
        U = um[fill], np.where(um[fill], uvm, dm.NP[vt](0))
        V = un[fill], np.where(un[fill], uvn, dm.NP[vt](0))
        ug, vg = to_gb(gb, U), to_gb(gb, V)
        tag = f"{_rep_id(sr3)} {fill}"
        e = expect(mon, mul, dt, dm.mxv, A, U, what=tag)
        if pair is not None and fill == "full":
            lists = e[1].lists()
            t = sc.named(zt, sc.TERMINAL[mon])
            assert lists[(0, 0)][0] == t and lists[(3, 0)][550] == t and lists[(4, 0)][-1] == t
        check_T(Ag.mxv(ug, sr).new(), e, zt, mon, f"{tag} mxv")
        check_T(Atg.T.mxv(ug, sr).new(), expect(mon, mul, dt, dm.mxv, At, U, tran0=True), zt, mon, f"{tag} At.T.mxv")
        check_T(ug.vxm(Atg, sr).new(), expect(mon, mul, dt, dm.vxm, U, At), zt, mon, f"{tag} vxm At")
        check_T(ug.vxm(Ag.T, sr).new(), expect(mon, mul, dt, dm.vxm, U, A, tran1=True), zt, mon, f"{tag} vxm A.T")
        # the short lists of the same matrices: the index spaces the other way round
        check_T(vg.vxm(Ag, sr).new(), expect(mon, mul, dt, dm.vxm, V, A), zt, mon, f"{tag} vxm")
        check_T(Ag.T.mxv(vg, sr).new(), expect(mon, mul, dt, dm.mxv, A, V, tran0=True), zt, mon, f"{tag} A.T.mxv")
        check_T(Atg.mxv(vg, sr).new(), expect(mon, mul, dt, dm.mxv, At, V), zt, mon, f"{tag} mxv At")
        check_T(vg.vxm(Atg.T, sr).new(), expect(mon, mul, dt, dm.vxm, V, At, tran1=True), zt, mon,
                f"{tag} vxm At.T")


# ---- hot-column relabel
HOT = [("min", "firsti", "INT64"), ("plus", "firstj1", "INT32"), ("max", "secondi", "INT32"),
       ("any", "secondj1", "INT64"), ("min", "minus", "INT16"), ("plus", "div", "INT64"),
       ("max", "rdiv", "UINT32"), ("lor", "gt", "FP32"), ("plus", "minus", "FP32")]


@pytest.mark.parametrize("sr3", HOT, ids=_rep_id)
def test_spmv_hot_columns(gb, sr3):
    """a full u on a 300 x 500 matrix whose first columns are hot, with the relabel forced (xhot =
    2, 64 hot columns): a positional multiplier must still see the true column, an ordered one
    the x value of the true column"""
    mon, mul, dt = sr3
    sr, zt = lookup(gb, mon, mul, dt)
    rng = sc.rng_of("hot", sr3)
    vt = _vt(mul, dt)
    n, m = 300, 500
    weight = 1.0 / (1 + rng.permutation(m))  # a few columns take most entries, scattered over the range
    p = rng.random((n, m)) < np.minimum(1.0, 12 * weight / weight.sum() * 6)[None, :]
    p[7] = True  # a full row
    A = p, np.where(p, sc.draw(vt, rng, (n, m), mon, mul), dm.NP[vt](0))
    U = np.ones(m, bool), sc.draw(vt, rng, m, mon, mul)
    V = np.ones(n, bool), sc.draw(vt, rng, n, mon, mul)
    mk = rng.random(n) < 0.5, np.ones(n, bool)
    empty = np.zeros(n, bool), np.zeros(n, dm.NP[zt])
    with _knobs(gb, xhot=2, xhot_cols=64):
        Ag, ug, vg, mg = to_gb(gb, A), to_gb(gb, U), to_gb(gb, V), to_gb(gb, mk)
        tag = _rep_id(sr3)
        e = expect(mon, mul, dt, dm.mxv, A, U, what=tag)
        check_T(Ag.mxv(ug, sr).new(), e, zt, mon, f"{tag} mxv")
        masked = dm.write_back(empty, e[0], mask=mk, mask_struct=True), e[1], e[2]
        check_T(Ag.mxv(ug, sr).new(mask=mg.S), masked, zt, mon, f"{tag} mxv mask")
        check_T(vg.vxm(Ag, sr).new(), expect(mon, mul, dt, dm.vxm, V, A), zt, mon, f"{tag} vxm")
        check_T(Ag.T.mxv(vg, sr).new(), expect(mon, mul, dt, dm.mxv, A, V, tran0=True), zt, mon, f"{tag} A.T.mxv")
        check_T(ug.vxm(Ag.T, sr).new(), expect(mon, mul, dt, dm.vxm, U, A, tran1=True), zt, mon, f"{tag} vxm A.T")


# ---- iso operands
# (monoid, multiplier, dtype, a, u, which operands are iso: "both", or "read" = only the one the multiplier reads)
ISO = [("max", "minus", "INT16", 5, -3, "both"), ("min", "div", "FP64", 3.0, -0.5, "both"),
       ("bor", "band", "UINT8", 0xF5, 0x3C, "both"), ("band", "bor", "UINT16", 0xF500, 0x3C, "both"),
       ("land", "gt", "INT32", 7, -2, "both"), ("lor", "le", "FP32", 0.5, 0.25, "both"),
       ("min", "first", "UINT64", 9, 4, "read"), ("max", "second", "INT8", -9, 4, "read"),
       ("any", "first", "INT32", 11, 4, "both"),
       ("plus", "times", "INT64", 3, 5, "both"), ("lxor", "land", "BOOL", True, True, "both")]
IDEMPOTENT = {"any", "min", "max", "lor", "land", "bor", "band"}


def _iso_spmv_operands(gb, case, n):
    """The operands of one ISO case on the n x (n + 13) pattern with one long row: yields
    (kind, fill, Ag, ug, expected) for mxv and vxm with a one-entry and a dense u."""
    mon, mul, dt, a, b, which = case
    rng = sc.rng_of("iso", case, n)
    m = n + 13
    p = rng.random((n, m)) < 8.0 / n
    p[3] = rng.random(m) < 0.5  # one long row
    A_iso_g, A_iso = iso_gb(gb, p, a, dt)
    assert is_iso(A_iso_g)
    if which == "read":
        noise_A = np.zeros((n, m), dm.NP[dt])
        noise_A[p] = sc.draw(dt, rng, int(p.sum()))
        noise_A = p, noise_A
        A_var_g = to_gb(gb, noise_A)
    for fill in ("one", "dense"):
        for kind in ("mxv", "vxm"):
            size = m if kind == "mxv" else n
            up = np.zeros(size, bool)
            if fill == "one":
                up[size // 3] = True
            else:
                up[:] = True
            u_iso_g, U_iso = iso_gb(gb, up, b, dt)
            U_var = up, np.where(up, sc.draw(dt, rng, size), dm.NP[dt](0))
            # which operand does the multiplier read?  mxv: mult(a, u); vxm: mult(u, a)
            reads_first, reads_second = mul != "second", mul != "first"
            reads_A = reads_first if kind == "mxv" else reads_second
            reads_u = reads_second if kind == "mxv" else reads_first
            if which == "read":
                Ag, Am = (A_iso_g, A_iso) if reads_A else (A_var_g, noise_A)
                ug, Um = (u_iso_g, U_iso) if reads_u else (to_gb(gb, U_var), U_var)
            else:
                Ag, Am, ug, Um = A_iso_g, A_iso, u_iso_g, U_iso
            if kind == "mxv":
                e = expect(mon, mul, dt, dm.mxv, Am, Um)
            else:
                e = expect(mon, mul, dt, dm.vxm, Um, Am)
            yield kind, fill, Ag, ug, e


@pytest.mark.parametrize("n", [300, 5000])
@pytest.mark.parametrize("case", ISO, ids=lambda c: f"{c[0]}_{c[1]}-{c[2]}-{c[5]}")
def test_iso_operands_spmv(gb, case, n):
    """A and u built from a scalar: an idempotent monoid gives an iso result (the BFS kernel,
    k_iso_work, with the one value from gb_iso_eval), in every direction, for a one-entry and a
    dense u; FIRST / SECOND need only the operand they read to be iso, also under the vxm swap.
    A non-idempotent monoid must not come out iso: its values are counts and parities."""
    mon, mul, dt = case[:3]
    sr, zt = lookup(gb, mon, mul, dt)
    want_iso = mon in IDEMPOTENT
    for kind, fill, Ag, ug, e in _iso_spmv_operands(gb, case, n):
        for direction in (0, 1, 2):
            with _knobs(gb, spmv_direction=direction):
                w = (Ag.mxv(ug, sr) if kind == "mxv" else ug.vxm(Ag, sr)).new()
            what = f"{mon}_{mul}[{dt}] n={n} {kind} u={fill} direction={direction}"
            check_T(w, e, zt, mon, what)
            assert is_iso(w) == want_iso, f"{what}: iso {is_iso(w)}, expected {want_iso}"


# z is bool and x is not; z = x, not bool; only the operand that is read is iso
ISO_LAUNCH = [c for c in ISO if c[:3] in {("land", "gt", "INT32"), ("max", "minus", "INT16"), ("min", "first", "UINT64")}]


@pytest.mark.parametrize("case", ISO_LAUNCH, ids=lambda c: f"{c[0]}_{c[1]}-{c[2]}-{c[5]}")
def test_iso_value_in_every_launch_shape(gb, case):
    """The iso value has one writer, gb_iso_eval in k_iso_work, whatever launches the call
    makes: with and without the prep launch (host_dir 1 forces it when nothing is known about
    the frontier), in every direction, with the packed finish (value written up front) and the
    unpacked one (iso_packed 1: written late, by the finishing block)."""
    mon, mul, dt = case[:3]
    assert len(ISO_LAUNCH) == 3
    sr, zt = lookup(gb, mon, mul, dt)
    for kind, fill, Ag, ug, e in _iso_spmv_operands(gb, case, 300):
        for direction in (0, 1, 2):
            for host_dir in (0, 1):
                for iso_packed in (0, 1):
                    with _knobs(gb, spmv_direction=direction, host_dir=host_dir, iso_packed=iso_packed):
                        w = (Ag.mxv(ug, sr) if kind == "mxv" else ug.vxm(Ag, sr)).new()
                    what = (f"{mon}_{mul}[{dt}] {kind} u={fill} direction={direction} host_dir={host_dir} "
                            f"iso_packed={iso_packed}")
                    check_T(w, e, zt, mon, what)
                    assert is_iso(w), f"{what}: not iso"


@pytest.mark.parametrize("case", ISO, ids=lambda c: f"{c[0]}_{c[1]}-{c[2]}-{c[5]}")
def test_iso_operands_mxm(gb, case):
    mon, mul, dt, a, b, which = case
    sr, zt = lookup(gb, mon, mul, dt)
    rng = sc.rng_of("iso-mxm", case)
    n, k, m = 60, 45, 70
    pa, pb = rng.random((n, k)) < 0.2, rng.random((k, m)) < 0.2
    mk = rng.random((n, m)) < 0.3
    mk = mk, mk.copy()
    Ag, A = iso_gb(gb, pa, a, dt)
    Bg, B = iso_gb(gb, pb, b, dt)
    if which == "read":  # only the operand the multiplier reads is iso
        if mul == "first":
            B = pb, np.where(pb, sc.draw(dt, rng, (k, m)), dm.NP[dt](0))
            Bg = to_gb(gb, B)
        else:
            A = pa, np.where(pa, sc.draw(dt, rng, (n, k)), dm.NP[dt](0))
            Ag = to_gb(gb, A)
    e = expect(mon, mul, dt, dm.mxm, A, B)
    what = f"{mon}_{mul}[{dt}] iso mxm"
    C = Ag.mxm(Bg, sr).new()
    check_T(C, e, zt, mon, what)
    assert is_iso(C) == (mon in IDEMPOTENT), f"{what}: iso {is_iso(C)}"
    empty = np.zeros((n, m), bool), np.zeros((n, m), dm.NP[zt])
    masked = dm.write_back(empty, e[0], mask=mk, mask_struct=True), e[1], e[2]
    C = Ag.mxm(Bg, sr).new(mask=to_gb(gb, mk).S)
    check_T(C, masked, zt, mon, f"{what} struct")
    assert is_iso(C) == (mon in IDEMPOTENT), f"{what} struct: iso {is_iso(C)}"


# ---- masked dot with long lists over the narrowing boundaries
DOT = [("min", "div", "INT64"), ("plus", "minus", "INT64"), ("max", "minus", "INT32"), ("bxnor", "bxnor", "UINT64"),
       ("bxor", "band", "UINT32"), ("lor", "gt", "INT64"), ("land", "gt", "INT16"), ("plus", "times", "INT64"),
       ("min", "plus", "INT32"), ("times", "plus", "INT8"), ("max", "second", "UINT16")]
DOT_KNOBS = [(0, 0, 0, 0), (128, 256, 0, 0), (300, 256, 1, 0)]


DOT_KINDS = ["s8", "u8", "s16", "u16", "s32", "u32", "full"]


def _edge_values(dt, kind):
    """the edges of a signed (s) or unsigned (u) integer of that many bits, or of dt itself: a
    matrix of them narrows to exactly that width"""
    lo, hi = dm.tmin(dt), dm.tmax(dt)
    if kind == "full":
        vals = [lo, lo + 1, hi - 1, hi, 0, 1] + ([-1] if lo < 0 else [])
    else:
        b = 1 << (int(kind[1:]) - 1)
        vals = [-b, -b + 1, -1, 0, 1, b - 2, b - 1] if kind[0] == "s" else [0, 1, b - 1, b, 2 * b - 2, 2 * b - 1]
    assert all(lo <= v <= hi for v in vals), (dt, kind)
    return np.array(vals, dtype=object).astype(dm.NP[dt])


def _dot_params():
    out = []
    for sr3 in DOT:
        lo, hi = dm.tmin(sr3[2]), dm.tmax(sr3[2])
        for kind in DOT_KINDS:
            if kind != "full":
                bits = int(kind[1:])
                if (kind[0] == "s" and -(1 << (bits - 1)) < lo) or (1 << bits) - 1 > hi and kind[0] == "u" or \
                        (kind[0] == "s" and (1 << (bits - 1)) - 1 >= hi):
                    continue  # not a narrower kind of this dtype
            out.append(pytest.param(sr3, kind, id=f"{_rep_id(sr3)}-{kind}"))
    return out


def _long_both(rng, shape, long_rows, long_cols, L):
    p = rng.random(shape) < 4.0 / shape[1]
    for i in long_rows:
        p[i, rng.choice(shape[1], L, replace=False)] = True
    for j in long_cols:
        p[rng.choice(shape[0], min(L, shape[0]), replace=False), j] = True
    return p


@pytest.mark.parametrize("sr3,kind", _dot_params())
def test_masked_dot_long_lists(gb, sr3, kind):
    """C<M.S> = A (+).(x) B with rows of A and columns of B of 320 entries, under the knob tuples
    of the two-sided dot (defaults; short task windows; a cap of 300 keys with the hub lists on
    the per-entry kernel); the values sit on the edges of +-127/128, +-32767/32768, +-2^31 and of
    the type, so each narrowed copy (1, 2, 4 bytes, signed and unsigned) and the wide values run"""
    mon, mul, dt = sr3
    sr, zt = lookup(gb, mon, mul, dt)
    rng = sc.rng_of("dot", sr3, kind)
    n, k, m = 330, 400, 350
    hubs_r, hubs_c = [0, 5, 77, 329], [1, 9, 200, 349]
    pa = _long_both(rng, (n, k), hubs_r, [3, 250], 320)
    pb = _long_both(rng, (k, m), [3, 250], hubs_c, 320)
    ev = _edge_values(dt, kind)
    A = pa, np.where(pa, ev[rng.integers(0, ev.size, (n, k))], dm.NP[dt](0))
    B = pb, np.where(pb, ev[rng.integers(0, ev.size, (k, m))], dm.NP[dt](0))
    mp = rng.random((n, m)) < 0.05
    mp[np.ix_(hubs_r, hubs_c)] = True
    mp[0], mp[:, 1] = True, True
    mk = mp, mp.copy()
    empty = np.zeros((n, m), bool), np.zeros((n, m), dm.NP[zt])
    e = expect(mon, mul, dt, dm.mxm, A, B)
    assert e[1].lists()[(0, 1)].size > 200
    masked = dm.write_back(empty, e[0], mask=mk, mask_struct=True), e[1], e[2]
    for cap, win, pieces, yblk in DOT_KNOBS:
        with _knobs(gb, dot_cap=cap, dot_win=win, dot_pieces=pieces, dot_yblk=yblk, dot_pmin=1):
            # fresh matrices: their narrow copies are built under these knobs
            Ag, Bg, Btg, Mg = to_gb(gb, A), to_gb(gb, B), to_gb(gb, dm.transpose(B)), to_gb(gb, mk)
            what = f"{_rep_id(sr3)} {kind} knobs {(cap, win, pieces, yblk)}"
            check_T(Ag.mxm(Bg, sr).new(mask=Mg.S), masked, zt, mon, f"{what} A B")
            check_T(Ag.mxm(Btg.T, sr).new(mask=Mg.S), masked, zt, mon, f"{what} A Bt.T")
            check_T(Ag.mxm(Bg, sr).new(mask=Mg.V), masked, zt, mon, f"{what} A B value mask")


# ---- hash bins
HASH = [("min", "firsti", "INT64"), ("plus", "firstj1", "INT32"), ("max", "secondi", "INT32"),
        ("any", "secondj1", "INT64"), ("plus", "secondj", "INT64"), ("plus", "minus", "INT32"),
        ("min", "div", "INT16"), ("max", "rdiv", "UINT32"), ("lor", "gt", "INT8"), ("times", "times", "INT32"),
        ("bxnor", "bxor", "UINT16"), ("plus", "minus", "FP32"), ("min", "rminus", "FP64")]
HASH_METHODS = ["hash", "hash_window", "hash_window_c", "hash_window_lw10"]


@pytest.mark.parametrize("sr3", HASH, ids=_rep_id)
def test_hash_spgemm_rmat(gb, sr3):
    """C = A (+).(x) B unmasked, A an R-MAT of scale 10 (rows in every bin of the hash Gustavson;
    with hash_window every row on the column-window kernel, which rebuilds j from its window
    offset).  B is [A' A A'] cut to 2500 columns: the three index spaces differ, and window_lw =
    10 cuts it into three windows of 1024 columns (at 1024 columns or fewer there is one window,
    its offset is 0 and a lost offset would not show)"""
    import oracle as O

    mon, mul, dt = sr3
    sr, zt = lookup(gb, mon, mul, dt)
    rng = sc.rng_of("hash", sr3)
    vt = _vt(mul, dt)
    G = O.rmat(10, 16, 7)
    r, c, _ = G.to_coo()
    n = G.nrows
    pa = np.zeros((n, n), bool)
    pa[r, c] = True
    pb = np.ascontiguousarray(np.hstack([pa.T, pa, pa.T])[:, :2500])
    A = pa, np.where(pa, sc.draw(vt, rng, (n, n), mon, mul), dm.NP[vt](0))
    B = pb, np.where(pb, sc.draw(vt, rng, pb.shape, mon, mul), dm.NP[vt](0))
    e = expect(mon, mul, dt, dm.mxm, A, B, what=_rep_id(sr3))
    Ag, Bg = to_gb(gb, A), to_gb(gb, B)
    for method in HASH_METHODS:
        with _knobs(gb, hash_window=int(method != "hash"), window_vcap=512 if method == "hash_window_c" else 0,
                    window_in_c_groups=1 if method == "hash_window_c" else 0,
                    window_lw=10 if method == "hash_window_lw10" else 0):
            check_T(Ag.mxm(Bg, sr).new(), e, zt, mon, f"{_rep_id(sr3)} {method}")


# ---- operands of another type than the semiring's
def _fp64_wild(rng, shape):
    pool = np.array([0.0, -0.0, 0.5, -0.5, 1.0, 1.5, 2.75, -3.25, 127.0, 128.9, 255.0, 255.5, 256.0, 300.7, -1.0,
                     -129.0, 2.0 ** 31, -2.0 ** 31 - 1, 2.0 ** 40, 1e300, -1e300, np.inf, -np.inf, np.nan])
    return pool[rng.integers(0, pool.size, shape)]


CASTS = [("plus", "times", "INT32", "INT8", "FP64"), ("lor", "gt", "UINT8", "FP64", "FP64"),
         ("plus", "plus", "FP32", "BOOL", "BOOL")]


@pytest.mark.parametrize("mon,mul,dt,ta,tb", CASTS, ids=lambda x: str(x).lower())
def test_operands_of_another_type(gb, mon, mul, dt, ta, tb):
    """gb_view_vals_as casts A, B and u to the multiplier's input type: FP64 saturates into the
    integer types (NaN -> 0, fractions truncate), BOOL becomes 0 / 1"""
    sr, zt = lookup(gb, mon, mul, dt)
    rng = sc.rng_of("casts", mon, mul, dt)
    n, k, m = sc.N, sc.K, sc.M

    def operand(t, shape):
        p = rng.random(shape) < 0.35
        v = _fp64_wild(rng, shape) if t == "FP64" else sc.draw(t, rng, shape)
        return p, np.where(p, v, dm.NP[t](0))

    A, B = operand(ta, (n, k)), operand(tb, (k, m))
    uk, un = operand(tb, (k,)), operand(tb, (n,))
    mp = rng.random((n, m)) < 0.4
    mk = mp, mp.copy()
    Ag, Bg, ukg, ung, Mg = to_gb(gb, A), to_gb(gb, B), to_gb(gb, uk), to_gb(gb, un), to_gb(gb, mk)
    assert Ag.dtype == ta and Bg.dtype == tb
    what = f"{mon}_{mul}[{dt}] on {ta} x {tb}"
    e = expect(mon, mul, dt, dm.mxm, A, B, what=what)
    empty = np.zeros((n, m), bool), np.zeros((n, m), dm.NP[zt])
    check_T(Ag.mxm(Bg, sr).new(), e, zt, mon, f"{what} mxm")
    with _knobs(gb, spgemm_method=1):
        check_T(Ag.mxm(Bg, sr).new(), e, zt, mon, f"{what} mxm esc")
    masked = dm.write_back(empty, e[0], mask=mk, mask_struct=True), e[1], e[2]
    check_T(Ag.mxm(Bg, sr).new(mask=Mg.S), masked, zt, mon, f"{what} mxm struct")
    with _knobs(gb, dot_method=1):
        check_T(Ag.mxm(Bg, sr).new(mask=Mg.S), masked, zt, mon, f"{what} mxm struct dot_method=1")
    check_T(Ag.mxv(ukg, sr).new(), expect(mon, mul, dt, dm.mxv, A, uk), zt, mon, f"{what} mxv")
    check_T(ung.vxm(Ag, sr).new(), expect(mon, mul, dt, dm.vxm, un, A), zt, mon, f"{what} vxm")
    check_T(Ag.T.mxv(ung, sr).new(), expect(mon, mul, dt, dm.mxv, A, un, tran0=True), zt, mon, f"{what} A.T.mxv")
    check_T(ukg.vxm(Ag.T, sr).new(), expect(mon, mul, dt, dm.vxm, uk, A, tran1=True), zt, mon, f"{what} vxm A.T")
