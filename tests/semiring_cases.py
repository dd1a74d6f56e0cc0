"""Inputs and expected results of the semiring sweep (test_semiring_sweep_gpu.py), built from the
dense model alone so that test_dense_model.py can check them without a GPU.

The builtin table.  `table()` reads graphblas_amd/_builtins.py (as a file: no device needed) and
groups the 1499 semirings by (monoid, multiplier); every entry carries the front-end name and the
dtype it is keyed by (the multiplier's input type; the result type for a positional multiplier).

Value pools.  The kernels fold in lane, chunk or arrival order, so the pools are chosen to make
the model's own result independent of the order:
  integers, bool   0, +-1, the type's extremes (all ones for unsigned) and a few mid values;
                   wrap-around arithmetic is associative and commutative, so any order is exact.
                   Where the multiplier can produce them at all, the monoid's terminal value and
                   its identity are planted as the first product of an entry of A.B.
  floats           +-2^e with e in [-2, 2], +-3.2^e unless the multiplier divides or the monoid
                   is TIMES, and +-0.0, +-inf, NaN.  Sums of at most 29 such products are exact
                   in FP32, so PLUS is order-free; for TIMES no list is longer than 4 products
                   (sums of two powers of two carry 5 bits: 20 bits in all, no overflow).
`dm.order_dependent` folds every expected entry ascending, descending and shuffled and raises unless all
three agree in every entry: no entry is ever dropped.
"""
import importlib.util
import os
import zlib

import numpy as np

import dense_model as dm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, K, M = 24, 17, 29  # all distinct: an index-space mix-up changes the result or the shape

TERMINAL = {"min": "tmin", "max": "tmax", "times": 0, "bor": "ones", "band": 0, "lor": 1, "land": 0}
IDENTITY = {"plus": 0, "times": 1, "min": "tmax", "max": "tmin", "lor": 0, "land": 1, "lxor": 0, "lxnor": 1,
            "bor": 0, "band": "ones", "bxor": 0, "bxnor": "ones"}


def _builtins():
    path = os.path.join(ROOT, "graph-python_amd", "graphblas_amd", "_builtins.py")
    spec = importlib.util.spec_from_file_location("_gb_builtins_table", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def table():
    """{(monoid, multiplier): [(front-end name, dtype key, monoid dtype, {library names})]}"""
    b = _builtins()
    out = {}
    for gbname, (mon, bop, aliases) in b.SEMIRINGS.items():
        m, mt, _ = b.MONOIDS[mon]
        op, xt, _zt = b.BINOPS[bop]
        src = aliases[0] if aliases else gbname
        parts = src[4:].replace("_SEMIRING", "").split("_")
        pyname, key = "_".join(parts[:-1]).lower(), parts[-1]
        assert key == (xt if xt is not None else mt), gbname
        out.setdefault((m.lower(), op.lower()), []).append((pyname, key, mt, {gbname, *aliases}))
    return out


def rng_of(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


# ---------------------------------------------------------------------- pools
def named(dt, v):
    t = dm.NP[dt]
    if isinstance(v, str):
        if dt == "BOOL":
            return t(v in ("tmax", "ones"))
        if dm.is_float(dt):
            return t({"tmin": -np.inf, "tmax": np.inf}[v])
        return t(dm.tmin(dt) if v == "tmin" else dm.tmax(dt))  # ones: unsigned types only
    return t(v)


def pool(dt, monoid="plus", mul="times"):
    t = dm.NP[dt]
    if dt == "BOOL":
        return np.array([False, True])
    if dm.is_int(dt):
        lo, hi = dm.tmin(dt), dm.tmax(dt)
        vals = [0, 1, hi, hi - 1, 2, 3, 5, 100, hi // 2 + 1, hi // 3]
        if lo < 0:
            vals += [-1, lo, lo + 1, -2, -100]
        return np.array(vals, t)
    mant = [1.0] if mul in ("div", "rdiv") or monoid == "times" else [1.0, 3.0]
    fin = [s * c * 2.0 ** e for s in (1, -1) for c in mant for e in range(-2, 3)]
    return np.array(fin + [0.0, -0.0, np.inf, -np.inf, np.nan], t)


def draw(dt, rng, shape, monoid="plus", mul="times"):
    p = pool(dt, monoid, mul)
    if not dm.is_float(dt):
        return p[rng.integers(0, p.size, shape)]
    nfin = p.size - 5
    w = np.r_[np.full(nfin, 0.8 / nfin), [0.04, 0.04, 0.03, 0.03, 0.06]]
    return p[rng.choice(p.size, size=shape, p=w)]


def _thin(ap, bp, cap):
    """drop entries of A until no entry of A.B has more than `cap` products"""
    ap = ap.copy()
    while True:
        cnt = ap.astype(np.int64) @ bp.astype(np.int64)
        if cnt.max() <= cap:
            return ap
        i, j = np.unravel_index(np.argmax(cnt), cnt.shape)
        ap[i, np.flatnonzero(ap[i] & bp[:, j])[-1]] = False


class Case:
    """The operands of one (monoid, multiplier, dtype) and the expected result of every form."""

    def __init__(self, monoid, mul, dt, zt):
        self.monoid, self.mul, self.dt, self.zt = monoid, mul, dt, zt
        rng = rng_of("sweep", monoid, mul, dt)
        positional = mul in dm.POSITIONAL
        vt = "INT64" if positional else dt  # operand values of a positional product are not read
        ap, bp = rng.random((N, K)) < 0.3, rng.random((K, M)) < 0.3
        un, uk = rng.random(N) < 0.4, rng.random(K) < 0.4
        self.planted = []
        if dm.is_float(dt) and monoid == "times":
            ap = _thin(ap, np.ones((K, 1), bool), 4)
            ap = _thin(ap.T, np.ones((N, 1), bool), 4).T
            bp = _thin(bp.T, ap.T, 4).T
        av, bv = draw(vt, rng, (N, K), monoid, mul), draw(vt, rng, (K, M), monoid, mul)
        if not positional and not dm.is_float(dt):
            self._plant(ap, av, bp, bv)
        z = dm.NP[vt](0)
        self.A = ap, np.where(ap, av, z)
        self.B = bp, np.where(bp, bv, z)
        self.u = {("k", "sparse"): (uk, np.where(uk, draw(vt, rng, K, monoid, mul), z)),
                  ("k", "full"): (np.ones(K, bool), draw(vt, rng, K, monoid, mul)),
                  ("n", "sparse"): (un, np.where(un, draw(vt, rng, N, monoid, mul), z)),
                  ("n", "full"): (np.ones(N, bool), draw(vt, rng, N, monoid, mul))}
        mp = rng.random((N, M)) < 0.4
        self.mask = mp, mp.copy()
        cp = rng.random((N, M)) < 0.3
        self.C0 = cp, np.where(cp, draw(zt, rng, (N, M)), dm.NP[zt](0))
        self.products = {}
        self.want = {}
        self._expect()

    def _plant(self, ap, av, bp, bv):
        """the monoid's terminal value and identity as the first product of T(q, q), q = 0, 1,
        followed by at least one more product"""
        p = pool(self.dt)
        x, y = [a.ravel() for a in np.meshgrid(p, p, indexing="ij")]
        zs = dm.cast(dm.binop(self.mul, self.dt, x, y), self.zt)
        targets = [d[self.monoid] for d in (TERMINAL, IDENTITY) if self.monoid in d]
        for q, target in enumerate(targets):
            hit = np.flatnonzero(zs == named(self.zt, target))
            if hit.size == 0:
                continue  # this multiplier cannot produce it from the pool
            ap[q, :2] = bp[:2, q] = True
            av[q, 0], bv[0, q] = x[hit[0]], y[hit[0]]
            self.planted.append((q, named(self.zt, target)))

    def _T(self, name, fn, *args, **kw):
        T, P = fn(self.monoid, self.mul, self.dt, *args, products=True, **kw)
        assert T[1].dtype == dm.NP[self.zt], (name, T[1].dtype)
        if self.monoid != "any":
            bad = dm.order_dependent(self.monoid, P)
            if bad.any():
                raise AssertionError(f"{self.monoid}_{self.mul}[{self.dt}] {name}: {int(bad.sum())} of {bad.size} "
                                     f"expected entries depend on the fold order; fix the pool")
        self.products[name] = P
        return T

    def _expect(self):
        A, B, mask, C0, zt = self.A, self.B, self.mask, self.C0, self.zt
        T = self._T("AB", dm.mxm, A, B)
        empty = np.zeros((N, M), bool), np.zeros((N, M), dm.NP[zt])
        w = self.want
        w["mxm"] = ("AB", T)
        w["mxm_struct"] = ("AB", dm.write_back(empty, T, mask=mask, mask_struct=True))
        w["mxm_comp_replace"] = ("AB", dm.write_back(C0, T, mask=mask, mask_comp=True, mask_struct=True,
                                                     replace=True))
        # the same product with a stored transpose undone by the descriptor: the model transposes
        # back itself, so the positional indices are those of the operands as multiplied
        for name, kw in (("AtB", dict(tran0=True)), ("ABt", dict(tran1=True))):
            X = dm.transpose(A) if "tran0" in kw else A
            Y = dm.transpose(B) if "tran1" in kw else B
            Tt = self._T(name, dm.mxm, X, Y, **kw)
            w[f"mxm_{name}"] = (name, Tt)
            w[f"mxm_{name}_struct"] = (name, dm.write_back(empty, Tt, mask=mask, mask_struct=True))
        for fill in ("sparse", "full"):
            uk, un = self.u[("k", fill)], self.u[("n", fill)]
            w[f"mxv_{fill}"] = (f"mxv_{fill}", self._T(f"mxv_{fill}", dm.mxv, A, uk))
            w[f"vxm_{fill}"] = (f"vxm_{fill}", self._T(f"vxm_{fill}", dm.vxm, un, A))
            w[f"mxv_T_{fill}"] = (f"mxv_T_{fill}", self._T(f"mxv_T_{fill}", dm.mxv, A, un, tran0=True))
            w[f"vxm_T_{fill}"] = (f"vxm_T_{fill}", self._T(f"vxm_T_{fill}", dm.vxm, uk, A, tran1=True))

    def check_planted(self):
        """every planted terminal / identity is the first of at least two products of its entry"""
        lists = self.products["AB"].lists()
        for q, value in self.planted:
            z = lists[(q, q)]
            assert z.size >= 2 and z[0] == value, (self.monoid, self.mul, self.dt, q, z, value)

    def loose(self, form):
        """dense mask of the entries whose zero may have either sign (dm.zero_sign_free)"""
        name, (wp, _) = self.want[form]
        P = self.products[name]
        if not dm.is_float(self.zt):
            return None
        return P.dense(dm.zero_sign_free(self.monoid, P), False).reshape(wp.shape)
