"""The case tables of tests/test_indexing_gpu.py (extract, assign, element access, resize) and the
model expectation of every case, without a GPU: the GPU file runs each case on the device and
compares with `build(case).want`; tests/test_dense_model.py walks the same tables on the CPU, so
every form the GPU file uses goes through the model there too.

A case is an operation name plus a dict of parameters; inputs are seeded by zlib.crc32 of them.
`assert_coverage()` states what the tables must hold (every type, every mask kind, every listed
size, for each operation) and is run by both files.
"""
import itertools
import types
import zlib

import numpy as np

import dense_model as dm

MASK_KINDS = ("none", "S", "V", "~S", "~V")
# a write-back variant: (mask kind, replace, accumulator name or None); the front end refuses
# replace without a mask
WB_PLAIN = ("none", False, None)
WB_ALL = [(k, r, a) for k in MASK_KINDS for r in (False, True) if not (k == "none" and r) for a in (None, "plus")]
WB_ASSIGN = [(k, r, a) for k in MASK_KINDS for r in (False, True) if not (k == "none" and r)
             for a in (None, "plus", "second")]


def rng_of(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def wb_kw(wb, M):
    """the model's keyword arguments of a write-back variant"""
    kind, rep, acc = wb
    kw = dict(replace=rep, accum=acc)
    if kind != "none":
        kw.update(mask=M, mask_struct="S" in kind, mask_comp=kind.startswith("~"))
    return kw


# ---------------------------------------------------------------------- value pools
def specials(dt):
    """the pools of test_general_ops_gpu.py: type minimum / maximum, +-0.0, NaN, infinities"""
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
                     f.smallest_normal, 1.0, -1.0, 0.5, -0.5, 1.5, 2.5, -2.5, f.max, -f.max], t)


def draw(dt, rng, n):
    """n values of dt: half of them specials, the others random"""
    t = dm.NP[dt]
    if dt == "BOOL":
        return rng.random(n) < 0.5
    if dm.is_int(dt):
        out = rng.integers(dm.tmin(dt), dm.tmax(dt), n, dtype=t, endpoint=True)
    else:
        out = (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, n)).astype(t)
    sp = specials(dt)
    return np.where(rng.random(n) < 0.5, sp[rng.integers(0, sp.size, n)], out).astype(t)


def iso_value(dt):
    """the one value of an iso object of dt (non-zero, so it is true as a value mask)"""
    return dm.NP[dt](True if dt == "BOOL" else (dm.tmax(dt) - 1 if dm.is_int(dt) else -2.5))


def scalar_value(dt, key):
    """a scalar to assign: a non-trivial special of dt"""
    sp = specials(dt)
    return sp[int(rng_of("x", dt, key).integers(1, sp.size))]


def obj(dt, shape, key, density=0.5, kind="sparse"):
    """a model object: kind sparse / full / empty / iso (every entry iso_value(dt)) / never (no
    entry, and the device object has never been written)"""
    rng = rng_of("obj", dt, shape, key, kind)
    n = int(np.prod(shape))
    if kind in ("empty", "never"):
        p = np.zeros(n, bool)
    elif kind == "full":
        p = np.ones(n, bool)
    else:
        p = rng.random(n) < density
    v = np.full(n, iso_value(dt)) if kind == "iso" else draw(dt, rng, n)
    return p.reshape(shape), np.where(p, v, dm.NP[dt](0)).reshape(shape)


MASK_CONTENTS = ("sparse", "iso_true", "iso_false", "empty", "full", "fp64")


def mask_obj(shape, key, content="sparse"):
    """a mask object: sparse (BOOL with stored false), iso_true / iso_false (one BOOL value), empty,
    full (BOOL with stored false) or fp64 (FP64 values: 0.0 and -0.0 are false, NaN is true)"""
    rng = rng_of("mask", shape, key, content)
    n = int(np.prod(shape))
    p = {"empty": np.zeros(n, bool), "full": np.ones(n, bool)}.get(content, rng.random(n) < 0.5)
    if content == "fp64":
        v = np.array([0.0, -0.0, np.nan, 1.5, -np.inf, 5e-324])[rng.integers(0, 6, n)]
    elif content in ("iso_true", "iso_false"):
        v = np.full(n, content == "iso_true")
    else:
        v = rng.random(n) < 0.5
    return p.reshape(shape), np.where(p, v, v.dtype.type(0)).reshape(shape)


# ---------------------------------------------------------------------- named matrices and lists
ROW_LENGTHS = (0, 1, 63, 64, 65, 128, 129, 300)  # rows 0..7 of the 70 x 300 matrix "rows"
HOT_ROW, HOT_COL = 6, 137                        # the 129-entry row holds column 137
LINE_LENGTHS = (0, 1, 65, 1000)                  # columns 0..3 of the 1000 x 70 matrix "lines"


def _ragged(rng, nrows, ncols, maxrow=3):
    p = np.zeros((nrows, ncols), bool)
    lens = rng.integers(0, maxrow + 1, nrows)
    for k in range(maxrow):
        rows = np.flatnonzero(lens > k)
        p[rows, rng.integers(0, ncols, rows.size)] = True
    return p


_MATRICES = {}


def matrix_named(name, dt, kind="sparse"):
    """rows   70 x 300: rows of 0, 1, 63, 64, 65, 128, 129 and 300 entries, the others 0..3
    empty  70 x 300 without entries
    small  70 x 90 of density 0.2;  square  70 x 70 of density 0.3;  low  40 x 90 (at most 64 rows)
    tall   140000 x 70 with 0..3 entries per row;  wide  70 x 140000, its transpose shape
    lines  1000 x 70: columns of 0, 1, 65 and 1000 entries, the others of density 0.3
    one    1 x 1 with its entry"""
    key = (name, dt, kind)
    if key in _MATRICES:
        return _MATRICES[key]
    rng = rng_of("matrix", name, dt)
    if name in ("rows", "empty"):
        p = np.zeros((70, 300), bool)
        if name == "rows":
            p[8:] = _ragged(rng, 62, 300)
            for i, k in enumerate(ROW_LENGTHS):
                p[i, rng.permutation(300)[:k]] = True
            if not p[HOT_ROW, HOT_COL]:
                p[HOT_ROW, np.flatnonzero(p[HOT_ROW])[0]] = False
                p[HOT_ROW, HOT_COL] = True
            assert tuple(p[:8].sum(axis=1)) == ROW_LENGTHS
    elif name in ("small", "square", "low"):
        shape = {"small": (70, 90), "square": (70, 70), "low": (40, 90)}[name]
        p = rng.random(shape) < (0.3 if name == "square" else 0.2)
    elif name == "tall":
        p = _ragged(rng, 140000, 70)
    elif name == "wide":
        p = np.ascontiguousarray(_ragged(rng, 140000, 70).T)
    elif name == "lines":
        p = rng.random((1000, 70)) < 0.3
        for j, k in enumerate(LINE_LENGTHS):
            p[:, j] = False
            p[rng.permutation(1000)[:k], j] = True
    elif name == "one":
        p = np.ones((1, 1), bool)
    else:
        raise KeyError(name)
    v = np.full(p.shape, iso_value(dt)) if kind == "iso" else draw(dt, rng, p.size).reshape(p.shape)
    A = p, np.where(p, v, dm.NP[dt](0))
    if p.size > 10**6:  # only the big ones are worth caching
        _MATRICES[key] = A
    return A


def index_named(name, n, key, hot=0):
    """None (GrB_ALL) or an int64 list over range(n):
    all; one; empty; rev (reversed range); perm; unsorted (a permutation's first 2/5); sorted (the
    same, ascending); revsorted; dup (n/2 + 3 random picks: repeats); rep100 / rep200 (`hot` that
    many times; rep200 among 20 other columns); special (rows 0..7 twice and 20 others, shuffled);
    len<k> (k random picks); prefix<k> (the first k of a permutation, a tenth overwritten by picks:
    repeats)"""
    rng = rng_of("index", name, n, key)
    if name == "all":
        return None
    if name == "one":
        return np.array([hot if hot < n else n // 2], np.int64)
    if name == "empty":
        return np.zeros(0, np.int64)
    if name == "rev":
        return np.arange(n, dtype=np.int64)[::-1].copy()
    if name == "perm":
        return rng.permutation(n).astype(np.int64)
    if name in ("unsorted", "sorted", "revsorted"):
        I = rng.permutation(n)[:max(1, 2 * n // 5)].astype(np.int64)
        return I if name == "unsorted" else (np.sort(I) if name == "sorted" else np.sort(I)[::-1].copy())
    if name == "dup":
        return rng.integers(0, n, n // 2 + 3)
    if name == "rep100":
        return np.full(100, hot, np.int64)
    if name == "rep200":
        return rng.permutation(np.r_[np.full(200, hot), rng.permutation(n)[:20]]).astype(np.int64)
    if name == "special":
        return rng.permutation(np.r_[np.arange(8), np.arange(8), rng.integers(8, n, 20)]).astype(np.int64)
    if name.startswith("len"):
        return rng.integers(0, n, int(name[3:]))
    if name.startswith("prefix"):
        k = int(name[6:])
        I = rng.permutation(n)[:k].astype(np.int64)
        I[rng.integers(0, k, k // 10)] = rng.integers(0, n, k // 10)
        return I
    raise KeyError(name)


# ---------------------------------------------------------------------- cases
class Case:
    def __init__(self, op, **p):
        self.op, self.p = op, p

    def get(self, k, default=None):
        return self.p.get(k, default)

    @property
    def id(self):
        return self.op + "(" + ", ".join(f"{k}={v}" for k, v in self.p.items()) + ")"

    def __repr__(self):
        return self.id


def _result(**kw):
    return types.SimpleNamespace(**kw)


def _write_back(c, B, T, shape, key):
    """the output side shared by the extracts: none (.new()), or C<M> = accum(C, T) with C of type
    `ctype`, optionally aliasing an input"""
    dt, wb = c.p["dt"], c.get("wb")
    if wb is None:
        B.want, B.want_dt = T, dt
        return B
    ct = c.get("ctype", dt)
    alias = c.get("alias")
    B.C = B.A if alias == "C=A" else obj(ct, shape, key + ("C",), 0.4)
    B.M = {"M=C": B.C, "M=A": B.A}.get(alias) or mask_obj(shape, key)
    assert B.C[0].shape == shape and B.M[0].shape == shape
    B.want, B.want_dt = dm.write_back(B.C, T, **wb_kw(wb, B.M)), ct
    return B


def _matrix_extract_cases():
    out = []
    add = lambda **p: out.append(Case("matrix_extract", **p))
    for dt in dm.ALL:  # every row length and value size, J all and J a list
        add(A="rows", dt=dt, I="special", J="all")
        add(A="rows", dt=dt, I="special", J="dup")
    for J in ("unsorted", "rev", "dup", "rep200", "one", "empty"):
        add(A="rows", dt="INT32", I="special", J=J)
        add(A="rows", dt="FP64", I="all", J=J)
    for I in ("dup", "rep100", "one", "empty"):
        add(A="rows", dt="INT16", I=I, J="all")
        add(A="rows", dt="FP32", I=I, J="unsorted")
    add(A="rows", dt="INT8", I="rep100", J="rep200")
    for J in ("all", "dup"):
        add(A="rows", dt="INT32", I="special", J=J, kind="iso")
        add(A="rows", dt="UINT8", I="special", J=J, kind="iso")
        add(A="empty", dt="FP64", I="dup", J=J)
    add(A="one", dt="INT64", I="all", J="all")
    add(A="one", dt="INT64", I="len5", J="len3")
    # scans and stride loops: 133125 = 131072 + 2048 + 5 output rows (the tile scan of cnt, the
    # wave stride loop above 65536 rows), again through hipCUB, and one row short of the threshold
    add(A="tall", dt="INT32", I="prefix133125", J="all")
    add(A="tall", dt="INT32", I="prefix133125", J="len40")
    add(A="tall", dt="INT32", I="prefix133125", J="len40", scan_u8=1)
    add(A="tall", dt="INT32", I="prefix131071", J="len40")
    add(A="wide", dt="INT16", I="all", J="len3000")  # the tile scan of jcnt over 140000 columns
    add(A="wide", dt="INT16", I="dup", J="len3000", scan_u8=1)
    for wb in WB_ALL:
        add(A="small", dt="INT64", I="dup", J="unsorted", wb=wb)
    for wb in (WB_PLAIN, ("V", False, "plus"), ("~S", True, None)):
        add(A="small", dt="FP64", I="dup", J="unsorted", wb=wb, ctype="INT8")
        add(A="small", dt="INT64", I="dup", J="unsorted", wb=wb, ctype="BOOL")
    for acc in (None, "plus"):
        add(A="square", dt="INT32", I="perm", J="perm", wb=("none", False, acc), alias="C=A")
        add(A="square", dt="INT32", I="perm", J="perm", wb=("V", False, acc), alias="C=A")
        for mk in ("S", "V", "~V"):
            add(A="square", dt="INT32", I="perm", J="perm", wb=(mk, True, acc), alias="M=C")
            add(A="square", dt="INT32", I="perm", J="perm", wb=(mk, False, acc), alias="M=A")
    for wb in (WB_PLAIN, ("S", True, "plus"), ("~V", False, None)):  # GrB_DESC_T0, the CSC cached
        add(A="small", dt="INT64", I="dup", J="unsorted", wb=wb, tran=True)
    add(A="rows", dt="FP32", I="dup", J="all", wb=WB_PLAIN, tran=True)
    return out


def _build_matrix_extract(c):
    key = (c.id,)
    dt = c.p["dt"]
    A = matrix_named(c.p["A"], dt, c.get("kind", "sparse"))
    src = dm.transpose(A) if c.get("tran") else A
    B = _result(A=A)
    B.I = index_named(c.p["I"], src[0].shape[0], key + ("I",), HOT_ROW)
    B.J = index_named(c.p["J"], src[0].shape[1], key + ("J",), HOT_COL)
    T = dm.extract(src, B.I, B.J)
    return _write_back(c, B, T, T[0].shape, key)


COL_I = ("len1", "len63", "len64", "len65", "len257", "len1000", "all", "dup", "empty")


def _col_extract_cases():
    out = []
    add = lambda **p: out.append(Case("col_extract", **p))
    for orient in ("col", "row"):
        for j in range(5):  # lines of 0, 1, 65, 1000 and about 300 entries
            for I in COL_I:
                add(orient=orient, dt="INT32", j=j, I=I)
        for dt in dm.ALL:
            add(orient=orient, dt=dt, j=2, I="len257")
            add(orient=orient, dt=dt, j=3, I="all")
        add(orient=orient, dt="INT16", j=4, I="len257", kind="iso")
        add(orient=orient, dt="FP64", j=3, I="len65", kind="iso")
        for wb in WB_ALL:
            add(orient=orient, dt="INT64", j=4, I="len65", wb=wb)
        add(orient=orient, dt="FP64", j=4, I="len65", wb=("V", False, "plus"), ctype="INT8")
    return out


def _build_col_extract(c):
    """A(I, j) of the 1000 x 70 matrix "lines" (orient col), or A(j, I) of its transpose (row):
    the same vector either way"""
    key = (c.id,)
    dt = c.p["dt"]
    K = matrix_named("lines", dt, c.get("kind", "sparse"))
    B = _result(A=K if c.p["orient"] == "col" else dm.transpose(K), j=c.p["j"])
    B.I = index_named(c.p["I"], 1000, key + ("I",))
    T = dm.extract_vec((K[0][:, B.j], K[1][:, B.j]), B.I)
    return _write_back(c, B, T, T[0].shape, key)


VEC_SIZES = (1, 63, 64, 65, 70001)
VEC_KINDS = ("sparse", "full", "empty", "iso")


def _vector_extract_cases():
    out = []
    add = lambda **p: out.append(Case("vector_extract", **p))
    for n in VEC_SIZES:
        for kind in VEC_KINDS:
            for I in ("all", "rev", "dup"):
                add(n=n, dt="INT32", kind=kind, I=I)
        for m in (1, 64, 65, 70001):  # output lengths
            add(n=n, dt="FP64", kind="sparse", I=f"len{m}")
    for dt in dm.ALL:
        add(n=65, dt=dt, kind="sparse", I="len65")
        add(n=70001, dt=dt, kind="sparse", I="len257")
    for wb in WB_ALL:
        add(n=300, dt="INT64", kind="sparse", I="len65", wb=wb)
        add(n=300, dt="INT64", kind="iso", I="len63", wb=wb, ctype="FP32")
    for n in (1, 65, 70001):
        for acc in (None, "plus"):
            add(n=n, dt="INT32", kind="sparse", I="perm", wb=("none", False, acc), alias="C=A")
        add(n=n, dt="INT32", kind="sparse", I="perm", wb=("~V", True, None), alias="M=C")
    return out


def _build_vector_extract(c):
    key = (c.id,)
    B = _result(A=obj(c.p["dt"], (c.p["n"],), key, kind=c.p["kind"]))
    B.I = index_named(c.p["I"], c.p["n"], key + ("I",))
    T = dm.extract_vec(B.A, B.I)
    return _write_back(c, B, T, T[0].shape, key)


# ---- scalar assign into a vector
# k_assign_mask_words: a block of 256 threads is 4 waves of 16 mask words each, and the launch is
# capped at 2048 blocks, so one sweep covers 2048 * 64 words of 64 bits; 5 more words and 37 bits
# enter the stride loop and end in a partial word
ASSIGN_STRIDE_N = 2048 * 64 * 64 + 64 * 5 + 37
ASSIGN_SIZES = (1, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4133, 262245, ASSIGN_STRIDE_N)
ASSIGN_MASKS = MASK_CONTENTS + ("alias",)
W_KINDS = ("never", "iso", "sparse", "full")


def _vector_assign_scalar_cases():
    out = []
    add = lambda **p: out.append(Case("vector_assign_scalar", **p))
    for n in ASSIGN_SIZES:
        if n == ASSIGN_STRIDE_N:  # about 70 MB of values: one type, three mask kinds
            for wb in (("S", False, None), ("V", False, None), ("~S", True, None)):
                add(n=n, dt="INT64", w="sparse", mask="sparse", wb=wb)
            continue
        big = n > 5000
        add(n=n, dt="INT32", w="sparse", mask="none", wb=WB_PLAIN)
        add(n=n, dt="INT32", w="never", mask="none", wb=WB_PLAIN)
        masks = ("sparse", "iso_true", "alias") if big else ASSIGN_MASKS
        for q, (mask, kind, rep) in enumerate(itertools.product(masks, MASK_KINDS[1:], (False, True))):
            # the state of w before the call rotates through the table; all four are crossed below
            add(n=n, dt="INT32", w=W_KINDS[q % 4], mask=mask, wb=(kind, rep, None))
    for n in (65, 1025):
        for w in W_KINDS:  # every state of w before the call against every kind of mask
            add(n=n, dt="UINT16", w=w, mask="none", wb=WB_PLAIN)
            for mask, kind, rep in itertools.product(("sparse", "iso_true", "alias"), MASK_KINDS[1:], (False, True)):
                add(n=n, dt="UINT16", w=w, mask=mask, wb=(kind, rep, None))
        for wb in WB_ALL:
            add(n=n, dt="FP64", w="sparse", mask="none" if wb[0] == "none" else "sparse", wb=wb)
        for dt in dm.ALL:  # x and w of every type
            add(n=n, dt=dt, w="sparse", mask="sparse", wb=("V", False, None))
            add(n=n, dt=dt, w="iso", mask="sparse", wb=("~V", True, None))
            add(n=n, dt=dt, w="never", mask="none", wb=WB_PLAIN)
    # x of another type than w, through the typed entry point of x's type
    for dt in ("INT8", "UINT8", "BOOL"):
        for x in (np.nan, 1e30, -0.5):
            add(n=65, dt=dt, xdt="FP64", x=x, w="sparse", mask="sparse", wb=("S", False, None))
            add(n=65, dt=dt, xdt="FP64", x=x, w="sparse", mask="none", wb=("none", False, "plus"))
    add(n=65, dt="FP64", xdt="INT64", x=2**53 + 1, w="sparse", mask="sparse", wb=("~S", False, None))
    add(n=65, dt="INT64", xdt="FP64", x=float(2**53 + 2), w="sparse", mask="sparse", wb=("V", True, None))
    # accumulators and index lists (repeats allowed), the empty scalar
    for n in (1, 63, 65, 1025):
        for acc in ("plus", "min"):
            for kind, rep in (("none", False), ("S", False), ("V", True), ("~S", True), ("~V", False)):
                add(n=n, dt="INT16", w="sparse", mask="sparse", wb=(kind, rep, acc))
                add(n=n, dt="FP32", w="iso", mask="sparse", wb=(kind, rep, acc), I="dup")
        for kind, rep in (("none", False), ("S", False), ("V", True), ("~S", True), ("~V", False), ("S", True)):
            add(n=n, dt="INT64", w="sparse", mask="sparse", wb=(kind, rep, None), I="dup")
            add(n=n, dt="INT64", w="full", mask="alias", wb=(kind, rep, None), I="unsorted")
            add(n=n, dt="INT32", w="sparse", mask="sparse", wb=(kind, rep, None), I="dup", x=None)
            add(n=n, dt="INT32", w="sparse", mask="sparse", wb=(kind, rep, None), x=None)
        add(n=n, dt="INT32", w="sparse", mask="sparse", wb=("none", False, "plus"), I="dup", x=None)
        add(n=n, dt="INT32", w="sparse", mask="sparse", wb=("S", False, "plus"), x=None)
    return out


def _scalar_of(c, key):
    """(x as a numpy scalar of its own type, or None for the empty scalar; the type's name)"""
    xdt = c.get("xdt", c.p["dt"])
    if "x" in c.p:
        return (None if c.p["x"] is None else dm.NP[xdt](c.p["x"])), xdt
    return scalar_value(xdt, key), xdt


def _build_vector_assign_scalar(c):
    key = (c.id,)
    n, dt = c.p["n"], c.p["dt"]
    B = _result(w=obj(dt, (n,), key, kind=c.p["w"]))
    if c.p["wb"][0] == "none":
        B.M = None
    else:
        B.M = B.w if c.p["mask"] == "alias" else mask_obj((n,), key, c.p["mask"])
    B.x, B.xdt = _scalar_of(c, key)
    B.I = index_named(c.get("I", "all"), n, key + ("I",))
    B.want, B.want_dt = dm.assign_vec(B.w, B.x, B.I, **wb_kw(c.p["wb"], B.M)), dt
    return B


# ---- object assign into a vector
def _vector_assign_cases():
    out = []
    add = lambda **p: out.append(Case("vector_assign", **p))
    for n in VEC_SIZES:
        for I in ("sorted", "revsorted", "unsorted", "empty", "all"):
            for u in ("empty", "sparse", "full", "iso"):
                add(n=n, dt="INT32", u=u, I=I, wb=WB_PLAIN)
                add(n=n, dt="INT32", u=u, I=I, wb=("~V", False, None))
        add(n=n, dt="INT8", udt="FP64", u="sparse", I="unsorted", wb=WB_PLAIN)
        add(n=n, dt="FP32", udt="INT64", u="sparse", I="all", wb=("S", True, "plus"))
    for n in (1, 63, 65, 70001):
        for wb in WB_ASSIGN:
            if n < 70001 or wb[2] != "second":
                add(n=n, dt="INT64", u="sparse", I="unsorted", wb=wb)
                add(n=n, dt="INT64", u="sparse", I="all", wb=wb)
        for acc in (None, "plus"):  # the mask aliasing w (two code paths), the mask aliasing u
            for kind, rep in (("S", False), ("V", True), ("~S", True), ("~V", False)):
                add(n=n, dt="INT16", u="sparse", I="unsorted", wb=(kind, rep, acc), alias="M=w")
                add(n=n, dt="INT16", u="sparse", I="perm", wb=(kind, rep, acc), alias="M=u")
                add(n=n, dt="INT16", u="sparse", I="all", wb=(kind, rep, acc), alias="M=u")
    for dt in dm.ALL:
        add(n=65, dt=dt, u="sparse", I="unsorted", wb=("V", False, None))
    return out


def _build_vector_assign(c):
    key = (c.id,)
    n, dt = c.p["n"], c.p["dt"]
    B = _result(w=obj(dt, (n,), key + ("w",), 0.6))
    B.I = index_named(c.p["I"], n, key + ("I",))
    m = n if B.I is None else B.I.size
    B.u = obj(c.get("udt", dt), (m,), key + ("u",), kind=c.p["u"])
    alias = c.get("alias")
    B.M = {"M=w": B.w, "M=u": B.u}.get(alias) or mask_obj((n,), key)
    B.want, B.want_dt = dm.assign_vec(B.w, B.u, B.I, **wb_kw(c.p["wb"], B.M)), dt
    return B


# ---- scalar and object assign into a matrix
def _matrix_assign_cases():
    out = []
    add = lambda **p: out.append(Case("matrix_assign", **p))
    lists = (("dup", "dup"), ("all", "dup"), ("unsorted", "all"), ("empty", "dup"), ("dup", "empty"), ("all", "all"))
    for C in ("small", "low"):  # low: at most 64 rows, the column-word format's domain
        for I, J in lists:
            for wb in WB_ALL if (C, I, J) in (("small", "dup", "dup"), ("small", "all", "all")) else \
                    (WB_PLAIN, ("V", True, None), ("~S", False, "plus")):
                add(C=C, dt="INT64", value="scalar", I=I, J=J, wb=wb)
                add(C=C, dt="INT64", value="scalar", I=I, J=J, wb=wb, x=None)
    for dt in dm.ALL:
        add(C="small", dt=dt, value="scalar", I="dup", J="unsorted", wb=("V", False, None))
        add(C="small", dt=dt, value="scalar", I="all", J="all", wb=("~S", True, None))
    for value in ("A", "A.T"):
        for wb in WB_ALL:
            add(C="small", dt="INT64", value=value, I="all", J="all", wb=wb)
        add(C="small", dt="INT8", adt="FP64", value=value, I="all", J="all", wb=("V", False, "plus"))
        add(C="small", dt="BOOL", adt="INT64", value=value, I="all", J="all", wb=WB_PLAIN)
        add(C="low", dt="INT32", value=value, I="all", J="all", wb=("S", True, None))
    return out


def _build_matrix_assign(c):
    key = (c.id,)
    dt = c.p["dt"]
    B = _result(C=matrix_named(c.p["C"], dt))
    shape = B.C[0].shape
    B.I = index_named(c.p["I"], shape[0], key + ("I",))
    B.J = index_named(c.p["J"], shape[1], key + ("J",))
    B.M = mask_obj(shape, key)
    if c.p["value"] == "scalar":
        B.x, B.xdt = _scalar_of(c, key)
        value = B.x
    else:
        value = obj(c.get("adt", dt), shape, key + ("A",), 0.3)
        B.A = dm.transpose(value) if c.p["value"] == "A.T" else value  # what the device is given
    B.want, B.want_dt = dm.assign(B.C, value, B.I, B.J, **wb_kw(c.p["wb"], B.M)), dt
    return B


_TABLES = {"matrix_extract": (_matrix_extract_cases, _build_matrix_extract),
           "col_extract": (_col_extract_cases, _build_col_extract),
           "vector_extract": (_vector_extract_cases, _build_vector_extract),
           "vector_assign_scalar": (_vector_assign_scalar_cases, _build_vector_assign_scalar),
           "vector_assign": (_vector_assign_cases, _build_vector_assign),
           "matrix_assign": (_matrix_assign_cases, _build_matrix_assign)}
OPS = tuple(_TABLES)
CASE_COUNT = 2230  # all tables together, pinned so that a lost loop is noticed
_CASES = {}


def cases(op):
    if op not in _CASES:
        # the loops above overlap here and there: a case named twice runs once
        _CASES[op] = list({c.id: c for c in _TABLES[op][0]()}.values())
    return _CASES[op]


def build(c):
    """the model inputs of a case and the expected result: .want (present, values), .want_dt"""
    B = _TABLES[c.op][1](c)
    assert B.want[1].dtype == dm.NP[B.want_dt], c.id
    return B


def assert_coverage():
    """what the issue lists, per operation: every type, every mask kind (with and without replace
    and accumulator) and every size"""
    for op in OPS:
        cs = cases(op)
        assert {c.p["dt"] for c in cs} == set(dm.ALL), op
        wbs = {c.p["wb"] for c in cs if c.get("wb")}
        assert {w[0] for w in wbs} == set(MASK_KINDS), op
        for kind in MASK_KINDS[1:]:
            assert {(kind, r, a) for r in (False, True) for a in (None, "plus")} <= wbs, (op, kind)
    mx = cases("matrix_extract")
    assert {c.p["J"] for c in mx} >= {"all", "unsorted", "rev", "dup", "rep200", "one", "empty"}
    assert {c.p["I"] for c in mx} >= {"all", "dup", "rep100", "one", "empty", "prefix133125", "prefix131071"}
    assert {c.get("alias") for c in mx} >= {"C=A", "M=C", "M=A"} and any(c.get("tran") for c in mx)
    assert {c.get("scan_u8") for c in mx if c.p["A"] == "tall"} == {None, 1}
    assert {c.get("ctype") for c in mx} >= {"INT8", "BOOL"} and any(c.get("kind") == "iso" for c in mx)
    ce = cases("col_extract")
    for orient in ("col", "row"):
        sub = [c for c in ce if c.p["orient"] == orient]
        assert {(c.p["j"], c.p["I"]) for c in sub} >= set(itertools.product(range(4), COL_I)), orient
        assert {c.p["dt"] for c in sub} == set(dm.ALL) and any(c.get("kind") == "iso" for c in sub)
    ve = cases("vector_extract")
    assert {(c.p["n"], c.p["kind"], c.p["I"]) for c in ve} >= set(itertools.product(VEC_SIZES, VEC_KINDS,
                                                                                   ("all", "rev", "dup")))
    assert {c.p["I"] for c in ve} >= {"len1", "len64", "len65", "len70001"} and any(c.get("alias") for c in ve)
    vs = cases("vector_assign_scalar")
    assert {c.p["n"] for c in vs} == set(ASSIGN_SIZES)
    for n in ASSIGN_SIZES[:10]:
        sub = [c for c in vs if c.p["n"] == n]
        assert {(c.p["mask"], c.p["wb"][0], c.p["wb"][1]) for c in sub} >= set(
            itertools.product(ASSIGN_MASKS, MASK_KINDS[1:], (False, True))), n
        assert {c.p["w"] for c in sub} == set(W_KINDS), n
    assert {(c.p["w"], c.p["mask"]) for c in vs if c.p["n"] == 65} >= set(
        itertools.product(W_KINDS, ("none", "sparse", "iso_true", "alias")))
    assert sum(c.p["n"] == ASSIGN_STRIDE_N for c in vs) == 3
    assert {c.p["wb"][2] for c in vs} == {None, "plus", "min"}
    assert any("x" in c.p and c.p["x"] is None for c in vs) and any(c.get("xdt") for c in vs)
    va = cases("vector_assign")
    assert {(c.p["n"], c.p["I"], c.p["u"]) for c in va} >= set(itertools.product(
        VEC_SIZES, ("sorted", "revsorted", "unsorted", "empty", "all"), ("empty", "sparse", "full", "iso")))
    assert {c.p["wb"] for c in va} >= set(WB_ASSIGN) and {c.get("alias") for c in va} >= {"M=w", "M=u"}
    assert any(c.get("udt") for c in va)
    ma = cases("matrix_assign")
    assert {c.p["C"] for c in ma} == {"small", "low"} and {c.p["value"] for c in ma} == {"scalar", "A", "A.T"}
    assert any("x" in c.p for c in ma) and any(c.get("adt") for c in ma)
