"""The probe objects, probes and mutators of test_derived_state_gpu.py (no GPU needed to import).

A matrix carries, next to its CSR, structures derived from it that the hot kernels read instead
(csrc/gb_internal.h: the cached CSC and its position map, the column-word form, and per
orientation the hub table, the non-empty-row bitmap with its ranks, the pull heads, the long-row
table, the hot-column relabel and the narrow values); a vector carries host-side beliefs about
its device state (count, mailbox, hint, iso).  Each is right only while every writer of the
object drops or updates it.  A *probe* runs one consumer of one such structure and returns
(result, expected), the expectation from the dense numpy model (dense_model.py); a *mutator*
changes the device object and its model the same way.  READS maps every derived field to the
probe that reads it; test_derived_state_cases.py checks the table against the header.

Models are `Model` objects: `pv` is the (present, values) pair of dense_model.py, `dtype` the
GraphBLAS type name, `iso` whether the device object is built from one value.  Every value is a
small integer, so every plus_times / min_plus result is exact and compared bit for bit.
"""
import contextlib
import ctypes

import numpy as np

import dense_model as dm

N = 700            # eleven bitmap words, the last one a tail of 60 rows
N_SMALL = 650      # the same word count: the pools keyed by word count are shared with N
SRC = 2            # BFS source of every loop
HUB = 300          # the row with more than 128 entries
HUB_DEG = 140
EMPTY_ROWS = (0, 63, 64, 127)  # and n - 1, and the whole word EMPTY_WORD
EMPTY_WORD = 5     # rows 320..383
SPMV_LONG = 128    # csrc/gb_mxv.hip: rows longer than this go to the long-row table
PUSH_HEAVY = 8     # the hubs probe's push_heavy


class Model:
    def __init__(self, pv, dtype, iso=False):
        self.pv = (np.array(pv[0], bool), np.array(pv[1], dm.NP[dtype]))
        self.dtype = dtype
        self.iso = iso

    @property
    def shape(self):
        return self.pv[0].shape

    def copy(self):
        return Model(self.pv, self.dtype, self.iso)

    def coo(self):
        r, c, v = dm.to_coo(self.pv)
        return r.astype(np.int64), c.astype(np.int64), v


# ---------------------------------------------------------------------- the probe objects
def graph(n=N, seed=1, hub=HUB, empty_word=EMPTY_WORD):
    """structure of a symmetric graph on n vertices: a chain over the vertices that have entries
    (each joined to the next one and the next but one: rows of 4, of 2 and 3 at the ends), a few
    chain links cut (rows of 3), a hub joined to HUB_DEG seeded vertices (theirs grow to 5).
    Rows 0, 63, 64, 127, n - 1 and one whole 64-row word have no entry."""
    rng = np.random.default_rng(seed)
    dead = np.zeros(n, bool)
    dead[list(EMPTY_ROWS) + [n - 1]] = True
    dead[64 * empty_word:64 * (empty_word + 1)] = True
    live = np.flatnonzero(~dead)
    p = np.zeros((n, n), bool)
    for k in (1, 2):
        p[live[:-k], live[k:]] = True
    cut = live[40:-40:45]  # links to the next vertex, far from the ends
    nxt = live[np.searchsorted(live, cut) + 1]
    p[cut, nxt] = False
    others = live[(live != hub) & (np.abs(live - hub) > 2)]
    p[hub, rng.choice(others, HUB_DEG - 4, replace=False)] = True
    p |= p.T
    assert not p.diagonal().any()
    return p


def _values(p, dtype, lo, hi, seed):
    rng = np.random.default_rng(seed)
    v = np.zeros(p.shape, dm.NP[dtype])
    v[p] = rng.integers(lo, hi + 1, int(p.sum())).astype(dm.NP[dtype])
    return v


def make(name):
    """a fresh Model of the probe object `name`"""
    if name in ("G", "G2", "Gs", "G2s"):
        n = N_SMALL if name.endswith("s") else N
        p = graph(n, 1, HUB, EMPTY_WORD) if name[:2] != "G2" else graph(n, 2, 200, 7)
        return Model((p, p.copy()), "BOOL", iso=True)
    p = graph()
    if name == "Gi":  # INT64 iso copy
        return Model((p, p.astype(np.int64)), "INT64", iso=True)
    if name == "W":   # 1..255: the narrow copy is 1 byte unsigned
        return Model((p, _values(p, "INT64", 1, 255, 3)), "INT64")
    if name == "Wu":  # -100..100: 1 byte signed
        return Model((p, _values(p, "INT64", -100, 100, 4)), "INT64")
    if name == "F":   # small integers in FP64: every plus_times sum is exact
        return Model((p, _values(p, "FP64", 1, 4, 5)), "FP64")
    raise KeyError(name)


def to_gb(gb, m):
    r, c, v = m.coo()
    nr, nc = m.shape
    if m.iso and len(v):
        return gb.Matrix.from_coo(r, c, v[0].item(), dtype=m.dtype, nrows=nr, ncols=nc)
    return gb.Matrix.from_coo(r, c, v, dtype=m.dtype, nrows=nr, ncols=nc)


def coo(A):
    r, c, v = A.to_coo()
    return r.astype(np.int64), c.astype(np.int64), np.asarray(v)


def vec_coo(w):
    i, v = w.to_coo()
    return i.astype(np.int64), np.asarray(v)


def model_vec_coo(u):
    i, v = dm.to_coo(u)
    return i.astype(np.int64), v


def same(got, exp):
    """bit-exact comparison of two (nested) tuples of arrays or ints: None, or what differs"""
    if isinstance(exp, (tuple, list)):
        if not isinstance(got, (tuple, list)) or len(got) != len(exp):
            return f"length {len(got) if isinstance(got, (tuple, list)) else got} != {len(exp)}"
        for k, (g, e) in enumerate(zip(got, exp)):
            d = same(g, e)
            if d:
                return f"[{k}] {d}"
        return None
    g, e = np.asarray(got), np.asarray(exp)
    if g.shape != e.shape:
        return f"shape {g.shape} != {e.shape}"
    if g.dtype != e.dtype:
        return f"dtype {g.dtype} != {e.dtype}"
    if not np.array_equal(g, e):
        bad = np.flatnonzero(g.ravel() != e.ravel())
        return f"{bad.size} of {g.size} differ, first at {bad[0]}: {g.ravel()[bad[0]]} != {e.ravel()[bad[0]]}"
    return None


@contextlib.contextmanager
def knobs(gb, **kw):
    for k, v in kw.items():
        gb.set_knob(k, v)
    try:
        yield
    finally:
        for k in kw:
            gb.set_knob(k, 0)


# ---------------------------------------------------------------------- the probes
def ref_bfs(p, src):
    """numpy restatement of the level loop on the structure p: (levels, nvals(q) per level)"""
    n = p.shape[0]
    v = np.zeros(n, np.int32)
    q = np.zeros(n, bool)
    q[src] = True
    counts, d = [], 0
    while True:
        d += 1
        v[q] = d
        q = p[q].any(axis=0) & (v == 0)
        counts.append(int(q.sum()))
        if not counts[-1]:
            return v, counts


def gpu_bfs(gb, A, src, q=None, v=None):
    """the notebook loop of test_pull_compact.py; q and v may be vectors to reuse (cleared here)"""
    n = A.nrows
    v = gb.Vector(gb.INT32, n) if v is None else v
    q = gb.Vector(bool, n) if q is None else q
    v.clear()
    q.clear()
    q[int(src)] = True
    counts, d = [], 0
    while True:
        d += 1
        v(mask=q.V)[:] = d
        q(~v.S, replace=True) << q.vxm(A, gb.semiring.any_pair)
        counts.append(int(q.nvals))
        if not counts[-1]:
            break
    got = np.zeros(n, np.int32)
    i, x = v.to_coo()
    got[i.astype(np.int64)] = x
    return got, counts


def _sparse_u(m, dtype):
    """a sparse non-iso vector over the columns of m: every 7th position from 3, values 1..3"""
    n = m.shape[1]
    p = np.zeros(n, bool)
    p[3::7] = True
    v = np.where(p, np.arange(n) % 3 + 1, 0).astype(dm.NP[dtype])
    return p, v


def _full_u(m, dtype):
    n = m.shape[1]
    return np.ones(n, bool), (np.arange(n) % 5 + 1).astype(dm.NP[dtype])


def _gb_vec(gb, u, dtype):
    i, v = model_vec_coo(u)
    return gb.Vector.from_coo(i, v, dtype=dtype, size=len(u[0]))


def _plus(m):
    """the plus monoid, lor for BOOL (which has no plus_times / plus_pair)"""
    return "lor" if m.dtype == "BOOL" else "plus"


def _times(m):
    return "land" if m.dtype == "BOOL" else "times"


def probe_csc(gb, A, m):
    """t_rowptr / t_colidx / t_vals: the transpose itself, and u A with a sparse u"""
    T = A.T.new()
    u = _sparse_u(Model(dm.transpose(m.pv), m.dtype), m.dtype)
    w = _gb_vec(gb, u, m.dtype).vxm(A, getattr(gb.semiring, f"{_plus(m)}_{_times(m)}")).new()
    exp_w = dm.vxm(_plus(m), _times(m), m.dtype, u, m.pv)
    return (coo(T), vec_coo(w)), (dm.to_coo(dm.transpose(m.pv)), model_vec_coo(exp_w))


def probe_csc_perm(gb, A, m):
    """t_perm: A as the structural mask of the two-sided dot"""
    nr = m.shape[0]
    with knobs(gb, mxm_method=1):
        C = gb.Matrix(m.dtype, nr, nr)
        C(A.S) << A.mxm(A.T, getattr(gb.semiring, f"{_plus(m)}_pair"))
    T = dm.mxm(_plus(m), "pair", m.dtype, m.pv, m.pv, tran1=True)
    zero = (np.zeros((nr, nr), bool), np.zeros((nr, nr), T[1].dtype))
    exp = dm.write_back(zero, T, mask=m.pv, mask_struct=True)
    return coo(C), dm.to_coo(exp)


def _loops(gb, A, m, settings):
    got, exp = [], []
    ref = ref_bfs(m.pv[0], SRC)
    for kw in settings:
        with knobs(gb, **kw):
            lev, counts = gpu_bfs(gb, A, SRC)
        got.append((lev, np.asarray(counts)))
        exp.append((ref[0], np.asarray(ref[1])))
    return tuple(got), tuple(exp)


def probe_heads(gb, A, m):
    """rows_ne / ne_rank / phead / pdeg: every level pulls through the heads, packed and per step"""
    return _loops(gb, A, m, [dict(spmv_direction=1, iso_pack=0), dict(spmv_direction=1, iso_pack=1)])


def probe_hubs(gb, A, m):
    """hub_tab / hub_n / hub_H / maxdeg: every level pushes through the hub table, then the
    default direction, whose host-side choice reads maxdeg"""
    got, exp = _loops(gb, A, m, [dict(spmv_direction=2, push_heavy=PUSH_HEAVY),
                                 dict(spmv_direction=0, push_heavy=PUSH_HEAVY)])
    # one level from a frontier the host built (no root, no hint from a previous level) under an
    # empty complemented mask: the direction is decided on the host from nvals(q) * maxdeg
    n = m.shape[0]
    front = np.zeros(n, bool)
    front[[SRC, SRC + 1]] = True
    q = gb.Vector.from_coo(np.flatnonzero(front), True, dtype=bool, size=n)
    v = gb.Vector(gb.INT32, n)
    assert q.nvals == 2 and v.nvals == 0
    with knobs(gb, push_heavy=PUSH_HEAVY):
        w = gb.Vector(bool, n)
        w(~v.S, replace=True) << q.vxm(A, gb.semiring.any_pair)
    nxt = m.pv[0][front].any(axis=0)
    return got + (vec_coo(w),), exp + ((np.flatnonzero(nxt), np.ones(int(nxt.sum()), bool)),)


def _mxv(gb, A, m, u, **kw):
    x = _gb_vec(gb, u, m.dtype)
    assert x.nvals == int(u[0].sum())  # the host now knows the count: `full` is decided from it
    with knobs(gb, **kw):
        w = gb.Vector(m.dtype, m.shape[0])
        w << A.mxv(x, gb.semiring.plus_times)
    return vec_coo(w), model_vec_coo(dm.mxv("plus", "times", m.dtype, m.pv, u))


def probe_long(gb, A, m):
    """long_tab / long_n: the general SpMV with a sparse non-iso input"""
    return _mxv(gb, A, m, _sparse_u(m, m.dtype))


def probe_hot(gb, A, m):
    """hot_ci / hot_cols / hot_n: the general SpMV with a full non-iso input, relabel forced"""
    return _mxv(gb, A, m, _full_u(m, m.dtype), xhot=2, xhot_cols=16)


def mask_model(shape, seed=9):
    rng = np.random.default_rng(seed)
    p = rng.random(shape) < 0.02
    p[HUB % shape[0], :] = True  # the hub row's dots: long row against every row
    return p, p.copy()


def probe_narrow(gb, A, m):
    """nar_vx / nar_k / nar_done: the masked min_plus dot reads one narrow value per hit"""
    nr = m.shape[0]
    M = mask_model((nr, nr))
    Mg = to_gb(gb, Model(M, "BOOL", iso=True))
    with knobs(gb, mxm_method=1):
        C = gb.Matrix(m.dtype, nr, nr)
        C(Mg.S) << A.mxm(A.T, gb.semiring.min_plus)
    T = dm.mxm("min", "plus", m.dtype, m.pv, m.pv, tran1=True)
    zero = (np.zeros((nr, nr), bool), np.zeros((nr, nr), T[1].dtype))
    return coo(C), dm.to_coo(dm.write_back(zero, T, mask=M, mask_struct=True))


CW_ROWS = 13
CW_HUB = 64  # colbits_hub of the probe: below G's longest row (the default, 512, is above)


def frontier_model(n):
    """13 frontiers that cover every vertex: vertex k is in frontier k mod 13, so every row of
    the graph -- the hub's too, whichever row that is after a mutation -- bears on the result"""
    p = np.zeros((CW_ROWS, n), bool)
    p[np.arange(n) % CW_ROWS, np.arange(n)] = True
    return p, p.copy()


def probe_colwords(gb, A, m):
    """the hub tables read by the column-word mxm (gb_colbits_mxm), and cw / cw_vals / cw_stat of
    its result: 13 frontiers at once, Q = Q0 any.pair A, in the direction the device chooses
    (both tables are built), then pull only and push only"""
    Q0m = frontier_model(m.shape[0])
    T = dm.mxm("any", "pair", "BOOL", Q0m, (m.pv[0], m.pv[0].copy()))
    r, c, _ = dm.to_coo(T)
    got, exp = [], []
    for direction in (0, 1, 2):
        Q0 = to_gb(gb, Model(Q0m, "BOOL", iso=True))
        with knobs(gb, colbits=1, colbits_hub=CW_HUB, colbits_direction=direction):  # the hub row is a hub of both tables
            Q = gb.Matrix(bool, CW_ROWS, m.shape[1])
            Q << Q0.mxm(A, gb.semiring.any_pair)
            nvals = int(Q.nvals)  # read from the column-word form's own count
        gr, gc, gv = coo(Q)
        got.append((gr, gc, gv.astype(bool), nvals))
        exp.append((r, c, np.ones(len(r), bool), len(r)))
    return tuple(got), tuple(exp)


class Probe:
    def __init__(self, name, fn, counters, bases):
        self.name, self.fn, self.counters, self.bases = name, fn, counters, bases

    def ok_for(self, m):
        """the probe's preconditions on a (mutated) model"""
        nr, nc = m.shape
        if nr != nc or nr < 128 or m.dtype not in self.types():
            return False
        if self.name in ("heads", "hubs"):
            return m.pv[0][SRC].any()  # the source has out-edges: more than one level
        if self.name in ("long", "hot", "narrow"):
            return m.pv[0].any()
        return True

    def types(self):
        return {make(b).dtype for b in self.bases}


ANY = ("G", "W", "F", "Gi", "Wu", "G2", "Gs", "G2s")
# counters: name -> rise on a fresh object (what the first run builds); the first one is the
# probe's own, asserted after every mutation
PROBES = {p.name: p for p in [
    Probe("csc", probe_csc, {"transposes_cached": 1}, ANY),
    Probe("csc_perm", probe_csc_perm, {"csc_perms_built": 1, "transposes_cached": 1}, ANY),
    # the pull of u A runs along A's columns: the CSC, its bitmap and ranks, its heads
    Probe("heads", probe_heads, {"pull_heads_built": 1, "nonempty_built": 1, "transposes_cached": 1}, ANY),
    # the push runs along A's rows; the pull it may fall back to needs the CSC side too
    Probe("hubs", probe_hubs, {"hub_tables_built": 1}, ANY),
    Probe("long", probe_long, {"long_tables_built": 1, "nonempty_built": 1}, ("F", "W", "Wu", "Gi")),
    Probe("hot", probe_hot, {"hot_relabels_built": 1, "nonempty_built": 1}, ("F", "W", "Wu", "Gi")),
    Probe("narrow", probe_narrow, {"narrow_built": 1}, ("W", "Wu")),
    # pull rows (CSC side) and push rows (CSR side): one hub table each
    Probe("colwords", probe_colwords, {"hub_tables_built": 2, "transposes_cached": 1}, ("G", "G2", "Gs", "G2s")),
]}

# every derived field of csrc/gb_internal.h -> the probe that reads it
READS = {
    "t_valid": "csc", "t_rowptr": "csc", "t_colidx": "csc", "t_vals": "csc",
    "t_perm": "csc_perm",
    "cw": "colwords", "cw_vals": "colwords", "cw_stat": "colwords",
    "hub_tab": "hubs", "hub_n": "hubs", "hub_H": "hubs", "maxdeg": "hubs",
    "rows_ne": "heads", "ne_rank": "heads", "phead": "heads", "pdeg": "heads",
    "long_tab": "long", "long_n": "long",
    "hot_ci": "hot", "hot_cols": "hot", "hot_n": "hot",
    "nar_vx": "narrow", "nar_k": "narrow", "nar_done": "narrow",
    # the vector-side beliefs: the vector consumers of test_derived_state_gpu.py
    "nvals_valid": "vector", "pub": "vector", "pub_seq": "vector", "pub_epoch": "vector",
    "hint_valid": "vector", "hint_key": "vector", "d_nvals": "vector",
}
COUNTERS = ("hub_tables_built", "nonempty_built", "pull_heads_built", "long_tables_built",
            "hot_relabels_built", "narrow_built", "csc_perms_built")  # new in csrc; + transposes_cached


def counters(gb):
    return {c: gb.get_knob("stat_" + c) for c in COUNTERS + ("transposes_cached",)}


# ---------------------------------------------------------------------- the mutators
def _first_entry(m, row):
    return int(np.flatnonzero(m.pv[0][row])[0])


def _val(m, x):
    return dm.NP[m.dtype](x)


def _set(A, m, i, j, x):
    A[i, j] = _val(m, x).item()
    m.pv = dm.set_element(m.pv, (i, j), _val(m, x))


def _del(A, m, i, j):
    del A[i, j]
    m.pv = dm.remove_element(m.pv, (i, j))


def mut_set_row64(gb, A, m):
    """an entry into the empty row 64 (and its mirror): every later rank shifts"""
    far = m.shape[0] - 3
    _set(A, m, 64, far, 1)
    _set(A, m, far, 64, 1)


def mut_set_row0(gb, A, m):
    """an entry into the empty row 0 (and its mirror): all ranks shift"""
    far = m.shape[0] - 3
    _set(A, m, 0, far, 1)
    _set(A, m, far, 0, 1)


def mut_overwrite_wide(gb, A, m):
    """an existing value becomes 70000: the narrow copy no longer fits one or two bytes"""
    _set(A, m, HUB, _first_entry(m, HUB), 70000)


def mut_overwrite_negative(gb, A, m):
    """an existing value becomes -3: the narrow copy turns signed"""
    _set(A, m, HUB, _first_entry(m, HUB), -3)


def mut_set_same_iso(gb, A, m):
    """an existing entry of an iso matrix set to the iso value: no change, stays iso"""
    _set(A, m, HUB, _first_entry(m, HUB), m.pv[1][HUB, _first_entry(m, HUB)])


def mut_set_other_iso(gb, A, m):
    """an existing entry of an INT iso matrix set to another value: no longer iso"""
    _set(A, m, HUB, _first_entry(m, HUB), 9)
    m.iso = False


def mut_remove_row(gb, A, m):
    """removeElement until row 1 is empty (and its mirror entries)"""
    for j in np.flatnonzero(m.pv[0][1]):
        _del(A, m, 1, int(j))
        _del(A, m, int(j), 1)


def mut_remove_hub(gb, A, m):
    """removeElement from the hub row down to exactly SPMV_LONG entries"""
    cols = np.flatnonzero(m.pv[0][HUB])
    for j in cols[SPMV_LONG:]:
        _del(A, m, HUB, int(j))


def mut_remove_absent(gb, A, m):
    """removeElement of an entry that is not there: no change"""
    assert not m.pv[0][HUB, 0]
    _del(A, m, HUB, 0)


def mut_clear_build(gb, A, m):
    """clear(), then build of another graph's structure with the same values rule"""
    p = graph(m.shape[0], 7, 400, 2)
    v = np.where(p, (np.add.outer(np.arange(p.shape[0]), np.arange(p.shape[1])) % 7 + 1), 0)
    new = Model((p, v.astype(dm.NP[m.dtype]) if m.dtype != "BOOL" else p), m.dtype)
    r, c, x = new.coo()
    A.clear()
    A.build(r, c, x)
    m.pv, m.iso = new.pv, False


def mut_resize_shrink_grow(gb, A, m):
    """resize to 650 x 650 and back: the entries past 650 are gone"""
    n = m.shape[0]
    for k in (n - 50, n):
        A.resize(k, k)
        m.pv = dm.resize(m.pv, (k, k))


def mut_resize_cols(gb, A, m):
    """resize of the columns only, to 650 and back"""
    n = m.shape[0]
    for k in (n - 50, n):
        A.resize(n, k)
        m.pv = dm.resize(m.pv, (n, k))


def mut_reshape_roundtrip(gb, A, m):
    """in-place reshape to n/2 x 2n and back: the same matrix, through two new CSRs"""
    n = m.shape[0]
    A.ss.reshape(n // 2, 2 * n, inplace=True)
    A.ss.reshape(n, n, inplace=True)


def prep_asymmetric(m):
    """the probe object with the entry (64, n - 3) and no mirror of it, before it is built and
    probed: its transpose differs from it, and the write-backs below meet every cache live"""
    m.pv = dm.set_element(m.pv, (64, m.shape[0] - 3), m.pv[1][m.pv[0]][0])


def mut_transpose_self(gb, A, m):
    """A << A.T of an asymmetric matrix (prep_asymmetric): nothing else touches A"""
    assert not np.array_equal(m.pv[0], m.pv[0].T)
    A << A.T
    m.pv = dm.transpose(m.pv)


def mut_ewise_add_self(gb, A, m):
    """A << A.ewise_add(A.T, lor / plus) of an asymmetric matrix: the whole-object install"""
    assert not np.array_equal(m.pv[0], m.pv[0].T)
    op = "lor" if m.dtype == "BOOL" else "plus"
    A << A.ewise_add(A.T, getattr(gb.binary, op))
    m.pv = dm.ewise("add", op, m.dtype, m.pv, dm.transpose(m.pv))
    m.iso = False


def _other(gb, m, seed=11):
    """a second operand of A's shape and type: sparse, touching the empty rows"""
    rng = np.random.default_rng(seed)
    p = rng.random(m.shape) < 0.004
    p[64, :] = False
    p[64, 5:9] = True
    p[0, 100:103] = True
    v = np.where(p, rng.integers(1, 4, m.shape), 0).astype(dm.NP[m.dtype])
    B = Model((p, v), m.dtype)
    return to_gb(gb, B), B


def _mask(gb, m, seed=12):
    rng = np.random.default_rng(seed)
    p = rng.random(m.shape) < 0.3
    p[:130, :] = True
    M = Model((p, p.copy()), "BOOL", iso=True)
    return to_gb(gb, M), M


def mut_masked_write(gb, A, m):
    """A(M.S) << B: the merge branch of the write-back"""
    (B, Bm), (M, Mm) = _other(gb, m), _mask(gb, m)
    A(M.S) << B
    m.pv = dm.write_back(m.pv, Bm.pv, mask=Mm.pv, mask_struct=True)
    m.iso = False


def mut_accum_write(gb, A, m):
    """A(accum=plus) << B"""
    B, Bm = _other(gb, m)
    op = "lor" if m.dtype == "BOOL" else "plus"
    A(getattr(gb.binary, op)) << B
    m.pv = dm.write_back(m.pv, Bm.pv, accum=op)
    m.iso = False


def mut_masked_replace(gb, A, m):
    """A(M.S, replace=True) << B"""
    (B, Bm), (M, Mm) = _other(gb, m), _mask(gb, m)
    p = Bm.pv[0] | (m.pv[0] & (np.arange(m.shape[0]) % 2 == 0)[:, None])  # keep half of A's rows
    Bm = Model((p, np.where(p, np.where(Bm.pv[0], Bm.pv[1], m.pv[1]), 0)), m.dtype)
    B = to_gb(gb, Bm)
    A(M.S, replace=True) << B
    m.pv = dm.write_back(m.pv, Bm.pv, mask=Mm.pv, mask_struct=True, replace=True)
    m.iso = False


REGION_I = np.array([64, 0, 5, 300, 640])
REGION_J = np.array([7, 64, 129, 500])


def mut_assign_scalar(gb, A, m):
    """A[I, J] << s"""
    A[REGION_I, REGION_J] << _val(m, 2).item()
    m.pv = dm.assign(m.pv, _val(m, 2), REGION_I, REGION_J)
    m.iso = False


def mut_assign_matrix(gb, A, m):
    """A[I, J] << B"""
    rng = np.random.default_rng(13)
    p = rng.random((len(REGION_I), len(REGION_J))) < 0.6
    Bm = Model((p, np.where(p, 3, 0)), m.dtype)
    A[REGION_I, REGION_J] << to_gb(gb, Bm)
    m.pv = dm.assign(m.pv, Bm.pv, REGION_I, REGION_J)
    m.iso = False


def _line(gb, m):
    n = m.shape[0]
    p = np.zeros(n, bool)
    p[10::50] = True
    u = p, np.where(p, 2, 0).astype(dm.NP[m.dtype])
    return _gb_vec(gb, u, m.dtype), u


def mut_assign_row(gb, A, m):
    """A[i, :] << v into the empty row 64"""
    v, u = _line(gb, m)
    A[64, :] << v
    m.pv = dm.assign(m.pv, (u[0][None, :], u[1][None, :]), [64], None)
    m.iso = False


def mut_assign_col(gb, A, m):
    """A[:, j] << v into the empty column 64"""
    v, u = _line(gb, m)
    A[:, 64] << v
    m.pv = dm.assign(m.pv, (u[0][:, None], u[1][:, None]), None, [64])
    m.iso = False


def _asymmetric(gb, m):
    """a used operand B that differs from A: A's model with row 64 filled"""
    Bm = m.copy()
    Bm.pv = dm.set_element(Bm.pv, (64, m.shape[0] - 3), _val(m, 1))
    Bm.iso = False
    return to_gb(gb, Bm), Bm


def mut_select_into(gb, A, m):
    """A << B.select("tril", -1): A, an input so far, becomes the output"""
    B, Bm = _asymmetric(gb, m)
    A << B.select("tril", -1)
    keep = np.tril(Bm.pv[0], -1)
    m.pv = (keep, np.where(keep, Bm.pv[1], 0).astype(dm.NP[m.dtype]))
    m.iso = False


def mut_apply_index_into(gb, A, m):
    """A << B.apply("rowindex", 1): the row index + 1 of every entry, cast to A's type"""
    B, Bm = _asymmetric(gb, m)
    A << B.apply("rowindex", 1)
    p = Bm.pv[0]
    rows = np.broadcast_to(np.arange(p.shape[0], dtype=np.int64)[:, None] + 1, p.shape)
    m.pv = (p.copy(), np.where(p, dm.cast(rows, m.dtype), 0).astype(dm.NP[m.dtype]))
    m.iso = False


def mut_concat_into(gb, A, m):
    """A.ss.concat of four tiles of a used operand, the two tile columns swapped"""
    B, Bm = _asymmetric(gb, m)
    n = m.shape[0]
    h = 320
    (t00, t01), (t10, t11) = B.ss.split([[h, n - h], [n - h, h]])
    bp, bv = Bm.pv
    tiles_p = [[bp[:h, n - h:], bp[:h, :n - h]], [bp[h:, n - h:], bp[h:, :n - h]]]
    tiles_v = [[bv[:h, n - h:], bv[:h, :n - h]], [bv[h:, n - h:], bv[h:, :n - h]]]
    A.ss.concat([[t01, t00], [t11, t10]])
    m.pv = (np.block(tiles_p), np.block(tiles_v))
    m.iso = False


def mut_kronecker_into(gb, A, m):
    """A << K.kronecker(L): 7 x 7 (x) n/7 x n/7"""
    n = m.shape[0]
    assert n % 7 == 0
    b = n // 7
    rng = np.random.default_rng(14)
    kp = rng.random((7, 7)) < 0.4
    lp = rng.random((b, b)) < 0.05
    Km = Model((kp, np.where(kp, 2, 0)), m.dtype)
    Lm = Model((lp, np.where(lp, rng.integers(1, 4, (b, b)), 0)), m.dtype)
    op = "land" if m.dtype == "BOOL" else "times"
    A << to_gb(gb, Km).kronecker(to_gb(gb, Lm), getattr(gb.binary, op))
    p = np.kron(kp, lp)
    v = np.kron(Km.pv[1], Lm.pv[1]) if m.dtype != "BOOL" else p
    m.pv = (p, np.where(p, v, 0).astype(dm.NP[m.dtype]))
    m.iso = False


def mut_diag_into(gb, A, m):
    """A.ss.build_diag(v, 1): a vector on the first superdiagonal"""
    n = m.shape[0]
    p = np.ones(n - 1, bool)
    p[::9] = False
    u = p, np.where(p, np.arange(n - 1) % 4 + 1, 0).astype(dm.NP[m.dtype])
    A.ss.build_diag(_gb_vec(gb, u, m.dtype), 1)
    P, V = np.zeros(m.shape, bool), np.zeros(m.shape, dm.NP[m.dtype])
    i = np.arange(n - 1)
    P[i, i + 1], V[i, i + 1] = u[0], u[1]
    m.pv = (P, V)
    m.iso = False


def mut_union_into(gb, A, m):
    """A << A.ewise_union(B, plus / lor, 1, 1)"""
    import union_model as um

    B, Bm = _other(gb, m)
    op = "lor" if m.dtype == "BOOL" else "plus"
    A << A.ewise_union(B, getattr(gb.binary, op), _val(m, 1).item(), _val(m, 1).item())
    m.pv = um.ewise_union(op, m.dtype, m.pv, _val(m, 1), Bm.pv, _val(m, 1))
    m.iso = False


def mut_sort_into(gb, A, m):
    """GxB_Matrix_sort of a used operand's rows into A (the low-level call: ss.sort makes new outputs)"""
    import sort_model as som

    B, Bm = _asymmetric(gb, m)
    op = gb.ss._sort_op(B, gb.binary.lt)
    gb.base.call("GxB_Matrix_sort", [A, None, op, B, gb.base.descriptor_lookup(transpose_first=False)])
    m.pv = som.sort_matrix(Bm.pv, "lt")[0]
    m.iso = False


class Mutator:
    """prepare: applied to the model before the object is built (and first probed)"""

    def __init__(self, fn, bases=ANY, rebuilds=True, changes=True, prepare=None):
        self.name = fn.__name__[4:]
        self.fn, self.bases, self.rebuilds, self.changes, self.prepare = fn, bases, rebuilds, changes, prepare


MUTATORS = {x.name: x for x in [
    Mutator(mut_set_row64),
    Mutator(mut_set_row0),
    Mutator(mut_overwrite_wide, ("W", "Wu")),
    Mutator(mut_overwrite_negative, ("W",)),
    Mutator(mut_set_same_iso, ("G", "Gi"), rebuilds=False, changes=False),
    Mutator(mut_set_other_iso, ("Gi",)),
    Mutator(mut_remove_row),
    Mutator(mut_remove_hub),
    Mutator(mut_remove_absent, rebuilds=False, changes=False),
    Mutator(mut_clear_build),
    Mutator(mut_resize_shrink_grow),
    Mutator(mut_resize_cols),
    Mutator(mut_reshape_roundtrip, changes=False),
    Mutator(mut_transpose_self, prepare=prep_asymmetric),
    Mutator(mut_ewise_add_self, prepare=prep_asymmetric),
    Mutator(mut_masked_write),
    Mutator(mut_accum_write),
    Mutator(mut_masked_replace),
    Mutator(mut_assign_scalar),
    Mutator(mut_assign_matrix),
    Mutator(mut_assign_row),
    Mutator(mut_assign_col),
    Mutator(mut_select_into),
    Mutator(mut_apply_index_into, ("W", "F", "Wu", "Gi")),
    Mutator(mut_concat_into),
    Mutator(mut_kronecker_into),
    Mutator(mut_diag_into),
    Mutator(mut_union_into),
    Mutator(mut_sort_into, ("W", "F", "Wu", "Gi")),
]}


def base_for(probe, mutator):
    """the first probe object both accept, or None"""
    for b in PROBES[probe].bases:
        if b in MUTATORS[mutator].bases:
            return b
    return None


def start_model(base, mutator):
    """the model a (probe, mutator, base) case builds its object from"""
    m = make(base)
    if MUTATORS[mutator].prepare:
        MUTATORS[mutator].prepare(m)
    return m


PAIRS = [(p, x, base_for(p, x)) for p in PROBES for x in MUTATORS if base_for(p, x)]
# the narrow probe again on the signed one-byte copy: width change, rank shifts, structure changes
PAIRS += [("narrow", x, "Wu") for x in ("overwrite_wide", "set_row64", "set_row0", "remove_row", "remove_hub",
                                        "transpose_self", "masked_write", "select_into")]

# under grid_cap = 1: the rank-shifting setElements against the probes whose builders and
# consumers loop over a grid
CAPPED_PAIRS = [(p, x, base_for(p, x)) for p in ("heads", "hubs", "long", "narrow")
                for x in ("set_row64", "set_row0")]


# ---------------------------------------------------------------------- vectors
NV = 700


def full_vec():
    return np.ones(NV, bool), (np.arange(NV) % 4 + 1).astype(np.float64)


def empty_vec(dtype="BOOL"):
    return np.zeros(NV, bool), np.zeros(NV, dm.NP[dtype])


class VModel:
    def __init__(self, pv, dtype):
        self.pv, self.dtype = (np.array(pv[0], bool), np.array(pv[1], dm.NP[dtype])), dtype


def vmut_set_first(gb, w, m):
    """setElement of an entry that is not there (on a full vector: after removing it)"""
    if m.pv[0][5]:
        del w[5]
        m.pv = dm.remove_element(m.pv, 5)
    w[5] = dm.NP[m.dtype](3).item()
    m.pv = dm.set_element(m.pv, 5, dm.NP[m.dtype](3))


def vmut_set_existing(gb, w, m):
    """setElement twice at one position: the second overwrites"""
    for x in (1, 2):
        w[64] = dm.NP[m.dtype](x).item()
        m.pv = dm.set_element(m.pv, 64, dm.NP[m.dtype](x))


def vmut_set_iso_changed(gb, w, m):
    """the whole vector assigned one value (iso), then one entry given another"""
    w[:] = dm.NP[m.dtype](1).item()
    m.pv = dm.assign_vec(m.pv, dm.NP[m.dtype](1))
    w[699] = dm.NP[m.dtype](0).item()
    m.pv = dm.set_element(m.pv, 699, dm.NP[m.dtype](0))


def vmut_remove(gb, w, m):
    for i in (0, 64, 699):
        del w[i]
        m.pv = dm.remove_element(m.pv, i)


def vmut_clear(gb, w, m):
    w.clear()
    m.pv = (np.zeros_like(m.pv[0]), np.zeros_like(m.pv[1]))


def vmut_resize(gb, w, m):
    """grow by a word, set an entry in the new part and one below, shrink below the size, grow back"""
    w.resize(NV + 64)
    m.pv = dm.resize(m.pv, NV + 64)
    for i in (NV + 3, 7):  # one in the new part, one that stays
        w[i] = dm.NP[m.dtype](1).item()
        m.pv = dm.set_element(m.pv, i, dm.NP[m.dtype](1))
    w.resize(NV - 100)
    m.pv = dm.resize(m.pv, NV - 100)
    w.resize(NV)
    m.pv = dm.resize(m.pv, NV)


VREGION = np.array([0, 63, 64, 300, 699])


def vmut_assign_region(gb, w, m):
    """w[I] << s"""
    w[VREGION] << dm.NP[m.dtype](2).item()
    m.pv = dm.assign_vec(m.pv, dm.NP[m.dtype](2), VREGION)


def _vmask():
    p = np.arange(NV) % 3 == 0
    return p, p.copy()


def vmut_masked_scalar(gb, w, m):
    """w(k.S) << s"""
    k = _vmask()
    w(_gb_vec(gb, k, "BOOL").S) << dm.NP[m.dtype](2).item()
    m.pv = dm.assign_vec(m.pv, dm.NP[m.dtype](2), None, mask=k, mask_struct=True)


def vmut_expr(gb, w, m):
    """w << expr: the product of two sparse vectors"""
    a = _vmask()
    b = np.arange(NV) % 2 == 0, np.arange(NV) % 2 == 0
    av = a[0], np.where(a[0], 2, 0).astype(dm.NP[m.dtype])
    bv = b[0], np.where(b[0], 1, 0).astype(dm.NP[m.dtype])
    op = "land" if m.dtype == "BOOL" else "times"
    w << _gb_vec(gb, av, m.dtype).ewise_mult(_gb_vec(gb, bv, m.dtype), getattr(gb.binary, op))
    m.pv = dm.ewise("mult", op, m.dtype, av, bv)


def _words(p):
    nw = (len(p) + 63) // 64
    bits = np.zeros(nw * 64, bool)
    bits[:len(p)] = p
    return np.packbits(bits.reshape(nw, 64), axis=1, bitorder="little").view("<u8").ravel().astype(np.int64)


def vmut_bitmap_import(gb, w, m):
    """GxB_Vector_bitmap_import of device words: the vector becomes iso true with that structure"""
    import torch

    p = np.arange(NV) % 5 != 0
    words = torch.from_numpy(_words(p)).cuda()
    torch.cuda.synchronize()
    rc = gb.lib.GxB_Vector_bitmap_import(w._h, ctypes.c_void_p(words.data_ptr()), len(words))
    assert rc == 0, rc
    m.pv = (p, np.where(p, 1, 0).astype(dm.NP[m.dtype]))


VMUTATORS = {f.__name__[5:]: f for f in [
    vmut_set_first, vmut_set_existing, vmut_set_iso_changed, vmut_remove, vmut_clear, vmut_resize,
    vmut_assign_region, vmut_masked_scalar, vmut_expr, vmut_bitmap_import]}
VSTARTS = ("full", "empty")  # what the host believes of the vector before the change
