"""Pull heads and next-frontier hints indexed by non-empty row rank (csrc/gb_mxv.hip
gb_view_nonempty / gb_view_pullfirst / k_pull_head, csrc/gb_spmv_iso.hip both pull paths).
A row's record sits at ne_rank[r >> 6] + popcount(rows_ne[r >> 6] & bits below r & 63); rows
without entries have no record.  A wrong rank reads another row's heads (wrong levels or counts)
or a slot past the table.

Every case runs the notebook loop (`v(mask=q.V)[:] = d; q(~v.S, replace=True) << q.vxm(A, sr)`,
and the same level through `At.mxv(q, sr)` on the transposed operand) with spmv_direction=1 --
every level pulls through the heads -- under iso_pack 0 (packed pull) and 1 (per-step pull), for
any_pair and lor_land, and checks the levels against the oracle or a numpy restatement of the
loop and that the per-level q.nvals sequences are those of the restatement under every setting.
Shapes are the smallest that can break a rank: n around one word, every row non-empty (rank =
row id), only the last (tail) word non-empty, alternating whole words empty, one row per word
at bit 0 and at bit 63, rows of 3, 4 and 5 entries between empty rows whose heads miss, a
rectangular operand, R-MAT with a fifth to a third of the rows empty, a matrix changed after its heads were built,
and 65 words in one block (a wave's second group)."""
import contextlib

import numpy as np
import pytest

import oracle as O

pytestmark = pytest.mark.gpu
PACKS = (0, 1)  # knob iso_pack: 0 the packed pull, 1 the per-step pull
SEMIRINGS = ("any_pair", "lor_land")


@pytest.fixture(scope="module")
def gb():
    import graphblas_amd

    return graphblas_amd


@contextlib.contextmanager
def knobs(gb, **kw):
    for k, v in kw.items():
        gb.set_knob(k, v)
    try:
        yield
    finally:
        for k in kw:
            gb.set_knob(k, 0)


def csr_of(n, a, b):
    """boolean graph of the directed edges a[i] -> b[i]"""
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    if not a.size:
        return O.Csr.empty(n, n, "BOOL")
    e = np.unique(np.stack([a, b], 1), axis=0)
    return O.Csr.from_coo(e[:, 0], e[:, 1], True, nrows=n, ncols=n, dtype="BOOL")


def csr_sym(n, a, b):
    """symmetric boolean graph of the undirected edges (a[i], b[i])"""
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    if not a.size:
        return O.Csr.empty(n, n, "BOOL")
    e = np.unique(np.stack([np.concatenate([a, b]), np.concatenate([b, a])], 1), axis=0)
    return O.Csr.from_coo(e[:, 0], e[:, 1], True, nrows=n, ncols=n, dtype="BOOL")


def to_gb(gb, G):
    """G and its transpose on the device (vxm pulls along A's columns, mxv along At's rows)"""
    r, c, _ = G.to_coo()
    return (gb.Matrix.from_coo(r, c, True, dtype=bool, nrows=G.nrows, ncols=G.ncols),
            gb.Matrix.from_coo(c, r, True, dtype=bool, nrows=G.ncols, ncols=G.nrows))


def ref_loop(G, frontier):
    """numpy restatement of the notebook loop from a frontier set: (levels, nvals(q) per level)"""
    n = G.nrows
    rows = np.repeat(np.arange(n), np.diff(G.indptr))
    v = np.zeros(n, np.int32)
    q = np.zeros(n, bool)
    q[np.asarray(frontier, np.int64)] = True
    counts = []
    d = 0
    while True:
        d += 1
        v[q] = d
        nxt = np.zeros(n, bool)
        nxt[G.indices[q[rows]]] = True
        q = nxt & (v == 0)
        counts.append(int(q.sum()))
        if not counts[-1]:
            return v, counts


def gpu_loop(gb, A, At, n, src, sr_name, call):
    sr = getattr(gb.semiring, sr_name)
    v = gb.Vector(gb.INT32, n)
    q = gb.Vector(bool, n)
    q[int(src)] = True
    counts = []
    d = 0
    while True:
        d += 1
        v(mask=q.V)[:] = d
        if call == "vxm":
            q(~v.S, replace=True) << q.vxm(A, sr)
        else:
            q(~v.S, replace=True) << At.mxv(q, sr)
        counts.append(int(q.nvals))
        if not counts[-1]:
            break
    got = np.zeros(n, np.int32)
    i, x = v.to_coo()
    got[i.astype(np.int64)] = x
    return got, counts


def check_loops(gb, G, mats, src, ref=None, grids=(0,)):
    """the loop from `src` under every setting against the restatement (and `ref`)"""
    exp, exp_counts = ref_loop(G, [src])
    if ref is not None:
        assert np.array_equal(exp, ref)
    A, At = mats
    for grid in grids:
        for sr_name in SEMIRINGS:
            for pack in PACKS:
                for call in ("vxm", "mxv"):
                    with knobs(gb, iso_pack=pack, spmv_direction=1, iso_work_grid=grid):
                        got, counts = gpu_loop(gb, A, At, G.nrows, src, sr_name, call)
                    what = (sr_name, pack, call, grid)
                    assert np.array_equal(got, exp), what
                    assert counts == exp_counts, (what, counts, exp_counts)
    return exp, exp_counts


def band_on(n, verts, skip=16):
    """the vertices `verts` (ascending) joined to their 3 nearest neighbours on either side in
    that order and to the ones `skip` places away (rows of 3 to 8 entries, few levels); every
    other vertex has no entries"""
    verts = np.asarray(verts, np.int64)
    m = len(verts)
    a = np.concatenate([verts[:max(m - k, 0)] for k in (1, 2, 3, skip)])
    b = np.concatenate([verts[k:] for k in (1, 2, 3, skip)])
    return csr_sym(n, a, b)


def check_band(gb, n, verts, grids=(0,)):
    """(at most 16 words: the default grid is one block too)"""
    G = band_on(n, verts)
    ne = np.flatnonzero(np.diff(G.indptr))
    assert np.array_equal(ne, np.asarray(verts) if len(verts) > 1 else [])
    for src in (verts[0], verts[-1]):
        ref = O.bfs_levels(G, int(src))[0]
        assert (ref[verts] > 0).all() and np.count_nonzero(ref) == len(verts)
        check_loops(gb, G, to_gb(gb, G), int(src), ref, grids)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_tiny_n(gb, n):
    """one word or a little more, a tail word, n no multiple of 64; every third vertex empty (for
    n = 1: no entry at all, then one self-loop)"""
    if n == 1:
        for G in (csr_of(1, [], []), csr_of(1, [0], [0])):
            check_loops(gb, G, to_gb(gb, G), 0)
        return
    check_band(gb, n, np.flatnonzero(np.arange(n) % 3 != 1))


def test_every_row_nonempty(gb):
    """rank = row id: 200 rows, four words with a tail"""
    check_band(gb, 200, np.arange(200))


def test_last_word_only(gb):
    """330 rows, only the 10 rows of the tail word have entries: rank = row - 320"""
    check_band(gb, 330, np.arange(320, 330))


@pytest.mark.parametrize("parity", [0, 1])
def test_alternating_words(gb, parity):
    """whole words without entries between full ones: the prefix is constant across an empty word"""
    n = 64 * 6
    check_band(gb, n, np.flatnonzero((np.arange(n) >> 6) % 2 == parity))


@pytest.mark.parametrize("bit", [0, 63])
def test_one_row_per_word(gb, bit):
    """8 words, one non-empty row each, at bit 0 (nothing below it) and at bit 63 (everything)"""
    check_band(gb, 64 * 8, np.arange(8) * 64 + bit)


def test_head_walk_boundary(gb):
    """rows of exactly 3, 4 and 5 entries (65, 67, 69) between rows without entries.  At level 1
    (frontier {0}) all three miss their heads; at level 2 (frontier {x = 1}) the short rows find x
    among their heads (their whole row), while the 5-entry row's three heads are the hubs
    10, 11, 12 -- not reached yet -- so it walks its list to find x."""
    n, x = 200, 1
    a, b = [0], [x]
    for r, others in ((65, [130, 131]), (67, [132, 133, 134]), (69, [10, 11, 12, 135])):
        a += [r] * (len(others) + 1)
        b += [x] + others
    for i, h in enumerate((10, 11, 12)):
        a += [h] * 8
        b += list(range(20 + 8 * i, 28 + 8 * i))
    G = csr_sym(n, a, b)
    deg = np.diff(G.indptr)
    assert [deg[r] for r in (65, 67, 69)] == [3, 4, 5] and not deg[[64, 66, 68, 70]].any()
    row = G.indices[G.indptr[69]:G.indptr[70]]
    assert sorted(row[np.argsort(-deg[row], kind="stable")][:3]) == [10, 11, 12]  # the heads: not x
    ref = O.bfs_levels(G, 0)[0]
    assert ref[x] == 2 and ref[65] == ref[67] == ref[69] == 3 and ref[10] == 4 and ref[20] == 5
    check_loops(gb, G, to_gb(gb, G), 0, ref)


def vec_idx(w):
    return np.sort(w.to_coo()[0].astype(np.int64))


def test_rectangular(gb):
    """A 700 x 1500 with entries in every other row and in two columns of three: w<!m.S, replace>
    = A u pulls along 350 of 700 rows (the other orientation has 1500), w<!m.S, replace> = u A
    along 1000 of 1500 columns; against the oracle's mxv / vxm"""
    rng = np.random.default_rng(11)
    nr, nc = 700, 1500
    cols = np.flatnonzero(np.arange(nc) % 3 != 0)
    e = np.unique(np.stack([2 * rng.integers(0, nr // 2, 6000), rng.choice(cols, 6000)], 1), axis=0)
    G = O.Csr.from_coo(e[:, 0], e[:, 1], True, nrows=nr, ncols=nc, dtype="BOOL")
    A = gb.Matrix.from_coo(e[:, 0], e[:, 1], True, dtype=bool, nrows=nr, ncols=nc)
    sr_o = ("LOR", "LAND", "BOOL")
    for call, n_in, n_out in (("mxv", nc, nr), ("vxm", nr, nc)):
        ui = np.sort(rng.choice(n_in, 200, replace=False))
        mi = np.sort(rng.choice(n_out, 250, replace=False))
        uo = O.Vec(n_in, "BOOL", ui, np.ones(len(ui), bool))
        mo = O.Vec(n_out, "BOOL", mi, np.ones(len(mi), bool))
        kw = dict(mask=mo, mask_comp=True, mask_struct=True, replace=True)
        ref = (O.mxv(O.Vec(n_out, "BOOL", [], []), G, uo, sr_o, **kw) if call == "mxv" else
               O.vxm(O.Vec(n_out, "BOOL", [], []), uo, G, sr_o, **kw))
        assert 0 < len(ref.indices) < n_out
        u = gb.Vector.from_coo(ui, True, dtype=bool, size=n_in)
        m = gb.Vector.from_coo(mi, True, dtype=bool, size=n_out)
        for sr_name in SEMIRINGS:
            sr = getattr(gb.semiring, sr_name)
            for pack in PACKS:
                for grid in (1, 0):
                    with knobs(gb, iso_pack=pack, spmv_direction=1, iso_work_grid=grid):
                        w = gb.Vector(bool, n_out)
                        w(~m.S, replace=True) << (A.mxv(u, sr) if call == "mxv" else u.vxm(A, sr))
                        assert np.array_equal(vec_idx(w), ref.indices), (call, sr_name, pack, grid)


@pytest.fixture(scope="module")
def rmats(gb):
    out = {}
    for scale in (10, 13):
        G = O.rmat(scale, 16, 42)
        deg = np.diff(G.indptr)
        # rows and columns without entries: 20 % and 23 % at s10, 30 % at s13 (half at s22)
        cols = np.count_nonzero(np.bincount(G.indices, minlength=G.ncols))
        assert 0.6 < np.count_nonzero(deg) / G.nrows < 0.85 and 0.6 < cols / G.ncols < 0.85
        cand = np.flatnonzero(deg > 0)
        roots = [int(np.argmax(deg))] + [int(r) for r in np.random.default_rng(scale).choice(cand, 3, replace=False)]
        out[scale] = (G, to_gb(gb, G), [(r, O.bfs_levels(G, r)[0]) for r in roots])
    return out


@pytest.mark.parametrize("grid", [1, 0])
@pytest.mark.parametrize("scale", [10, 13])
def test_rmat_roots(gb, rmats, scale, grid):
    """the hub and three seeded roots with out-edges, one block (every wave has several steps and,
    at s13, two groups) and the default grid"""
    G, mats, roots = rmats[scale]
    for src, ref in roots:
        check_loops(gb, G, mats, src, ref, (grid,))


def test_cache_drop(gb):
    """the heads are built by the first pull; an entry added to a row of a middle word that had
    none shifts the rank of every later row, one added to a row of the first word shifts them
    all: the caches must be rebuilt, not reused"""
    n = 64 * 5
    verts = np.flatnonzero((np.arange(n) % 2 == 0) & (np.arange(n) >= 64))
    G = band_on(n, verts)
    A, At = to_gb(gb, G)
    src = int(verts[0])
    check_loops(gb, G, (A, At), src, O.bfs_levels(G, src)[0])
    a, b, _ = G.to_coo()
    for new in (64 * 2 + 31, 5):  # formerly empty rows: the middle word, then the first word
        assert not np.diff(G.indptr)[new]
        far = int(verts[-1])
        for M in (A, At):
            M[new, far] = True
            M[far, new] = True
        a, b = np.concatenate([a, [new, far]]), np.concatenate([b, [far, new]])
        G = csr_of(n, a, b)
        ref = O.bfs_levels(G, src)[0]
        assert ref[new] == ref[far] + 1
        check_loops(gb, G, (A, At), src, ref)


def test_many_words(gb):
    """4 x 16 + 1 words in one block: every wave owns 16 words in its first group and wave 0 a
    second group (the tail word, 57 rows); about half the rows have entries"""
    n = 64 * 64 + 57
    rng = np.random.default_rng(7)
    verts = np.sort(rng.choice(n, n // 2, replace=False))
    verts = np.union1d(verts, [n - 1])
    G = band_on(n, verts, skip=64)
    src = int(verts[len(verts) // 2])
    check_loops(gb, G, to_gb(gb, G), src, O.bfs_levels(G, src)[0], (1,))
