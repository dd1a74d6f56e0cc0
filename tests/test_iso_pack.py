"""Open rows packed across a wave's steps in the iso SpMV's pull and push (csrc/gb_spmv_iso.hip,
knob iso_pack: 0 both on -- the default --, 1 both off: the per-step loops, 2 pull only, 3 push
only).  The packed pull takes a wave's words in groups of 4 steps (16 words, one lane each),
packs the open rows by a prefix sum of the words' popcounts and runs its chain of reads once per
batch of 256 packed rows; the push appends the frontier rows of successive steps to one segment
list and walks it when the next step's rows would not fit 256 or the words run out.

Every case runs the notebook loop (`v(mask=q.V)[:] = d; q(~v.S, replace=True) << q.vxm(A, sr)`)
or one masked call under the four settings, for any_pair and lor_land, and checks the result
against the oracle or a numpy restatement of the loop, and that the per-level q.nvals sequences
of the four settings are equal (and the restatement's).  Shapes are the smallest that reach each
path: one block (iso_work_grid 1) so a wave has several steps, more than one group (R-MAT s13:
8 steps a wave), several batches in a group, a group of exactly 256 open rows, word counts that
are no multiple of 4, a tail word, waves without a word, list rounds past the first cap, a
level with nothing open, a rectangular operand, null stamp / mask words, and a push list that
is walked once or mid-way."""
import contextlib

import numpy as np
import pytest

import oracle as O

pytestmark = pytest.mark.gpu
SETTINGS = (0, 1, 2, 3)
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


def csr_sym(n, a, b):
    """symmetric boolean graph of the undirected edges (a[i], b[i])"""
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    e = np.unique(np.stack([np.concatenate([a, b]), np.concatenate([b, a])], 1), axis=0)
    return O.Csr.from_coo(e[:, 0], e[:, 1], True, nrows=n, ncols=n, dtype="BOOL")


def to_gb(gb, G):
    r, c, _ = G.to_coo()
    return gb.Matrix.from_coo(r, c, True, nrows=G.nrows, ncols=G.ncols)


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


def gpu_loop(gb, A, n, frontier, sr_name):
    sr = getattr(gb.semiring, sr_name)
    v = gb.Vector(gb.INT32, n)
    if np.ndim(frontier) == 0:
        q = gb.Vector(bool, n)
        q[int(frontier)] = True
    else:
        q = gb.Vector.from_coo(np.asarray(frontier, np.int64), True, dtype=bool, size=n)
    counts = []
    d = 0
    while True:
        d += 1
        v(mask=q.V)[:] = d
        q(~v.S, replace=True) << q.vxm(A, sr)
        counts.append(int(q.nvals))
        if not counts[-1]:
            break
    got = np.zeros(n, np.int32)
    i, x = v.to_coo()
    got[i.astype(np.int64)] = x
    return got, counts


def check_loops(gb, G, A, frontier, ref=None, **kn):
    """the loop under the four settings and both semirings against the restatement (and `ref`)"""
    exp, exp_counts = ref_loop(G, np.atleast_1d(frontier))
    if ref is not None:
        assert np.array_equal(exp, ref)
    for sr_name in SEMIRINGS:
        for s in SETTINGS:
            with knobs(gb, iso_pack=s, **kn):
                got, counts = gpu_loop(gb, A, G.nrows, frontier, sr_name)
            assert np.array_equal(got, exp), (sr_name, s)
            assert counts == exp_counts, (sr_name, s, counts, exp_counts)
    return exp, exp_counts


@pytest.fixture(scope="module")
def rmats(gb):
    out = {}
    for scale in (10, 13):
        G = O.rmat(scale, 16, 42)
        src = int(np.argmax(np.diff(G.indptr)))
        out[scale] = (G, to_gb(gb, G), src, O.bfs_levels(G, src)[0])
    return out


@pytest.mark.parametrize("grid", [1, 0])
@pytest.mark.parametrize("direction", [1, 2, 0])  # pull only, push only, device-chosen
@pytest.mark.parametrize("scale", [10, 13])
def test_rmat_bfs(gb, rmats, scale, direction, grid):
    """one block takes every word: 8 steps per wave at s13 (two groups, several batches)"""
    G, A, src, ref = rmats[scale]
    check_loops(gb, G, A, src, ref, spmv_direction=direction, iso_work_grid=grid)


def band(n, m=None):
    """vertices 0 .. m-1 joined to their 6 nearest neighbours (the rest without entries)"""
    m = n if m is None else m
    a = np.concatenate([np.arange(m - k) for k in (1, 2, 3)])
    b = np.concatenate([np.arange(k, m) for k in (1, 2, 3)])
    return csr_sym(n, a, b)


def test_dense_open_pull(gb):
    """n = 1221: 20 words (no multiple of 4, a 5-row tail word); with one block wave 0 owns words
    0-3 and 16-19 -- the first level has ~500 open rows in the group: two batches"""
    n = 1024 + 64 * 3 + 5
    G = band(n)
    ref = O.bfs_levels(G, 0)[0]
    assert ref.min() > 0
    check_loops(gb, G, to_gb(gb, G), 0, ref, spmv_direction=1, iso_work_grid=1)


def test_group_of_exactly_256_open_rows(gb):
    """n = 257, BFS from 256: wave 0 owns words 0-3, all 256 rows open at the first level (one
    full batch, no second); wave 1 owns the 1-row tail word, waves 2 and 3 none"""
    n = 257
    G = band(n)
    ref = O.bfs_levels(G, 256)[0]
    check_loops(gb, G, to_gb(gb, G), 256, ref, spmv_direction=1, iso_work_grid=1)


@pytest.mark.parametrize("cap", [0, 16])
def test_long_unsettled_rows(gb, cap):
    """three rows of 300 entries: 299 leaves each (numbered below the chain, 5 of them a clique
    so the pull heads are leaves) and, as the row's last entry, one vertex of a chain walked
    from its start.  Until the chain reaches that vertex the rows miss their heads and walk all
    300 entries in list rounds (cap 64, 128, 256; with pull_cap 16: 16 .. 256); then the hit
    comes in the last round."""
    hubs, nleaf, nchain = 3, 299, 8
    chain0 = hubs + hubs * nleaf
    n = chain0 + nchain
    a, b = [], []
    for h in range(hubs):
        leaves = hubs + h * nleaf + np.arange(nleaf)
        a += [h] * nleaf + [h]
        b += leaves.tolist() + [chain0 + 2 + h]
        for i in range(5):
            for j in range(i + 1, 5):
                a.append(int(leaves[i]))
                b.append(int(leaves[j]))
    a += (chain0 + np.arange(nchain - 1)).tolist()
    b += (chain0 + np.arange(1, nchain)).tolist()
    G = csr_sym(n, a, b)
    assert all(G.indptr[h + 1] - G.indptr[h] == 300 for h in range(hubs))
    assert all(G.indices[G.indptr[h + 1] - 1] == chain0 + 2 + h for h in range(hubs))
    ref = O.bfs_levels(G, chain0)[0]
    assert ref[0] == 4 and ref[2] == 6 and ref.min() > 0  # two levels and more without a hit
    A = to_gb(gb, G)
    for grid in (1, 0):
        check_loops(gb, G, A, chain0, ref, spmv_direction=1, iso_work_grid=grid, pull_cap=cap)


def test_nothing_open(gb):
    """a band over the first 600 of 1221 vertices: the last level finds every row with entries
    closed by the mask and every other row without entries -- no group has an open row, every
    output word is still written"""
    n = 1221
    G = band(n, 600)
    ref = O.bfs_levels(G, 0)[0]
    assert (ref[:600] > 0).all() and not ref[600:].any()
    for direction in (1, 0):
        _, counts = check_loops(gb, G, to_gb(gb, G), 0, ref, spmv_direction=direction, iso_work_grid=1)
        assert counts[-1] == 0


def vec_idx(w):
    return np.sort(w.to_coo()[0].astype(np.int64))


def test_rectangular_mxv(gb):
    """w<!m.S, replace> = A u with A 700 x 1500 (the sharded loop's shape: the result's length is
    not the frontier's), pull only, against the oracle's mxv"""
    rng = np.random.default_rng(5)
    nr, nc = 700, 1500
    e = np.unique(np.stack([rng.integers(0, nr, 6000), rng.integers(0, nc, 6000)], 1), axis=0)
    G = O.Csr.from_coo(e[:, 0], e[:, 1], True, nrows=nr, ncols=nc, dtype="BOOL")
    ui = np.sort(rng.choice(nc, 200, replace=False))
    mi = np.sort(rng.choice(nr, 250, replace=False))
    ref = O.mxv(O.Vec(nr, "BOOL", [], []), G, O.Vec(nc, "BOOL", ui, np.ones(len(ui), bool)),
                ("LOR", "LAND", "BOOL"), mask=O.Vec(nr, "BOOL", mi, np.ones(len(mi), bool)), mask_comp=True,
                mask_struct=True, replace=True)
    assert 0 < len(ref.indices) < nr
    A = gb.Matrix.from_coo(e[:, 0], e[:, 1], True, nrows=nr, ncols=nc)
    u = gb.Vector.from_coo(ui, True, dtype=bool, size=nc)
    m = gb.Vector.from_coo(mi, True, dtype=bool, size=nr)
    for sr_name in SEMIRINGS:
        for s in SETTINGS:
            for grid in (1, 0):
                with knobs(gb, iso_pack=s, spmv_direction=1, iso_work_grid=grid):
                    w = gb.Vector(bool, nr)
                    w(~m.S, replace=True) << A.mxv(u, getattr(gb.semiring, sr_name))
                    assert np.array_equal(vec_idx(w), ref.indices), (sr_name, s, grid)
                    assert w.to_coo()[1].all()


@pytest.mark.parametrize("direction", [1, 2])
def test_no_stamp_no_mask(gb, rmats, direction):
    """a plain q.vxm(A) and a non-complemented structural mask: the stamp's and the mask's words
    are null pointers in the kernel"""
    G, A, _, _ = rmats[10]
    n = G.nrows
    rng = np.random.default_rng(3)
    qi = np.sort(rng.choice(n, 40, replace=False))
    mi = np.sort(rng.choice(n, 300, replace=False))
    qo = O.Vec(n, "BOOL", qi, np.ones(len(qi), bool))
    plain = O.vxm(O.Vec(n, "BOOL", [], []), qo, G, ("LOR", "LAND", "BOOL"))
    masked = O.vxm(O.Vec(n, "BOOL", [], []), qo, G, ("LOR", "LAND", "BOOL"),
                   mask=O.Vec(n, "BOOL", mi, np.ones(len(mi), bool)), mask_struct=True)
    assert len(plain.indices) > len(masked.indices) > 0
    q = gb.Vector.from_coo(qi, True, dtype=bool, size=n)
    m = gb.Vector.from_coo(mi, True, dtype=bool, size=n)
    for sr_name in SEMIRINGS:
        sr = getattr(gb.semiring, sr_name)
        for s in SETTINGS:
            for grid in (1, 0):
                with knobs(gb, iso_pack=s, spmv_direction=direction, iso_work_grid=grid):
                    assert np.array_equal(vec_idx(q.vxm(A, sr).new()), plain.indices), (sr_name, s, grid)
                    assert np.array_equal(vec_idx(q.vxm(A, sr).new(mask=m.S)), masked.indices), (sr_name, s, grid)


@pytest.mark.parametrize("frontier", ["sparse", "over_256"])
def test_push_merge(gb, frontier):
    """4096 vertices in chains of 16 (degree 2), push only, one block: wave 0 owns words 0-3,
    16-19, 32-35, 48-51 in its four steps.  sparse: two vertices in two words of every step of
    every wave, 4 rows a step -- the list is walked once; over_256: every even vertex, 128 rows
    a step -- the third step's rows do not fit, the list is walked mid-way and at the end."""
    n = 4096
    i = np.arange(n - 1)
    i = i[(i % 16) != 15]
    G = csr_sym(n, i, i + 1)
    assert np.diff(G.indptr).max() == 2
    if frontier == "sparse":
        words = np.array([w for w in range(64) if w % 4 < 2])
        f = np.sort(np.concatenate([words * 64, words * 64 + 32]))
    else:
        f = np.arange(0, n, 2)
    A = to_gb(gb, G)
    for grid in (1, 0):
        check_loops(gb, G, A, f, None, spmv_direction=2, iso_work_grid=grid)
