"""The push levels' shorter chains of dependent reads (csrc/gb_spmv_iso.hip gb_push_phase,
gb_push_root, gb_push_targets; the hub table's sections, csrc/gb_mxv.hip gb_view_hubs):

* a hub piece carries its first edge position and its length in the table, and is expanded 512
  edges a step (8 per lane) -- pieces shorter than that, pieces of push_heavy 1024 (two strides)
  and rows that end in a short piece must come out the same;
* the next-frontier hint reads one 32-bit row length per added vertex, all of a step's at once;
* the first step's row bounds and the stamp's word are read with the hub entries' probes.

Graphs of 5 000 vertices (79 bitmap words: no multiple of 4, a tail word) hold rows of length
1, H - 1, H, H + 1, 2H, 2H + 1 and 3H + 7 for H = push_heavy in {8, 512, 1024} (distinct
targets within a row), 30 more rows of 3H + 7 so the hub table has over 120 pieces (one block
sweeps it twice), and two entries in every other row.  Every case runs the level loop through
the C ABI from a root whose row lists the seven special vertices and from the 3H + 7 vertex
itself (a pending root whose row is a hub), for any_pair and lor_land, a structural and a value
stamp, push forced and the device's choice, one block, two blocks and the full grid (grid_cap
and iso_work_grid: the hub sweep and the word loop run several rounds per wave) and iso_pack 0
and 1; mxv runs on the transposed matrix.  Levels and per-level counts must equal the oracle's
and a run without speculation.

The hint is exact or the next level's direction may differ: test_hint_at_the_alpha_threshold
sizes a frontier so that Beamer's rule flips if the hint is off by one row length, on either
side.  The direction the device took shows in the count of launches that pushed
(GxB_Global_get_int "stat_iso_push_launches"); with the speculation off (one launch per level)
it must equal the rule replayed on the host with the exact edge counts, level by level, and
differ between the two sides by the one level that was sized.  Levels, counts and the number of
adopted speculations (speculation on) are checked as well."""
import contextlib
import ctypes
import itertools

import numpy as np
import pytest

import oracle as O

pytestmark = pytest.mark.gpu
U64 = ctypes.c_uint64
N = 5000
HEAVY = (8, 512, 1024)


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


def stat(gb, key):
    v = ctypes.c_int64()
    assert gb.lib.GxB_Global_get_int(key.encode(), ctypes.byref(v)) == 0
    return v.value


def special_lengths(H):
    return [1, H - 1, H, H + 1, 2 * H, 2 * H + 1, 3 * H + 7]


def build_graph(H, seed):
    """vertex 0: a row listing the special vertices 1..7 (lengths special_lengths(H)); vertices
    8..37: 30 rows of 3H + 7; every other vertex: 2 entries"""
    rng = np.random.default_rng(seed)
    lens = np.full(N, 2)
    lens[1:8] = special_lengths(H)
    lens[8:38] = 3 * H + 7
    rows, cols = [np.zeros(7, np.int64)], [np.arange(1, 8)]
    for r in range(1, N):
        rows.append(np.full(lens[r], r, np.int64))
        cols.append(rng.choice(N, lens[r], replace=False))
    r, c = np.concatenate(rows), np.concatenate(cols)
    G = O.Csr.from_coo(r, c, True, nrows=N, ncols=N, dtype="BOOL")
    assert np.array_equal(np.diff(G.indptr)[1:8], special_lengths(H))
    return G, r, c


@pytest.fixture(scope="module")
def graphs(gb):
    out = {}
    for H in HEAVY:
        G, r, c = build_graph(H, 100 + H)
        A = gb.Matrix.from_coo(r, c, True, nrows=N, ncols=N)
        AT = gb.Matrix.from_coo(c, r, True, nrows=N, ncols=N)
        refs = {src: O.bfs_levels(G, src)[0] for src in (0, 7)}
        assert all(ref.max() >= 3 for ref in refs.values())
        out[H] = (A, AT, refs)
    return out


def run_loop(gb, A, n, src, sr_name, mxv, structural, max_levels=64):
    """v<q> = d; q<!v.S, replace> = q (+).(x) A through the C ABI: (levels, nvals(q) per level)"""
    lib = gb.lib
    sr = lib.GxB_ANY_PAIR_BOOL if sr_name == "any_pair" else lib.GrB_LOR_LAND_SEMIRING_BOOL
    desc = lib.GrB_DESC_S if structural else None
    q, v = ctypes.c_void_p(), ctypes.c_void_p()
    assert lib.GrB_Vector_new(ctypes.byref(q), lib.GrB_BOOL, n) == 0
    assert lib.GrB_Vector_new(ctypes.byref(v), lib.GrB_INT32, n) == 0
    assert lib.GrB_Vector_setElement_BOOL(q, True, int(src)) == 0
    nv = U64()
    counts = []
    for d in range(1, max_levels):
        assert lib.GrB_Vector_assign_INT32(v, q, None, d, lib.GrB_ALL, n, desc) == 0
        if mxv:
            assert lib.GrB_mxv(q, v, None, sr, A._carg, q, lib.GrB_DESC_RSC) == 0
        else:
            assert lib.GrB_vxm(q, v, None, sr, q, A._carg, lib.GrB_DESC_RSC) == 0
        assert lib.GrB_Vector_nvals(ctypes.byref(nv), q) == 0
        counts.append(nv.value)
        if nv.value == 0:
            break
    assert lib.GrB_Vector_nvals(ctypes.byref(nv), v) == 0
    idx = np.empty(nv.value, np.uint64)
    x = np.empty(nv.value, np.int32)
    assert lib.GrB_Vector_extractTuples_INT32(ctypes.c_void_p(idx.ctypes.data), ctypes.c_void_p(x.ctypes.data),
                                              ctypes.byref(nv), v) == 0
    lib.GrB_Vector_free(ctypes.byref(q))
    lib.GrB_Vector_free(ctypes.byref(v))
    got = np.zeros(n, np.int32)
    got[idx.astype(np.int64)] = x
    return got, counts


def ref_counts(ref):
    depth = int(ref.max())
    return [int((ref == d + 1).sum()) for d in range(1, depth + 1)]


@pytest.mark.parametrize("mxv", [False, True])
@pytest.mark.parametrize("H", HEAVY)
def test_hub_rows_every_setting(gb, graphs, H, mxv):
    A, AT, refs = graphs[H]
    M = AT if mxv else A
    for src, sr_name, structural, direction, cap, pack in itertools.product(
            (0, 7), ("any_pair", "lor_land"), (True, False), (2, 0), (1, 2, 0), (0, 1)):
        ref = refs[src]
        kn = dict(push_heavy=H, spmv_direction=direction, grid_cap=cap, iso_work_grid=cap, iso_pack=pack)
        runs = {}
        with knobs(gb, **kn):
            runs["spec"] = run_loop(gb, M, N, src, sr_name, mxv, structural)
        with knobs(gb, bfs_spec=1, **kn):
            runs["nospec"] = run_loop(gb, M, N, src, sr_name, mxv, structural)
        what = (src, sr_name, structural, direction, cap, pack)
        for key, (got, counts) in runs.items():
            assert np.array_equal(got, ref), (what, key)
            assert counts == ref_counts(ref), (what, key, counts)


def threshold_graph(side, alpha):
    """Root 0 -> 40 vertices (1..40) with rows of 1 to 6 entries into 41..1999: the hint of the
    root level's result is the sum mf of those 40 row lengths, and the next level pushes iff
    mf * alpha < open * nnz / n (open: the rows not yet visited).  Filler entries among vertices
    the BFS never reaches (3000..4095) set nnz so that the rule holds by less than one unit of
    mf * alpha ("push") or fails by less than one ("pull"): a hint off by the shortest row flips
    it.  The level after that is sized the same way by nothing -- it runs as the rule says."""
    n = 4096
    rng = np.random.default_rng(7)
    lens = rng.integers(1, 7, 40)
    rows = [np.zeros(40, np.int64)]
    cols = [np.arange(1, 41)]
    for i, d in enumerate(lens):
        rows.append(np.full(d, i + 1, np.int64))
        cols.append(rng.choice(np.arange(41, 2000), d, replace=False))
    second = np.unique(np.concatenate(cols[1:]))
    for t in second:  # the level after: one entry each, so the loop goes on
        rows.append(np.array([t]))
        cols.append(np.array([2000 + (t % 500)]))
    r, c = np.concatenate(rows), np.concatenate(cols)
    mf = int(lens.sum())
    open_rows = n - 1 - 40  # the mask's count when the second level decides: the root and its 40
    base = len(r)
    # nnz with open * nnz / n just above (push) or just below or at (pull) mf * alpha
    need = mf * alpha * n / open_rows
    nnz = int(np.floor(need)) + 1 if side == "push" else int(np.floor(need))
    rule = mf * alpha < open_rows * (nnz / n)
    assert rule == (side == "push")
    assert ((mf + 1) * alpha < open_rows * (nnz / n)) != ((mf - 1) * alpha < open_rows * (nnz / n))
    fill = nnz - base
    assert 0 < fill < 1000 * 1000
    fr = 3000 + np.arange(fill) // 1000
    fc = 3000 + np.arange(fill) % 1000
    r, c = np.concatenate([r, fr]), np.concatenate([c, fc])
    G = O.Csr.from_coo(r, c, True, nrows=n, ncols=n, dtype="BOOL")
    assert G.nvals == nnz
    return G, r, c


def replay_pushes(G, ref, alpha):
    """the levels that push when the rule is replayed on the host with exact edge counts: the
    root's level (host-decided), then m_f * alpha < open rows * average degree"""
    n, nnz = G.nrows, G.nvals
    deg = np.diff(G.indptr)
    out, seen = [], 0
    for d in range(1, int(ref.max()) + 1):
        at = ref == d
        seen += int(at.sum())
        mf = int(deg[at].sum())
        out.append(d == 1 or float(mf) * float(alpha) < float(n - seen) * (float(nnz) / float(n)))
    return out


@pytest.mark.parametrize("side", ["push", "pull"])
def test_hint_at_the_alpha_threshold(gb, side):
    alpha = 48
    G, r, c = threshold_graph(side, alpha)
    n = G.nrows
    A = gb.Matrix.from_coo(r, c, True, nrows=n, ncols=n)
    ref = O.bfs_levels(G, 0)[0]
    assert ref.max() == 4
    pushes = replay_pushes(G, ref, alpha)
    assert pushes[0] and pushes[1] == (side == "push")  # the sized level is the second
    # (the third level, 7 248 against 7 163, is within two row lengths of its own threshold too)
    with knobs(gb, push_alpha=alpha, bfs_spec=1):
        p0 = stat(gb, "stat_iso_push_launches")
        got, counts = run_loop(gb, A, n, 0, "any_pair", False, True)
        pushed = stat(gb, "stat_iso_push_launches") - p0
    assert np.array_equal(got, ref) and counts == ref_counts(ref), counts
    assert pushed == sum(pushes), (side, pushed, pushes)
    with knobs(gb, push_alpha=alpha):
        a0 = stat(gb, "stat_bfs_spec_adopted")
        got2, counts2 = run_loop(gb, A, n, 0, "any_pair", False, True)
        adopted = stat(gb, "stat_bfs_spec_adopted") - a0
    assert np.array_equal(got2, ref) and counts2 == counts
    assert adopted > 0
