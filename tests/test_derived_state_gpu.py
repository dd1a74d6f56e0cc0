"""No cached view of a matrix or vector outlives a change to it.

Every (probe, mutator) pair of derived_state_cases.py: a fresh object is probed (the probe's
structures are built: its counters rise by what it builds), probed again (nothing is rebuilt),
mutated, and probed a third time -- the result must be the mutated model's, bit for bit, equal to
the same probe on a fresh object built from the mutated model, and the structure must have been
rebuilt (or, for the declared no-ops, kept).  Then every other probe runs once on the mutated
object: a drop that frees one field and forgets its neighbour shows there.  The vector cases do
the same for the host-side beliefs about a vector (count, mailbox, hint, iso, full / empty).

The rebuilt / reused figure of every case is printed at the end of the module (pytest -s).
The file's 308 cases take 12 s on an MI355X, the slowest 0.35 s."""
import time

import numpy as np
import pytest

import dense_model as dm
import derived_state_cases as dc

pytestmark = pytest.mark.gpu

_TABLE = {}  # (probe, mutator) -> rise of the probe's own counter after the mutation


@pytest.fixture(scope="module")
def gb():
    import graphblas_amd

    t0 = time.perf_counter()
    yield graphblas_amd
    graphblas_amd.set_knob("grid_cap", 0)
    for (p, x), d in sorted(_TABLE.items()):
        print(f"\n{p:9s} {x:22s} {'rebuilt' if d else 'reused'} ({d})", end="")
    print(f"\ntest_derived_state_gpu.py: {time.perf_counter() - t0:.1f} s")


def run(gb, probe, A, m, what):
    """the probe on A against the model: (result, rise of every counter)"""
    c0 = dc.counters(gb)
    got, exp = probe.fn(gb, A, m)
    c1 = dc.counters(gb)
    diff = dc.same(got, exp)
    assert diff is None, f"{what}: {probe.name} differs from the model: {diff}"
    return got, {k: c1[k] - c0[k] for k in c0}


def check_pair(gb, pname, xname, base):
    P, X = dc.PROBES[pname], dc.MUTATORS[xname]
    own = next(iter(P.counters))
    m = dc.start_model(base, xname)
    A = dc.to_gb(gb, m)
    _, rise = run(gb, P, A, m, "fresh")
    for c, k in P.counters.items():
        assert rise[c] == k, f"first run: {c} rose by {rise[c]}, not {k}"
    _, rise = run(gb, P, A, m, "second run")
    for c in P.counters:
        assert rise[c] == 0, f"second run, nothing changed: {c} rose by {rise[c]}"
    X.fn(gb, A, m)
    assert P.ok_for(m)
    got, rise = run(gb, P, A, m, f"after {xname}")
    _TABLE[(pname, xname)] = rise[own]
    if X.rebuilds:
        assert rise[own] >= 1, f"after {xname}: {own} did not rise: the old structure was reused"
    else:
        for c in P.counters:
            assert rise[c] == 0, f"after {xname} (no change): {c} rose by {rise[c]}"
    fresh, _ = run(gb, P, dc.to_gb(gb, m), m, f"fresh object of the model after {xname}")
    diff = dc.same(got, fresh)
    assert diff is None, f"after {xname}: {pname} differs from a fresh object's: {diff}"
    for Q in dc.PROBES.values():
        if Q is not P and Q.ok_for(m):
            run(gb, Q, A, m, f"after {xname} (probed by {pname} before)")


@pytest.mark.parametrize("probe,mutator,base", dc.PAIRS, ids=[f"{p}-{x}-{b}" for p, x, b in dc.PAIRS])
def test_probe_after_mutation(gb, probe, mutator, base):
    check_pair(gb, probe, mutator, base)


@pytest.mark.parametrize("probe,mutator,base", dc.CAPPED_PAIRS, ids=[f"{p}-{x}-{b}" for p, x, b in dc.CAPPED_PAIRS])
def test_probe_after_mutation_one_block(gb, probe, mutator, base):
    """the same under grid_cap = 1: every builder and consumer sweeps its grid loop many times"""
    gb.set_knob("grid_cap", 1)
    try:
        check_pair(gb, probe, mutator, base)
    finally:
        gb.set_knob("grid_cap", 0)


# ---------------------------------------------------------------------- dup
@pytest.mark.parametrize("probe", list(dc.PROBES))
def test_dup_is_independent(gb, probe):
    """a dup of a probed matrix shares none of its structures: mutate the dup, the original's
    probe is unchanged and reuses its cache; mutate the original, the dup's is unchanged"""
    P = dc.PROBES[probe]
    own = next(iter(P.counters))
    base = P.bases[0]
    m = dc.make(base)
    A = dc.to_gb(gb, m)
    run(gb, P, A, m, "original")
    B, mb = A.dup(), m.copy()
    dc.mut_set_row64(gb, B, mb)
    _, rise = run(gb, P, A, m, "original after its dup changed")
    assert rise[own] == 0
    _, rise = run(gb, P, B, mb, "mutated dup")
    assert rise[own] >= 1
    dc.mut_set_row0(gb, A, m)
    _, rise = run(gb, P, B, mb, "dup after the original changed")
    assert rise[own] == 0
    _, rise = run(gb, P, A, m, "mutated original")
    assert rise[own] >= 1


# ---------------------------------------------------------------------- a tile of a split
def test_split_tile_of_a_used_matrix(gb):
    """one tile of a split of a probed matrix is an object of its own: every probe on it"""
    m = dc.make("W")
    A = dc.to_gb(gb, m)
    for P in dc.PROBES.values():
        if P.ok_for(m):
            run(gb, P, A, m, "before the split")
    n = m.shape[0]
    tile = A.ss.split([[n], [n - 1, 1]])[0][0]  # all rows, all columns but the last
    tm = dc.Model((np.pad(m.pv[0][:, :n - 1], ((0, 0), (0, 1))), np.pad(m.pv[1][:, :n - 1], ((0, 0), (0, 1)))), m.dtype)
    tile.resize(n, n)
    for P in dc.PROBES.values():
        if P.ok_for(tm):
            run(gb, P, tile, tm, "tile of a split")


# ---------------------------------------------------------------------- knobs between calls
def test_push_heavy_changed_between_calls(gb):
    """the hub table is keyed on the threshold: 8 -> 200 rebuilds, and both give the levels"""
    m = dc.make("G")
    A = dc.to_gb(gb, m)
    ref = dc.ref_bfs(m.pv[0], dc.SRC)
    rises = []
    for heavy in (8, 8, 200, 200, 8):
        c0 = dc.counters(gb)
        with dc.knobs(gb, spmv_direction=2, push_heavy=heavy):
            lev, counts = dc.gpu_bfs(gb, A, dc.SRC)
        rises.append(dc.counters(gb)["hub_tables_built"] - c0["hub_tables_built"])
        assert np.array_equal(lev, ref[0]) and counts == ref[1], heavy
    assert rises == [1, 0, 1, 0, 1]


def test_xhot_cols_changed_between_calls(gb):
    """the relabel is keyed on presence only: 16 -> 64 hot columns keeps the 16-column relabel
    (recorded: no rebuild), and the result is the model's either way"""
    m = dc.make("F")
    A = dc.to_gb(gb, m)
    u = dc._full_u(m, m.dtype)
    rises = []
    for cols in (16, 64, 16):
        c0 = dc.counters(gb)
        got, exp = dc._mxv(gb, A, m, u, xhot=2, xhot_cols=cols)
        rises.append(dc.counters(gb)["hot_relabels_built"] - c0["hot_relabels_built"])
        assert dc.same(got, exp) is None, cols
    print(f"\nxhot_cols 16 -> 64 -> 16: hot_relabels_built rose by {rises}")
    _TABLE[("hot", "knob xhot_cols 16->64")] = rises[1]
    assert rises[0] == 1 and rises[2] == 0


def test_narrow_knob_toggled(gb):
    """narrow 0 -> 1 -> 0: the narrow copy is built once, ignored while off, reused after"""
    for base in ("W", "Wu"):
        m = dc.make(base)
        A = dc.to_gb(gb, m)
        rises = []
        for off in (0, 1, 0):
            gb.set_knob("narrow", off)
            try:
                _, rise = run(gb, dc.PROBES["narrow"], A, m, f"narrow={off}")
            finally:
                gb.set_knob("narrow", 0)
            rises.append(rise["narrow_built"])
        assert rises == [1, 0, 0], base


# ---------------------------------------------------------------------- interleaving
@pytest.mark.parametrize("names", [("G", "G2"), ("G", "G2s"), ("Gs", "G2")])
def test_two_graphs_alternate(gb, names):
    """the heads and hubs probes alternate between two graphs (of one size, and of two sizes with
    one word count: the push's spare bitmap and the cleared-vector pool are keyed by word count),
    then with one loop's q and v cleared and reused for the other graph"""
    ms = [dc.make(k) for k in names]
    As = [dc.to_gb(gb, m) for m in ms]
    for rnd in range(2):
        for P in (dc.PROBES["heads"], dc.PROBES["hubs"]):
            for A, m in zip(As, ms):
                _, rise = run(gb, P, A, m, f"round {rnd}")
                if rnd:
                    assert rise[next(iter(P.counters))] == 0
    if ms[0].shape != ms[1].shape:
        return
    n = ms[0].shape[0]
    q, v = gb.Vector(bool, n), gb.Vector(gb.INT32, n)
    for kw in (dict(spmv_direction=1), dict(spmv_direction=2, push_heavy=dc.PUSH_HEAVY), dict()):
        for A, m in list(zip(As, ms)) * 2:
            with dc.knobs(gb, **kw):
                lev, counts = dc.gpu_bfs(gb, A, dc.SRC, q, v)
            ref = dc.ref_bfs(m.pv[0], dc.SRC)
            assert np.array_equal(lev, ref[0]) and counts == ref[1], kw


def test_frontier_of_a_freed_graph(gb):
    """q produced against G carries a hint keyed by a device address of G; G is freed and another
    matrix of the same shape built at once (the allocator may hand the address out again): the
    next level from that q against the new matrix must be the model's"""
    for kw in (dict(), dict(spmv_direction=2, push_heavy=dc.PUSH_HEAVY), dict(spmv_direction=1)):
        m = dc.make("G")
        A = dc.to_gb(gb, m)
        n = m.shape[0]
        v, q = gb.Vector(gb.INT32, n), gb.Vector(bool, n)
        q[dc.SRC] = True
        with dc.knobs(gb, **kw):
            for d in (1, 2, 3):
                v(mask=q.V)[:] = d
                q(~v.S, replace=True) << q.vxm(A, gb.semiring.any_pair)
            del A
            m2 = dc.make("G2")
            A2 = dc.to_gb(gb, m2)
            v(mask=q.V)[:] = 4
            q(~v.S, replace=True) << q.vxm(A2, gb.semiring.any_pair)
        lev, _ = dc.ref_bfs(m.pv[0], dc.SRC)
        front = lev == 4
        seen = (lev > 0) & (lev <= 4)
        exp = m2.pv[0][front].any(axis=0) & ~seen
        assert q.nvals == int(exp.sum()), kw
        assert np.array_equal(dc.vec_coo(q)[0], np.flatnonzero(exp)), kw


# ---------------------------------------------------------------------- the column-word form
def _cw_result(gb, A, m):
    """Q = Q0 any.pair A in column-word form, with its model"""
    Q0m = dc.frontier_model(m.shape[0])
    Q0 = dc.to_gb(gb, dc.Model(Q0m, "BOOL", iso=True))
    Q = gb.Matrix(bool, dc.CW_ROWS, m.shape[1])
    built = dc.counters(gb)["hub_tables_built"]
    with dc.knobs(gb, colbits=1):
        Q << Q0.mxm(A, gb.semiring.any_pair)
    # the column-word mxm ran (it builds A's two hub tables): Q is held in column words
    assert dc.counters(gb)["hub_tables_built"] - built == 2
    T = dm.mxm("any", "pair", "BOOL", Q0m, (m.pv[0], m.pv[0].copy()))
    return Q, dc.Model((T[0], T[0].copy()), "BOOL")


def _check_matrix(A, m, what):
    r, c, x = m.coo()
    diff = dc.same(dc.coo(A), (r, c, x))
    assert diff is None, f"{what}: {diff}"
    assert A.nvals == len(r), what


@pytest.mark.parametrize("change", ["set", "remove", "resize", "select_output", "csc_input", "next_level"])
def test_column_word_matrix_changes(gb, change):
    """a 13 x 700 result held in column words is changed, or read, by operations outside
    gb_colbits.hip: they must see (and leave) the CSR of the same matrix"""
    m = dc.make("G")
    A = dc.to_gb(gb, m)
    Q, qm = _cw_result(gb, A, m)
    n = m.shape[1]
    if change == "set":
        assert not qm.pv[0][12, 0]
        Q[12, 0] = True
        qm.pv = dm.set_element(qm.pv, (12, 0), True)
    elif change == "remove":
        j = int(np.flatnonzero(qm.pv[0][1])[0])
        del Q[1, j]
        qm.pv = dm.remove_element(qm.pv, (1, j))
    elif change == "resize":
        for k in (65, dc.CW_ROWS):  # past 64 rows the column-word form does not exist
            Q.resize(k, n)
            qm.pv = dm.resize(qm.pv, (k, n))
    elif change == "select_output":
        S = dc.to_gb(gb, qm)
        Q << S.select("triu", 100)
        keep = np.triu(qm.pv[0], 100)
        qm.pv = (keep, keep.copy())
    elif change == "csc_input":
        T = Q.T.new()
        diff = dc.same(dc.coo(T), dm.to_coo(dm.transpose(qm.pv)))
        assert diff is None, diff
    if change != "next_level":  # next_level: Q enters the next mxm still in column words
        _check_matrix(Q, qm, change)
    with dc.knobs(gb, colbits=1):
        R = gb.Matrix(bool, Q.nrows, n)
        R << Q.mxm(A, gb.semiring.any_pair)
    T = dm.mxm("any", "pair", "BOOL", qm.pv, (m.pv[0], m.pv[0].copy()))
    _check_matrix(R, dc.Model((T[0], T[0].copy()), "BOOL"), f"{change}, next level")
    _check_matrix(Q, qm, f"{change}, after the next level")
    diff = dc.same(dc.coo(Q.T.new()), dm.to_coo(dm.transpose(qm.pv)))  # its CSC, built after the change
    assert diff is None, f"{change}: transpose: {diff}"


# ---------------------------------------------------------------------- vectors
def _device_touch(gb, w, m):
    """w[I] << s, then half of I's bits and a whole word cleared through GxB_Vector_device_view,
    followed by GxB_Vector_device_touch"""
    import torch
    from graphblas_amd import device as gdev

    dc.vmut_assign_region(gb, w, m)
    assert w.nvals == int(m.pv[0].sum())  # the host believes the old count
    keep = np.ones(dc.NV, bool)
    keep[dc.VREGION[::2]] = False
    keep[128:192] = False
    words = torch.from_numpy(dc._words(keep)).cuda()
    torch.cuda.synchronize()
    nw = (dc.NV + 63) // 64
    bits = gdev.device_tensor(torch, gdev.vector_view(w._h).bitmap, nw)
    bits &= words
    torch.cuda.synchronize()
    assert gb.lib.GxB_Vector_device_touch(w._h) == 0
    m.pv = (m.pv[0] & keep, np.where(keep, m.pv[1], 0).astype(m.pv[1].dtype))


VMUTATORS = dict(dc.VMUTATORS, device_touch=_device_touch)


@pytest.fixture(scope="module")
def operand(gb):
    m = dc.make("F")
    return dc.to_gb(gb, m), m


def _consumers(gb, F, Fm, u, um, k, km, what):
    """u.nvals, F u, and F u under the mask k.S and ~k.S with replace, against the model"""
    assert u.nvals == int(um.pv[0].sum()), what
    assert k.nvals == int(km.pv[0].sum()), what
    n = Fm.shape[0]
    T = dm.mxv("plus", "times", "FP64", Fm.pv, um.pv)
    zero = np.zeros(n, bool), np.zeros(n, np.float64)
    w = gb.Vector("FP64", n)
    w << F.mxv(u, gb.semiring.plus_times)
    diff = dc.same(dc.vec_coo(w), dc.model_vec_coo(T))
    assert diff is None, f"{what}: F u: {diff}"
    for comp in (False, True):
        w = gb.Vector("FP64", n)
        w[dc.VREGION] << 7.0  # replace must delete these
        w((~k.S if comp else k.S), replace=True) << F.mxv(u, gb.semiring.plus_times)
        exp = dm.write_back(zero, T, mask=km.pv, mask_struct=True, mask_comp=comp, replace=True)
        diff = dc.same(dc.vec_coo(w), dc.model_vec_coo(exp))
        assert diff is None, f"{what}: F u under {'~' if comp else ''}k.S: {diff}"
        assert w.nvals == int(exp[0].sum()), what


@pytest.mark.parametrize("role", ["input", "mask"])
@pytest.mark.parametrize("start", dc.VSTARTS)
@pytest.mark.parametrize("mutator", list(VMUTATORS))
def test_vector_after_mutation(gb, operand, mutator, start, role):
    """the mutated vector is the input u (FP64) or the mask k (BOOL) of w<k.S, replace> = F u; it
    starts full or empty, is consumed (the host now believes it full / empty), changed, consumed"""
    F, Fm = operand
    dtype = "FP64" if role == "input" else "BOOL"
    x = gb.Vector(dtype, dc.NV)
    if start == "empty":
        xm = dc.VModel(dc.empty_vec(dtype), dtype)
    elif dtype == "BOOL" or mutator == "set_iso_changed":  # full and iso
        x[:] << dm.NP[dtype](1).item()
        xm = dc.VModel((np.ones(dc.NV, bool), np.ones(dc.NV, dm.NP[dtype])), dtype)
    else:  # full, values 1..4
        xm = dc.VModel(dc.full_vec(), dtype)
        x = dc._gb_vec(gb, xm.pv, dtype)
    other_pv = dc._vmask() if role == "input" else dc.full_vec()
    om = dc.VModel(other_pv, "BOOL" if role == "input" else "FP64")
    o = dc._gb_vec(gb, om.pv, om.dtype)
    args = (x, xm, o, om) if role == "input" else (o, om, x, xm)
    _consumers(gb, F, Fm, *args, "before")
    VMUTATORS[mutator](gb, x, xm)
    _consumers(gb, F, Fm, *args, f"after {mutator}")
    VMUTATORS[mutator](gb, x, xm)  # and once more on the changed vector
    _consumers(gb, F, Fm, *args, f"after {mutator} twice")


def test_full_and_empty_flip(gb, operand):
    """full -> not full -> full and empty -> non-empty -> empty by single elements, consumed at
    every step: `full` and the empty mask's host count are decided from the host's belief"""
    F, Fm = operand
    um = dc.VModel(dc.full_vec(), "FP64")
    u = dc._gb_vec(gb, um.pv, "FP64")
    km = dc.VModel(dc.empty_vec("BOOL"), "BOOL")
    k = gb.Vector(bool, dc.NV)
    _consumers(gb, F, Fm, u, um, k, km, "full, empty")
    del u[dc.HUB]
    um.pv = dm.remove_element(um.pv, dc.HUB)
    k[3] = True
    km.pv = dm.set_element(km.pv, 3, True)
    _consumers(gb, F, Fm, u, um, k, km, "one short of full, one entry")
    u[dc.HUB] = 2.0
    um.pv = dm.set_element(um.pv, dc.HUB, 2.0)
    del k[3]
    km.pv = dm.remove_element(km.pv, 3)
    _consumers(gb, F, Fm, u, um, k, km, "full again, empty again")
