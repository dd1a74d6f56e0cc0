"""The later grid sweeps of every capped launch, at small shapes (-m gpu).

Almost every kernel is launched as gb_grid(items, per_block, cap) blocks and walks its items in a
grid-stride loop; the caps are 8192 or 16384 blocks, so the shapes of the other suites run each
loop once per thread.  The knob grid_cap = k clamps every such grid to k blocks (csrc/gb_internal.h)
and counts each call site at which that clamp bit as stat_grid_clamped:<file>:<line>.  Here the
operations run under grid_cap 1 (one block of four waves, the most sweeps), 3 (a stride that is no
power of two, 12 waves), 33 (one block more than GB_GRID_SHARDS; with 31 and 32 where the call
counts through gb_grid_sum / gb_grid_add) and 0, against the models the other suites already use:
dense_model, union_model, tile_model, reindex_model, subassign_model, sort_model,
index_apply_model, semiring_cases, kron_model and the C oracle.  No model is new.

Comparisons go through to_coo() / the CSR export: indices, their order, nvals, dtype and values bit
for bit; the one bound is dense_model's n eps sum|x| for a float plus reduction.

Shapes: vectors of 70001 (1094 words, the last one partial; 65 where the cap never bites), matrices
1300 x 700 and 700 x 1300 of about 20000 entries whose first 70, middle 130 and last 70 rows are
empty (the row hint a wave carries from chunk to chunk crosses long empty runs, and rowptr[i] ==
nvals at the tail), with a hub row of 700 entries and rows of 63, 64 and 65 entries side by side.
A per-thread loop has three sweeps at cap 1 from 768 items, a per-wave loop from 12 units.

The last test scans csrc/ for gb_grid( call sites and asserts that every one was clamped during
the cap-1 runs, but for the sites of NOT_REACHED; test_not_reached_table_matches_the_sources checks
that table without a GPU.
"""
import ctypes
import functools
import os
import re
import time

import numpy as np
import pytest

import dense_model as dm
import index_apply_model as im
import oracle as O
import reindex_model as rm
import semiring_cases as sc
import sort_model as som
import subassign_model as sam
import test_general_ops_gpu as G
import test_semiring_sweep_gpu as S
import tile_model as tm
import union_model as um
from test_kronecker_abi import kron_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "graph-python_amd", "csrc")

CAPS = (1, 3, 33, 0)
CAPS_SUM = (1, 3, 31, 32, 33, 0)  # calls that count through gb_grid_sum / gb_grid_add
NVEC = 70001
SHAPE, SHAPE_T = (1300, 700), (700, 1300)
HUB = 100
ID = "INT64"

to_gb, check, iso_gb = G.to_gb, G.check, G.iso_gb


@pytest.fixture(scope="module")
def gb():
    import graphblas_amd

    t0 = time.perf_counter()
    yield graphblas_amd
    graphblas_amd.set_knob("grid_cap", 0)
    print(f"\ntest_grid_sweeps_gpu.py: {time.perf_counter() - t0:.1f} s")


# ---------------------------------------------------------------------- the cases and their caps
_CASES = {}   # name -> (prepare, caps): prepare(gb) returns the callable that runs and checks
_DONE = set()  # cases whose cap-1 run has finished in this process


def _run(gb, name, caps):
    run = _CASES[name][0](gb)
    for k in caps:
        gb.set_knob("grid_cap", k)
        try:
            run()
        except AssertionError as e:
            raise AssertionError(f"grid_cap={k}: {e}") from e
        finally:
            gb.set_knob("grid_cap", 0)
        if k == 1:
            _DONE.add(name)


def sweep(caps=CAPS):
    def deco(prepare):
        name = prepare.__name__
        _CASES[name] = (prepare, caps)

        @pytest.mark.gpu
        def test(gb):
            _run(gb, name, caps)

        test.__name__ = name
        test.__doc__ = prepare.__doc__
        return test

    return deco


# ---------------------------------------------------------------------- operands
def _lengths(nr, nc, rng):
    avg = (20000 - 700 - 192) / (nr - 270 - 4)
    lens = rng.integers(0, int(2 * avg) + 1, nr)
    mid = nr // 2 - 65
    lens[:70] = lens[-70:] = lens[mid:mid + 130] = 0
    lens[HUB] = 700
    lens[200:203] = 63, 64, 65
    return lens


@functools.lru_cache(maxsize=None)
def mat(dt, shape, key):
    """the structured matrix of the module docstring (shared: never written to)"""
    rng = G._rng("sweeps", dt, shape, key)
    nr, nc = shape
    p = np.zeros(shape, bool)
    for i, n in enumerate(_lengths(nr, nc, rng)):
        p[i, rng.choice(nc, n, replace=False)] = True
    v = np.where(p, G.draw(dt, rng, p.size).reshape(shape), dm.NP[dt](0))
    p.setflags(write=False)
    v.setflags(write=False)
    return p, v


@functools.lru_cache(maxsize=None)
def vec(dt, n, kind, key):
    """kind: half, sparse (1 in 50), full, empty"""
    rng = G._rng("sweeps-vec", dt, n, kind, key)
    p = rng.random(n) < {"half": 0.5, "sparse": 0.02, "full": 2.0, "empty": -1.0}[kind]
    v = np.where(p, G.draw(dt, rng, n), dm.NP[dt](0))
    p.setflags(write=False)
    v.setflags(write=False)
    return p, v


def mask_of(shape, key, density=0.5):
    """a mask with stored false values"""
    rng = G._rng("sweeps-mask", shape, key)
    p = rng.random(shape) < density
    return p, p & (rng.random(shape) < 0.5)


def mat_mask(shape, key):
    rng = G._rng("sweeps-mmask", shape, key)
    p = mat("BOOL", shape, key)[0]
    return p, p & (rng.random(shape) < 0.5)


# (model keywords, how the device call binds them); m: the device mask
WB = [("accum", dict(accum="plus"), lambda gb, m: dict(accum=gb.binary.plus)),
      ("S replace", dict(mask_struct=True, replace=True), lambda gb, m: dict(mask=m.S, replace=True)),
      ("V accum", dict(accum="plus"), lambda gb, m: dict(mask=m.V, accum=gb.binary.plus)),
      ("~S replace accum", dict(mask_struct=True, mask_comp=True, replace=True, accum="plus"),
       lambda gb, m: dict(mask=~m.S, replace=True, accum=gb.binary.plus)),
      ("~V", dict(mask_comp=True), lambda gb, m: dict(mask=~m.V))]


def wb_model(C, T, M, tag, kw, **more):
    return dm.write_back(C, T, mask=None if tag == "accum" else M, **kw, **more)


# ---------------------------------------------------------------------- write-back
@sweep(CAPS_SUM)
def test_write_back_vector(gb):
    """k_vec_merge / k_vec_restore / the mask kernels: every mask kind, replace, plus, and an
    accumulator of another type than C; C and T of every fill"""
    jobs = []
    fills = [("half", "half"), ("sparse", "full"), ("full", "sparse"), ("half", "empty"), ("empty", "half")]
    for n in (NVEC, 65):
        M = mask_of((n,), "wbv")
        for k, (ck, tk) in enumerate(fills):
            C, T = vec(ID, n, ck, "wb C"), vec("INT32", n, tk, "wb T")
            tag, kw, bind = WB[k % len(WB)]
            jobs.append((C, T, M, bind, None, wb_model(C, T, M, tag, kw), ID, f"n={n} C {ck} T {tk} {tag}"))
        T = vec("INT32", n, "half", "wb T")
        for k, (tag, kw, bind) in enumerate(WB):
            C = vec(ID, n, "half", "wb C")
            jobs.append((C, T, M, bind, None, wb_model(C, T, M, tag, kw), ID, f"n={n} {tag}"))
        p = vec(ID, n, "half", "wb iso")[0]
        Ciso = (p, np.where(p, np.int64(3), np.int64(0)))
        jobs.append((Ciso, T, M, WB[1][2], 3, wb_model(Ciso, T, M, *WB[1][:2]), ID, f"n={n} iso C"))
    Ca, Ta, Ma = G.accum_case(ID, (NVEC,), "sweeps")
    want = dm.write_back(Ca, Ta, mask=Ma, mask_struct=True, mask_comp=True, accum="plus", accum_dtype="FP64")
    T32 = vec("INT32", NVEC, "half", "wb T")  # a third type: T alone is cast straight to C's type
    want32 = dm.write_back(Ca, T32, mask=Ma, mask_struct=True, accum="plus", accum_dtype="FP64")

    def run():
        for C, T, M, bind, iso, want_, dt, what in jobs:
            c = iso_gb(gb, C[0], iso, dt)[0] if iso is not None else to_gb(gb, C)
            c(**bind(gb, to_gb(gb, M))) << to_gb(gb, T).apply(gb.unary.identity)
            check(c, want_, dt, what="vector write-back " + what)
        c = to_gb(gb, Ca)
        c(~to_gb(gb, Ma).S, gb.binary.plus["FP64"]) << to_gb(gb, Ta).apply(gb.unary.identity)
        check(c, want, ID, what="vector write-back plus[FP64] into INT64")
        c = to_gb(gb, Ca)
        c(to_gb(gb, Ma).S, gb.binary.plus["FP64"]) << to_gb(gb, T32).apply(gb.unary.identity)
        check(c, want32, ID, what="vector write-back plus[FP64] of INT32 into INT64")

    return run


@sweep()
def test_write_back_matrix(gb):
    """the matrix merge (flags, row pointer, placement) behind apply and behind the object assign"""
    C, T, M = mat(ID, SHAPE, "wb C"), mat("INT32", SHAPE, "wb T"), mat_mask(SHAPE, "wb M")
    wants = [wb_model(C, T, M, tag, kw) for tag, kw, _ in WB]
    Tf = (T[0], T[1].astype(np.float64) * 0.5)
    want_f = dm.write_back(C, Tf, mask=M, mask_struct=True, accum="plus", accum_dtype="FP64")
    want_3 = dm.write_back(C, T, mask=M, mask_struct=True, accum="plus", accum_dtype="FP64")  # INT32 T

    def run():
        t, m = to_gb(gb, T), to_gb(gb, M)
        for k, ((tag, kw, bind), want) in enumerate(zip(WB, wants)):
            c = to_gb(gb, C)
            c(**bind(gb, m)) << (t.apply(gb.unary.identity) if k % 2 else t)
            check(c, want, ID, what=f"matrix write-back {tag}")
        c = to_gb(gb, C)
        c(m.S, gb.binary.plus["FP64"]) << to_gb(gb, Tf)
        check(c, want_f, ID, what="matrix write-back plus[FP64] into INT64")
        c = to_gb(gb, C)
        c(m.S, gb.binary.plus["FP64"]) << t
        check(c, want_3, ID, what="matrix write-back plus[FP64] of INT32 into INT64")

    return run


# ---------------------------------------------------------------------- gb_ops.hip
@sweep(CAPS_SUM)
def test_ewise_and_apply_vector(gb):
    pairs = [("half", "half"), ("sparse", "full"), ("empty", "half")]
    jobs = []
    for n in (NVEC, 65):
        for ak, bk in pairs:
            A, B = vec(ID, n, ak, "ew a"), vec(ID, n, bk, "ew b")
            jobs.append((A, B, [dm.ewise(kind, "plus", ID, A, B) for kind in ("mult", "add")]))
    A = vec(ID, NVEC, "half", "ew a")
    Biso = (vec(ID, NVEC, "sparse", "ew b")[0], None)
    Biso = (Biso[0], np.where(Biso[0], np.int64(3), np.int64(0)))
    iso_wants = [dm.ewise(kind, "minus", ID, A, Biso) for kind in ("mult", "add")]
    three = np.int64(3)
    ap_wants = [dm.apply("ainv", ID, A), dm.apply("minus", ID, A, left=three)]

    def run():
        for A_, B_, wants in jobs:
            a, b = to_gb(gb, A_), to_gb(gb, B_)
            for kind, want in zip(("mult", "add"), wants):
                check(getattr(a, f"ewise_{kind}")(b, gb.binary.plus).new(), want, ID, what=f"vector ewise_{kind}")
        a, b = to_gb(gb, A), iso_gb(gb, Biso[0], 3, ID)[0]
        for kind, want in zip(("mult", "add"), iso_wants):
            check(getattr(a, f"ewise_{kind}")(b, gb.binary.minus).new(), want, ID, what=f"vector ewise_{kind} iso")
        check(a.apply(gb.unary.ainv).new(), ap_wants[0], ID, what="vector apply ainv")
        check(a.apply(gb.binary.minus, left=three).new(), ap_wants[1], ID, what="vector apply bind-first")

    return run


@sweep()
def test_ewise_apply_transpose_matrix(gb):
    A, B = mat(ID, SHAPE, "ew A"), mat(ID, SHAPE, "ew B")
    At = dm.transpose(A)
    wants = {kind: dm.ewise(kind, "plus", ID, A, B) for kind in ("mult", "add")}
    three = np.int64(3)
    ap = [dm.apply("abs", ID, A), dm.apply("minus", ID, A, left=three)]
    Mt = mat_mask(SHAPE_T, "tr M")
    Ct = mat(ID, SHAPE_T, "tr C")
    want_t = dm.write_back(Ct, At, mask=Mt, mask_struct=True, accum="plus")

    def run():
        a, b = to_gb(gb, A), to_gb(gb, B)
        for kind, want in wants.items():
            check(getattr(a, f"ewise_{kind}")(b, gb.binary.plus).new(), want, ID, what=f"matrix ewise_{kind}")
        check(a.apply(gb.unary.abs).new(), ap[0], ID, what="matrix apply abs")
        check(a.apply(gb.binary.minus, left=three).new(), ap[1], ID, what="matrix apply bind-first")
        at = a.T.new()
        check(at, At, ID, what="A.T.new()")
        check(at.T.ewise_mult(b, gb.binary.plus).new(), wants["mult"], ID, what="(A.T).T * B: the CSC build")
        c = to_gb(gb, Ct)
        c(to_gb(gb, Mt).S, gb.binary.plus) << a.T
        check(c, want_t, ID, what="C(M.S, plus) << A.T")

    return run


@sweep(CAPS_SUM)
def test_reduce(gb):
    """to a scalar (k_reduce_partial), to rows and to columns; float plus within n eps sum|x|"""
    vs = [(mon, dt, G.reduce_input(mon, dt, (NVEC,), "sweeps", 0.5)) for mon, dt in
          (("plus", ID), ("min", "INT32"), ("plus", "FP64"), ("bxor", "UINT16"))]
    A = mat(ID, SHAPE, "red A")
    A32 = (A[0], dm.cast(A[1], "INT32"))
    At, At32 = dm.transpose(A), dm.transpose(A32)

    def run():
        for mon, dt, V in vs:
            got = G.scalar_value(to_gb(gb, V).reduce(getattr(gb.monoid, mon)).new(), dt)
            G.check_reduced(got, V[1][V[0]], mon, dt, f"reduce {mon}[{dt}] {NVEC}", verbose=True)
        a, a32 = to_gb(gb, A), to_gb(gb, A32)
        got = G.scalar_value(a.reduce_scalar(gb.monoid.plus).new(), ID)
        G.check_reduced(got, A[1][A[0]], "plus", ID, "reduce_scalar plus")
        G.check_reduced_vector(a.reduce_rowwise(gb.monoid.plus).new(), A, "plus", ID, "reduce_rowwise plus")
        G.check_reduced_vector(a32.reduce_rowwise(gb.monoid.min).new(), A32, "min", "INT32", "reduce_rowwise min")
        G.check_reduced_vector(a.reduce_columnwise(gb.monoid.plus).new(), At, "plus", ID, "reduce_columnwise plus")
        G.check_reduced_vector(a32.reduce_columnwise(gb.monoid.max).new(), At32, "max", "INT32",
                               "reduce_columnwise max")

    return run


@sweep(CAPS_SUM)
def test_scalar_assign(gb):
    """w<m> = s and w = s on bitmaps (k_assign_mask_words and its kin), C<M> = s on a matrix"""
    seven = np.int64(7)
    jobs = []
    for n in (NVEC, 65):
        W, M = vec(ID, n, "half", "sa W"), mask_of((n,), "sa M", 0.3)
        jobs.append((W, M, "V", dm.assign_vec(W, seven, mask=M)))
        jobs.append((W, M, "S", dm.assign_vec(W, seven, mask=M, mask_struct=True)))
        jobs.append((W, M, "~S replace", dm.assign_vec(W, seven, mask=M, mask_struct=True, mask_comp=True,
                                                       replace=True)))
        jobs.append((W, M, "none", dm.assign_vec(W, seven)))
        E = vec(ID, n, "empty", "sa W")
        jobs.append((E, M, "V", dm.assign_vec(E, seven, mask=M)))
    C, Mm = mat(ID, SHAPE, "sa C"), mat_mask(SHAPE, "sa M")
    want_m = dm.assign(C, seven, mask=Mm, mask_struct=True)
    want_v = dm.assign(C, seven, mask=Mm, accum="plus")
    # GrB_assign of a vector at an index list: the region is cleared first (k_clear_region)
    rng = G._rng("sweeps-assign-list")
    Wl, Ml = vec(ID, NVEC, "half", "sa W"), mask_of((NVEC,), "sa M", 0.3)
    K = rng.permutation(NVEC)[:30000].astype(np.int64)
    ul = vec(ID, K.size, "half", "sa u")
    want_l = dm.assign_vec(Wl, ul, K, mask=Ml, mask_struct=True)

    def run():
        w = to_gb(gb, Wl)
        w(mask=to_gb(gb, Ml).S)[K] << to_gb(gb, ul)
        check(w, want_l, ID, what="w(m.S)[K] << u")
        for W, M, kind, want in jobs:
            w, m = to_gb(gb, W), to_gb(gb, M)
            if kind == "none":
                w[:] = 7
            elif kind == "V":
                w(mask=m.V)[:] = 7
            elif kind == "S":
                w(mask=m.S)[:] = 7
            else:
                w(mask=~m.S, replace=True)[:] = 7
            check(w, want, ID, what=f"vector scalar assign {kind} n={W[0].size}")
        m = to_gb(gb, Mm)
        c = to_gb(gb, C)
        c(mask=m.S)[:, :] = 7
        check(c, want_m, ID, what="matrix scalar assign M.S")
        c = to_gb(gb, C)
        c(mask=m.V, accum=gb.binary.plus)[:, :] = 7
        check(c, want_v, ID, what="matrix scalar assign M.V plus")

    return run


# ---------------------------------------------------------------------- gb_object.hip
@sweep(CAPS_SUM)
def test_build_export_import(gb):
    """from_coo of 60000 unsorted tuples with duplicates under plus, the bitmap vector's to_coo, the
    CSR import with its sortedness check and the CSR export"""
    rng = G._rng("sweeps-build")
    n = 60000
    A = mat(ID, SHAPE, "build")
    pr, pc = np.nonzero(A[0])
    pick = rng.integers(0, pr.size, n)  # duplicates of the structured matrix' own positions
    r, c = pr[pick], pc[pick]
    vals = rng.integers(-100, 100, n)
    want = dm.build(SHAPE, (r, c), vals, "plus", ID)
    flat = (r * SHAPE[1] + c) % NVEC
    want_v = dm.build((NVEC,), (flat,), vals, "plus", ID)
    indptr = np.concatenate([[0], np.cumsum(A[0].sum(axis=1))])
    unsorted = pc.copy()
    p0 = indptr[HUB]
    ca, cb = int(pc[p0 + 300]), int(pc[p0 + 301])
    unsorted[p0 + 300], unsorted[p0 + 301] = cb, ca  # a jumbled row is sorted: the values follow their columns
    jv = A[1].copy()
    jv[HUB, ca], jv[HUB, cb] = A[1][HUB, cb], A[1][HUB, ca]
    Aj = A[0], jv

    def run():
        check(gb.Matrix.from_coo(r, c, vals, dtype=ID, nrows=SHAPE[0], ncols=SHAPE[1], dup_op=gb.binary.plus), want,
              ID, what="Matrix.from_coo plus")
        check(gb.Vector.from_coo(flat, vals, dtype=ID, size=NVEC, dup_op=gb.binary.plus), want_v, ID,
              what="Vector.from_coo plus")
        m = gb.Matrix.from_csr(indptr, pc, A[1][pr, pc], dtype=ID, ncols=SHAPE[1])
        check(m, A, ID, what="CSR import")
        ap, ai, ax = m.to_csr()
        assert np.array_equal(ap, indptr) and np.array_equal(ai, pc) and np.array_equal(ax, A[1][pr, pc])
        check(gb.Matrix.from_csr(indptr, unsorted, A[1][pr, pc], dtype=ID, ncols=SHAPE[1]), Aj, ID,
              what="CSR import of a jumbled row")

    return run


@sweep()
def test_elements_and_resize(gb):
    A = mat(ID, SHAPE, "elem")
    B = dm.remove_element(A, (HUB, 350))
    steps = [("remove", (HUB, 350), B)]
    Bs = dm.set_element(B, (HUB, 350), -77)
    steps.append(("set", (HUB, 350), Bs))
    Bt = dm.set_element(Bs, (HUB + 1, 5), -78) if not A[0][HUB + 1, 5] else dm.set_element(Bs, (0, 5), -78)
    steps.append(("set", (HUB + 1, 5) if not A[0][HUB + 1, 5] else (0, 5), Bt))
    shrink = dm.resize(Bt, (SHAPE[0] - 100, SHAPE[1] - 9))
    grow = dm.resize(shrink, (SHAPE[0] + 64, SHAPE[1] + 5))
    V = vec(ID, NVEC, "half", "elem")
    vshrink, vgrow = dm.resize(V, NVEC - 4000), dm.resize(dm.resize(V, NVEC - 4000), NVEC + 100)
    # another value into an iso object: its one value is expanded first (gb_expand_iso)
    Aiso = (A[0], np.where(A[0], np.int64(3), np.int64(0)))
    Aiso_set = dm.set_element(Aiso, (HUB, 350), -77)
    p = V[0]
    Viso = (p, np.where(p, np.int64(3), np.int64(0)))
    i_in = int(np.flatnonzero(p)[-1])
    Viso_set = dm.set_element(Viso, i_in, -77)

    def run():
        ai = iso_gb(gb, A[0], 3, ID)[0]
        ai[HUB, 350] = -77
        check(ai, Aiso_set, ID, what="set another value in an iso matrix")
        vi = iso_gb(gb, p, 3, ID)[0]
        vi[i_in] = -77
        check(vi, Viso_set, ID, what="set another value in an iso vector")
        a = to_gb(gb, A)
        for what, ij, want in steps:
            if what == "remove":
                del a[ij]
            else:
                a[ij] = int(want[1][ij])
            check(a, want, ID, what=f"{what} {ij}")
        a.resize(*shrink[0].shape)
        check(a, shrink, ID, what="resize down")
        a.resize(*grow[0].shape)
        check(a, grow, ID, what="resize up")
        v = to_gb(gb, V)
        v.resize(NVEC - 4000)
        check(v, vshrink, ID, what="vector resize down")
        v.resize(NVEC + 100)
        check(v, vgrow, ID, what="vector resize up")

    return run


# ---------------------------------------------------------------------- gb_prim.hip
@sweep((1,))
def test_wave_tile_scan_hands_over(gb):
    """133125 rows: at cap 1 the four waves of the wave-tile scans (scanw, gb_exclusive_scan_u8)
    each own many tiles, so toff[t] is handed from a wave's tile to its next one"""
    shape = (133125, 64)
    A, B = G.ragged(*shape, "INT32", "a"), G.ragged(*shape, "INT32", "b")
    wants = {kind: dm.ewise(kind, "plus", "INT32", A, B) for kind in ("mult", "add")}
    At = dm.transpose(A)

    def run():
        with G._knobs(gb, scan_u8=0):
            a, b = to_gb(gb, A), to_gb(gb, B)
            check(a, A, "INT32", what="build 133125 rows")
            for kind, want in wants.items():
                check(getattr(a, f"ewise_{kind}")(b, gb.binary.plus).new(), want, "INT32", what=f"ewise_{kind} 133125")
            at = a.T.new()
            check(at, At, "INT32", what="A.T.new() 133125")
            check(at.T.new(), A, "INT32", what="transpose back 133125")
            check(a.select(">", 0).new(), (A[0] & (A[1] > 0), np.where(A[1] > 0, A[1], 0)), "INT32",
                  what="select 133125")

    return run


@sweep()
def test_chunked_scan_carry(gb):
    """scan_chunk = 20000 with scan_u8 = 1: hipCUB scans in chunks, each later chunk adds the
    previous chunk's total (k_add_carry; by default only from 2^30 items)"""
    rng = G._rng("sweeps-carry")
    n = 60000
    r, c = rng.integers(0, SHAPE[0], n), rng.integers(0, SHAPE[1], n)
    vals = rng.integers(-100, 100, n)
    want = dm.build(SHAPE, (r, c), vals, "plus", ID)
    V = vec(ID, NVEC, "half", "carry")
    I = rng.permutation(NVEC)[:50000]
    want_x = dm.extract_vec(V, I)

    def run():
        with G._knobs(gb, scan_u8=1, scan_chunk=20000):
            check(gb.Matrix.from_coo(r, c, vals, dtype=ID, nrows=SHAPE[0], ncols=SHAPE[1], dup_op=gb.binary.plus),
                  want, ID, what="from_coo, chunked scans")
            check(to_gb(gb, V)[I].new(), want_x, ID, what="vector extract, chunked scans")

    return run


# ---------------------------------------------------------------------- select, apply with index
def _selected(A, z):
    keep = A[0] & z[0] & (z[1] != 0)
    return keep, np.where(keep, A[1], A[1].dtype.type(0))


@sweep()
def test_select(gb):
    A, V = mat(ID, SHAPE, "sel"), vec(ID, NVEC, "half", "sel")
    wants = [_selected(A, im.index_apply(A, "tril", None, -3)), _selected(A, im.index_apply(A, "valuegt", ID, 0)),
             _selected(A, im.index_apply(A, "colgt", None, 300))]
    vwants = [_selected(V, im.index_apply(V, "rowle", None, NVEC // 2)),
              _selected(V, im.index_apply(V, "valuelt", ID, 1))]

    def run():
        a, v = to_gb(gb, A), to_gb(gb, V)
        check(a.select("tril", -3).new(), wants[0], ID, what="select tril")
        check(a.select(">", 0).new(), wants[1], ID, what="select >")
        check(a.select("col>", 300).new(), wants[2], ID, what="select col>")
        check(v.select("index<=", NVEC // 2).new(), vwants[0], ID, what="vector select index<=")
        check(v.select("<", 1).new(), vwants[1], ID, what="vector select <")

    return run


@sweep()
def test_apply_index_unary(gb):
    A, V = mat(ID, SHAPE, "idx"), vec(ID, NVEC, "half", "idx")
    cases = [(A, "rowindex", ID, 5), (A, "diagindex", "INT32", -2), (A, "valuegt", ID, 1), (A, "tril", None, 0),
             (V, "rowindex", ID, -100), (V, "valuele", ID, 2)]
    wants = [im.index_apply(X, op, t, y) for X, op, t, y in cases]
    want_t = im.index_apply(dm.transpose(A), "rowindex", ID, 1)

    def run():
        dev = {id(A): to_gb(gb, A), id(V): to_gb(gb, V)}
        for (X, op, t, y), want in zip(cases, wants):
            typed = getattr(gb.indexunary, op)
            typed = typed if t is None else typed[t]
            check(dev[id(X)].apply(typed, y).new(), want, im.result_dtype(op, t), what=f"apply {op}[{t}] y={y}")
        check(dev[id(A)].T.apply(gb.indexunary.rowindex[ID], 1).new(), want_t, ID, what="A.T apply rowindex")

    return run


# ---------------------------------------------------------------------- diag, reshape, flatten
@sweep()
def test_diag_reshape_flatten(gb):
    A = mat(ID, SHAPE, "rix")
    V = vec(ID, 2500, "half", "rix")
    diag_wants = {k: rm.diag_vector(A, k) for k in (0, -200, 150)}
    vdiag = {k: rm.diag_matrix(V, k) for k in (0, 3, -2)}
    resh = {(new, order): rm.reshape(A, new, order) for new, order in
            ((SHAPE_T, "rowwise"), ((2600, 350), "columnwise"), ((130, 7000), "rowwise"))}
    flat = {order: rm.flatten(A, order) for order in ("rowwise", "columnwise")}

    def run():
        a, v = to_gb(gb, A), to_gb(gb, V)
        for k, want in diag_wants.items():
            check(a.diag(k), want, ID, what=f"A.diag({k})")
        for k, want in vdiag.items():
            check(v.diag(k), want, ID, what=f"v.diag({k})")
        for (new, order), want in resh.items():
            check(a.ss.reshape(new, order=order), want, ID, what=f"reshape {new} {order}")
        for order, want in flat.items():
            f = a.ss.flatten(order)
            check(f, want, ID, what=f"flatten {order}")
            check(f.ss.reshape(*SHAPE, order), A, ID, what=f"flatten {order} and back")

    return run


# ---------------------------------------------------------------------- concat / split
@sweep()
def test_concat_split(gb):
    """a 3 x 2 grid whose column cut goes through the hub row; a vector cut inside words"""
    A = mat(ID, SHAPE, "tile")
    chunks = [[90, 500, 710], [333, 367]]
    want = tm.split(A, chunks)
    V = vec(ID, NVEC, "half", "tile")
    vchunks = [[1000, 33001, 36000]]
    vwant = tm.split(V, vchunks)
    # 20 x 13 iso tiles: more tile records than one block of the iso test has threads
    Aiso = (A[0], np.where(A[0], np.int64(3), np.int64(0)))
    many = [[65] * 20, [54] * 12 + [52]]
    want_many = tm.split(Aiso, many)
    # an iso piece between two others: its value is spread over its part of the result
    p2 = vec(ID, 33001, "half", "tile iso")[0]
    Viso = (p2, np.where(p2, np.int64(3), np.int64(0)))
    want_cat = tm.concat([vwant[0], Viso, vwant[2]], ID)

    def run():
        ai = iso_gb(gb, A[0], 3, ID)[0]
        tiles = ai.ss.split(many)
        for i, j in ((0, 0), (1, 12), (10, 6), (19, 12)):
            check(tiles[i][j], want_many[i][j], ID, what=f"iso tile {i}x{j} of 20 x 13")
        check(gb.ss.concat(tiles), Aiso, ID, what="concat of 260 iso tiles")
        pieces = [to_gb(gb, vwant[0]), iso_gb(gb, p2, 3, ID)[0], to_gb(gb, vwant[2])]
        check(gb.ss.concat(pieces), want_cat, ID, what="vector concat with an iso piece")
        a = to_gb(gb, A)
        tiles = a.ss.split(chunks)
        for i, (trow, wrow) in enumerate(zip(tiles, want)):
            for j, (t, w) in enumerate(zip(trow, wrow)):
                check(t, w, ID, what=f"split tile {i}x{j}")
        check(gb.ss.concat(tiles), A, ID, what="concat(split)")
        v = to_gb(gb, V)
        parts = v.ss.split(vchunks[0])
        for i, (t, w) in enumerate(zip(parts, vwant)):
            check(t, w, ID, what=f"vector piece {i}")
        check(gb.ss.concat(parts), V, ID, what="vector concat(split)")

    return run


# ---------------------------------------------------------------------- eWiseUnion
@sweep(CAPS_SUM)
def test_ewise_union(gb):
    A, B = mat(ID, SHAPE, "uni A"), mat(ID, SHAPE, "uni B")
    want = um.ewise_union("minus", ID, A, 10, B, 20)
    U, V = vec(ID, NVEC, "half", "uni u"), vec(ID, NVEC, "sparse", "uni v")
    vwant = um.ewise_union("minus", ID, U, 10, V, 20)
    want_t = um.ewise_union("minus", ID, dm.transpose(A), 10, dm.transpose(B), 20)

    def run():
        a, b = to_gb(gb, A), to_gb(gb, B)
        check(a.ewise_union(b, gb.binary.minus[ID], 10, 20).new(), want, ID, what="matrix eWiseUnion")
        check(a.T.ewise_union(b.T, gb.binary.minus[ID], 10, 20).new(), want_t, ID, what="A.T, B.T eWiseUnion")
        check(to_gb(gb, U).ewise_union(to_gb(gb, V), gb.binary.minus[ID], 10, 20).new(), vwant, ID,
              what="vector eWiseUnion")

    return run


# ---------------------------------------------------------------------- subassign, Row / Col assign
@sweep()
def test_subassign(gb):
    rng = G._rng("sweeps-subassign")
    C = mat(ID, SHAPE, "sub C")
    I = np.r_[HUB, rng.permutation(SHAPE[0])[:399]].astype(np.int64)
    I = I[np.sort(np.unique(I, return_index=True)[1])]
    J = rng.permutation(SHAPE[1])[:300].astype(np.int64)
    ap = rng.random((I.size, J.size)) < 0.1
    A = ap, np.where(ap, G.draw(ID, rng, ap.size).reshape(ap.shape), np.int64(0))
    M = mask_of(ap.shape, "sub M")
    wants = [sam.subassign(C, A, I, J), sam.subassign(C, A, I, J, mask=M, mask_struct=True, replace=True, accum="plus"),
             sam.subassign(C, A, I, J, mask=M, mask_comp=True)]
    Js = np.sort(J)  # a sorted J takes k_sa_cols, an unsorted one the key sort
    wants += [sam.subassign(C, A, I, Js, mask=M, mask_struct=True),
              sam.subassign(C, np.int64(4), I, J, mask=M, mask_struct=True)]
    Jr = rng.permutation(SHAPE[1])[:400].astype(np.int64)
    u = vec(ID, Jr.size, "half", "sub u")
    Mrow, Mrs = mask_of((SHAPE[1],), "sub Mrow"), mask_of((Jr.size,), "sub Mrs")
    row_wants = [sam.row_assign(C, u, HUB, Jr, mask=Mrow, mask_struct=True, replace=True),
                 sam.row_subassign(C, u, HUB, Jr, mask=Mrs, accum="plus")]
    Ic = rng.permutation(SHAPE[0])[:900].astype(np.int64)
    uc = vec(ID, Ic.size, "half", "sub uc")
    Mcol, Mcs = mask_of((SHAPE[0],), "sub Mcol"), mask_of((Ic.size,), "sub Mcs")
    col_wants = [sam.col_assign(C, uc, Ic, 5, mask=Mcol, accum="plus"),
                 sam.col_subassign(C, uc, Ic, 5, mask=Mcs, mask_struct=True, replace=True)]
    W = vec(ID, NVEC, "half", "sub W")
    K = rng.permutation(NVEC)[:30000].astype(np.int64)
    uk = vec(ID, K.size, "half", "sub uk")
    Mk = mask_of((K.size,), "sub Mk")
    vwant = sam.subassign(W, uk, K, None, mask=Mk, mask_struct=True, accum="plus")

    def run():
        a, m = to_gb(gb, A), to_gb(gb, M)
        c = to_gb(gb, C)
        c[I, J] << a
        check(c, wants[0], ID, what="C[I, J] << A")
        c = to_gb(gb, C)
        c[I, J](mask=m.S, replace=True, accum=gb.binary.plus) << a
        check(c, wants[1], ID, what="C[I, J](M.S, replace, plus) << A")
        c = to_gb(gb, C)
        c[I, J](mask=~m.V) << a
        check(c, wants[2], ID, what="C[I, J](~M.V) << A")
        c = to_gb(gb, C)
        c[I, Js](mask=m.S) << a
        check(c, wants[3], ID, what="C[I, sorted J](M.S) << A")
        c = to_gb(gb, C)
        c[I, J](mask=m.S) << 4
        check(c, wants[4], ID, what="C[I, J](M.S) << 4")
        ug = to_gb(gb, u)
        c = to_gb(gb, C)
        c(mask=to_gb(gb, Mrow).S, replace=True)[HUB, Jr] << ug
        check(c, row_wants[0], ID, what="GrB_Row_assign into the hub row")
        c = to_gb(gb, C)
        c[HUB, Jr](mask=to_gb(gb, Mrs).V, accum=gb.binary.plus) << ug
        check(c, row_wants[1], ID, what="GxB_Row_subassign into the hub row")
        ucg = to_gb(gb, uc)
        c = to_gb(gb, C)
        c(mask=to_gb(gb, Mcol).V, accum=gb.binary.plus)[Ic, 5] << ucg
        check(c, col_wants[0], ID, what="GrB_Col_assign")
        c = to_gb(gb, C)
        c[Ic, 5](mask=to_gb(gb, Mcs).S, replace=True) << ucg
        check(c, col_wants[1], ID, what="GxB_Col_subassign")
        w = to_gb(gb, W)
        w[K](mask=to_gb(gb, Mk).S, accum=gb.binary.plus) << to_gb(gb, uk)
        check(w, vwant, ID, what="w[K](m.S, plus) << u")

    return run


# ---------------------------------------------------------------------- extract
@sweep()
def test_extract(gb):
    rng = G._rng("sweeps-extract")
    A = mat(ID, SHAPE, "ext")
    I = np.r_[rng.integers(0, SHAPE[0], 900), HUB, HUB].astype(np.int64)
    J = np.r_[rng.integers(0, SHAPE[1], 500), 3, 3, 3].astype(np.int64)  # repeated columns
    want = dm.extract(A, I, J)
    Js = np.sort(rng.permutation(SHAPE[1])[:400]).astype(np.int64)
    want_s = dm.extract(A, None, Js)
    hubcol = int(np.argmax(A[0].sum(axis=0)))
    Ic = rng.integers(0, SHAPE[0], 1000).astype(np.int64)
    want_c = dm.extract_vec((A[0][:, hubcol], A[1][:, hubcol]), Ic)
    V = vec(ID, NVEC, "half", "ext")
    K = rng.integers(0, NVEC, 40000).astype(np.int64)
    want_v = dm.extract_vec(V, K)
    # through the C ABI a vector is an n x 1 matrix: GrB_Matrix_extract from a vector into a vector
    # converts the bitmap to CSR and the n x 1 result back (gb_bitmap_to_csr, gb_csr_col_to_bitmap)
    Ku = np.ascontiguousarray(K[:20000], np.uint64)
    zero = np.zeros(1, np.uint64)
    want_m = dm.extract_vec(V, K[:20000])

    def run():
        v = to_gb(gb, V)
        w = gb.Vector(ID, Ku.size)
        assert gb.lib.GrB_Matrix_extract(w._h, None, None, v._h, ctypes.c_void_p(Ku.ctypes.data), Ku.size,
                                         ctypes.c_void_p(zero.ctypes.data), 1, None) == 0
        check(w, want_m, ID, what="GrB_Matrix_extract on vectors")
        a = to_gb(gb, A)
        check(a[I, J].new(), want, ID, what="A[I, J] with a repeated J")
        check(a[:, Js].new(), want_s, ID, what="A[:, J] sorted")
        check(a[Ic, hubcol].new(), want_c, ID, what="GrB_Col_extract")
        check(to_gb(gb, V)[K].new(), want_v, ID, what="vector extract")

    return run


# ---------------------------------------------------------------------- kronecker
@sweep()
def test_kronecker(gb):
    """13 x 7 (x) 100 x 100: the product has the shape of the others"""
    rng = G._rng("sweeps-kron")
    ap, bp = rng.random((13, 7)) < 0.45, rng.random((100, 100)) < 0.05
    ap[0] = ap[-1] = False
    bp[:5] = False
    A = ap, np.where(ap, G.draw(ID, rng, ap.size).reshape(ap.shape), np.int64(0))
    B = bp, np.where(bp, G.draw(ID, rng, bp.size).reshape(bp.shape), np.int64(0))
    coo = lambda X: (*np.nonzero(X[0]), X[1][np.nonzero(X[0])])  # noqa: E731
    (wr, wc, wv), zt = kron_model(coo(A), coo(B), ((13, 7), (100, 100)), "times", ID)

    def run():
        got = to_gb(gb, A).kronecker(to_gb(gb, B), gb.binary.times).new()
        assert got.dtype == zt and tuple(got.shape) == SHAPE and got.nvals == wr.size
        r, c, v = got.to_coo()
        assert np.array_equal(r.astype(np.int64), wr) and np.array_equal(c.astype(np.int64), wc), "kron indices"
        assert v.dtype == wv.dtype and np.array_equal(v, wv), "kron values"

    return run


# ---------------------------------------------------------------------- sort
@sweep()
def test_sort(gb):
    A, V = mat(ID, SHAPE, "sort"), vec(ID, NVEC, "half", "sort")
    wc, wp = som.sort_matrix(A, "lt")
    wcc, wpc = som.sort_matrix(A, "gt", columnwise=True)
    vw, vp = som.sort_vector(V, "lt")
    Aiso = (A[0], np.where(A[0], np.int64(3), np.int64(0)))
    wci, wpi = som.sort_matrix(Aiso, "lt")

    def run():
        a = to_gb(gb, A)
        with G._knobs(gb, sort_method=1):  # every row through the segmented radix sort
            C, P = a.ss.sort(gb.binary.lt[ID], "rowwise")
            check(C, wc, ID, what="sort lt C, sort_method=1")
            check(P, wp, "UINT64", what="sort lt P, sort_method=1")
        C, P = iso_gb(gb, A[0], 3, ID)[0].ss.sort(gb.binary.lt[ID], "rowwise")
        check(C, wci, ID, what="iso sort C")
        check(P, wpi, "UINT64", what="iso sort P")
        C, P = a.ss.sort(gb.binary.lt[ID], "rowwise")
        check(C, wc, ID, what="sort lt C")
        check(P, wp, "UINT64", what="sort lt P")
        C, P = a.ss.sort(gb.binary.gt[ID], "columnwise")
        check(C, wcc, ID, what="sort gt columnwise C")
        check(P, wpc, "UINT64", what="sort gt columnwise P")
        w, p = to_gb(gb, V).ss.sort(gb.binary.lt[ID])
        check(w, vw, ID, what="vector sort w")
        check(p, vp, "UINT64", what="vector sort p")

    return run


# ---------------------------------------------------------------------- column words
@sweep()
def test_colbits(gb):
    """the batched BFS on column words against the oracle's levels: CSR -> column words, the masked
    scalar assign V<Q> = d, the steps, and column words -> CSR behind to_coo"""
    import test_colbits as CB

    Gr = O.rmat(11, 16, 42)
    n = Gr.nrows
    r, c, _ = Gr.to_coo()
    deg = np.diff(Gr.indptr)
    roots = np.flatnonzero(deg > 0)[::97][:8].copy()  # 8 rows of INT32: the four-row layer kernel
    roots[0] = int(np.argmax(deg))
    levels = [O.bfs_levels(Gr, int(s))[0] for s in roots]
    # single calls against the oracle's GrB_mxm, as test_colbits_mxm_vs_oracle: 13 x 1300 with 845
    # entries (CSR -> column words over more than one block), a complemented mask with replace
    rng = np.random.default_rng(20)
    k, m = 12, 1300
    Ao, Bo = CB._rand(rng, k, m, 0.05, iso=True), CB._rand(rng, m, m, 0.01, iso=True)
    Mo = CB._rand(rng, k, m, 0.3)  # bool values, some false
    ref = O.mxm(O.Csr.empty(k, m, "BOOL"), Ao, Bo, ("LOR", "LAND", "BOOL"), mask=Mo, mask_struct=True,
                mask_comp=True, replace=True)
    # the masked scalar assign, as test_colbits_assign_vs_numpy: structural, then by value
    mr, mc, mv = Mo.to_coo()
    exp, have = np.zeros((k, m), np.int32), np.zeros((k, m), bool)
    exp[0, 3], have[0, 3] = 11, True
    exp[mr, mc], have[mr, mc] = 5, True
    exp[mr[mv], mc[mv]] = 2
    want_c = have, exp
    pf = np.zeros((k, m), bool)
    rr, rc, _ = ref.to_coo()
    pf[rr, rc] = True
    vf = pf.copy()
    pf[mr, mc], vf[mr, mc] = True, False
    want_f = pf, vf

    def run():
        A = gb.Matrix.from_coo(r, c, True, nrows=n, ncols=n)
        for direction, more in ((0, {}), (1, {}), (2, {}), (1, dict(xhot=2, xhot_cols=300)), (0, dict(colbits_eager=1))):
            with G._knobs(gb, colbits=1, colbits_direction=direction, **more):
                got, _ = CB._msbfs(gb, A, roots, n)
            for i, lev in enumerate(levels):
                assert np.array_equal(got[i], lev), f"direction {direction} {more} root {roots[i]}"
        Ag, Bg, Mg = CB._gbm(gb, Ao, True), CB._gbm(gb, Bo, True), CB._gbm(gb, Mo)
        Cg = gb.Matrix("BOOL", k, m)
        C = gb.Matrix("INT32", k, m)
        C[0, 3] = 11
        with G._knobs(gb, colbits=1):
            Cg(~Mg.S, replace=True) << Ag.mxm(Bg, gb.semiring.lor_land["BOOL"])
            _same_as_oracle(Cg, ref, "column-word mxm, ~M.S replace")
            Cg(Mg.S)[:, :] = False  # into the iso product: its one value is spread first
            check(Cg, want_f, "BOOL", what="column-word scalar assign into an iso matrix")
            C(Mg.S)[:, :] = 5
            C(Mg.V)[:, :] = 2
            check(C, want_c, "INT32", what="column-word scalar assign M.S then M.V")
        q, Q = G.colbits_q(gb)
        check(q, Q, "BOOL", what="column words -> CSR")
        q, _ = G.colbits_q(gb)
        check(q.T.new(), dm.transpose(Q), "BOOL", what="column words .T")

    return run


# ---------------------------------------------------------------------- products
def _csr(X, dt):
    r, c = np.nonzero(X[0])
    return O.Csr.from_coo(r, c, X[1][r, c], nrows=X[0].shape[0], ncols=X[0].shape[1], dtype=dt)


def _small(shape, key):
    p = mat("BOOL", shape, key)[0]
    rng = G._rng("sweeps-small", shape, key)
    return p, np.where(p, rng.integers(-3, 4, shape), 0).astype(np.int64)


def _same_as_oracle(got, ref, what):
    r, c, v = got.to_coo()
    er, ec, ev = ref.to_coo()
    assert got.nvals == er.size, f"{what}: nvals {got.nvals}, expected {er.size}"
    assert np.array_equal(r.astype(np.int64), er) and np.array_equal(c.astype(np.int64), ec), f"{what}: indices"
    assert v.dtype == ev.dtype and np.array_equal(v, ev), f"{what}: values"


@sweep()
def test_mxm(gb):
    """ESC (spgemm_method = 1), the hash default, and the masked dot (default and dot_method = 1)"""
    A, B = _small(SHAPE, "mxm A"), _small(SHAPE_T, "mxm B")
    M = _small((SHAPE[0], SHAPE[0]), "mxm M")
    Ao, Bo, Mo = _csr(A, ID), _csr(B, ID), _csr(M, ID)
    empty = O.Csr.empty(SHAPE[0], SHAPE[0], ID)
    full = {sr: O.mxm(empty, Ao, Bo, sr) for sr in (("PLUS", "TIMES", ID), ("MIN", "PLUS", ID))}
    masked = {sr: O.mxm(empty, Ao, Bo, sr, mask=Mo, mask_struct=True) for sr in full}
    names = {("PLUS", "TIMES", ID): "plus_times", ("MIN", "PLUS", ID): "min_plus"}

    def run():
        a, b, m = to_gb(gb, A), to_gb(gb, B), to_gb(gb, M)
        for key, name in names.items():
            sr = getattr(gb.semiring, name)[ID]
            with G._knobs(gb, spgemm_method=1):
                _same_as_oracle(a.mxm(b, sr).new(), full[key], f"mxm esc {name}")
            _same_as_oracle(a.mxm(b, sr).new(), full[key], f"mxm {name}")
            _same_as_oracle(a.mxm(b, sr).new(mask=m.S), masked[key], f"masked mxm {name}")
            with G._knobs(gb, dot_method=1):
                _same_as_oracle(a.mxm(b, sr).new(mask=m.S), masked[key], f"masked mxm dot_method=1 {name}")
            with G._knobs(gb, dot_method=1, dot_group=1):  # a thread per mask entry
                _same_as_oracle(a.mxm(b, sr).new(mask=m.S), masked[key], f"masked mxm dot_group=1 {name}")
            with G._knobs(gb, dot_yblk=4):  # the two-sided dot's tasks ordered by y block
                _same_as_oracle(a.mxm(b, sr).new(mask=m.S), masked[key], f"masked mxm dot_yblk=4 {name}")
            # a list cap of 300 keys and short task windows, as test_masked_spgemm_two_sided_vs_oracle:
            # the 700-entry hub lists run as pieces, or (dot_pieces = 1) on the per-entry kernel
            for pieces in (0, 1):
                with G._knobs(gb, dot_cap=300, dot_win=256, dot_pmin=1, dot_pieces=pieces):
                    _same_as_oracle(a.mxm(b, sr).new(mask=m.S), masked[key],
                                    f"masked mxm dot_cap=300 dot_pieces={pieces} {name}")
            with G._knobs(gb, dot_cap=300, dot_win=256):  # few hub entries: handed to the per-entry kernel
                _same_as_oracle(a.mxm(b, sr).new(mask=m.S), masked[key], f"masked mxm dot_cap=300 {name}")

    return run


@sweep(CAPS_SUM)
def test_spmv_general(gb):
    """the general-semiring SpMV and its views on the 700 x 1300 long-row shape of the semiring
    sweep, by words (default), under spmv_general = 1 and under spmv_words = 2"""
    jobs = []
    for sr3 in (("plus", "times", ID), ("min", "plus", "INT32"), ("lor", "land", "BOOL")):
        mon, mul, dt = sr3
        rng = sc.rng_of("sweeps-long", sr3)
        n, m = S.LONG_SHAPE
        p = S._long_rows(rng)
        A = p, np.where(p, sc.draw(dt, rng, (n, m), mon, mul), dm.NP[dt](0))
        um_ = rng.random(m) < 0.5
        U = um_, np.where(um_, sc.draw(dt, rng, m, mon, mul), dm.NP[dt](0))
        Uf = np.ones(m, bool), sc.draw(dt, rng, m, mon, mul)
        vn = rng.random(n) < 0.5
        V = vn, np.where(vn, sc.draw(dt, rng, n, mon, mul), dm.NP[dt](0))
        exps = [S.expect(mon, mul, dt, dm.mxv, A, U), S.expect(mon, mul, dt, dm.mxv, A, Uf),
                S.expect(mon, mul, dt, dm.vxm, V, A), S.expect(mon, mul, dt, dm.mxv, A, V, tran0=True),
                S.expect(mon, mul, dt, dm.vxm, U, A, tran1=True)]
        jobs.append((sr3, A, U, Uf, V, exps))
    # 350 rows of 130 entries: more long-row chunks than one block of k_spmv_fold has threads
    rng = sc.rng_of("sweeps-many-long")
    n, m = S.LONG_SHAPE
    p = np.zeros((n, m), bool)
    for i in range(n):
        p[i, rng.choice(m, 130 if i % 2 == 0 else int(rng.integers(0, 7)), replace=False)] = True
    Al = p, np.where(p, sc.draw(ID, rng, (n, m)), np.int64(0))
    Ul = np.ones(m, bool), sc.draw(ID, rng, m)
    exp_l = S.expect("plus", "times", ID, dm.mxv, Al, Ul)

    def run():
        sr, zt = S.lookup(gb, "plus", "times", ID)
        for kn in ({}, {"xhot": 2, "xhot_cols": 300}):  # the second: the hot-column relabel, 300 hot columns
            with G._knobs(gb, **kn):
                S.check_T(S.to_gb(gb, Al).mxv(S.to_gb(gb, Ul), sr).new(), exp_l, zt, "plus", f"many long rows {kn}")
        for (mon, mul, dt), A, U, Uf, V, exps in jobs:
            sr, zt = S.lookup(gb, mon, mul, dt)
            for kn in ({}, {"spmv_general": 1}, {"spmv_words": 2}):
                with G._knobs(gb, **kn):
                    a, u, uf, v = S.to_gb(gb, A), S.to_gb(gb, U), S.to_gb(gb, Uf), S.to_gb(gb, V)
                    tag = f"{mon}_{mul}[{dt}] {kn}"
                    S.check_T(a.mxv(u, sr).new(), exps[0], zt, mon, f"{tag} mxv")
                    S.check_T(a.mxv(uf, sr).new(), exps[1], zt, mon, f"{tag} mxv full")
                    S.check_T(v.vxm(a, sr).new(), exps[2], zt, mon, f"{tag} vxm")
                    S.check_T(a.T.mxv(v, sr).new(), exps[3], zt, mon, f"{tag} A.T.mxv")
                    S.check_T(u.vxm(a.T, sr).new(), exps[4], zt, mon, f"{tag} vxm A.T")

    return run


@sweep()
def test_bfs_views(gb):
    """the level BFS of the smoke test at 32768 rows: its kernels take no gb_grid, the views they
    read do (non-empty rows and their ranks, pull heads, hub tables, the longest row)"""
    Gr = O.rmat(15, 16, 42)
    n = Gr.nrows
    r, c, _ = Gr.to_coo()
    src = int(np.argmax(np.diff(Gr.indptr)))
    lev = O.bfs_levels(Gr, src)[0]

    def run():
        P = gb.Matrix.from_coo(r, c, True, nrows=n, ncols=n)
        v, q = gb.Vector(gb.INT32, n), gb.Vector(bool, n)
        q[src] = True
        d = 0
        while True:
            d += 1
            v(mask=q.V)[:] = d
            q(~v.S, replace=True) << q.vxm(P, gb.semiring.lor_land)
            if q.nvals == 0:
                break
        idx, lv = v.to_coo()
        got = np.zeros(n, np.int32)
        got[idx.astype(np.int64)] = lv
        assert np.array_equal(got, lev), "BFS levels differ from the oracle"

    return run


@sweep()
def test_rmat(gb):
    Gr = O.rmat(10, 16, 42, values="INT64", value_seed=2)

    def run():
        h = ctypes.c_void_p()
        assert gb.lib.GxB_Matrix_rmat(ctypes.byref(h), 10, 16, 42, 1, 2, 0, 0) == 0
        D = gb.Matrix.__new__(gb.Matrix)
        D._h, D.dtype, D.name = h, gb.INT64, "rmat"
        D._nrows = D._ncols = 1 << 10
        _same_as_oracle(D, Gr, "GxB_Matrix_rmat")

    return run


# ---------------------------------------------------------------------- the trace and the coverage
# gb_grid( call sites that no case clamps: "file:line" -> (kernel, why).  At most 15, and none from
# the files of NO_EXCEPTIONS.
NOT_REACHED = {
    "gb_colbits.hip:1032": ("k_cw_recount", "GxB_Matrix_colwords_touch, the frontier exchange's hook after a raw device "
                                            "copy: test_colbits.py::test_colwords_view_touch"),
    "gb_dot.hip:1223": ("k_dt_hub_classify", "a block per chunk of a hub group: one chunk at these shapes; covered by "
                                             "test_scale_parity.py"),
    "gb_dot.hip:1337": ("k_dt_hub_compact", "a block per hub chunk, as k_dt_hub_classify; covered by "
                                            "test_scale_parity.py"),
    "gb_dot.hip:1353": ("k_dt_huge_to_csr", "lists of more than 65535 pieces (2^29 keys): out of a test's reach"),
}
NO_EXCEPTIONS = ("gb_select.hip", "gb_tile.hip", "gb_reindex.hip", "gb_apply_index.hip", "gb_ewise_union.hip",
                 "gb_subassign.hip", "gb_extract.hip", "gb_writeback.hip", "gb_ops.hip", "gb_prim.hip")


def _api_spans(lines):
    """(first, last) line index of every gb_api(...) macro invocation: a call inside its
    lambda argument is reported at the invocation's line"""
    spans = []
    for i, text in enumerate(lines):
        at = text.split("//")[0].find("gb_api(")
        if at < 0 or "#define" in text:
            continue
        depth, j, k = 0, i, at + len("gb_api")
        while j < len(lines):
            for ch in lines[j].split("//")[0][k:]:
                depth += (ch == "(") - (ch == ")")
                if depth == 0:
                    break
            if depth == 0:
                break
            j, k = j + 1, 0
        spans.append((i, j))
    return spans


def grid_sites():
    """{"file:line": (file, first line, last line of the statement that holds the call, lines of
    the gb_api invocations around it)}: the compiler reports a call nested in a macro's
    arguments (a multi-line hipLaunchKernelGGL, the lambda of gb_api) at a line of the macro's
    invocation, so a reported line is matched to the statements that contain the call"""
    sites = {}
    for f in sorted(os.listdir(CSRC)):
        if not f.endswith((".hip", ".cuh", ".h")):
            continue
        with open(os.path.join(CSRC, f)) as fh:
            lines = fh.read().split("\n")
        spans = _api_spans(lines)
        for i, text in enumerate(lines):
            code = text.split("//")[0]
            if not re.search(r"\bgb_grid\(", code) or re.search(r"inline unsigned gb_grid\(", code):
                continue
            lo = i
            while lo > 0 and not re.search(r"[;{}]\s*(//.*)?$", lines[lo - 1]) and lines[lo - 1].strip() \
                    and not lines[lo - 1].lstrip().startswith("//"):
                lo -= 1
            hi = i
            while hi + 1 < len(lines) and not re.search(r";\s*(//.*)?$", lines[hi]):
                hi += 1
            outer = tuple(x + 1 for a, b in spans if a < i <= b for x in (a, b))
            sites[f"{f}:{i + 1}"] = (f, lo + 1, hi + 1, outer)
    return sites


def clamp_count(gb, site):
    f, lo, hi, outer = site
    return sum(gb.get_knob(f"stat_grid_clamped:{f}:{line}") for line in (*range(lo, hi + 1), *outer))


def test_not_reached_table_matches_the_sources():
    sites = grid_sites()
    assert len(sites) >= 140, f"only {len(sites)} gb_grid( call sites found: the scan is broken"
    assert len(NOT_REACHED) <= 15
    for key, (kernel, why) in NOT_REACHED.items():
        assert key in sites, f"{key} ({kernel}) is no gb_grid( call site any more"
        assert key.split(":")[0] not in NO_EXCEPTIONS, f"{key}: no exceptions in this file"
        assert kernel.startswith("k_") and why
        f, lo, hi, _ = sites[key]
        with open(os.path.join(CSRC, f)) as fh:
            stmt = "\n".join(fh.read().split("\n")[lo - 1:hi + 3])
        assert kernel in stmt, f"{key}: {kernel} is not launched there"


@pytest.mark.gpu
def test_no_trace_without_the_knob(gb):
    sites = grid_sites()
    before = {k: clamp_count(gb, s) for k, s in sites.items()}
    assert gb.get_knob("grid_cap") == 0
    _CASES["test_select"][0](gb)()
    _CASES["test_write_back_vector"][0](gb)()
    assert {k: clamp_count(gb, s) for k, s in sites.items()} == before


@pytest.mark.gpu
def test_every_site_was_clamped(gb):
    """the last test: every gb_grid( call site ran clamped at cap 1, but for NOT_REACHED"""
    for name, (_, caps) in _CASES.items():
        if name not in _DONE:  # this test selected on its own: run what has not run
            _run(gb, name, (1,))
    sites = grid_sites()
    missed = sorted(k for k, s in sites.items() if clamp_count(gb, s) == 0)
    print(f"\n{len(sites)} gb_grid( call sites, {len(missed)} never clamped")
    for k in missed:
        print(f"NOT CLAMPED {k}{'  (listed)' if k in NOT_REACHED else ''}")
    unlisted = [k for k in missed if k not in NOT_REACHED]
    assert not unlisted, f"call sites no case clamps: {unlisted}"
    stale = [k for k in NOT_REACHED if k not in missed]
    assert not stale, f"listed as not reached, but clamped (or gone): {stale}"
