"""GPU parity of GxB_{Matrix,Vector,Row,Col}_subassign, GrB_Row_assign / GrB_Col_assign and the
two GrB_Scalar forms with the numpy model of tests/subassign_model.py (its two formulations are
held against each other and against the reference's cases by tests/test_subassign_abi.py).

Every comparison is exact and goes through test_general_ops_gpu.check: structure, order, nvals,
dtype, values, NaN payload and the sign of zero.  Values are only moved, cast, or combined by one
accumulator application on two operands: there is no reduction and no tolerance.

Shapes, and the path each one is for
  rows   70 x 300   rows of 0, 1, 63, 64, 65, 128, 129 and 300 entries: the merge of kept and
                    placed entries ends before, on and after a wave's width; a full-density A under
                    an unsorted J places rows longer than 64 and sorts them
  400 x 40          runs of more than 64 empty rows (the row search of an entry skips them)
  heavy  301 x 6007 one row of 5200 entries, half of them inside J
  tall   140000 x 70 with 56000 unsorted rows in I: more rows than waves in the grid
  wide   70 x 140000 with 56000 sorted / unsorted columns: a column bitmap of 2188 words, sort
                    keys with large columns
  low    40 x 90    in column-word format after a whole-matrix masked scalar assign
  one    1 x 1
  lines  1000 x 70  columns of 0, 1, 65 and 1000 entries for the column forms
  vectors 0, 1, 63, 64, 65, 1000, 100000: an empty bitmap, one word, a word boundary, many blocks
"""
import ctypes
import time

import numpy as np
import pytest

import dense_model as dm
import indexing_cases as ic
import subassign_model as sm
from test_general_ops_gpu import check, heavy, iso_gb, to_gb
from test_indexing_gpu import EmptyScalar, abi_out, bitmap_words, is_iso
from test_subassign_abi import apply_step

pytestmark = pytest.mark.gpu

NULL_POINTER, UNINITIALIZED, INVALID_VALUE, INVALID_INDEX, DIMENSION_MISMATCH, INDEX_OUT_OF_BOUNDS = \
    -2, -1, -3, -4, -6, -105
RANGE, STRIDE, BACKWARDS = 2**63 - 1, 2**63 - 2, 2**63 - 3
G = sm.golden()

# (mask kind, replace, accum): no mask, accum only, the four kinds with and without replace, one with accum
VARIANTS = [("none", False, None), ("none", False, "plus"), ("S", False, None), ("S", True, None),
            ("V", False, None), ("V", True, None), ("~S", False, None), ("~S", True, None),
            ("~V", False, None), ("~V", True, None), ("V", True, "plus")]


@pytest.fixture(scope="module")
def gb():
    import graphblas_amd

    return graphblas_amd


@pytest.fixture(scope="module", autouse=True)
def report_run_time():
    t0 = time.perf_counter()
    yield
    print(f"\ntest_subassign_gpu.py: {time.perf_counter() - t0:.1f} s")


def stat(gb, key):
    out = ctypes.c_int64()
    assert gb.lib.GxB_Global_get_int(key.encode(), ctypes.byref(out)) == 0
    return out.value


def key_of(I):
    return slice(None) if I is None else I


def length(I, n):
    return n if I is None else len(I)


def bind_sub(gb, target, wb, m):
    """target[...] bound with a write-back variant: the submask form"""
    kind, rep, acc = wb
    kw = {}
    if kind != "none":
        mk = m.S if "S" in kind else m.V
        kw["mask"] = ~mk if kind.startswith("~") else mk
        kw["replace"] = rep
    if acc is not None:
        kw["accum"] = getattr(gb.binary, acc)
    return target(**kw)


def abi_list(gb, L, n):
    """(pointer, count, keep-alive) of None (GrB_ALL), an explicit list, or (code, [begin, end(, inc)])"""
    if L is None:
        return gb.lib.GrB_ALL, n, None
    if isinstance(L, tuple):
        a = np.ascontiguousarray(L[1], np.uint64)
        return ctypes.c_void_p(a.ctypes.data), L[0], a
    a = np.ascontiguousarray(L, np.uint64)
    return ctypes.c_void_p(a.ctypes.data), a.size, a


def expand(L, n):
    """the explicit list of an encoded one"""
    if not isinstance(L, tuple):
        return L
    code, a = L
    if code == RANGE:
        return list(range(a[0], a[1] + 1))
    if code == STRIDE:
        return list(range(a[0], a[1] + 1, a[2]))
    return list(range(a[0], a[1] - 1, -a[2]))


# ---------------------------------------------------------------------- the golden steps
@pytest.mark.parametrize("name", sm.CHAINS)
def test_golden_chains(gb, name):
    from graphblas_amd.exceptions import DimensionMismatch

    case = G[name]
    objs = sm.golden_objects(G, case)
    dev = {k: to_gb(gb, x) for k, x in objs.items()}
    results = [sm.pair_of(r) for r in case["results"]]
    exc = {"DimensionMismatch": DimensionMismatch, "TypeError": TypeError}
    state = {}
    for step in case["steps"]:
        t = step["target"]
        if step["fresh"] or t not in state:
            state[t] = dev[t].dup()
        C = state[t]
        before = C.dup()
        if step.get("needs_matrix_assign") or "raises" in step["expect"]:
            err, match = (NotImplementedError, "GrB_Matrix_assign with index lists") \
                if step.get("needs_matrix_assign") else (exc[step["expect"]["raises"]], step["expect"]["match"])
            with pytest.raises(err, match=match):
                apply_step(gb, C, step, dev)
            assert C.isequal(before, check_dtype=True), step["src"]
            continue
        apply_step(gb, C, step, dev)
        want = results[step["expect"]["result"]]
        want = dm.resize(want, C.shape)
        check(C, want, dm.name_of(want[1].dtype), what=step["src"])


@pytest.mark.parametrize("case", sm.combo_cases(G), ids=lambda c: c["id"])
def test_golden_combos(gb, case):
    shape = case["shape"]
    wrap = {"vector": lambda x: x, "row": sm.as_row, "matrix": sm.as_row, "column": sm.as_col}[shape]
    c, want = to_gb(gb, wrap(case["self"])), wrap(case["want"])
    val = to_gb(gb, wrap(case["val"]) if shape == "matrix" else case["val"])
    m = to_gb(gb, wrap(case["mask"]) if shape == "matrix" else case["mask"])
    mask = {"S": m.S, "V": m.V, "CS": ~m.S, "CV": ~m.V}[case["mask_kind"]]
    index = case["index"]
    keys = {"vector": index, "row": (0, index), "column": (index, 0), "matrix": ([0], index)}[shape]
    c[keys](gb.binary.plus, mask, replace=case["replace"]) << val
    check(c, want, "INT64", what=case["src"])


# ---------------------------------------------------------------------- the pair sweep
PAIRS = [("all", "all"), ("all", "unsorted"), ("one300", "perm"), ("one0", "unsorted"), ("empty", "unsorted"),
         ("rev", "sorted"), ("perm", "perm"), ("unsorted", "unsorted"), ("sorted", "one"), ("revsorted", "empty"),
         ("perm", "range"), ("unsorted", "stride"), ("sorted", "backwards"), ("all", "range"), ("rev", "unsorted"),
         ("sorted", "sorted"), ("one300", "all"), ("perm", "backwards"), ("unsorted", "all"), ("revsorted", "perm")]


def sweep_list(name, n, key):
    if name == "one300":
        return np.array([7], np.int64)  # the 300-entry row
    if name == "one0":
        return np.array([0], np.int64)  # an empty row
    if name == "range":
        return (RANGE, [10, 200])
    if name == "stride":
        return (STRIDE, [3, 290, 7])
    if name == "backwards":
        return (BACKWARDS, [280, 5, 3])
    return ic.index_named(name, n, key)


@pytest.mark.parametrize("cname", ["rows", "empty"])
@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"I={p[0]},J={p[1]}")
def test_pair_sweep(gb, pair, cname):
    dt = "INT64"
    C = ic.matrix_named(cname, dt)
    c0 = to_gb(gb, C)
    LI, LJ = sweep_list(pair[0], 70, ("sweep I", pair)), sweep_list(pair[1], 300, ("sweep J", pair))
    I, J = expand(LI, 70), expand(LJ, 300)
    ni, nj = length(I, 70), length(J, 300)
    encoded = isinstance(LJ, tuple)
    variants = VARIANTS if cname == "rows" else VARIANTS[:3] + VARIANTS[-1:]
    for k, wb in enumerate(variants):
        a_kind = ("full", "sparse", "empty")[k % 3] if k else "full"  # the unmasked case places full rows
        m_kind = ("sparse", "full", "empty")[(k // 3) % 3]
        A = ic.obj(dt, (ni, nj), ("sweep A", pair, k), 0.5, a_kind)
        M = ic.mask_obj((ni, nj), ("sweep M", pair, k), m_kind)
        want = sm.subassign(C, A, I, J, **ic.wb_kw(wb, M))
        c, a, m = c0.dup(), to_gb(gb, A), to_gb(gb, M)
        what = f"{cname} I={pair[0]} J={pair[1]} {wb} A={a_kind} M={m_kind}"
        if encoded or (I is None and J is None and wb[0] == "none"):
            # the slice encodings reach the library through the ABI only, and C[:, :] << A is GrB_Matrix_assign
            mask, accum, desc = abi_out(gb, wb, m, dt)
            Ip, nI, _i = abi_list(gb, LI, 70)
            Jp, nJ, _j = abi_list(gb, LJ, 300)
            assert gb.lib.GxB_Matrix_subassign(c._h, mask, accum, a._h, Ip, nI, Jp, nJ, desc) == 0, what
        elif wb == ("none", False, None):
            c[key_of(I), key_of(J)] << a
        else:
            bind_sub(gb, c[key_of(I), key_of(J)], wb, m) << a
        check(c, want, dt, what=what)
        jsorted = J is None or all(x < y for x, y in zip(J[:-1], J[1:]))
        assert stat(gb, "stat_subassign_jsort") == (0 if jsorted else 1), what
        assert stat(gb, "stat_subassign_extract") == (0 if wb == ("none", False, None) else 1), what


# ---------------------------------------------------------------------- types and iso
TYPES = [("BOOL", "INT64", None, None), ("INT8", "FP64", "plus", "FP64"), ("INT64", "INT8", "min", "INT64"),
         ("FP32", "INT64", "plus", "FP64"), ("FP64", "FP32", "second", "FP32"), ("INT8", "INT64", None, None),
         ("FP32", "FP64", None, None)]


@pytest.mark.parametrize("ct,at,accum,adt", TYPES)
def test_types_and_casts(gb, ct, at, accum, adt):
    C = ic.obj(ct, (37, 53), ("types C", ct, at))
    I, J = ic.index_named("unsorted", 37, "types I"), ic.index_named("perm", 53, "types J")
    A = ic.obj(at, (len(I), 53), ("types A", ct, at), 0.6)
    M = ic.mask_obj((len(I), 53), ("types M", ct, at), "fp64")
    a, m = to_gb(gb, A), to_gb(gb, M)
    for wb in (("none", False, None), ("V", False, None), ("~S", True, None)):
        c = to_gb(gb, C)
        bind_sub(gb, c[I, J], wb, m) << a
        check(c, sm.subassign(C, A, I, J, **ic.wb_kw(wb, M)), ct, what=f"{ct} << {at} {wb}")
    if accum is not None:
        for wb in (("none", False, accum), ("S", True, accum)):
            c = to_gb(gb, C)
            mask, acc, desc = abi_out(gb, wb, m, adt)
            Ip, nI, _i = abi_list(gb, I, 37)
            Jp, nJ, _j = abi_list(gb, J, 53)
            assert gb.lib.GxB_Matrix_subassign(c._h, mask, acc, a._h, Ip, nI, Jp, nJ, desc) == 0
            want = sm.subassign(C, A, I, J, accum_dtype=adt, **ic.wb_kw(wb, M))
            check(c, want, ct, what=f"{ct} << {at} accum {accum}[{adt}] {wb}")


@pytest.mark.parametrize("c_iso,a_iso,same", [(True, False, False), (False, True, False), (True, True, True),
                                               (True, True, False)])
def test_iso_operands(gb, c_iso, a_iso, same):
    dt = "FP64"
    C = ic.matrix_named("rows", dt)
    I, J = ic.index_named("sorted", 70, "iso I"), ic.index_named("unsorted", 300, "iso J")
    A = ic.obj(dt, (len(I), len(J)), "iso A", 0.5)
    M = ic.mask_obj((len(I), len(J)), "iso M")
    m = to_gb(gb, M)
    for wb in (("none", False, None), ("V", False, None), ("S", True, "plus")):
        c, Cm = iso_gb(gb, C[0], -2.5, dt) if c_iso else (to_gb(gb, C), C)
        a, Am = iso_gb(gb, A[0], -2.5 if same else 7.25, dt) if a_iso else (to_gb(gb, A), A)
        assert is_iso(c) == c_iso and is_iso(a) == a_iso
        bind_sub(gb, c[I, J], wb, m) << a
        check(c, sm.subassign(Cm, Am, I, J, **ic.wb_kw(wb, M)), dt, what=f"iso C={c_iso} A={a_iso} {wb}")


# ---------------------------------------------------------------------- larger and special shapes
def run_shape(gb, C, I, J, key, wbs, density=0.5, dt="INT64"):
    ni, nj = length(I, C[0].shape[0]), length(J, C[0].shape[1])
    A = ic.obj(dt, (ni, nj), ("shape A", key), density)
    M = ic.mask_obj((ni, nj), ("shape M", key))
    c0, a, m = to_gb(gb, C), to_gb(gb, A), to_gb(gb, M)
    for wb in wbs:
        c = c0.dup()
        bind_sub(gb, c[key_of(I), key_of(J)], wb, m) << a
        check(c, sm.subassign(C, A, I, J, **ic.wb_kw(wb, M)), dt, what=f"{key} {wb}")


def test_runs_of_empty_rows(gb):
    rng = ic.rng_of("empty runs")
    p = rng.random((400, 40)) < 0.3
    p[20:120] = False
    p[200:330] = False
    C = (p, np.where(p, ic.draw("INT64", rng, p.size).reshape(p.shape), 0))
    I = np.r_[np.arange(10, 90), np.arange(250, 399)][::-1].copy()  # rows inside and outside the runs
    run_shape(gb, C, I, ic.index_named("unsorted", 40, "runs J"), "runs", VARIANTS[:4] + VARIANTS[-1:])


def test_heavy_row(gb):
    C = heavy("INT64", "subassign")
    hub = np.flatnonzero(C[0][7])
    assert hub.size == 5200
    rng = ic.rng_of("heavy J")
    J = rng.permutation(np.r_[hub[::2], np.setdiff1d(np.arange(6007), hub)[:400]])  # half of the hub row's columns
    I = np.array([300, 7, 0, 150], np.int64)
    run_shape(gb, C, I, J, "heavy", [VARIANTS[0], VARIANTS[4], VARIANTS[-1]], density=0.7)
    run_shape(gb, C, I, np.sort(J), "heavy sorted", [VARIANTS[0], VARIANTS[3]], density=0.7)


def test_tall(gb):
    C = ic.matrix_named("tall", "INT64")
    I = ic.index_named("unsorted", 140000, "tall I")
    assert len(I) == 56000
    run_shape(gb, C, I, ic.index_named("perm", 70, "tall J"), "tall", [VARIANTS[0], VARIANTS[-1]], density=0.05)


@pytest.mark.parametrize("name", ["sorted", "unsorted"])
def test_wide(gb, name):
    W = ic.matrix_named("wide", "INT64")
    J = ic.index_named(name, 140000, "wide J")
    assert len(J) == 56000
    run_shape(gb, W, ic.index_named("perm", 70, "wide I"), J, f"wide {name}", [VARIANTS[0], VARIANTS[5]], density=0.05)
    assert stat(gb, "stat_subassign_jsort") == (name == "unsorted")


def test_column_word_target_and_one_by_one(gb):
    C = ic.matrix_named("low", "INT64")
    c = to_gb(gb, C)
    gb.set_knob("colbits", 1)
    try:
        c(mask=c.S)[:, :] = 5  # a whole-matrix masked scalar assign: C is now held in column words
    finally:
        gb.set_knob("colbits", 0)
    Cm = (C[0], np.where(C[0], np.int64(5), 0))
    I, J = ic.index_named("unsorted", 40, "low I"), ic.index_named("unsorted", 90, "low J")
    A = ic.obj("INT64", (len(I), len(J)), "low A")
    c[I, J] << to_gb(gb, A)
    check(c, sm.subassign(Cm, A, I, J), "INT64", what="low, from column words")
    one = ic.matrix_named("one", "INT64")
    for A in (ic.obj("INT64", (1, 1), "one A", kind="full"), ic.obj("INT64", (1, 1), "one E", kind="empty")):
        for wb in (("none", False, None), ("S", True, "plus")):
            c = to_gb(gb, one)
            bind_sub(gb, c[[0], [0]], wb, c) << to_gb(gb, A)  # the mask is C
            check(c, sm.subassign(one, A, [0], [0], **ic.wb_kw(wb, one)), "INT64", what=f"one {wb}")


# ---------------------------------------------------------------------- row and column forms
LINE_WB = [("none", False, None), ("none", False, "plus"), ("S", False, None), ("S", True, None), ("V", True, None),
           ("~S", True, None), ("~V", False, None), ("~S", False, "plus")]


@pytest.mark.parametrize("row", [0, 3, 7])
def test_row_forms(gb, row):
    dt = "INT64"
    C = ic.matrix_named("rows", dt)
    assert C[0][row].sum() in (0, 64, 300)
    c0 = to_gb(gb, C)
    deleted_outside = left_outside = False
    for nj in (0, 1, 63, 64, 65, 300):
        J = None if nj == 300 else ic.rng_of("row J", row, nj).permutation(300)[:nj].astype(np.int64)
        for k, wb in enumerate(LINE_WB):
            u = ic.obj(dt, (nj,), ("row u", row, nj, k), 0.5, ("sparse", "full", "empty")[k % 3])
            ug = to_gb(gb, u)
            # assign: the mask spans the row
            M = ic.mask_obj((300,), ("row M", row, nj, k))
            want = sm.row_assign(C, u, row, J, **ic.wb_kw(wb, M))
            c = c0.dup()
            bind_sub(gb, c, wb, to_gb(gb, M))[row, key_of(J)] << ug
            check(c, want, dt, what=f"GrB_Row_assign row {row} nj {nj} {wb}")
            # subassign: the mask spans J
            Ms = ic.mask_obj((nj,), ("row Ms", row, nj, k))
            wants = sm.row_subassign(C, u, row, J, **ic.wb_kw(wb, Ms))
            c = c0.dup()
            bind_sub(gb, c[row, key_of(J)], wb, to_gb(gb, Ms)) << ug
            check(c, wants, dt, what=f"GxB_Row_subassign row {row} nj {nj} {wb}")
            if wb[1] and J is not None and nj:
                out = np.setdiff1d(np.arange(300), J)
                deleted_outside |= bool((C[0][row, out] & ~want[0][row, out]).any())
                left_outside |= np.array_equal(C[0][row, out], wants[0][row, out]) and bool(C[0][row, out].any())
    if C[0][row].any():
        assert deleted_outside and left_outside  # replace reaches outside J for assign only


@pytest.mark.parametrize("col", [0, 1, 2, 3])
def test_column_forms(gb, col):
    dt = "INT64"
    C = ic.matrix_named("lines", dt)
    assert C[0][:, col].sum() == ic.LINE_LENGTHS[col]
    c0 = to_gb(gb, C)
    for name in ("all", "unsorted", "one", "empty"):
        I = ic.index_named(name, 1000, ("col I", col))
        ni = length(I, 1000)
        for k, wb in enumerate(LINE_WB):
            u = ic.obj(dt, (ni,), ("col u", col, name, k), 0.5, ("sparse", "full", "empty")[k % 3])
            ug = to_gb(gb, u)
            M = ic.mask_obj((1000,), ("col M", col, name, k))
            c = c0.dup()
            bind_sub(gb, c, wb, to_gb(gb, M))[key_of(I), col] << ug
            check(c, sm.col_assign(C, u, I, col, **ic.wb_kw(wb, M)), dt, what=f"GrB_Col_assign {col} {name} {wb}")
            Ms = ic.mask_obj((ni,), ("col Ms", col, name, k))
            c = c0.dup()
            bind_sub(gb, c[key_of(I), col], wb, to_gb(gb, Ms)) << ug
            check(c, sm.col_subassign(C, u, I, col, **ic.wb_kw(wb, Ms)), dt,
                  what=f"GxB_Col_subassign {col} {name} {wb}")


def test_scalar_onto_a_row_with_a_vector_mask(gb):
    C = ic.matrix_named("rows", "INT64")
    J = ic.index_named("unsorted", 300, "scalar row J")
    M, Ms = ic.mask_obj((300,), "scalar row M"), ic.mask_obj((len(J),), "scalar row Ms")
    c = to_gb(gb, C)
    c(to_gb(gb, M).V, replace=True)[6, J] << 9
    check(c, sm.row_assign(C, np.int64(9), 6, J, mask=M, replace=True), "INT64", what="C(m)[i, J] << c")
    c = to_gb(gb, C)
    c[6, J](to_gb(gb, Ms).S, gb.binary.plus) << 9
    check(c, sm.row_subassign(C, np.int64(9), 6, J, mask=Ms, mask_struct=True, accum="plus"), "INT64",
          what="C[i, J](m) << c")


# ---------------------------------------------------------------------- vectors
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1000, 100000])
def test_vector_forms(gb, n):
    dt = "FP64"
    for wkind in ("sparse", "iso", "never"):
        W = ic.obj(dt, (n,), ("vec W", n), 0.5, wkind)
        lists = [("all", None), ("perm", ic.index_named("perm", n, "vec")), ("empty", np.zeros(0, np.int64))]
        if n > 1:
            lists += [("unsorted", ic.index_named("unsorted", n, "vec")), ("range", (RANGE, [n // 4, n - 2]))]
        for lname, L in lists:
            I = expand(L, n)
            ni = length(I, n)
            for k, wb in enumerate(VARIANTS if n <= 1000 and wkind == "sparse" else VARIANTS[:1] + VARIANTS[-3:]):
                u = ic.obj("INT64" if k % 2 else dt, (ni,), ("vec u", n, lname, k), 0.5,
                           ("sparse", "full", "empty")[k % 3])
                M = ic.mask_obj((ni,), ("vec M", n, lname, k), ("sparse", "fp64", "full")[k % 3])
                if wkind == "iso" and W[0].any():
                    w = iso_gb(gb, W[0], W[1][W[0]][0], dt)[0]
                elif wkind == "never":
                    w = gb.Vector(dt, n)
                else:
                    w = to_gb(gb, W)
                ug, m = to_gb(gb, u), to_gb(gb, M)
                what = f"vector n={n} w={wkind} I={lname} {wb}"
                if isinstance(L, tuple):
                    mask, accum, desc = abi_out(gb, wb, m, dt)
                    Ip, nI, _i = abi_list(gb, L, n)
                    assert gb.lib.GxB_Vector_subassign(w._h, mask, accum, ug._h, Ip, nI, desc) == 0, what
                else:
                    bind_sub(gb, w[key_of(I)], wb, m) << ug
                want = sm.subassign(W, u, I, None, **ic.wb_kw(wb, M))
                check(w, want, dt, what=what)
                bits = np.zeros(((n + 63) // 64) * 64, bool)
                bits[:n] = want[0]
                packed = np.packbits(bits, bitorder="little").view(np.uint64)
                assert np.array_equal(bitmap_words(gb, w), packed), f"{what}: bitmap words"
                assert w.nvals == int(want[0].sum())


# ---------------------------------------------------------------------- scalar forms
def test_scalar_forms(gb):
    dt = "INT64"
    C = ic.matrix_named("rows", dt)
    I, J = ic.index_named("unsorted", 70, "scalar I"), ic.index_named("unsorted", 300, "scalar J")
    M = ic.mask_obj((len(I), len(J)), "scalar M")
    W = ic.obj(dt, (1000,), "scalar W")
    K = ic.index_named("unsorted", 1000, "scalar K")
    Mv = ic.mask_obj((len(K),), "scalar Mv")
    m, mv = to_gb(gb, M), to_gb(gb, Mv)
    for wb in (("none", False, None), ("V", False, None), ("~S", True, "plus"), ("none", False, "plus")):
        for x in (np.int32(-7), None):  # a value of another type, and the empty scalar
            c, w = to_gb(gb, C), to_gb(gb, W)
            what = f"scalar {x} {wb}"
            if x is None:
                mask, accum, desc = abi_out(gb, wb, m, dt)
                Ip, nI, _i = abi_list(gb, I, 70)
                Jp, nJ, _j = abi_list(gb, J, 300)
                Kp, nK, _k = abi_list(gb, K, 1000)
                with EmptyScalar(gb, "INT32") as s:
                    assert gb.lib.GxB_Matrix_subassign_Scalar(c._h, mask, accum, s, Ip, nI, Jp, nJ, desc) == 0
                    vmask = abi_out(gb, wb, mv, dt)[0]
                    assert gb.lib.GxB_Vector_subassign_Scalar(w._h, vmask, accum, s, Kp, nK, desc) == 0
            elif wb[0] == "none":  # C[I, J](accum) << x is GrB_Matrix_assign_<T>; the scalar entry point by the ABI
                s = gb.Scalar.from_value(int(x), "INT32")
                mask, accum, desc = abi_out(gb, wb, m, dt)
                Ip, nI, _i = abi_list(gb, I, 70)
                Jp, nJ, _j = abi_list(gb, J, 300)
                assert gb.lib.GxB_Matrix_subassign_Scalar(c._h, mask, accum, s._h, Ip, nI, Jp, nJ, desc) == 0
                bind_sub(gb, w[K], wb, mv) << s
            else:
                bind_sub(gb, c[I, J], wb, m) << int(x)
                bind_sub(gb, w[K], wb, mv) << gb.Scalar.from_value(int(x), "INT32")
            check(c, sm.subassign(C, x, I, J, **ic.wb_kw(wb, M)), dt, what=what)
            check(w, sm.subassign(W, x, K, None, **ic.wb_kw(wb, Mv)), dt, what=what + " (vector)")
    c = to_gb(gb, C)
    c[I, J] << 4  # C[I, J] << scalar: the existing GrB_Matrix_assign_<T> with lists
    check(c, sm.subassign(C, np.int64(4), I, J), dt, what="C[I, J] << 4")


# ---------------------------------------------------------------------- aliasing, transposes, determinism
def test_aliasing(gb):
    dt = "INT64"
    C = ic.matrix_named("square", dt)
    I, J = ic.index_named("perm", 70, "alias I"), ic.index_named("perm", 70, "alias J")
    for wb in (("none", False, None), ("none", False, "plus"), ("V", True, None), ("~S", False, "plus")):
        c = to_gb(gb, C)
        bind_sub(gb, c[I, J], wb, c) << c  # A is C, and the mask is C
        check(c, sm.subassign(C, C, I, J, **ic.wb_kw(wb, C)), dt, what=f"A = M = C {wb}")
        A = ic.obj(dt, (70, 70), "alias A")
        c, a = to_gb(gb, C), to_gb(gb, A)
        bind_sub(gb, c[I, J], ("S", wb[1], wb[2]), a) << a  # the mask is A
        check(c, sm.subassign(C, A, I, J, **ic.wb_kw(("S", wb[1], wb[2]), A)), dt, what=f"M = A {wb}")
    W = ic.obj(dt, (1000,), "alias W")
    K = ic.index_named("perm", 1000, "alias K")
    w = to_gb(gb, W)
    w[K](w.V, gb.binary.plus, replace=True) << w
    check(w, sm.subassign(W, W, K, None, mask=W, accum="plus", replace=True), dt, what="w[K](w.V) << w")


def test_transposes(gb):
    dt = "INT64"
    C = ic.matrix_named("small", dt)
    I, J = ic.index_named("unsorted", 70, "tran I"), ic.index_named("sorted", 90, "tran J")
    A = ic.obj(dt, (len(J), len(I)), "tran A")  # the region's shape, transposed
    M = ic.mask_obj((len(I), len(J)), "tran M")
    a, m = to_gb(gb, A), to_gb(gb, M)
    for wb in (("none", False, None), ("V", True, "plus")):
        c = to_gb(gb, C)
        assert gb.lib.GxB_Matrix_prepare_transpose(c._h) == 0  # a cached transpose that the call must drop
        bind_sub(gb, c[I, J], wb, m) << a.T
        want = sm.subassign(C, dm.transpose(A), I, J, **ic.wb_kw(wb, M))
        check(c, want, dt, what=f"INP0 transposed {wb}")
        check(c.T.new(), dm.transpose(want), dt, what=f"C.T after the subassign {wb}")


def csr_bytes(gb, c):
    import torch
    from graphblas_amd.device import device_tensor, matrix_view

    v = matrix_view(c._h)
    size = dm.NP[c.dtype.name]().itemsize
    torch.cuda.synchronize()
    rp = device_tensor(torch, v.rowptr, v.nrows + 1).cpu().numpy()
    ci = device_tensor(torch, v.colidx, v.nvals, "<i4").cpu().numpy() if v.nvals else np.zeros(0, np.int32)
    vx = device_tensor(torch, v.values, (1 if v.iso else v.nvals) * size, "|u1").cpu().numpy() if v.nvals \
        else np.zeros(0, np.uint8)
    return rp, ci, vx


def test_determinism_and_ascending_columns(gb):
    dt = "FP64"
    C = ic.matrix_named("rows", dt)
    I, J = ic.index_named("perm", 70, "det I"), ic.index_named("unsorted", 300, "det J")
    A = ic.obj(dt, (70, len(J)), "det A", 0.8)
    M = ic.mask_obj((70, len(J)), "det M")
    a, m = to_gb(gb, A), to_gb(gb, M)
    for wb in (("none", False, None), ("~V", True, "plus")):
        got = []
        for rep in range(2):
            c = to_gb(gb, C).dup()
            bind_sub(gb, c[I, J], wb, m) << a
            got.append(csr_bytes(gb, c))
        for x, y in zip(*got):
            assert x.tobytes() == y.tobytes(), wb
        rp, ci, _ = got[0]
        for r in range(70):
            assert np.all(np.diff(ci[rp[r]:rp[r + 1]]) > 0), (wb, r)


def test_counters(gb):
    dt = "INT64"
    C = ic.matrix_named("rows", dt)
    I = ic.index_named("sorted", 70, "stat I")
    for name, L, want in [("all", None, 0), ("range", (RANGE, [10, 200]), 0), ("sorted", "sorted", 0),
                          ("perm", "perm", 1), ("unsorted", "unsorted", 1), ("backwards", (BACKWARDS, [280, 5, 3]), 1)]:
        L = ic.index_named(L, 300, "stat J") if isinstance(L, str) else L
        J = expand(L, 300)
        A = ic.obj(dt, (len(I), length(J, 300)), ("stat A", name), kind="full")
        M = ic.mask_obj(A[0].shape, ("stat M", name))
        for wb in (("none", False, None), ("none", False, "plus"), ("S", False, None)):
            c, a, m = to_gb(gb, C), to_gb(gb, A), to_gb(gb, M)
            mask, accum, desc = abi_out(gb, wb, m, dt)
            Ip, nI, _i = abi_list(gb, I, 70)
            Jp, nJ, _j = abi_list(gb, L, 300)
            assert gb.lib.GxB_Matrix_subassign(c._h, mask, accum, a._h, Ip, nI, Jp, nJ, desc) == 0
            check(c, sm.subassign(C, A, I, J, **ic.wb_kw(wb, M)), dt, what=f"counters J={name} {wb}")
            assert stat(gb, "stat_subassign_jsort") == want, (name, wb)
            assert stat(gb, "stat_subassign_extract") == (0 if wb == ("none", False, None) else 1), (name, wb)


# ---------------------------------------------------------------------- refusals
def test_refusals_leave_c_untouched(gb):
    dt = "INT64"
    lib = gb.lib
    C = ic.matrix_named("small", dt)  # 70 x 90
    c = to_gb(gb, C)
    A34, u4, u3 = ic.obj(dt, (3, 4), "ref A"), ic.obj(dt, (4,), "ref u4"), ic.obj(dt, (3,), "ref u3")
    a, g4, g3 = to_gb(gb, A34), to_gb(gb, u4), to_gb(gb, u3)
    m34, m90, m70 = to_gb(gb, ic.mask_obj((3, 4), "ref m")), to_gb(gb, ic.mask_obj((90,), "ref m90")), \
        to_gb(gb, ic.mask_obj((70,), "ref m70"))
    W = ic.obj(dt, (100,), "ref W")
    w = to_gb(gb, W)
    plus = gb.binary.plus[dt]._carg

    def L(x):
        arr = np.ascontiguousarray(x, np.uint64)
        return ctypes.c_void_p(arr.ctypes.data), arr.size, arr

    I3, J4, Idup, Jdup, Ioob, Joob = L([1, 2, 3]), L([4, 5, 6, 7]), L([1, 2, 1]), L([4, 5, 6, 4]), L([1, 70, 3]), \
        L([4, 5, 90, 7])
    K3, Kdup, Koob = L([5, 6, 7]), L([5, 6, 5]), L([5, 100, 7])
    with EmptyScalar(gb, dt) as s:
        calls = [
            # a repeated index, in every entry point (scalar forms included)
            (INVALID_VALUE, lambda: lib.GxB_Matrix_subassign(c._h, None, None, a._h, *Idup[:2], *J4[:2], None)),
            (INVALID_VALUE, lambda: lib.GxB_Matrix_subassign(c._h, None, plus, a._h, *I3[:2], *Jdup[:2], None)),
            (INVALID_VALUE, lambda: lib.GxB_Matrix_subassign_Scalar(c._h, None, None, s, *Idup[:2], *J4[:2], None)),
            (INVALID_VALUE, lambda: lib.GxB_Row_subassign(c._h, None, None, g4._h, 2, *Jdup[:2], None)),
            (INVALID_VALUE, lambda: lib.GrB_Row_assign(c._h, None, None, g4._h, 2, *Jdup[:2], None)),
            (INVALID_VALUE, lambda: lib.GxB_Col_subassign(c._h, None, None, g3._h, *Idup[:2], 2, None)),
            (INVALID_VALUE, lambda: lib.GrB_Col_assign(c._h, None, None, g3._h, *Idup[:2], 2, None)),
            (INVALID_VALUE, lambda: lib.GxB_Vector_subassign(w._h, None, None, g3._h, *Kdup[:2], None)),
            (INVALID_VALUE, lambda: lib.GxB_Vector_subassign_Scalar(w._h, None, None, s, *Kdup[:2], None)),
            # a list entry out of range
            (INDEX_OUT_OF_BOUNDS, lambda: lib.GxB_Matrix_subassign(c._h, None, None, a._h, *Ioob[:2], *J4[:2], None)),
            (INDEX_OUT_OF_BOUNDS, lambda: lib.GxB_Matrix_subassign(c._h, m34._h, plus, a._h, *I3[:2], *Joob[:2], None)),
            (INDEX_OUT_OF_BOUNDS, lambda: lib.GrB_Row_assign(c._h, None, None, g4._h, 2, *Joob[:2], None)),
            (INDEX_OUT_OF_BOUNDS, lambda: lib.GxB_Col_subassign(c._h, None, None, g3._h, *Ioob[:2], 2, None)),
            (INDEX_OUT_OF_BOUNDS, lambda: lib.GxB_Vector_subassign(w._h, None, None, g3._h, *Koob[:2], None)),
            # i or j out of range
            (INVALID_INDEX, lambda: lib.GrB_Row_assign(c._h, None, None, g4._h, 70, *J4[:2], None)),
            (INVALID_INDEX, lambda: lib.GxB_Row_subassign(c._h, None, None, g4._h, 70, *J4[:2], None)),
            (INVALID_INDEX, lambda: lib.GrB_Col_assign(c._h, None, None, g3._h, *I3[:2], 90, None)),
            (INVALID_INDEX, lambda: lib.GxB_Col_subassign(c._h, None, None, g3._h, *I3[:2], 90, None)),
            # A, u or the mask of the wrong shape
            (DIMENSION_MISMATCH, lambda: lib.GxB_Matrix_subassign(c._h, None, None, a._h, *J4[:2], *I3[:2], None)),
            (DIMENSION_MISMATCH, lambda: lib.GxB_Matrix_subassign(c._h, c._h, None, a._h, *I3[:2], *J4[:2], None)),
            (DIMENSION_MISMATCH, lambda: lib.GxB_Matrix_subassign_Scalar(c._h, c._h, None, s, *I3[:2], *J4[:2], None)),
            (DIMENSION_MISMATCH, lambda: lib.GxB_Row_subassign(c._h, None, None, g3._h, 2, *J4[:2], None)),
            (DIMENSION_MISMATCH, lambda: lib.GxB_Row_subassign(c._h, m90._h, None, g4._h, 2, *J4[:2], None)),
            (DIMENSION_MISMATCH, lambda: lib.GrB_Row_assign(c._h, g4._h, None, g4._h, 2, *J4[:2], None)),
            (DIMENSION_MISMATCH, lambda: lib.GrB_Row_assign(c._h, m70._h, plus, g4._h, 2, *J4[:2], None)),
            (DIMENSION_MISMATCH, lambda: lib.GrB_Col_assign(c._h, m90._h, None, g3._h, *I3[:2], 2, None)),
            (DIMENSION_MISMATCH, lambda: lib.GxB_Col_subassign(c._h, m70._h, None, g3._h, *I3[:2], 2, None)),
            (DIMENSION_MISMATCH, lambda: lib.GxB_Vector_subassign(w._h, None, None, g4._h, *K3[:2], None)),
            (DIMENSION_MISMATCH, lambda: lib.GxB_Vector_subassign(w._h, w._h, plus, g3._h, *K3[:2], None)),
            (DIMENSION_MISMATCH, lambda: lib.GxB_Vector_subassign_Scalar(w._h, w._h, None, s, *K3[:2], None)),
            # a null handle
            (NULL_POINTER, lambda: lib.GxB_Matrix_subassign(None, None, None, a._h, *I3[:2], *J4[:2], None)),
            (NULL_POINTER, lambda: lib.GxB_Matrix_subassign(c._h, None, None, None, *I3[:2], *J4[:2], None)),
            (NULL_POINTER, lambda: lib.GxB_Matrix_subassign_Scalar(c._h, None, None, None, *I3[:2], *J4[:2], None)),
            (NULL_POINTER, lambda: lib.GrB_Row_assign(c._h, None, None, None, 2, *J4[:2], None)),
            (NULL_POINTER, lambda: lib.GxB_Col_subassign(c._h, None, None, None, *I3[:2], 2, None)),
            (NULL_POINTER, lambda: lib.GxB_Vector_subassign(w._h, None, None, None, *K3[:2], None)),
            (NULL_POINTER, lambda: lib.GxB_Matrix_subassign(c._h, None, None, a._h, None, 3, *J4[:2], None)),
        ]
        for k, (code, call) in enumerate(calls):
            assert call() == code, f"refusal {k}"
            check(c, C, dt, what=f"C after refusal {k}")
            check(w, W, dt, what=f"w after refusal {k}")
