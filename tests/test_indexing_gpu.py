"""GPU parity of the operations that edit structure by index -- GrB_Matrix_extract, GrB_Col_extract,
GrB_Vector_extract (gb_extract.hip), scalar and object assign (gb_ops.hip), setElement,
removeElement, extractElement, resize, dup and clear (gb_object.hip) -- with the dense numpy model
of tests/dense_model.py.  The cases and their expectations are tables in tests/indexing_cases.py
(walked on the CPU by test_dense_model.py); this file runs them on the device.

Everything is index and byte work: every comparison is exact, through to_coo() -- indices, their
order, nvals, the dtype and the values by bits (test_general_ops_gpu.check).  isequal never judges.

Shapes, and the path each one is for
  matrix extract  70 x 300 with rows of 0, 1, 63, 64, 65, 128, 129 and 300 entries: the 64-entry
                  chunk loop of k_ext_rows runs 0, 1, 2, 3 and 5 times and the output cursor is
                  carried across chunks; J = column 137 two hundred times, stored in the 129-entry
                  row, writes `pos + k` across a chunk boundary; 140000 x 70 with 133125 output
                  rows: the wave-tile scan (scanw) of cnt and the wave stride loop above 65536
                  rows, again with knob scan_u8 = 1 (hipCUB), and 131071 rows (hipCUB by size);
                  70 x 140000 with 3000 columns: the tile scan of jcnt
  col extract     lines of 0, 1, 65 and 1000 entries (the depth of k_ext_col's binary search), index
                  lists of 1, 63, 64, 65, 257 and 1000 (a partial last bitmap word, four blocks)
  vectors         1, 63, 64, 65, 70001; scalar assign also 1023 .. 4133 around k_assign_mask_words'
                  16 words per wave step and 64 per block, 262245 past k_assign_all_scalar's 1024
                  blocks, and 2048 * 64 * 64 + 64 * 5 + 37 inside k_assign_mask_words' stride loop
  matrices        70 x 90 (off the column-word format), 40 x 90 (on it), 1 x 1

Two invariants are checked along the way, not in tests of their own:
  tail bits       after every vector-producing call at n = 1, 63, 65 the exported bitmap equals the
                  packed model bits word for word (no bit at or beyond n) and resize(n + 64) on a
                  copy reveals no entry (check_obj)
  stale transposes  after every mutator of a matrix whose CSC copy is cached, A.T.new(), A[I, j],
                  A.T.mxv(u) and a GrB_DESC_T0 extract agree with the model of the mutated A
"""
import ctypes

import numpy as np
import pytest

import dense_model as dm
import indexing_cases as ic
from test_general_ops_gpu import _knobs, check, iso_gb, to_gb

pytestmark = pytest.mark.gpu

INDEX_OUT_OF_BOUNDS, INVALID_INDEX, DIMENSION_MISMATCH, NOT_IMPLEMENTED, NO_VALUE = -105, -4, -6, -8, 1


@pytest.fixture(scope="module")
def gb():
    import graphblas_amd

    return graphblas_amd


def test_case_tables_cover_the_issue():
    ic.assert_coverage()
    assert sum(len(ic.cases(op)) for op in ic.OPS) == ic.CASE_COUNT


# ---------------------------------------------------------------------- device <-> model
def is_iso(obj):
    from graphblas_amd.device import matrix_view, vector_view

    return bool((vector_view if obj.ndim == 1 else matrix_view)(obj._h).iso)


def dev(gb, X, kind="sparse"):
    """the device object of a model object: built from a scalar for the iso kinds, never written
    for `never`"""
    p, v = X
    dt = dm.name_of(v.dtype)
    if kind == "never":
        return gb.Vector(dt, p.shape[0]) if p.ndim == 1 else gb.Matrix(dt, *p.shape)
    if kind in ("iso", "iso_true", "iso_false") and p.any():
        g = iso_gb(gb, p, v[p][0], dt)[0]
        assert is_iso(g)
        return g
    return to_gb(gb, X)


def bitmap_words(gb, w):
    """the vector's bitmap as GxB_Vector_bitmap_export copies it (device to device)"""
    import torch

    nw = (w.size + 63) // 64
    buf = torch.zeros(max(nw, 1), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    assert gb.lib.GxB_Vector_bitmap_export(w._h, ctypes.c_void_p(buf.data_ptr()), nw) == 0
    torch.cuda.synchronize()
    return buf.cpu().numpy().view(np.uint64)[:nw]


def check_obj(gb, obj, want, dt, what):
    """check(), and for a vector of 1, 63 or 65 the tail-bit invariant"""
    check(obj, want, dt, what=what)
    if obj.ndim == 1 and obj.size in (1, 63, 65):
        n = obj.size
        bits = np.zeros(((n + 63) // 64) * 64, bool)
        bits[:n] = want[0]
        packed = np.packbits(bits, bitorder="little").view(np.uint64)
        got = bitmap_words(gb, obj)
        assert np.array_equal(got, packed), f"{what}: bitmap {got.tolist()}, expected {packed.tolist()}"
        grown = obj.dup()
        grown.resize(n + 64)
        check(grown, dm.resize(want, n + 64), dt, what=f"{what}, then resize({n + 64})")


def key_of(I):
    return slice(None) if I is None else I


def bind(gb, c, wb, m):
    """c(mask, accum, replace) of a write-back variant"""
    kind, rep, acc = wb
    kw = {}
    if kind != "none":
        mk = m.S if "S" in kind else m.V
        kw["mask"] = ~mk if kind.startswith("~") else mk
        kw["replace"] = rep
    if acc is not None:
        kw["accum"] = getattr(gb.binary, acc)
    return c(**kw)


def outputs(gb, c, B, a):
    """the output and the mask of an extract case, aliased as the case says"""
    alias = c.get("alias")
    cobj = a if alias == "C=A" else to_gb(gb, B.C)
    m = {"M=C": cobj, "M=A": a}.get(alias)
    return cobj, (to_gb(gb, B.M) if m is None else m)


# ---- the C ABI, for what the front end does not take
def abi_list(gb, I, n):
    """(pointer, count, the array to keep alive)"""
    if I is None:
        return gb.lib.GrB_ALL, n, None
    a = np.ascontiguousarray(I, np.uint64)
    return ctypes.c_void_p(a.ctypes.data), a.size, a


def abi_out(gb, wb, m, ct, tran=False):
    """(mask, accum, descriptor) arguments of a write-back variant"""
    from graphblas_amd.base import descriptor_lookup

    kind, rep, acc = wb
    d = descriptor_lookup(output_replace=rep, mask_complement=kind.startswith("~"), mask_structure="S" in kind,
                          transpose_first=tran)
    return (None if kind == "none" else m._h, None if acc is None else getattr(gb.binary, acc)[ct]._carg,
            None if d is None else d._carg)


class EmptyScalar:
    def __init__(self, gb, dt):
        self.lib, self.h = gb.lib, ctypes.c_void_p()
        assert self.lib.GrB_Scalar_new(ctypes.byref(self.h), getattr(self.lib, f"GrB_{dt}")) == 0

    def __enter__(self):
        return self.h

    def __exit__(self, *a):
        self.lib.GrB_Scalar_free(ctypes.byref(self.h))


# ---------------------------------------------------------------------- extract
@pytest.mark.parametrize("c", ic.cases("matrix_extract"), ids=lambda c: c.id)
def test_matrix_extract(gb, c):
    B = ic.build(c)
    a = dev(gb, B.A, c.get("kind", "sparse"))
    wb = c.get("wb")
    with _knobs(gb, scan_u8=c.get("scan_u8", 0)):
        if c.get("tran"):  # GrB_DESC_T0 through the ABI, on a matrix whose CSC is already cached
            assert gb.lib.GxB_Matrix_prepare_transpose(a._h) == 0
            got, m = outputs(gb, c, B, a)
            mask, accum, desc = abi_out(gb, wb, m, B.want_dt, tran=True)
            Ip, ni, _i = abi_list(gb, B.I, B.A[0].shape[1])
            Jp, nj, _j = abi_list(gb, B.J, B.A[0].shape[0])
            assert gb.lib.GrB_Matrix_extract(got._h, mask, accum, a._h, Ip, ni, Jp, nj, desc) == 0
        elif wb is None:
            got = a[key_of(B.I), key_of(B.J)].new()
            if c.get("kind") == "iso":
                assert is_iso(got), f"{c.id}: the extract of an iso matrix is not iso"
        else:
            got, m = outputs(gb, c, B, a)
            bind(gb, got, wb, m) << a[key_of(B.I), key_of(B.J)]
    check_obj(gb, got, B.want, B.want_dt, c.id)


def test_matrix_extract_into_a_vector_through_the_abi(gb):
    """GrB_Matrix_extract admits a GrB_Vector output when nj = 1; the front end never takes it"""
    A = ic.matrix_named("rows", "INT32")
    a = to_gb(gb, A)
    for name in ("special", "len65", "len1", "all"):
        I = ic.index_named(name, 70, ("vector output",))
        n = 70 if I is None else I.size
        for wb in (ic.WB_PLAIN, ("~S", True, "plus")):
            W, M = ic.obj("INT32", (n,), ("vector output", name), 0.4), ic.mask_obj((n,), ("vector output", name))
            w, m = to_gb(gb, W), to_gb(gb, M)
            mask, accum, desc = abi_out(gb, wb, m, "INT32")
            Ip, ni, _i = abi_list(gb, I, 70)
            Jp, nj, _j = abi_list(gb, [ic.HOT_COL], 300)
            assert gb.lib.GrB_Matrix_extract(w._h, mask, accum, a._h, Ip, ni, Jp, nj, desc) == 0
            T = dm.extract(A, I, [ic.HOT_COL])
            want = dm.write_back(W, (T[0][:, 0], T[1][:, 0]), **ic.wb_kw(wb, M))
            check_obj(gb, w, want, "INT32", f"vector output, I={name}, {wb}")


def test_extract_errors_leave_the_output_untouched(gb):
    lib = gb.lib
    A = ic.matrix_named("small", "INT64")
    a = to_gb(gb, A)
    C = ic.obj("INT64", (3, 4), "errors", 0.6)
    c = to_gb(gb, C)
    plus = gb.binary.plus["INT64"]._carg
    for I, J, rc in (([0, 70, 1], [1, 2, 3, 4], INDEX_OUT_OF_BOUNDS), ([0, 1, 2], [1, 2, 3, 90], INDEX_OUT_OF_BOUNDS),
                     ([0, 1], [1, 2, 3, 4], DIMENSION_MISMATCH), ([0, 1, 2], [1, 2, 3], DIMENSION_MISMATCH),
                     ([], [1, 2, 3, 4], DIMENSION_MISMATCH)):
        Ip, ni, _i = abi_list(gb, I, 70)
        Jp, nj, _j = abi_list(gb, J, 90)
        assert lib.GrB_Matrix_extract(c._h, None, plus, a._h, Ip, ni, Jp, nj, None) == rc, (I, J)
        check(c, C, "INT64", what=f"C after the refused extract {I} x {J}")
    W = ic.obj("INT64", (3,), "errors", 0.7)
    w = to_gb(gb, W)
    u = to_gb(gb, ic.obj("INT64", (70,), "errors u"))
    Ip, ni, _i = abi_list(gb, [0, 1, 2], 70)
    from graphblas_amd.base import descriptor_lookup
    t0 = descriptor_lookup(transpose_first=True)._carg
    assert lib.GrB_Col_extract(w._h, None, None, a._h, Ip, ni, 90, None) == INVALID_INDEX
    assert lib.GrB_Col_extract(w._h, None, None, a._h, Ip, ni, 70, t0) == INVALID_INDEX
    Bp, nb, _b = abi_list(gb, [0, 70, 2], 70)
    assert lib.GrB_Col_extract(w._h, None, None, a._h, Bp, nb, 5, None) == INDEX_OUT_OF_BOUNDS
    assert lib.GrB_Vector_extract(w._h, None, None, u._h, Bp, nb, None) == INDEX_OUT_OF_BOUNDS
    Sp, ns, _s = abi_list(gb, [0, 1], 70)
    assert lib.GrB_Col_extract(w._h, None, None, a._h, Sp, ns, 5, None) == DIMENSION_MISMATCH
    assert lib.GrB_Vector_extract(w._h, None, plus, u._h, Sp, ns, None) == DIMENSION_MISMATCH
    check_obj(gb, w, W, "INT64", "w after the refused extracts")


@pytest.mark.parametrize("orient", ["col", "row"])
def test_col_extract(gb, orient):
    devs = {}
    for c in ic.cases("col_extract"):
        if c.p["orient"] != orient:
            continue
        B = ic.build(c)
        k = (c.p["dt"], c.get("kind", "sparse"))
        if k not in devs:
            devs[k] = dev(gb, B.A, k[1])
        a = devs[k]
        expr = a[key_of(B.I), B.j] if orient == "col" else a[B.j, key_of(B.I)]
        if c.get("wb") is None:
            got = expr.new()
            if c.get("kind") == "iso":
                assert is_iso(got), c.id
        else:
            got, m = outputs(gb, c, B, a)
            bind(gb, got, c.p["wb"], m) << expr
        check_obj(gb, got, B.want, B.want_dt, c.id)


@pytest.mark.parametrize("n", sorted({c.p["n"] for c in ic.cases("vector_extract")}))
def test_vector_extract(gb, n):
    for c in ic.cases("vector_extract"):
        if c.p["n"] != n:
            continue
        B = ic.build(c)
        u = dev(gb, B.A, c.p["kind"])
        if c.get("wb") is None:
            got = u[key_of(B.I)].new()
            if c.p["kind"] == "iso" and B.A[0].any():
                assert is_iso(got), c.id
        else:
            got, m = outputs(gb, c, B, u)
            bind(gb, got, c.p["wb"], m) << u[key_of(B.I)]
        check_obj(gb, got, B.want, B.want_dt, c.id)


# ---------------------------------------------------------------------- assign
def run_vector_assign_scalar(gb, c, B):
    n, dt, wb = c.p["n"], c.p["dt"], c.p["wb"]
    w = dev(gb, B.w, c.p["w"])
    m = None if B.M is None else (w if c.p["mask"] == "alias" else dev(gb, B.M, c.p["mask"]))
    if B.x is not None and B.xdt == dt:
        bind(gb, w, wb, m)[key_of(B.I)] = B.x.item()
    else:  # the empty scalar, and a scalar of another type through that type's entry point
        mask, accum, desc = abi_out(gb, wb, m, dt)
        Ip, ni, _i = abi_list(gb, B.I, n)
        if B.x is None:
            with EmptyScalar(gb, B.xdt) as s:
                assert gb.lib.GrB_Vector_assign_Scalar(w._h, mask, accum, s, Ip, ni, desc) == 0
        else:
            assert getattr(gb.lib, f"GrB_Vector_assign_{B.xdt}")(w._h, mask, accum, B.x.item(), Ip, ni, desc) == 0
    check_obj(gb, w, B.want, dt, c.id)
    if wb == ic.WB_PLAIN and B.I is None and B.x is not None:
        assert is_iso(w), f"{c.id}: w = x over everything is not iso"


@pytest.mark.parametrize("fuse_assign", [0, 1])
@pytest.mark.parametrize("n", ic.ASSIGN_SIZES)
def test_vector_assign_scalar(gb, n, fuse_assign):
    with _knobs(gb, fuse_assign=fuse_assign):
        for c in ic.cases("vector_assign_scalar"):
            if c.p["n"] == n:
                run_vector_assign_scalar(gb, c, ic.build(c))


ACTIONS = ["nvals", "to_coo", "element", "set", "del", "dup", "resize", "ewise", "mask", "q_set", "q_clear",
           "q_resize", "q_del"]


@pytest.mark.parametrize("fuse_assign", [0, 1])
@pytest.mark.parametrize("kind", ["V", "S"])
@pytest.mark.parametrize("action", ACTIONS)
def test_deferred_assign_is_never_observable(gb, action, kind, fuse_assign):
    """w(q.V)[:] = x with an iso q, and w(q.S)[:] = x, may be recorded and carried out later; whatever
    comes next must find everything as if it had run at once"""
    n = 300
    W = ic.obj("INT32", (n,), "deferral w")
    Q = ic.mask_obj((n,), "deferral q", "iso_true" if kind == "V" else "sparse")
    O = ic.obj("INT32", (n,), "deferral other")
    S = dict(mask_struct=kind == "S")
    with _knobs(gb, fuse_assign=fuse_assign):
        w, q, o = to_gb(gb, W), dev(gb, Q, "iso_true" if kind == "V" else "sparse"), to_gb(gb, O)
        i_in, i_out = int(np.flatnonzero(Q[0])[3]), int(np.flatnonzero(~Q[0])[3])
        w(mask=q.V if kind == "V" else q.S)[:] = 5
        W = dm.assign_vec(W, np.int32(5), None, mask=Q, **S)
        what = f"after {action}"
        if action == "nvals":
            assert w.nvals == W[0].sum()
        elif action == "element":
            assert w[i_in].value == 5
            assert w[i_out].value == (int(W[1][i_out]) if W[0][i_out] else None)
        elif action == "set":
            w[i_in] = 9
            w[i_out] = -9
            W = dm.set_element(dm.set_element(W, i_in, 9), i_out, -9)
        elif action == "del":
            del w[i_in]
            W = dm.remove_element(W, i_in)
        elif action == "dup":
            d = w.dup()
            w[i_in] = 9
            check(d, W, "INT32", what="the copy")
            W = dm.set_element(W, i_in, 9)
        elif action == "resize":
            w.resize(200)
            W = dm.resize(W, 200)
        elif action == "ewise":
            check(w.ewise_add(o, gb.binary.plus).new(), dm.ewise("add", "plus", "INT32", W, O), "INT32", what=what)
            check(o.ewise_mult(w, gb.binary.minus).new(), dm.ewise("mult", "minus", "INT32", O, W), "INT32", what=what)
        elif action == "mask":
            r = gb.Vector("INT32", n)
            r(w.S) << o
            empty = ic.obj("INT32", (n,), "r", kind="empty")
            check(r, dm.write_back(empty, O, mask=W, mask_struct=True), "INT32", what=what)
        elif action == "q_set":
            q[i_out] = True
            Q = dm.set_element(Q, i_out, True)
        elif action == "q_clear":
            q.clear()
            Q = ic.mask_obj((n,), "cleared", "empty")
        elif action == "q_resize":
            q.resize(100)
            Q = dm.resize(Q, 100)
        elif action == "q_del":
            del q
            q = None
        check(w, W, "INT32", what=f"w {what}")
        if q is not None:
            check(q, Q, "BOOL", what=f"q {what}")
        check(o, O, "INT32", what=f"the bystander {what}")


@pytest.mark.parametrize("n", sorted({c.p["n"] for c in ic.cases("vector_assign")}))
def test_vector_assign(gb, n):
    for c in ic.cases("vector_assign"):
        if c.p["n"] != n:
            continue
        B = ic.build(c)
        w, u = to_gb(gb, B.w), dev(gb, B.u, c.p["u"])
        m = {"M=w": w, "M=u": u}.get(c.get("alias"))
        m = to_gb(gb, B.M) if m is None else m
        bind(gb, w, c.p["wb"], m)[key_of(B.I)] = u
        check_obj(gb, w, B.want, B.want_dt, c.id)
        if c.get("alias") != "M=u":
            check(u, B.u, dm.name_of(B.u[1].dtype), what=f"{c.id}: u afterwards")


@pytest.mark.parametrize("target", ["small", "low"])
def test_matrix_assign(gb, target):
    for c in ic.cases("matrix_assign"):
        if c.p["C"] != target:
            continue
        B = ic.build(c)
        dt, wb = c.p["dt"], c.p["wb"]
        C, m = to_gb(gb, B.C), to_gb(gb, B.M)
        if c.p["value"] != "scalar":
            a = to_gb(gb, B.A)
            bind(gb, C, wb, m)[:, :] = a.T if c.p["value"] == "A.T" else a
        elif B.x is not None and B.I is None and B.J is None:
            bind(gb, C, wb, m)[:, :] = B.x.item()
        else:
            mask, accum, desc = abi_out(gb, wb, m, dt)
            Ip, ni, _i = abi_list(gb, B.I, B.C[0].shape[0])
            Jp, nj, _j = abi_list(gb, B.J, B.C[0].shape[1])
            if B.x is None:
                with EmptyScalar(gb, dt) as s:
                    assert gb.lib.GrB_Matrix_assign_Scalar(C._h, mask, accum, s, Ip, ni, Jp, nj, desc) == 0
            else:
                fn = getattr(gb.lib, f"GrB_Matrix_assign_{dt}")
                assert fn(C._h, mask, accum, B.x.item(), Ip, ni, Jp, nj, desc) == 0
        check(C, B.want, dt, what=c.id)


def test_matrix_index_list_object_assign_is_refused(gb):
    """a feature the library does not have: GrB_NOT_IMPLEMENTED, and C as it was"""
    C, A = ic.matrix_named("small", "INT64"), ic.obj("INT64", (3, 4), "refused")
    c, a = to_gb(gb, C), to_gb(gb, A)
    for I, J in (([1, 2, 3], [4, 5, 6, 7]), (None, [4, 5, 6, 7]), ([1, 2, 3], None)):
        Ip, ni, _i = abi_list(gb, I, 70)
        Jp, nj, _j = abi_list(gb, J, 90)
        assert gb.lib.GrB_Matrix_assign(c._h, None, None, a._h, Ip, ni, Jp, nj, None) == NOT_IMPLEMENTED
        check(c, C, "INT64", what="C after the refused assign")


# ---------------------------------------------------------------------- stale transposes
def views_agree(gb, a, A, what):
    """everything that reads a's transpose against the model of A as it is now"""
    dt = dm.name_of(A[1].dtype)
    nr, nc = A[0].shape
    rng = ic.rng_of("views", what)
    check(a.T.new(), dm.transpose(A), dt, what=f"{what}: A.T.new()")
    for j in rng.integers(0, nc, 3):
        I = rng.integers(0, nr, 40)
        check(a[I, int(j)].new(), dm.extract_vec((A[0][:, j], A[1][:, j]), I), dt, what=f"{what}: A[I, {j}]")
    U = ic.obj("INT8", (nr,), ("views u", what), 0.6)
    U = U[0], (U[1] % 7).astype(dm.NP[dt])  # 0..6: a float plus_times stays exact in any order
    w = a.T.mxv(to_gb(gb, U), gb.semiring.plus_times).new()
    check(w, dm.mxv("plus", "times", dt, A, U, tran0=True), dt, what=f"{what}: A.T.mxv(u)")
    I, J = rng.integers(0, nc, 30), rng.permutation(nr)[:20]
    c = gb.Matrix(dt, 30, 20)
    Ip, ni, _i = abi_list(gb, I, nc)
    Jp, nj, _j = abi_list(gb, J, nr)
    from graphblas_amd.base import descriptor_lookup
    assert gb.lib.GrB_Matrix_extract(c._h, None, None, a._h, Ip, ni, Jp, nj,
                                     descriptor_lookup(transpose_first=True)._carg) == 0
    check(c, dm.extract(dm.transpose(A), I, J), dt, what=f"{what}: the GrB_DESC_T0 extract")
    check(a, A, dt, what=f"{what}: A itself")


def primed(gb, A, kind="sparse"):
    """a device matrix whose transpose has been built and used"""
    a = dev(gb, A, kind)
    assert gb.lib.GxB_Matrix_prepare_transpose(a._h) == 0
    dt = dm.name_of(A[1].dtype)
    u = to_gb(gb, ic.obj(dt, (A[0].shape[0],), "prime", 0.5))
    a.T.mxv(u, gb.semiring.plus_times).new()
    a[:, 0].new()
    return a


MUTATORS = ["set existing", "set new", "set existing on iso", "set same on iso", "set new on iso", "remove",
            "remove on iso", "resize", "clear and build", "assign matrix", "assign scalar", "assign scalar lists"]


@pytest.mark.parametrize("shape", ["small", "low"])
@pytest.mark.parametrize("mutator", MUTATORS)
def test_no_transpose_survives_a_mutation(gb, mutator, shape):
    iso = "iso" in mutator
    A = ic.matrix_named(shape, "INT64", "iso" if iso else "sparse")
    A = A[0], (A[1] if iso else A[1] % 1000)  # small values: plus_times stays exact in any order
    a = primed(gb, A, "iso" if iso else "sparse")
    views_agree(gb, a, A, f"{mutator} {shape}: before")
    nr, nc = A[0].shape
    rng = ic.rng_of("mutator", mutator, shape)
    present, absent = np.argwhere(A[0]), np.argwhere(~A[0])
    pi, pj = (int(x) for x in present[rng.integers(0, len(present))])
    ai, aj = (int(x) for x in absent[rng.integers(0, len(absent))])
    if mutator in ("set existing", "set existing on iso"):
        a[pi, pj] = -77
        A = dm.set_element(A, (pi, pj), -77)
    elif mutator == "set same on iso":
        a[pi, pj] = int(A[1][pi, pj])
        assert is_iso(a)
    elif mutator in ("set new", "set new on iso"):
        a[ai, aj] = -77
        A = dm.set_element(A, (ai, aj), -77)
    elif mutator in ("remove", "remove on iso"):
        del a[pi, pj]
        A = dm.remove_element(A, (pi, pj))
        assert is_iso(a) == iso
    elif mutator == "resize":
        a.resize(nr - 9, nc + 5)
        A = dm.resize(A, (nr - 9, nc + 5))
    elif mutator == "clear and build":
        a.clear()
        N = ic.obj("INT64", (nr, nc), "rebuilt", 0.25)
        A = N[0], N[1] % 1000
        r, c = np.nonzero(A[0])
        a.build(r, c, A[1][r, c])
    elif mutator == "assign matrix":
        N = ic.obj("INT64", (nr, nc), "assigned", 0.25)
        N = N[0], N[1] % 1000
        a[:, :] = to_gb(gb, N)
        A = dm.assign(A, N)
    elif mutator == "assign scalar":
        M = ic.mask_obj((nr, nc), "assign scalar")
        a(to_gb(gb, M).V)[:, :] = 5
        A = dm.assign(A, np.int64(5), mask=M)
    else:
        I, J = rng.integers(0, nr, 9), rng.integers(0, nc, 11)
        Ip, ni, _i = abi_list(gb, I, nr)
        Jp, nj, _j = abi_list(gb, J, nc)
        assert gb.lib.GrB_Matrix_assign_INT64(a._h, None, None, 5, Ip, ni, Jp, nj, None) == 0
        A = dm.assign(A, np.int64(5), I, J)
    views_agree(gb, a, A, f"{mutator} {shape}: after")


# ---------------------------------------------------------------------- elements
def positions(A):
    """insert positions worth a look: before the first entry of a row, after the last, an empty
    row, the first and the last row; and entries to overwrite or remove: first, last, one inside"""
    p = A[0]
    nr, nc = p.shape
    ins, hit = [], []
    rows = p.sum(axis=1)
    for i in {0, nr - 1, int(np.argmax(rows)), *np.flatnonzero(rows > 0)[:2].tolist()}:
        cols = np.flatnonzero(p[i])
        if cols.size and cols[0] > 0:
            ins.append((i, int(cols[0]) - 1))
        if cols.size and cols[-1] < nc - 1:
            ins.append((i, int(cols[-1]) + 1))
        if cols.size:
            hit += [(i, int(cols[0])), (i, int(cols[-1]))]
        for j in (0, nc - 1, nc // 2):
            if not p[i, j]:
                ins.append((i, j))
    r, c = np.nonzero(p)
    if r.size:
        hit += [(int(r[0]), int(c[0])), (int(r[-1]), int(c[-1])), (int(r[r.size // 2]), int(c[r.size // 2]))]
    return list(dict.fromkeys(ins)), list(dict.fromkeys(hit))


@pytest.mark.parametrize("dt", ["INT8", "UINT16", "FP32", "INT64", "BOOL"])
def test_matrix_set_remove_element(gb, dt):
    x, y = ic.scalar_value(dt, "set x"), ic.scalar_value(dt, "set y")
    A = ic.obj(dt, (70, 90), "elements", 0.1)
    A[0][17] = False  # an empty row
    A = A[0], np.where(A[0], A[1], dm.NP[dt](0))
    ins, hit = positions(A)
    ins.append((17, 40))
    assert len(ins) >= 8 and len(hit) >= 5
    a = to_gb(gb, A)
    for k, ij in enumerate(ins):  # inserts pile up: each one shifts what follows it
        a[ij] = x.item()
        A = dm.set_element(A, ij, x)
        if k % 3 == 0:
            check(a, A, dt, what=f"insert {ij}")
    check(a, A, dt, what="the inserts")
    for ij in hit:
        a[ij] = y.item()
        A = dm.set_element(A, ij, y)
    check(a, A, dt, what="the overwrites")
    for k, ij in enumerate(hit + ins[:3] + [(17, 41)]):  # the last one is absent: no change
        del a[ij]
        A = dm.remove_element(A, ij)
        if k % 3 == 0:
            check(a, A, dt, what=f"remove {ij}")
    check(a, A, dt, what="the removals")
    # an empty matrix, a 1 x 1 matrix, the only entry
    for shape, ij in (((70, 90), (69, 89)), ((70, 90), (0, 0)), ((1, 1), (0, 0))):
        E = ic.obj(dt, shape, "empty", kind="empty")
        e = gb.Matrix(dt, *shape)
        del e[ij]
        check(e, E, dt, what="remove from an empty matrix")
        e[ij] = x.item()
        E = dm.set_element(E, ij, x)
        check(e, E, dt, what=f"insert {ij} into an empty {shape} matrix")
        e[ij] = y.item()
        check(e, dm.set_element(E, ij, y), dt, what="overwrite the only entry")
        del e[ij]
        check(e, dm.remove_element(E, ij), dt, what="remove the only entry")
        e[ij] = x.item()
        check(e, E, dt, what="and insert again")
    # iso: the same value keeps it iso; another value or position de-isos and keeps every other value
    v = ic.iso_value(dt)
    other = dm.NP[dt](not v) if dt == "BOOL" else dm.NP[dt](3)
    I = ic.obj(dt, (70, 90), "iso elements", 0.1, kind="iso")
    ins, hit = positions(I)
    g = dev(gb, I, "iso")
    g[hit[0]] = v.item()
    assert is_iso(g)
    check(g, I, dt, what="iso: the same value over an entry")
    del g[hit[1]]
    I = dm.remove_element(I, hit[1])
    assert is_iso(g)
    check(g, I, dt, what="iso: remove")
    g[hit[2]] = other.item()
    I = dm.set_element(I, hit[2], other)
    check(g, I, dt, what="iso: another value over an entry")
    I = ic.obj(dt, (70, 90), "iso elements 2", 0.1, kind="iso")
    g = dev(gb, I, "iso")
    new = positions(I)[0][0]
    assert not I[0][new]
    g[new] = other.item()
    check(g, dm.set_element(I, new, other), dt, what="iso: another value at a new position")


@pytest.mark.parametrize("n", [1, 64, 65, 5000])
def test_vector_set_remove_element(gb, n):
    for dt in ("INT8", "FP64", "BOOL", "UINT32"):
        x, y = ic.scalar_value(dt, "vset x"), ic.scalar_value(dt, "vset y")
        for kind in ("sparse", "never", "iso", "full"):
            W = ic.obj(dt, (n,), ("velements", kind), 0.4, kind=kind)
            w = dev(gb, W, kind)
            spots = sorted({0, n - 1, n // 2, min(63, n - 1), min(64, n - 1)})
            for k, i in enumerate(spots):
                val = x if k % 2 == 0 else y
                w[i] = val.item()
                W = dm.set_element(W, i, val)
            check_obj(gb, w, W, dt, f"{dt} {kind} {n}: the sets")
            S = ic.obj(dt, (n,), ("velements", kind), 0.4, kind=kind)
            if kind == "iso" and S[0].any():
                same = dev(gb, S, kind)
                i = int(np.flatnonzero(S[0])[0])
                same[i] = ic.iso_value(dt).item()
                assert is_iso(same)
                check_obj(gb, same, S, dt, f"{dt} iso {n}: the same value")
            for i in spots[::2] + [spots[0]]:  # the last one is absent by now
                del w[i]
                W = dm.remove_element(W, i)
            check_obj(gb, w, W, dt, f"{dt} {kind} {n}: the removals")


def test_extract_element_casts_and_index_errors(gb):
    lib = gb.lib
    A = ic.obj("FP64", (70, 90), "extractElement", 0.3)
    a = to_gb(gb, A)
    W = ic.obj("INT64", (65,), "extractElement", 0.5)
    w = to_gb(gb, W)
    rng = ic.rng_of("extractElement")
    for dt in ("INT8", "UINT8", "BOOL", "INT64", "FP32"):
        out = np.zeros(1, dm.NP[dt])
        ptr = ctypes.c_void_p(out.ctypes.data)
        for i, j in zip(rng.integers(0, 70, 40), rng.integers(0, 90, 40)):
            rc = getattr(lib, f"GrB_Matrix_extractElement_{dt}")(ptr, a._h, int(i), int(j))
            assert rc == (0 if A[0][i, j] else NO_VALUE)
            if A[0][i, j]:
                assert np.array_equal(out, dm.cast(A[1][i:i + 1, j], dt), equal_nan=True), (dt, i, j, A[1][i, j])
        for i in range(65):
            rc = getattr(lib, f"GrB_Vector_extractElement_{dt}")(ptr, w._h, i)
            assert rc == (0 if W[0][i] else NO_VALUE)
            if W[0][i]:
                assert np.array_equal(out, dm.cast(W[1][i:i + 1], dt)), (dt, i)
    out = np.zeros(1, np.float64)
    ptr = ctypes.c_void_p(out.ctypes.data)
    for i, j in ((70, 0), (0, 90), (2**40, 0)):
        assert lib.GrB_Matrix_extractElement_FP64(ptr, a._h, i, j) == INVALID_INDEX
        assert lib.GrB_Matrix_setElement_FP64(a._h, 1.0, i, j) == INVALID_INDEX
        assert lib.GrB_Matrix_removeElement(a._h, i, j) == INVALID_INDEX
    for i in (65, 2**40):
        assert lib.GrB_Vector_extractElement_FP64(ptr, w._h, i) == INVALID_INDEX
        assert lib.GrB_Vector_setElement_INT64(w._h, 1, i) == INVALID_INDEX
        assert lib.GrB_Vector_removeElement(w._h, i) == INVALID_INDEX
    check(a, A, "FP64", what="A after the refused calls")
    check_obj(gb, w, W, "INT64", "w after the refused calls")


@pytest.mark.parametrize("ndim", [1, 2])
def test_mixed_element_sequence(gb, ndim):
    """200 seeded set / remove / read steps, compared with the model after every 20"""
    shape = (70, 90) if ndim == 2 else (65,)
    X = ic.obj("INT32", shape, "sequence", 0.15)
    x = to_gb(gb, X)
    rng = ic.rng_of("sequence", ndim)
    for step in range(200):
        idx = tuple(int(rng.integers(0, s)) for s in shape)
        if rng.random() < 0.4 and X[0].any():  # aim at an entry
            hits = np.argwhere(X[0])
            idx = tuple(int(t) for t in hits[rng.integers(0, len(hits))])
        key = idx if ndim == 2 else idx[0]
        op = rng.integers(0, 3)
        if op == 0:
            val = int(rng.integers(-2**31, 2**31))
            x[key] = val
            X = dm.set_element(X, idx, val)
        elif op == 1:
            del x[key]
            X = dm.remove_element(X, idx)
        else:
            assert x[key].value == (int(X[1][idx]) if X[0][idx] else None), (step, idx)
        if step % 20 == 19:
            check_obj(gb, x, X, "INT32", f"after step {step}")


# ---------------------------------------------------------------------- resize, dup, clear
def test_matrix_resize(gb):
    for dt, kind in (("INT16", "sparse"), ("FP64", "iso")):
        A = ic.obj(dt, (70, 90), ("resize", kind), 0.2, kind=kind)
        A[0][:, 40:] &= ic.rng_of("resize rows").random((70, 1)) < 0.5  # half the rows end before column 40
        A = A[0], np.where(A[0], A[1], dm.NP[dt](0))
        for shapes in ([(90, 90)], [(30, 90)], [(70, 120)], [(70, 40)], [(100, 50)], [(20, 130)], [(0, 0), (5, 5)],
                       [(0, 90), (70, 90)], [(70, 0), (70, 90)], [(1, 1), (70, 90)], [(30, 40), (70, 90)]):
            a, M = dev(gb, A, kind), A
            for s in shapes:
                a.resize(*s)
                M = dm.resize(M, s)
                assert tuple(a.shape) == s and (kind != "iso" or is_iso(a) or not M[0].any())
                check(a, M, dt, what=f"{dt} {kind} 70 x 90 -> {shapes} at {s}")
        e = gb.Matrix(dt, 0, 0)  # grow from 0 x 0, then use
        e.resize(3, 4)
        e[2, 3] = ic.iso_value(dt).item()
        check(e, dm.set_element(ic.obj(dt, (3, 4), "grown", kind="empty"), (2, 3), ic.iso_value(dt)), dt,
              what="grown from 0 x 0")


@pytest.mark.parametrize("scan_u8", [0, 1])
def test_matrix_resize_tall(gb, scan_u8):
    """140000 x 70 -> 133125 x 40: the row counts go through the wave-tile scan, or hipCUB"""
    A = ic.matrix_named("tall", "INT32")
    a = to_gb(gb, A)
    with _knobs(gb, scan_u8=scan_u8):
        a.resize(133125, 40)
    check(a, dm.resize(A, (133125, 40)), "INT32", what="tall resize")


def test_vector_resize(gb):
    for dt in ("INT8", "FP64"):
        for kind in ("sparse", "iso", "full", "never"):
            W = ic.obj(dt, (65,), ("vresize", kind), 0.7, kind=kind)
            w = dev(gb, W, kind)
            for n in (64, 63, 1, 0, 130):  # whatever was cut off must not come back
                w.resize(n)
                W = dm.resize(W, n)
                assert w.size == n
                check_obj(gb, w, W, dt, f"{dt} {kind}: 65 -> ... -> {n}")
            assert w.nvals == 0
            w[129] = ic.iso_value(dt).item()
            check(w, dm.set_element(W, 129, ic.iso_value(dt)), dt, what="use after the resizes")
            for n0, n1 in ((1, 65), (63, 64), (63, 127), (65, 5000), (5000, 65)):
                W = ic.obj(dt, (n0,), ("vgrow", kind, n0), 0.7, kind=kind)
                w = dev(gb, W, kind)
                w.resize(n1)
                check_obj(gb, w, dm.resize(W, n1), dt, f"{dt} {kind}: {n0} -> {n1}")
                w.resize(n0)
                check_obj(gb, w, dm.resize(dm.resize(W, n1), n0), dt, f"{dt} {kind}: {n0} -> {n1} -> {n0}")


def test_dup_is_independent(gb):
    for kind in ("sparse", "iso", "empty"):
        A = ic.obj("INT32", (70, 90), ("dup", kind), 0.2, kind=kind)
        a = primed(gb, A, kind) if kind != "empty" else gb.Matrix("INT32", 70, 90)
        b = a.dup()
        a[3, 3] = 41
        check(b, A, "INT32", what=f"{kind}: the copy after the original changed")
        views_agree(gb, b, A, f"dup {kind}: the copy")
        b[4, 4] = 42
        del b[3, 3]
        check(a, dm.set_element(A, (3, 3), 41), "INT32", what=f"{kind}: the original after the copy changed")
        check(b, dm.remove_element(dm.set_element(A, (4, 4), 42), (3, 3)), "INT32", what=f"{kind}: the copy")
        W = ic.obj("INT32", (65,), ("dup", kind), 0.4, kind=kind)
        w = dev(gb, W, "never" if kind == "empty" else kind)
        d = w.dup()
        w[64] = 41
        check_obj(gb, d, W, "INT32", f"{kind}: the vector copy after the original changed")
        d[0] = 42
        check_obj(gb, w, dm.set_element(W, 64, 41), "INT32", f"{kind}: the vector after its copy changed")
        check_obj(gb, d, dm.set_element(W, 0, 42), "INT32", f"{kind}: the vector copy")


def test_clear_then_reuse(gb):
    A = ic.obj("FP32", (70, 90), "clear", 0.2)
    a = primed(gb, A)
    a.clear()
    E = ic.obj("FP32", (70, 90), "clear", kind="empty")
    check(a, E, "FP32", what="cleared")
    a[69, 0] = 1.5
    a[0, 89] = -0.0
    E = dm.set_element(dm.set_element(E, (69, 0), 1.5), (0, 89), -0.0)
    views_agree(gb, a, E, "cleared and refilled")
    for kind in ("sparse", "iso", "full"):
        W = ic.obj("FP32", (65,), ("clear", kind), kind=kind)
        w = dev(gb, W, kind)
        w.clear()
        Z = ic.obj("FP32", (65,), "clear", kind="empty")
        check_obj(gb, w, Z, "FP32", f"{kind}: cleared")
        w[64] = 2.5
        w(accum=gb.binary.plus) << to_gb(gb, W)
        check_obj(gb, w, dm.write_back(dm.set_element(Z, 64, 2.5), W, accum="plus"), "FP32", f"{kind}: reused")
