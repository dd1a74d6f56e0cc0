"""GPU parity of GxB_Matrix_eWiseUnion / GxB_Vector_eWiseUnion (csrc/gb_ewise_union.hip) with the
numpy model of tests/union_model.py, through the front end and through ctypes.

Every comparison goes through to_coo() and is exact, except pow, atan2 and hypot on floats, held
to the ULP_BOUND table of test_general_ops_gpu.py (the evaluator is the same device gb_binop_z).
The stat_union_* counters are asserted against the model's counts, so each of the three cases
(both stored, A only, B only) is known to have run.

Shapes, and the path each one is for
  vectors  1, 63, 64, 65   one bitmap word: tail lanes, a full word, one bit in a second word (at
                           1, 63, 65 the exported bitmap words are compared: no bit at or past n)
           70001, 262245   many blocks; 1024 x 256 + 64 + 37 is past the vector kernel's 1024
                           blocks: a second grid sweep ending in a partial word
  matrices 70 x 300        rows of 0, 1, 63, 64, 65, 128, 129, 300 entries in A against B rows that
                           are empty, identical, a subset, a superset, interleaved, before, after
           400 x 40        runs of more than 64 empty rows in A, in B and in both (the row search)
           10 x 300        B with exactly 64, 128, 129 entries: a full last mark word and the zero
                           word after it
           301 x 6007      a 5200-entry hub row in A, in B, and a 3000-entry one in both with half
                           the columns shared: where a serial row walk and a balanced one differ
           133125 x 64, 131071 x 64   about 2 x 10^5 entries over 10^5 rows of 0..3: many chunks
                           per wave with the per-lane row boundaries, B row pointers that name the
                           word after the last mark word, and the write-back's row scans on the
                           wave-tile path and (scan_u8 = 1, or one row fewer) on hipCUB.  The
                           mark-word scan itself takes its wave-tile path only from 2^24 entries
                           of B on: tools/ewise_union_probe.py compares results at that size.
There is one matrix path (no union_method knob): see DESIGN.md §4.
"""
import ctypes

import numpy as np
import pytest

import dense_model as dm
import union_model as um
from test_general_ops_gpu import (BINARY, MIXED, ULP_BOUND, _knobs, binary_inputs, check, draw, heavy, iso_gb,
                                  ragged, specials, to_gb)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gb():
    import graphblas_amd

    return graphblas_amd


def rng_of(*key):
    import zlib

    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def stats(gb):
    return tuple(gb.get_knob(f"stat_union_{c}") for c in ("both", "a_only", "b_only"))


def masked(A):
    """(present, values) with the values outside the structure zeroed"""
    p, v = A
    return p, np.where(p, v, v.dtype.type(0))


def union_check(gb, op, dt, A, al, B, be, *, a=None, b=None, what="", ulps=False, zero_sign=True):
    """a.ewise_union(b, op[dt], al, be).new() against the model, counters included"""
    a = to_gb(gb, A) if a is None else a
    b = to_gb(gb, B) if b is None else b
    got = a.ewise_union(b, getattr(gb.binary, op)[dt], al, be).new()
    counts = stats(gb)
    assert counts == um.case_counts(A, B), f"{what}: counters {counts}"
    d = check(got, um.ewise_union(op, dt, A, al, B, be), dm.binop_return_dtype(op, dt), ulps=ulps,
              zero_sign=zero_sign, what=what)
    return got, d


# ---------------------------------------------------------------------- every operator
def with_all_three_cases(A, B):
    """the last cell only in A, the one before only in B (the first cells hold the special pairs,
    both present): every case is non-empty by construction"""
    (ap, av), (bp, bv) = (A[0].copy(), A[1].copy()), (B[0].copy(), B[1].copy())
    fa, fb = ap.reshape(-1), bp.reshape(-1)  # views
    fa[-1], fb[-1] = True, False
    fa[-2], fb[-2] = False, True
    one = av.dtype.type(1)
    av.reshape(-1)[-1], bv.reshape(-1)[-2] = one, one
    return masked((ap, av)), masked((bp, bv))


def sweep_defaults(op, dt, rng):
    t = dm.NP[dt]
    sp = specials(dt)
    if op in ("min", "max") and dm.is_float(dt):
        sp = sp[sp != 0]  # never -0.0 against +0.0: either answer is right
    al, be = sp[rng.integers(0, sp.size)], sp[rng.integers(0, sp.size)]
    if op == "pow" and dm.is_int(dt):
        al, be = t(2), t(3)  # the domain binary_inputs keeps float64 pow exact in
    if op == "ldexp":
        be = t(7)
    return al, be


@pytest.mark.parametrize("op", BINARY)
def test_every_binary_op(gb, op):
    opobj = getattr(gb.binary, op)
    measured = []
    for dtobj in opobj.types:
        dt = dtobj.name
        if opobj[dt].type.name != dt:
            continue  # a coerced type runs the operator of another type, swept under its own name
        inexact = op in dm.TRANSCENDENTAL and dm.is_float(dt)
        worst = 0
        for shape in [(65,), (37, 53)]:
            A, B = with_all_three_cases(*binary_inputs(op, dt, shape, "union"))
            both, a_only, b_only = um.case_counts(A, B)
            assert both and a_only and b_only
            al, be = sweep_defaults(op, dt, rng_of("defaults", op, dt, shape))
            _, d = union_check(gb, op, dt, A, al, B, be, ulps=inexact, zero_sign=op not in ("min", "max"),
                               what=f"ewise_union {op}[{dt}] {shape} defaults {al!r}, {be!r}")
            worst = max(worst, d)
        if inexact:
            measured.append((op, dt, worst))
    for name, dt, worst in measured:
        print(f"\nULP {name} {dt} {worst} ewise_union")
    for name, dt, worst in measured:
        assert worst <= ULP_BOUND.get((name, dt), 0), f"{name}[{dt}]: {worst} ulps"


# ---------------------------------------------------------------------- matrix structure
ALENS = [0, 1, 63, 64, 65, 128, 129, 300]
RELATIONS = ["empty", "identical", "subset", "superset", "interleaved", "before", "after"]


def edge_rows():
    """70 x 300 presence pair: row 7 k + r holds ALENS[k] entries in A against a B row in
    RELATIONS[r].  A full row leaves no free column: its superset and interleaved rows are
    identical ones, its before / after rows empty ones; an empty row has no strict subset."""
    ap, bp = np.zeros((70, 300), bool), np.zeros((70, 300), bool)
    for k, n in enumerate(ALENS):
        for r, rel in enumerate(RELATIONS):
            i = 7 * k + r
            if rel == "interleaved" and n <= 150:
                a, b = 2 * np.arange(n), 2 * np.arange(max(n, 1)) + 1
            else:
                s = (300 - n) // 2
                a = s + np.arange(n)
                b = {"empty": a[:0], "identical": a, "subset": a[1::2], "interleaved": a,
                     "superset": np.r_[np.arange(s - 1, s) if s else a[:0], a, np.arange(s + n, min(s + n + 2, 300))],
                     "before": np.arange(0, s), "after": np.arange(s + n, 300)}[rel]
            ap[i, a] = True
            bp[i, b.astype(np.int64)] = True
    return ap, bp


def int_values(p, rng):
    return masked((p, rng.integers(-50, 51, p.shape)))


def rowptr_of(gb, C):
    import torch

    from graphblas_amd.device import device_tensor, matrix_view

    view = matrix_view(C._h)
    torch.cuda.synchronize()
    return device_tensor(torch, view.rowptr, C.nrows + 1, "<i8").cpu().numpy()


def model_rowptr(present):
    return np.concatenate([[0], np.cumsum(np.bincount(np.nonzero(present)[0], minlength=present.shape[0]))])


def test_row_length_and_overlap_edges(gb):
    rng = rng_of("edges")
    ap, bp = edge_rows()
    assert [int(x) for x in ap.sum(axis=1)[::7][:len(ALENS)]] == ALENS
    A, B = int_values(ap, rng), int_values(bp, rng)
    got, _ = union_check(gb, "minus", "INT64", A, 1000, B, 100000, what="70 x 300 edges")
    assert np.array_equal(rowptr_of(gb, got), model_rowptr(ap | bp))
    # and with the operands exchanged: the B side now has the long rows
    got, _ = union_check(gb, "minus", "INT64", B, 1000, A, 100000, what="70 x 300 edges, exchanged")
    assert np.array_equal(rowptr_of(gb, got), model_rowptr(ap | bp))


def test_runs_of_empty_rows(gb):
    rng = rng_of("runs")
    ap, bp = rng.random((400, 40)) < 0.3, rng.random((400, 40)) < 0.3
    ap[100:200] = False  # A: 100 empty rows; both: 150 .. 199; B: 150 empty rows
    bp[150:300] = False
    union_check(gb, "minus", "INT64", int_values(ap, rng), 7, int_values(bp, rng), 9, what="empty-row runs")


@pytest.mark.parametrize("bnz", [64, 128, 129])
def test_b_entry_counts_at_word_boundaries(gb, bnz):
    rng = rng_of("words", bnz)
    ap = rng.random((10, 300)) < 0.2
    bp = np.zeros(3000, bool)
    bp[rng.permutation(3000)[:bnz]] = True
    bp = bp.reshape(10, 300)
    A, B = int_values(ap, rng), int_values(bp, rng)
    union_check(gb, "minus", "INT64", A, 7, B, 9, what=f"nnz(B) = {bnz}")
    union_check(gb, "minus", "INT64", B, 7, A, 9, what=f"nnz(A) = {bnz}")
    # every entry of B only in B, then none: the last mark word full of ones, then all zero
    union_check(gb, "plus", "INT64", (np.zeros_like(bp), np.zeros(bp.shape, np.int64)), 7, B, 9, what="A empty")
    union_check(gb, "plus", "INT64", B, 7, B, 9, what="B identical")


def test_degenerate_shapes(gb):
    rng = rng_of("degenerate")
    p = rng.random((37, 53)) < 0.4
    X = int_values(p, rng)
    E = (np.zeros_like(p), np.zeros(p.shape, np.int64))
    union_check(gb, "minus", "INT64", E, 3, X, 5, what="A empty")
    union_check(gb, "minus", "INT64", X, 3, E, 5, what="B empty")
    union_check(gb, "minus", "INT64", E, 3, E, 5, what="both empty")
    one = lambda present, v: (np.array([[present]]), np.array([[v if present else 0]], np.int64))  # noqa: E731
    for pa in (False, True):
        for pb in (False, True):
            union_check(gb, "minus", "INT64", one(pa, 11), 3, one(pb, 4), 5, what=f"1 x 1 {pa} {pb}")
    Z = (np.zeros((0, 5), bool), np.zeros((0, 5), np.int64))
    union_check(gb, "minus", "INT64", Z, 3, Z, 5, what="0 x 5")


def hub_pair():
    """heavy()'s shape with a 3000-entry hub row in both operands, 1500 of its columns shared"""
    A, B = heavy("INT64", "ua", hub_entries=60), heavy("INT64", "ub", hub_entries=60)
    perm = rng_of("hub").permutation(6007)
    for (p, v), cols in ((A, perm[:3000]), (B, perm[1500:4500])):
        p[7] = False
        p[7, cols] = True
        v[7, cols] = 5
    return masked(A), masked(B)


def test_hub_rows(gb):
    H, G = heavy("INT64", "ua"), heavy("INT64", "ub")
    L = heavy("INT64", "ul", hub_entries=60)
    assert H[0][7].sum() == 5200 and L[0][7].sum() == 60
    got, _ = union_check(gb, "minus", "INT64", H, 1000, L, 100000, what="hub in A")
    assert np.array_equal(rowptr_of(gb, got), model_rowptr(H[0] | L[0]))
    got, _ = union_check(gb, "minus", "INT64", L, 1000, G, 100000, what="hub in B")
    assert np.array_equal(rowptr_of(gb, got), model_rowptr(L[0] | G[0]))
    A, B = hub_pair()
    assert (A[0][7] & B[0][7]).sum() == 1500
    got, _ = union_check(gb, "minus", "INT64", A, 1000, B, 100000, what="hub in both")
    assert np.array_equal(rowptr_of(gb, got), model_rowptr(A[0] | B[0]))


@pytest.mark.parametrize("shape,scan_u8", [((133125, 64), 0), ((133125, 64), 1), ((131071, 64), 0)])
def test_many_short_rows(gb, shape, scan_u8):
    A, B = ragged(*shape, "INT32", "ua"), ragged(*shape, "INT32", "ub")
    with _knobs(gb, scan_u8=scan_u8):
        union_check(gb, "minus", "INT32", A, 3, B, 5, what=f"{shape} scan_u8={scan_u8}")


def test_results_repeat_bit_for_bit(gb):
    A, B = hub_pair()
    a, b = to_gb(gb, (A[0], A[1].astype(np.float64) / 3)), to_gb(gb, (B[0], B[1].astype(np.float64) / 7))
    first = a.ewise_union(b, gb.binary.div, 1.5, -2.5).new().to_coo()
    for _ in range(3):
        again = a.ewise_union(b, gb.binary.div, 1.5, -2.5).new().to_coo()
        assert all(x.tobytes() == y.tobytes() for x, y in zip(first, again))  # 0 / 0 is among them: bytes
    assert np.all(np.diff(first[0].astype(np.int64) * 6007 + first[1].astype(np.int64)) > 0)  # columns ascend


# ---------------------------------------------------------------------- vectors
def bitmap_words(gb, w):
    import torch

    nw = (w.size + 63) // 64
    buf = torch.zeros(max(nw, 1), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    assert gb.lib.GxB_Vector_bitmap_export(w._h, ctypes.c_void_p(buf.data_ptr()), nw) == 0
    torch.cuda.synchronize()
    return buf.cpu().numpy().view(np.uint64)[:nw]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 70001, 262245])
def test_vectors(gb, n):
    rng = rng_of("vec", n)
    dt = "INT32"
    sparse = lambda d: masked((rng.random(n) < d, draw(dt, rng, n)))  # noqa: E731
    S1, S2 = sparse(0.5), sparse(0.3)
    F = (np.ones(n, bool), draw(dt, rng, n))
    E = (np.zeros(n, bool), np.zeros(n, dm.NP[dt]))
    iso, I = iso_gb(gb, rng.random(n) < 0.6, 3, dt)
    forms = [("sparse", S1, to_gb(gb, S1)), ("full", F, to_gb(gb, F)), ("empty", E, to_gb(gb, E)), ("iso", I, iso)]
    for na, A, a in forms:
        for nb, B, b in forms + [("sparse2", S2, to_gb(gb, S2))]:
            got, _ = union_check(gb, "minus", dt, A, 1000, B, 100000, a=a, b=b, what=f"n={n} {na},{nb}")
            if n in (1, 63, 65):
                bits = np.zeros(((n + 63) // 64) * 64, bool)
                bits[:n] = A[0] | B[0]
                packed = np.packbits(bits, bitorder="little").view(np.uint64)
                words = bitmap_words(gb, got)
                assert np.array_equal(words, packed), f"n={n} {na},{nb}: bitmap {words.tolist()}"
    # a comparison: BOOL out of INT32 operands
    union_check(gb, "ge", dt, S1, 0, S2, 0, what=f"n={n} ge")


# ---------------------------------------------------------------------- types and casts
@pytest.mark.parametrize("op", ["plus", "div", "min", "eq", "lor", "first", "second", "bxor"])
def test_mixed_dtypes_with_defaults_of_a_fourth_type(gb, op):
    opobj = getattr(gb.binary, op)
    for da, db, dz in MIXED:
        if dz not in [t.name for t in opobj.types] or opobj[dz].type.name != dz:
            continue
        fourth = next(t for t in ("FP32", "INT16", "UINT32", "FP64") if t not in (da, db, dz))
        for shape in [(65,), (37, 53)]:
            rng = rng_of("mixed", op, da, db, shape)
            n = int(np.prod(shape))
            pa, pb = rng.random(shape) < 0.7, rng.random(shape) < 0.7
            va, vb = draw(da, rng, n).reshape(shape), draw(db, rng, n).reshape(shape)
            if op == "min":
                va, vb = np.where(va == 0, dm.NP[da](1), va), np.where(vb == 0, dm.NP[db](1), vb)
            al, be = dm.NP[fourth](3), dm.NP[fourth](200)
            if dm.is_float(fourth):
                al, be = dm.NP[fourth](-2.75), dm.NP[fourth](70000.5)  # truncates, saturates a narrow dz
            A, B = masked((pa, va)), masked((pb, vb))
            # the front end types the operator from the defaults and the operands; pin it instead
            union_check(gb, op, dz, A, al, B, be, what=f"{op}[{dz}] {da} x {db}, defaults {fourth} {shape}")


def test_float_defaults_into_an_int8_operator(gb):
    rng = rng_of("int8")
    for shape in [(65,), (37, 53)]:
        A = masked((rng.random(shape) < 0.6, draw("INT8", rng, int(np.prod(shape))).reshape(shape)))
        B = masked((rng.random(shape) < 0.6, draw("INT8", rng, int(np.prod(shape))).reshape(shape)))
        for al, be in [(np.nan, 1e9), (-1e9, 2.9), (-0.5, 127.9), (np.inf, -np.inf)]:
            for op in ("plus", "minus", "max", "lt"):
                union_check(gb, op, "INT8", A, np.float64(al), B, np.float64(be),
                            what=f"{op}[INT8] defaults {al}, {be} {shape}")
    # through the front end's own typing FP64 defaults make the operator FP64
    a, b = to_gb(gb, A), to_gb(gb, B)
    e = a.ewise_union(b, gb.binary.plus, 0.5, 0.25)
    assert e.op.type == "FP64"
    check(e.new(), um.ewise_union("plus", "FP64", A, 0.5, B, 0.25), "FP64", what="upcast")


@pytest.mark.parametrize("dt", ["FP32", "FP64"])
def test_signed_zero_and_nan_defaults(gb, dt):
    t = dm.NP[dt]
    rng = rng_of("zeros", dt)
    for shape in [(65,), (37, 53)]:
        n = int(np.prod(shape))
        v = np.where(rng.random(n) < 0.5, t(1.5), t(-2.5)).reshape(shape)  # no zeros among the operands
        A, B = masked((rng.random(shape) < 0.6, v)), masked((rng.random(shape) < 0.6, -v))
        for al, be in [(t(-0.0), t(0.0)), (t(np.nan), t(-0.0)), (t(0.0), t(np.nan)), (t(np.nan), t(np.nan))]:
            for op in ("min", "max", "copysign", "minus", "times"):
                union_check(gb, op, dt, A, al, B, be, what=f"{op}[{dt}] defaults {al!r}, {be!r} {shape}")


@pytest.mark.parametrize("dt", ["INT32", "FP64", "BOOL", "UINT8"])
def test_iso_operands(gb, dt):
    for shape in [(65,), (37, 53), (3, 300)]:
        rng = rng_of("iso", dt, shape)
        pa, pb = rng.random(shape) < 0.6, rng.random(shape) < 0.6
        sa, sb = (True, True) if dt == "BOOL" else (3, 2)
        a_iso, A_iso = iso_gb(gb, pa, sa, dt)
        b_iso, B_iso = iso_gb(gb, pb, sb, dt)
        vb = draw(dt, rng, pb.size).reshape(shape)
        if dt == "FP64":
            vb = np.where(np.isnan(vb) | (vb == 0), 1.0, vb)
        B = masked((pb, vb))
        b = to_gb(gb, B)
        al, be = (True, False) if dt == "BOOL" else (7, 5)
        for op in ("plus", "minus", "max", "eq", "second"):
            for (x, X), (y, Y), tag in (((a_iso, A_iso), (b, B), "iso,full"), ((b, B), (a_iso, A_iso), "full,iso"),
                                        ((a_iso, A_iso), (b_iso, B_iso), "iso,iso")):
                union_check(gb, op, dt, X, al, Y, be, a=x, b=y, zero_sign=op != "max",
                            what=f"{op}[{dt}] {shape} {tag}")


# ---------------------------------------------------------------------- write-back
MASKS = [("none", False), ("S", False), ("V", False), ("~S", False), ("~V", False), ("S", True), ("V", True),
         ("~S", True), ("~V", True)]


@pytest.fixture(scope="module", params=[(37, 53), (200,)], ids=["37x53", "200"])
def wb(request):
    shape = request.param
    rng = rng_of("writeback", shape)
    n = int(np.prod(shape))
    mk = lambda d, dt: masked((rng.random(shape) < d, draw(dt, rng, n).reshape(shape)))  # noqa: E731
    A, B, C = mk(0.5, "INT64"), mk(0.5, "INT64"), mk(0.4, "FP64")
    C = masked((C[0], np.where(np.isfinite(C[1]), C[1], 1.5)))
    M = masked((rng.random(shape) < 0.5, rng.integers(0, 2, shape)))  # stored false values
    assert (M[0] & (M[1] == 0)).any()
    return dict(A=A, B=B, C=C, M=M, T=um.ewise_union("minus", "INT64", A, 10, B, 20))


@pytest.mark.parametrize("kind,replace", MASKS)
@pytest.mark.parametrize("accum", [None, "plus"])
def test_masks_replace_and_accum(gb, wb, kind, replace, accum):
    a, b, c, m = (to_gb(gb, wb[k]) for k in "ABCM")
    kw = {}
    if kind != "none":
        mk = m.S if "S" in kind else m.V
        kw = {"mask": ~mk if kind.startswith("~") else mk, "replace": replace}
    if accum:
        kw["accum"] = getattr(gb.binary, accum)
    c(**kw) << a.ewise_union(b, gb.binary.minus, 10, 20)
    want = dm.write_back(wb["C"], wb["T"], mask=None if kind == "none" else wb["M"], mask_comp=kind.startswith("~"),
                         mask_struct="S" in kind, replace=replace, accum=accum)
    check(c, want, "FP64", what=f"mask {kind} replace={replace} accum={accum}")


def test_output_aliases_an_input_or_the_mask(gb, wb):
    A, B, M, T = wb["A"], wb["B"], wb["M"], wb["T"]
    expr = lambda x, y: x.ewise_union(y, gb.binary.minus, 10, 20)  # noqa: E731
    a, b = to_gb(gb, A), to_gb(gb, B)
    a << expr(a, b)  # C is A
    check(a, T, "INT64", what="C is A")
    a, b = to_gb(gb, A), to_gb(gb, B)
    b << expr(a, b)  # C is B
    check(b, T, "INT64", what="C is B")
    a = to_gb(gb, A)
    a << expr(a, a)  # A and B are one handle, and C too
    check(a, um.ewise_union("minus", "INT64", A, 10, A, 20), "INT64", what="C is A is B")
    assert stats(gb) == (int(A[0].sum()), 0, 0)
    a, b = to_gb(gb, A), to_gb(gb, B)
    m = to_gb(gb, (M[0], M[1].astype(np.int64)))
    m(m.V, replace=True) << expr(a, b)  # C is the mask
    check(m, dm.write_back((M[0], M[1].astype(np.int64)), T, mask=M, replace=True), "INT64", what="C is the mask")
    a, b = to_gb(gb, A), to_gb(gb, B)
    a(a.S, accum=gb.binary.plus) << expr(a, b)  # C is A and the mask
    check(a, dm.write_back(A, T, mask=A, mask_struct=True, accum="plus"), "INT64", what="C is A is the mask")


def test_descriptor_transposes(gb):
    rng = rng_of("desc")
    A = masked((rng.random((37, 53)) < 0.5, rng.integers(-9, 10, (37, 53))))
    B = masked((rng.random((37, 53)) < 0.5, rng.integers(-9, 10, (37, 53))))
    a, b, at, bt = to_gb(gb, A), to_gb(gb, B), to_gb(gb, dm.transpose(A)), to_gb(gb, dm.transpose(B))
    lib = gb.lib
    s10, s20 = gb.Scalar.from_value(10, "INT64"), gb.Scalar.from_value(20, "INT64")
    want = um.ewise_union("minus", "INT64", A, 10, B, 20)
    for x, y, desc, tag in ((at, b, lib.GrB_DESC_T0, "T0"), (a, bt, lib.GrB_DESC_T1, "T1"),
                            (at, bt, lib.GrB_DESC_T0T1, "T0T1")):
        C = gb.Matrix("INT64", 37, 53)
        assert lib.GxB_Matrix_eWiseUnion(C._h, None, None, lib.GrB_MINUS_INT64, x._h, s10._h, y._h, s20._h, desc) == 0
        check(C, want, "INT64", what=tag)
        assert stats(gb) == um.case_counts(A, B)
    # without the descriptor the same operands do not conform
    C = gb.Matrix("INT64", 37, 53)
    assert lib.GxB_Matrix_eWiseUnion(C._h, None, None, lib.GrB_MINUS_INT64, at._h, s10._h, b._h, s20._h, None) \
        == lib.GrB_DIMENSION_MISMATCH
    # and through the front end
    check(at.T.ewise_union(b, gb.binary.minus, 10, 20).new(), want, "INT64", what="A.T, B")
    check(a.ewise_union(bt.T, gb.binary.minus, 10, 20).new(), want, "INT64", what="A, B.T")
    check(at.T.ewise_union(bt.T, gb.binary.minus, 10, 20).new(), want, "INT64", what="A.T, B.T")
    check(a.T.ewise_union(bt, gb.binary.minus, 10, 20).new(), dm.transpose(want), "INT64", what="(A.T, Bt)")


# ---------------------------------------------------------------------- against the composition
def composed(gb, A, B, op, ld, rd, dtype):
    """python-graphblas's five-call fallback (reference core/matrix.py:70-79) on this library"""
    nl = gb.Matrix(dtype, *A.shape)
    nl << B.apply(gb.binary.second, right=ld)
    nl << A.ewise_add(nl, gb.binary.first)
    nr = gb.Matrix(dtype, *A.shape)
    nr << A.apply(gb.binary.second, right=rd)
    nr << B.ewise_add(nr, gb.binary.first)
    return nl.ewise_mult(nr, op).new()


@pytest.mark.parametrize("dt", ["INT64", "FP64"])
def test_equals_the_five_call_composition(gb, dt):
    rng = rng_of("composition", dt)
    t = dm.NP[dt]
    mk = lambda: masked((rng.random((300, 300)) < 0.1, (rng.standard_normal((300, 300)) * 100).astype(t)))  # noqa: E731
    A, B = mk(), mk()
    a, b = to_gb(gb, A), to_gb(gb, B)
    for op, ld, rd in (("minus", t(0), t(0)), ("div", t(1), t(1)), ("minus", t(3), t(-4))):
        got = a.ewise_union(b, getattr(gb.binary, op), ld, rd).new()
        ref = composed(gb, a, b, getattr(gb.binary, op), ld, rd, dt)
        assert got.dtype == ref.dtype == dt and got.nvals == ref.nvals == int((A[0] | B[0]).sum())
        for x, y in zip(got.to_coo(), ref.to_coo()):
            assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), (op, dt)


# ---------------------------------------------------------------------- golden cases
def golden_gb(gb, d):
    if "cols" in d:
        return gb.Matrix.from_coo(d["rows"], d["cols"], np.asarray(d["vals"], dm.NP[d["dtype"]]), nrows=d["nrows"],
                                  ncols=d["ncols"])
    return gb.Vector.from_coo(d["rows"], np.asarray(d["vals"], dm.NP[d["dtype"]]), size=d["size"])


def golden_check(got, case, what):
    e = case["expect"]
    assert got.dtype == e["dtype"], what
    *idx, vals = got.to_coo()
    assert np.array_equal(idx[0], e["rows"]), what
    if "cols" in e:
        assert np.array_equal(idx[1], e["cols"]), what
    if case["close"]:
        assert np.allclose(vals, e["vals"], rtol=1e-7, atol=0), what
    else:
        assert np.array_equal(vals, np.asarray(e["vals"], dm.NP[e["dtype"]])), what


@pytest.mark.parametrize("case", um.golden_cases(), ids=lambda c: c["source"].split(" ")[0])
def test_golden_cases(gb, case):
    lib = gb.lib
    a, b = golden_gb(gb, case["A"]), golden_gb(gb, case["B"])
    x, y = (a.T if case["at"] else a), (b.T if case["bt"] else b)
    ld, rd = case["left_default"]["value"], case["right_default"]["value"]
    opobj = getattr(gb.monoid if case["opclass"] == "monoid" else gb.binary, case["op"])
    expr = x.ewise_union(y, opobj, ld, rd)
    assert expr.op.type == case["dtype"]
    golden_check(expr.new(), case, "front end")
    if "scalars" in case["forms"]:
        golden_check(x.ewise_union(y, opobj, gb.Scalar.from_value(ld), gb.Scalar.from_value(rd)).new(), case, "Scalars")
    if "infix" in case["forms"]:
        golden_check((x - y).new(), case, "A - B")
    if "functional" in case["forms"]:
        golden_check(opobj(x | y, left_default=ld, right_default=rd).new(), case, "functional")
    # ctypes: the typed operator, GrB_Scalars of the defaults' own types, the descriptor's transposes
    e = case["expect"]
    kind = "Matrix" if "cols" in e else "Vector"
    C = gb.Matrix(e["dtype"], e["nrows"], e["ncols"]) if kind == "Matrix" else gb.Vector(e["dtype"], e["size"])
    s1 = gb.Scalar.from_value(ld, case["left_default"]["dtype"])
    s2 = gb.Scalar.from_value(rd, case["right_default"]["dtype"])
    desc = {(False, False): None, (True, False): lib.GrB_DESC_T0, (False, True): lib.GrB_DESC_T1,
            (True, True): lib.GrB_DESC_T0T1}[(case["at"], case["bt"])]
    add = getattr(lib, f"GrB_{case['op'].upper()}_{case['dtype']}")
    rc = getattr(lib, f"GxB_{kind}_eWiseUnion")(C._h, None, None, add, a._h, s1._h, b._h, s2._h, desc)
    assert rc == 0
    golden_check(C, case, "ctypes")


# ---------------------------------------------------------------------- errors
def test_error_codes_leave_the_output_untouched(gb):
    lib = gb.lib
    A = gb.Matrix.from_coo([0, 1, 2], [1, 2, 0], [1, 2, 3], nrows=3, ncols=4)
    B = gb.Matrix.from_coo([0, 2], [1, 3], [5, 6], nrows=3, ncols=4)
    C = gb.Matrix.from_coo([1], [1], [42], nrows=3, ncols=4)
    u, v = gb.Vector.from_coo([0, 2], [1, 2], size=5), gb.Vector.from_coo([1], [7], size=5)
    w = gb.Vector.from_coo([4], [42], size=5)
    s, empty = gb.Scalar.from_value(1, "INT64"), gb.Scalar("INT64")
    junk = ctypes.create_string_buffer(4096)  # no magic number: not an object
    J = ctypes.c_void_p(ctypes.addressof(junk))
    plus = lib.GrB_PLUS_INT64
    before_c, before_w = C.to_coo(), w.to_coo()

    def untouched():
        assert all(np.array_equal(x, y) for x, y in zip(C.to_coo(), before_c))
        assert all(np.array_equal(x, y) for x, y in zip(w.to_coo(), before_w))

    mat = lambda *args: lib.GxB_Matrix_eWiseUnion(*args)  # noqa: E731
    vec = lambda *args: lib.GxB_Vector_eWiseUnion(*args)  # noqa: E731
    ok_m = [C._h, None, None, plus, A._h, s._h, B._h, s._h, None]
    ok_v = [w._h, None, None, plus, u._h, s._h, v._h, s._h, None]
    for k in (0, 3, 4, 5, 6, 7):  # C, add, A, alpha, B, beta
        for fn, ok in ((mat, ok_m), (vec, ok_v)):
            args = list(ok)
            args[k] = None
            assert fn(*args) == lib.GrB_NULL_POINTER, k
            if k != 0:
                args[k] = J
                assert fn(*args) == lib.GrB_UNINITIALIZED_OBJECT, k
            untouched()
    assert mat(J, None, None, plus, A._h, s._h, B._h, s._h, None) == lib.GrB_UNINITIALIZED_OBJECT
    for al, be in ((empty, s), (s, empty), (empty, empty)):
        assert mat(C._h, None, None, plus, A._h, al._h, B._h, be._h, None) == lib.GrB_EMPTY_OBJECT
        assert vec(w._h, None, None, plus, u._h, al._h, v._h, be._h, None) == lib.GrB_EMPTY_OBJECT
        msg = ctypes.c_char_p()
        assert lib.GrB_Matrix_error(ctypes.byref(msg), C._h) == 0 and b"no value" in msg.value
        with pytest.raises(gb.exceptions.EmptyObject):
            C << A.ewise_union(B, gb.binary.plus, al, be)
        with pytest.raises(gb.exceptions.EmptyObject):
            w << u.ewise_union(v, gb.binary.plus, al, be)
        untouched()
    bad = gb.Matrix.from_coo([0], [0], [1], nrows=4, ncols=3)
    assert mat(C._h, None, None, plus, A._h, s._h, bad._h, s._h, None) == lib.GrB_DIMENSION_MISMATCH
    assert mat(C._h, None, None, plus, bad._h, s._h, B._h, s._h, None) == lib.GrB_DIMENSION_MISMATCH
    short = gb.Vector.from_coo([0], [1], size=4)
    assert vec(w._h, None, None, plus, u._h, s._h, short._h, s._h, None) == lib.GrB_DIMENSION_MISMATCH
    assert vec(short._h, None, None, plus, u._h, s._h, v._h, s._h, None) == lib.GrB_DIMENSION_MISMATCH
    assert mat(C._h, None, None, lib.GxB_FIRSTI_INT64, A._h, s._h, B._h, s._h, None) == lib.GrB_NOT_IMPLEMENTED
    assert vec(w._h, None, None, lib.GxB_FIRSTI_INT64, u._h, s._h, v._h, s._h, None) == lib.GrB_NOT_IMPLEMENTED
    msg = ctypes.c_char_p()
    assert lib.GrB_Matrix_error(ctypes.byref(msg), C._h) == 0 and b"positional" in msg.value
    untouched()
    assert mat(*ok_m) == 0 and vec(*ok_v) == 0  # and the same handles do work
    assert C.nvals == 4 and w.nvals == 3


# ---------------------------------------------------------------------- a graph use
def test_graph_difference_is_antisymmetric(gb):
    from graphblas_amd.matrix import Matrix

    scale = 10
    n = 1 << scale
    G = Matrix.__new__(Matrix)
    G.dtype, G.name, G._h, G._nrows, G._ncols = gb.INT64, "G", ctypes.c_void_p(), n, n
    assert gb.lib.GxB_Matrix_rmat(ctypes.byref(G._h), scale, 16, 42, 1, 2, 0, 0) == 0
    D = gb.Matrix("INT64", n, n)
    D << G.ewise_union(G.T, gb.binary.minus, 0, 0)
    r, c, v = (np.asarray(x).astype(np.int64) for x in G.to_coo())
    Gd, Gp = np.zeros((n, n), np.int64), np.zeros((n, n), bool)
    Gd[r, c], Gp[r, c] = v, True
    dr, dc, dv = (np.asarray(x).astype(np.int64) for x in D.to_coo())
    Dd, Dp = np.zeros((n, n), np.int64), np.zeros((n, n), bool)
    Dd[dr, dc], Dp[dr, dc] = dv, True
    assert np.array_equal(Dp, Gp | Gp.T)
    assert np.array_equal(Dd, -Dd.T) and np.array_equal(Dd, Gd - Gd.T)
    both = G.ewise_mult(G.T, gb.binary.pair).new().nvals
    assert D.nvals == G.nvals + G.T.new().nvals - both
    assert stats(gb)[0] == both
