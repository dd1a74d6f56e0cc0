"""Hand-worked checks of tests/dense_model.py, the numpy reference the GPU tests of the general
operations (test_general_ops_gpu.py) compare with.  Not marked gpu: a wrong model must not be able
to agree quietly with a wrong kernel.

The golden file records no eWise, apply, reduce or transpose case of the reference; its accum and
mask cases (C = A.dup(); C(mask, accum) << A.mxm(A) and the vxm ones) do exercise the write-back
rule, with T the recorded unmasked product, so the model's write_back runs on those.

The indexing functions (extract, assign, set_element, remove_element, resize) are pinned by
hand-worked cases, by the expectations test_extract.py and test_scalar_args.py state, and by
the reference's own extract / assign / resize / delete cases of golden/indexing_golden.json;
the last test builds the expectation of every case of test_indexing_gpu.py.
"""
import math
import zlib

import numpy as np

import dense_model as dm


def _b(name, dtype, x, y):
    return dm.binop(name, dtype, np.array([x], dm.NP[dtype]), np.array([y], dm.NP[dtype]))[0]


def _u(name, dtype, x):
    return dm.unop(name, dtype, np.array([x], dm.NP[dtype]))[0]


def _c(x, src, dst):
    return dm.cast(np.array([x], dm.NP[src]), dst)[0]


def test_dense_model_rules():
    # integer division
    assert _b("div", "INT8", -128, -1) == -128
    assert _b("div", "INT8", 5, 0) == 127
    assert _b("div", "INT8", -5, 0) == -128
    assert _b("div", "UINT8", 0, 0) == 0
    assert _b("div", "UINT8", 7, 0) == 255
    assert _b("div", "INT8", 0, 0) == 0
    assert _b("div", "INT32", -7, 2) == -3 and _b("div", "INT32", 7, -2) == -3  # toward zero
    assert _b("div", "INT32", -7, -2) == 3 and _b("div", "INT32", -6, 2) == -3
    assert _b("div", "INT64", -2**63, -1) == -2**63 and _b("div", "INT64", 5, -1) == -5
    assert _b("rdiv", "INT8", 0, 5) == 127 and _b("rdiv", "INT16", 4, -9) == -2
    assert _u("minv", "INT8", 0) == 127 and _u("minv", "INT8", -1) == -1 and _u("minv", "INT8", 2) == 0
    assert _u("minv", "UINT16", 0) == 65535 and _u("minv", "UINT16", 1) == 1
    # integer pow: the saturating cast of a float64 pow
    assert _b("pow", "INT8", 3, 5) == 127 and _b("times", "INT8", _b("times", "INT8", 81, 3), 1) == -13
    assert _b("pow", "INT64", -2, 63) == -2**63
    assert _b("pow", "INT64", 2, 63) == 2**63 - 1
    assert _b("pow", "INT32", 0, -1) == 2**31 - 1
    assert _b("pow", "INT32", 2, -1) == 0
    assert _b("pow", "UINT8", 2, 7) == 128 and _b("pow", "UINT8", 2, 8) == 255
    assert _b("pow", "INT16", -3, 3) == -27 and _b("pow", "INT16", -9, 5) == -32768
    # wrapping arithmetic
    assert _b("plus", "INT8", 127, 1) == -128 and _b("minus", "UINT8", 0, 1) == 255
    assert _b("rminus", "INT8", 1, -128) == 127 and _b("times", "UINT16", 256, 256) == 0
    assert _b("times", "INT64", 2**62, 2) == -2**63
    assert _u("ainv", "INT8", -128) == -128 and _u("abs", "INT8", -128) == -128 and _u("ainv", "UINT8", 1) == 255
    # casts
    assert _c(-1.5, "FP64", "UINT8") == 0
    assert _c(300.7, "FP64", "INT8") == 127
    assert _c(math.nan, "FP64", "INT32") == 0
    assert _c(-5, "INT32", "INT64") == -5
    assert _c(-5, "INT32", "UINT64") == 2**64 - 5
    assert _c(-300.7, "FP32", "INT8") == -128 and _c(-1.9, "FP64", "INT8") == -1 and _c(2.9, "FP32", "UINT8") == 2
    assert _c(math.inf, "FP64", "INT64") == 2**63 - 1 and _c(-math.inf, "FP64", "INT64") == -2**63
    assert _c(2.0**63, "FP64", "INT64") == 2**63 - 1 and _c(2.0**64, "FP64", "UINT64") == 2**64 - 1
    assert _c(300, "INT32", "UINT8") == 44 and _c(200, "UINT8", "INT8") == -56
    assert _c(2**53 + 1, "INT64", "FP64") == 2.0**53
    assert _c(0.25, "FP64", "BOOL") and _c(math.nan, "FP64", "BOOL") and not _c(-0.0, "FP64", "BOOL")
    assert _c(True, "BOOL", "INT8") == 1 and _c(True, "BOOL", "FP32") == 1.0
    # round is half away from zero
    assert _u("round", "FP64", 2.5) == 3.0
    r = _u("round", "FP64", -0.5)
    assert r == -1.0
    assert _u("round", "FP32", 0.5) == 1.0 and _u("round", "FP64", 1.5) == 2.0 and _u("round", "FP64", -2.5) == -3.0
    assert _u("round", "FP64", 0.49999999999999994) == 0.0
    z = _u("round", "FP64", -0.25)
    assert z == 0.0 and np.signbit(z)
    assert np.isnan(_u("round", "FP64", math.nan)) and _u("round", "FP64", -math.inf) == -math.inf
    # ainv of a float is -x: the sign of zero flips
    assert np.signbit(_u("ainv", "FP64", 0.0)) and not np.signbit(_u("ainv", "FP32", -0.0))
    # float min / max omit NaN
    assert _b("min", "FP64", math.nan, 2.0) == 2.0 and _b("max", "FP32", 1.0, math.nan) == 1.0
    assert np.isnan(_b("min", "FP64", math.nan, math.nan))
    # IEEE remainder and C fmod
    assert _b("remainder", "FP64", 5.0, 3.0) == -1.0 and _b("fmod", "FP64", 5.0, 3.0) == 2.0
    assert _b("remainder", "FP64", 7.0, 2.0) == -1.0 and _b("fmod", "FP64", -7.0, 2.0) == -1.0  # ties to even
    assert np.isnan(_b("remainder", "FP64", 1.0, 0.0)) and np.isnan(_b("fmod", "FP32", math.inf, 2.0))
    assert _b("ldexp", "FP32", 3.0, -2.0) == 0.75 and _b("copysign", "FP64", 2.0, -0.0) == -2.0
    # bool renames
    T, F = True, False
    for x in (F, T):
        for y in (F, T):
            assert _b("plus", "BOOL", x, y) == _b("max", "BOOL", x, y) == (x or y)
            assert _b("times", "BOOL", x, y) == _b("min", "BOOL", x, y) == (x and y)
            assert _b("minus", "BOOL", x, y) == _b("ne", "BOOL", x, y) == _b("rminus", "BOOL", x, y) == (x != y)
            assert _b("div", "BOOL", x, y) == x and _b("rdiv", "BOOL", x, y) == y
            assert _b("pow", "BOOL", x, y) == (x or not y)
            assert _b("eq", "BOOL", x, y) == _b("iseq", "BOOL", x, y) == _b("lxnor", "BOOL", x, y) == (x == y)
            assert _b("gt", "BOOL", x, y) == _b("isgt", "BOOL", x, y) == (x and not y)
            assert _b("le", "BOOL", x, y) == (not x or y) and _b("pair", "BOOL", x, y)
        assert _u("minv", "BOOL", x) and _u("lnot", "BOOL", x) == (not x) and _u("ainv", "BOOL", x) == x
    # logical and is* operators on other types return 1/0 of that type; comparisons return bool
    assert _b("lor", "INT8", 0, -3) == 1 and _b("lor", "INT8", 0, -3).dtype == np.int8
    assert _b("land", "FP32", 0.5, math.nan) == 1.0 and _b("lxor", "UINT8", 2, 3) == 0
    assert _b("lxnor", "FP64", 0.0, -0.0) == 1.0 and _u("lnot", "FP64", -0.0) == 1.0 and _u("lnot", "INT16", 7) == 0
    assert _b("isgt", "INT8", 3, 2) == 1 and _b("isgt", "INT8", 3, 2).dtype == np.int8
    assert _b("isne", "FP64", math.nan, math.nan) == 1.0 and _b("iseq", "FP32", 1.0, 1.0).dtype == np.float32
    assert _b("gt", "UINT64", 2**64 - 1, 2**63) and _b("gt", "UINT64", 1, 0).dtype == np.bool_
    assert not _b("eq", "FP64", math.nan, math.nan) and _b("ne", "FP64", math.nan, math.nan)
    # bitwise
    assert _b("bxnor", "UINT8", 0b1100, 0b1010) == 0b11111001 and _b("bxnor", "INT8", 5, 5) == -1
    assert _u("bnot", "UINT16", 1) == 65534 and _u("bnot", "INT8", 0) == -1
    assert _b("any", "INT8", 3, 4) == 4 and _b("first", "INT8", 3, 4) == 3 and _b("pair", "FP32", 3, 4) == 1.0


def test_monoid_folds_match_their_definition():
    rng = np.random.default_rng(5)
    for name, dtypes in [("plus", ["INT8", "UINT64"]), ("times", ["INT8", "UINT16"]), ("min", ["INT16", "FP32"]),
                         ("max", ["UINT8", "FP64"]), ("lor", ["BOOL"]), ("land", ["BOOL"]), ("lxor", ["BOOL"]),
                         ("lxnor", ["BOOL"]), ("bor", ["UINT8"]), ("band", ["UINT32"]), ("bxor", ["UINT64"]),
                         ("bxnor", ["UINT8", "UINT64"])]:
        for dt in dtypes:
            for n in (1, 2, 3, 8, 9):
                if dt == "BOOL":
                    for bias in (0.1, 0.5, 0.9, 1.0):
                        v = rng.random(n) < bias
                        assert dm.monoid_fold(name, dt, v) == dm.monoid_fold_sequential(name, dt, v), (name, n)
                    continue
                v = rng.integers(0, 200, n).astype(dm.NP[dt])
                if dm.is_float(dt):
                    v[0] = np.nan
                a, b = dm.monoid_fold(name, dt, v), dm.monoid_fold_sequential(name, dt, v)
                assert np.array_equal(a, b, equal_nan=dm.is_float(dt)) and np.asarray(a).dtype == dm.NP[dt], (name, dt, n)
    assert dm.monoid_identity("min", "INT8") == 127 and dm.monoid_identity("max", "UINT8") == 0
    assert dm.monoid_identity("min", "FP32") == np.inf and dm.monoid_identity("band", "UINT16") == 65535
    assert dm.monoid_identity("times", "FP64") == 1.0 and dm.monoid_identity("lxnor", "BOOL")
    # the identity does not change a fold
    for name, dt in [("plus", "INT8"), ("times", "UINT8"), ("min", "INT32"), ("max", "FP64"), ("lor", "BOOL"),
                     ("land", "BOOL"), ("lxor", "BOOL"), ("lxnor", "BOOL"), ("bor", "UINT8"), ("band", "UINT8"),
                     ("bxor", "UINT8"), ("bxnor", "UINT8")]:
        for x in ([0, 1, 5, 77] if dt != "BOOL" else [False, True]):
            x = np.array([x], dm.NP[dt])
            assert dm.binop(name, dt, x, np.array([dm.monoid_identity(name, dt)]))[0] == x[0], (name, dt)


def test_ewise_apply_reduce_transpose_small():
    A = dm.to_dense((2, 3), ([0, 0, 1], [0, 2, 1]), np.array([1, -2, 3], np.int8))
    B = dm.to_dense((2, 3), ([0, 1, 1], [2, 1, 2]), np.array([2.5, 300.0, -1.0]))
    p, v = dm.ewise("mult", "plus", "FP64", A, B)
    assert dm.to_coo((p, v))[0].tolist() == [0, 1] and v[p].tolist() == [0.5, 303.0]
    p, v = dm.ewise("add", "gt", "FP64", A, B)  # one-sided entries: the value cast to bool
    assert v.dtype == np.bool_ and p.sum() == 4
    assert v[0, 0] and not v[0, 2] and not v[1, 1] and v[1, 2]
    p, v = dm.ewise("add", "plus", "INT8", A, B)  # operands cast first: 300.0 -> 127, 3 + 127 wraps
    assert v.dtype == np.int8 and v[1, 1] == -126 and v[0, 2] == 0 and v[1, 2] == -1 and v[0, 0] == 1
    p, v = dm.apply("minus", "INT8", A, right=np.int64(130))  # the scalar is cast to the operator's type
    assert v[0, 0] == 127 and v[0, 2] == 124
    p, v = dm.apply("minus", "INT8", A, left=np.int8(1))
    assert v[0, 2] == 3 and v[1, 1] == -2 and not p[1, 0]
    assert dm.reduce_scalar("plus", "INT8", A) == 2 and dm.reduce_scalar("plus", "INT8", (A[0] & False, A[1])) is None
    p, v = dm.reduce_rows("min", "INT8", A)
    assert p.tolist() == [True, True] and v.tolist() == [-2, 3]
    p, v = dm.reduce_cols("max", "FP64", B)
    assert p.tolist() == [False, True, True] and v[1:].tolist() == [300.0, 2.5]
    tp, tv = dm.transpose(A)
    assert tp.shape == (3, 2) and tv[2, 0] == -2 and tp[1, 1] and not tp[0, 1]


def test_build_folds_in_input_order():
    idx = np.array([2, 0, 2, 2, 0, 1])
    vals = np.array([10, 1, 3, 4, 7, 9])
    for op, want in [("plus", [8, 9, 17]), ("minus", [-6, 9, 3]), ("first", [1, 9, 10]), ("second", [7, 9, 4]),
                     ("min", [1, 9, 3]), ("rminus", [6, 9, 11])]:
        p, v = dm.build((4,), (idx,), vals, op, "INT64")
        assert p.tolist() == [True, True, True, False] and v[:3].tolist() == want, op
    # the cast runs before the fold: 200 + 100 as INT8 is -56 + 100
    p, v = dm.build((1, 2), ([0, 0], [1, 1]), np.array([200, 100]), "plus", "INT8")
    assert v[0, 1] == 44 and p.sum() == 1
    p, v = dm.build((2,), ([1, 1, 1],), np.array([0.5, 2.0, 0.0]), "plus", "BOOL")  # lor of the casts
    assert v[1] and v.dtype == np.bool_


def test_write_back_rules():
    big = 2**53 + 1
    C = dm.to_dense((5,), ([0, 1, 2, 3],), np.array([big, -(2**62) - 3, 7, 8], np.int64))
    T = dm.to_dense((5,), ([1, 2, 4],), np.array([0.5, 1.75, 300.25]))
    # plus evaluated in FP64: untouched entries keep their bits, both -> cast(float(c) + t)
    p, v = dm.write_back(C, T, accum="plus", accum_dtype="FP64")
    assert p.all() and v.tolist() == [big, -(2**62), 8, 8, 300]
    # in INT64 (the default for an untyped accumulator): t is cast first
    p, v = dm.write_back(C, T, accum="plus")
    assert v.tolist() == [big, -(2**62) - 3, 8, 8, 300]
    M = dm.to_dense((5,), ([0, 2, 4],), np.array([False, True, True]))
    p, v = dm.write_back(C, T, mask=M, mask_struct=True, accum="plus", accum_dtype="FP64")
    assert p.all() and v.tolist() == [big, -(2**62) - 3, 8, 8, 300]
    p, v = dm.write_back(C, T, mask=M, accum="plus", accum_dtype="FP64")  # value mask: index 0 is outside
    assert v.tolist() == [big, -(2**62) - 3, 8, 8, 300]
    p, v = dm.write_back(C, T, mask=M, mask_struct=True, mask_comp=True, replace=True)  # no accum: Z = T
    assert p.tolist() == [False, True, False, False, False] and v[1] == 0
    p, v = dm.write_back(C, T, mask=M, mask_struct=True, mask_comp=True, replace=True, accum="plus",
                         accum_dtype="FP64")
    assert p.tolist() == [False, True, False, True, False] and v[1] == -(2**62) and v[3] == 8
    # no mask, no accum: C = T cast to C's type, old entries gone
    p, v = dm.write_back(C, T)
    assert p.tolist() == [False, True, True, False, True] and v[[1, 2, 4]].tolist() == [0, 1, 300]
    # C UINT8 with max evaluated in INT64: the result wraps into UINT8; a T-only entry saturates
    C8 = dm.to_dense((3,), ([0, 1],), np.array([200, 5], np.uint8))
    T8 = dm.to_dense((3,), ([0, 1, 2],), np.array([300.0, -4.0, 1e9]))
    p, v = dm.write_back(C8, T8, accum="max", accum_dtype="INT64")
    assert v.tolist() == [44, 5, 255]


def _gold(case, shape):
    if "indices" in case:
        return dm.to_dense(shape, (case["indices"],), np.array(case["values"]))
    return dm.to_dense(shape, (case["rows"], case["cols"]), np.array(case["values"]))


def _same(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1][got[0]], want[1][want[0]])


def test_write_back_on_the_reference_golden_cases(golden):
    c = golden["cases"]
    A = _gold(golden["A"], (7, 7))
    v = _gold(golden["v"], (7,))
    T = _gold(c["test_mxm"]["expected"], (7, 7))
    assert _same(dm.write_back(A, T, accum="plus"), _gold(c["test_mxm_accum"]["expected"], (7, 7)))
    mm = c["test_mxm_mask"]
    vm, sm = _gold(mm["val_mask"], (7, 7)), _gold(mm["struct_mask"], (7, 7))
    assert _same(dm.write_back(A, T, mask=vm), _gold(mm["expected_value"], (7, 7)))
    assert _same(dm.write_back(A, T, mask=vm, mask_comp=True), _gold(mm["expected_comp"], (7, 7)))
    assert _same(dm.write_back(A, T, mask=sm, mask_struct=True, replace=True),
                 _gold(mm["expected_struct_replace"], (7, 7)))
    t = _gold(c["test_vxm"]["expected"], (7,))
    assert _same(dm.write_back(v, t, accum="plus"), _gold(c["test_vxm_accum"]["expected"], (7,)))
    vmk = c["test_vxm_mask"]
    vm, sm = _gold(vmk["val_mask"], (7,)), _gold(vmk["struct_mask"], (7,))
    assert _same(dm.write_back(v, t, mask=sm, mask_struct=True), _gold(vmk["expected_struct"], (7,)))
    assert _same(dm.write_back(v, t, mask=sm, mask_struct=True, mask_comp=True), _gold(vmk["expected_comp"], (7,)))
    assert _same(dm.write_back(v, t, mask=vm, replace=True), _gold(vmk["expected_value_replace"], (7,)))


def test_ulp_distance():
    a = np.array([1.0, -1.0, 0.0, np.inf, np.nan], np.float32)
    assert dm.ulp_distance(a, a) == 0
    b = a.copy()
    b[0] = np.nextafter(np.float32(1.0), np.float32(2.0))
    b[1] = np.nextafter(np.nextafter(np.float32(-1.0), np.float32(-2.0)), np.float32(-2.0))
    assert dm.ulp_distance(b, a) == 2
    assert dm.ulp_distance(np.array([-0.0]), np.array([5e-324])) == 1
    assert dm.ulp_distance(np.array([np.nan, 1.0]), np.array([1.0, 1.0])) == math.inf
    assert dm.ulp_distance(np.array([np.inf]), np.array([-np.inf])) == math.inf


# ---------------------------------------------------------------------- mxm, mxv, vxm
def _coo_equal(got, want):
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(got[1][got[0]], want[1][want[0]], equal_nan=got[1].dtype.kind == "f")


def test_mxm_on_the_reference_golden_cases(golden):
    c = golden["cases"]
    A, v = _gold(golden["A"], (7, 7)), _gold(golden["v"], (7,))
    pt = ("plus", "times", "INT64")
    _coo_equal(dm.mxm(*pt, A, A), _gold(c["test_mxm"]["expected"], (7, 7)))
    _coo_equal(dm.mxm(*pt, A, A, tran1=True), _gold(c["test_mxm_transpose_AAT"]["expected"], (7, 7)))
    _coo_equal(dm.mxm(*pt, A, A, tran0=True), _gold(c["test_mxm_transpose_ATA"]["expected"], (7, 7)))
    _coo_equal(dm.mxv(*pt, A, v), _gold(c["test_mxv"]["expected"], (7,)))
    _coo_equal(dm.vxm(*pt, v, A), _gold(c["test_vxm"]["expected"], (7,)))
    _coo_equal(dm.vxm(*pt, v, A, tran1=True), _gold(c["test_vxm_transpose"]["expected"], (7,)))
    ns = c["test_mxm_nonsquare"]
    p, x = dm.mxm("max", "plus", "INT64", _gold(ns["A"], (1, 5)), _gold(ns["B"], (5, 1)))
    assert p.tolist() == [[True]] and x[0, 0] == ns["expected_scalar"]
    vn = c["test_vxm_nonsquare"]
    _coo_equal(dm.vxm("min", "plus", "INT64", v, _gold(vn["A"], (7, 2))), _gold(vn["expected"], (2,)))
    # inner: u' u as 1 x n times n x 1
    p, x = dm.mxm(*pt, (v[0][None, :], v[1][None, :]), (v[0][:, None], v[1][:, None]))
    assert p[0, 0] and x[0, 0] == c["test_inner"]["expected_scalar"]
    d = c["docs_mxv_plus_times"]
    Ad = _gold(d["A"], (d["A"].get("nrows", max(d["A"]["rows"]) + 1), d["A"].get("ncols", max(d["A"]["cols"]) + 1)))
    vd = _gold(d["v"], (Ad[0].shape[1],))
    want = _gold(d["expected"], (Ad[0].shape[0],))
    _coo_equal(dm.mxv("plus", "times", "FP64", (Ad[0], Ad[1].astype(float)), (vd[0], vd[1].astype(float))),
               (want[0], want[1].astype(float)))


def _dense_of(M):
    r, c, x = M.to_coo()
    return dm.to_dense((M.nrows, M.ncols), (r, c), x)


def _dense_vec(u):
    return dm.to_dense((u.size,), (u.indices,), u.values)


def test_mxm_matches_the_oracle_on_the_parity_semirings():
    import oracle as O
    from test_gpu_parity import SEMIRINGS, _rand_csr

    n, k, m = 37, 53, 41
    for name, mon, mul, dt in SEMIRINGS:
        rng = np.random.default_rng(zlib.crc32(repr((name, dt, "model")).encode()))
        sr = (mon, mul, dt)
        model = (mon.lower(), mul.lower(), dt)
        shapes = {(False, False): ((n, k), (k, m)), (True, False): ((k, n), (k, m)),
                  (False, True): ((n, k), (m, k)), (True, True): ((k, n), (m, k))}
        for (t0, t1), (sa, sb) in shapes.items():
            Ao, Bo = _rand_csr(rng, *sa, 0.15, dt), _rand_csr(rng, *sb, 0.15, dt)
            ref = _dense_of(O.mxm(O.Csr.empty(n, m, dt), Ao, Bo, sr, tran0=t0, tran1=t1))
            got = dm.mxm(*model, _dense_of(Ao), _dense_of(Bo), tran0=t0, tran1=t1)
            assert got[1].dtype == dm.NP[dt]
            if mon == "ANY":
                assert np.array_equal(got[0], ref[0])
            else:
                _coo_equal(got, ref)
        for t in (False, True):
            Ao = _rand_csr(rng, n, k, 0.15, dt)
            uk, un = O.Vec.from_col(_rand_csr(rng, k, 1, 0.4, dt)), O.Vec.from_col(_rand_csr(rng, n, 1, 0.4, dt))
            u_mxv, u_vxm = (un, uk) if t else (uk, un)
            ref_mxv = O.mxv(O.Vec(k if t else n, dt, [], []), Ao, u_mxv, sr, tran0=t)
            ref_vxm = O.vxm(O.Vec(n if t else k, dt, [], []), u_vxm, Ao, sr, tran1=t)
            got_mxv = dm.mxv(*model, _dense_of(Ao), _dense_vec(u_mxv), tran0=t)
            got_vxm = dm.vxm(*model, _dense_vec(u_vxm), _dense_of(Ao), tran1=t)
            for got, ref in ((got_mxv, ref_mxv), (got_vxm, ref_vxm)):
                if mon == "ANY":
                    assert np.array_equal(got[0], _dense_vec(ref)[0])
                else:
                    _coo_equal(got, _dense_vec(ref))


def test_positional_multipliers_by_hand():
    """A is 2 x 3 with A(0,1), A(0,2), A(1,0); B is 3 x 4 with B(0,2), B(1,3), B(2,0), B(2,3):
    T(0,0) takes k = 2, T(0,3) takes k = 1, 2, T(1,2) takes k = 0"""
    A = dm.to_dense((2, 3), ([0, 0, 1], [1, 2, 0]), np.array([9, 9, 9]))
    B = dm.to_dense((3, 4), ([0, 1, 2, 2], [2, 3, 0, 3]), np.array([7, 7, 7, 7]))
    want = {"firsti": (0, 0, 1), "firsti1": (1, 2, 2), "firstj": (2, 3, 0), "firstj1": (3, 5, 1),
            "secondi": (2, 3, 0), "secondi1": (3, 5, 1), "secondj": (0, 6, 2), "secondj1": (1, 8, 3)}
    full3, full2 = (np.ones(3, bool), np.array([4, 4, 4])), (np.ones(2, bool), np.array([4, 4]))
    # mxv: w0 folds k = 1, 2 and w1 k = 0, with j = 0; vxm: w0 takes k = 1, w1 and w2 take k = 0, with i = 0
    want_mxv = {"firsti": (0, 1), "firsti1": (2, 2), "firstj": (3, 0), "firstj1": (5, 1), "secondi": (3, 0),
                "secondi1": (5, 1), "secondj": (0, 0), "secondj1": (2, 1)}
    want_vxm = {"firsti": (0, 0, 0), "firsti1": (1, 1, 1), "firstj": (1, 0, 0), "firstj1": (2, 1, 1),
                "secondi": (1, 0, 0), "secondi1": (2, 1, 1), "secondj": (0, 1, 2), "secondj1": (1, 2, 3)}
    for op in dm.POSITIONAL:
        for dt in ("INT32", "INT64"):
            for kw, X, Y in (({}, A, B), (dict(tran0=True), dm.transpose(A), B), (dict(tran1=True), A, dm.transpose(B)),
                             (dict(tran0=True, tran1=True), dm.transpose(A), dm.transpose(B))):
                p, x = dm.mxm("plus", op, dt, X, Y, **kw)
                assert x.dtype == dm.NP[dt] and p.sum() == 3
                assert (x[0, 0], x[0, 3], x[1, 2]) == want[op], (op, kw)
            p, x = dm.mxv("plus", op, dt, A, full3)
            assert p.all() and tuple(x) == want_mxv[op], op
            p, x = dm.mxv("plus", op, dt, dm.transpose(A), full3, tran0=True)
            assert tuple(x) == want_mxv[op], op
            p, x = dm.vxm("plus", op, dt, full2, A)
            assert p.all() and tuple(x) == want_vxm[op], op
            p, x = dm.vxm("plus", op, dt, full2, dm.transpose(A), tran1=True)
            assert tuple(x) == want_vxm[op], op
    # the lists come in ascending k
    P = dm.mxm_products("secondi", "INT64", A, B)
    assert P.lists()[(0, 3)].tolist() == [1, 2] and P.k.tolist() == [2, 1, 2, 0]
    assert P.member(np.array([0, 0, 1]), np.array([3, 0, 2]), np.array([2, 3, 0])).tolist() == [True, False, True]


def test_ordered_multipliers_by_hand():
    """A = [[5 . 7] [. 2 .]], u = [1 10 100], v = [3 4], B = [[1 .] [. 10] [100 1000]]: an operand
    swap anywhere in the model changes every one of these"""
    A = dm.to_dense((2, 3), ([0, 0, 1], [0, 2, 1]), np.array([5, 7, 2]))
    B = dm.to_dense((3, 2), ([0, 1, 2, 2], [0, 1, 0, 1]), np.array([1, 10, 100, 1000]))
    u = np.ones(3, bool), np.array([1, 10, 100])
    v = np.ones(2, bool), np.array([3, 4])
    At, Bt = dm.transpose(A), dm.transpose(B)
    want = {  # mxv A u, vxm v A, mxv A' v, mxm A B at (0,0), (0,1), (1,1)
        "minus": ([-89, -8], [-2, 2, -4], [2, -2, 4], [-89, -993, -8]),
        "rminus": ([89, 8], [2, -2, 4], [-2, 2, -4], [89, 993, 8]),
        "div": ([5, 0], [0, 2, 0], [1, 0, 2], [5, 0, 0]),
        "rdiv": ([14, 5], [1, 0, 2], [0, 2, 0], [14, 142, 5]),
    }
    for op, (w_mxv, w_vxm, w_mxvT, w_mxm) in want.items():
        s = ("plus", op, "INT64")
        assert dm.mxv(*s, A, u)[1].tolist() == w_mxv, op
        assert dm.mxv(*s, At, u, tran0=True)[1].tolist() == w_mxv, op
        assert dm.vxm(*s, v, A)[1].tolist() == w_vxm, op
        assert dm.vxm(*s, v, At, tran1=True)[1].tolist() == w_vxm, op
        assert dm.mxv(*s, At, v)[1].tolist() == w_mxvT, op
        assert dm.mxv(*s, A, v, tran0=True)[1].tolist() == w_mxvT, op
        for kw, X, Y in (({}, A, B), (dict(tran0=True), At, B), (dict(tran1=True), A, Bt)):
            p, x = dm.mxm(*s, X, Y, **kw)
            assert p.tolist() == [[True, True], [False, True]] and [x[0, 0], x[0, 1], x[1, 1]] == w_mxm, (op, kw)
    g = ("lor", "gt", "INT64")
    assert dm.mxv(*g, A, u)[1].tolist() == [True, False] and dm.mxv(*g, A, u)[1].dtype == np.bool_
    assert dm.vxm(*g, v, A)[1].tolist() == [False, True, False]
    assert dm.mxv(*g, A, v, tran0=True)[1].tolist() == [True, False, True]
    assert dm.mxm(*g, A, Bt, tran1=True)[1].tolist() == [[True, False], [False, False]]
    # operands are cast to the multiplier's type first: 300.7 -> INT8 127, 1.5 -> 1
    Af = dm.to_dense((1, 2), ([0, 0], [0, 1]), np.array([300.7, 1.5]))
    p, x = dm.mxv("plus", "times", "INT8", Af, (np.ones(2, bool), np.array([2, 3], np.int64)))
    assert x.dtype == np.int8 and x.tolist() == [1]  # 127 * 2 + 1 * 3 = 257 wraps to 1


def test_fold_of_all_lists_matches_the_sequential_fold():
    rng = np.random.default_rng(11)
    A = rng.random((9, 7)) < 0.6, rng.integers(0, 250, (9, 7)).astype(np.uint8)
    B = rng.random((7, 8)) < 0.6, rng.integers(0, 250, (7, 8)).astype(np.uint8)
    for mon in ("plus", "times", "min", "max", "bor", "band", "bxor", "bxnor", "lxor"):
        (p, x), P = dm.mxm(mon, "plus", "UINT8", A, B, products=True)
        for (i, j), z in P.lists().items():
            assert p[i, j] and x[i, j] == dm.monoid_fold_sequential(mon, "UINT8", z), (mon, i, j)
        assert p.sum() == len(P.lists())


_CASES = {}


def _sweep_case(mon, mul, dt, zt):
    import semiring_cases as sc

    key = (mon, mul, dt)
    if key not in _CASES:
        _CASES[key] = sc.Case(mon, mul, dt, zt)
    return _CASES[key]


def test_sweep_inputs_are_order_free_and_reach_terminals_and_identities():
    """Every case of the GPU sweep, model only: Case() raises if the fold of any expected entry
    depends on the order (ascending, descending, shuffled); every terminal value and identity
    the multiplier can produce is the first product of an entry with more products after it."""
    import semiring_cases as sc

    tab = sc.table()
    assert len(tab) == 210 and sum(len(v) for v in tab.values()) == 1499
    planted = {}
    for (mon, mul), entries in tab.items():
        for pyname, dt, zt, names in entries:
            case = sc.Case(mon, mul, dt, zt)
            case.check_planted()
            planted[(mon, mul, dt)] = len(case.planted)
    # the plain arithmetic multipliers reach both values, the bounded ones what their range holds
    assert planted[("min", "plus", "INT8")] == 2 and planted[("times", "minus", "UINT64")] == 2
    assert planted[("bor", "band", "UINT64")] == 2 and planted[("land", "lxor", "BOOL")] == 2
    assert planted[("max", "isgt", "INT8")] == 0 and planted[("times", "pair", "INT8")] == 1


def test_zero_sign_rules_of_the_float_products():
    pz, nz = 0.0, -0.0
    A = dm.to_dense((1, 3), ([0, 0, 0], [0, 1, 2]), np.array([pz, 1.0, np.nan]))
    u = np.ones(3, bool), np.array([nz, 2.0, np.nan])
    (p, x), P = dm.mxv("plus", "max", "FP64", A, u, products=True)
    assert P.clash.tolist() == [True, False, False] and dm.zero_sign_free("plus", P).tolist() == [True]
    # membership for ANY: the clash zero in either sign, any NaN, but 2.0 only as itself
    for v, ok in ((pz, True), (nz, True), (2.0, True), (-2.0, False), (-np.nan, True)):
        assert P.member(np.array([0]), np.array([0]), np.array([v])).tolist() == [ok], v
    (p, x), P = dm.mxv("min", "first", "FP64", A, u, products=True)
    assert not P.clash.any() and dm.zero_sign_free("min", P).tolist() == [False]
    B = dm.to_dense((1, 2), ([0, 0], [0, 1]), np.array([pz, nz]))
    (p, x), P = dm.mxv("max", "first", "FP64", B, (np.ones(2, bool), np.ones(2)), products=True)
    assert dm.zero_sign_free("max", P).tolist() == [True] and dm.zero_sign_free("plus", P).tolist() == [False]
    assert not dm.order_dependent("max", P).any() and not dm.order_dependent("plus", P).any()


# ---------------------------------------------------------------------- indexing operations
def _vec(d, n, dtype=np.int64):
    return dm.to_dense((n,), (list(d),), np.array(list(d.values()), dtype))


def _vdict(w):
    i, x = dm.to_coo(w)
    return dict(zip(i.tolist(), x.tolist()))


def _mdict(C):
    r, c, x = dm.to_coo(C)
    return {(a, b): y for a, b, y in zip(r.tolist(), c.tolist(), x.tolist())}


def test_extract_set_remove_resize_by_hand():
    """A = [[1 . 3] [. 5 .]]: T(r, c) = A(I[r], J[c]) with repeats and any order"""
    A = dm.to_dense((2, 3), ([0, 0, 1], [0, 2, 1]), np.array([1, 3, 5], np.int16))
    T = dm.extract(A, [1, 0, 1], [2, 2, 0, 1])
    assert T[1].dtype == np.int16 and T[0].shape == (3, 4)
    assert _mdict(T) == {(0, 3): 5, (1, 0): 3, (1, 1): 3, (1, 2): 1, (2, 3): 5}
    assert _mdict(dm.extract(A)) == _mdict(A) and dm.extract(A, [], None)[0].shape == (0, 3)
    assert _mdict(dm.extract(A, None, [1])) == {(1, 0): 5}
    u = _vec({1: 10, 2: 20}, 4)
    assert _vdict(dm.extract_vec(u, [2, 2, 0, 1])) == {0: 20, 1: 20, 3: 10}
    assert _vdict(dm.extract_vec(u)) == {1: 10, 2: 20}
    # setElement casts to the object's type; removeElement of an absent entry changes nothing
    B = dm.set_element(A, (1, 2), 300.7)
    assert B[1].dtype == np.int16 and _mdict(B) == {(0, 0): 1, (0, 2): 3, (1, 1): 5, (1, 2): 300}
    assert _mdict(A) == {(0, 0): 1, (0, 2): 3, (1, 1): 5}  # the input is not edited
    assert _mdict(dm.set_element(A, (0, 0), -7)) == {(0, 0): -7, (0, 2): 3, (1, 1): 5}
    assert _mdict(dm.remove_element(A, (0, 2))) == {(0, 0): 1, (1, 1): 5}
    assert _mdict(dm.remove_element(A, (1, 0))) == _mdict(A)
    assert _vdict(dm.set_element(_vec({}, 3, np.uint8), 2, -1)) == {2: 255}
    # resize: shrinking drops, growing adds nothing, and what was dropped does not come back
    assert _mdict(dm.resize(A, (1, 3))) == {(0, 0): 1, (0, 2): 3}
    assert _mdict(dm.resize(A, (2, 2))) == {(0, 0): 1, (1, 1): 5}
    assert _mdict(dm.resize(A, (5, 7))) == _mdict(A) and dm.resize(A, (5, 7))[0].shape == (5, 7)
    assert dm.resize(A, (0, 0))[0].shape == (0, 0) and dm.resize(A, (0, 3))[0].shape == (0, 3)
    assert _mdict(dm.resize(dm.resize(A, (2, 2)), (2, 3))) == {(0, 0): 1, (1, 1): 5}
    assert _vdict(dm.resize(dm.resize(u, 2), 4)) == {1: 10}


def test_assign_by_hand():
    """GrB_assign, not subassign: the mask has C's size and replace reaches outside the region"""
    C = _vec({0: 100, 1: 101, 2: 102, 4: 104}, 6)
    u = _vec({0: -1, 2: -3}, 3)
    I = [4, 1, 3]  # w(4) = u(0), w(1) = u(1), w(3) = u(2)
    assert _vdict(dm.assign_vec(C, u, I)) == {0: 100, 2: 102, 3: -3, 4: -1}  # 1 is deleted
    assert _vdict(dm.assign_vec(C, u, I, accum="plus")) == {0: 100, 1: 101, 2: 102, 3: -3, 4: 103}
    M = dm.to_dense((6,), ([0, 1, 3],), np.array([True, False, True]))
    assert _vdict(dm.assign_vec(C, u, I, mask=M, mask_struct=True)) == {0: 100, 2: 102, 3: -3, 4: 104}
    assert _vdict(dm.assign_vec(C, u, I, mask=M)) == {0: 100, 1: 101, 2: 102, 3: -3, 4: 104}
    # replace deletes outside the mask, outside the region too (index 2 and 4)
    assert _vdict(dm.assign_vec(C, u, I, mask=M, mask_struct=True, replace=True)) == {0: 100, 3: -3}
    assert _vdict(dm.assign_vec(C, u, I, mask=M, mask_comp=True, replace=True)) == {2: 102, 4: -1}
    # scalars: repeats in the list are fine; an empty scalar deletes (nothing under accum)
    assert _vdict(dm.assign_vec(C, np.int64(7), [1, 1, 5])) == {0: 100, 1: 7, 2: 102, 4: 104, 5: 7}
    assert _vdict(dm.assign_vec(C, np.int64(7), [1, 1, 5], accum="plus")) == {0: 100, 1: 108, 2: 102, 4: 104, 5: 7}
    assert _vdict(dm.assign_vec(C, None, [1, 1, 5])) == {0: 100, 2: 102, 4: 104}
    assert _vdict(dm.assign_vec(C, None, [1, 1, 5], accum="plus")) == _vdict(C)
    assert _vdict(dm.assign_vec(C, np.float64(np.nan), None, mask=M)) == {0: 0, 1: 101, 2: 102, 3: 0, 4: 104}
    assert _vdict(dm.assign_vec(_vec({1: 5}, 3, np.int8), np.float64(1e30), None)) == {0: 127, 1: 127, 2: 127}
    # the accumulator runs in its own type: 2^53 + 1 survives INT64 plus, not FP64 plus
    big = _vec({0: 2**53}, 1)
    assert _vdict(dm.assign_vec(big, np.int64(1), None, accum="plus")) == {0: 2**53 + 1}
    assert _vdict(dm.assign_vec(big, np.int64(1), None, accum="plus", accum_dtype="FP64")) == {0: 2**53}
    # matrices: the region is I x J
    A = dm.to_dense((3, 3), ([0, 1, 1, 2], [0, 0, 1, 2]), np.array([1, 2, 3, 4]))
    S = dm.to_dense((2, 2), ([0], [1]), np.array([9]))
    assert _mdict(dm.assign(A, S, [1, 2], [0, 2])) == {(0, 0): 1, (1, 1): 3, (1, 2): 9}
    assert _mdict(dm.assign(A, S, [1, 2], [0, 2], accum="second")) == {(0, 0): 1, (1, 0): 2, (1, 1): 3, (1, 2): 9,
                                                                       (2, 2): 4}
    assert _mdict(dm.assign(A, np.int64(0), None, [1])) == {(0, 0): 1, (0, 1): 0, (1, 0): 2, (1, 1): 0, (2, 1): 0,
                                                           (2, 2): 4}
    assert _mdict(dm.assign(A, np.int64(5), [], None)) == _mdict(A)


def test_assign_restates_the_device_tests():
    """the expectations test_extract.py::test_vector_index_assign_replaces_region and
    test_scalar_args.py state as dictionaries, from the model"""
    n = 12
    w = _vec({k: k + 100 for k in range(n)}, n)
    u = _vec({0: -1, 2: -3}, 4)
    I = [1, 3, 5, 7]
    exp = {k: k + 100 for k in range(n) if k not in (3, 7)}
    exp.update({1: -1, 5: -3})
    assert _vdict(dm.assign_vec(w, u, I)) == exp  # the region delete
    m = dm.to_dense((n,), ([3, 5],), np.array([True, True]))
    exp = {k: k + 100 for k in range(n) if k != 3}
    exp[5] = -3
    assert _vdict(dm.assign_vec(w, u, I, mask=m, mask_struct=True)) == exp
    exp = {k: k + 100 for k in range(n)}
    exp[1] += -1
    exp[5] += -3
    assert _vdict(dm.assign_vec(w, u, I, accum="plus")) == exp
    keep = [k for k in range(n) if k != 5]
    w4 = _vec({k: k + 100 for k in keep}, n)
    exp = {k: k + 100 for k in keep if k not in (3, 7)}
    exp[1] = -1
    assert _vdict(dm.assign_vec(w4, u, I, mask=w4, mask_struct=True)) == exp  # the mask aliases the output
    vals = np.arange(n) + 100
    vals[1] = 0
    w5 = np.ones(n, bool), vals
    exp = {k: int(vals[k]) for k in range(n) if k not in (3, 7)}
    exp[5] = -3
    assert _vdict(dm.assign_vec(w5, u, I, mask=w5)) == exp  # value mask: 1 holds 0 and keeps it
    # test_scalar_args.py::test_vector_assign_scalar
    base = {k: 100 + k for k in range(0, 10, 2)}
    w, I = _vec(base, 10), [0, 1, 2, 3, 4, 5]
    m = dm.to_dense((10,), ([1, 2, 3, 8],), np.ones(4, bool))
    S = dict(mask=m, mask_struct=True)
    exp = dict(base)
    exp.update({1: -5, 2: -5, 3: -5})
    assert _vdict(dm.assign_vec(w, np.int32(-5), I, **S)) == exp
    assert _vdict(dm.assign_vec(w, None, I, **S)) == {k: x for k, x in base.items() if k != 2}
    assert _vdict(dm.assign_vec(w, None, I)) == {k: x for k, x in base.items() if k > 5}
    assert _vdict(dm.assign_vec(w, None, I, accum="plus")) == base
    assert _vdict(dm.assign_vec(w, None, None, mask_comp=True, replace=True, **S)) == {}
    exp = {k: -5 for k in range(10) if k not in (1, 2, 3, 8)}
    exp[2], exp[8] = base[2], base[8]
    assert _vdict(dm.assign_vec(w, np.int32(-5), None, mask_comp=True, **S)) == exp
    # test_scalar_args.py::test_matrix_assign_scalar
    rng = np.random.default_rng(5)
    have, vals = rng.random((7, 9)) < 0.5, rng.integers(1, 50, (7, 9))
    mhave = rng.random((7, 9)) < 0.5
    C, M = (have, np.where(have, vals, 0)), (mhave, mhave.copy())
    Il, Jl = [1, 3, 4, 6], [0, 2, 5, 7, 8]
    region = np.zeros((7, 9), bool)
    region[np.ix_(Il, Jl)] = True
    sel = region & mhave
    S = dict(mask=M, mask_struct=True)
    p, v = dm.assign(C, np.int64(77), Il, Jl, **S)
    assert np.array_equal(p, have | sel) and np.array_equal(v[p], np.where(sel, 77, vals)[p])
    assert np.array_equal(dm.assign(C, None, Il, Jl, **S)[0], have & ~sel)
    assert np.array_equal(dm.assign(C, None, Il, Jl, mask_comp=True, replace=True, **S)[0],
                          have & ~(region & ~mhave) & ~mhave)
    assert np.array_equal(dm.assign(C, None, Il, Jl, accum="plus")[0], have)
    assert not dm.assign(C, None, None, None)[0].any()


def test_indexing_golden_cases():
    """the reference's own extract / assign / resize / delete expectations (indexing_golden.json)"""
    import json
    import os

    with open(os.path.join(os.path.dirname(__file__), "golden", "indexing_golden.json")) as f:
        g = json.load(f)
    V = lambda d: dm.to_dense((d["size"],), (d["indices"],), np.array(d["values"], np.int64))
    Mx = lambda d: dm.to_dense((d["nrows"], d["ncols"]), (d["rows"], d["cols"]), np.array(d["values"], np.int64))
    same = lambda a, b: a[0].shape == b[0].shape and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    v, A, c = V(g["v"]), Mx(g["A"]), g["cases"]
    w = v
    for step in c["vector_resize"]["steps"]:
        w = dm.resize(w, step["size"])
        assert w[0].sum() == step["nvals"] and not w[0][step.get("absent", 0)]
    assert same(w, V(c["vector_resize"]["expected_last"]))
    assert same(dm.remove_element(v, c["vector_remove_element"]["remove"]), V(c["vector_remove_element"]["expected"]))
    assert same(dm.extract_vec(v, c["vector_extract"]["I"]), V(c["vector_extract"]["expected"]))
    k = c["vector_assign"]
    assert same(dm.assign_vec(v, V(k["u"]), k["I"]), V(k["expected"]))
    k = c["vector_assign_scalar"]
    assert same(dm.assign_vec(v, np.int64(k["x"]), k["I"]), V(k["expected"]))
    k = c["vector_assign_scalar_mask"]
    for kind, want in k["expected"].items():
        got = dm.assign_vec(v, np.int64(k["x"]), None, mask=V(k["mask"]), mask_struct="S" in kind,
                            mask_comp=kind.startswith("~"))
        assert same(got, V(want)), kind
    k = c["vector_delete_via_scalar"]
    w = dm.assign_vec(v, None, k["I"])
    assert same(w, V(k["expected"])) and dm.assign_vec(w, None, None)[0].sum() == k["then_all_nvals"]
    C = A
    for step in c["matrix_resize"]["steps"]:
        C = dm.resize(C, step["shape"])
        assert C[0].sum() == step["nvals"] and ("absent" not in step or not C[0][tuple(step["absent"])])
    assert same(C, Mx(c["matrix_resize"]["expected_last"]))
    k = c["matrix_remove_element"]
    C = dm.remove_element(A, tuple(k["remove"]))
    assert not C[0][tuple(k["absent"])] and C[1][tuple(k["kept"]["index"])] == k["kept"]["value"]
    assert C[0].sum() == k["nvals"]
    k = c["matrix_extract"]
    assert same(dm.extract(A, k["I"], k["J"]), Mx(k["expected"]))
    k = c["matrix_extract_row"]
    row = dm.extract(A, [k["i"]], k["J"])
    assert same((row[0][0], row[1][0]), V(k["expected"]))
    At = dm.transpose(A)  # the same through A.T[J, i]
    col = dm.extract(At, k["J"], [k["i"]])
    assert same((col[0][:, 0], col[1][:, 0]), V(k["expected"]))
    k = c["matrix_extract_column"]
    col = dm.extract(A, k["I"], [k["j"]])
    assert same((col[0][:, 0], col[1][:, 0]), V(k["expected"]))
    k = c["matrix_assign_scalar"]
    assert same(dm.assign(A, np.int64(k["x"]), k["I"], k["J"]), Mx(k["expected"]))
    C = A
    for step in c["matrix_delete_via_scalar"]["steps"]:
        C = dm.assign(C, None, step["I"], step["J"])
        assert C[0].sum() == step["nvals"]


def test_indexing_case_tables_build_every_expectation():
    """Every case of test_indexing_gpu.py, model only: the tables hold what the issue lists
    (assert_coverage) and each expectation builds, has the output's shape and type, and differs
    from the untouched output where the case is meant to change something."""
    import indexing_cases as ic

    ic.assert_coverage()
    total = changed = 0
    for op in ic.OPS:
        for c in ic.cases(op):
            B = ic.build(c)
            total += 1
            before = getattr(B, "C", None) if hasattr(B, "C") else getattr(B, "w", None)
            if before is not None:
                assert B.want[0].shape == before[0].shape and B.want[1].dtype == before[1].dtype, c.id
                changed += not (np.array_equal(B.want[0], before[0]) and
                                np.array_equal(B.want[1], before[1], equal_nan=B.want[1].dtype.kind == "f"))
            assert not B.want[1][~B.want[0]].any(), c.id  # absent cells carry no value
    assert total == ic.CASE_COUNT, total
    assert changed > total // 2
