"""GPU parity of GxB_Matrix_concat / GxB_Matrix_split (csrc/gb_tile.hip) with the numpy model of
tests/tile_model.py, through the front end and through ctypes.

Every comparison is exact and goes through to_coo(); for vectors the exported bitmap words are
compared too (no bit may be set at or past n).  stat_concat_bitmap / stat_split_bitmap say which
path ran, stat_concat_iso whether the concat came out iso.

Shapes, and the path each one is for
  vectors  pieces 1, 63, 64, 65, 0, 127, 3, 5, 7   bit offsets 0, 1 and 64, pieces that end on a
                           word boundary, one of 65 that starts on one and spills a bit, an empty
                           piece, three pieces inside one word
           70001 by 1000   71 pieces, most at unaligned offsets
           262245 = 131071 + 131174   two long moves, the second from bit offset 63 of its first
                           source word and ending in a partial word
  matrices 70 x 300        rows of 0, 1, 63, 64, 65, 128, 129, 300 entries; tiles without rows,
                           one-column tiles, 1 x 1
           400 x 40        runs of more than 64 empty rows with a row boundary inside; empty tiles
           301 x 6007      a 5200-entry hub row cut by the column boundaries; 40 tile columns
           133125 x 64, 131071 x 64   about 2 x 10^5 entries over rows of 0..3: many chunks per
                           wave, the layout scan on its wave-tile path and (scan_u8 = 1) on hipCUB
"""
import ctypes
import time

import numpy as np
import pytest

import dense_model as dm
import tile_model as tm
from test_ewise_union_gpu import bitmap_words
from test_general_ops_gpu import _knobs, check, draw, heavy, iso_gb, ragged, to_gb

pytestmark = pytest.mark.gpu

DIMENSION_MISMATCH, NULL_POINTER, INVALID_VALUE = -6, -2, -3


@pytest.fixture(scope="module")
def gb():
    import graphblas_amd

    return graphblas_amd


@pytest.fixture(scope="module", autouse=True)
def report_run_time():
    t0 = time.perf_counter()
    yield
    print(f"\ntest_concat_split_gpu.py: {time.perf_counter() - t0:.1f} s")


def rng_of(*key):
    import zlib

    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def is_iso(obj):
    from graphblas_amd.device import matrix_view, vector_view

    return bool((vector_view if obj.ndim == 1 else matrix_view)(obj._h).iso)


def stat(gb, name):
    return gb.get_knob(f"stat_{name}")


def model_words(p):
    return np.packbits(np.pad(p, (0, -p.size % 64)), bitorder="little").view(np.uint64)


def check_vector(gb, w, want, dt, what):
    check(w, want, dt, what=what)
    assert np.array_equal(bitmap_words(gb, w), model_words(want[0])), f"{what}: bitmap words"


def random_vector(n, dt, key, density=0.5):
    rng = rng_of("vector", n, dt, key)
    p = rng.random(n) < density
    return p, np.where(p, draw(dt, rng, n), dm.NP[dt](0))


def random_matrix(shape, dt, key, density=0.2):
    rng = rng_of("matrix", shape, dt, key)
    p = rng.random(shape) < density
    return p, np.where(p, draw(dt, rng, p.size).reshape(shape), dm.NP[dt](0))


def same_coo(x, y):
    """the same entries with the same bits (isequal would call a NaN different from itself)"""
    cx, cy = x.to_coo(), y.to_coo()
    return all(np.array_equal(a, b) for a, b in zip(cx[:-1], cy[:-1])) and cx[-1].tobytes() == cy[-1].tobytes()


def split_check(gb, a, A, chunks, what, compare_extract=False):
    """a.ss.split(chunks) against the model (and against extract), then concat back against A"""
    dt = dm.name_of(A[1].dtype)
    norm = tm.normalize_chunks(chunks, A[0].shape)
    tiles = a.ss.split(chunks, name="T")
    assert stat(gb, "split_bitmap") == 0
    want = tm.split(A, norm)
    rb, cb = tm.bounds(norm[0]), tm.bounds(norm[1])
    assert len(tiles) == len(want)
    for i, (trow, wrow) in enumerate(zip(tiles, want)):
        assert len(trow) == len(wrow)
        for j, (t, w) in enumerate(zip(trow, wrow)):
            assert t.name == f"T_{i}x{j}"
            check(t, w, dt, what=f"{what}: tile {i}x{j}")
            if compare_extract and w[0].size:
                e = a[int(rb[i]):int(rb[i + 1]), int(cb[j]):int(cb[j + 1])].new()
                assert e.dtype == t.dtype and e.shape == t.shape and same_coo(e, t), \
                    f"{what}: tile {i}x{j} against extract"
    back = gb.ss.concat(tiles)
    assert stat(gb, "concat_bitmap") == 0
    check(back, A, dt, what=f"{what}: concat(split)")
    return tiles


# ---------------------------------------------------------------------- the reference's own cases
def golden_gb(gb, name):
    G = tm.golden()
    if name == "A.T":
        return to_gb(gb, tm.golden_operand(G["A"])).T
    return to_gb(gb, tm.golden_operand(G[name]))


def test_golden_split(gb):
    G = tm.golden()
    for case in G["split"]:
        x = golden_gb(gb, case["of"])
        for chunks in case["chunks"]:
            tiles = x.ss.split(tm.golden_chunks(chunks), name=case.get("name"))
            want = case["expect"]
            if x.ndim == 1:
                tiles, want = [tiles], [want]
                if "names" in case:
                    assert [t.name for t in tiles[0]] == case["names"]
            for trow, wrow in zip(tiles, want):
                assert len(trow) == len(wrow)
                for t, w in zip(trow, wrow):
                    check(t, tm.golden_operand(w), w["dtype"], what=case["source"])
    for case in G["split_errors"]:
        with pytest.raises(gb.DimensionMismatch):
            golden_gb(gb, case["of"]).ss.split(case["chunks"])


def test_golden_concat(gb):
    G = tm.golden()
    for case in G["concat"]:
        spec = case["tiles"]
        if spec == "split":
            tiles = golden_gb(gb, "A").ss.split([4, 3])
        elif isinstance(spec[0], list):
            tiles = [[golden_gb(gb, t) for t in row] for row in spec]
        else:
            tiles = [golden_gb(gb, t) for t in spec]
        want = tm.golden_operand(case["expect"])
        if case.get("into"):
            out = (gb.Vector(case["dtype"], want[0].shape[0]) if want[0].ndim == 1 else
                   gb.Matrix(case["dtype"], *want[0].shape))
            out.ss.concat(tiles)
        else:
            out = gb.ss.concat(tiles, dtype=case["dtype"])
        check(out, want, case["dtype"], what=case["source"])
        assert stat(gb, "concat_bitmap") == (1 if want[0].ndim == 1 else 0)


def test_default_dtype_is_the_unification(gb):
    a = to_gb(gb, random_matrix((5, 4), "INT8", "u1"))
    b = to_gb(gb, random_matrix((5, 3), "FP32", "u2"))
    c = to_gb(gb, random_matrix((5, 2), "UINT16", "u3"))
    assert gb.ss.concat([[a, b, c]]).dtype == "FP32"
    assert gb.ss.concat([[a, c]]).dtype == "INT32"
    assert gb.ss.concat([[c, a]], dtype="FP64").dtype == "FP64"


# ---------------------------------------------------------------------- vectors
PIECES = [1, 63, 64, 65, 0, 127, 3, 5, 7]


@pytest.mark.parametrize("dt", ["INT16", "FP64", "BOOL"])
def test_vector_pieces(gb, dt):
    n = sum(PIECES)
    V = random_vector(n, dt, "pieces")
    v = to_gb(gb, V)
    parts = v.ss.split(PIECES, name="w")
    assert stat(gb, "split_bitmap") == 1
    want = tm.split(V, [PIECES])
    assert [p.size for p in parts] == PIECES and [p.name for p in parts] == [f"w_{i}" for i in range(len(PIECES))]
    for i, (p, w) in enumerate(zip(parts, want)):
        check_vector(gb, p, w, dt, f"piece {i} of {PIECES}")
    back = gb.ss.concat(parts)
    assert stat(gb, "concat_bitmap") == 1 and stat(gb, "concat_iso") == 0
    check_vector(gb, back, V, dt, "concat of the pieces")
    # into an existing vector with other contents, and in another order: every offset changes
    order = [5, 2, 8, 0, 3, 7, 1, 4, 6]
    out = to_gb(gb, random_vector(n, dt, "old contents"))
    out.ss.concat([parts[k] for k in order])
    check_vector(gb, out, tm.concat([want[k] for k in order], dt), dt, "concat of the pieces, reordered")
    # full pieces: every bit set, so a stray or a dropped bit shows
    F = (np.ones(n, bool), draw(dt, rng_of("full", dt), n))
    fparts = to_gb(gb, F).ss.split(PIECES)
    for i, (p, w) in enumerate(zip(fparts, tm.split(F, [PIECES]))):
        check_vector(gb, p, w, dt, f"full piece {i}")
    check_vector(gb, gb.ss.concat(fparts), F, dt, "concat of the full pieces")


@pytest.mark.parametrize("n,chunks", [(70001, 1000), (262245, [131071, 131174])])
def test_vector_big(gb, n, chunks):
    dt = "INT32"
    V = random_vector(n, dt, "big")
    v = to_gb(gb, V)
    parts = v.ss.split(chunks)
    norm = tm.normalize_chunks([chunks, None], (n, 1))[:1]
    want = tm.split(V, norm)
    assert len(parts) == len(want) == (71 if n == 70001 else 2)
    for i, (p, w) in enumerate(zip(parts, want)):
        check_vector(gb, p, w, dt, f"{n}: piece {i}")
    check_vector(gb, gb.ss.concat(parts), V, dt, f"{n}: concat")
    # the same vector is its own first tile
    parts[0].ss.concat([parts[0]])
    check_vector(gb, parts[0], want[0], dt, f"{n}: a vector concatenated into itself")


def test_vector_iso_and_types(gb):
    n = 335
    p = rng_of("iso").random(n) < 0.4
    # an iso source: the pieces stay iso
    v, V = iso_gb(gb, p, 7, "INT32")
    assert is_iso(v)
    parts = v.ss.split(PIECES)
    want = tm.split(V, [PIECES])
    for i, (q, w) in enumerate(zip(parts, want)):
        check_vector(gb, q, w, "INT32", f"iso piece {i}")
        assert is_iso(q) or q.nvals == 0
    # iso pieces of equal values: iso, and the counter says so
    back = gb.ss.concat(parts)
    assert stat(gb, "concat_iso") == 1 and is_iso(back)
    check_vector(gb, back, V, "INT32", "concat of iso pieces")
    # equal after the cast to the output's type (7 and 7.5 into INT16), unequal before
    a, A = iso_gb(gb, p[:100], 7, "INT32")
    b, B = iso_gb(gb, p[100:], 7.5, "FP64")
    out = gb.ss.concat([a, b], dtype="INT16")
    assert stat(gb, "concat_iso") == 1 and is_iso(out)
    check_vector(gb, out, tm.concat([A, B], "INT16"), "INT16", "iso pieces equal after the cast")
    out = gb.ss.concat([a, b])
    assert out.dtype == "FP64" and stat(gb, "concat_iso") == 0 and not is_iso(out)
    check_vector(gb, out, tm.concat([A, B], "FP64"), "FP64", "iso pieces of unequal values")
    # an iso piece next to a non-iso one, and an empty iso piece that decides nothing
    c = to_gb(gb, random_vector(65, "INT32", "mixed"))
    C = random_vector(65, "INT32", "mixed")
    e = gb.Vector("INT8", 13)
    E = (np.zeros(13, bool), np.zeros(13, np.int8))
    out = gb.ss.concat([a, e, c])
    assert stat(gb, "concat_iso") == 0
    check_vector(gb, out, tm.concat([A, E, C], "INT32"), "INT32", "iso, empty and non-iso pieces")
    out = gb.ss.concat([e, a, e])
    assert stat(gb, "concat_iso") == 1
    check_vector(gb, out, tm.concat([E, A, E], "INT32"), "INT32", "an iso piece between empty ones")
    # FP64 pieces into an INT8 vector: the saturating cast
    F1, F2 = random_vector(65, "FP64", "f1"), random_vector(127, "FP64", "f2")
    for F, vals in ((F1, [np.nan, 1e9, -1e9, 2.9]), (F2, [-2.9, np.inf, -np.inf, 127.5])):
        idx = np.flatnonzero(F[0])[:4]
        F[1][idx] = vals
    out = gb.Vector("INT8", 192)
    out.ss.concat([to_gb(gb, F1), to_gb(gb, F2)])
    check_vector(gb, out, tm.concat([F1, F2], "INT8"), "INT8", "FP64 pieces into INT8")


# ---------------------------------------------------------------------- matrices
LENS = [0, 1, 63, 64, 65, 128, 129, 300]


def edge_matrix(dt):
    rng = rng_of("edge", dt)
    p = np.zeros((70, 300), bool)
    for r in range(70):
        p[r, rng.permutation(300)[:LENS[r % 8]]] = True
    return p, np.where(p, draw(dt, rng, p.size).reshape(p.shape), dm.NP[dt](0))


@pytest.mark.parametrize("chunks", [([7, 0, 63], [1, 63, 64, 65, 107]), (1, 1), (None, [300, 0]), ([0, 70], None)],
                         ids=["7-0-63 x 1-63-64-65-107", "1 x 1 tiles", "empty last column", "empty first row"])
def test_matrix_edge_rows(gb, chunks):
    if chunks == (1, 1):
        A = random_matrix((9, 11), "INT64", "tiny", 0.5)
    else:
        A = edge_matrix("FP32")
    split_check(gb, to_gb(gb, A), A, list(chunks), f"edge rows {chunks}", compare_extract=True)


def test_matrix_empty_row_runs(gb):
    rng = rng_of("runs")
    p = np.zeros((400, 40), bool)
    for lo, hi in ((0, 10), (100, 121), (300, 400)):
        p[lo:hi] = rng.random((hi - lo, 40)) < 0.3
    A = (p, np.where(p, draw("INT16", rng, p.size).reshape(p.shape), np.int16(0)))
    tiles = split_check(gb, to_gb(gb, A), A, [[50, 100, 150, 100], [13, 27]], "empty row runs", compare_extract=True)
    assert tiles[2][0].nvals == 0 and tiles[2][1].nvals == 0
    empty = (np.zeros((400, 40), bool), np.zeros((400, 40), np.int16))
    split_check(gb, gb.Matrix("INT16", 400, 40), empty, [[50, 350], 7], "an empty matrix")


@pytest.mark.parametrize("chunks", [([7, 1, 293], [1000, 2000, 3007]), (100, 151)], ids=["3 x 3", "4 x 40"])
def test_matrix_hub_row(gb, chunks):
    A = heavy("INT32", "tile")
    assert A[0][7].sum() == 5200
    tiles = split_check(gb, to_gb(gb, A), A, list(chunks), f"hub {chunks}")
    if chunks == (100, 151):
        assert len(tiles) == 4 and len(tiles[0]) == 40


@pytest.mark.parametrize("shape,scan_u8", [((133125, 64), 0), ((133125, 64), 1), ((131071, 64), 0)])
def test_many_short_rows(gb, shape, scan_u8):
    A = ragged(*shape, "INT32", "tile")
    with _knobs(gb, scan_u8=scan_u8):
        tiles = split_check(gb, to_gb(gb, A), A, [-(-shape[0] // 3), [31, 33]], f"{shape} scan_u8={scan_u8}")
    assert len(tiles) == 3 and len(tiles[0]) == 2


def test_matrix_iso_stays_iso(gb):
    p = rng_of("isomat").random((70, 300)) < 0.2
    a, A = iso_gb(gb, p, -3, "INT16")
    tiles = a.ss.split([[7, 0, 63], [1, 63, 64, 65, 107]])
    for row, wrow in zip(tiles, tm.split(A, [[7, 0, 63], [1, 63, 64, 65, 107]])):
        for t, w in zip(row, wrow):
            check(t, w, "INT16", what="iso tile")
            assert is_iso(t) == bool(w[0].any())
    back = gb.ss.concat(tiles)
    assert stat(gb, "concat_iso") == 1 and is_iso(back)
    check(back, A, "INT16", what="concat of iso tiles")


def test_kronecker_power_cut_in_four(gb):
    seed = gb.Matrix.from_coo([0, 0, 1, 2, 2], [0, 1, 1, 0, 2], True, dtype="BOOL", nrows=3, ncols=3)
    K = seed.kronecker(seed, "land").new()
    K = K.kronecker(seed, "land").new()
    K = K.kronecker(seed, "land").new()
    assert is_iso(K) and K.shape == (81, 81)
    r, c, v = K.to_coo()
    P = np.zeros((81, 81), bool)
    P[r.astype(np.int64), c.astype(np.int64)] = True
    tiles = K.ss.split([[40, 41], [27, 54]])
    for row, wrow in zip(tiles, tm.split((P, P.copy()), [[40, 41], [27, 54]])):
        for t, w in zip(row, wrow):
            check(t, w, "BOOL", what="quarter of a Kronecker power")
            assert is_iso(t) == bool(w[0].any())
    back = gb.ss.concat(tiles)
    assert stat(gb, "concat_iso") == 1 and is_iso(back)
    assert back.dtype == K.dtype and same_coo(back, K)


# ---------------------------------------------------------------------- mixed tiles
def test_mixed_tiles(gb):
    A, B = random_matrix((65, 70), "INT32", "mA"), random_matrix((70, 65), "FP64", "mB")
    U, W = random_vector(65, "UINT8", "mu"), random_vector(65, "FP32", "mw")
    a, b, u, w = to_gb(gb, A), to_gb(gb, B), to_gb(gb, U), to_gb(gb, W)
    # [[A, v]] and [[v], [v]] into a Matrix
    check(gb.ss.concat([[a, u]]), tm.concat([[A, U]], "INT32"), "INT32", what="[[A, v]]")
    check(gb.ss.concat([[u], [w]]), tm.concat([[U], [W]], "FP32"), "FP32", what="[[v], [v]]")
    assert stat(gb, "concat_bitmap") == 0
    # a TransposedMatrix tile, tiles of three dtypes into FP32 and into INT8
    for dt in ("FP32", "INT8"):
        got = gb.ss.concat([[a, b.T, u], [a, b.T, w]], dtype=dt)
        check(got, tm.concat([[A, dm.transpose(B), U], [A, dm.transpose(B), W]], dt), dt,
              what=f"three dtypes into {dt}")
    # iso and non-iso tiles together
    i, I = iso_gb(gb, A[0], 5, "INT64")
    got = gb.ss.concat([[i, a], [a, i]])
    assert stat(gb, "concat_iso") == 0 and not is_iso(got)
    check(got, tm.concat([[I, A], [A, I]], "INT64"), "INT64", what="iso and non-iso tiles")
    # a Matrix from vectors only, and an N x 1 Matrix into a Vector: the views between the formats
    m1 = gb.ss.concat([[u]])
    out = gb.Vector("INT32", 130)
    tiles = (ctypes.c_void_p * 2)(m1._h.value, w._h.value)
    assert gb.lib.GxB_Matrix_concat(out._h, tiles, 2, 1, None) == 0
    assert stat(gb, "concat_bitmap") == 1
    check_vector(gb, out, tm.concat([U, W], "INT32"), "INT32", "an N x 1 Matrix piece of a Vector")
    # C is one of its own tiles
    big = gb.Matrix("INT32", 130, 70)
    big.ss.concat([[a], [a]])
    check(big, tm.concat([[A], [A]], "INT32"), "INT32", what="[[A], [A]] into a Matrix")
    a2 = gb.Matrix("INT32", 65, 70)
    a2.ss.concat([[a]])
    a2.ss.concat([[a2]])
    check(a2, A, "INT32", what="a Matrix concatenated into itself")


def test_block_matrix_from_quadrants(gb):
    A = random_matrix((33, 33), "INT32", "quad")
    a = to_gb(gb, A)
    Z = (np.zeros((33, 33), bool), np.zeros((33, 33), np.int32))
    eye = (np.eye(33, dtype=bool), np.eye(33, dtype=np.int32))
    got = gb.ss.concat([[a, gb.Matrix("INT32", 33, 33)], [to_gb(gb, eye), a.T]])
    check(got, tm.concat([[A, Z], [eye, dm.transpose(A)]], "INT32"), "INT32", what="[[A, 0], [I, A.T]]")


def test_results_repeat_bit_for_bit(gb):
    A = heavy("FP64", "repeat")
    a = to_gb(gb, A)
    first = [[t.to_coo() for t in row] for row in a.ss.split((100, 151))]
    tiles = a.ss.split((100, 151))
    again = [[t.to_coo() for t in row] for row in tiles]
    for r1, r2 in zip(first, again):
        for t1, t2 in zip(r1, r2):
            assert all(np.array_equal(x, y) for x, y in zip(t1[:2], t2[:2]))
            assert t1[2].tobytes() == t2[2].tobytes()
    c1, c2 = gb.ss.concat(tiles).to_coo(), gb.ss.concat(tiles).to_coo()
    assert all(np.array_equal(x, y) for x, y in zip(c1[:2], c2[:2])) and c1[2].tobytes() == c2[2].tobytes()


# ---------------------------------------------------------------------- errors
def test_errors(gb):
    A = random_matrix((9, 11), "INT64", "err", 0.5)
    a = to_gb(gb, A)
    b = to_gb(gb, random_matrix((8, 11), "INT64", "err2", 0.5))
    # ragged tile rows, tile columns, and sums that are not C's shape
    with pytest.raises(gb.DimensionMismatch):
        gb.ss.concat([[a, b]])
    with pytest.raises(gb.DimensionMismatch):
        gb.ss.concat([[a, a], [b, a]])
    C = to_gb(gb, A)
    with pytest.raises(gb.DimensionMismatch):
        C.ss.concat([[a, a]])
    check(C, A, "INT64", what="C after a failed concat")
    v = to_gb(gb, random_vector(9, "INT64", "errv"))
    w = to_gb(gb, random_vector(9, "INT64", "errw"))
    with pytest.raises(gb.DimensionMismatch):
        w.ss.concat([v, v])
    check(w, random_vector(9, "INT64", "errw"), "INT64", what="w after a failed concat")
    # chunks that do not sum to the shape
    for chunks in ([[5, 5], 3], [[4, 4], None], [None, [5, 5]], [[9, 1], None]):
        with pytest.raises(gb.DimensionMismatch):
            a.ss.split(chunks)
    with pytest.raises(gb.DimensionMismatch):
        v.ss.split([5, 5])
    # after a failed split no tile exists; NULL pointers and zero counts
    lib = gb.lib
    tiles = (ctypes.c_void_p * 4)(*[0xdead] * 4)
    nr, nc = (ctypes.c_uint64 * 2)(5, 5), (ctypes.c_uint64 * 2)(5, 6)
    assert lib.GxB_Matrix_split(tiles, 2, 2, nr, nc, a._h, None) == DIMENSION_MISMATCH
    assert [t for t in tiles] == [None] * 4
    nr[1] = 4
    assert lib.GxB_Matrix_split(None, 2, 2, nr, nc, a._h, None) == NULL_POINTER
    assert lib.GxB_Matrix_split(tiles, 2, 2, None, nc, a._h, None) == NULL_POINTER
    assert lib.GxB_Matrix_split(tiles, 0, 2, nr, nc, a._h, None) == INVALID_VALUE
    assert lib.GxB_Matrix_split(tiles, 2, 0, nr, nc, a._h, None) == INVALID_VALUE
    assert lib.GxB_Matrix_split(tiles, 2, 2, nr, nc, None, None) == NULL_POINTER
    # a vector is split along its one dimension only
    one, two = (ctypes.c_uint64 * 1)(9), (ctypes.c_uint64 * 2)(1, 0)
    assert lib.GxB_Matrix_split(tiles, 1, 2, one, two, v._h, None) == DIMENSION_MISMATCH
    assert lib.GxB_Matrix_split(tiles, 2, 2, nr, nc, a._h, None) == 0
    got = [ctypes.c_void_p(t) for t in tiles]
    assert all(t.value for t in got)
    assert lib.GxB_Matrix_concat(C._h, None, 2, 2, None) == NULL_POINTER
    assert lib.GxB_Matrix_concat(C._h, tiles, 0, 2, None) == INVALID_VALUE
    assert lib.GxB_Matrix_concat(C._h, tiles, 2, 0, None) == INVALID_VALUE
    assert lib.GxB_Matrix_concat(None, tiles, 2, 2, None) == NULL_POINTER
    holed = (ctypes.c_void_p * 4)(tiles[0], None, tiles[2], tiles[3])
    assert lib.GxB_Matrix_concat(C._h, holed, 2, 2, None) == NULL_POINTER
    check(C, A, "INT64", what="C after refused concats")
    assert lib.GxB_Matrix_concat(C._h, tiles, 2, 2, None) == 0
    check(C, A, "INT64", what="C from the ctypes tiles")
    for t in got:
        assert lib.GrB_Matrix_free(ctypes.byref(t)) == 0
