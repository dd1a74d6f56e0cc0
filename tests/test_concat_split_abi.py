"""CPU checks of the concat / split surface: GxB_Matrix_concat / GxB_Matrix_split are exported,
declared in both headers and typed in _lib; the numpy model the GPU tests compare with
(tests/tile_model.py) reproduces the reference's own cases (tests/golden/concat_split_golden.json);
the front end's chunk normalisation reproduces the reference's examples and errors; the layout
formulas of csrc/gb_tile.hip hold on random structures; and the argument errors of
graphblas_amd.ss.concat / Matrix.ss.concat / Vector.ss.concat are raised before any library call
(reference core/ss/matrix.py:65-116, 281-381, core/ss/vector.py:185-267, ss/_core.py:73-107).
No compute calls: objects are stubs without handles."""
import ctypes
import os
import re

import numpy as np
import pytest

import dense_model as dm
import tile_model as tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = {
    "GxB_Matrix_concat": "GrB_Matrix C, const GrB_Matrix *Tiles, const GrB_Index m, const GrB_Index n, "
                         "const GrB_Descriptor desc",
    "GxB_Matrix_split": "GrB_Matrix *Tiles, const GrB_Index m, const GrB_Index n, const GrB_Index *Tile_nrows, "
                        "const GrB_Index *Tile_ncols, const GrB_Matrix A, const GrB_Descriptor desc",
}
G = tm.golden()
EXC = {"TypeError": TypeError, "ValueError": ValueError}


def ident(case):
    return case["source"].split(" ")[0]


# ---------------------------------------------------------------------- the C ABI
def test_entry_points_are_exported_and_declared():
    import graphblas_amd
    from graphblas_amd import _lib

    dll = ctypes.CDLL(graphblas_amd.LIB_PATH)
    for path in ("graphblas_amd.h", "graphblas_amd_cdef.h"):
        text = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", path)).read())
        for name, args in ENTRY_POINTS.items():
            assert f"GrB_Info {name}({args});" in text, (path, name)
    P, I = ctypes.c_void_p, ctypes.c_uint64
    sigs = {"GxB_Matrix_concat": [P, P, I, I, P], "GxB_Matrix_split": [P, I, I, P, P, P, P]}
    for name in ENTRY_POINTS:
        assert hasattr(dll, name), name
        assert _lib._SIGS[name] == sigs[name], name
        assert name in dir(_lib.lib)
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "GxB_Matrix_concat" in text and "GxB_Matrix_split" in text


def test_adapter_exposes_the_symbols():
    cdef = open(os.path.join(ROOT, "include", "graphblas_amd_cdef.h")).read()
    adapter = open(os.path.join(ROOT, "graph-python_amd", "suitesparse_graphblas_amd", "__init__.py")).read()
    assert "graphblas_amd_cdef.h" in adapter  # the adapter's cdef() is that header
    for name in ENTRY_POINTS:
        assert f"GrB_Info {name}(" in cdef


# ---------------------------------------------------------------------- the model
def fixture(name):
    if name == "A.T":
        return dm.transpose(tm.golden_operand(G["A"]))
    return tm.golden_operand(G[name])


@pytest.mark.parametrize("case", G["split"], ids=ident)
def test_model_split_reproduces_the_golden_tiles(case):
    A = fixture(case["of"])
    for chunks in case["chunks"]:
        shape = A[0].shape
        norm = tm.normalize_chunks([chunks, None], (shape[0], 1))[:1] if len(shape) == 1 else \
            tm.normalize_chunks(chunks, shape)
        assert norm == case["normalized"]
        got = tm.split(A, norm)
        want = case["expect"]
        if len(shape) == 1:
            got, want = [got], [want]
        assert len(got) == len(want)
        for grow, wrow in zip(got, want):
            assert len(grow) == len(wrow)
            for g, w in zip(grow, wrow):
                wp, wv = tm.golden_operand(w)
                assert g[0].shape == wp.shape and np.array_equal(g[0], wp)
                assert np.array_equal(np.where(g[0], g[1], 0), wv)
    if "row_boundaries" in case:
        assert tm.bounds(case["normalized"][0]).tolist() == case["row_boundaries"]
        assert tm.bounds(case["normalized"][1]).tolist() == case["col_boundaries"]


@pytest.mark.parametrize("case", G["concat"], ids=ident)
def test_model_concat_reproduces_the_golden_cases(case):
    if case["tiles"] == "split":
        tiles = tm.split(fixture("A"), G["split"][0]["normalized"])
    elif isinstance(case["tiles"][0], list):
        tiles = [[fixture(t) for t in row] for row in case["tiles"]]
    else:
        tiles = [fixture(t) for t in case["tiles"]]
    p, v = tm.concat(tiles, case["dtype"])
    wp, wv = tm.golden_operand(case["expect"])
    assert p.shape == wp.shape and np.array_equal(p, wp)
    assert v.dtype == wv.dtype and np.array_equal(v, wv)


def test_model_hand_worked_cases():
    t, f = True, False
    # the saturating cast on the way into the output's type: NaN -> 0, 1e9 -> 127, -1e9 -> -128
    a = (np.array([t, t, f]), np.array([np.nan, 1e9, 5.0]))
    b = (np.array([t, f, t, t]), np.array([-1e9, 0.0, 2.9, -2.9]))
    p, v = tm.concat([a, b], "INT8")
    assert v.dtype == np.int8 and p.tolist() == [t, t, f, t, f, t, t] and v.tolist() == [0, 127, 0, -128, 0, 2, -2]
    # a vector inside a matrix concat is N x 1; zero-sized tiles vanish
    A = (np.array([[t, f], [f, t]]), np.array([[1, 0], [0, 2]], np.int16))
    u = (np.array([f, t]), np.array([0, 7], np.int32))
    E = (np.zeros((0, 2), bool), np.zeros((0, 2), np.int16))
    e = (np.zeros(0, bool), np.zeros(0, np.int32))
    p, v = tm.concat([[A, u], [E, e]], "INT64")
    assert p.tolist() == [[t, f, f], [f, t, t]] and v.tolist() == [[1, 0, 0], [0, 2, 7]] and v.dtype == np.int64
    # split with empty parts gives tiles without rows or columns, and concat puts them back
    tiles = tm.split((p, v), [[0, 2, 0], [1, 0, 2]])
    assert [[q[0].shape for q in row] for row in tiles] == [[(0, 1), (0, 0), (0, 2)], [(2, 1), (2, 0), (2, 2)],
                                                             [(0, 1), (0, 0), (0, 2)]]
    back = tm.concat(tiles, "INT64")
    assert np.array_equal(back[0], p) and np.array_equal(back[1], v)
    # the iso rule: tiles without entries do not count; equal after the cast is equal
    one = lambda val, dt, n=2: (np.ones(n, bool), np.full(n, val, dm.NP[dt]))  # noqa: E731
    none = (np.zeros(3, bool), np.zeros(3, np.float64))
    assert tm.is_iso([(one(3, "INT8"), True), (none, False), (one(3.7, "FP64"), True)], "INT32")
    assert not tm.is_iso([(one(3, "INT8"), True), (one(3.7, "FP64"), True)], "FP32")
    assert not tm.is_iso([(one(3, "INT8"), True), (one(3, "INT8"), False)], "INT8")
    assert not tm.is_iso([(none, True)], "INT8")


# ---------------------------------------------------------------------- chunk normalisation
def normalizers():
    from graphblas_amd import ss

    return [("model", tm.normalize_chunks), ("front end", ss.normalize_chunks)]


@pytest.mark.parametrize("case", G["chunks"], ids=ident)
def test_chunks_reproduce_the_golden_examples(case):
    for who, fn in normalizers():
        got = fn(tm.golden_chunks(case["chunks"]), tuple(case["shape"]))
        assert [list(x) for x in got] == case["expect"], who
        assert all(type(c) is int for x in got for c in x), who


@pytest.mark.parametrize("case", G["chunk_errors"], ids=ident)
def test_chunks_raise_the_golden_errors(case):
    for who, fn in normalizers():
        with pytest.raises(EXC[case["raises"]], match=case["match"] if who == "front end" else None):
            fn(tm.golden_chunks(case["chunks"]), tuple(case["shape"]))


def test_chunks_further_cases():
    for who, fn in normalizers():
        assert fn([[4, None], 3], (7, 7)) == [[4, 3], [3, 3, 1]], who      # the reference's own split
        assert fn([[4, 3, None], 7], (7, 7)) == [[4, 3, 0], [7]], who      # "the rest" may be nothing
        assert fn([4, None], (7, 1)) == [[4, 3], [1]], who                 # how a vector is split
        assert fn(np.int64(3), (7,)) == [[3, 3, 1]], who
        assert fn([np.array([1, 63, 0, 6])], (70,)) == [[1, 63, 0, 6]], who
        assert fn([[5, 5]], (7,)) == [[5, 5]], who  # sizes that do not add up are the library's to refuse
        with pytest.raises(TypeError):
            fn([[1, None, None]], (7,))  # two Nones
        with pytest.raises(ValueError):
            fn([[3, -1, None]], (7,))  # a negative size
        with pytest.raises(ValueError):
            fn([[5, 5, None]], (7,))  # an overfull list
        with pytest.raises(ValueError):
            fn((3, 3), (7,))  # a wrong-length tuple
        with pytest.raises(ValueError):
            fn((3,), (7, 7))


# ---------------------------------------------------------------------- the kernels' formulas
def csr_of(p):
    r, c = np.nonzero(p)
    return np.concatenate([[0], np.cumsum(np.bincount(r, minlength=p.shape[0]))]).astype(np.int64), c


def random_cut(rng, size, parts):
    cuts = np.sort(rng.integers(0, size + 1, parts - 1))
    return np.diff(np.concatenate([[0], cuts, [size]])).tolist()


def test_concat_position_formulas():
    """csrc/gb_tile.hip: crp[rb_i + l] = ebase_i + sum_j rp_ij[l]; entry p of tile (i, j), local
    row l, lands at start_ij[l] + p with start_ij[l] = crp[rb_i + l] + (row l's entries in the
    tiles left of j) - rp_ij[l] -- on random structures with empty tiles, rows and columns"""
    rng = np.random.default_rng(5)
    for trial in range(40):
        nr, nc = int(rng.integers(1, 12)), int(rng.integers(1, 40))
        p = rng.random((nr, nc)) < rng.random()
        p[rng.integers(0, nr)] = False
        chunks = [random_cut(rng, nr, int(rng.integers(1, 5))), random_cut(rng, nc, int(rng.integers(1, 6)))]
        tiles = tm.split((p, p.astype(np.int8)), chunks)
        rb, cb = tm.bounds(chunks[0]), tm.bounds(chunks[1])
        want_rp, want_ci = csr_of(p)
        crp, out = np.zeros(nr + 1, np.int64), np.full(want_ci.size, -1)
        ebase = 0
        for i, row in enumerate(tiles):
            csrs = [csr_of(q[0]) for q in row]
            for l in range(rb[i + 1] - rb[i]):
                crp[rb[i] + l] = ebase + sum(rp[l] for rp, _ in csrs)
                left = 0
                for j, (rp, ci) in enumerate(csrs):
                    start = crp[rb[i] + l] + left - rp[l]
                    for q in range(rp[l], rp[l + 1]):
                        assert out[start + q] == -1
                        out[start + q] = ci[q] + cb[j]
                    left += rp[l + 1] - rp[l]
            ebase += sum(rp[-1] for rp, _ in csrs)
        crp[nr] = ebase
        assert np.array_equal(crp, want_rp) and np.array_equal(out, want_ci)


def test_split_position_formulas():
    """csrc/gb_tile.hip: the counts of every tile in one layout (tile t at loff[t], nrows_i + 1
    slots, the last zero), one exclusive scan S: rowptr_t[l] = S[loff_t + l] - S[loff_t]; entry p
    of A lands at p + rowptr_t[l] - cut in its tile, cut = where row r's part in [cb_j, cb_j+1)
    starts; the tile-row / tile-column of an entry is the last bound at or below it"""
    rng = np.random.default_rng(6)
    for trial in range(40):
        nr, nc = int(rng.integers(1, 12)), int(rng.integers(1, 40))
        p = rng.random((nr, nc)) < rng.random()
        chunks = [random_cut(rng, nr, int(rng.integers(1, 5))), random_cut(rng, nc, int(rng.integers(1, 6)))]
        rb, cb = tm.bounds(chunks[0]), tm.bounds(chunks[1])
        m, n = len(chunks[0]), len(chunks[1])
        arp, aci = csr_of(p)
        loff = np.concatenate([[0], np.cumsum([chunks[0][t // n] + 1 for t in range(m * n)])])
        cnt, cut = np.zeros(loff[-1], np.int64), np.zeros(loff[-1], np.int64)
        for t in range(m * n):
            i, j = divmod(t, n)
            for l in range(chunks[0][i]):
                r = rb[i] + l
                row = aci[arp[r]:arp[r + 1]]
                a, b = arp[r] + np.searchsorted(row, cb[j]), arp[r] + np.searchsorted(row, cb[j + 1])
                cnt[loff[t] + l], cut[loff[t] + l] = b - a, a
        S = np.concatenate([[0], np.cumsum(cnt)])
        want = tm.split((p, p.astype(np.int8)), chunks)
        outs = [np.full(int(S[loff[t + 1]] - S[loff[t]]), -1) for t in range(m * n)]
        for r in range(nr):
            for q in range(arp[r], arp[r + 1]):
                i = np.searchsorted(rb, r, side="right") - 1
                j = np.searchsorted(cb, aci[q], side="right") - 1
                t, l = i * n + j, r - rb[i]
                dst = q + (S[loff[t] + l] - S[loff[t]]) - cut[loff[t] + l]
                assert outs[t][dst] == -1
                outs[t][dst] = aci[q] - cb[j]
        for t in range(m * n):
            i, j = divmod(t, n)
            wrp, wci = csr_of(want[i][j][0])
            got_rp = S[loff[t]:loff[t + 1]] - S[loff[t]]
            assert np.array_equal(got_rp, wrp) and np.array_equal(outs[t], wci)


def test_bit_range_formula():
    """k_tile_bits: destination word w of a move of bits [s, s + len) to bit d is the 64 source
    bits from q = 64 w - d + s on (two words, a funnel shift), masked to the range"""
    rng = np.random.default_rng(7)
    for trial in range(300):
        nsrc = int(rng.integers(1, 300))
        src = rng.random(nsrc) < 0.5
        s = int(rng.integers(0, nsrc))
        ln = int(rng.integers(1, nsrc - s + 1))
        d = int(rng.integers(0, 200))
        ndst = d + ln + int(rng.integers(0, 70))
        words = np.packbits(np.pad(src, (0, -nsrc % 64)), bitorder="little").view(np.uint64)
        word = lambda k: int(words[k]) if 0 <= k < words.size else 0  # noqa: E731
        dst = np.zeros(ndst, bool)
        for w in range(d >> 6, ((d + ln - 1) >> 6) + 1):
            b0, b1 = max(w * 64, d), min(w * 64 + 64, d + ln)
            mask = ((1 << (b1 - b0)) - 1) << (b0 & 63)
            q = w * 64 - d + s
            sw, sh = q >> 6, q & 63
            v = (word(sw) >> sh) | ((word(sw + 1) << (64 - sh)) & (2 ** 64 - 1) if sh else 0)
            v &= mask
            for b in range(64):
                if (v >> b) & 1:
                    dst[w * 64 + b] = True
        want = np.zeros(ndst, bool)
        want[d:d + ln] = src[s:s + ln]
        assert np.array_equal(dst, want), (nsrc, s, ln, d)


# ---------------------------------------------------------------------- the front end's argument errors
def stub(name):
    """a Matrix (A), its transpose (A.T) or a Vector (v) without a handle"""
    import graphblas_amd as gb

    if name == "v":
        v = gb.Vector.__new__(gb.Vector)
        v.dtype, v.name, v._size, v._h = gb.dtypes.INT64, "v", 7, None
        return v
    A = gb.Matrix.__new__(gb.Matrix)
    A.dtype, A.name, A._nrows, A._ncols, A._h = gb.dtypes.INT64, "A", 7, 7, None
    return A.T if name == "A.T" else A


def stubs(x):
    if isinstance(x, list):
        return [stubs(y) for y in x]
    return stub(x) if isinstance(x, str) else x


@pytest.mark.parametrize("case", G["concat_errors"], ids=ident)
def test_concat_argument_errors(case):
    import graphblas_amd as gb

    assert gb.ss.concat is not None
    with pytest.raises(EXC[case["raises"]], match=case["match"] or None):
        if case.get("method") == "Vector.ss.concat":
            stub("v").ss.concat(stubs(case["tiles"]))
        else:
            gb.ss.concat(stubs(case["tiles"]))


def test_concat_argument_errors_of_the_methods():
    A, v = stub("A"), stub("v")
    with pytest.raises(TypeError, match="tiles must be lists or tuples"):
        A.ss.concat([v, v])  # a Matrix takes a list of lists, also of vectors
    with pytest.raises(TypeError, match="tiles argument must be list or tuple"):
        v.ss.concat(v)
    with pytest.raises(TypeError, match="Bad tile type for concat at position \\[0, 1\\]"):
        A.ss.concat([[A, 3]])
    with pytest.raises(TypeError, match="tiles must be lists or tuples"):
        v.ss.concat([v, A])  # a Matrix is no piece of a Vector
    with pytest.raises(ValueError, match="tiles must not be empty"):
        A.ss.concat([[], []])


def test_concat_tiles_shapes_and_kinds():
    from graphblas_amd import ss

    A, v, At = stub("A"), stub("v"), stub("A.T")
    rows, m, n, is_matrix = ss._concat_tiles([[A, v], (At, v)])
    assert (m, n, is_matrix) == (2, 2, True) and rows[1][0] is At
    rows, m, n, is_matrix = ss._concat_tiles((v, v, v))
    assert (m, n, is_matrix) == (3, 1, False) and rows == [[v], [v], [v]]
    assert ss._tile_shape(v) == (7, 1) and ss._tile_shape(At) == (7, 7)
