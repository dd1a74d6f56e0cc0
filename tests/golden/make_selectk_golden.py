"""Writes selectk_golden.json: the cases of the reference's own selectk / compactify tests.

Usage: python tests/golden/make_selectk_golden.py <python-graphblas checkout>

The reference's tests are read as text (never imported or run): the integer list literals of
graphblas/tests/test_matrix.py test_ss_firstk, test_ss_lastk, test_ss_compactify, test_ss_random
and graphblas/tests/test_vector.py test_ss_firstk, test_ss_lastk, test_ss_largestk,
test_ss_smallestk, test_ss_compactify are taken in source order, and the calls those tests make
with them are spelled out below.  What the tests derive from a literal (``expected[:, :n]``, the
``reverse`` helper that flips every row of a compacted result) is derived here the same way.

Left out, each for the reason given:
  * the retry loops around "random" (they wait for a chance result; the counts test_ss_random
    asserts are kept as ``count_range``);
  * ``selectk("last", 0)`` of test_vector.py test_ss_lastk: the reference slices ``[-0:]``, which
    is everything, where the library keeps min(k, d) = 0 entries.
Where the reference accepts either of two tied results (test_ss_largestk, test_ss_smallestk), both
are recorded under ``accept``.
"""
import ast
import json
import os
import sys


def literals(path, name):
    """(the integer list literals of function ``name`` in source order, "file:first-last")"""
    with open(path) as f:
        tree = ast.parse(f.read())
    fn = next(n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef) and n.name == name)
    found = []
    for n in ast.walk(fn):
        if isinstance(n, ast.List) and n.elts and all(
                isinstance(e, ast.Constant) and type(e.value) is int for e in n.elts):
            found.append((n.lineno, n.col_offset, [e.value for e in n.elts]))
    found.sort()
    rel = "tests/" + os.path.basename(path)
    return [x[2] for x in found], f"{rel}:{fn.lineno}-{fn.end_lineno}"


def compacted(rows, vals):
    """rows of a compacted result -> {row: [values at columns 0 ..]} (rows are sorted)"""
    out = {}
    for r, x in zip(rows, vals):
        out.setdefault(r, []).append(x)
    return out


def flat(byrow):
    rows, cols, vals = [], [], []
    for r in sorted(byrow):
        for c, x in enumerate(byrow[r]):
            rows.append(r)
            cols.append(c)
            vals.append(x)
    return rows, cols, vals


def trim(byrow, n):
    return byrow if n is None else {r: x[:n] for r, x in byrow.items()}


def flip(byrow):
    return {r: x[::-1] for r, x in byrow.items()}


def matrix_cases(ref):
    path = os.path.join(ref, "graphblas", "tests", "test_matrix.py")
    cases = []
    for how in ("first", "last"):
        lits, src = literals(path, f"test_ss_{how}k")
        calls = [(1, "rowwise"), (2, "rowwise"), (1, "columnwise"), (2, "columnwise")]
        assert len(lits) == 3 * len(calls)
        for i, (k, order) in enumerate(calls):
            r, c, x = lits[3 * i:3 * i + 3]
            cases.append(dict(source=src, input="A", op="selectk", how=how, k=k, order=order,
                              accept=[dict(rows=r, cols=c, vals=x)]))
        for order in ("rowwise", "columnwise"):
            cases.append(dict(source=src, input="A", op="selectk", how=how, k=3, order=order, accept=["input"]))
    lits, src = literals(path, "test_ss_compactify")
    rows, new_cols, orig_cols, v_first, v_small, i_small = lits[:6]
    assert len(lits) == 12 and new_cols == flat(compacted(rows, rows))[1]
    for iso in (False, True):
        one = [1] * len(rows)
        bases = [("first", "last", one if iso else v_first, False, 0),
                 ("first", "last", orig_cols, True, 0),
                 ("smallest", "largest", one if iso else v_small, False, 0)]
        if not iso:
            bases.append(("smallest", "largest", i_small, True, 2))
        for how_a, how_b, vals, asindex, stop in bases:
            E = compacted(rows, vals)
            for how, full in ((how_a, E), (how_b, flip(E))):
                for n in [None] + list(reversed(range(stop, 4))):
                    for reverse in (False, True):
                        want = trim(full, n)
                        r, c, x = flat(flip(want) if reverse else want)
                        cases.append(dict(source=src, input="A_iso" if iso else "A", op="compactify", how=how, k=n,
                                          order="rowwise", reverse=reverse, asindex=asindex,
                                          accept=[dict(rows=r, cols=c, vals=x)]))
        r0, c0, x0, r1, c1, x1 = lits[6:12]
        cases.append(dict(source=src, input="A_iso" if iso else "A", op="compactify", how="first", k=1,
                          order="columnwise", reverse=False, asindex=False,
                          accept=[dict(rows=r0, cols=c0, vals=[1] * 7 if iso else x0)]))
        cases.append(dict(source=src, input="A_iso" if iso else "A", op="compactify", how="last", k=1,
                          order="columnwise", reverse=False, asindex=True, accept=[dict(rows=r1, cols=c1, vals=x1)]))
    _, src = literals(path, "test_ss_random")
    for inp in ("A", "A_iso"):
        cases.append(dict(source=src, input=inp, op="selectk", how="random", k=1, order="rowwise", count_range=[1, 1]))
    cases.append(dict(source=src, input="A", op="selectk", how="random", k=1, order="columnwise", count_range=[1, 1]))
    cases.append(dict(source=src, input="A", op="selectk", how="random", k=2, order="rowwise", count_range=[1, 2]))
    return cases


def vector_cases(ref):
    path = os.path.join(ref, "graphblas", "tests", "test_vector.py")
    cases = []
    for how in ("first", "last"):
        lits, src = literals(path, f"test_ss_{how}k")
        mixed, iso = lits[0:2], lits[2:4]
        for inp, (idx, vals) in (("v", mixed), ("v_iso", iso)):
            for k in range(0 if how == "first" else 1, len(idx) + 1):
                sl = slice(None, k) if how == "first" else slice(-k, None)
                cases.append(dict(source=src, input=inp, op="selectk", how=how, k=k,
                                  accept=[dict(idx=idx[sl], vals=vals[sl])]))
    for how in ("largest", "smallest"):
        lits, src = literals(path, f"test_ss_{how}k")
        assert len(lits) == 8
        pairs = [dict(idx=lits[i], vals=lits[i + 1]) for i in range(0, 8, 2)]
        cases.append(dict(source=src, input="v", op="selectk", how=how, k=1, accept=pairs[0:1]))
        cases.append(dict(source=src, input="v", op="selectk", how=how, k=2, accept=pairs[1:3]))
        cases.append(dict(source=src, input="v", op="selectk", how=how, k=3, accept=pairs[3:4]))
    lits, src = literals(path, "test_ss_compactify")
    orig, new, v_in, v_first, v_small, i_small = lits[:6]
    assert new == list(range(4)) and v_in == v_first
    for iso in (False, True):
        one = [1] * 4
        bases = [("first", "last", one if iso else v_first, False, 0), ("first", "last", orig, True, 0),
                 ("smallest", "largest", one if iso else v_small, False, 0)]
        if not iso:
            bases.append(("smallest", "largest", i_small, True, 3))
        for how_a, how_b, vals, asindex, stop in bases:
            for how, full in ((how_a, vals), (how_b, vals[::-1])):
                for n in [None] + list(reversed(range(stop, 5))):
                    for reverse in (False, True):
                        want = full if n is None else full[:n]
                        want = want[::-1] if reverse else want
                        cases.append(dict(source=src, input="vc_iso" if iso else "vc", op="compactify", how=how,
                                          k=n, reverse=reverse, asindex=asindex,
                                          accept=[dict(idx=list(range(len(want))), vals=want)]))
    return cases, dict(idx=orig, vals=v_in)


def main(ref):
    mpath = os.path.join(ref, "graphblas", "tests", "test_matrix.py")
    vpath = os.path.join(ref, "graphblas", "tests", "test_vector.py")
    a, _ = literals(mpath, "A")
    v, _ = literals(vpath, "v")
    vcases, vc = vector_cases(ref)
    out = {
        "comment": "The reference's selectk / compactify cases; written by make_selectk_golden.py, see its docstring.",
        "A": dict(nrows=7, ncols=7, dtype="INT64", rows=a[0], cols=a[1], vals=a[2]),
        "v": dict(size=7, dtype="INT64", idx=v[0], vals=v[1]),
        "vc": dict(size=7, dtype="INT64", idx=vc["idx"], vals=vc["vals"]),
        "matrix_cases": matrix_cases(ref),
        "vector_cases": vcases,
    }
    here = os.path.dirname(os.path.abspath(__file__))
    with open(os.path.join(here, "selectk_golden.json"), "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    print(len(out["matrix_cases"]), "matrix cases,", len(out["vector_cases"]), "vector cases")


if __name__ == "__main__":
    main(sys.argv[1])
