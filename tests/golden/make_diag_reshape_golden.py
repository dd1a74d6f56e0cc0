#!/usr/bin/env python3
"""Generate tests/golden/diag_reshape_golden.json from the reference's tests of diag, flatten and
reshape: tests/test_matrix.py::test_diag (with its parametrisation), tests/test_vector.py::test_diag,
tests/test_matrix.py::test_ss_flatten and tests/test_matrix.py::test_ss_reshape.

    python tests/golden/make_diag_reshape_golden.py <root of the python-graphblas checkout>

The reference is read as TEXT: `ast` pulls the parametrisation, the literal `data` lists, the
`range` of k, the shapes, the arguments of every `.ss.reshape(...)` / `.ss.flatten(...)` call and
the `pytest.raises` blocks out of the four functions.  Nothing of the reference is imported or
executed.  The arithmetic the tests state in Python (`row * A.ncols + col`, `idx // 16`, ...) is
restated here, next to the line it comes from; every case records its file:line.  The parts of
test_ss_flatten that go through `ss.export` / `import_*` are left out: their flatten / reshape
statements are kept, applied to the fixture itself.  The fixtures A (7 x 7) and v (size 7) are
those of select_golden.json.
"""
import ast
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def function(tree, name):
    for node in ast.walk(tree):
        if isinstance(node, ast.FunctionDef) and node.name == name:
            return node
    raise KeyError(name)


def evaluate(node, shape):
    """a literal; `<name>.shape` is shape[name], also starred inside a tuple or a call"""
    if isinstance(node, ast.Attribute) and node.attr == "shape":
        return list(shape[node.value.id])
    if isinstance(node, ast.Tuple):
        out = []
        for e in node.elts:
            if isinstance(e, ast.Starred):
                out.extend(evaluate(e.value, shape))
            else:
                out.append(evaluate(e, shape))
        return out
    return ast.literal_eval(node)


def call_args(call, shape):
    args = []
    for a in call.args:
        if isinstance(a, ast.Starred):
            args.extend(evaluate(a.value, shape))
        else:
            args.append(evaluate(a, shape))
    return {"args": args, "kwargs": {k.arg: ast.literal_eval(k.value) for k in call.keywords}}


def ss_calls(fn, method):
    """every `<name>.ss.<method>(...)` call of fn outside its `with pytest.raises` blocks, in source
    order: (line, receiver, call)"""
    inside = {id(n) for w in ast.walk(fn) if isinstance(w, ast.With) for n in ast.walk(w)}
    out = []
    for node in ast.walk(fn):
        if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr == method \
                and isinstance(node.func.value, ast.Attribute) and node.func.value.attr == "ss" \
                and id(node) not in inside:
            out.append((node.lineno, node.func.value.value.id, node))
    return sorted(out, key=lambda t: t[0])


def unique(forms):
    return [f for i, f in enumerate(forms) if f not in forms[:i]]


def raises_blocks(fn, rel, shapes):
    """the `with pytest.raises(E, match=...)` blocks of fn whose body is one .ss.reshape / .ss.flatten call"""
    out = []
    for node in ast.walk(fn):
        if not isinstance(node, ast.With):
            continue
        ctx = node.items[0].context_expr
        if not (isinstance(ctx, ast.Call) and getattr(ctx.func, "attr", "") == "raises"):
            continue
        call = node.body[0].value
        recv = call.func.value.value.id
        rec = {"src": f"{rel}:{node.lineno}", "raises": ctx.args[0].id,
               "match": {k.arg: ast.literal_eval(k.value) for k in ctx.keywords}["match"],
               "of": recv, "method": call.func.attr,
               "shape": list(shapes[recv]) if recv in shapes else [shapes["A"][0] * shapes["A"][1]]}  # v = A.ss.flatten()
        rec.update(call_args(call, shapes))
        out.append(rec)
    return sorted(out, key=lambda r: int(r["src"].split(":")[1]))


def main(ref):
    sel = json.load(open(os.path.join(HERE, "select_golden.json")))
    A, v = sel["A"], sel["v"]
    out = {"note": "fixtures, expected tuples and call arguments of the reference's diag / flatten / reshape "
                   "tests (numbers and argument lists only)", "A": A, "v": v}

    # ---- tests/test_matrix.py::test_diag: expected = Vector.from_coo(indices, values, size=max(0, A.nrows - abs(k)))
    rel = "tests/test_matrix.py"
    tree = ast.parse(open(os.path.join(ref, "graphblas", rel)).read())
    fn = function(tree, "test_diag")
    (params,) = [d.args[1] for d in fn.decorator_list if isinstance(d, ast.Call) and getattr(d.func, "attr", "") == "parametrize"]
    out["matrix_diag"] = []
    for elt in params.elts:
        k, idx, vals = ast.literal_eval(elt)
        out["matrix_diag"].append({"src": f"{rel}:{elt.lineno}", "k": k, "size": max(0, A["nrows"] - abs(k)),
                                   "idx": idx, "vals": vals})

    # ---- tests/test_matrix.py::test_ss_flatten
    fn = function(tree, "test_ss_flatten")
    (data,) = [st.value for st in fn.body if isinstance(st, ast.Assign) and getattr(st.targets[0], "id", "") == "data"]
    r, c, x = ast.literal_eval(data)
    assert (r, c, x) == (A["rows"], A["cols"], A["vals"])  # the test's data is the fixture
    nr, nc = A["nrows"], A["ncols"]
    assigns = [st for st in fn.body if isinstance(st, ast.Assign) and getattr(st.targets[0], "id", "") == "indices"]
    flat = []
    for st, order in zip(assigns, ("rowwise", "columnwise")):
        # indices = [row * A.ncols + col ...] / [col * A.nrows + row ...]; expected = Vector.from_coo(indices, data[2], size=A.nrows * A.ncols)
        lin = [i * nc + j for i, j in zip(r, c)] if order == "rowwise" else [j * nr + i for i, j in zip(r, c)]
        flat.append({"src": f"{rel}:{st.lineno}", "order": order, "size": nr * nc, "idx": lin, "vals": x,
                     "flatten_forms": [], "reshape_forms": []})
    split = assigns[1].lineno
    for line, recv, call in ss_calls(fn, "flatten"):  # v = B.ss.flatten(...); assert v.isequal(expected)
        flat[line > split]["flatten_forms"].append(call_args(call, {"A": (nr, nc), "B": (nr, nc)}))
    for line, recv, call in ss_calls(fn, "reshape"):  # C = v.ss.reshape(...); assert C.isequal(B)
        flat[line > split]["reshape_forms"].append(call_args(call, {"A": (nr, nc), "B": (nr, nc)}))
    for f in flat:
        f["flatten_forms"], f["reshape_forms"] = unique(f["flatten_forms"]), unique(f["reshape_forms"])
    out["flatten"] = flat
    errors = raises_blocks(fn, rel, {"A": (nr, nc)})

    # ---- tests/test_matrix.py::test_ss_reshape: A.resize(8, 8); idx = c + 8 * r;
    # expected = Matrix.from_coo(idx // 16, idx % 16, v, nrows=4, ncols=16); then idx = r + 8 * c;
    # expected = Matrix.from_coo(idx % 4, idx // 4, v, nrows=4, ncols=16)
    fn = function(tree, "test_ss_reshape")
    (resize,) = [n for n in ast.walk(fn) if isinstance(n, ast.Call) and getattr(n.func, "attr", "") == "resize"]
    n0, n1 = [ast.literal_eval(a) for a in resize.args]
    expected = [st for st in fn.body if isinstance(st, ast.Assign) and getattr(st.targets[0], "id", "") == "expected"]
    cases = []
    for st, order in zip(expected, ("rowwise", "columnwise")):
        kw = {k.arg: ast.literal_eval(k.value) for k in st.value.keywords}
        m, n = kw["nrows"], kw["ncols"]
        if order == "rowwise":
            lin = [j + n1 * i for i, j in zip(r, c)]
            rows, cols = [q // n for q in lin], [q % n for q in lin]
        else:
            lin = [i + n0 * j for i, j in zip(r, c)]
            rows, cols = [q % m for q in lin], [q // m for q in lin]
        cases.append({"src": f"{rel}:{st.lineno}", "order": order, "nrows": m, "ncols": n, "rows": rows,
                      "cols": cols, "vals": x, "forms": []})
    back = None
    for line, recv, call in ss_calls(fn, "reshape"):
        form = call_args(call, {"A": (n0, n1)})
        if recv == "rv":  # assert rv.ss.reshape(8, 8, inplace=True) is None; assert rv.isequal(A)
            back = dict(form, src=f"{rel}:{line}")
        else:  # rv = A.ss.reshape(...); assert rv.isequal(expected)
            cases[line > expected[1].lineno]["forms"].append(form)
    out["reshape"] = {"resize": [n0, n1], "cases": cases, "inplace_back": back}
    errors += raises_blocks(fn, rel, {"A": (n0, n1)})
    out["errors"] = errors

    # ---- tests/test_vector.py::test_diag: for k in range(-5, 5): size = v.size + abs(k);
    # rows = indices + max(0, -k); cols = indices + max(0, k);
    # expected = Matrix.from_coo(rows, cols, values, nrows=size, ncols=size, dtype=v.dtype);
    # then A.diag(k) and A.T.diag(-k, dtype=float) give v back (INT64 and FP64)
    rel = "tests/test_vector.py"
    fn = function(ast.parse(open(os.path.join(ref, "graphblas", rel)).read()), "test_diag")
    (loop,) = [st for st in fn.body if isinstance(st, ast.For)]
    lo, hi = [ast.literal_eval(a) for a in loop.iter.args]
    (exp,) = [st for st in loop.body if isinstance(st, ast.Assign) and getattr(st.targets[0], "id", "") == "expected"]
    out["vector_diag"] = [{"src": f"{rel}:{exp.lineno}", "k": k, "n": v["size"] + abs(k),
                           "rows": [i + max(0, -k) for i in v["idx"]], "cols": [i + max(0, k) for i in v["idx"]],
                           "vals": v["vals"]} for k in range(lo, hi)]
    with open(os.path.join(HERE, "diag_reshape_golden.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1])
