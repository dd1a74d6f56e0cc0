#!/usr/bin/env python3
"""Generate tests/golden/subassign_golden.json from the reference's tests of assign and subassign on
regions: tests/test_matrix.py::test_assign (its two block assignments), test_assign_row,
test_assign_column, test_subassign_row_col, test_subassign_matrix, test_assign_row_col_matrix_mask,
test_subassign_combos, and tests/test_vector.py::test_subassign.

    python tests/golden/make_subassign_golden.py <root of the python-graphblas checkout>

The reference is read as TEXT: `ast` pulls every `from_coo(...)` literal (with the name it is bound
to and its line), the `params` table of test_subassign_combos, and the line of every assigning
statement (`X[...] = v`, `X[...](...) << v`, `X(...)[...] << v`, `....update(v)`) out of the
functions.  Nothing of the reference is imported or executed.  What each statement says -- target,
index lists, mask and its kind, accum, replace, value -- is restated below by hand as one tuple per
statement, in source order; the generator checks that there are as many tuples as the text has
statements and records each with its file:line.  The k-th object bound to a name that starts with
`result` is the state expected after the k-th non-raising step.  The steps `C(B.S)[...] << v2`
(a Matrix mask of C's shape with a row or column index) need GrB_Matrix_assign with index lists
and are marked `needs_matrix_assign`.  The fixtures A (7 x 7) and v (size 7) are those of
select_golden.json.
"""
import ast
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ALL = "all"


def function(tree, name):
    for node in ast.walk(tree):
        if isinstance(node, ast.FunctionDef) and node.name == name:
            return node
    raise KeyError(name)


def coo_objects(fn, rel):
    """every `name = Matrix.from_coo(...)` / `Vector.from_coo(...)` of fn in source order"""
    out = []
    for node in ast.walk(fn):
        if isinstance(node, ast.Assign) and isinstance(node.value, ast.Call) \
                and getattr(node.value.func, "attr", "") == "from_coo" and isinstance(node.targets[0], ast.Name):
            try:
                args = [ast.literal_eval(a) for a in node.value.args]
            except ValueError:
                continue  # built from variables (test_subassign_combos' expected)
            kw = {k.arg: ast.literal_eval(k.value) for k in node.value.keywords if k.arg != "name"}
            kind = node.value.func.value.id
            rec = {"name": node.targets[0].id, "src": f"{rel}:{node.lineno}", "kind": kind.lower()}
            if kind == "Matrix":
                rec.update(rows=args[0], cols=args[1], vals=args[2], nrows=kw.get("nrows", max(args[0]) + 1),
                           ncols=kw.get("ncols", max(args[1]) + 1))
            else:
                rec.update(idx=args[0], vals=args[1], size=kw.get("size", max(args[0]) + 1))
            out.append(rec)
    return sorted(out, key=lambda r: int(r["src"].split(":")[1]))


def is_assigning(node):
    if isinstance(node, ast.Assign):
        return isinstance(node.targets[0], ast.Subscript)
    if isinstance(node, ast.Expr):
        v = node.value
        if isinstance(v, ast.BinOp) and isinstance(v.op, ast.LShift):
            return any(isinstance(n, ast.Subscript) for n in ast.walk(v.left))
        return isinstance(v, ast.Call) and getattr(v.func, "attr", "") == "update"
    return False


def statement_lines(fn):
    return sorted(n.lineno for n in ast.walk(fn) if is_assigning(n))


def chain(fn, rel, table, fixtures=(), limit=None):
    """the hand-written tuples of `table` joined with the statements of fn"""
    lines = statement_lines(fn)[:limit]
    assert len(lines) == len(table), (fn.name, len(lines), len(table))
    objs = coo_objects(fn, rel)
    results = [o for o in objs if o["name"].startswith("result")]
    steps, k = [], 0
    for line, (target, fresh, form, I, J, mask, mkind, accum, replace, value, expect) in zip(lines, table):
        st = {"src": f"{rel}:{line}", "target": target, "fresh": fresh, "form": form, "I": I, "J": J, "mask": mask,
              "mask_kind": mkind, "accum": accum, "replace": replace, "value": value}
        if expect == "result":
            st["expect"] = {"result": k}
            k += 1
        elif expect == "needs_matrix_assign":
            st["needs_matrix_assign"] = True
            st["expect"] = {"result": k}
            k += 1
        elif expect[0] == "result_at":  # the text compares with an object it has used before
            st["expect"] = {"result": expect[1]}
        else:
            st["expect"] = {"raises": expect[0], "match": expect[1]}
        steps.append(st)
    assert k == len(results), (fn.name, k, len(results))
    return {"fixtures": list(fixtures), "objects": [o for o in objs if not o["name"].startswith("result")],
            "results": results, "steps": steps}


def sc(x):
    return {"scalar": x}


SUBMASK_VECTOR = "Indices for subassign imply Vector submask, but got Matrix mask instead"

# (target, fresh copy of the target's base first, form, I, J, mask, mask kind, accum, replace, value, expect)
T_ASSIGN = [  # C()[[0, 2], [0, 5]] = B;  C[:3:2, :6:5]() << B
    ("A", True, "assign", [0, 2], [0, 5], None, None, None, False, "B", "result"),
    ("A", True, "subassign", {"slice": [None, 3, 2]}, {"slice": [None, 6, 5]}, None, None, None, False, "B",
     ("result_at", 0)),
]
T_ASSIGN_ROW = [("A", True, "assign", 0, ALL, None, None, None, False, "v", "result")]
T_ASSIGN_COL = [("A", True, "assign", ALL, 1, None, None, None, False, "v", "result")]
T_SUB_ROW_COL = [
    ("A", False, "subassign", [0, 1], 0, "m", "S", None, False, "v", "result"),
    ("A", False, "subassign", 1, [1, 2], "m", "V", "plus", False, "v", "result"),
    ("A", False, "subassign", [0, 1], 0, "m", "S", "plus", True, "v", "result"),
    ("A", False, "assign", [0, 1], 0, "m", "S", None, False, "v", ("DimensionMismatch", None)),
    ("A", False, "subassign", [0, 1], 0, "m", "S", None, False, sc(99), "result"),
    ("A", False, "subassign", [1, 2], 0, "m", "S", "plus", True, sc(100), "result"),
    ("A", False, "subassign", 2, [0, 1], "m", "S", None, False, sc(-1), "result"),
]
T_SUB_MATRIX = [
    ("A", False, "subassign", [0, 1], [0], "m", "S", None, False, "v", "result"),
    ("A", False, "subassign", [1], [1, 2], "mT", "V", "plus", False, "v.T", "result"),
    ("A", False, "subassign", [0, 1], [0], "m", "S", "plus", True, "v", "result"),
    ("A", False, "assign", [0, 1], [0], "m", "S", None, False, "v", ("DimensionMismatch", None)),
    ("A", False, "subassign", [0, 1], [0], "m", "S", None, False, sc(99), "result"),
    ("A", False, "subassign", [1, 2], [0], "m", "S", "plus", True, sc(100), "result"),
    ("A", False, "subassign", [2], [0, 1], "mT", "S", None, False, sc(-1), "result"),
]
T_ROW_COL_MATRIX_MASK = [
    ("A", True, "assign", 0, ALL, "B", "S", None, False, "v2", "needs_matrix_assign"),
    ("A", True, "assign", 1, ALL, "B", "S", "plus", False, "v2", "needs_matrix_assign"),
    ("A", True, "assign", 1, ALL, "B", "S", None, True, "v2", "needs_matrix_assign"),
    ("A", True, "assign", ALL, 0, "B", "S", None, False, "v2", "needs_matrix_assign"),
    ("A", True, "assign", ALL, 1, "B", "S", "plus", False, "v2", "needs_matrix_assign"),
    ("A", True, "assign", ALL, 1, "B", "S", None, True, "v2", "needs_matrix_assign"),
    ("A", True, "assign", 0, ALL, "B", "S", None, False, sc(100), "result"),
    ("A", True, "assign", 1, ALL, "B", "S", "plus", False, sc(100), "result"),
    ("A", True, "assign", 1, ALL, "B", "S", None, True, sc(100), "result"),
    ("A", True, "assign", ALL, 0, "B", "S", None, False, sc(100), "result"),
    ("A", True, "assign", ALL, 1, "B", "S", "plus", False, sc(100), "result"),
    ("A", True, "assign", ALL, 1, "B", "S", None, True, sc(100), "result"),
    ("A", True, "subassign", 0, ALL, "v2", "S", None, False, "v2", "result"),
    ("A", True, "subassign", 0, [0], "v1", "S", None, False, "v1", "result"),
    ("A", False, "subassign", 0, ALL, "B", "S", None, False, "v2", ("TypeError", SUBMASK_VECTOR)),
    ("A", True, "subassign", ALL, 0, "v2", "S", None, False, "v2", "result"),
    ("A", True, "subassign", [0], 0, "v1", "S", None, False, "v1", "result"),
    ("A", False, "subassign", ALL, 0, "B", "S", None, False, "v2", ("TypeError", SUBMASK_VECTOR)),
    ("A", True, "subassign", 0, ALL, "v2", "S", None, False, sc(100), "result"),
    ("A", True, "subassign", 0, [0], "v1", "S", None, False, sc(100), "result"),
    ("A", False, "subassign", ALL, 0, "B", "S", None, False, sc(100), ("TypeError", SUBMASK_VECTOR)),
    ("A", True, "subassign", ALL, 0, "v2", "S", None, False, sc(100), "result"),
    ("A", True, "subassign", [0], 0, "v1", "S", None, False, sc(100), "result"),
    ("A", False, "subassign", ALL, 0, "B", "S", None, False, sc(100), ("TypeError", SUBMASK_VECTOR)),
    ("A", False, "subassign", 0, 0, "B", "S", None, False, sc(100),
     ("TypeError", "Single element assign does not accept a submask")),
]
T_VECTOR_SUBASSIGN = [  # the mask is `v` itself in the DimensionMismatch steps; `fixtureA` is the 7 x 7 fixture
    ("v", False, "subassign", [0, 1], None, "m", "S", None, False, "w", "result"),
    ("v", False, "subassign", [0, 1], None, "v", "S", None, False, "w", ("DimensionMismatch", None)),
    ("v", False, "subassign", [0, 1], None, "m", "S", None, False, "v", ("DimensionMismatch", None)),
    ("v", False, "subassign", [0, 1], None, "m", "S", None, False, sc(100), "result"),
    ("v", False, "subassign", [0, 1], None, "v", "S", None, False, sc(99), ("DimensionMismatch", None)),
    ("v", False, "subassign", [0, 1], None, "fixtureA", "S", None, False, sc(88),
     ("TypeError", "Mask object must be type Vector")),
    ("v", False, "subassign", [0, 1], None, "fixtureA", "S", None, False, "w",
     ("TypeError", "Mask object must be type Vector")),
]


def combos(fn, rel):
    """test_subassign_combos: self[index](binary.plus, mask, replace=replace) << val in four shapes"""
    base = {o["name"]: o for o in coo_objects(fn, rel)}
    (params,) = [st.value for st in fn.body if isinstance(st, ast.Assign) and getattr(st.targets[0], "id", "") == "params"]
    rows = []
    for elt in params.elts:
        kind = elt.elts[0].id
        replace, idx, vals = [ast.literal_eval(e) for e in elt.elts[1:]]
        rows.append({"src": f"{rel}:{elt.lineno}", "mask_kind": kind, "replace": replace, "idx": idx, "vals": vals})
    (deco,) = [d for d in fn.decorator_list if isinstance(d, ast.Call) and getattr(d.func, "attr", "") == "parametrize"]
    index = []
    for e in deco.args[1].elts:  # slice(12), list(range(12))
        index.append("slice" if e.func.id == "slice" else "list")
        n = e.args[0] if e.func.id == "slice" else e.args[0].args[0]
        assert ast.literal_eval(n) == 12
    loops = [st for st in fn.body if isinstance(st, ast.For)]
    assert len(loops) == 4
    shapes = [{"src": f"{rel}:{lp.lineno}", "shape": s} for lp, s in zip(loops, ("vector", "row", "column", "matrix"))]
    return {"mask": base["mask_base"], "val": base["val_base"], "self": base["self_base"], "accum": "plus",
            "n": 12, "index": index, "shapes": shapes, "params": rows}


def main(ref):
    sel = json.load(open(os.path.join(HERE, "select_golden.json")))
    out = {"note": "fixtures, expected tuples and statement descriptions of the reference's assign / subassign "
                   "tests on regions (numbers, names and argument descriptions only)", "A": sel["A"], "v": sel["v"]}
    rel = "tests/test_matrix.py"
    tree = ast.parse(open(os.path.join(ref, "graphblas", rel)).read())
    out["test_assign"] = chain(function(tree, "test_assign"), rel, T_ASSIGN, ("A",), limit=2)
    out["test_assign_row"] = chain(function(tree, "test_assign_row"), rel, T_ASSIGN_ROW, ("A", "v"))
    out["test_assign_column"] = chain(function(tree, "test_assign_column"), rel, T_ASSIGN_COL, ("A", "v"))
    out["test_subassign_row_col"] = chain(function(tree, "test_subassign_row_col"), rel, T_SUB_ROW_COL)
    out["test_subassign_matrix"] = chain(function(tree, "test_subassign_matrix"), rel, T_SUB_MATRIX)
    out["test_assign_row_col_matrix_mask"] = chain(function(tree, "test_assign_row_col_matrix_mask"), rel,
                                                   T_ROW_COL_MATRIX_MASK)
    out["test_subassign_combos"] = combos(function(tree, "test_subassign_combos"), rel)
    rel = "tests/test_vector.py"
    tree = ast.parse(open(os.path.join(ref, "graphblas", rel)).read())
    out["test_vector_subassign"] = chain(function(tree, "test_subassign"), rel, T_VECTOR_SUBASSIGN, ("fixtureA",),
                                         limit=len(T_VECTOR_SUBASSIGN))
    with open(os.path.join(HERE, "subassign_golden.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1])
