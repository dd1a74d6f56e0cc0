#!/usr/bin/env python3
"""Generate tests/golden/index_apply_golden.json from the reference's two tests of apply with an
index-unary operator: tests/test_matrix.py::test_apply_indexunary and
tests/test_vector.py::test_apply_indexunary.

    python tests/golden/make_index_apply_golden.py <root of the python-graphblas checkout>

The reference is read as TEXT: `ast` pulls the literal index lists, the arguments of the
`Matrix.from_coo` / `Vector.from_coo` calls (names resolved to the literal lists assigned in the
same function; `[c + 2 for c in cidx]` is the one comprehension, worked out here) and the scalar
thunks out of the two functions.  Nothing of the reference is imported or executed.  Every case
records the file:line of its expected object.  Which front-end forms lead to each expected object
is restated here in words (they are the tests' own statements, e.g. ``A.apply("colindex", 2)``).
The fixtures A (7 x 7) and v (size 7) are those of select_golden.json.
"""
import ast
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def function(path, name):
    for node in ast.walk(ast.parse(open(path).read())):
        if isinstance(node, ast.FunctionDef) and node.name == name:
            return node
    raise KeyError(f"{path}::{name}")


def value_of(node, env):
    """a literal, a name bound to one, or [name + const for name in list]"""
    if isinstance(node, ast.Name):
        return env[node.id]
    if isinstance(node, ast.ListComp):
        (gen,) = node.generators
        elt = node.elt
        assert isinstance(elt, ast.BinOp) and isinstance(elt.op, ast.Add) and not gen.ifs
        assert isinstance(elt.left, ast.Name) and elt.left.id == gen.target.id
        return [x + ast.literal_eval(elt.right) for x in value_of(gen.iter, env)]
    return ast.literal_eval(node)


def expected_objects(fn, rel):
    """{variable: the from_coo call assigned to it, as plain lists} in source order"""
    env, out = {}, {}
    for st in fn.body:
        if not (isinstance(st, ast.Assign) and len(st.targets) == 1 and isinstance(st.targets[0], ast.Name)):
            continue
        name, val = st.targets[0].id, st.value
        if isinstance(val, ast.Call) and isinstance(val.func, ast.Attribute) and val.func.attr == "from_coo":
            args = [value_of(a, env) for a in val.args]
            kw = {}
            for k in val.keywords:
                kw[k.arg] = k.value.id if isinstance(k.value, ast.Name) else ast.literal_eval(k.value)
            out[name] = {"src": f"{rel}:{st.lineno}", "args": args, "kw": kw}
        elif isinstance(val, (ast.List, ast.ListComp)):
            env[name] = value_of(val, env)
    return out


def scalar_thunk(fn, name):
    """the value of Scalar `name`: Scalar.from_value(x, ...) or `name.value = x`"""
    for node in ast.walk(fn):
        if isinstance(node, ast.Assign) and len(node.targets) == 1:
            t, v = node.targets[0], node.value
            if isinstance(t, ast.Name) and t.id == name and isinstance(v, ast.Call) \
                    and getattr(v.func, "attr", "") == "from_value":
                return ast.literal_eval(v.args[0])
            if isinstance(t, ast.Attribute) and t.attr == "value" and getattr(t.value, "id", "") == name:
                return ast.literal_eval(v)
    raise KeyError(name)


def main(ref):
    sel = json.load(open(os.path.join(HERE, "select_golden.json")))
    out = {"note": "fixtures and expected triples of the reference's apply-with-index-unary tests "
                   "(numbers only); forms: [how the operator is given, its name, the thunk]",
           "A": sel["A"], "v": sel["v"]}

    rel = "tests/test_matrix.py"
    fn = function(os.path.join(ref, "graphblas", rel), "test_apply_indexunary")
    obj = expected_objects(fn, rel)
    s3 = scalar_thunk(fn, "s3")

    def mcase(name, var, dtype, forms):
        o = obj[var]
        r, c, v = o["args"]
        return {"src": o["src"], "name": name, "dtype": dtype, "forms": forms, "rows": r, "cols": c,
                "vals": [int(x) for x in v]}

    out["matrix_cases"] = [
        # r1 = A.apply("rowindex"); r2 = A.apply(indexunary.rowindex); r3 = indexunary.rowindex(A)
        mcase("rowindex", "Ar", "INT64", [["str", "rowindex", None], ["op", "rowindex", None],
                                          ["call", "rowindex", None]]),
        # c1 = A.apply("colindex", 2); c2 = A.apply(indexunary.colindex, 2);
        # c3 = indexunary.colindex(A, thunk=2)
        mcase("colindex2", "Ac", "INT64", [["str", "colindex", 2], ["op", "colindex", 2],
                                           ["call_thunk_kw", "colindex", 2]]),
        # w1 = A.apply(indexunary.valueeq, s3); w2 = A.apply(select.valueeq, s3);
        # w3 = A.apply("==", s3); w4 = indexunary.valueeq(A, s3)   (s3 an INT64 Scalar)
        mcase("valueeq3", "A3", "BOOL", [["op_scalar", "valueeq", s3], ["selectop_scalar", "valueeq", s3],
                                         ["str_scalar", "==", s3], ["call_scalar", "valueeq", s3]]),
    ]
    assert obj["A3"]["kw"] == {"dtype": "bool"}

    rel = "tests/test_vector.py"
    fn = function(os.path.join(ref, "graphblas", rel), "test_apply_indexunary")
    obj = expected_objects(fn, rel)
    s2 = scalar_thunk(fn, "s2")

    def vcase(name, var, dtype, forms):
        o = obj[var]
        i, v = o["args"]
        return {"src": o["src"], "name": name, "dtype": dtype, "forms": forms, "idx": i, "vals": [int(x) for x in v]}

    out["vector_cases"] = [
        # r1 = v.apply(indexunary.index); r2 = v.apply("index"); r3 = indexunary.index(v)
        vcase("index", "vr", "INT64", [["op", "index", None], ["str", "index", None], ["call", "index", None]]),
        # w1 = v.apply("==", s2); w2 = v.apply(indexunary.valueeq, s2); w3 = v.apply(select.valueeq, s2);
        # w4 = indexunary.valueeq(v, s2)   (s2 an INT64 Scalar)
        vcase("valueeq2", "v2", "BOOL", [["str_scalar", "==", s2], ["op_scalar", "valueeq", s2],
                                         ["selectop_scalar", "valueeq", s2], ["call_scalar", "valueeq", s2]]),
    ]
    with open(os.path.join(HERE, "index_apply_golden.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1])
