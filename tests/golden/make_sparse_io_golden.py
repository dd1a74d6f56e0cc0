#!/usr/bin/env python3
"""Generate tests/golden/sparse_io_golden.json from the reference's tests of the sparse constructors
and exports: tests/test_matrix.py::test_from_coo, ::test_from_coo_scalar, ::test_to_csr_from_csc
(with the 7 x 7 fixture `A` they use) and tests/test_vector.py::test_from_coo.

    python tests/golden/make_sparse_io_golden.py <root of the python-graphblas checkout>

The reference is read as TEXT: `ast` walks the statements of the four functions and records what
each line states -- a constructor call with literal arguments, the asserts on the object it named
(nrows, ncols, size, nvals, dtype, one element), an `isequal` between two such objects, a round
trip of the fixture through an export and a constructor, a `pytest.raises` block.  Nothing of the
reference is imported or executed; every case records its file:line.

Left out, on purpose: statements that need SuiteSparse's `.ss` namespace, an index array of floats
(test_vector.py:131-135: this library refuses both forms), `C[0, 0] = 0` (an assign, not an import)
and the `InvalidObject` of test_matrix.py:3990-3991 (an index past ncols is GrB_INDEX_OUT_OF_BOUNDS
here; the GPU suite tests that refusal itself).
"""
import ast
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCES = [("graphblas/tests/test_matrix.py", "test_from_coo"),
           ("graphblas/tests/test_matrix.py", "test_from_coo_scalar"),
           ("graphblas/tests/test_matrix.py", "test_to_csr_from_csc"),
           ("graphblas/tests/test_vector.py", "test_from_coo")]
SKIP = {"graphblas/tests/test_vector.py": {135}, "graphblas/tests/test_matrix.py": {3991}}  # see above
CONSTRUCTORS = ("from_coo", "from_csr", "from_csc")
EXPORTS = ("to_csr", "to_csc", "to_coo")
DTYPES = {"bool": "BOOL", "int": "INT64", "float": "FP64"}


def function(tree, name):
    for node in tree.body:
        if isinstance(node, ast.FunctionDef) and node.name == name:
            return node
    raise KeyError(name)


def dotted(node):
    parts = []
    while isinstance(node, ast.Attribute):
        parts.append(node.attr)
        node = node.value
    if not isinstance(node, ast.Name):
        return None
    return ".".join([node.id] + parts[::-1])


class Unreadable(Exception):
    pass


def literal(node):
    """a literal, a dtype or operator name, or an export of the fixture"""
    name = dotted(node)
    if name in DTYPES:
        return {"dtype": DTYPES[name]}
    if name and name.startswith("dtypes."):
        return {"dtype": name.split(".")[1]}
    if name and name.split(".")[0] in ("binary", "monoid"):
        return {"op": name}
    try:
        return ast.literal_eval(node)
    except ValueError:
        raise Unreadable(ast.dump(node)) from None


def export_of(node):
    """{"of": "A" | "A.T", "export", "kwargs"} of `A.to_csr(...)` / `A.T.to_csc(...)`, else None"""
    if not isinstance(node, ast.Call):
        return None
    name = dotted(node.func)
    if not name or name.split(".")[-1] not in EXPORTS or name.split(".")[0] != "A":
        return None
    kwargs = {k.arg: literal(k.value) for k in node.keywords}
    return {"of": ".".join(name.split(".")[:-1]), "export": name.split(".")[-1], "kwargs": kwargs}


class Reader:
    def __init__(self, rel):
        self.rel, self.objects, self.cases = rel, {}, []

    def src(self, node):
        return f"{self.rel}:{node.lineno}"

    def constructor(self, call):
        """the record of a Matrix / Vector constructor call, else None"""
        if not isinstance(call, ast.Call):
            return None
        name = dotted(call.func)
        if name in ("Matrix", "Vector"):  # Matrix(int, 2, 2), Vector(dtypes.INT64, size=10)
            args = [literal(a) for a in call.args]
            kwargs = {k.arg: literal(k.value) for k in call.keywords}
            return {"kind": name, "how": "new", "args": args, "kwargs": kwargs, "src": self.src(call)}
        if not name or name.split(".")[-1] not in CONSTRUCTORS or name.split(".")[0] not in ("Matrix", "Vector"):
            return None
        kind, how = name.split(".")
        args = []
        for a in call.args:
            if isinstance(a, ast.Starred):
                ex = export_of(a.value)
                if ex is None:
                    raise Unreadable(ast.dump(a))
                args.append({"star": ex})
            else:
                args.append(literal(a))
        kwargs = {k.arg: literal(k.value) for k in call.keywords}
        return {"kind": kind, "how": how, "args": args, "kwargs": kwargs, "src": self.src(call)}

    def operand(self, node):
        """an object: a name bound earlier, the fixture, or a constructor call"""
        if isinstance(node, ast.Name):
            if node.id == "A":
                return {"fixture": "A"}
            if node.id in self.objects:
                return self.objects[node.id]
            raise Unreadable(node.id)
        if isinstance(node, ast.Call) and dotted(node.func) == "A.dup":
            return {"fixture": "A", "dup": literal(node.args[0])}
        rec = self.constructor(node)
        if rec is None:
            raise Unreadable(ast.dump(node))
        return rec

    def assertion(self, test, node):
        if isinstance(test, ast.Compare) and len(test.ops) == 1 and isinstance(test.ops[0], ast.Eq):
            left, right = test.left, test.comparators[0]
            name = dotted(left)
            if name and name.split(".")[0] in self.objects and len(name.split(".")) == 2:
                obj, attr = name.split(".")
                if attr in ("nrows", "ncols", "size", "nvals", "dtype"):
                    v = literal(right)
                    self.cases.append({"check": "attribute", "of": self.objects[obj], "attribute": attr,
                                       "expect": v["dtype"] if isinstance(v, dict) else v, "src": self.src(node)})
                    return
            # C3[1, 1].new() == 6
            if isinstance(left, ast.Call) and isinstance(left.func, ast.Attribute) and left.func.attr == "new" \
                    and isinstance(left.func.value, ast.Subscript) and isinstance(left.func.value.value, ast.Name) \
                    and left.func.value.value.id in self.objects:
                sub = left.func.value
                index = literal(sub.slice)
                self.cases.append({"check": "element", "of": self.objects[sub.value.id],
                                   "index": list(index) if isinstance(index, tuple) else [index],
                                   "expect": literal(right), "src": self.src(node)})
                return
            raise Unreadable(ast.dump(test))
        if isinstance(test, ast.Call) and isinstance(test.func, ast.Attribute) and test.func.attr == "isequal":
            kwargs = {k.arg: literal(k.value) for k in test.keywords}
            self.cases.append({"check": "isequal", "left": self.operand(test.func.value),
                               "right": self.operand(test.args[0]), "check_dtype": bool(kwargs.get("check_dtype")),
                               "src": self.src(node)})
            return
        raise Unreadable(ast.dump(test))

    def raises(self, node):
        item = node.items[0].context_expr
        if not (isinstance(item, ast.Call) and dotted(item.func) == "pytest.raises"):
            raise Unreadable("with")
        exc = dotted(item.args[0])
        match = next((literal(k.value) for k in item.keywords if k.arg == "match"), None)
        for stmt in node.body:
            call = stmt.value if isinstance(stmt, ast.Expr) else stmt.test if isinstance(stmt, ast.Assert) else None
            rec = self.constructor(call)
            if rec is None:
                raise Unreadable(ast.dump(stmt))
            self.cases.append({"check": "raises", "call": rec, "raises": exc, "match": match, "src": self.src(stmt)})

    def statement(self, node):
        if isinstance(node, ast.Assign) and len(node.targets) == 1 and isinstance(node.targets[0], ast.Name):
            rec = self.constructor(node.value)
            if rec is None:
                raise Unreadable(ast.dump(node))
            self.objects[node.targets[0].id] = rec
        elif isinstance(node, ast.Assert):
            self.assertion(node.test, node)
        elif isinstance(node, ast.With):
            self.raises(node)
        else:
            raise Unreadable(ast.dump(node))


def fixture_A(tree):
    """the three lists of the fixture `A`: rows, columns, values"""
    fn = function(tree, "A")
    for node in fn.body:
        if isinstance(node, ast.Assign) and node.targets[0].id == "data":
            return ast.literal_eval(node.value)
    raise KeyError("data")


def main(root):
    cases, skipped, fixture = [], [], None
    for rel, name in SOURCES:
        with open(os.path.join(root, rel)) as f:
            tree = ast.parse(f.read())
        if rel.endswith("test_matrix.py") and fixture is None:
            fixture = fixture_A(tree)
        reader = Reader(rel)
        for node in function(tree, name).body:
            if isinstance(node, ast.If):  # `if suitesparse:` blocks
                skipped.append(reader.src(node))
                continue
            try:
                reader.statement(node)
            except Unreadable:
                skipped.append(reader.src(node))
        for c in reader.cases:
            c["test"] = name
            if int(c["src"].split(":")[1]) in SKIP.get(rel, ()):
                skipped.append(c["src"])
            else:
                cases.append(c)
    out = {"source": "python-graphblas, graphblas/tests (read as text by make_sparse_io_golden.py)",
           "fixture_A": {"rows": fixture[0], "columns": fixture[1], "values": fixture[2]},
           "not_read": skipped, "cases": cases}
    with open(os.path.join(HERE, "sparse_io_golden.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(f"{len(cases)} cases, {len(skipped)} statements not read: {skipped}")


if __name__ == "__main__":
    main(sys.argv[1])
