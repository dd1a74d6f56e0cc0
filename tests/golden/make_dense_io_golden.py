#!/usr/bin/env python3
"""Generate tests/golden/dense_io_golden.json from the reference's tests of from_dense / to_dense:
tests/test_matrix.py::test_to_dense_from_dense (:4171-4198), tests/test_vector.py::
test_to_dense_from_dense (:2552-2577) and the from_dense / to_dense lines of tests/test_io.py::
test_vector_to_from_numpy (:55-57, with the array of :54 and the comparison of :58) and
::test_matrix_to_from_numpy (:101-103, with :100 and :104).

    python tests/golden/make_dense_io_golden.py <root of the python-graphblas checkout>

The reference is read as TEXT: `ast` walks the statements of the four functions and a small
interpreter of the few forms they use (literals, np.arange(n).reshape(...), np.array(...),
Scalar.from_value(x), from_dense / from_coo, resize, del A[i, j], isequal, assert_array_equal and
the `pytest.raises` blocks) records what each line states.  Nothing of the reference is imported or
executed; every case records its file:line.

Left out, on purpose:
  * test_vector.py:2561-2563, where a plain `Vector.to_dense(4.5)` upcasts the result: this
    library's `Vector.to_dense` without `out=` / `bitmap=` keeps its result type;
  * test_matrix.py:4195-4196 and test_vector.py:2574-2575, which need sub-array dtypes
    ("INT64[2]").
"""
import ast
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
SKIP = {"graphblas/tests/test_vector.py": set(range(2561, 2564)) | {2574, 2575},
        "graphblas/tests/test_matrix.py": {4195, 4196}}
SOURCES = [("graphblas/tests/test_matrix.py", "test_to_dense_from_dense", None),
           ("graphblas/tests/test_vector.py", "test_to_dense_from_dense", None),
           ("graphblas/tests/test_io.py", "test_vector_to_from_numpy", (55, 58)),
           ("graphblas/tests/test_io.py", "test_matrix_to_from_numpy", (101, 104))]


def function(tree, name):
    for node in ast.walk(tree):
        if isinstance(node, ast.FunctionDef) and node.name == name:
            return node
    raise KeyError(name)


def dotted(node):
    """'np.testing.assert_array_equal' of an attribute chain, None for anything else"""
    parts = []
    while isinstance(node, ast.Attribute):
        parts.append(node.attr)
        node = node.value
    if not isinstance(node, ast.Name):
        return None
    return ".".join([node.id] + parts[::-1])


def arange(n, shape=None):
    flat = list(range(n))
    if shape is None:
        return flat
    assert len(shape) in (2, 3)

    def cut(xs, dims):
        if len(dims) == 1:
            return xs
        step = len(xs) // dims[0]
        return [cut(xs[i * step:(i + 1) * step], dims[1:]) for i in range(dims[0])]

    return cut(flat, list(shape))


class Reader:
    def __init__(self, rel):
        self.rel, self.env, self.cases = rel, {}, []

    def src(self, node):
        return f"{self.rel}:{node.lineno}"

    # ------------------------------------------------------------------ expressions
    def value(self, node):
        """a literal, an array expression, a named array, a Scalar or a Python type"""
        if isinstance(node, ast.Name):
            if node.id in ("int", "float"):
                return {"type": node.id}
            return self.env[node.id]["array"]
        if isinstance(node, ast.Call):
            name = dotted(node.func)
            if name == "object":
                return {"object": True}
            if name == "Scalar.from_value":
                return {"scalar": ast.literal_eval(node.args[0])}
            if name == "np.arange":
                return arange(ast.literal_eval(node.args[0]))
            if name == "np.array":
                return ast.literal_eval(node.args[0])
            if isinstance(node.func, ast.Attribute) and node.func.attr == "reshape":
                inner = node.func.value
                assert dotted(inner.func) == "np.arange"
                return arange(ast.literal_eval(inner.args[0]), [ast.literal_eval(a) for a in node.args])
        return ast.literal_eval(node)

    def arguments(self, call):
        return ([self.value(a) for a in call.args],
                {k.arg: (ast.literal_eval(k.value) if isinstance(k.value, ast.Constant) else self.value(k.value))
                 for k in call.keywords})

    def constructor(self, call):
        """{"kind", "how", "args", "kwargs", "steps"} of a Matrix / Vector .from_dense / .from_coo call, else None"""
        name = dotted(call.func) if isinstance(call, ast.Call) else None
        if not name or name.split(".")[-1] not in ("from_dense", "from_coo"):
            return None
        kind, how = name.split(".")[-2:]
        args, kwargs = self.arguments(call)
        return {"kind": kind, "how": how, "args": args, "kwargs": kwargs, "steps": [], "src": self.src(call)}

    def method_call(self, node):
        """(object state, transposed, method, args, kwargs) of `<name>[.T].<method>(...)`"""
        recv, transposed = node.func.value, False
        if isinstance(recv, ast.Attribute) and recv.attr == "T":
            recv, transposed = recv.value, True
        args, kwargs = self.arguments(node)
        return self.env[recv.id], transposed, node.func.attr, args, kwargs

    def snapshot(self, obj):
        return {k: (list(v) if k == "steps" else v) for k, v in obj.items()}

    # ------------------------------------------------------------------ statements
    def statement(self, st):
        if isinstance(st, ast.Assign):
            target = st.targets[0].id
            made = self.constructor(st.value)
            if made is not None:
                self.env[target] = made
            elif isinstance(st.value, ast.Call) and isinstance(st.value.func, ast.Attribute) \
                    and st.value.func.attr == "to_dense":
                obj, transposed, _, args, kwargs = self.method_call(st.value)
                self.env[target] = {"to_dense": (self.snapshot(obj), transposed, args, kwargs), "src": self.src(st)}
            else:
                self.env[target] = {"array": self.value(st.value)}
        elif isinstance(st, ast.Delete):
            sub = st.targets[0]
            self.env[sub.value.id]["steps"].append(["del", list(ast.literal_eval(sub.slice))])
        elif isinstance(st, ast.Assert):
            call = st.test
            assert call.func.attr == "isequal" and ast.literal_eval(call.keywords[0].value) is True
            left, right = self.env[call.func.value.id], call.args[0]
            right = self.constructor(right) or self.env[right.id]
            self.cases.append({"src": self.src(st), "check": "isequal", "left": self.snapshot(left),
                               "right": self.snapshot(right)})
        elif isinstance(st, ast.Expr) and isinstance(st.value, ast.Call):
            call = st.value
            name = dotted(call.func)
            if name and name.endswith("assert_array_equal"):
                self.array_equal(call)
            else:  # A.resize(3, 4)
                assert call.func.attr == "resize"
                self.env[call.func.value.id]["steps"].append(["resize", [ast.literal_eval(a) for a in call.args]])
        elif isinstance(st, ast.With):
            self.raises(st)
        else:
            raise ValueError(f"{self.src(st)}: statement not understood")

    def array_equal(self, call):
        a, b = call.args
        if isinstance(a, ast.Call):  # assert_array_equal(A.to_dense(...), expected)
            obj, transposed, method, args, kwargs = self.method_call(a)
            assert method == "to_dense"
            obj, expect, src = self.snapshot(obj), self.value(b), self.src(call)
        else:  # a2 = v.to_dense(0) ... assert_array_equal(a, a2)
            (obj, transposed, args, kwargs), src = self.env[b.id]["to_dense"], self.env[b.id]["src"]
            expect = self.value(a)
        self.cases.append({"src": src, "check": "to_dense", "of": obj, "T": transposed, "args": args,
                           "kwargs": kwargs, "expect": expect})

    def raises(self, st):
        ctx = st.items[0].context_expr
        assert dotted(ctx.func) == "pytest.raises" and len(st.body) == 1
        call = st.body[0].value
        case = {"src": self.src(st), "check": "raises", "raises": ctx.args[0].id,
                "match": ast.literal_eval(ctx.keywords[0].value)}
        made = self.constructor(call)
        if made is not None:
            case.update(kind=made["kind"], method=made["how"], args=made["args"], kwargs=made["kwargs"])
        else:
            obj, transposed, method, args, kwargs = self.method_call(call)
            case.update(kind=obj["kind"], method=method, of=self.snapshot(obj), args=args, kwargs=kwargs)
        self.cases.append(case)


def main(root):
    cases = []
    for rel, name, lines in SOURCES:
        with open(os.path.join(root, rel)) as f:
            fn = function(ast.parse(f.read()), name)
        reader = Reader(rel)
        for st in fn.body:
            last = getattr(st, "end_lineno", st.lineno)
            if lines is not None and not (lines[0] <= st.lineno and last <= lines[1]):
                if st.lineno < lines[0] and isinstance(st, ast.Assign) and isinstance(st.value, ast.Call) \
                        and dotted(st.value.func) == "np.array":
                    reader.statement(st)  # the array the lines in range speak of
                continue
            if SKIP.get(rel, set()) & set(range(st.lineno, last + 1)):
                continue
            reader.statement(st)
        cases.extend(reader.cases)
    out = os.path.join(HERE, "dense_io_golden.json")
    with open(out, "w") as f:
        json.dump({"generator": "tests/golden/make_dense_io_golden.py", "cases": cases}, f, indent=1)
        f.write("\n")
    print(f"{len(cases)} cases -> {out}")


if __name__ == "__main__":
    main(sys.argv[1])
