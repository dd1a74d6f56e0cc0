"""Results depend on an object's content, not on how it is stored.

Part A: every consumer of representation_cases.CONSUMERS on a vector whose don't-care slots (the
elements of the value array under a clear bit, which no producer writes) hold 0x5a, then 0xff,
in every byte: the result is the dense model's, computed from the content alone, and the two
results are equal bit for bit.  The same consumer runs on clean storage first, so a wrong
expectation reads differently from a dependence on the slots; a case that poisoned no slot fails.

Part B: every producer of representation_cases.PRODUCERS hands its output, as it was left, to a
fixed battery of consumers, a freshly produced one per call, next to R = from_coo(*P.to_coo()):
the two results are equal bit for bit.  P's own to_coo() is checked against its model first.
A sparse non-iso vector output goes through the battery once more with its slots poisoned.

The level loop's deferrals (a pending root, a deferred stamp, a speculated level) are global
records that the library carries out at the first call that does not continue the loop, so no
battery can hold one: test_live_deferral_meets_its_consumer builds every operand and expectation
first, creates the deferral, checks that it is live ("stat_deferred_live"), and makes the one
consuming call.

Every comparison is exact.  The case counts and the file's run time are printed at the end of
the module (pytest -s).  The file's 970 tests take 21.5 s on an MI355X, the slowest 0.42 s."""
import re
import time

import numpy as np
import pytest

import dense_model as dm
import representation_cases as rc

pytestmark = pytest.mark.gpu

_COUNT = {"poisoned vectors": 0, "slots written": 0, "battery calls": 0, "poisoned battery calls": 0}


@pytest.fixture(scope="module")
def gb():
    import graphblas_amd

    t0 = time.perf_counter()
    yield graphblas_amd
    print(f"\ntest_representation_gpu.py: {time.perf_counter() - t0:.1f} s; "
          + ", ".join(f"{v} {k}" for k, v in _COUNT.items()))


# ---------------------------------------------------------------------- part A
A_CASES = [(c.name, dt, n) for c in rc.CONSUMERS.values() for dt in c.types for n in rc.SIZES]


@pytest.mark.parametrize("name,dt,n", A_CASES, ids=[f"{a}-{b}-{c}" for a, b, c in A_CASES])
def test_poisoned_slots(gb, name, dt, n):
    C = rc.CONSUMERS[name]
    got, exp = C.fn(rc.Case(gb, n, dt, None))
    diff = rc.same(got, exp)
    assert diff is None, f"{name} on clean storage differs from the model: {diff}"
    results = []
    for pattern in rc.PATTERNS:
        case = rc.Case(gb, n, dt, pattern)
        got, exp = C.fn(case)
        assert case.written and min(case.written) > 0, f"{name}: a vector with no poisoned slot"
        _COUNT["poisoned vectors"] += len(case.written)
        _COUNT["slots written"] += sum(case.written)
        diff = rc.same(got, exp)
        assert diff is None, f"{name} with 0x{pattern:02x} in the don't-care slots differs from the model: {diff}"
        results.append(got)
    diff = rc.same(results[0], results[1])
    assert diff is None, f"{name}: the results under 0x5a and 0xff differ: {diff}"


_ALL_T = "(" + "|".join(dm.ALL) + ")"
# called through ctypes directly, not through base.call: the recorder does not see them
_UNRECORDED = {"GrB_Vector_nvals", "GrB_Vector_extractTuples_T", "GrB_Vector_extractElement_T",
               "GxB_Vector_bitmap_export", "GxB_Vector_bitmap_import"}


@pytest.mark.parametrize("name", list(rc.CONSUMERS))
def test_consumer_calls_its_entry_points(gb, name):
    """the table's claim, checked against the recorder: the consumer reaches the entry points its
    row names (the table test counts on that)"""
    C = rc.CONSUMERS[name]
    dt = "INT32"
    with gb.Recorder() as rec:
        C.fn(rc.Case(gb, 65, dt, None))
    text = "\n".join(rec.data)
    for e in C.entries:
        if e in _UNRECORDED:
            continue
        pat = (re.escape(e[:-2]) + "_" + _ALL_T if e.endswith("_T") else re.escape(e)) + r"\("
        assert re.search(r"(^|\n)" + pat, text), f"{name} never called {e}"


# ---------------------------------------------------------------------- part B
B_CASES = [(p.name, dt) for p in rc.PRODUCERS.values() for dt in p.types]
_UNRECORDED_B = {"GxB_Matrix_prepare_transpose", "GxB_Vector_device_touch", "GxB_Vector_bitmap_import"}


@pytest.mark.parametrize("name", list(rc.PRODUCERS))
def test_producer_calls_its_entry_points(gb, name):
    P = rc.PRODUCERS[name]
    with gb.Recorder() as rec:
        P.fn(gb, P.types[0])
    text = "\n".join(rec.data)
    for e in P.entries:
        if e in _UNRECORDED_B:
            continue
        pat = (re.escape(e[:-2]) + "_" + _ALL_T if e.endswith("_T") else re.escape(e)) + r"\("
        assert re.search(r"(^|\n)" + pat, text), f"{name} never called {e}"


def _coo(X):
    return rc.vc(X) if X.ndim == 1 else rc.mc(X)


def _model_coo(m):
    return rc.mvc(m) if m[0].ndim == 1 else rc.mmc(m)


def _battery(gb, P, name, dt, fresh, pattern=None):
    battery = rc.VECTOR_BATTERY if P.ndim == 1 else rc.MATRIX_BATTERY
    for bname, fn in battery.items():
        R = rc.rebuilt(gb, fresh())
        X = fresh()  # produced last: it reaches the consumer straight from its producer
        if pattern is not None:
            rc.poison(X, pattern)
            _COUNT["poisoned battery calls"] += 1
        a, b = fn(gb, X, dt), fn(gb, R, dt)
        _COUNT["battery calls"] += 1
        diff = rc.same(a, b)
        how = "" if pattern is None else f" (slots poisoned with 0x{pattern:02x})"
        assert diff is None, f"{bname} of the output of {name}{how} differs from that of a rebuilt copy: {diff}"
    R = rc.rebuilt(gb, fresh())
    X = fresh()
    if pattern is not None:
        rc.poison(X, pattern)
    assert X.isequal(R) is True and R.isequal(X) is True, f"isequal of the output of {name} and a rebuilt copy"
    assert X.isequal(R, check_dtype=True) is True


@pytest.mark.parametrize("name,dt", B_CASES, ids=[f"{a}-{b}" for a, b in B_CASES])
def test_producer_output_as_it_was_left(gb, name, dt):
    P = rc.PRODUCERS[name]

    def fresh():
        return P.fn(gb, dt)[0]

    X, model = P.fn(gb, dt)
    assert X.dtype.name == rc.dm.name_of(model[1].dtype), f"{name}: dtype {X.dtype.name}"
    assert tuple(X.shape) == model[0].shape, f"{name}: shape {X.shape}"
    diff = rc.same(_coo(X), _model_coo(model))
    assert diff is None, f"the output of {name} differs from its model: {diff}"
    assert X.nvals == int(model[0].sum())
    xdt = X.dtype.name
    _battery(gb, X, name, xdt, fresh)
    if X.ndim == 1:
        from graphblas_amd import device as gdev

        Y = fresh()
        view = gdev.vector_view(Y._h)
        if not view.iso and view.values and 0 < view.nvals < view.nrows:
            for pattern in rc.PATTERNS:
                _battery(gb, X, name, xdt, fresh, pattern)


def test_the_interesting_forms_are_reached(gb):
    """what makes a producer's output differ from a build is really there, where the library
    shows it: iso set by the producer, the column-word mxm (it builds the operand's two hub
    tables), an iso frontier whose count came through the mailbox and not through a device copy,
    vector outputs with clear bits and a value array"""
    from graphblas_amd import device as gdev

    C = rc.PRODUCERS["mxm_any_pair"].fn(gb, "INT32")[0]
    assert gdev.matrix_view(C._h).iso == 1
    for name in ("mxm_colbits", "colbits_stamp"):
        built = gb.get_knob("stat_hub_tables_built")
        Q = rc.PRODUCERS[name].fn(gb, rc.PRODUCERS[name].types[0])[0]
        assert gb.get_knob("stat_hub_tables_built") - built == 2, name
    copies = gb.get_knob("stat_nvals_copy")
    q = rc.PRODUCERS["vxm_iso_bfs"].fn(gb, "BOOL")[0]
    assert gb.get_knob("stat_nvals_copy") == copies  # nobody has read q's count from the device
    assert gdev.vector_view(q._h).iso == 1
    sparse = 0
    for name, dt in B_CASES:
        X = rc.PRODUCERS[name].fn(gb, dt)[0]
        if X.ndim == 1:
            v = gdev.vector_view(X._h)
            sparse += bool(not v.iso and v.values and 0 < v.nvals < v.nrows)
    assert sparse >= 30, sparse


# ---------------------------------------------------------------------- live deferrals
SPEC, ROOT, STAMP = 1, 2, 4  # the bits of "stat_deferred_live"
N = rc.dc.N


def _live(gb):
    return gb.get_knob("stat_deferred_live")


class _Loop:
    """every operand, output and expectation of the consumers below, built before anything is
    deferred; start() then leaves the chosen deferrals live"""

    def __init__(self, gb):
        self.gb = gb
        self.Gm = rc.dc.make("G")
        self.G = rc.dc.to_gb(gb, self.Gm)
        self.Fi = rc.mat_model(40, N, "INT32", seed=61, density=0.05)
        self.Fb = rc.mat_model(40, N, "BOOL", seed=62, density=0.05)
        self.A2 = rc.mat_model(N, 50, "INT32", seed=5, density=0.1)
        self.u2 = rc.other_model(50, "INT32", seed=8)
        self.w0 = rc.other_model(N, "INT32", seed=9)
        self.T = dm.mxv("plus", "times", "INT32", self.A2, self.u2)
        self.fi, self.fb, self.a2 = rc.gmat(gb, self.Fi, "INT32"), rc.gmat(gb, self.Fb, "BOOL"), rc.gmat(gb, self.A2, "INT32")
        self.gu2, self.wN = rc.gvec(gb, self.u2, "INT32"), rc.gvec(gb, self.w0, "INT32")
        self.w40, self.wb40 = gb.Vector("INT32", 40), gb.Vector(bool, 40)
        self.pt, self.ap = gb.semiring.plus_times["INT32"], gb.semiring.any_pair["BOOL"]
        self.plus = gb.binary.plus["INT32"]
        self.v, self.q = gb.Vector("INT32", N), gb.Vector(bool, N)

    def start(self, want):
        gb, v, q = self.gb, self.v, self.q
        v[5] = 7
        self.vm = dm.set_element(rc.zero_of(N, "INT32"), 5, np.int32(7))
        front = [rc.dc.SRC] if want & ROOT else [rc.dc.SRC, rc.dc.SRC + 1]
        if want & ROOT:
            q[rc.dc.SRC] = True
        else:
            q.build(front, True)
        self.qm = rc.pv_of(np.isin(np.arange(N), front), True, "BOOL")
        if want & STAMP:  # a root stays pending under its value mask; a built q is not iso: its structure
            v(mask=q.V if want & ROOT else q.S)[:] = 1
            self.vm = dm.assign_vec(self.vm, np.int32(1), mask=self.qm)
        assert _live(gb) == want, f"live deferrals {_live(gb)}, wanted {want}"


def _v_as_u(L):
    L.w40 << L.fi.mxv(L.v, L.pt)
    return L.w40, dm.mxv("plus", "times", "INT32", L.Fi, L.vm)


def _masked(which, kind, replace):
    def fn(L):
        k, km = (L.v, L.vm) if which == "v" else (L.q, L.qm)
        L.wN(rc.mask_of(k, kind), replace=replace) << L.a2.mxv(L.gu2, L.pt)
        return L.wN, dm.write_back(L.w0, L.T, mask=km, replace=replace, **rc.mask_kw(kind))
    return fn


def _v_as_w(L):
    L.v(L.plus) << L.a2.mxv(L.gu2, L.pt)
    L.vm = dm.write_back(L.vm, L.T, accum="plus")
    return L.v, L.vm


def _q_as_u(L):
    L.wb40 << L.fb.mxv(L.q, L.ap)
    return L.wb40, dm.mxv("any", "pair", "BOOL", L.Fb, L.qm)


def _level(L):
    """the loop's own next call: the stamp is fused into its kernel, the root pushed from"""
    L.q(~L.v.S, replace=True) << L.q.vxm(L.G, L.ap)
    nxt = L.Gm.pv[0][L.qm[0]].any(axis=0) & ~L.vm[0]
    L.qm = rc.pv_of(nxt, True, "BOOL")
    return L.q, L.qm


LIVE_CONSUMERS = {"v_as_u": _v_as_u, "v_as_mask_S": _masked("v", "S", False), "v_as_mask_V_replace": _masked("v", "V", True),
                  "v_as_mask_cS_replace": _masked("v", "~S", True), "v_as_w_accum": _v_as_w, "q_as_u": _q_as_u,
                  "q_as_mask_S": _masked("q", "S", False), "q_as_mask_cV_replace": _masked("q", "~V", True),
                  "level": _level}


@pytest.mark.parametrize("want", [ROOT | STAMP, STAMP, ROOT], ids=["root+stamp", "stamp", "root"])
@pytest.mark.parametrize("name", list(LIVE_CONSUMERS))
def test_live_deferral_meets_its_consumer(gb, name, want):
    """GrB_mxv / GrB_vxm are the calls that meet a live deferral (every other call has it carried
    out first): the loop's v or q as their u, mask or output while the root and the stamp are
    pending.  One call of the same shape runs first on objects of its own, so that the call
    under test is the first library call after the deferral."""
    fn = LIVE_CONSUMERS[name]
    warm = _Loop(gb)
    warm.start(0)
    fn(warm)
    L = _Loop(gb)
    L.start(want)
    with gb.Recorder() as rec:
        out, exp = fn(L)
        assert len(rec.data) == 1 and rec.data[0].startswith(("GrB_mxv(", "GrB_vxm(")), rec.data
        assert _live(gb) & (ROOT | STAMP) == 0, "the consuming call left a root or a stamp pending"
    diff = rc.same(_coo(out), _model_coo(exp))
    assert diff is None, f"{name} with deferrals {want} live: {diff}"
    for what, X, m in (("v", L.v, L.vm), ("q", L.q, L.qm)):
        diff = rc.same(_coo(X), _model_coo(m))
        assert diff is None, f"{name} with deferrals {want} live: {what} afterwards: {diff}"
        assert X.nvals == int(m[0].sum())


@pytest.mark.parametrize("name", ["q_nvals", "v_as_u", "v_as_mask_S", "q_as_u", "v_nvals"])
def test_live_speculation_meets_its_consumer(gb, name):
    """after a fused level the next one is speculated: the count of q leaves it live, and v as an
    operand of another product, or the count of v, rolls it back first"""
    L = _Loop(gb)
    L.start(ROOT | STAMP)
    _level(L)
    assert _live(gb) == SPEC, f"after a fused level: {_live(gb)}"
    if name == "q_nvals":
        assert L.q.nvals == int(L.qm[0].sum()) and _live(gb) == SPEC
    elif name == "v_nvals":
        assert L.v.nvals == int(L.vm[0].sum()) and _live(gb) == 0
    else:
        out, exp = LIVE_CONSUMERS[name](L)
        assert _live(gb) == 0
        diff = rc.same(_coo(out), _model_coo(exp))
        assert diff is None, f"{name} with a speculated level live: {diff}"
    for what, X, m in (("v", L.v, L.vm), ("q", L.q, L.qm)):
        diff = rc.same(_coo(X), _model_coo(m))
        assert diff is None, f"{name} with a speculated level live: {what} afterwards: {diff}"
