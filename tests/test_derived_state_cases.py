"""The probe objects and tables of derived_state_cases.py checked without a GPU: the stated
properties of the graphs, that every mutator's model change is real (or a declared no-op) and
keeps the probe's preconditions, that READS names every derived field of csrc/gb_internal.h, and
that each build counter appears exactly once in csrc."""
import os
import re

import numpy as np
import pytest

import dense_model as dm
import derived_state_cases as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "graph-python_amd", "csrc")


@pytest.mark.parametrize("name", ["G", "G2", "Gs", "G2s"])
def test_graph_properties(name):
    m = dc.make(name)
    p = m.pv[0]
    n = p.shape[0]
    assert p.shape == (n, n) and n == (dc.N_SMALL if name.endswith("s") else dc.N)
    assert n % 64 and (n + 63) // 64 == 11  # a tail word; N and N_SMALL share the word count
    assert m.dtype == "BOOL" and m.iso and np.array_equal(p, m.pv[1]) and np.array_equal(p, p.T)
    deg = p.sum(1)
    for r in dc.EMPTY_ROWS + (n - 1,):
        assert deg[r] == 0, r
    words = np.add.reduceat(deg, np.arange(0, n, 64))
    assert (words == 0).sum() >= 1 and words[-1] > 0  # a whole word without entries; the tail has some
    assert deg.max() > max(dc.SPMV_LONG, dc.PUSH_HEAVY) and (deg > dc.SPMV_LONG).sum() == 1
    if name in ("G", "Gs"):
        assert deg[dc.HUB] == deg.max() == dc.HUB_DEG
    for k in (3, 4, 5):  # the head / walk boundary of k_pull_head
        assert (deg == k).sum() >= 3, (k, int((deg == k).sum()))
    lev, counts = dc.ref_bfs(p, dc.SRC)
    assert deg[dc.SRC] > 0 and len(counts) >= 4 and lev.max() >= 4
    assert np.count_nonzero(lev) == np.count_nonzero(deg)  # connected but for the empty rows


def test_weighted_copies():
    g = dc.make("G").pv[0]
    for name, dtype, lo, hi in (("W", "INT64", 1, 255), ("Wu", "INT64", -100, 100), ("F", "FP64", 1, 4),
                                ("Gi", "INT64", 1, 1)):
        m = dc.make(name)
        assert m.dtype == dtype and np.array_equal(m.pv[0], g)
        v = m.pv[1][g]
        assert v.min() >= lo and v.max() <= hi and np.array_equal(v, np.round(v))
        assert not m.pv[1][~g].any()
    w, wu = dc.make("W").pv[1][g], dc.make("Wu").pv[1][g]
    assert w.min() >= 0 and w.max() > 127      # one byte, unsigned only
    assert wu.min() < 0 and wu.min() >= -128 and wu.max() <= 127  # one byte, signed
    # exact sums: the largest plus_times sum stays far below 2^53
    f = dc.make("F").pv[1]
    assert np.abs(f).sum(1).max() * 5 < 2 ** 40
    assert len(np.unique(dc.make("F").pv[1][g])) > 1 and len(np.unique(w)) > 100


class _Recorder:
    """stands in for the device object: the mutators' model half runs without a GPU"""

    def __getattr__(self, k):
        return _Recorder()

    def __call__(self, *a, **k):
        return _Recorder()

    def __getitem__(self, k):
        return _Recorder()

    def __setitem__(self, k, v):
        pass

    def __delitem__(self, k):
        pass

    def __lshift__(self, o):
        return None

    def __iter__(self):  # ss.split(...) unpacks into two rows of two tiles
        return iter([(_Recorder(), _Recorder()), (_Recorder(), _Recorder())])


def _mutated(mutator, base):
    m = dc.start_model(base, mutator)
    before = m.copy()
    dc.MUTATORS[mutator].fn(_Recorder(), _Recorder(), m)
    return before, m


def test_every_pair_is_listed_once_and_has_a_base():
    assert len(set(dc.PAIRS)) == len(dc.PAIRS)
    for p in dc.PROBES:
        assert sum(1 for q, _, _ in dc.PAIRS if q == p) >= 10, p
    for x in dc.MUTATORS:
        assert any(y == x for _, y, _ in dc.PAIRS), x
    for p, x, b in dc.PAIRS + dc.CAPPED_PAIRS:
        assert b in dc.PROBES[p].bases and b in dc.MUTATORS[x].bases
    assert {p for p, _, _ in dc.CAPPED_PAIRS} == {"heads", "hubs", "long", "narrow"}
    assert {x for _, x, _ in dc.CAPPED_PAIRS} == {"set_row64", "set_row0"}


@pytest.mark.parametrize("mutator,base", sorted({(x, b) for _, x, b in dc.PAIRS}))
def test_mutator_changes_the_model(mutator, base):
    before, after = _mutated(mutator, base)
    X = dc.MUTATORS[mutator]
    changed = not (np.array_equal(before.pv[0], after.pv[0]) and np.array_equal(before.pv[1], after.pv[1]))
    assert changed == X.changes, mutator
    assert after.pv[0].dtype == bool and after.pv[1].dtype == dm.NP[after.dtype]
    assert not after.pv[1][~after.pv[0]].any()  # the model convention: zero where absent
    for p, x, b in dc.PAIRS:
        if (x, b) == (mutator, base):
            assert dc.PROBES[p].ok_for(before) and dc.PROBES[p].ok_for(after), (p, mutator)


def test_intended_boundaries():
    _, m = _mutated("remove_hub", "G")
    assert m.pv[0][dc.HUB].sum() == dc.SPMV_LONG  # exactly at the long-row threshold: no longer long
    _, m = _mutated("remove_row", "G")
    assert not m.pv[0][1].any() and not m.pv[0][:, 1].any()
    for name, first in (("set_row64", 64), ("set_row0", 0)):
        before, m = _mutated(name, "G")
        ne0, ne1 = before.pv[0].any(1), m.pv[0].any(1)
        assert not ne0[first] and ne1[first]
        assert (np.cumsum(ne1) - np.cumsum(ne0))[first:].min() == 1  # every later rank shifts
    _, m = _mutated("overwrite_wide", "W")
    assert m.pv[1].max() == 70000
    _, m = _mutated("overwrite_negative", "W")
    assert m.pv[1].min() == -3
    _, m = _mutated("set_other_iso", "Gi")
    assert len(np.unique(m.pv[1][m.pv[0]])) == 2
    for name in ("transpose_self", "ewise_add_self"):  # nothing but the write-back changes A
        before, m = _mutated(name, "G")
        assert before.pv[0][64, dc.N - 3] and not before.pv[0][dc.N - 3, 64] and m.pv[0][dc.N - 3, 64]
    deg = dc.make("G").pv[0].sum(1)
    assert (deg > dc.CW_HUB).sum() == 1 and deg.max() < 512  # a hub of the column-word tables only at CW_HUB
    assert {(p, b) for p, x, b in dc.PAIRS if x == "overwrite_wide"} >= {("narrow", "W"), ("narrow", "Wu")}


def test_vector_mutators_change_the_model():
    for start in dc.VSTARTS:
        for name, fn in dc.VMUTATORS.items():
            if name == "bitmap_import":
                continue  # needs device memory
            m = dc.VModel(dc.full_vec() if start == "full" else dc.empty_vec("FP64"), "FP64")
            before = m.pv[0].copy(), m.pv[1].copy()
            fn(_Recorder(), _Recorder(), m)
            assert m.pv[0].shape == (dc.NV,)
            changed = not (np.array_equal(before[0], m.pv[0]) and np.array_equal(before[1], m.pv[1]))
            assert changed or (start, name) in (("empty", "clear"), ("empty", "remove")), (start, name)
            # full -> not full and empty -> not empty are both exercised
            if start == "full" and name in ("remove", "clear", "resize", "expr"):
                assert not m.pv[0].all()
            if start == "empty" and name != "clear" and name != "remove":
                assert m.pv[0].any()


# ---------------------------------------------------------------------- the field guard
def _struct_body(text, name):
    k = re.search(r"struct\s+" + name + r"\s*\{", text)
    assert k, name
    depth, i = 1, k.end()
    while depth:
        depth += {"{": 1, "}": -1}.get(text[i], 0)
        i += 1
    return text[k.end():i - 1]


def _fields(body):
    """names of the members declared in a struct body (comments stripped; `a, b = 0, *c;` too)"""
    body = re.sub(r"//[^\n]*", "", body)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl or "(" in decl.split("=")[0]:
            continue
        k = re.match(r"(?:const\s+)?(?:struct\s+)?[\w:]+(?:\s+const)?\s*(.*)$", decl, re.S)
        for part in re.split(r",(?![^\[]*\])", k.group(1)):
            name = re.match(r"\s*\**\s*(\w+)", part)
            if name:
                out.append(name.group(1))
    return out


def test_every_derived_field_has_a_probe():
    with open(os.path.join(CSRC, "gb_internal.h")) as f:
        text = f.read()
    cache = _fields(_struct_body(text, "gb_orient_cache"))
    assert {"hub_tab", "hub_n", "hub_H", "rows_ne", "ne_rank", "phead", "pdeg", "maxdeg", "long_tab",
            "nar_done"} <= set(cache)  # the parser finds the members of multi-name declarations
    obj = _fields(_struct_body(text, "GB_Matrix_opaque"))
    assert {"rowptr", "t_perm", "oc", "pub_seq", "pub_epoch", "cw_stat", "invalid"} <= set(obj)
    # of the object itself: everything but its identity, its CSR / bitmap storage and its error state
    primary = {"magic", "kind", "type", "nrows", "ncols", "iso", "nvals", "rowptr", "colidx", "vals", "oc",
               "bits", "dense", "err", "invalid"}
    derived = cache + [x for x in obj if x not in primary]
    missing = [x for x in derived if x not in dc.READS]
    assert not missing, f"derived fields without a probe in READS: {missing}"
    stale = [x for x in dc.READS if x not in derived]
    assert not stale, f"READS names fields that are gone: {stale}"
    assert set(dc.READS.values()) <= set(dc.PROBES) | {"vector"}
    assert set(dc.PROBES) <= set(dc.READS.values())  # no probe without a field


def test_each_counter_appears_once_in_csrc():
    text = ""
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".hip", ".cpp", ".cuh", ".h")):
            with open(os.path.join(CSRC, name)) as f:
                text += f.read()
    for c in dc.COUNTERS + ("transposes_cached",):
        assert len(re.findall(r'gb_stat_add\("' + c + r'"', text)) == 1, c
    for p in dc.PROBES.values():
        assert set(p.counters) <= set(dc.COUNTERS + ("transposes_cached",))
