"""Connectivity classes, the CPU restatement (probe.PlaneCells.classes / cells_at, probe.Table.classes /
render_class_table): a 4-pod table worked out by hand; config #1 from the oracle's planes against the rows and columns
of the README table fixture; the defining property (the class table plus the two index arrays give back every cell, and
no two representatives behave alike) on a generated 130-pod problem; and the rendering."""
import json
import os

import numpy as np
import pytest

from classgen import VIEWS, ClassProblem
from cyclonus_amd import _lib
from cyclonus_amd._lib import CyclonusError
from cyclonus_amd.probe import PlaneCells, Pod, Resources, Table, new_probe_config
from oracle.oracle import Oracle

GOLD = os.path.join(os.path.dirname(__file__), "golden")
V, NJ, BNP, BPP = _lib.JOB_VALID, _lib.JOB_NONE, _lib.JOB_BAD_NAMED_PORT, _lib.JOB_BAD_PORT_PROTOCOL


def _planes(status, ingress, egress):
    """status [P][K]; ingress[d][k] and egress[s][k] as lists of set bits -> PlaneCells (one word per row)."""
    word = lambda bits: np.uint64(sum(1 << b for b in bits))  # noqa: E731
    to_plane = lambda rows: np.array([[[word(bits)] for bits in row] for row in rows], np.uint64)  # noqa: E731
    return PlaneCells(np.array(status, np.uint8), to_plane(ingress), to_plane(egress))


def test_four_pods_by_hand():
    """One slot.  Ingress rows (who may enter d): d0 {0,1,2,3}, d1 {0,1,2,3}, d2 {0,1}, d3 anything (BAD_NAMED_PORT).
    Egress rows (where s may go): s0 {0,1,2,3}, s1 {0,1,2,3}, s2 {0,1}, s3 {0,1}; bit 9 (beyond P) set for s1 only.
      Ingress codes, row s: s0 = s1 = [. . . P], s2 = s3 = [. . X P]        -> sources {0,1} {2,3}
      Egress codes:         s0 = s1 = [. . . ?], s2 = s3 = [. . X ?]        -> sources {0,1} {2,3}
      Combined:             s0 = s1 = [. . . P], s2 = s3 = [. . X P]        -> sources {0,1} {2,3}
      columns: d0 = d1 everywhere; d2 differs from them; d3 is the invalid one -> destinations {0,1} {2} {3}"""
    c = _planes([[V], [V], [V], [BNP]], [[[0, 1, 2, 3]], [[0, 1, 2, 3]], [[0, 1]], [[0, 2, 3]]],
                [[[0, 1, 2, 3]], [[0, 1, 2, 3, 9]], [[0, 1]], [[0, 1]]])
    for view in VIEWS + (_lib.VIEW_COMBINED,):
        got = c.classes(view)
        assert got["src"].tolist() == [0, 0, 1, 1] and got["n_src"] == 2, view
        assert got["dst"].tolist() == [0, 0, 1, 2] and got["n_dst"] == 3, view
        assert got["src"].dtype == np.int32 and got["dst"].dtype == np.int32
    # egress view alone sees s2's way to d2 once the ingress side closes it for nobody: open d2's ingress to all
    c = _planes([[V], [V], [V], [BNP]], [[[0, 1, 2, 3]], [[0, 1, 2, 3]], [[0, 1, 2, 3]], [[]]],
                [[[0, 1, 2, 3]], [[0, 1, 2, 3]], [[0, 1]], [[0]]])
    assert c.classes("ingress")["src"].tolist() == [0, 0, 0, 0]
    assert c.classes("ingress")["dst"].tolist() == [0, 0, 0, 1]
    assert c.classes("egress")["src"].tolist() == [0, 0, 1, 2]
    assert c.classes("combined")["src"].tolist() == [0, 0, 1, 2]
    assert c.classes("egress")["dst"].tolist() == [0, 1, 2, 3]  # (columns [. . . .], [. . . X], [. . X X], [? ? ? ?])
    # each side alone; the empty slot range; a bad view and slot range
    assert set(c.classes("egress", want=("dst",))) == {"dst", "n_dst"}
    got = c.classes("egress", 0, 0)
    assert got["src"].tolist() == [0] * 4 and got["dst"].tolist() == [0] * 4 and (got["n_src"], got["n_dst"]) == (1, 1)
    with pytest.raises(CyclonusError, match="unknown view"):
        c.classes(3)
    with pytest.raises(CyclonusError, match="slot range out of bounds"):
        c.classes("egress", 0, 2)
    none = PlaneCells(np.zeros((0, 1), np.uint8), np.zeros((0, 1, 0), np.uint64), np.zeros((0, 1, 0), np.uint64)).classes()
    assert (none["n_src"], none["n_dst"], len(none["src"])) == (0, 0, 0)


def test_statuses_separate_destinations_only():
    """Two slots, every plane bit set.  Destinations: d0 [VALID, NONE], d1 [VALID, BNP], d2 [VALID, BPP], d3 [VALID, BNP]:
    the sources never split; under Ingress and Combined the destinations are {0} {1,3} {2}, under Egress {0} {1,2,3}."""
    full = [[[0, 1, 2, 3]] * 2] * 4
    c = _planes([[V, NJ], [V, BNP], [V, BPP], [V, BNP]], full, full)
    for view in VIEWS:
        got = c.classes(view)
        assert got["src"].tolist() == [0, 0, 0, 0]
        assert got["dst"].tolist() == ([0, 1, 1, 1] if view == "egress" else [0, 1, 2, 1]), view
        assert c.classes(view, 0, 1)["dst"].tolist() == [0, 0, 0, 0]


def _config1():
    c = json.load(open(os.path.join(GOLD, "config1.json")))
    status, inp, egp = Oracle(c["policies"], c["resources"]).probe(c["probes"])
    return c, Resources.from_json(c["resources"]), PlaneCells(status, inp, egp)


def test_config1_classes_are_the_equal_rows_of_the_readme_table():
    c, res, cells = _config1()
    fix = c["readme_combined_tcp80"]
    names = [p.pod_string() for p in res.pods]
    row = {n: "".join(fix["rows"][n][h] for h in fix["header"]) for n in names}
    col = {n: "".join(fix["rows"][s][n.upper()] for s in sorted(names)) for n in names}
    got = cells.classes("combined", 0, 1)
    assert 1 < got["n_src"] < len(names) and 1 < got["n_dst"] < len(names)
    for i, p in enumerate(names):
        for j, q in enumerate(names):
            assert (got["src"][i] == got["src"][j]) == (row[p] == row[q]), (p, q)
            assert (got["dst"][i] == got["dst"][j]) == (col[p] == col[q]), (p, q)


def _property(cells_at, cells, classes, ctx):
    """The class table and the two index arrays are the table: cells_at(reps, reps)[src_class[s], dst_class[d]] ==
    cells[s, d] for every cell, and no two representative rows and no two representative columns are equal."""
    src, dst = classes["src"], classes["dst"]
    reps_s = [int(np.nonzero(src == x)[0][0]) for x in range(classes["n_src"])]
    reps_d = [int(np.nonzero(dst == x)[0][0]) for x in range(classes["n_dst"])]
    table = cells_at(reps_s, reps_d)
    assert table.shape[:2] == (len(reps_s), len(reps_d)), ctx
    assert np.array_equal(table[src][:, dst], cells), f"{ctx}: the class table does not give the cells back"
    assert len({table[i].tobytes() for i in range(len(reps_s))}) == len(reps_s), f"{ctx}: two source classes with equal rows"
    assert len({table[:, j].tobytes() for j in range(len(reps_d))}) == len(reps_d), f"{ctx}: two destination classes with equal columns"


@pytest.mark.parametrize("view", VIEWS)
def test_defining_property_on_a_generated_problem(view):
    P, K = 130, 3
    g = ClassProblem(P, K, 14)
    cells = g.cells()
    for k_lo, k_hi in ((0, 3), (1, 2)):
        got = cells.classes(view, k_lo, k_hi)
        all_cells = cells.cells(0, P, 0, P, k_lo, k_hi, want=(view,))[view]
        _property(lambda s, d: cells.cells_at(s, d, k_lo, k_hi, want=(view,))[view], all_cells, got, f"{view} [{k_lo}, {k_hi})")


def test_cells_at_is_fancy_indexing():
    g = ClassProblem(65, 2, 12)
    cells = g.cells()
    whole = cells.cells(0, 65, 0, 65, 0, 2)
    s, d = [64, 0, 0, 7], [3, 64, 3]
    got = cells.cells_at(s, d)
    for n in ("ingress", "egress", "combined"):
        assert got[n].shape == (4, 3, 2) and got[n].dtype == np.uint8
        assert np.array_equal(got[n], whole[n][s][:, d])
    assert cells.cells_at([], d, want=("egress",))["egress"].shape == (0, 3, 2)
    assert cells.cells_at(s, [5], 1, 2, want=("egress",))["egress"].shape == (4, 1, 1)
    with pytest.raises(CyclonusError, match=r"dsts\[1\] = 65 is not a pod in \[0, 65\)"):
        cells.cells_at(s, [0, 65])
    with pytest.raises(CyclonusError, match=r"srcs\[0\] = -1 is not a pod"):
        cells.cells_at([-1], d)


def test_table_classes_and_class_table_on_config1():
    c, res, cells = _config1()
    t = Table(res, new_probe_config(80, "TCP"), cells, 0, 1)
    got = t.classes()
    names = [p.pod_string() for p in res.pods]
    for side in ("sources", "destinations"):
        assert sorted(n for cl in got[side] for n in cl) == sorted(names)
        assert [cl[0] for cl in got[side]] == sorted((cl[0] for cl in got[side]), key=names.index)  # classes by first pod
        assert all(cl == sorted(cl, key=names.index) for cl in got[side])  # members in plane order
    idx = cells.classes("combined", 0, 1)
    assert [[names.index(n) for n in cl] for cl in got["sources"]] == [np.nonzero(idx["src"] == x)[0].tolist() for x in range(idx["n_src"])]
    text = t.render_class_table()
    lines = text.splitlines()
    fix = c["readme_combined_tcp80"]
    label = lambda cl: cl[0] + (f" (+{len(cl) - 1})" if len(cl) > 1 else "")  # noqa: E731
    split = lambda ln: [x.strip() for x in ln.strip("|").split("|")]  # noqa: E731
    # a column per destination class and a row per source class, each labelled by its first pod and the number of its
    # other members; the cells are the README table's cells of the first pods
    assert lines[0] == lines[2] == lines[-1] and set(lines[0]) == {"+", "-"}
    assert split(lines[1]) == [""] + [label(cl).upper() for cl in got["destinations"]]
    rows = lines[3:-1]
    assert len(rows) == len(got["sources"]) < len(names)
    for ln, cl in zip(rows, got["sources"]):
        assert split(ln) == [label(cl)] + [fix["rows"][cl[0]][dc[0].upper()] for dc in got["destinations"]]
    assert any("(+" in ln for ln in rows)
    with pytest.raises(ValueError, match="invalid view"):
        t.classes("both")
    # several slots: a line per slot in every cell, "-" where a pod has no job
    t3 = Table(res, new_probe_config(80, "TCP"), cells, 0, cells.status.shape[1])
    assert t3.render_class_table("ingress").count("\n") > text.count("\n")


def test_class_table_of_singleton_classes_is_the_table():
    """Every pod its own class as a source and as a destination, one slot, pods in sorted order: the class table is
    render_table() byte for byte."""
    res = Resources({"x": {}}, [Pod("x", n, {}, f"10.0.0.{i}", []) for i, n in enumerate("abc")])
    cells = _planes([[V], [V], [V]], [[[0]], [[0, 1]], [[0, 1, 2]]], [[[0, 1, 2]], [[1, 2]], [[2]]])
    t = Table(res, new_probe_config(80, "TCP"), cells, 0, 1)
    got = t.classes()
    assert got["sources"] == [["x/a"], ["x/b"], ["x/c"]] and got["destinations"] == got["sources"]
    assert t.render_class_table() == t.render_table()
    assert t.render_class_table("ingress") == t.render_ingress() and t.render_class_table("egress") == t.render_egress()
