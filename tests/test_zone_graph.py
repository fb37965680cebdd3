"""The zone graph through the numpy restatement on the CPU (probe.PlaneCells.zone_graph, probe.Table.zone_graph /
render_zone_graph): a 6-pod table worked out by hand, zonegen's closed forms at small P, config #1 from the oracle's
planes, and the defining properties on random digraphs: the cover edges generate the zone reach matrix, none of them can
go, each is witnessed by a pod edge, the tiers rise along them."""
import json
import os

import numpy as np
import pytest

import closuregen as cg
import zonegen as zg
from cyclonus_amd import _lib
from cyclonus_amd._lib import CyclonusError
from cyclonus_amd.probe import PlaneCells, Pod, Resources, Table, new_probe_config
from oracle.oracle import Oracle
from test_closure import _planes

GOLD = os.path.join(os.path.dirname(__file__), "golden")
V = _lib.JOB_VALID
ALL = ("zone", "rep", "size", "tier", "edges", "reach")


def same_as_expected(got, want, ctx):
    """A zone_graph dict (numpy values; "reach" a u64 plane) against zonegen.expected's."""
    assert got["n_zones"] == want["n_zones"] and got["n_edges"] == want["n_edges"], f"{ctx}: {got['n_zones']} zones, {got['n_edges']} edges"
    for x, dt in (("zone", np.int32), ("rep", np.int32), ("size", np.int64), ("tier", np.int32), ("edges", np.int32)):
        if x in got:
            assert got[x].dtype == dt and got[x].shape == want[x].shape, f"{ctx}: {x} {got[x].dtype} {got[x].shape}"
            assert np.array_equal(got[x], want[x]), f"{ctx}: {x} differs at {np.argwhere(got[x] != want[x])[:5].tolist()}"
    if "reach" in got:
        w = zg.pack_zone_plane(want["reach"])
        assert got["reach"].shape == w.shape and np.array_equal(got["reach"], w), f"{ctx}: the zone reach plane"


def _closed(edges, Z):
    m = np.eye(Z, dtype=bool)
    for a, b in edges:
        m[a, b] = True
    for k in range(Z):
        m |= m[:, k:k + 1] & m[k:k + 1, :]
    return m


def defining_properties(cells, k_lo, k_hi, ctx):
    g = cells.zone_graph(k_lo, k_hi, want=ALL)
    Z, zone, edges = g["n_zones"], g["zone"], g["edges"].tolist()
    R = cg.unpack(g["reach"], Z) if Z else np.zeros((0, 0), bool)
    assert g["edges"].tolist() == sorted(edges) and all(a != b for a, b in edges), ctx
    assert np.array_equal(_closed(edges, Z), R), f"{ctx}: the cover edges do not generate the zone reach matrix"
    for i in range(len(edges)):
        assert not np.array_equal(_closed(edges[:i] + edges[i + 1:], Z), R), f"{ctx}: edge {edges[i]} is implied by the others"
    adj = cg.unpack(cells.adjacency("from", k_lo, k_hi), len(zone))
    for a, b in edges:
        assert adj[zone == a][:, zone == b].any(), f"{ctx}: no pod edge behind {a} -> {b}"
    tier = g["tier"]
    assert all(tier[a] < tier[b] for a, b in edges), f"{ctx}: a tier does not rise along an edge"
    entered = np.zeros(Z, bool)
    entered[[b for _, b in edges]] = True
    assert np.array_equal(tier == 0, ~entered), f"{ctx}: tier 0 is not exactly the zones without an incoming edge"
    # and what the other outputs are by definition
    z = cells.zones(k_lo, k_hi, want=("zone",))
    assert np.array_equal(zone, z["zone"]) and Z == z["n_zones"] and g["size"].tolist() == np.bincount(zone, minlength=Z).tolist()
    assert g["rep"].tolist() == [int(np.flatnonzero(zone == x)[0]) for x in range(Z)]
    rows = cg.unpack(cells.closure("from", k_lo, k_hi)["plane"], len(zone))
    assert np.array_equal(R, rows[g["rep"]][:, g["rep"]]), f"{ctx}: the zone reach matrix is not the closure at the zones' first pods"
    return g


TEXT = """tier 0: x/a (+1), x/e
tier 1: x/c (+1)
tier 2: x/f
x/a (+1) -> x/c (+1)
x/c (+1) -> x/f
"""
DOT = """digraph zones {
  z0 [label="x/a (+1)"];
  z1 [label="x/c (+1)"];
  z2 [label="x/e"];
  z3 [label="x/f"];
  { rank=same; z0; z2; }
  { rank=same; z1; }
  { rank=same; z3; }
  z0 -> z1;
  z1 -> z3;
}
"""


def test_six_pods_by_hand():
    """One slot.  Edges: a <-> b, b -> c, c <-> d, d -> f, a -> f, e -> e.  Decoys: f -> a as an egress bit alone (taken for
    an edge it makes one zone of a, b, c, d, f) and bit 9 in d's egress row.
      zones {a, b} = 0, {c, d} = 1, {e} = 2, {f} = 3;  zone 0 reaches 1 and 3, zone 1 reaches 3
      0 -> 3 has zone 1 between: the cover edges are 0 -> 1 and 1 -> 3;  tiers 0, 1, 0, 2"""
    ingress = [[[1]], [[0]], [[1, 3]], [[2]], [[4]], [[3, 0]]]
    egress = [[[1, 5]], [[0, 2]], [[3]], [[2, 5, 9]], [[4]], [[0]]]
    cells = _planes([[V]] * 6, ingress, egress)
    g = cells.zone_graph(want=ALL)
    assert g["zone"].tolist() == [0, 0, 1, 1, 2, 3] and g["n_zones"] == 4 and g["rep"].tolist() == [0, 2, 4, 5] and g["size"].tolist() == [2, 2, 1, 1]
    assert g["edges"].tolist() == [[0, 1], [1, 3]] and g["n_edges"] == 2 and g["tier"].tolist() == [0, 1, 0, 2]
    assert g["reach"].dtype == np.uint64 and g["reach"][:, 0].tolist() == [0b1011, 0b1010, 0b0100, 0b1000]
    assert (g["zone"].dtype, g["rep"].dtype, g["size"].dtype, g["tier"].dtype, g["edges"].dtype) == (np.int32, np.int32, np.int64, np.int32, np.int32)
    assert set(cells.zone_graph()) == {"zone", "rep", "size", "tier", "edges", "n_zones", "n_edges"}
    assert set(cells.zone_graph(want=("tier",))) == {"tier", "n_zones", "n_edges"}
    defining_properties(cells, 0, 1, "by hand")
    empty = cells.zone_graph(0, 0, want=ALL)  # no slot: every pod its own zone, the identity
    assert empty["n_zones"] == 6 and empty["n_edges"] == 0 and empty["edges"].shape == (0, 2) and empty["tier"].tolist() == [0] * 6
    assert empty["zone"].tolist() == empty["rep"].tolist() == list(range(6)) and empty["reach"][:, 0].tolist() == [1 << i for i in range(6)]
    with pytest.raises(CyclonusError, match="slot range out of bounds"):
        cells.zone_graph(0, 2)
    none = PlaneCells(np.zeros((0, 1), np.uint8), np.zeros((0, 1, 0), np.uint64), np.zeros((0, 1, 0), np.uint64)).zone_graph(want=ALL)
    assert none["n_zones"] == 0 and none["n_edges"] == 0 and none["edges"].shape == (0, 2) and none["reach"].shape == (0, 0)
    # the probe mirror
    res = Resources({"x": {}}, [Pod("x", n, {}, f"10.0.0.{i}", []) for i, n in enumerate("abcdef")])
    t = Table(res, new_probe_config(80, "TCP"), cells, 0, 1)
    assert t.zone_graph() == {"zones": [["x/a", "x/b"], ["x/c", "x/d"], ["x/e"], ["x/f"]], "tiers": [0, 1, 0, 2], "edges": [[0, 1], [1, 3]]}
    assert t.render_zone_graph() == TEXT and t.render_zone_graph("text") == TEXT
    assert t.render_zone_graph("dot") == DOT
    with pytest.raises(ValueError, match="invalid format"):
        t.render_zone_graph("svg")
    t0 = Table(res, new_probe_config(80, "TCP"), cells, 0, 0)
    assert t0.zone_graph() == {"zones": [[f"x/{n}"] for n in "abcdef"], "tiers": [0] * 6, "edges": []}
    assert t0.render_zone_graph() == "tier 0: " + ", ".join(f"x/{n}" for n in "abcdef") + "\n"


def _small_cases():
    out = [zg.forward_chain(P) for P in (1, 2, 65)] + [zg.reverse_chain(P) for P in (2, 65, 130)]
    out += [zg.ring_dag(129, 140, 3), zg.ring_dag(64, 75, 1), zg.diamond(), zg.diamond(9)]
    out += [zg.layers(L, n, 30 + L) for L, n in ((7, 9), (8, 8), (5, 13), (10, 13))]
    out += zg.two_slots(66) + [zg.shuffled_ring(65, 2), zg.loopbacks(65)]
    return out


@pytest.mark.parametrize("case", _small_cases(), ids=lambda c: f"{c.name} P {c.g.P} [{c.k_lo}, {c.k_hi})")
def test_closed_forms(case):
    got = case.g.cells().zone_graph(case.k_lo, case.k_hi, want=ALL)
    same_as_expected(got, zg.expected(case), case.name)


@pytest.mark.parametrize("P,K,seed", ((129, 3, 1), (100, 1, 2), (65, 2, 3)))
def test_defining_properties_on_random_digraphs(P, K, seed):
    cells = cg.random_sparse(P, K, seed).g.cells()
    g = defining_properties(cells, 0, K, f"P {P} seed {seed}")
    assert g["n_zones"] > 1 and g["n_edges"] > 0 and g["tier"].max() >= 2  # (the case says something)
    if K > 1:
        defining_properties(cells, 0, 1, f"P {P} seed {seed} slot 0")


def test_config1():
    c = json.load(open(os.path.join(GOLD, "config1.json")))
    status, inp, egp = Oracle(c["policies"], c["resources"]).probe(c["probes"])
    res, cells = Resources.from_json(c["resources"]), PlaneCells(status, inp, egp)
    names = [p.pod_string() for p in res.pods]
    for k_lo, k_hi in ((0, 1), (0, status.shape[1])):
        g = defining_properties(cells, k_lo, k_hi, f"config #1 [{k_lo}, {k_hi})")
        t = Table(res, new_probe_config(80, "TCP"), cells, k_lo, k_hi)
        tg = t.zone_graph()
        assert tg["zones"] == t.zones()["zones"] and tg["tiers"] == g["tier"].tolist() and tg["edges"] == g["edges"].tolist()
        out = {n: set(t.reach(n, "from")) for n in names}
        heads = [z[0] for z in tg["zones"]]
        for a, b in tg["edges"]:  # an edge is a strict reach with nothing between, by a search from every pod
            assert heads[b] in out[heads[a]] and heads[a] not in out[heads[b]]
            assert not any(heads[x] in out[heads[a]] and heads[b] in out[heads[x]] for x in range(len(heads)) if x not in (a, b))
        text = t.render_zone_graph().splitlines()
        assert len(text) == max(tg["tiers"]) + 1 + len(tg["edges"]) and text[0].startswith("tier 0: ")
        dot = t.render_zone_graph("dot")
        assert dot.startswith("digraph zones {\n") and dot.endswith("}\n") and dot.count(" -> ") == len(tg["edges"]) and dot.count("rank=same") == max(tg["tiers"]) + 1
