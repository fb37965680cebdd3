"""The transitive closure and the zones through the probe mirror on the CPU (probe.Table.zones / blast_radius /
render_zone_table over probe.PlaneCells.closure / .zones): a 5-pod table worked out by hand, and config #1 from the
oracle's planes against Table.reach's search from every pod."""
import json
import os

import numpy as np
import pytest

from cyclonus_amd import _lib
from cyclonus_amd._lib import CyclonusError
from cyclonus_amd.probe import PlaneCells, Pod, Resources, Table, new_probe_config
from oracle.oracle import Oracle

GOLD = os.path.join(os.path.dirname(__file__), "golden")
V, BNP = _lib.JOB_VALID, _lib.JOB_BAD_NAMED_PORT


def _planes(status, ingress, egress):
    """status [P][K]; ingress[d][k] and egress[s][k] as lists of set bits -> PlaneCells (one word per row)."""
    word = lambda bits: np.uint64(sum(1 << b for b in bits))  # noqa: E731
    to_plane = lambda rows: np.array([[[word(bits)] for bits in row] for row in rows], np.uint64)  # noqa: E731
    return PlaneCells(np.array(status, np.uint8), to_plane(ingress), to_plane(egress))


def _split(line):
    return [x.strip() for x in line.strip("|").split("|")]


def test_five_pods_by_hand():
    """One slot.  Edges (both bits under a VALID destination): a <-> b, b -> c, c <-> d, e -> e.  Decoys: d -> e as an egress
    bit alone, bit 9 (beyond P) in d's egress row, and in the second table every source into e under BAD_NAMED_PORT.
      from a or b: a b c d;  from c or d: c d;  from e: e              -> zones {a, b} {c, d} {e}
      into a or b: a b;      into c or d: a b c d;  into e: e"""
    ingress = [[[1]], [[0]], [[1, 3]], [[2]], [[4]]]
    egress = [[[1]], [[0, 2]], [[3]], [[2, 4, 9]], [[4]]]
    cells = _planes([[V]] * 5, ingress, egress)
    rows = {"from": [0b01111, 0b01111, 0b01100, 0b01100, 0b10000], "to": [0b00011, 0b00011, 0b01111, 0b01111, 0b10000]}
    for direction in ("from", "to", _lib.REACH_FROM, _lib.REACH_TO):
        got = cells.closure(direction)
        want = rows[{_lib.REACH_FROM: "from", _lib.REACH_TO: "to"}.get(direction, direction)]
        assert got["plane"].dtype == np.uint64 and got["plane"].shape == (5, 1) and got["plane"][:, 0].tolist() == want
        assert got["n_reach"].tolist() == [bin(x).count("1") for x in want]
    z = cells.zones()
    assert z["zone"].tolist() == [0, 0, 1, 1, 2] and z["n_zones"] == 3
    assert z["n_from"].tolist() == [4, 4, 2, 2, 1] and z["n_to"].tolist() == [2, 2, 4, 4, 1]
    assert set(cells.zones(want=("n_from",))) == {"n_from"} and set(cells.zones(want=("zone",))) == {"zone", "n_zones"}
    # the same edges with e's slot not VALID and both bits of every source into it: nothing reaches e any more, e -> e included
    bad = _planes([[V]] * 4 + [[BNP]], ingress[:4] + [[[0, 1, 2, 3, 4]]], [[row[0] + [4]] for row in egress])
    assert bad.closure("from")["plane"][:, 0].tolist() == rows["from"] and bad.zones()["zone"].tolist() == [0, 0, 1, 1, 2]
    with pytest.raises(CyclonusError, match="unknown direction"):
        cells.closure(2)
    with pytest.raises(CyclonusError, match="slot range out of bounds"):
        cells.zones(0, 2)
    none = PlaneCells(np.zeros((0, 1), np.uint8), np.zeros((0, 1, 0), np.uint64), np.zeros((0, 1, 0), np.uint64))
    assert none.zones()["n_zones"] == 0 and none.closure()["plane"].shape == (0, 0)
    # the probe mirror
    res = Resources({"x": {}}, [Pod("x", n, {}, f"10.0.0.{i}", []) for i, n in enumerate("abcde")])
    t = Table(res, new_probe_config(80, "TCP"), cells, 0, 1)
    assert t.zones() == {"zones": [["x/a", "x/b"], ["x/c", "x/d"], ["x/e"]]}
    assert t.blast_radius() == {"x/a": (4, 2), "x/b": (4, 2), "x/c": (2, 4), "x/d": (2, 4), "x/e": (1, 1)}
    lines = t.render_zone_table().splitlines()
    assert lines[0] == lines[2] == lines[-1] and set(lines[0]) == {"+", "-"}
    assert _split(lines[1]) == ["", "X/A (+1)", "X/C (+1)", "X/E"]
    assert [_split(ln) for ln in lines[3:-1]] == [["x/a (+1)", "X", "X", "."], ["x/c (+1)", ".", "X", "."], ["x/e", ".", ".", "X"]]
    # no slot at all: every pod its own zone
    t0 = Table(res, new_probe_config(80, "TCP"), cells, 0, 0)
    assert t0.zones() == {"zones": [[n] for n in ("x/a", "x/b", "x/c", "x/d", "x/e")]}
    assert set(t0.blast_radius().values()) == {(1, 1)}


def test_config1_against_a_search_from_every_pod():
    c = json.load(open(os.path.join(GOLD, "config1.json")))
    status, inp, egp = Oracle(c["policies"], c["resources"]).probe(c["probes"])
    res, cells = Resources.from_json(c["resources"]), PlaneCells(status, inp, egp)
    names = [p.pod_string() for p in res.pods]
    for k_lo, k_hi in ((0, 1), (0, status.shape[1])):
        t = Table(res, new_probe_config(80, "TCP"), cells, k_lo, k_hi)
        out = {n: set(t.reach(n, "from")) for n in names}
        into = {n: set(t.reach(n, "to")) for n in names}
        assert t.blast_radius() == {n: (len(out[n]), len(into[n])) for n in names}
        zones = t.zones()["zones"]
        assert sorted(n for z in zones for n in z) == sorted(names)
        assert [z[0] for z in zones] == sorted((z[0] for z in zones), key=names.index)  # zones by first pod
        assert all(z == sorted(z, key=names.index) for z in zones)  # members in plane order
        of = {n: i for i, z in enumerate(zones) for n in z}
        for p in names:
            for q in names:
                assert (of[p] == of[q]) == (q in out[p] and p in out[q]), (p, q)
        label = lambda z: z[0] + (f" (+{len(z) - 1})" if len(z) > 1 else "")  # noqa: E731
        lines = t.render_zone_table().splitlines()
        assert _split(lines[1]) == [""] + [label(z).upper() for z in zones]
        rows = lines[3:-1]
        assert len(rows) == len(zones)
        for ln, z in zip(rows, zones):
            assert _split(ln) == [label(z)] + ["X" if y[0] in out[z[0]] else "." for y in zones]
    assert 1 <= len(zones) <= len(names)
