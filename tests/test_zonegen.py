"""tests/zonegen.py's closed forms at small P against the definition, spelt out zone by zone on closuregen's `reaches` and
apart from probe.PlaneCells: a -> b is a cover edge iff a strictly reaches b and no third zone c lies between them (a
triple loop over the zones); the tier of a zone is the longest chain of cover edges that ends in it.  Also that the
closed-form reaches of the new cases are the closure of the edges the planes hold."""
import numpy as np
import pytest

import closuregen as cg
import zonegen as zg
from reachgen import bfs


def _cases():
    out = []
    for P in (1, 2, 63, 65, 130):
        out += [zg.forward_chain(P), zg.reverse_chain(P), zg.loopbacks(P), zg.shuffled_ring(P, 3 + P)]
    out += [zg.ring_dag(P, 11 + P, K) for P, K in ((64, 1), (129, 3), (130, 2))]
    out += [zg.diamond(s) for s in (5, 6)]
    out += [zg.layers(L, n, 20 + L) for L, n in ((7, 9), (4, 16), (5, 13), (10, 13), (2, 3), (3, 1))]
    out += zg.two_slots(2) + zg.two_slots(66)
    return out


def _brute(case):
    """(edges, tiers) by the definition, in canonical zone ids."""
    zone, Z = cg.zones_of(case.reaches)
    rep = [int(np.flatnonzero(zone == z)[0]) for z in range(Z)]
    S = [[bool(case.reaches[rep[a], rep[b]]) and a != b for b in range(Z)] for a in range(Z)]
    edges = []
    for a in range(Z):
        for b in range(Z):
            if S[a][b]:
                between = False
                for c in range(Z):
                    if S[a][c] and S[c][b]:
                        between = True
                        break
                if not between:
                    edges.append((a, b))
    into = [[] for _ in range(Z)]
    for a, b in edges:
        into[b].append(a)
    memo = {}

    def tier(z):  # (an iterative walk: a chain of 130 zones is deeper than it is worth recursing)
        stack = [z]
        while stack:
            x = stack[-1]
            todo = [a for a in into[x] if a not in memo]
            if todo:
                stack += todo
            else:
                memo[x] = max((memo[a] + 1 for a in into[x]), default=0)
                stack.pop()
        return memo[z]
    return edges, [tier(z) for z in range(Z)]


@pytest.mark.parametrize("case", _cases(), ids=lambda c: f"{c.name} P {c.g.P} [{c.k_lo}, {c.k_hi})")
def test_closed_forms_are_the_definition(case):
    P = case.g.P
    # the closed-form reaches are the closure of the planes' edges (closuregen's own cases are pinned by its own test too)
    found = cg.edges_of(case)
    for p in range(P):
        assert [h >= 0 for h in bfs(P, found, [p])] == case.reaches[p].tolist(), f"row {p} of reaches"
    want = zg.expected(case)
    edges, tiers = _brute(case)
    assert want["edges"].tolist() == [list(e) for e in edges]
    assert want["tier"].tolist() == tiers
    assert want["n_zones"] == len(tiers) and want["size"].sum() == P and want["rep"][0] == 0
    assert (np.diff(want["rep"]) > 0).all()


def test_the_shapes_the_cases_promise():
    """Chains: Z = P and P - 1 edges out of a full triangle of P (P - 1) / 2 strict pairs; layers: (L - 1) n^2 edges; the
    diamond: 4 of 5; two slots: one edge, then one zone less and none."""
    for P in (2, 65, 130):
        for case in (zg.forward_chain(P), zg.reverse_chain(P)):
            e = zg.expected(case)
            assert e["n_zones"] == P and e["n_edges"] == P - 1 and e["reach"].sum() - P == P * (P - 1) // 2
            assert sorted(e["tier"].tolist()) == list(range(P))
    for L, n in ((7, 9), (10, 13)):
        case = zg.layers(L, n, 1)
        e = zg.expected(case)
        assert e["n_edges"] == (L - 1) * n * n and e["n_zones"] == L * n
        assert len(cg.edges_of(case)) > e["n_edges"], "no shortcut was planted"
    e = zg.expected(zg.diamond())
    assert e["n_zones"] == 4 and e["n_edges"] == 4 and sorted(e["tier"].tolist()) == [0, 1, 1, 2] and sorted(e["size"].tolist()) == [1, 2, 3, 65]
    one, both = (zg.expected(c) for c in zg.two_slots(66))
    assert (one["n_zones"], one["n_edges"], both["n_zones"], both["n_edges"]) == (66, 1, 65, 0)
    assert zg.expected(zg.shuffled_ring(65, 1))["n_zones"] == 1 and zg.expected(zg.loopbacks(65))["n_edges"] == 0
