"""Multi-hop reachability, the CPU restatement (probe.PlaneCells.adjacency / reach, probe.Table.reach): small graphs
written as packed planes (reachgen.GraphPlanes) with hop values worked out by hand or by a search over the edge list
written in the test helpers; the decoys that must never make an edge; and config #1's table against a search over the
Items of Table.get."""
import json
import os

import numpy as np
import pytest

from cyclonus_amd import _lib
from cyclonus_amd._lib import CyclonusError
from cyclonus_amd.probe import ALLOWED, PlaneCells, Resources, Table, new_all_available
from oracle.oracle import Oracle
from reachgen import NOT_VALID, GraphPlanes, bfs, chain

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def _bits(words, P):
    """A row of u64 words as the list of its set bits (every bit of the words, also those at or beyond P)."""
    return [b for b in range(len(words) * 64) if (int(words[b // 64]) >> (b % 64)) & 1]


def _hops(g, seeds, direction="from", max_hops=-1, **kw):
    """reach of one seed set -> the hops list; reach and levels are checked against it on the way."""
    r = g.cells().reach([seeds], direction, max_hops=max_hops, **kw)
    hops = r["hops"][0].tolist()
    assert r["hops"].dtype == np.int32 and r["reach"].dtype == np.uint64 and r["levels"].dtype == np.int64
    assert r["hops"].shape == (1, g.P) and r["reach"].shape == (1, g.W) and r["levels"].shape == (1,)
    assert _bits(r["reach"][0], g.P) == [p for p in range(g.P) if hops[p] >= 0]
    assert int(r["levels"][0]) == max(hops, default=-1)
    return hops


def test_chain():
    g = chain(4)
    assert _hops(g, [0]) == [0, 1, 2, 3]
    assert _hops(g, [0], max_hops=2) == [0, 1, 2, -1]
    assert int(g.cells().reach([[0]], max_hops=2)["levels"][0]) == 2
    assert _hops(g, [0], max_hops=0) == [0, -1, -1, -1]
    assert _hops(g, [3], "to") == [3, 2, 1, 0]
    assert _hops(g, [3], "to", max_hops=1) == [-1, -1, 1, 0]
    assert _hops(g, [3]) == [-1, -1, -1, 0]
    assert _hops(g, [0], "to") == [0, -1, -1, -1]
    assert _hops(g, [1], _lib.REACH_FROM) == [-1, 0, 1, 2] and _hops(g, [1], _lib.REACH_TO) == [1, 0, -1, -1]


def test_cycle_loopback_and_sets():
    g = GraphPlanes(70).edge([0, 1, 2], [1, 2, 0])  # a cycle
    g.edge(5, 5)  # a pod whose only edge is a loopback
    g.edge([10, 11, 12, 20, 21], [11, 12, 13, 21, 13])  # 10 -> 11 -> 12 -> 13 <- 21 <- 20
    assert _hops(g, [0])[:3] == [0, 1, 2] and _hops(g, [1])[:3] == [2, 0, 1]
    assert _hops(g, [0], "to")[:3] == [0, 2, 1]
    assert sum(h >= 0 for h in _hops(g, [0])) == 3
    for direction in ("from", "to"):
        assert [p for p, h in enumerate(_hops(g, [5], direction)) if h >= 0] == [5]
    adj = g.cells().adjacency("from")
    assert _bits(adj[5], 70) == [5] and _bits(adj[0], 70) == [1]  # (the loopback edge is kept in the plane)
    # an empty set: nothing reached; duplicates: as the set without them
    assert _hops(g, []) == [-1] * 70
    r = g.cells().reach([[]])
    assert not r["reach"].any() and r["levels"].tolist() == [-1]
    assert _hops(g, [10, 10, 10]) == _hops(g, [10])
    # two seeds whose regions overlap: the lesser hop value wins (13 is 3 from 10 and 2 from 20)
    h = _hops(g, [10, 20])
    assert [h[p] for p in (10, 11, 12, 13, 20, 21)] == [0, 1, 2, 2, 0, 1]
    assert _hops(g, [20, 10, 20]) == h
    # several sets in one call are the single calls
    sets = [[0], [], [10, 20], [5, 5], [69]]
    r = g.cells().reach(sets)
    assert r["hops"].tolist() == [_hops(g, s) for s in sets] and r["levels"].tolist() == [2, -1, 2, 0, 0]
    assert set(g.cells().reach(sets, want=("levels",))) == {"levels"}


def test_slot_ranges():
    g = GraphPlanes(66, 3).edge(0, 65, 1)  # an edge in slot 1 alone
    for k_lo, k_hi, seen in ((0, 3, True), (1, 2, True), (0, 2, True), (0, 1, False), (2, 3, False), (1, 1, False)):
        assert (_hops(g, [0], k_lo=k_lo, k_hi=k_hi)[65] == 1) == seen, (k_lo, k_hi)
        assert (_bits(g.cells().adjacency("to", k_lo, k_hi)[65], 66) == [0]) == seen
    for k_lo, k_hi in ((-1, 2), (0, 4), (2, 1)):
        with pytest.raises(CyclonusError, match="slot range out of bounds"):
            g.cells().reach([[0]], k_lo=k_lo, k_hi=k_hi)


def test_the_decoys_never_make_an_edge():
    P = 70
    g = chain(P, 3, 1)  # the edges: slot 1
    g.ingress_only(P - 1, 0, 1).egress_only(P - 1, 0, 1 - 1)  # the two bits of (69 -> 0), in different slots
    g.ingress_only(40, 5, 0).egress_only(41, 5, 2)
    for i, st in enumerate(NOT_VALID):  # both bits of every source under each status that is not VALID
        g.not_valid(10 + i, 2, st)
    g.tail_bits()
    want = list(range(P))
    assert _hops(g, [0]) == want and _hops(g, [P - 1]) == [-1] * (P - 1) + [0]
    adj = g.cells().adjacency("from")
    assert [_bits(adj[s], P) for s in range(P)] == [[s + 1] if s + 1 < P else [] for s in range(P)]
    assert not (adj[:, -1] >> np.uint64(P % 64)).any()  # bits at or beyond P
    # the same cells under VALID are edges: the decoys are not inert bits
    g.status[:, 2] = _lib.JOB_VALID
    assert _hops(g, [0])[10:13] == [1, 1, 1]


def test_from_is_to_on_the_transpose():
    rng = np.random.default_rng(5)
    P, n = 131, 300
    s, d, k = rng.integers(0, P, n), rng.integers(0, P, n), rng.integers(0, 2, n)
    g, t = GraphPlanes(P, 2).edge(s, d, k).tail_bits(), GraphPlanes(P, 2).edge(d, s, k).tail_bits()
    sets = [[0], [7, 130], list(range(P)), []]
    a, b = g.cells().reach(sets, "from"), t.cells().reach(sets, "to")
    for n_ in ("reach", "hops", "levels"):
        assert np.array_equal(a[n_], b[n_]), n_
    assert np.array_equal(g.cells().adjacency("from"), t.cells().adjacency("to"))
    assert a["hops"][0].tolist() == bfs(P, list(zip(s.tolist(), d.tolist())), [0]) and a["levels"][0] >= 3
    # TO's plane is the bit transpose of FROM's
    fr, to = g.cells().adjacency("from"), g.cells().adjacency("to")
    assert all(_bits(to[p], P) == [q for q in range(P) if p in _bits(fr[q], P)] for p in (0, 63, 64, 130))
    for bad in ("sideways", 2, -1):
        with pytest.raises(CyclonusError, match="unknown direction"):
            g.cells().reach(sets, bad)
    for bad, msg in (([[0], [3, P]], f"seeds\\[2\\] = {P} is not a pod in \\[0, {P}\\)"), ([[-1]], f"seeds\\[0\\] = -1 is not a pod")):
        with pytest.raises(CyclonusError, match=msg):
            g.cells().reach(bad)


def test_config1_reach_equals_a_search_over_the_items():
    """Config #1 over the oracle's planes, every port of every pod: Table.reach of each pod, both directions and a
    bound, against a search written here over the Combined values of Table.get's Items."""
    c = json.load(open(os.path.join(GOLD, "config1.json")))
    res, cfg = Resources.from_json(c["resources"]), new_all_available()
    st, ing, eg = Oracle(c["policies"], c["resources"]).probe([cfg.to_json()])
    table = Table(res, cfg, PlaneCells(st, ing, eg), 0, st.shape[1])
    names = table.items
    assert len(names) == 9
    edges = {(fr, to) for fr, to in table.keys() if any(r.combined == ALLOWED for r in table.get(fr, to).job_results.values())}
    assert 0 < len(edges) < 81

    def search(seed, flip, max_hops):
        hops, level, h = {seed: 0}, [seed], 0
        while level and (max_hops < 0 or h < max_hops):
            h += 1
            nxt = []
            for p in level:
                for q in names:
                    if ((q, p) if flip else (p, q)) in edges and q not in hops:
                        hops[q] = h
                        nxt.append(q)
            level = nxt
        return hops

    depth = 0
    for pod in names:
        for direction, flip in (("from", False), ("to", True)):
            for max_hops in (-1, 0, 1, 2):
                want = search(pod, flip, max_hops)
                assert table.reach(pod, direction, max_hops) == want, (pod, direction, max_hops)
                depth = max(depth, *want.values())
    assert depth >= 1
    assert table.reach([names[0], names[1]]) == {p: min(h for h in (search(names[0], False, -1).get(p), search(names[1], False, -1).get(p))
                                                        if h is not None)
                                                 for p in names if p in search(names[0], False, -1) or p in search(names[1], False, -1)}


@pytest.mark.parametrize("P,K", ((1, 1), (64, 3), (65, 1), (130, 3)))
def test_the_edges_are_the_allowed_combined_cells(P, K):
    """Random dense planes with all four statuses and set bits at or beyond P: the restatement's edges, read off the
    unpacked bits, are exactly the cells whose Combined code is allowed in some slot of the range."""
    rng = np.random.default_rng(P * 10 + K)
    W = (P + 63) // 64
    cells = PlaneCells(rng.integers(0, 4, (P, K)).astype(np.uint8), rng.integers(0, 2**64, (P, K, W), dtype=np.uint64),
                       rng.integers(0, 2**64, (P, K, W), dtype=np.uint64))
    for k_lo, k_hi in ((0, K), (K - 1, K), (0, 0)):
        allowed = (cells.cells(0, P, 0, P, k_lo, k_hi, want=("combined",))["combined"] == _lib.CONN_ALLOWED).any(axis=2)
        s, d = cells._edge_pairs(k_lo, k_hi)
        got = np.zeros((P, P), bool)
        got[s, d] = True
        assert np.array_equal(got, allowed) and len(s) == int(allowed.sum())
        fr, to = cells.adjacency("from", k_lo, k_hi), cells.adjacency("to", k_lo, k_hi)
        assert [_bits(fr[p], P) for p in range(P)] == [np.nonzero(allowed[p])[0].tolist() for p in range(P)]
        assert [_bits(to[p], P) for p in range(P)] == [np.nonzero(allowed[:, p])[0].tolist() for p in range(P)]
