"""The closure generator (tests/closuregen.py) and the CPU restatement (probe.PlaneCells.closure / .zones) pinned with
numpy and reachgen.bfs alone: the restatement's rows equal a search from every pod in both directions, the TO closure is
the transpose of the FROM closure, the closed forms hold, the decoys would change the closure if they were edges, and the
random digraphs are not trivial."""
import numpy as np
import pytest

import closuregen as cg
from reachgen import bfs

SIZES = (1, 2, 63, 64, 65, 129, 300)


def _cases(P):
    out = [cg.forward_chain(P), cg.reverse_chain(P), cg.shuffled_ring(P, 40 + P), cg.loopbacks(P), cg.ring_dag(P, 50 + P)[0],
           cg.ring_dag(P, 60 + P, K=1)[0], cg.random_sparse(P, 3, 70 + P), cg.random_sparse(P, 1, 80 + P)]
    return out + (cg.two_slots(P) if P > 1 else [])


def _searched(case, reverse=False):
    """bool [P, P] by reachgen.bfs from every pod over the edges read off the planes' bits."""
    P = case.g.P
    edges = [(d, s) for s, d in cg.edges_of(case)] if reverse else cg.edges_of(case)
    return np.array([[h >= 0 for h in bfs(P, edges, [p])] for p in range(P)], bool).reshape(P, P)


@pytest.mark.parametrize("P", SIZES)
def test_restatement_equals_a_search_from_every_pod(P):
    for case in _cases(P):
        ctx = f"P {P} {case.name}"
        cells = case.g.cells()
        want = _searched(case)
        if case.reaches is not None:
            assert np.array_equal(case.reaches, want), f"{ctx}: the closed form"
        assert want.diagonal().all()
        got = {d: cells.closure(d, case.k_lo, case.k_hi) for d in ("from", "to")}
        assert np.array_equal(cg.unpack(got["from"]["plane"], P), want), f"{ctx}: from"
        assert np.array_equal(cg.unpack(got["to"]["plane"], P), _searched(case, reverse=True)), f"{ctx}: to"
        assert np.array_equal(cg.unpack(got["to"]["plane"], P), want.T), f"{ctx}: to is not the transpose"
        assert got["from"]["n_reach"].tolist() == want.sum(axis=1).tolist() and got["to"]["n_reach"].tolist() == want.sum(axis=0).tolist(), ctx
        assert got["from"]["n_reach"].dtype == np.int64 and got["from"]["plane"].dtype == np.uint64
        assert np.array_equal(cg.pack(want), got["from"]["plane"]), f"{ctx}: pack"
        assert set(cells.closure("to", case.k_lo, case.k_hi, want=("n_reach",))) == {"n_reach"}
        z = cells.zones(case.k_lo, case.k_hi)
        zone, n = cg.zones_of(want)
        assert z["zone"].dtype == np.int32 and z["zone"].tolist() == zone.tolist() and z["n_zones"] == n, f"{ctx}: zones"
        assert z["n_from"].tolist() == want.sum(axis=1).tolist() and z["n_to"].tolist() == want.sum(axis=0).tolist(), ctx
        assert z["zone"][0] == 0 and set(cells.zones(case.k_lo, case.k_hi, want=("n_to",))) == {"n_to"}
        # an empty slot range: the identity
        e = cells.closure("from", case.k_lo, case.k_lo)
        assert np.array_equal(cg.unpack(e["plane"], P), np.eye(P, dtype=bool)) and (e["n_reach"] == 1).all()
        ze = cells.zones(case.k_lo, case.k_lo)
        assert ze["zone"].tolist() == list(range(P)) and ze["n_zones"] == P and (ze["n_from"] == 1).all() and (ze["n_to"] == 1).all()


@pytest.mark.parametrize("P", (300, 513))
def test_closed_forms_by_zone(P):
    one = cg.shuffled_ring(P, 1)
    assert cg.zones_of(one.reaches)[1] == 1 and one.g.egress[:, 0, -1].max() >> np.uint64(P % 64) != 0  # (the tail bits are set)
    assert cg.zones_of(cg.loopbacks(P).reaches)[1] == P
    assert cg.zones_of(cg.forward_chain(P).reaches)[1] == P and cg.zones_of(cg.reverse_chain(P).reaches)[1] == P
    first, both = cg.two_slots(P)
    assert cg.zones_of(first.reaches)[1] == P and cg.zones_of(both.reaches)[1] == P - 1
    assert cg.zones_of(both.reaches)[0][P - 1] == 0
    for K in (1, 2):
        case, ring_of = cg.ring_dag(P, 90 + P, K)
        zone, n = cg.zones_of(case.reaches)
        sizes = np.bincount(ring_of).tolist()
        assert n == len(sizes) and sizes[:6] == list(cg.RING_SIZES)[:6]
        assert ((zone[:, None] == zone[None, :]) == (ring_of[:, None] == ring_of[None, :])).all(), "the zones are the rings"
        # consecutive members of the large rings sit in unrelated words
        m = np.flatnonzero(ring_of == 4)
        assert len(set((m // 64).tolist())) >= 2


def _closure_of(edge):
    """The reflexive transitive closure of a bool edge matrix by repeated squaring."""
    m = edge | np.eye(len(edge), dtype=bool)
    while True:
        n = (m.astype(np.uint32) @ m.astype(np.uint32)) > 0
        if np.array_equal(n, m):
            return m
        m = n


@pytest.mark.parametrize("K", (1, 2))
def test_decoys_would_change_the_closure(K):
    """Taken for an edge, the one-bit cells merge two zones (the ways back along the bridges) and extend a row (the
    bridges between the paths); the cells under a status that is not VALID do either."""
    P = 300
    case, _ = cg.ring_dag(P, 17, K)
    g = case.g
    bits = lambda plane, k: cg.unpack(np.ascontiguousarray(plane[:, k]) & _low(P), P)  # noqa: E731
    edge = np.zeros((P, P), bool)
    for s, d in cg.edges_of(case):
        edge[s, d] = True
    real = _closure_of(edge)
    assert np.array_equal(real, case.reaches)
    n_real = cg.zones_of(real)[1]
    ing, eg = bits(g.ingress, 0).T, bits(g.egress, 0)  # [s, d]
    for name, decoy in (("ingress bit alone", ing & ~eg), ("egress bit alone", eg & ~ing)):
        assert decoy.any(), name
        taken = _closure_of(edge | decoy)
        if name.startswith("ingress"):
            assert cg.zones_of(taken)[1] < n_real, "no one-bit decoy merges two zones"
        else:
            assert cg.zones_of(taken)[1] == n_real and (taken.sum(axis=1) > real.sum(axis=1)).any(), "no one-bit decoy extends a row"
    if K > 1:
        assert set(g.status[:, K - 1].tolist()) == {0, 1, 2, 3}
        both = bits(g.ingress, K - 1).T & bits(g.egress, K - 1) & (g.status[:, K - 1] != 1)[None, :]
        assert both.sum() == 3 * P
        taken = _closure_of(edge | both)
        assert cg.zones_of(taken)[1] < n_real and (taken.sum(axis=1) > real.sum(axis=1)).any()


def _low(P):
    """u64 [W]: the bits below P."""
    W = (P + 63) // 64
    m = np.full(W, np.uint64(0xFFFFFFFFFFFFFFFF))
    if P % 64:
        m[-1] = np.uint64((1 << (P % 64)) - 1)
    return m


@pytest.mark.parametrize("K", (1, 3))
def test_random_digraphs_are_not_trivial(K):
    P = 300
    case = cg.random_sparse(P, K, 70 + P if K == 3 else 80 + P)
    reaches = _searched(case)
    zone, n = cg.zones_of(reaches)
    assert n >= P / 8, n
    assert np.bincount(zone).max() >= 8, np.bincount(zone).max()
    assert 0.05 <= reaches.mean() <= 0.95, reaches.mean()
