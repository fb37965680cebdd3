"""Directed graphs as packed verdict planes with their reflexive transitive closure in closed form, for the closure tests
(tests/test_closuregen.py, tests/test_gpu_closure.py), on top of reachgen.GraphPlanes.  A case is (name, GraphPlanes,
slot range, reaches) where reaches is the closed form as a bool matrix [P, P], [p, q] = a path of >= 0 edges leads from p
to q over the edges of the slot range, or None where there is no closed form (the random digraphs: reachgen.bfs knows).
The decoys are reachgen's ways of almost making an edge, planted where taking one for an edge changes the closure."""
from collections import namedtuple

import numpy as np

from reachgen import NOT_VALID, GraphPlanes

Case = namedtuple("Case", "name g k_lo k_hi reaches")
RING_SIZES = (1, 2, 3, 63, 64, 65)
SEGMENT = 4  # rings joined by one-way bridges into a path; a decoy stands where the next path would begin


def pack(m):
    """bool [P, P] -> u64 [P, W] (bit q of row p)."""
    P = m.shape[0]
    W = (P + 63) // 64
    b = np.zeros((P, W * 64), np.uint8)
    b[:, :P] = m
    return np.packbits(b, axis=1, bitorder="little").view(np.uint64).reshape(P, W)


def unpack(plane, P):
    """u64 [P, W] -> bool [P, P]; no bit at or beyond P may be set."""
    bits = np.unpackbits(np.ascontiguousarray(plane).view(np.uint8), axis=1, bitorder="little").astype(bool).reshape(P, -1)
    assert not bits[:, P:].any(), "a bit at or beyond P is set"
    return bits[:, :P]


def zones_of(reaches):
    """(zone i32 [P], n_zones) by the definition: p and q share a zone iff each reaches the other; zones numbered by
    their smallest pod.  Pod by pod, apart from PlaneCells.zones."""
    P = reaches.shape[0]
    zone, n = np.full(P, -1, np.int32), 0
    for p in range(P):
        if zone[p] < 0:
            zone[reaches[p] & reaches[:, p]] = n
            n += 1
    return zone, n


def forward_chain(P):
    """0 -> 1 -> ... -> P - 1: p reaches every q >= p.  The pivots come in the order of the path."""
    p = np.arange(P)
    return Case("forward chain", GraphPlanes(P).edge(p[:-1], p[1:]).tail_bits(), 0, 1, p[None, :] >= p[:, None])


def reverse_chain(P):
    """P - 1 -> ... -> 0: p reaches every q <= p.  Every pivot comes before the pivots its row leads to."""
    p = np.arange(P)
    return Case("reverse chain", GraphPlanes(P).edge(p[1:], p[:-1]).tail_bits(), 0, 1, p[None, :] <= p[:, None])


def shuffled_ring(P, seed):
    """One ring through every pod in a seeded order: one zone, every row all ones up to P and zero beyond."""
    order = np.random.default_rng(seed).permutation(P)
    g = GraphPlanes(P).edge(order, np.roll(order, -1)).tail_bits()
    return Case("shuffled ring", g, 0, 1, np.ones((P, P), bool))


def loopbacks(P):
    """Every pod's edge to itself and nothing else: the identity."""
    p = np.arange(P)
    return Case("loopbacks", GraphPlanes(P).edge(p, p).tail_bits(), 0, 1, np.eye(P, dtype=bool))


def two_slots(P):
    """0 -> P - 1 in slot 0, its back edge in slot 2 (K = 3): two zones over [0, 1), one over [0, 3)."""
    g = GraphPlanes(P, 3).edge(0, P - 1, 0).edge(P - 1, 0, 2).tail_bits()
    one, both = np.eye(P, dtype=bool), np.eye(P, dtype=bool)
    one[0, P - 1] = both[0, P - 1] = both[P - 1, 0] = True
    return [Case("two slots, the first", g, 0, 1, one), Case("two slots, all", g, 0, 3, both)]


def ring_sizes(P, rng):
    """RING_SIZES, then random sizes up to 96, cut to P pods."""
    sizes, left = [], P
    for s in list(RING_SIZES) + [int(x) for x in rng.integers(1, 97, P)]:
        if left <= 0:
            break
        sizes.append(min(s, left))
        left -= sizes[-1]
    return sizes


def ring_dag(P, seed, K=2):
    """Rings of ring_sizes' sizes over a seeded permutation of the pods (consecutive members of a ring lie in unrelated
    words), ring r -> ring r + 1 by a one-way bridge except where r + 1 begins a new path of SEGMENT rings: the zones are
    the rings, and a ring reaches itself and the later rings of its path.  The edges sit in slot 0.  Decoys: the way
    back along every bridge as an ingress bit alone (taken for an edge it merges two zones), the bridge to the next path
    as an egress bit alone (it extends every row of the path), and for K > 1 in the last slot both bits of every source
    into the first pod of three rings under each status that is not VALID (either), and the tail bits."""
    rng = np.random.default_rng(seed)
    order, sizes = rng.permutation(P), ring_sizes(P, rng)
    g = GraphPlanes(P, K)
    ring_of, start = np.zeros(P, np.int64), 0
    rings = []
    for r, n in enumerate(sizes):
        m = order[start:start + n]
        rings.append(m)
        ring_of[m] = r
        if n > 1:
            g.edge(m, np.roll(m, -1), 0)
        start += n
    for r in range(len(rings) - 1):
        a, b = int(rng.choice(rings[r])), int(rng.choice(rings[r + 1]))
        if (r + 1) % SEGMENT:
            g.edge(a, b, 0).ingress_only(b, a, 0)
        else:
            g.egress_only(a, b, 0)
    if K > 1:
        for i, st in enumerate(NOT_VALID):
            if i < len(rings):
                g.not_valid(int(rings[-1 - i][0]), K - 1, st)
    g.tail_bits()
    r = ring_of
    reaches = (r[:, None] // SEGMENT == r[None, :] // SEGMENT) & (r[None, :] >= r[:, None])
    return Case(f"ring dag seed {seed}", g, 0, K, reaches), ring_of


def random_sparse(P, K, seed):
    """1.3 * P random edges in random slots: many small zones and a few large ones, a mean reach of a tenth to a fifth of
    the pods (2 * P edges would collapse into one giant zone).  Then one-bit cells at random, every (P // 12)-th
    destination's last slot under a status that is not VALID with both bits of every source, and the tail bits.  No closed
    form."""
    rng = np.random.default_rng(seed)
    g = GraphPlanes(P, K)
    n = int(1.3 * P)
    g.edge(rng.integers(0, P, n), rng.integers(0, P, n), rng.integers(0, max(K - 1, 1), n))
    g.ingress_only(rng.integers(0, P, 2 * P), rng.integers(0, P, 2 * P), rng.integers(0, K, 2 * P))
    g.egress_only(rng.integers(0, P, 2 * P), rng.integers(0, P, 2 * P), rng.integers(0, K, 2 * P))
    if K > 1:
        for i, d in enumerate(range(3, P, max(8, P // 12))):
            g.not_valid(d, K - 1, NOT_VALID[i % 3])
    return Case(f"random sparse seed {seed}", g.tail_bits(), 0, K, None)


def edges_of(case):
    """[(s, d)] of a case's slot range straight from GraphPlanes' arrays, on the unpacked bits (small P only)."""
    g = case.g
    edge = np.zeros((g.P, g.P), bool)
    bits = lambda plane, k: np.unpackbits(np.ascontiguousarray(plane[:, k]).view(np.uint8), axis=1, bitorder="little")[:, :g.P].astype(bool)  # noqa: E731
    for k in range(case.k_lo, case.k_hi):
        edge |= bits(g.egress, k) & bits(g.ingress, k).T & (g.status[:, k] == 1)[None, :]  # (1: JOB_VALID of the destination)
    return [(int(s), int(d)) for s, d in np.argwhere(edge)]
