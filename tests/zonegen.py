"""Graphs whose zone graph is known in closed form, for the zone graph tests (tests/test_zonegen.py, tests/test_zone_graph.py,
tests/test_gpu_zone_graph.py), on top of closuregen and reachgen.  A case is (name, GraphPlanes, slot range, reaches,
group_of, edges, tiers): reaches as in closuregen; group_of [P] puts every pod into a group (a ring, a layer's pod, ...)
and the groups are the zones; edges are the cover edges and tiers the tiers, both in group ids.  expected() maps them to
the canonical zone ids (zones numbered by their smallest pod) through closuregen.zones_of."""
from collections import namedtuple

import numpy as np

import closuregen as cg
from reachgen import GraphPlanes

ZCase = namedtuple("ZCase", "name g k_lo k_hi reaches group_of edges tiers")
DIAMOND_RINGS = (1, 2, 65, 3)


def _from(case, group_of, edges, tiers):
    return ZCase(case.name, case.g, case.k_lo, case.k_hi, case.reaches, np.asarray(group_of, np.int64), list(edges), dict(tiers))


def forward_chain(P):
    """P singleton zones, p -> p + 1, tier p; the strict reach is the full upper triangle: every shortcut must go."""
    return _from(cg.forward_chain(P), np.arange(P), [(p, p + 1) for p in range(P - 1)], {p: p for p in range(P)})


def reverse_chain(P):
    """p -> p - 1, tier P - 1 - p: the pivots of a row come before it."""
    return _from(cg.reverse_chain(P), np.arange(P), [(p, p - 1) for p in range(1, P)], {p: P - 1 - p for p in range(P)})


def ring_dag(P, seed, K=2):
    """The zones are the rings; ring r -> ring r + 1 inside a path of SEGMENT rings, tier r % SEGMENT.  closuregen's
    decoys stay: an ingress-only back bridge taken for an edge merges two zones, the egress-only bridge adds an edge."""
    case, ring_of = cg.ring_dag(P, seed, K)
    n = int(ring_of.max()) + 1
    return _from(case, ring_of, [(r, r + 1) for r in range(n - 1) if (r + 1) % cg.SEGMENT], {r: r % cg.SEGMENT for r in range(n)})


def diamond(seed=5):
    """Rings a, b, c, d of DIAMOND_RINGS' sizes over a seeded permutation with a -> b, a -> c, b -> d, c -> d and the
    shortcut a -> d: four cover edges, tiers 0, 1, 1, 2."""
    rng = np.random.default_rng(seed)
    P = sum(DIAMOND_RINGS)
    order, g = rng.permutation(P), GraphPlanes(P)
    ring_of, rings, start = np.zeros(P, np.int64), [], 0
    for r, n in enumerate(DIAMOND_RINGS):
        m = order[start:start + n]
        rings.append(m)
        ring_of[m] = r
        if n > 1:
            g.edge(m, np.roll(m, -1))
        start += n
    for a, b in ((0, 1), (0, 2), (1, 3), (2, 3), (0, 3)):
        g.edge(int(rng.choice(rings[a])), int(rng.choice(rings[b])))
    g.tail_bits()
    zr = np.array([[1, 1, 1, 1], [0, 1, 0, 1], [0, 0, 1, 1], [0, 0, 0, 1]], bool)
    case = cg.Case("diamond with a shortcut", g, 0, 1, zr[ring_of][:, ring_of])
    return _from(case, ring_of, [(0, 1), (0, 2), (1, 3), (2, 3)], {0: 0, 1: 1, 2: 1, 3: 2})


def layers(L, n, seed):
    """L layers of n singleton zones over a seeded permutation of the pods: every zone of layer i -> every zone of layer
    i + 1, and random shortcuts from layer i to the layers from i + 2 on.  The cover is exactly the (L - 1) * n * n edges
    between consecutive layers; the tier is the layer."""
    rng = np.random.default_rng(seed)
    P = L * n
    order, g = rng.permutation(P), GraphPlanes(P)
    layer_of = np.zeros(P, np.int64)
    layer_of[order] = np.arange(P) // n
    pods = [order[i * n:(i + 1) * n] for i in range(L)]
    edges = []
    for i in range(L - 1):
        s, d = np.meshgrid(pods[i], pods[i + 1], indexing="ij")
        g.edge(s.ravel(), d.ravel())
        edges += [(int(a), int(b)) for a, b in zip(s.ravel(), d.ravel())]
    for i in range(L - 2):
        for _ in range(2 * n):
            g.edge(int(rng.choice(pods[i])), int(rng.choice(pods[int(rng.integers(i + 2, L))])))
    g.tail_bits()
    reaches = (layer_of[None, :] > layer_of[:, None]) | np.eye(P, dtype=bool)
    case = cg.Case(f"{L} layers of {n} seed {seed}", g, 0, 1, reaches)
    return _from(case, np.arange(P), edges, {p: int(layer_of[p]) for p in range(P)})


def two_slots(P):
    """closuregen.two_slots: one edge 0 -> P - 1 over [0, 1); over [0, 3) the two pods are one zone and no edge is left."""
    one, both = cg.two_slots(P)
    merged = np.arange(P)
    merged[P - 1] = 0
    return [_from(one, np.arange(P), [(0, P - 1)], {p: int(p == P - 1) for p in range(P)}), _from(both, merged, [], {p: 0 for p in range(P - 1)})]


def shuffled_ring(P, seed):
    """One zone, no edge."""
    return _from(cg.shuffled_ring(P, seed), np.zeros(P), [], {0: 0})


def loopbacks(P):
    """P zones, no edge."""
    return _from(cg.loopbacks(P), np.arange(P), [], {p: 0 for p in range(P)})


def expected(case):
    """What cyc_table_zone_graph returns for a case: {"zone", "n_zones", "rep", "size", "tier", "edges", "n_edges", "reach"
    (bool [Z, Z])}, with the groups checked to be the zones of the closed form."""
    zone, Z = cg.zones_of(case.reaches)
    zid = {}
    for p, grp in enumerate(case.group_of.tolist()):
        assert zid.setdefault(grp, int(zone[p])) == zone[p], f"{case.name}: group {grp} is not inside one zone"
    assert len(set(zid.values())) == len(zid) == Z, f"{case.name}: the groups are not the zones"
    rep = np.unique(zone, return_index=True)[1].astype(np.int32)  # the first pod of every zone, in the order of the ids
    tier = np.zeros(Z, np.int32)
    for grp, t in case.tiers.items():
        tier[zid[grp]] = t
    edges = np.array(sorted((zid[a], zid[b]) for a, b in case.edges), np.int32).reshape(-1, 2)
    return {"zone": zone, "n_zones": Z, "rep": rep, "size": np.bincount(zone, minlength=Z).astype(np.int64), "tier": tier, "edges": edges,
            "n_edges": len(edges), "reach": case.reaches[rep][:, rep]}


def pack_zone_plane(reach):
    """bool [Z, Z] -> u64 [Z, ceil(Z / 64)]: the tight plane of d_zreach."""
    return cg.pack(reach) if reach.shape[0] else np.zeros((0, 0), np.uint64)
