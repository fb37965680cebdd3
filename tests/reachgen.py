"""Directed graphs as packed verdict planes, for the reachability tests (tests/test_reach.py, tests/test_gpu_reach.py):
an edge s -> d in slot k is the ingress bit (d, k, s) and the egress bit (s, k, d) under a VALID status[d][k].  The
decoys are the ways of almost making an edge: one of the two bits alone, both bits under a status that is not VALID,
bits at or beyond P."""
import numpy as np

from cyclonus_amd import _lib
from cyclonus_amd.probe import PlaneCells

NOT_VALID = (_lib.JOB_NONE, _lib.JOB_BAD_NAMED_PORT, _lib.JOB_BAD_PORT_PROTOCOL)


class GraphPlanes:
    def __init__(self, P, K=1):
        self.P, self.K, self.W = P, K, (P + 63) // 64
        self.status = np.full((P, K), _lib.JOB_VALID, np.uint8)
        self.ingress = np.zeros((P, K, self.W), np.uint64)
        self.egress = np.zeros((P, K, self.W), np.uint64)

    @staticmethod
    def _set(plane, row, k, col):
        row, k, col = np.broadcast_arrays(np.asarray(row), np.asarray(k), np.asarray(col))
        np.bitwise_or.at(plane, (row, k, col // 64), np.uint64(1) << (col % 64).astype(np.uint64))

    def ingress_only(self, s, d, k=0):
        self._set(self.ingress, d, k, s)
        return self

    def egress_only(self, s, d, k=0):
        self._set(self.egress, s, k, d)
        return self

    def edge(self, s, d, k=0):
        """Both bits of s -> d in slot k (scalars or arrays): an edge wherever status[d][k] is VALID."""
        return self.ingress_only(s, d, k).egress_only(s, d, k)

    def not_valid(self, d, k, status):
        """status[d][k] = `status` with both bits of every source set: P would-be edges into d."""
        self.status[d, k] = status
        return self.edge(np.arange(self.P), d, k)

    def tail_bits(self):
        """Every plane bit at or beyond P set, in every row and slot."""
        if self.P % 64:
            m = np.uint64((1 << 64) - (1 << (self.P % 64)))
            self.ingress[:, :, -1] |= m
            self.egress[:, :, -1] |= m
        return self

    def cells(self):
        return PlaneCells(self.status, self.ingress, self.egress)

    def torch(self):
        """(status, ingress, egress) as the tensors tests/test_gpu_table_counts._Planes takes."""
        import torch

        return (torch.from_numpy(self.status.copy()), torch.from_numpy(self.ingress.view(np.int64).copy()),
                torch.from_numpy(self.egress.view(np.int64).copy()))


def chain(P, K=1, k=0):
    """0 -> 1 -> ... -> P - 1 in slot k."""
    return GraphPlanes(P, K).edge(np.arange(P - 1), np.arange(1, P), k)


def random_digraph(P, K, seed, degree=2):
    """`degree` * P random edges in random slots (so some pods have no way out and some no way in), then the decoys: one-bit cells at random, every eighth
    destination's last slot (of many pods: of twelve destinations) under a status that is not VALID with both bits of
    every source, and the tail bits."""
    rng = np.random.default_rng(seed)
    g = GraphPlanes(P, K)
    s = rng.integers(0, P, degree * P)
    g.edge(s, rng.integers(0, P, len(s)), rng.integers(0, K, len(s)))
    g.ingress_only(rng.integers(0, P, 2 * P), rng.integers(0, P, 2 * P), rng.integers(0, K, 2 * P))
    g.egress_only(rng.integers(0, P, 2 * P), rng.integers(0, P, 2 * P), rng.integers(0, K, 2 * P))
    for i, d in enumerate(range(3, P, max(8, P // 12))):
        g.not_valid(d, K - 1, NOT_VALID[i % 3])
    return g.tail_bits()


def bfs(P, edges, seeds, max_hops=-1):
    """hops list of a plain search over an edge list [(s, d)], written apart from PlaneCells.reach."""
    out = [[] for _ in range(P)]
    for s, d in edges:
        out[s].append(d)
    hops = [-1] * P
    level = sorted(set(seeds))
    for p in level:
        hops[p] = 0
    h = 0
    while level and (max_hops < 0 or h < max_hops):
        h += 1
        nxt = []
        for p in level:
            for q in out[p]:
                if hops[q] < 0:
                    hops[q] = h
                    nxt.append(q)
        level = nxt
    return hops
