"""Verdict planes with real connectivity classes, for the class tests (tests/test_classgen.py, tests/test_classes.py,
tests/test_gpu_classes.py).  Every pod has a source template and a destination template, assigned so that the members
of a class are not neighbours; the ingress and egress bits of a cell are QI[ts][td][k] and QE[ts][td][k] and the status
of (d, k) is ST[td][k], so pods with equal templates behave alike.  Then the decoys: pairs of pods with the same two
templates that differ in exactly one planted way, each with the verdict (splits or does not split, per view and side)
that the definition of include/cyclonus_hip.h gives:
  a  one cell at destination P - 1 in the last slot             splits sources
  b  one cell in word 0 of the first slot                       splits sources
  c  only the loopback cell (p, p) against (q, p)               splits sources (loopback is not special)
  d  plane bits at or beyond P (where P leaves any)             splits nothing
  e  plane bits under a non-VALID (d, k)                        splits neither sources nor destinations
  f  an ingress bit where both pods' egress bit is 0            splits sources under Ingress only; fe: the mirror image
  g  BAD_NAMED_PORT against BAD_PORT_PROTOCOL in one slot       splits destinations under Ingress and Combined only
  h  no job against a VALID job blocked from everywhere         splits destinations
Templates may merge (two templates can give the same codes under a view), so the number of classes is whatever the
restatement says, never the number of templates."""
import numpy as np

from cyclonus_amd import _lib
from cyclonus_amd.probe import PlaneCells

VIEWS = ("ingress", "egress", "combined")
ALL, NONE = {v: True for v in VIEWS}, {v: False for v in VIEWS}


class ClassProblem:
    def __init__(self, P, K, seed, n_src=5, n_dst=4):
        rng = np.random.default_rng(seed)
        self.P, self.K, self.W = P, K, (P + 63) // 64
        pods = np.arange(P)
        self.src_t, self.dst_t = pods % n_src, (pods + pods // n_dst) % n_dst
        qi, qe = rng.integers(0, 2, (n_src, n_dst, K), dtype=np.uint8), rng.integers(0, 2, (n_src, n_dst, K), dtype=np.uint8)
        st = rng.choice(np.array([_lib.JOB_VALID] * 5 + [_lib.JOB_NONE, _lib.JOB_BAD_NAMED_PORT, _lib.JOB_BAD_PORT_PROTOCOL], np.uint8), (n_dst, K))
        st[0] = _lib.JOB_VALID  # (one destination template with every job)
        self.status = np.ascontiguousarray(st[self.dst_t])
        # bit matrices [row pod, k, column pod]: ingress rows are destinations, egress rows are sources
        self._in = np.ascontiguousarray(qi[self.src_t][:, self.dst_t].transpose(1, 2, 0))
        self._eg = np.ascontiguousarray(qe[self.src_t][:, self.dst_t].transpose(0, 2, 1))
        self.tail = {"in": [], "eg": []}  # pods whose rows get every bit at or beyond P
        self.decoys = {}
        self._plant(rng)
        self.ingress, self.egress = self._pack(self._in, self.tail["in"]), self._pack(self._eg, self.tail["eg"])
        del self._in, self._eg

    def _pack(self, bits, tail_rows):
        P, K, W = self.P, self.K, self.W
        padded = np.zeros((P, K, W * 64), np.uint8)
        padded[:, :, :P] = bits
        padded[tail_rows, :, P:] = 1
        return np.packbits(padded, axis=2, bitorder="little").view(np.uint64).reshape(P, K, W)

    def _cell(self, s, d, k, i, e):
        """The cell (s, d, k) gets ingress bit i and egress bit e under a VALID status."""
        self._in[d, k, s], self._eg[s, k, d] = i, e
        self.status[d, k] = _lib.JOB_VALID

    def _plant(self, rng):
        P, K = self.P, self.K
        groups = {}
        for p in range(2, P - 1):  # (pods 0, 1 and P - 1 are the columns of decoys a and b and the first pod)
            groups.setdefault((int(self.src_t[p]), int(self.dst_t[p])), []).append(p)
        pairs = [(g[0], g[1]) for g in groups.values() if len(g) >= 2]
        rng.shuffle(pairs)
        used = {0, 1, P - 1} | {p for pr in pairs for p in pr}
        free = [p for p in range(2, P - 1) if p not in used]
        assert len(pairs) >= 10 and len(free) >= 2, "too few pods for the decoys"
        take = iter(pairs)
        k_mid = K // 2

        def decoy(name, side, splits):
            pr = next(take)
            self.decoys[name] = {"pair": (int(pr[0]), int(pr[1])), "side": side, "splits": splits}
            return pr

        p, q = decoy("a", "src", ALL)
        self._cell(p, P - 1, K - 1, 0, 0), self._cell(q, P - 1, K - 1, 1, 1)
        p, q = decoy("b", "src", ALL)
        self._cell(p, 1, 0, 0, 0), self._cell(q, 1, 0, 1, 1)
        p, q = decoy("c", "src", ALL)
        self._cell(p, p, k_mid, 1, 1), self._cell(q, p, k_mid, 0, 0)
        if P % 64:
            p, q = decoy("d", "both", NONE)
            self.tail["in"].append(p), self.tail["eg"].append(p)
        # e: a destination pair under the same non-VALID status with different bits, and a source pair that differs there
        d1, d2 = decoy("e_dst", "dst", NONE)
        self.status[[d1, d2], k_mid] = _lib.JOB_BAD_NAMED_PORT
        self._in[d1, k_mid], self._in[d2, k_mid] = 1, 0
        self._eg[:, k_mid, d1], self._eg[:, k_mid, d2] = 0, 1
        p, q = decoy("e", "src", NONE)
        self._in[d1, k_mid, p], self._eg[p, k_mid, d1], self._in[d1, k_mid, q], self._eg[q, k_mid, d1] = 1, 1, 0, 0
        p, q = decoy("f", "src", {"ingress": True, "egress": False, "combined": False})
        self._cell(p, free[0], k_mid, 1, 0), self._cell(q, free[0], k_mid, 0, 0)
        p, q = decoy("fe", "src", {"ingress": False, "egress": True, "combined": False})
        self._cell(p, free[1], k_mid, 0, 1), self._cell(q, free[1], k_mid, 0, 0)
        d1, d2 = decoy("g", "dst", {"ingress": True, "egress": False, "combined": True})
        self.status[d1, k_mid], self.status[d2, k_mid] = _lib.JOB_BAD_NAMED_PORT, _lib.JOB_BAD_PORT_PROTOCOL
        d1, d2 = decoy("h", "dst", ALL)
        self.status[d1, k_mid], self.status[d2, k_mid] = _lib.JOB_NONE, _lib.JOB_VALID
        self._in[d2, k_mid], self._eg[:, k_mid, d2] = 0, 0

    def cells(self):
        return PlaneCells(self.status, self.ingress, self.egress)

    def torch(self):
        """(status, ingress, egress) as the tensors tests/test_gpu_table_counts._Planes takes."""
        import torch

        return (torch.from_numpy(self.status.copy()), torch.from_numpy(self.ingress.view(np.int64).copy()),
                torch.from_numpy(self.egress.view(np.int64).copy()))

    def check_decoys(self, view, classes, ctx=""):
        """Every decoy pair is split, or not, as its verdict says (classes: the dict a classes() call returns)."""
        for name, dc in self.decoys.items():
            p, q = dc["pair"]
            for side in ("src", "dst") if dc["side"] == "both" else (dc["side"],):
                if side in classes:
                    split = bool(classes[side][p] != classes[side][q])
                    assert split == dc["splits"][view], f"{ctx} decoy {name} pods {p}, {q} as {side} under {view}: split {split}"
