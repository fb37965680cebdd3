"""connectivity.ComparisonTable (pkg/connectivity/comparisontable.go) over two lazy probe.Tables.

    kube = ...        # the observed probe.Table
    simulated = runner.run_probe_for_config(config, resources)
    ct = ComparisonTable(kube, simulated)
    ct.value_counts(ignore_loopback=True)      # {"same": .., "different": .., "ignored": ..}
    print(ct.render_success_table())

The reference builds one Item {Kube, Simulated} per (from, to) pair and walks them
(comparisontable.go:46-67); here the two tables' cells sources compare their Combined codes whole
(`compare`: cyc_table_compare on the device for DeviceTables, numpy for probe.PlaneCells) and this
class only turns the counts into the reference's maps.  The two tables must answer the same jobs:
the same pods in the same order and the same probe config slots.
"""
from __future__ import annotations

import numpy as np

from ._lib import CyclonusPanic
from .probe import _CONN, Table
from .tablewriter import render

# comparisontable.go:136-155
SAME, DIFFERENT, IGNORED = "same", "different", "ignored"
COMPARISONS = (SAME, DIFFERENT, IGNORED)
SHORT = {SAME: ".", DIFFERENT: "X", IGNORED: "?"}
PROTOCOLS = ("TCP", "SCTP", "UDP")  # the protocols ValueCountsByProtocol has maps for (:90)


def short_string(c: str) -> str:
    if c not in SHORT:
        raise CyclonusPanic(0, f"invalid Comparison value {c}")
    return SHORT[c]


class ComparisonTable:
    """NewComparisonTableFrom(kubeProbe, simulatedProbe) (comparisontable.go:46-67)."""

    def __init__(self, kube: Table, simulated: Table):
        # Froms and Tos of a probe.Table are both its sorted pod names (table.go:38-48)
        if len(kube.items) != len(simulated.items):
            raise CyclonusPanic(0, "cannot compare tables of different dimensions")
        for what in ("from", "to"):
            for i, name in enumerate(kube.items):
                if simulated.items[i] != name:
                    raise CyclonusPanic(0, f"cannot compare: {what} keys at index {i} do not match ({simulated.items[i]} vs {name})")
        # the cells sources are compared slot by slot, in plane order
        if [p.pod_string() for p in kube.resources.pods] != [p.pod_string() for p in simulated.resources.pods]:
            raise ValueError("the tables' planes hold the pods in different orders")
        if len(kube.slots) != len(simulated.slots) or kube.slots.start != simulated.slots.start:
            raise ValueError("the tables answer different job slots")
        for d in range(len(kube.resources.pods)):
            for j in range(min(len(kube.slots), len(kube.resources.pods[d].containers) if kube.config.all_available else 1)):
                if kube._job_key(d, j) != simulated._job_key(d, j):
                    raise ValueError(f"the tables answer different jobs for {kube.resources.pods[d].pod_string()}")
        self.kube, self.simulated = kube, simulated
        self.items = kube.items
        self._cmp = {}

    def _compare(self, ignore_loopback: bool, want_diff: bool = False):
        key = (bool(ignore_loopback), want_diff)
        if key not in self._cmp:
            k = self.kube.slots
            self._cmp[key] = self.kube.src.compare(self.simulated.src, k.start, k.stop, bool(ignore_loopback), want_diff=want_diff)
        return self._cmp[key]

    def _protocol(self, d: int, j: int) -> str:
        """Job.Protocol of destination d's job in slot j (resources.go:284-364)."""
        if self.kube.config.all_available:
            return self.kube.resources.pods[d].containers[j].protocol
        return self.kube.config.protocol

    def _by_protocol(self, dst):
        """dst[P, k, 3] summed over the jobs of each protocol: {protocol: [same, different, ignored]}."""
        out = {}
        for d, j in zip(*np.nonzero(dst.sum(axis=2))):
            p = self._protocol(int(d), int(j))
            out[p] = out.get(p, np.zeros(3, np.int64)) + dst[d, j]
        return out

    def value_counts(self, ignore_loopback: bool) -> dict:  # :109-123
        pairs = self._compare(ignore_loopback)["pairs"]
        return {c: int(n) for c, n in zip(COMPARISONS, pairs) if n}

    def results_by_protocol(self) -> dict:  # :69-79 over Item.ResultsByProtocol :14-20
        counts = {True: {}, False: {}}
        for p, v in self._by_protocol(self._compare(False)["dst"]).items():
            for ok, n in ((True, v[0]), (False, v[1])):
                if n:
                    counts[ok][p] = int(n)
        return counts

    def value_counts_by_protocol(self, ignore_loopback: bool) -> dict:  # :89-107
        counts = {p: {} for p in PROTOCOLS}
        for p, v in self._by_protocol(self._compare(ignore_loopback)["dst"]).items():
            if p not in counts:
                raise CyclonusPanic(0, "assignment to entry in nil map")
            counts[p] = {c: int(n) for c, n in zip(COMPARISONS, v) if n}
        return counts

    def _by_namespace(self, what: str, ignore_loopback: bool) -> dict:
        """The cells sources' group_compare (cyc_table_group_compare on the device for DeviceTables) with the pods'
        namespaces as groups: {(namespace from, namespace to): {comparison: count}}, zero counts left out."""
        names, groups = self.kube._namespaces()
        if not names:
            return {}
        k = self.kube.slots
        c = self.kube.src.group_compare(self.simulated.src, groups, len(names), k.start, k.stop, bool(ignore_loopback))[what]
        if what == "slots":
            c = c.sum(axis=2)
        return {(fr, to): {x: int(n) for x, n in zip(COMPARISONS, c[i, j]) if n} for i, fr in enumerate(names) for j, to in enumerate(names)}

    def value_counts_by_namespace(self, ignore_loopback: bool = False) -> dict:
        """value_counts (the (from, to) pairs) per pair of namespaces; an ignored loopback pair lies in (ns, ns)."""
        return self._by_namespace("pairs", ignore_loopback)

    def job_counts_by_namespace(self, ignore_loopback: bool = False) -> dict:
        """The per-job counts of value_counts_by_protocol, summed over the jobs, per pair of namespaces."""
        return self._by_namespace("slots", ignore_loopback)

    def _by_pod(self, what: str, ignore_loopback: bool) -> dict:
        """The cells sources' pod_compare (cyc_table_pod_compare on the device for DeviceTables):
        {pod: {"as_source": {comparison: count}, "as_destination": {...}}}, zero counts left out."""
        k = self.kube.slots
        c = self.kube.src.pod_compare(self.simulated.src, k.start, k.stop, bool(ignore_loopback))
        src, dst = c["src_" + what], c["dst_" + what]
        if what == "slots":
            src, dst = src.sum(axis=1), dst.sum(axis=1)
        tally = lambda row: {x: int(n) for x, n in zip(COMPARISONS, row) if n}  # noqa: E731
        return {p.pod_string(): {"as_source": tally(src[i]), "as_destination": tally(dst[i])}
                for i, p in enumerate(self.kube.resources.pods)}

    def value_counts_by_pod(self, ignore_loopback: bool = False) -> dict:
        """value_counts (the (from, to) pairs) per pod, as the pairs' source and as their destination: where the
        differences sit (an egress-side fault shows on the source, an ingress-side one on the destination)."""
        return self._by_pod("pairs", ignore_loopback)

    def job_counts_by_pod(self, ignore_loopback: bool = False) -> dict:
        """The per-job counts of value_counts_by_protocol, summed over the jobs, per pod."""
        return self._by_pod("slots", ignore_loopback)

    def different_jobs(self, ignore_loopback: bool, limit=None):
        """Yield (from, to, job key, kube Combined, simulated Combined) for every job counted as `different`
        (Item.ResultsByProtocol :14-20 under the loopback rule of :89-107), at most `limit` of them, in plane order
        (pod order, then job slots).  The simulated value is None where the simulated table lacks the job.  The
        cells sources list them (`compare_find`: cyc_table_compare_find on the device for DeviceTables)."""
        k, pods, n = self.kube.slots, self.kube.resources.pods, 0
        for page in self.kube.src.compare_find_all(self.simulated.src, k.start, k.stop, bool(ignore_loopback)):
            for r in page:
                if limit is not None and n >= limit:
                    return
                d, other = int(r["d"]), int(r["other"])
                yield (pods[int(r["s"])].pod_string(), pods[d].pod_string(), self.kube._job_key(d, int(r["k"]) - k.start),
                       _CONN[int(r["combined"])], _CONN.get(other))
                n += 1

    def differs(self) -> np.ndarray:
        """bool [P, P] in plane order: [s, d] = not Item(s, d).IsSuccess() (:22-36)."""
        diff = self._compare(False, True)["diff"]
        diff = np.ascontiguousarray(diff.cpu().numpy() if hasattr(diff, "cpu") else diff).view(np.uint64)
        P = len(self.kube.resources.pods)
        s = np.arange(P)
        return ((diff[:, s // 64] >> (s % 64).astype(np.uint64)) & np.uint64(1)).astype(bool).T

    def render_success_table(self) -> str:  # :125-134 through TruthTable.Table (truthtable.go:101-117)
        x = self.differs()
        at = [self.kube.index[name] for name in self.items]
        rows = [[fr] + ["X" if x[at[i], at[j]] else "." for j in range(len(self.items))] for i, fr in enumerate(self.items)]
        return render([""] + self.items, rows, row_line=False)
