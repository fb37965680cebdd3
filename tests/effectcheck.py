"""Oracle tally for cyc_probe_target_effects — TEST HELPER.

The job expansion of pkg/connectivity/probe/resources.go:286-364 restated over Resources / probe-config
dicts: `job(res, probes, d, k)` is slot k of destination d (its status and the resolved port, port name and
protocol), `traffic(res, probes, s, d, k)` the matcher.Traffic of the job cell (job.go:81-103).  `Tally` asks
the CPU oracle for the DirectionResult target lists of every VALID cell (Oracle.query_traffic_targets) and for
TargetsApplyingToPod of every pod (Oracle.query_targets), and keeps the four effect counters per (target,
target pod, slot), so any row range and slot range is a slice sum.
"""
from __future__ import annotations

import numpy as np

NONE, VALID, BAD_NAMED_PORT, BAD_PORT_PROTOCOL = 0, 1, 2, 3
ALLOWING, DENYING, SOLE_ALLOWING, SOLE_DENYING = range(4)
DIRECTIONS = ("Ingress", "Egress")


def slots(res, probes):
    """[(probe config, container index | None)] per job slot: an AllAvailable config has one slot per container
    of the pod with the most, a PortProtocol config one."""
    maxc = max((len(p.get("Containers") or []) for p in res["Pods"]), default=0)
    out = []
    for c in probes:
        out += [(c, j) for j in range(maxc)] if c.get("AllAvailable") else [(c, None)]
    return out


def job(res, probes, d, k, _slots=None):
    """(status, ResolvedPort, ResolvedPortName, Protocol) of slot k of destination d."""
    cfg, j = (_slots or slots(res, probes))[k]
    conts = res["Pods"][d].get("Containers") or []
    if j is not None:  # GetJobsAllAvailableServers, resources.go:336-364
        if j >= len(conts):
            return NONE, 0, "", ""
        return VALID, conts[j]["Port"], conts[j]["PortName"], conts[j]["Protocol"]
    port, proto = cfg["Port"], cfg["Protocol"]  # GetJobsForNamedPortProtocol, resources.go:284-334
    if isinstance(port, str):
        hit = next((c for c in conts if c["PortName"] == port), None)
        return (VALID, hit["Port"], port, proto) if hit else (BAD_NAMED_PORT, -1, port, proto)
    hit = next((c for c in conts if c["Port"] == port), None)
    return (VALID, port, hit["PortName"], proto) if hit else (BAD_PORT_PROTOCOL, port, "", proto)


def _end(res, p):
    pod = res["Pods"][p]
    return {"Internal": {"PodLabels": pod.get("Labels"), "NamespaceLabels": (res.get("Namespaces") or {}).get(pod["Namespace"]),
                         "Namespace": pod["Namespace"]}, "IP": pod["IP"]}


def traffic(res, probes, s, d, k, _slots=None):
    """matcher.Traffic of job cell (s, d, k), or None when the slot holds no VALID job."""
    st, port, name, proto = job(res, probes, d, k, _slots)
    if st != VALID:
        return None
    return {"Source": _end(res, s), "Destination": _end(res, d), "ResolvedPort": port, "ResolvedPortName": name, "Protocol": proto}


def primary_keys(oracle):
    """Per direction the targets' primary keys in the library's order (json.Marshal of a Go map: sorted bytes)."""
    pj = oracle.policy_json()
    return [sorted(pj[n] or {}, key=lambda s: s.encode()) for n in DIRECTIONS]


class Tally:
    """The oracle's per-cell target lists over pods rows [row_lo, row_hi) x all pods x all slots.

    eff[dir]      int64 [T, rows, K, 4]   the four counters per target pod of the rows
    applies[dir]  int64 [T, rows]         1 where the target applies to the pod
    allowed[dir]  bool  [rows, P, K]      DirectionResult.IsAllowed per VALID cell (target pod, other pod, slot)
    appliers[dir], allowers[dir]  int [rows, P, K]  targets in either list, in AllowingTargets, per cell
    multi[dir]    cells with two or more allowing targets
    """

    def __init__(self, oracle, res, probes, row_lo=0, row_hi=None, directions=(0, 1)):
        P = len(res["Pods"])
        row_hi = P if row_hi is None else row_hi
        sl = slots(res, probes)
        K = len(sl)
        self.P, self.K, self.row_lo, self.row_hi = P, K, row_lo, row_hi
        self.keys = primary_keys(oracle)
        index = [{k: i for i, k in enumerate(ks)} for ks in self.keys]
        rows = row_hi - row_lo
        self.status = np.array([[job(res, probes, d, k, sl)[0] for k in range(K)] for d in range(P)], np.uint8).reshape(P, K)
        self.eff = [np.zeros((len(ks), rows, K, 4), np.int64) for ks in self.keys]
        self.applies = [np.zeros((len(ks), rows), np.int64) for ks in self.keys]
        self.allowed = [np.zeros((rows, P, K), bool) for _ in DIRECTIONS]
        self.appliers = [np.zeros((rows, P, K), np.int32) for _ in DIRECTIONS]
        self.allowers = [np.zeros((rows, P, K), np.int32) for _ in DIRECTIONS]
        pods = [{"Namespace": res["Pods"][p]["Namespace"], "Labels": res["Pods"][p].get("Labels")} for p in range(row_lo, row_hi)]
        for r, got in enumerate(oracle.query_targets(pods) if pods else []):
            for dr in directions:
                for pk in got[DIRECTIONS[dr]]:
                    self.applies[dr][index[dr][pk], r] = 1
        for dr in directions:
            cells, docs = [], []
            for r in range(rows):
                for o in range(P):
                    s, d = (o, row_lo + r) if dr == 0 else (row_lo + r, o)
                    for k in range(K):
                        if self.status[d, k] == VALID:
                            cells.append((r, o, k))
                            docs.append(traffic(res, probes, s, d, k, sl))
            for (r, o, k), got in zip(cells, oracle.query_traffic_targets(docs) if docs else []):
                g = got[DIRECTIONS[dr]]
                al, de = g["AllowingTargets"], g["DenyingTargets"]
                self.allowed[dr][r, o, k] = g["IsAllowed"]
                for pk in al:
                    self.eff[dr][index[dr][pk], r, k, ALLOWING] += 1
                for pk in de:
                    self.eff[dr][index[dr][pk], r, k, DENYING] += 1
                if len(al) == 1 and de:
                    self.eff[dr][index[dr][al[0]], r, k, SOLE_ALLOWING] += 1
                if len(de) == 1 and not al:
                    self.eff[dr][index[dr][de[0]], r, k, SOLE_DENYING] += 1
                self.appliers[dr][r, o, k] = len(al) + len(de)
                self.allowers[dr][r, o, k] = len(al)
        self.multi = [int((a >= 2).sum()) for a in self.allowers]

    def effects(self, dr, row_lo=None, row_hi=None, k_lo=0, k_hi=None):
        """(effects [T, nk, 4], applies [T]) of rows [row_lo, row_hi) and slots [k_lo, k_hi)."""
        lo = (self.row_lo if row_lo is None else row_lo) - self.row_lo
        hi = (self.row_hi if row_hi is None else row_hi) - self.row_lo
        k_hi = self.K if k_hi is None else k_hi
        assert 0 <= lo <= hi <= self.row_hi - self.row_lo
        return self.eff[dr][:, lo:hi, k_lo:k_hi].sum(axis=1), self.applies[dr][:, lo:hi].sum(axis=1)
