"""Host-side mirror of the reference's pkg/connectivity/probe simulated path, on libcyclonus_hip.

    runner = new_simulated_runner(policy)                          # jobrunner.go:17-19
    table = runner.run_probe_for_config(new_probe_config(80, "TCP"), resources)   # :29-31
    print(table.render_table())                                    # table.go:66-68

`Table` is a lazy view over the packed verdict planes (it never materialises the P^2 Item
maps of truthtable.go:28-48); `Table.get(from, to)` builds one Item on demand.  Job keys,
statuses and the Connectivity values follow job.go:23-25 and jobrunner.go:33-94.
"""
from __future__ import annotations

import json
from dataclasses import dataclass, field
from typing import Dict, List, Optional

import numpy as np

from . import _lib
from .engine import Engine
from .matcher import Policy, _traffic_json
from .tablewriter import render

# connectivity.go:7-14 and ShortString :27-42
UNKNOWN, CHECK_FAILED, INVALID_NAMED_PORT, INVALID_PORT_PROTOCOL, BLOCKED, ALLOWED = (
    "unknown", "checkfailed", "invalidnamedport", "invalidportprotocol", "blocked", "allowed")
SHORT = {UNKNOWN: "?", CHECK_FAILED: "!", BLOCKED: "X", ALLOWED: ".", INVALID_NAMED_PORT: "P", INVALID_PORT_PROTOCOL: "N"}


def short_string(c: str) -> str:
    if c not in SHORT:
        raise ValueError(f"invalid Connectivity value: {c}")
    return SHORT[c]


# ----------------------------------------------------------------------------- model
@dataclass
class Container:  # pod.go:173-179
    name: str
    port: int
    protocol: str
    port_name: str

    def to_json(self):
        return {"Name": self.name, "Port": self.port, "Protocol": self.protocol, "PortName": self.port_name}


@dataclass
class Pod:  # pod.go:44-51
    namespace: str
    name: str
    labels: Optional[Dict[str, str]]
    ip: str
    containers: List[Container] = field(default_factory=list)

    def pod_string(self) -> str:  # podstring.go:11-14
        return f"{self.namespace}/{self.name}"

    def to_json(self):
        return {"Namespace": self.namespace, "Name": self.name, "Labels": self.labels, "IP": self.ip,
                "Containers": [c.to_json() for c in self.containers]}


@dataclass
class Resources:  # resources.go:15-19
    namespaces: Dict[str, Optional[Dict[str, str]]]
    pods: List[Pod]

    @staticmethod
    def from_json(doc) -> "Resources":
        doc = json.loads(doc) if isinstance(doc, (str, bytes)) else doc
        pods = [Pod(p.get("Namespace", ""), p.get("Name", ""), p.get("Labels"), p.get("IP", ""),
                    [Container(c.get("Name", ""), int(c.get("Port", 0)), c.get("Protocol", ""), c.get("PortName", ""))
                     for c in p.get("Containers") or []]) for p in doc.get("Pods") or []]
        return Resources(dict(doc.get("Namespaces") or {}), pods)

    def to_json(self):
        return {"Namespaces": self.namespaces, "Pods": [p.to_json() for p in self.pods]}

    def sorted_pod_names(self) -> List[str]:  # resources.go:223-230
        return sorted(p.pod_string() for p in self.pods)


@dataclass
class ProbeConfig:  # generator/testcase.go:139-156
    all_available: bool = False
    port: Optional[object] = None  # int or str (intstr.IntOrString)
    protocol: str = ""

    def to_json(self):
        if self.all_available:
            return {"AllAvailable": True}
        return {"Port": self.port, "Protocol": self.protocol}


def new_probe_config(port, protocol) -> ProbeConfig:
    return ProbeConfig(False, port, protocol)


def new_all_available() -> ProbeConfig:
    return ProbeConfig(True)


def _as_resources(r) -> Resources:
    return r if isinstance(r, Resources) else Resources.from_json(r)


def _as_probe(c) -> ProbeConfig:
    if isinstance(c, ProbeConfig):
        return c
    if c.get("AllAvailable"):
        return ProbeConfig(True)
    pp = c.get("PortProtocol", c)
    return ProbeConfig(False, pp.get("Port"), pp.get("Protocol", ""))


@dataclass
class JobResult:  # job.go:16-25
    key: str
    ingress: str
    egress: str
    combined: str


@dataclass
class Item:  # table.go:10-23
    from_: str
    to: str
    job_results: Dict[str, JobResult]


# ----------------------------------------------------------------------------- table view
_CONN = {_lib.CONN_UNKNOWN: UNKNOWN, _lib.CONN_CHECK_FAILED: CHECK_FAILED, _lib.CONN_INVALID_NAMED_PORT: INVALID_NAMED_PORT,
         _lib.CONN_INVALID_PORT_PROTOCOL: INVALID_PORT_PROTOCOL, _lib.CONN_BLOCKED: BLOCKED, _lib.CONN_ALLOWED: ALLOWED}


class PlaneCells:
    """Cells source over packed planes held on the host (status[P,K], ingress[P,K,W], egress[P,K,W]),
    e.g. the oracle's: the same Connectivity mapping as cyc_table_cells (jobrunner.go:36-55,85-93)."""

    def __init__(self, status, ingress, egress):
        self.status, self.ingress, self.egress = status, ingress, egress

    def cells(self, s_lo, s_hi, d_lo, d_hi, k_lo, k_hi, want=("ingress", "egress", "combined")):
        s = np.arange(s_lo, s_hi)[:, None, None]
        d = np.arange(d_lo, d_hi)[None, :, None]
        k = np.arange(k_lo, k_hi)[None, None, :]
        st = self.status[d, k]
        ai = ((self.ingress[d, k, s // 64] >> (s % 64).astype(np.uint64)) & np.uint64(1)).astype(bool)
        ae = ((self.egress[s, k, d // 64] >> (d % 64).astype(np.uint64)) & np.uint64(1)).astype(bool)
        valid, bpp, bnp = st == _lib.JOB_VALID, st == _lib.JOB_BAD_PORT_PROTOCOL, st == _lib.JOB_BAD_NAMED_PORT
        inv = np.where(bpp, _lib.CONN_INVALID_PORT_PROTOCOL, np.where(bnp, _lib.CONN_INVALID_NAMED_PORT, _lib.CONN_NO_JOB))
        allowed = lambda b: np.where(b, _lib.CONN_ALLOWED, _lib.CONN_BLOCKED)  # noqa: E731
        out = {"ingress": np.where(valid, allowed(ai), inv),
               "egress": np.where(valid, allowed(ae), np.where(bpp | bnp, _lib.CONN_UNKNOWN, _lib.CONN_NO_JOB)),
               "combined": np.where(valid, allowed(ai & ae), inv)}
        return {n: np.broadcast_to(out[n], (s_hi - s_lo, d_hi - d_lo, k_hi - k_lo)).astype(np.uint8) for n in want}

    # The whole-table consumers, cell by cell (the restatement cyc_table_counts / cyc_table_compare are
    # tested against; sources go through in chunks so the code arrays stay small).
    SOURCE_CHUNK = 64

    def _source_chunks(self):
        P = self.status.shape[0]
        return P, [(lo, min(lo + self.SOURCE_CHUNK, P)) for lo in range(0, P, self.SOURCE_CHUNK)]

    def counts(self, k_lo=0, k_hi=None, want=("ingress", "egress", "combined", "no_job")):
        """cyc_table_counts: {name: i64 [k, 6]} cells per Connectivity code, "no_job": cells without a job."""
        k_hi = self.status.shape[1] if k_hi is None else k_hi
        P, chunks = self._source_chunks()
        out = {n: np.zeros((max(k_hi - k_lo, 0), 6), np.int64) for n in ("ingress", "egress", "combined")}
        no_job = 0
        for lo, hi in chunks:
            cells = self.cells(lo, hi, 0, P, k_lo, k_hi)
            for n, codes in cells.items():
                for c in range(6):
                    out[n][:, c] += (codes == c).sum(axis=(0, 1))
            no_job += int((cells["combined"] == _lib.CONN_NO_JOB).sum())
        out["no_job"] = no_job
        return {n: out[n] for n in want}

    def compare(self, other, k_lo=0, k_hi=None, ignore_loopback=False, want_diff=False):
        """cyc_table_compare(self, other): Combined of self (the kube probe) against Combined of other:
        {"pairs": [3], "slots": [k, 3], "dst": [P, k, 3]} in (same, different, ignored) order
        (comparisontable.go:14-36,89-123), with want_diff "diff": u64 [P, W], row d bit s = the Items (s, d) differ."""
        k_hi = self.status.shape[1] if k_hi is None else k_hi
        P, chunks = self._source_chunks()
        if other.status.shape != self.status.shape:
            raise ValueError("cannot compare tables of different shapes")
        nk = max(k_hi - k_lo, 0)
        pairs, dst = np.zeros(3, np.int64), np.zeros((P, nk, 3), np.int64)
        diff = np.zeros((P, (P + 63) // 64), np.uint64)
        for lo, hi in chunks:
            ca = self.cells(lo, hi, 0, P, k_lo, k_hi, want=("combined",))["combined"]
            cb = other.cells(lo, hi, 0, P, k_lo, k_hi, want=("combined",))["combined"]
            loopback = (np.arange(lo, hi)[:, None] == np.arange(P)[None, :]) & bool(ignore_loopback)
            job = ca != _lib.CONN_NO_JOB  # every job of the kube Item, once
            ignored = job & loopback[:, :, None]
            same = job & ~ignored & (ca == cb)
            different = job & ~ignored & (ca != cb)  # (a job the other table lacks included)
            for x, m in enumerate((same, different, ignored)):
                dst[:, :, x] += m.sum(axis=0)
            item_differs = (ca != cb).any(axis=2)  # equalsDict over the job keys, NO_JOB included
            pairs += [int((~loopback & ~item_differs).sum()), int((~loopback & item_differs).sum()), int(loopback.sum())]
            s, d = np.nonzero(item_differs)
            np.bitwise_or.at(diff, (d, (s + lo) // 64), np.uint64(1) << ((s + lo) % 64).astype(np.uint64))
        out = {"pairs": pairs, "slots": dst.sum(axis=0), "dst": dst}
        if want_diff:
            out["diff"] = diff
        return out

    # The same two split by pod group pair (cyc_table_group_counts / cyc_table_group_compare), cell by cell:
    # what DeviceTable.group_counts / group_compare are tested against.
    def _groups(self, groups, n_groups):
        P = self.status.shape[0]
        g = np.asarray(groups, np.int64)
        if g.shape != (P,):
            raise ValueError(f"groups must hold one group id per pod ({P}), got shape {g.shape}")
        G = int(g.max(initial=-1)) + 1 if n_groups is None else int(n_groups)
        if G < 1:
            raise _lib.CyclonusError(_lib.ERR_ARG, "n_groups must be at least 1")
        bad = np.nonzero((g < -1) | (g >= G))[0]
        if len(bad):
            raise _lib.CyclonusError(_lib.ERR_ARG, f"group_of[{bad[0]}] = {g[bad[0]]} is neither -1 nor a group in [0, {G})")
        return g, G

    def _group_index(self, g, lo, hi, nk):
        """For the cells [lo:hi, P, nk] of a source chunk: which have both pods in a group, and their (source
        group, destination group, slot) indices, each broadcast to the chunk's shape."""
        shape = (hi - lo, len(g), nk)
        gs, gd, kk = g[lo:hi, None, None], g[None, :, None], np.arange(nk)[None, None, :]
        return (np.broadcast_to((gs >= 0) & (gd >= 0), shape), np.broadcast_to(gs, shape), np.broadcast_to(gd, shape),
                np.broadcast_to(kk, shape))

    def group_counts(self, groups, n_groups=None, k_lo=0, k_hi=None, want=("ingress", "egress", "combined", "no_job")):
        """cyc_table_group_counts: {name: i64 [G, G, k, 6]} cells per (source group, destination group, slot,
        Connectivity code), "no_job": i64 [G, G].  groups: a group id per pod, -1 = the pod is left out."""
        k_hi = self.status.shape[1] if k_hi is None else k_hi
        g, G = self._groups(groups, n_groups)
        P, chunks = self._source_chunks()
        nk = max(k_hi - k_lo, 0)
        out = {n: np.zeros((G, G, nk, 6), np.int64) for n in ("ingress", "egress", "combined")}
        out["no_job"] = np.zeros((G, G), np.int64)
        for lo, hi in chunks:
            cells = self.cells(lo, hi, 0, P, k_lo, k_hi)
            keep, gs, gd, kk = self._group_index(g, lo, hi, nk)
            for n, codes in cells.items():
                job = keep & (codes != _lib.CONN_NO_JOB)
                np.add.at(out[n], (gs[job], gd[job], kk[job], codes[job]), 1)
            none = keep & (cells["combined"] == _lib.CONN_NO_JOB)
            np.add.at(out["no_job"], (gs[none], gd[none]), 1)
        return {n: out[n] for n in want}

    def group_compare(self, other, groups, n_groups=None, k_lo=0, k_hi=None, ignore_loopback=False):
        """cyc_table_group_compare(self, other): {"pairs": i64 [G, G, 3], "slots": i64 [G, G, k, 3]} in (same,
        different, ignored) order: compare's pairs and per-job counts by (source group, destination group)."""
        k_hi = self.status.shape[1] if k_hi is None else k_hi
        if other.status.shape != self.status.shape:
            raise _lib.CyclonusError(_lib.ERR_ARG, "cannot compare tables of different devices, shapes, partitions or rows")
        g, G = self._groups(groups, n_groups)
        P, chunks = self._source_chunks()
        nk = max(k_hi - k_lo, 0)
        pairs, slots = np.zeros((G, G, 3), np.int64), np.zeros((G, G, nk, 3), np.int64)
        for lo, hi in chunks:
            ca = self.cells(lo, hi, 0, P, k_lo, k_hi, want=("combined",))["combined"]
            cb = other.cells(lo, hi, 0, P, k_lo, k_hi, want=("combined",))["combined"]
            keep, gs, gd, kk = self._group_index(g, lo, hi, nk)
            loopback = (np.arange(lo, hi)[:, None] == np.arange(P)[None, :]) & bool(ignore_loopback)
            job = keep & (ca != _lib.CONN_NO_JOB)  # every job of the kube Item, once
            ignored = job & loopback[:, :, None]
            for x, m in enumerate((job & ~ignored & (ca == cb), job & ~ignored & (ca != cb), ignored)):
                np.add.at(slots, (gs[m], gd[m], kk[m], x), 1)
            item_differs = (ca != cb).any(axis=2)  # equalsDict over the job keys, NO_JOB included
            keep, gs, gd, _ = (a[:, :, 0] for a in self._group_index(g, lo, hi, 1))
            for x, m in enumerate((~loopback & ~item_differs, ~loopback & item_differs, loopback)):
                m = m & keep
                np.add.at(pairs, (gs[m], gd[m], x), 1)
        return {"pairs": pairs, "slots": slots}

    # The pod level (cyc_table_pod_counts / cyc_table_pod_compare), cell by cell: what DeviceTable.pod_counts /
    # pod_compare are tested against.
    def pod_counts(self, view, k_lo=0, k_hi=None, want=("src", "dst")):
        """cyc_table_pod_counts: {"src": i64 [P, k, 7], "dst": i64 [P, k, 7]} cells per (source, slot, code) over
        every destination and per (destination, slot, code) over every source; column 6: cells without a job."""
        view = {v: n for n, v in _lib.VIEWS.items()}.get(view, view)
        if view not in _lib.VIEWS:
            raise _lib.CyclonusError(_lib.ERR_ARG, "unknown view")
        k_hi = self.status.shape[1] if k_hi is None else k_hi
        P, chunks = self._source_chunks()
        nk = max(k_hi - k_lo, 0)
        out = {"src": np.zeros((P, nk, _lib.POD_CODES), np.int64), "dst": np.zeros((P, nk, _lib.POD_CODES), np.int64)}
        for lo, hi in chunks:
            codes = self.cells(lo, hi, 0, P, k_lo, k_hi, want=(view,))[view]
            for c in range(_lib.POD_CODES):
                m = codes == (c if c < 6 else _lib.CONN_NO_JOB)
                out["src"][lo:hi, :, c] = m.sum(axis=1)
                out["dst"][:, :, c] += m.sum(axis=0)
        return {n: out[n] for n in want}

    def pod_compare(self, other, k_lo=0, k_hi=None, ignore_loopback=False):
        """cyc_table_pod_compare(self, other): {"src_pairs": [P, 3], "dst_pairs": [P, 3], "src_slots": [P, k, 3],
        "dst_slots": [P, k, 3]} in (same, different, ignored) order: compare's pairs and per-job counts by pod."""
        k_hi = self.status.shape[1] if k_hi is None else k_hi
        if other.status.shape != self.status.shape:
            raise _lib.CyclonusError(_lib.ERR_ARG, "cannot compare tables of different devices, shapes, partitions or rows")
        P, chunks = self._source_chunks()
        nk = max(k_hi - k_lo, 0)
        out = {"src_pairs": np.zeros((P, 3), np.int64), "dst_pairs": np.zeros((P, 3), np.int64),
               "src_slots": np.zeros((P, nk, 3), np.int64), "dst_slots": np.zeros((P, nk, 3), np.int64)}
        for lo, hi in chunks:
            ca = self.cells(lo, hi, 0, P, k_lo, k_hi, want=("combined",))["combined"]
            cb = other.cells(lo, hi, 0, P, k_lo, k_hi, want=("combined",))["combined"]
            loopback = (np.arange(lo, hi)[:, None] == np.arange(P)[None, :]) & bool(ignore_loopback)
            job = ca != _lib.CONN_NO_JOB  # every job of the kube Item, once
            ignored = job & loopback[:, :, None]
            for x, m in enumerate((job & ~ignored & (ca == cb), job & ~ignored & (ca != cb), ignored)):
                out["src_slots"][lo:hi, :, x] = m.sum(axis=1)
                out["dst_slots"][:, :, x] += m.sum(axis=0)
            item_differs = (ca != cb).any(axis=2)  # equalsDict over the job keys, NO_JOB included
            for x, m in enumerate((~loopback & ~item_differs, ~loopback & item_differs, loopback)):
                out["src_pairs"][lo:hi, x] = m.sum(axis=1)
                out["dst_pairs"][:, x] += m.sum(axis=0)
        return out

    # The listings (cyc_table_find / cyc_table_compare_find), cell by cell: the same contract as
    # DeviceTable.find / compare_find, which are tested against this restatement.
    def _page(self, matcher, k_lo, k_hi, s_from, cap):
        """matcher(lo, hi, k_lo, k_hi) -> (codes {name: [s, d, k]}, match bool [s, d, k], other u8 [s, d, k] or None)
        for sources [lo, hi).  cap None: pods * slots; cap 0: the count-only call."""
        P, K = self.status.shape
        k_hi = K if k_hi is None else k_hi
        s_from = 0 if s_from is None else s_from
        if not 0 <= k_lo <= k_hi <= K:
            raise _lib.CyclonusError(_lib.ERR_ARG, "slot range out of bounds")
        if not 0 <= s_from <= P:
            raise _lib.CyclonusError(_lib.ERR_ARG, "s_from outside the table's rows")
        nk, count_only = k_hi - k_lo, cap == 0
        cap = max(P * nk, 1) if cap is None else cap
        if cap < 0:
            raise _lib.CyclonusError(_lib.ERR_ARG, "negative cap")
        empty = np.zeros(0, _lib.CELL_DTYPE)
        if nk == 0:
            return empty, (s_from if count_only else P), 0
        pages, n, total, s_next, fits, first = [], 0, 0, s_from, not count_only, 0
        for lo in range(s_from, P, self.SOURCE_CHUNK):
            hi = min(lo + self.SOURCE_CHUNK, P)
            codes, match, other = matcher(lo, hi, k_lo, k_hi)
            per_source = match.sum(axis=(1, 2))
            total += int(per_source.sum())
            if lo == s_from:
                first = int(per_source[0])
            if not fits:
                continue
            for c in per_source:  # the longest run of sources whose records fit
                if n + int(c) > cap:
                    fits = False
                    break
                n, s_next = n + int(c), s_next + 1
            s, d, k = np.nonzero(match[:s_next - lo])  # (row-major: ascending (s, d, k))
            page = np.zeros(len(s), _lib.CELL_DTYPE)
            page["s"], page["d"], page["k"] = s + lo, d, k + k_lo
            for name in ("ingress", "egress", "combined"):
                page[name] = codes[name][s, d, k]
            if other is not None:
                page["other"] = other[s, d, k]
            pages.append(page)
        if not count_only and s_next == s_from and s_from < P:
            e = _lib.CyclonusError(_lib.ERR_ARG, f"source {s_from} alone has {first} matching cells, more than cap {cap}")
            e.total = total
            raise e
        return (np.concatenate(pages) if pages else empty), s_next, total

    def find(self, view, codes, k_lo=0, k_hi=None, s_from=None, cap=None):
        """cyc_table_find over host planes -> (records, s_next, total)."""
        view = {v: n for n, v in _lib.VIEWS.items()}.get(view, view)
        if view not in _lib.VIEWS:
            raise _lib.CyclonusError(_lib.ERR_ARG, "unknown view")
        mask = _lib.code_mask(codes)
        if not mask or mask >> 6:
            raise _lib.CyclonusError(_lib.ERR_ARG, "code_mask must name codes 0..5")
        wanted = np.zeros(256, bool)  # (CYC_CONN_NO_JOB is not a job and never matches)
        wanted[[c for c in range(6) if (mask >> c) & 1]] = True
        P = self.status.shape[0]

        def matcher(lo, hi, k0, k1):
            cells = self.cells(lo, hi, 0, P, k0, k1)
            return cells, wanted[cells[view]], None
        return self._page(matcher, k_lo, k_hi, s_from, cap)

    def compare_find(self, other, k_lo=0, k_hi=None, ignore_loopback=False, s_from=None, cap=None):
        """cyc_table_compare_find(self, other) over host planes: the cells compare counts as `different`."""
        if other.status.shape != self.status.shape:
            raise _lib.CyclonusError(_lib.ERR_ARG, "cannot compare tables of different devices, shapes, partitions or rows")
        P = self.status.shape[0]

        def matcher(lo, hi, k0, k1):
            cells = self.cells(lo, hi, 0, P, k0, k1)
            ca, cb = cells["combined"], other.cells(lo, hi, 0, P, k0, k1, want=("combined",))["combined"]
            loopback = (np.arange(lo, hi)[:, None] == np.arange(P)[None, :]) & bool(ignore_loopback)
            return cells, (ca != _lib.CONN_NO_JOB) & ~loopback[:, :, None] & (ca != cb), cb
        return self._page(matcher, k_lo, k_hi, s_from, cap)

    def find_all(self, view, codes, k_lo=0, k_hi=None, cap=None):
        yield from _lib.pages(lambda s: self.find(view, codes, k_lo, k_hi, s, cap), 0, self.status.shape[0])

    def compare_find_all(self, other, k_lo=0, k_hi=None, ignore_loopback=False, cap=None):
        yield from _lib.pages(lambda s: self.compare_find(other, k_lo, k_hi, ignore_loopback, s, cap), 0, self.status.shape[0])

    # Multi-hop reachability (cyc_table_adjacency / cyc_table_reach): an edge s -> d is a Combined of allowed in some
    # slot of the range, read off the unpacked bits and the status array; then a plain queue per seed set.
    def _edge_pairs(self, k_lo, k_hi):
        """(s, d) of every edge, s-major and without repeats: some slot k of [k_lo, k_hi) has status[d][k] VALID, the
        ingress bit (d, k, s) and the egress bit (s, k, d) set: cells()' Combined == allowed.  The egress words that
        hold no bit are skipped, so sparse planes of many pods stay cheap.  Kept per slot range: the planes of a
        PlaneCells are not expected to change under it."""
        P = self.status.shape[0]
        if not 0 <= k_lo <= k_hi <= self.status.shape[1]:
            raise _lib.CyclonusError(_lib.ERR_ARG, "slot range out of bounds")
        memo = self.__dict__.setdefault("_pairs", {})
        if (k_lo, k_hi) in memo:
            return memo[k_lo, k_hi]
        bit, found = np.arange(64, dtype=np.uint64), [np.zeros(0, np.int64)]
        for k in range(k_lo, k_hi):
            rows, words = np.nonzero(self.egress[:, k, :])
            for lo in range(0, len(rows), 1 << 16):
                r, w = rows[lo:lo + (1 << 16)], words[lo:lo + (1 << 16)]
                i, b = np.nonzero((self.egress[r, k, w][:, None] >> bit) & np.uint64(1))
                s, d = r[i], w[i] * 64 + b
                s, d = s[d < P], d[d < P]  # (plane bits at or beyond P)
                ingress = (self.ingress[d, k, s // 64] >> (s % 64).astype(np.uint64)) & np.uint64(1)
                ok = (self.status[d, k] == _lib.JOB_VALID) & ingress.astype(bool)
                found.append(s[ok] * P + d[ok])
        e = np.unique(np.concatenate(found))
        memo[k_lo, k_hi] = e // max(P, 1), e % max(P, 1)
        return memo[k_lo, k_hi]

    @staticmethod
    def _direction(direction):
        d = _lib.REACH_DIRECTIONS.get(direction, direction)
        if d not in (_lib.REACH_FROM, _lib.REACH_TO):
            raise _lib.CyclonusError(_lib.ERR_ARG, "unknown direction")
        return d

    def adjacency(self, direction="from", k_lo=0, k_hi=None):
        """cyc_table_adjacency: u64 [P, W]; "from": row s bit d, "to": row d bit s set iff there is an edge s -> d."""
        k_hi = self.status.shape[1] if k_hi is None else k_hi
        r, c = self._edge_pairs(k_lo, k_hi)
        if self._direction(direction) == _lib.REACH_TO:
            r, c = c, r
        P = self.status.shape[0]
        out = np.zeros((P, (P + 63) // 64), np.uint64)
        np.bitwise_or.at(out, (r, c // 64), np.uint64(1) << (c % 64).astype(np.uint64))
        return out

    def reach(self, seed_sets, direction="from", k_lo=0, k_hi=None, max_hops=-1, want=("reach", "hops", "levels")):
        """cyc_table_reach: {"reach": u64 [n, W], "hops": i32 [n, P], "levels": i64 [n]} (DeviceTable.reach)."""
        from collections import deque

        k_hi = self.status.shape[1] if k_hi is None else k_hi
        P = self.status.shape[0]
        a, b = self._edge_pairs(k_lo, k_hi)
        if self._direction(direction) == _lib.REACH_TO:
            a, b = b, a  # (a path to a seed is a path from it along the reversed edges)
        off, seeds = _lib.seed_arrays(seed_sets)
        bad = np.nonzero((seeds < 0) | (seeds >= P))[0]
        if len(bad):
            raise _lib.CyclonusError(_lib.ERR_ARG, f"seeds[{bad[0]}] = {seeds[bad[0]]} is not a pod in [0, {P})")
        nbrs = [[] for _ in range(P)]
        for p, q in zip(a.tolist(), b.tolist()):
            nbrs[p].append(q)
        n = len(off) - 1
        hops = np.full((n, P), -1, np.int32)
        for j in range(n):
            h, queue = [-1] * P, deque()
            for p in seeds[off[j]:off[j + 1]].tolist():
                if h[p] < 0:
                    h[p] = 0
                    queue.append(p)
            while queue:
                p = queue.popleft()
                if 0 <= max_hops <= h[p]:
                    continue
                for q in nbrs[p]:
                    if h[q] < 0:
                        h[q] = h[p] + 1
                        queue.append(q)
            hops[j] = h
        reach = np.zeros((n, (P + 63) // 64), np.uint64)
        j, p = np.nonzero(hops >= 0)
        np.bitwise_or.at(reach, (j, p // 64), np.uint64(1) << (p % 64).astype(np.uint64))
        out = {"reach": reach, "hops": hops, "levels": hops.max(axis=1, initial=-1).astype(np.int64)}
        return {x: out[x] for x in want}

    # All pairs (cyc_table_closure / cyc_table_zones): plain Warshall over the packed adjacency rows, a pivot pod a step;
    # the zones by the mutual test on the unpacked matrix.
    def closure(self, direction="from", k_lo=0, k_hi=None, d_out=None, want=("plane", "n_reach")):
        """cyc_table_closure: {"plane": u64 [P, W], "n_reach": i64 [P]} (DeviceTable.closure; d_out belongs to the
        device and is ignored)."""
        k_hi = self.status.shape[1] if k_hi is None else k_hi
        c = self.adjacency(direction, k_lo, k_hi)
        P = c.shape[0]
        p = np.arange(P)
        c[p, p // 64] |= np.uint64(1) << (p % 64).astype(np.uint64)
        for k in range(P):
            through = (c[:, k // 64] >> np.uint64(k % 64)) & np.uint64(1) != 0  # the rows that reach the pivot
            c[through] |= c[k]
        out = {"plane": c, "n_reach": np.unpackbits(c.view(np.uint8), axis=1).sum(axis=1, dtype=np.int64).reshape(P)}
        return {x: out[x] for x in want}

    def zones(self, k_lo=0, k_hi=None, want=("zone", "n_from", "n_to")):
        """cyc_table_zones: {"zone": i32 [P], "n_zones": int, "n_from": i64 [P], "n_to": i64 [P]} (DeviceTable.zones)."""
        P = self.status.shape[0]
        c = self.closure("from", k_lo, k_hi, want=("plane",))["plane"]
        m = np.unpackbits(c.view(np.uint8), axis=1, bitorder="little")[:, :P].astype(bool).reshape(P, P)
        first = (m & m.T).argmax(axis=1) if P else np.zeros(0, np.int64)  # the smallest pod a pod shares its zone with
        heads = np.flatnonzero(first == np.arange(P))
        out = {"zone": np.searchsorted(heads, first).astype(np.int32), "n_zones": len(heads),
               "n_from": m.sum(axis=1, dtype=np.int64), "n_to": m.sum(axis=0, dtype=np.int64)}
        return {x: out[x] for x in out if x in want or (x == "n_zones" and "zone" in want)}

    def zone_graph(self, k_lo=0, k_hi=None, want=("zone", "rep", "size", "tier", "edges"), max_zones=None, max_edges=None):
        """cyc_table_zone_graph: {"zone": i32 [P], "n_zones": int, "rep": i32 [Z], "size": i64 [Z], "tier": i32 [Z],
        "edges": i32 [n, 2], "n_edges": int, "reach": u64 [Z, ceil(Z / 64)]} (DeviceTable.zone_graph; max_zones and
        max_edges belong to the device and are ignored).  The cover edges by a matrix product over the unpacked zone matrix: small P only."""
        P = self.status.shape[0]
        c = self.closure("from", k_lo, k_hi, want=("plane",))["plane"]
        zone = self.zones(k_lo, k_hi, want=("zone",))["zone"]
        m = np.unpackbits(c.view(np.uint8), axis=1, bitorder="little")[:, :P].astype(bool).reshape(P, P)
        heads = np.unique(zone, return_index=True)[1]  # the first pod of every zone, in the order of the zone ids
        Z = len(heads)
        R = m[heads][:, heads]
        S = R & ~np.eye(Z, dtype=bool)
        cover = S & ~((S.astype(np.int32) @ S.astype(np.int32)) > 0)
        # the number of zones that reach a zone orders a strict partial order topologically: tiers by relaxing in it
        tier = np.zeros(Z, np.int32)
        for b in np.argsort(S.sum(axis=0), kind="stable"):
            into = np.flatnonzero(cover[:, b])
            if len(into):
                tier[b] = tier[into].max() + 1
        bits = np.zeros((Z, (Z + 63) // 64 * 64), np.uint8)
        bits[:, :Z] = R
        out = {"zone": zone, "n_zones": Z, "rep": heads.astype(np.int32), "size": np.bincount(zone, minlength=Z).astype(np.int64),
               "tier": tier, "edges": np.argwhere(cover).astype(np.int32).reshape(-1, 2), "n_edges": int(cover.sum()),
               "reach": np.packbits(bits, axis=1, bitorder="little").view(np.uint64).reshape(Z, (Z + 63) // 64)}
        return {x: out[x] for x in out if x in want or x in ("n_zones", "n_edges")}

    # Connectivity classes (cyc_table_classes / cyc_table_cells_at), cell by cell: the pods grouped by the bytes of their
    # row (as sources) or column (as destinations) of the view's cell codes, numbered by first occurrence.
    def classes(self, view="combined", k_lo=0, k_hi=None, want=("src", "dst"), hash_mask=None, stats=False):
        """cyc_table_classes: {"src": i32 [P], "n_src": int, "dst": i32 [P], "n_dst": int} (DeviceTable.classes;
        hash_mask and stats belong to the device's way of getting there and are ignored)."""
        view = {v: n for n, v in _lib.VIEWS.items()}.get(view, view)
        if view not in _lib.VIEWS:
            raise _lib.CyclonusError(_lib.ERR_ARG, "unknown view")
        P, K = self.status.shape
        k_hi = K if k_hi is None else k_hi
        if not 0 <= k_lo <= k_hi <= K:
            raise _lib.CyclonusError(_lib.ERR_ARG, "slot range out of bounds")
        _, chunks = self._source_chunks()
        out = {}
        for side in want:
            seen, cls = {}, np.zeros(P, np.int32)
            for lo, hi in chunks:
                if side == "src":
                    codes = self.cells(lo, hi, 0, P, k_lo, k_hi, want=(view,))[view]  # [pods of the chunk, d, k]
                else:
                    codes = self.cells(0, P, lo, hi, k_lo, k_hi, want=(view,))[view].transpose(1, 0, 2)  # [pods of the chunk, s, k]
                for p in range(lo, hi):
                    cls[p] = seen.setdefault(np.ascontiguousarray(codes[p - lo]).tobytes(), len(seen))
            out[side], out["n_" + side] = cls, len(seen)
        return out

    def cells_at(self, sources, dests, k_lo=0, k_hi=None, want=("ingress", "egress", "combined")):
        """cyc_table_cells_at: {name: u8 [n_s, n_d, k]} for lists of pods."""
        P, K = self.status.shape
        k_hi = K if k_hi is None else k_hi
        s, d = np.asarray(sources, np.int64).reshape(-1), np.asarray(dests, np.int64).reshape(-1)
        for name, x in (("srcs", s), ("dsts", d)):
            bad = np.nonzero((x < 0) | (x >= P))[0]
            if len(bad):
                raise _lib.CyclonusError(_lib.ERR_ARG, f"{name}[{bad[0]}] = {x[bad[0]]} is not a pod in [0, {P})")
        cells = self.cells(0, P, 0, P, k_lo, k_hi, want=want)
        return {n: np.ascontiguousarray(cells[n][s][:, d]) for n in want}


class Table:
    """Lazy probe.Table over one probe config's slots of a verdict table (table.go:24-56).

    `cells` is a cells source: the product's DeviceTable (cyc_table: planes resident on the GPU,
    Connectivity computed on the device per block of cells) or a PlaneCells view.  Items
    (table.go:10-23) are built on demand; the P^2 Item maps of truthtable.go:28-48 never exist."""

    CACHE_CELLS = 1 << 24  # whole-table Connectivity cache for rendering small tables

    def __init__(self, resources: Resources, config: ProbeConfig, cells, slot_lo: int, slot_hi: int):
        self.resources = resources
        self.config = config
        self.src = cells
        self.slots = range(slot_lo, slot_hi)
        self.items = resources.sorted_pod_names()
        self.index = {p.pod_string(): i for i, p in enumerate(resources.pods)}
        self._all = None
        self._rows = {}

    def _job_key(self, d: int, j: int) -> str:
        pod = self.resources.pods[d]
        if self.config.all_available:
            c = pod.containers[j]
            return f"{c.protocol}/{c.port}"
        port = self.config.port
        if isinstance(port, str):  # named port: ResolvedPort is -1 when it does not resolve
            hit = next((c for c in pod.containers if c.port_name == port), None)
            resolved = hit.port if hit is not None else -1
        else:
            resolved = int(port)
        return f"{self.config.protocol}/{resolved}"

    def _row(self, s: int):
        """Connectivity codes of source row s: {name: [P, nk]}."""
        P, lo, hi = len(self.resources.pods), self.slots.start, self.slots.stop
        if self._all is None and P * P * max(hi - lo, 1) <= self.CACHE_CELLS:
            self._all = self.src.cells(0, P, 0, P, lo, hi)
        if self._all is not None:
            return {n: a[s] for n, a in self._all.items()}
        if s not in self._rows:
            if len(self._rows) > 64:
                self._rows.clear()
            self._rows[s] = {n: a[0] for n, a in self.src.cells(s, s + 1, 0, P, lo, hi).items()}
        return self._rows[s]

    def get(self, fr: str, to: str) -> Item:
        s, d = self.index[fr], self.index[to]
        row = self._row(s)
        out = {}
        for j in range(len(self.slots)):
            ci = int(row["combined"][d, j])
            if ci == _lib.CONN_NO_JOB:
                continue
            key = self._job_key(d, j)
            out[key] = JobResult(key, _CONN[int(row["ingress"][d, j])], _CONN[int(row["egress"][d, j])], _CONN[ci])
        return Item(fr, to, out)

    def keys(self):
        return [(a, b) for a in self.items for b in self.items]

    def find(self, connectivity: str, view: str = "combined"):
        """Yield (from, to, JobResult) for every job of the table whose Ingress, Egress or Combined (`view`) is
        `connectivity`, listed by the cells source (cyc_table_find on the device for a DeviceTable).  The order is
        plane order (the pods as Resources holds them, then the job slots), not the sorted-name order of keys()."""
        code = next((c for c, name in _CONN.items() if name == connectivity), None)
        if code is None:
            raise ValueError(f"invalid Connectivity value: {connectivity}")
        pods = self.resources.pods
        for page in self.src.find_all(view, (code,), self.slots.start, self.slots.stop):
            for r in page:
                d, j = int(r["d"]), int(r["k"]) - self.slots.start
                key = self._job_key(d, j)
                yield (pods[int(r["s"])].pod_string(), pods[d].pod_string(),
                       JobResult(key, _CONN[int(r["ingress"])], _CONN[int(r["egress"])], _CONN[int(r["combined"])]))

    # The level between the whole-table totals and the listings: per pair of namespaces (the reference prints
    # whole pod tables only).
    def _namespaces(self):
        """(the pods' namespaces in sorted order, the int32 group id of every pod in plane order)."""
        names = sorted({p.namespace for p in self.resources.pods})
        at = {n: i for i, n in enumerate(names)}
        return names, np.array([at[p.namespace] for p in self.resources.pods], np.int32)

    def namespace_counts(self, view: str = "combined") -> dict:
        """{(namespace from, namespace to): {Connectivity: jobs}} over the table's slots for the jobs' Ingress, Egress
        or Combined (`view`), zero counts left out; counted by the cells source (cyc_table_group_counts on the device
        for a DeviceTable)."""
        if view not in _lib.VIEWS:
            raise ValueError(f"invalid view: {view}")
        names, groups = self._namespaces()
        if not names:
            return {}
        c = self.src.group_counts(groups, len(names), self.slots.start, self.slots.stop, want=(view,))[view].sum(axis=2)
        return {(fr, to): {_CONN[x]: int(c[i, j, x]) for x in range(6) if c[i, j, x]}
                for i, fr in enumerate(names) for j, to in enumerate(names)}

    def render_namespace_table(self, view: str = "combined") -> str:
        """Namespaces by namespaces, each cell "<allowed jobs>/<jobs>"."""
        names, _ = self._namespaces()
        counts = self.namespace_counts(view)
        rows = [[fr] + [f"{counts[fr, to].get(ALLOWED, 0)}/{sum(counts[fr, to].values())}" for to in names] for fr in names]
        return render([""] + names, rows, row_line=False)

    # The pod level: which pods reach everything or nothing, which are reached from everywhere.
    def pod_counts(self, view: str = "combined") -> dict:
        """{pod: {"as_source": {Connectivity: jobs}, "as_destination": {Connectivity: jobs}}} over the table's slots
        for the jobs' Ingress, Egress or Combined (`view`): the jobs from the pod to every pod and from every pod to it,
        zero counts left out; counted by the cells source (cyc_table_pod_counts on the device for a DeviceTable)."""
        if view not in _lib.VIEWS:
            raise ValueError(f"invalid view: {view}")
        c = self.src.pod_counts(view, self.slots.start, self.slots.stop)
        src, dst = c["src"].sum(axis=1), c["dst"].sum(axis=1)
        tally = lambda row: {_CONN[x]: int(row[x]) for x in range(6) if row[x]}  # noqa: E731
        return {p.pod_string(): {"as_source": tally(src[i]), "as_destination": tally(dst[i])} for i, p in enumerate(self.resources.pods)}

    def render_pod_table(self, view: str = "combined") -> str:
        """A row per pod in sorted-name order: "<allowed jobs>/<jobs>" as source and as destination."""
        counts = self.pod_counts(view)
        cell = lambda c: f"{c.get(ALLOWED, 0)}/{sum(c.values())}"  # noqa: E731
        rows = [[name, cell(counts[name]["as_source"]), cell(counts[name]["as_destination"])] for name in self.items]
        return render(["", "as source", "as destination"], rows, row_line=False)

    # Multi-hop: what the pods get to through other pods (the reference answers one hop at a time).
    def reach(self, pods, direction: str = "from", max_hops: int = -1) -> dict:
        """{pod: hops} for every pod reached from the seed pods ("ns/name" strings, or one) over edges that are a
        Combined of allowed in some slot of the table: the least number of edges from a seed (direction "to": to a
        seed; the seeds are 0), paths of at most max_hops edges (negative: no bound); searched by the cells source
        (cyc_table_reach on the device for a DeviceTable)."""
        seeds = [self.index[p] for p in ([pods] if isinstance(pods, str) else pods)]
        hops = self.src.reach([seeds], direction, self.slots.start, self.slots.stop, max_hops, want=("hops",))["hops"][0]
        return {p.pod_string(): int(hops[i]) for i, p in enumerate(self.resources.pods) if hops[i] >= 0}

    # All pairs through any number of hops: the zones (pods that all reach one another) and how far every pod gets.
    def _zones(self):
        z = self.src.zones(self.slots.start, self.slots.stop, want=("zone",))
        members = [[] for _ in range(z["n_zones"])]
        for p, x in enumerate(z["zone"].tolist()):
            members[x].append(p)
        return members

    def zones(self) -> dict:
        """{"zones": [[pods of zone 0], ...]}: the pods ("ns/name", in plane order) that all reach one another over edges
        that are a Combined of allowed in some slot of the table, whatever the number of hops; zones in the order of their
        first pod; found by the cells source (cyc_table_zones on the device for a DeviceTable)."""
        pods = self.resources.pods
        return {"zones": [[pods[p].pod_string() for p in z] for z in self._zones()]}

    def blast_radius(self) -> dict:
        """{pod: (reaches, reached_by)}: the number of pods the pod gets to through any number of hops and the number
        that get to it, each with the pod itself."""
        z = self.src.zones(self.slots.start, self.slots.stop, want=("n_from", "n_to"))
        return {p.pod_string(): (int(z["n_from"][i]), int(z["n_to"][i])) for i, p in enumerate(self.resources.pods)}

    def render_zone_table(self) -> str:
        """Zones by zones, each labelled by its first pod and " (+N)" for its N other members; a cell is "X" where the
        pods of the row's zone reach the pods of the column's zone, "." where they do not (read off the closure rows of
        the zones' first pods)."""
        m, pods = self._zones(), self.resources.pods
        label = lambda z: pods[z[0]].pod_string() + (f" (+{len(z) - 1})" if len(z) > 1 else "")  # noqa: E731
        heads = [z[0] for z in m]
        rows = self.src.closure("from", self.slots.start, self.slots.stop, want=("plane",))["plane"][heads]
        rows = (rows.cpu().numpy() if hasattr(rows, "cpu") else np.asarray(rows)).view(np.uint64).reshape(len(heads), -1)
        cell = lambda i, q: "X" if (int(rows[i, q // 64]) >> (q % 64)) & 1 else "."  # noqa: E731
        return render([""] + [label(z) for z in m], [[label(z)] + [cell(i, q) for q in heads] for i, z in enumerate(m)], row_line=False)

    # How the zones are connected: the cover edges between them (a -> b with no third zone between) and their tiers.
    def _zone_graph(self):
        g = self.src.zone_graph(self.slots.start, self.slots.stop, want=("zone", "tier", "edges"))
        members = [[] for _ in range(g["n_zones"])]
        for p, x in enumerate(g["zone"].tolist()):
            members[x].append(p)
        return members, g["tier"].tolist(), g["edges"].tolist()

    def zone_graph(self) -> dict:
        """{"zones": [[pods of zone 0], ...], "tiers": [tier of zone 0, ...], "edges": [[a, b], ...]}: zones() with the
        zone ids of the cover edges (zone a reaches zone b and no third zone lies between them; every other connection
        between zones follows from these) in ascending order, and per zone the edges of the longest chain of cover edges
        that ends in it (0: no other zone reaches it); found by the cells source (cyc_table_zone_graph on the device for
        a DeviceTable)."""
        m, tiers, edges = self._zone_graph()
        pods = self.resources.pods
        return {"zones": [[pods[p].pod_string() for p in z] for z in m], "tiers": tiers, "edges": edges}

    def render_zone_graph(self, fmt: str = "text") -> str:
        """The zone graph as text (the zones grouped by tier, then a line "a -> b" per cover edge) or as a Graphviz
        digraph ("dot": a rank=same group per tier); zones labelled like render_zone_table's."""
        if fmt not in ("text", "dot"):
            raise ValueError(f"invalid format: {fmt}")
        m, tiers, edges = self._zone_graph()
        pods = self.resources.pods
        label = [pods[z[0]].pod_string() + (f" (+{len(z) - 1})" if len(z) > 1 else "") for z in m]
        by_tier = [[z for z in range(len(m)) if tiers[z] == t] for t in range(max(tiers, default=-1) + 1)]
        if fmt == "text":
            out = [f"tier {t}: " + ", ".join(label[z] for z in zs) for t, zs in enumerate(by_tier)]
            out += [f"{label[a]} -> {label[b]}" for a, b in edges]
            return "\n".join(out) + "\n"
        out = ["digraph zones {"]
        out += [f'  z{z} [label="{label[z]}"];' for z in range(len(m))]
        out += ["  { rank=same; " + " ".join(f"z{z};" for z in zs) + " }" for zs in by_tier]
        out += [f"  z{a} -> z{b};" for a, b in edges]
        return "\n".join(out + ["}"]) + "\n"

    # The lossless summary: the pods that behave alike, and the table of one representative per class.
    def _classes(self, view):
        if view not in _lib.VIEWS:
            raise ValueError(f"invalid view: {view}")
        c = self.src.classes(view, self.slots.start, self.slots.stop)
        members = {side: [[] for _ in range(c["n_" + side])] for side in ("src", "dst")}
        for side in ("src", "dst"):
            for p, x in enumerate(c[side].tolist()):
                members[side][x].append(p)
        return members

    def classes(self, view: str = "combined") -> dict:
        """{"sources": [[pods of class 0], ...], "destinations": [...]}: the pods ("ns/name", in plane order) whose jobs'
        Ingress, Egress or Combined (`view`) agree towards every pod, and from every pod, over the table's slots;
        classes in the order of their first pod; found by the cells source (cyc_table_classes on the device for a
        DeviceTable)."""
        m, pods = self._classes(view), self.resources.pods
        return {name: [[pods[p].pod_string() for p in c] for c in m[side]] for name, side in (("sources", "src"), ("destinations", "dst"))}

    def render_class_table(self, view: str = "combined") -> str:
        """Source classes by destination classes, each labelled by its first pod and " (+N)" for its N other members;
        a cell holds the view's short string per slot for the two first pods, "-" for a slot without a job."""
        m, pods = self._classes(view), self.resources.pods
        label = lambda c: pods[c[0]].pod_string() + (f" (+{len(c) - 1})" if len(c) > 1 else "")  # noqa: E731
        codes = self.src.cells_at([c[0] for c in m["src"]], [c[0] for c in m["dst"]], self.slots.start, self.slots.stop, want=(view,))[view]
        short = lambda x: "-" if x == _lib.CONN_NO_JOB else short_string(_CONN[x])  # noqa: E731
        rows = [[label(c)] + ["\n".join(short(int(x)) for x in codes[i, j]) for j in range(len(m["dst"]))] for i, c in enumerate(m["src"])]
        return render([""] + [label(c) for c in m["dst"]], rows, row_line=len(self.slots) > 1)

    # table.go:58-156
    def render_ingress(self) -> str:
        return self._render(lambda r: short_string(r.ingress))

    def render_egress(self) -> str:
        return self._render(lambda r: short_string(r.egress))

    def render_table(self) -> str:
        return self._render(lambda r: short_string(r.combined))

    def _render(self, fn) -> str:
        uniform, single = True, True
        schema = set()
        for fr, to in self.keys():
            d = self.get(fr, to).job_results
            if len(d) != 1:
                single = False
                break
            schema.add("_".join(sorted(d)))
            if len(schema) > 1:
                uniform = False
                break
        if uniform and single:  # renderSimpleTable :96-105
            rows = [[fr] + [fn(next(iter(self.get(fr, to).job_results.values()))) for to in self.items] for fr in self.items]
            return render([""] + self.items, rows, row_line=False)
        if uniform:  # renderUniformMultiTable :107-123 (schema of the first cell)
            first = self.get(self.items[0], self.items[0]).job_results
            keys = sorted(first)
            rows = []
            for fr in self.items:
                row = [fr]
                for to in self.items:
                    d = self.get(fr, to).job_results
                    if any(k not in d for k in keys):
                        raise _lib.CyclonusPanic(0, "runtime error: invalid memory address or nil pointer dereference")
                    row.append("\n".join(fn(d[k]) for k in keys))
                rows.append(row)
            return render(["\n".join(keys)] + self.items, rows, row_line=True)
        rows = []  # renderNonuniformTable :125-140
        for fr in self.items:
            row = [fr]
            for to in self.items:
                d = self.get(fr, to).job_results
                row.append("\n".join(f"{k}: {fn(d[k])}" for k in sorted(d)))
            rows.append(row)
        return render([""] + self.items, rows, row_line=True)


# ----------------------------------------------------------------------------- runners
class Runner:
    """probe.Runner over the GPU engine (jobrunner.go:13-58)."""

    def __init__(self, policy: Policy):
        self.policy = policy
        self.job_runner = SimulatedJobRunner(policy)

    def run_probe_for_config(self, probe_config, resources) -> Table:
        return self.run_probes([probe_config], resources)[0]

    def run_probes(self, probe_configs, resources) -> List[Table]:
        """All configs in one batched GPU pass; one Table per config."""
        res = _as_resources(resources)
        cfgs = [_as_probe(c) for c in probe_configs]
        eng: Engine = self.policy.engine
        eng.load_resources(json.dumps(res.to_json()))
        eng.prepare([c.to_json() for c in cfgs])
        dt = eng.table()  # planes stay on the GPU; Items are built from device-computed cells
        maxc = max((len(p.containers) for p in res.pods), default=0)
        tables, lo = [], 0
        for c in cfgs:
            n = maxc if c.all_available else 1
            tables.append(Table(res, c, dt, lo, lo + n))
            lo += n
        return tables


class SimulatedJobRunner:
    """JobRunner.RunJobs (jobrunner.go:60-94) for explicit job lists: every job's Traffic
    (job.go:81-103) is evaluated on the GPU in one batch."""

    def __init__(self, policy: Policy):
        self.policies = policy

    def run_jobs(self, jobs) -> List[JobResult]:
        traffics = []
        for j in jobs:
            traffics.append({
                "Source": {"Internal": {"PodLabels": j.get("FromPodLabels"), "NamespaceLabels": j.get("FromNamespaceLabels"),
                                        "Namespace": j.get("FromNamespace", "")}, "IP": j.get("FromIP", "")},
                "Destination": {"Internal": {"PodLabels": j.get("ToPodLabels"), "NamespaceLabels": j.get("ToNamespaceLabels"),
                                             "Namespace": j.get("ToNamespace", "")}, "IP": j.get("ToIP", "")},
                "ResolvedPort": j.get("ResolvedPort", 0), "ResolvedPortName": j.get("ResolvedPortName", ""),
                "Protocol": j.get("Protocol", "")})
        out = []
        for j, r in zip(jobs, self.policies.is_traffic_allowed_batch([_traffic_json(t) for t in traffics])):
            ing = ALLOWED if r.ingress.is_allowed() else BLOCKED
            eg = ALLOWED if r.egress.is_allowed() else BLOCKED
            out.append(JobResult(f"{j.get('Protocol', '')}/{j.get('ResolvedPort', 0)}", ing, eg,
                                 ALLOWED if r.is_allowed() else BLOCKED))
        return out


def new_simulated_runner(policy: Policy) -> Runner:
    return Runner(policy)
