"""Engine: one libcyclonus_hip context on one GPU (thin wrapper over include/cyclonus_hip.h)."""
from __future__ import annotations

import ctypes
import json
from typing import Any, Optional

import numpy as np

from . import _lib
from ._lib import check, lib


def _bytes(doc: Any) -> bytes:
    if isinstance(doc, bytes):
        return doc
    if isinstance(doc, str):
        return doc.encode()
    return json.dumps(doc, separators=(",", ":")).encode()


class Engine:
    """A verdict-engine context bound to `device` (HIP device ordinal)."""

    def __init__(self, device: int = 0):
        self._ctx = ctypes.c_void_p()
        rc = lib().cyc_ctx_create(int(device), ctypes.byref(self._ctx))
        if rc != _lib.OK:
            raise _lib.CyclonusError(rc, f"cyc_ctx_create(device={device}) failed")
        self.device = device
        self.shape: Optional[dict] = None

    def close(self):
        if self._ctx:
            lib().cyc_ctx_destroy(self._ctx)
            self._ctx = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---------------------------------------------------------------- inputs
    def build_policies(self, netpols, simplify: bool = True) -> "Engine":
        b = _bytes(netpols)
        check(self._ctx, lib().cyc_policy_build_json(self._ctx, int(bool(simplify)), b, len(b)))
        return self

    def load_policy_ir(self, policy_ir) -> "Engine":
        b = _bytes(policy_ir)
        check(self._ctx, lib().cyc_policy_load_ir_json(self._ctx, b, len(b)))
        return self

    def _dump(self, fn) -> dict:
        """A JSON dump entry point (bytes needed, or -(cyc_status) with cyc_last_error set)."""
        n = fn(self._ctx, None, 0)
        if n < 0:
            check(self._ctx, int(-n))
        buf = ctypes.create_string_buffer(int(n))
        m = fn(self._ctx, buf, int(n))
        if m < 0:
            check(self._ctx, int(-m))
        return json.loads(buf.value.decode())

    def policy_ir(self) -> dict:
        return self._dump(lib().cyc_policy_ir_json)

    def load_resources(self, resources) -> "Engine":
        b = _bytes(resources)
        check(self._ctx, lib().cyc_resources_load_json(self._ctx, b, len(b)))
        return self

    # ---------------------------------------------------------------- flat tables (no JSON)
    def load_resources_tables(self, tables) -> "Engine":
        """cyc_resources_load: a flat.ResourceTables (or a probe.Resources dict, flattened here)."""
        from . import flat

        t = tables if isinstance(tables, flat.ResourceTables) else flat.ResourceTables(tables)
        check(self._ctx, lib().cyc_resources_load(self._ctx, ctypes.byref(t.c)))
        return self

    def load_policy_tables(self, tables) -> "Engine":
        """cyc_policy_load: a flat.PolicyTables (or a json.Marshal(*matcher.Policy) dict, flattened here)."""
        from . import flat

        t = tables if isinstance(tables, flat.PolicyTables) else flat.PolicyTables(tables)
        check(self._ctx, lib().cyc_policy_load(self._ctx, ctypes.byref(t.c)))
        return self

    def prepare_configs(self, probes) -> dict:
        """cyc_probe_prepare_configs: the probe configs as cyc_probe_config structs."""
        from . import flat

        cfg = probes if isinstance(probes, flat.ProbeConfigs) else flat.ProbeConfigs(probes)
        sh = _lib.ProbeShape()
        check(self._ctx, lib().cyc_probe_prepare_configs(self._ctx, cfg.c, cfg.n, ctypes.byref(sh)))
        self.shape = sh.as_dict()
        return self.shape

    def resources_json(self) -> dict:
        """The loaded probe model (cyc_resources_json: json.Marshal(*probe.Resources) of the kept fields)."""
        return self._dump(lib().cyc_resources_json)

    def prepare(self, probes) -> dict:
        b = _bytes(probes)
        sh = _lib.ProbeShape()
        check(self._ctx, lib().cyc_probe_prepare(self._ctx, b, len(b), ctypes.byref(sh)))
        self.shape = sh.as_dict()
        return self.shape

    # ---------------------------------------------------------------- runs
    # partition: "target" (rows are the pods both planes are keyed by) or "source" (rows are source
    # pods: every cell (s in rows, d, k); include/cyclonus_hip.h, cyc_rows)
    def layout(self, row_lo: int = 0, row_hi: Optional[int] = None, partition: str = "target"):
        """(ingress rows, ingress words per slot, egress rows, egress words per slot, window start word)."""
        hi = self.shape["pods"] if row_hi is None else row_hi
        v = (ctypes.c_int64 * 5)()
        check(self._ctx, lib().cyc_rows_layout(self._ctx, _lib.PARTITIONS[partition], int(row_lo), int(hi), v, 5))
        return tuple(int(x) for x in v)

    def run_host(self, row_lo: int = 0, row_hi: Optional[int] = None, partition: str = "target"):
        """Run on the GPU and copy back: (status[P,K] u8, ingress[rows_in,K,Wi] u64, egress[rows_eg,K,W] u64).
        Target rows: both planes are [row_hi - row_lo, K, W].  Source rows: ingress is [P, K, Wi], the
        words [row_lo/64, row_lo/64 + Wi) of every destination's row."""
        P, K = self.shape["pods"], self.shape["slots"]
        hi = P if row_hi is None else row_hi
        ri, wi, re_, we, _ = self.layout(row_lo, hi, partition)
        ing = np.zeros((ri, K, wi), np.uint64)
        eg = np.zeros((re_, K, we), np.uint64)
        st = np.zeros((P, K), np.uint8)
        check(
            self._ctx,
            lib().cyc_probe_run_host_rows(self._ctx, ing.ctypes.data, eg.ctypes.data, st.ctypes.data,
                                          _lib.PARTITIONS[partition], int(row_lo), int(hi)),
        )
        return st, ing, eg

    def run_device(self, d_ingress: int, d_egress: int, d_status: int, stream: int = 0, row_lo: int = 0, row_hi=None,
                   partition: str = "target"):
        """Enqueue the pipeline on `stream` writing device pointers (e.g. torch .data_ptr())."""
        P = self.shape["pods"]
        hi = P if row_hi is None else row_hi
        check(
            self._ctx,
            lib().cyc_probe_run_rows(
                self._ctx, ctypes.c_void_p(stream or None), ctypes.c_void_p(d_ingress), ctypes.c_void_p(d_egress),
                ctypes.c_void_p(d_status or None), _lib.PARTITIONS[partition], int(row_lo), int(hi),
            ),
        )

    def target_effects(self, direction, row_lo: int = 0, row_hi: Optional[int] = None, k_lo: int = 0, k_hi: Optional[int] = None):
        """cyc_probe_target_effects: which target decides.  direction: "ingress" / "egress" (or a cyc_direction);
        rows [row_lo, row_hi) are the pods the direction's policies target.  -> (effects int64 [T, nk, 4], applies
        int64 [T]): per target in primary-key order and slot the cells where it is in AllowingTargets, in
        DenyingTargets, the only allowing target beside a denying one, the only applying target and denying
        (_lib.EFFECTS); and the pods of the rows it applies to.  Needs a prepare, no run."""
        d = _lib.DIRECTIONS.get(direction, direction)
        sh = self.shape or {"pods": 0, "slots": 0, "targets_in": 0, "targets_eg": 0}
        hi = sh["pods"] if row_hi is None else row_hi
        k_hi = sh["slots"] if k_hi is None else k_hi
        T = sh["targets_eg" if d == _lib.DIR_EGRESS else "targets_in"]
        nk = max(int(k_hi) - int(k_lo), 0)
        eff = np.zeros((T, nk, 4), np.int64)
        app = np.zeros(T, np.int64)
        # (empty numpy arrays still have a data pointer: an empty output is never the NULL the library refuses)
        check(self._ctx, lib().cyc_probe_target_effects(self._ctx, int(d), int(row_lo), int(hi), int(k_lo), int(k_hi),
                                                        ctypes.c_void_p(eff.ctypes.data), ctypes.c_void_p(app.ctypes.data)))
        return eff, app

    def table(self, row_lo: int = 0, row_hi: Optional[int] = None, partition: str = "target") -> "DeviceTable":
        """Run the probe into a device-resident table (cyc_table_run_rows) for rows [row_lo, row_hi)."""
        hi = self.shape["pods"] if row_hi is None else row_hi
        t = ctypes.c_void_p()
        check(self._ctx, lib().cyc_table_run_rows(self._ctx, _lib.PARTITIONS[partition], int(row_lo), int(hi), ctypes.byref(t)))
        return DeviceTable(t, self.device)

    def wrap_table(self, d_ingress: int, d_egress: int, d_status: int, row_lo: int = 0, row_hi=None,
                   partition: str = "target") -> "DeviceTable":
        """A table over planes produced by run_device (cyc_table_wrap_rows; the caller keeps them alive)."""
        hi = self.shape["pods"] if row_hi is None else row_hi
        t = ctypes.c_void_p()
        check(self._ctx, lib().cyc_table_wrap_rows(self._ctx, ctypes.c_void_p(d_ingress), ctypes.c_void_p(d_egress),
                                                   ctypes.c_void_p(d_status), _lib.PARTITIONS[partition], int(row_lo), int(hi),
                                                   ctypes.byref(t)))
        return DeviceTable(t, self.device)

    # ---------------------------------------------------------------- multi-GPU assembly (RCCL, comm.hpp)
    @staticmethod
    def comm_unique_id() -> bytes:
        """cyc_comm_unique_id: the 128-byte RCCL unique id rank 0 makes and hands to every rank."""
        buf = (ctypes.c_uint8 * 128)()
        rc = lib().cyc_comm_unique_id(buf)
        if rc != _lib.OK:
            raise _lib.CyclonusError(rc, "cyc_comm_unique_id failed")
        return bytes(buf)

    def comm_init(self, nranks: int, rank: int, uid: bytes):
        """cyc_comm_init: collective over the ranks; the context owns the communicator."""
        buf = (ctypes.c_uint8 * 128).from_buffer_copy(uid)
        check(self._ctx, lib().cyc_comm_init(self._ctx, int(nranks), int(rank), buf))
        return self

    def comm_destroy(self):
        check(self._ctx, lib().cyc_comm_destroy(self._ctx))

    def rows_shard(self, nranks: int, rank: int, partition: str = "source"):
        """cyc_rows_shard: rank's rows [lo, hi) of the library's partition of the prepared pods."""
        lo, hi = ctypes.c_int64(0), ctypes.c_int64(0)
        check(self._ctx, lib().cyc_rows_shard(self._ctx, _lib.PARTITIONS[partition], int(nranks), int(rank),
                                              ctypes.byref(lo), ctypes.byref(hi)))
        return int(lo.value), int(hi.value)

    def planes_allgather(self, d_ingress: int, d_egress: int, d_ingress_full: int, d_egress_full: int, stream: int = 0,
                         partition: str = "source"):
        """cyc_planes_allgather (collective): this rank's shard planes -> the whole [P][K][W] planes."""
        check(self._ctx, lib().cyc_planes_allgather(self._ctx, ctypes.c_void_p(stream or None), _lib.PARTITIONS[partition],
                                                    ctypes.c_void_p(d_ingress), ctypes.c_void_p(d_egress),
                                                    ctypes.c_void_p(d_ingress_full), ctypes.c_void_p(d_egress_full)))

    def table_allgather(self, shard: "DeviceTable") -> "DeviceTable":
        """cyc_table_allgather (collective): a whole device table from this rank's shard table."""
        t = ctypes.c_void_p()
        check(self._ctx, lib().cyc_table_allgather(self._ctx, shard._t, ctypes.byref(t)))
        return DeviceTable(t, self.device)

    def merge_sources(self, d_slices, d_ingress_full: int, stream: int = 0):
        """cyc_rows_merge_sources: every source shard's ingress slices (device pointers, rank order) ->
        the whole ingress plane, on one GPU."""
        arr = (ctypes.c_void_p * len(d_slices))(*[ctypes.c_void_p(p) for p in d_slices])
        check(self._ctx, lib().cyc_rows_merge_sources(self._ctx, ctypes.c_void_p(stream or None), len(d_slices), arr,
                                                      ctypes.c_void_p(d_ingress_full)))

    # ---------------------------------------------------------------- batched blocks
    def prepare_blocks(self, probes, block_end, block_config) -> dict:
        """Batched independent problems (cyc_probe_prepare_blocks): block b = pods
        [block_end[b-1], block_end[b]) answering probes[block_config[b]] over its own pods."""
        b = _bytes(probes)
        ends = np.ascontiguousarray(block_end, np.int64)
        cfgs = np.ascontiguousarray(block_config, np.int32)
        sh = _lib.ProbeShape()
        check(self._ctx, lib().cyc_probe_prepare_blocks(self._ctx, b, len(b), ends.ctypes.data, cfgs.ctypes.data, len(ends),
                                                        ctypes.byref(sh)))
        self.shape = sh.as_dict()
        self.n_blocks = len(ends)
        lay = np.zeros(2 * (self.n_blocks + 1), np.int64)
        check(self._ctx, lib().cyc_blocks_layout(self._ctx, lay.ctypes.data, len(lay)))
        self.block_layout = lay.reshape(-1, 2)  # per block (plane slab offset in words, status offset); then totals
        return self.shape

    def run_blocks_device(self, d_ingress: int, d_egress: int, d_status: int, stream: int = 0):
        """Every block's slab on the device (cyc_probe_run_blocks) -> per block (cyc_status, message)."""
        rc = np.zeros(self.n_blocks, np.int32)
        check(self._ctx, lib().cyc_probe_run_blocks(self._ctx, ctypes.c_void_p(stream or None), ctypes.c_void_p(d_ingress),
                                                    ctypes.c_void_p(d_egress), ctypes.c_void_p(d_status), rc.ctypes.data))
        return [(int(c), lib().cyc_block_error(self._ctx, b).decode(errors="replace") if c else "") for b, c in enumerate(rc)]

    def query_traffic(self, traffics):
        """Policy.IsTrafficAllowed on the GPU for a list of matcher.Traffic dicts -> [(ingress, egress)]."""
        b = _bytes(list(traffics))
        n = len(traffics)
        out = np.zeros(max(n, 1), np.uint8)
        check(self._ctx, lib().cyc_query_traffic(self._ctx, b, len(b), out.ctypes.data, n))
        return [(bool(o & 1), bool(o & 2)) for o in out[:n]]

    def query_traffic_tables(self, traffics):
        """query_traffic through the flat tables (cyc_query_traffic_tables: no JSON)."""
        from . import flat

        t = traffics if isinstance(traffics, flat.TrafficTables) else flat.TrafficTables(traffics)
        out = np.zeros(max(t.n, 1), np.uint8)
        check(self._ctx, lib().cyc_query_traffic_tables(self._ctx, ctypes.byref(t.c), out.ctypes.data, t.n))
        return [(bool(o & 1), bool(o & 2)) for o in out[:t.n]]

    def _json_out(self, fn, doc):
        b = _bytes(doc)
        need = ctypes.c_size_t(0)
        cap = 1 << 16
        while True:
            buf = ctypes.create_string_buffer(cap)
            rc = fn(self._ctx, b, len(b), buf, cap, ctypes.byref(need))
            if rc == _lib.ERR_ARG and need.value > cap:
                cap = need.value
                continue
            check(self._ctx, rc)
            return json.loads(buf.value.decode())

    def query_traffic_targets(self, traffics):
        """IsTrafficAllowed with the DirectionResult lists: per traffic
        {"Ingress": {"AllowingTargets": [pk..], "DenyingTargets": [pk..], "IsAllowed": b}, "Egress": .., "IsAllowed": b}."""
        return self._json_out(lib().cyc_query_traffic_targets, list(traffics))

    def query_targets(self, pods):
        """TargetsApplyingToPod per direction for QueryTargetPod dicts {Namespace, Labels}."""
        return self._json_out(lib().cyc_query_targets, list(pods))

    def classes(self):
        """(ingress, egress) number of distinct classes of the last run."""
        out = (ctypes.c_int64 * 2)()
        check(self._ctx, lib().cyc_last_classes(self._ctx, out, 2))
        return int(out[0]), int(out[1])

    def last_emit(self):
        """(kernel name(s), launch count) of the last run's emit, as the library launched it."""
        buf = ctypes.create_string_buffer(256)
        n = ctypes.c_int64(0)
        check(self._ctx, lib().cyc_last_emit(self._ctx, buf, 256, ctypes.byref(n)))
        return buf.value.decode(), int(n.value)

    def set_option(self, name: str, value: int):
        check(self._ctx, lib().cyc_set_option(self._ctx, name.encode(), int(value)))

    def get_option(self, name: str) -> int:
        v = ctypes.c_int64(0)
        check(self._ctx, lib().cyc_get_option(self._ctx, name.encode(), ctypes.byref(v)))
        return int(v.value)

    def timings(self):
        """(pipeline_ms, emit_ms, class_rows_ms) of the last run, from HIP events on its stream."""
        ms = (ctypes.c_double * 3)()
        check(self._ctx, lib().cyc_last_timings(self._ctx, ms, 3))
        return tuple(ms)


class DeviceTable:
    """A cyc_table: verdict planes resident on the GPU; cells() returns probe.Connectivity codes, counts()
    and compare() the whole-table summaries, group_counts() / group_compare() and pod_counts() / pod_compare() the
    same per pair of pod groups and per pod, find() and compare_find() the cells behind them as records in
    (s, d, k) order (all computed on the device)."""

    def __init__(self, handle: ctypes.c_void_p, device: int = 0):
        self._t = handle
        self.device = device  # HIP ordinal of the GPU the planes live on
        v = (ctypes.c_int64 * 8)()
        lib().cyc_table_shape(self._t, v, 8)
        self.pods, self.slots, self.words, self.row_lo, self.row_hi = (int(x) for x in v[:5])
        self.partition = "source" if v[5] == _lib.ROWS_SOURCE else "target"
        self.window = (int(v[6]), int(v[7]))  # ingress words [first, first + count) of a source-row table

    def close(self):
        if self._t:
            lib().cyc_table_destroy(self._t)
            self._t = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def cells(self, s_lo, s_hi, d_lo, d_hi, k_lo=0, k_hi=None, want=("ingress", "egress", "combined")):
        """{name: u8 array [s, d, k]} of cyc_connectivity codes for the requested block."""
        k_hi = self.slots if k_hi is None else k_hi
        shp = (max(s_hi - s_lo, 0), max(d_hi - d_lo, 0), max(k_hi - k_lo, 0))
        out = {n: np.zeros(shp, np.uint8) for n in want}
        ptr = [out[n].ctypes.data if n in out else None for n in ("ingress", "egress", "combined")]
        rc = lib().cyc_table_cells(self._t, int(s_lo), int(s_hi), int(d_lo), int(d_hi), int(k_lo), int(k_hi), *ptr)
        if rc != _lib.OK:
            raise _lib.CyclonusError(rc, lib().cyc_table_error(self._t).decode(errors="replace"))
        return out

    def _check(self, rc):
        if rc != _lib.OK:
            raise _lib.CyclonusError(rc, lib().cyc_table_error(self._t).decode(errors="replace"))

    def counts(self, k_lo=0, k_hi=None, want=("ingress", "egress", "combined", "no_job")):
        """cyc_table_counts: {name: i64 [k, 6]} cells per cyc_connectivity code of slots [k_lo, k_hi) over every
        cell the table answers, and "no_job": the cells without a job."""
        k_hi = self.slots if k_hi is None else k_hi
        out = {n: np.zeros((max(k_hi - k_lo, 0), 6), np.int64) for n in want if n != "no_job"}
        nj = ctypes.c_int64(0)
        ptr = [out[n].ctypes.data if n in out else None for n in ("ingress", "egress", "combined")]
        self._check(lib().cyc_table_counts(self._t, int(k_lo), int(k_hi), *ptr, ctypes.byref(nj) if "no_job" in want else None))
        if "no_job" in want:
            out["no_job"] = int(nj.value)
        return out

    def compare(self, other: "DeviceTable", k_lo=0, k_hi=None, ignore_loopback=False, want_diff=False, d_diff=None):
        """cyc_table_compare(self, other): {"pairs": i64 [3], "slots": i64 [k, 3], "dst": i64 [P, k, 3]} in
        (same, different, ignored) order, and with want_diff "diff": a torch int64 tensor [P, window words] on the
        table's device, row d bit s set iff the Items (s, d) differ (d_diff: a device pointer to write that plane
        to instead)."""
        k_hi = self.slots if k_hi is None else k_hi
        nk = max(k_hi - k_lo, 0)
        out = {"pairs": np.zeros(3, np.int64), "slots": np.zeros((nk, 3), np.int64), "dst": np.zeros((self.pods, nk, 3), np.int64)}
        diff = None
        if want_diff:
            import torch

            diff = torch.empty((self.pods, self.window[1] if self.partition == "source" else self.words), dtype=torch.int64,
                               device=f"cuda:{self.device}")
        self._check(lib().cyc_table_compare(self._t, other._t, int(k_lo), int(k_hi), int(bool(ignore_loopback)),
                                            out["pairs"].ctypes.data, out["slots"].ctypes.data, out["dst"].ctypes.data,
                                            ctypes.c_void_p(d_diff or (diff.data_ptr() if want_diff and diff.numel() else None))))
        if want_diff:
            out["diff"] = diff
        return out

    def _groups(self, groups, n_groups):
        g = np.ascontiguousarray(groups, np.int32)
        if g.shape != (self.pods,):
            raise ValueError(f"groups must hold one group id per pod ({self.pods}), got shape {g.shape}")
        return g, int(g.max(initial=-1)) + 1 if n_groups is None else int(n_groups)

    GROUP_CELLS_MAX = 1 << 27  # n_groups^2 * slots of one call (include/cyclonus_hip.h)

    def _group_shape(self, G, k_lo, k_hi):
        """(G, G, k) of the outputs; empty where the library refuses the arguments (it writes nothing then)."""
        nk = k_hi - k_lo
        ok = 0 <= k_lo <= k_hi <= self.slots and G >= 1 and G * G * max(nk, 1) <= self.GROUP_CELLS_MAX
        return (G, G, nk) if ok else (0, 0, 0)

    def group_counts(self, groups, n_groups=None, k_lo=0, k_hi=None, want=("ingress", "egress", "combined", "no_job")):
        """cyc_table_group_counts: counts split by pod group pair.  groups: an int32 group id per pod (-1: the pod
        is left out); n_groups defaults to max(groups) + 1.  {name: i64 [G, G, k, 6]} cells per (source group,
        destination group, slot, cyc_connectivity code), and "no_job": i64 [G, G]."""
        k_hi = self.slots if k_hi is None else k_hi
        g, G = self._groups(groups, n_groups)
        shape = self._group_shape(G, k_lo, k_hi)
        out = {n: np.zeros(shape[:2] if n == "no_job" else shape + (6,), np.int64) for n in want}
        ptr = [out[n].ctypes.data if n in out else None for n in ("ingress", "egress", "combined", "no_job")]
        self._check(lib().cyc_table_group_counts(self._t, g.ctypes.data, G, int(k_lo), int(k_hi), *ptr))
        return out

    def group_compare(self, other: "DeviceTable", groups, n_groups=None, k_lo=0, k_hi=None, ignore_loopback=False):
        """cyc_table_group_compare(self, other): compare split by pod group pair: {"pairs": i64 [G, G, 3],
        "slots": i64 [G, G, k, 3]} in (same, different, ignored) order."""
        k_hi = self.slots if k_hi is None else k_hi
        g, G = self._groups(groups, n_groups)
        shape = self._group_shape(G, k_lo, k_hi)
        out = {"pairs": np.zeros(shape[:2] + (3,), np.int64), "slots": np.zeros(shape + (3,), np.int64)}
        self._check(lib().cyc_table_group_compare(self._t, other._t, g.ctypes.data, G, int(k_lo), int(k_hi), int(bool(ignore_loopback)),
                                                  out["pairs"].ctypes.data, out["slots"].ctypes.data))
        return out

    def pod_counts(self, view, k_lo=0, k_hi=None, want=("src", "dst")):
        """cyc_table_pod_counts: {"src": i64 [rows, k, 7], "dst": i64 [P, k, 7]}: per source of the table's rows
        (over every destination) and per destination (over those sources) the cells of slots [k_lo, k_hi) per
        cyc_connectivity code in `view` ("ingress", "egress", "combined" or a cyc_view); column 6: cells without a job."""
        k_hi = self.slots if k_hi is None else k_hi
        nk = max(k_hi - k_lo, 0)
        n = {"src": self.row_hi - self.row_lo, "dst": self.pods}
        out = {x: np.zeros((n[x], nk, _lib.POD_CODES), np.int64) for x in want}
        # (empty numpy arrays still have a data pointer: an empty output is never the NULL the library refuses)
        ptr = [ctypes.c_void_p(out[x].ctypes.data) if x in out else None for x in ("src", "dst")]
        self._check(lib().cyc_table_pod_counts(self._t, int(_lib.VIEWS.get(view, view)), int(k_lo), int(k_hi), *ptr))
        return out

    def pod_compare(self, other: "DeviceTable", k_lo=0, k_hi=None, ignore_loopback=False):
        """cyc_table_pod_compare(self, other): compare per pod, (same, different, ignored) last: {"src_pairs": i64
        [rows, 3], "dst_pairs": i64 [P, 3]} the (from, to) pairs of a source and of a destination, {"src_slots": i64
        [rows, k, 3], "dst_slots": i64 [P, k, 3]} the per-job counts (dst_slots is compare's "dst")."""
        k_hi = self.slots if k_hi is None else k_hi
        nk, rows = max(k_hi - k_lo, 0), self.row_hi - self.row_lo
        out = {"src_pairs": np.zeros((rows, 3), np.int64), "dst_pairs": np.zeros((self.pods, 3), np.int64),
               "src_slots": np.zeros((rows, nk, 3), np.int64), "dst_slots": np.zeros((self.pods, nk, 3), np.int64)}
        self._check(lib().cyc_table_pod_compare(self._t, other._t, int(k_lo), int(k_hi), int(bool(ignore_loopback)),
                                                *(ctypes.c_void_p(out[x].ctypes.data) for x in ("src_pairs", "dst_pairs", "src_slots", "dst_slots"))))
        return out

    def _find(self, call, k_lo, k_hi, s_from, cap, out):
        """One page of a listing: (records, s_next, total).  cap None: pods * slots of the range, which always
        makes progress; cap 0 without `out`: the count-only call.  `out`: a CELL_DTYPE array to write into (cap
        defaults to its length); the result is a view of its first n records."""
        k_hi = self.slots if k_hi is None else k_hi
        s_from = self.row_lo if s_from is None else s_from
        if cap is None:
            cap = len(out) if out is not None else max(self.pods * max(k_hi - k_lo, 0), 1)
        if out is None and cap:
            out = np.zeros(cap, _lib.CELL_DTYPE)
        if out is not None and (out.dtype != np.dtype(_lib.CELL_DTYPE) or not out.flags.c_contiguous or len(out) < cap):
            raise ValueError("out must be a contiguous CELL_DTYPE array of at least cap records")
        n, s_next, total = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
        rc = call(int(k_lo), int(k_hi), int(s_from), ctypes.c_void_p(out.ctypes.data if out is not None else None), int(cap),
                  ctypes.byref(n), ctypes.byref(s_next), ctypes.byref(total))
        if rc != _lib.OK:
            e = _lib.CyclonusError(rc, lib().cyc_table_error(self._t).decode(errors="replace"))
            e.total = int(total.value)
            raise e
        recs = out[:n.value] if out is not None else np.zeros(0, _lib.CELL_DTYPE)
        return recs, int(s_next.value), int(total.value)

    def find(self, view, codes, k_lo=0, k_hi=None, s_from=None, cap=None, out=None):
        """cyc_table_find: the cells of slots [k_lo, k_hi) whose Connectivity in `view` ("ingress", "egress",
        "combined" or a cyc_view) is one of `codes` (cyc_connectivity values), for the sources from s_from on that
        fit into cap records, in (s, d, k) order -> (records, s_next, total)."""
        v, mask = _lib.VIEWS.get(view, view), _lib.code_mask(codes)
        return self._find(lambda k0, k1, *rest: lib().cyc_table_find(self._t, int(v), mask, k0, k1, *rest), k_lo, k_hi, s_from, cap, out)

    def compare_find(self, other: "DeviceTable", k_lo=0, k_hi=None, ignore_loopback=False, s_from=None, cap=None, out=None):
        """cyc_table_compare_find: the cells cyc_table_compare counts as `different`, listed like find; a record's
        `other` is the other table's Combined code."""
        return self._find(lambda k0, k1, *rest: lib().cyc_table_compare_find(self._t, other._t, k0, k1, int(bool(ignore_loopback)), *rest),
                          k_lo, k_hi, s_from, cap, out)

    def find_all(self, view, codes, k_lo=0, k_hi=None, cap=None):
        """The pages of find, from the table's first source to its last."""
        yield from _lib.pages(lambda s: self.find(view, codes, k_lo, k_hi, s, cap), self.row_lo, self.row_hi)

    def compare_find_all(self, other, k_lo=0, k_hi=None, ignore_loopback=False, cap=None):
        yield from _lib.pages(lambda s: self.compare_find(other, k_lo, k_hi, ignore_loopback, s, cap), self.row_lo, self.row_hi)

    # ---- multi-hop reachability (cyc_table_adjacency, cyc_table_reach)
    def adjacency(self, direction="from", k_lo=0, k_hi=None, d_out=None):
        """cyc_table_adjacency: the edges of slots [k_lo, k_hi) as a bit plane [P, W] on the table's device: "from" row s
        bit d, "to" row d bit s set iff s -> d is a Combined of allowed in some slot.  Returns a torch int64 tensor that
        owns the plane, or with d_out (a device pointer to write the plane to) that pointer."""
        k_hi = self.slots if k_hi is None else k_hi
        adj = None
        if d_out is None:
            import torch

            adj = torch.empty((self.pods, self.words), dtype=torch.int64, device=f"cuda:{self.device}")
        ptr = d_out if d_out is not None else (adj.data_ptr() if adj.numel() else None)
        self._check(lib().cyc_table_adjacency(self._t, int(k_lo), int(k_hi), int(_lib.REACH_DIRECTIONS.get(direction, direction)),
                                              ctypes.c_void_p(ptr)))
        return d_out if d_out is not None else adj

    def reach(self, seed_sets, direction="from", k_lo=0, k_hi=None, max_hops=-1, want=("reach", "hops", "levels")):
        """cyc_table_reach: breadth-first search over those edges for every seed set (a sequence of sequences of pod
        indices) at once: {"reach": u64 [n, W] bit p = reached, "hops": i32 [n, P] least number of edges from a seed
        ("to": to a seed), -1 = not within max_hops (negative: no bound), "levels": i64 [n] the largest hop value,
        -1 for an empty set}."""
        k_hi = self.slots if k_hi is None else k_hi
        off, seeds = _lib.seed_arrays(seed_sets)
        n = len(off) - 1
        ok = n * max(self.words, 1) <= _lib.REACH_WORDS_MAX  # (the library refuses the rest and writes nothing)
        shape = {"reach": ((n, self.words), np.uint64), "hops": ((n, self.pods), np.int32), "levels": ((n,), np.int64)}
        out = {x: np.zeros(shape[x][0] if ok else (0,), shape[x][1]) for x in want}
        # (empty numpy arrays still have a data pointer: an empty output is never the NULL the library refuses)
        ptr = [ctypes.c_void_p(out[x].ctypes.data) if x in out else None for x in ("reach", "hops", "levels")]
        self._check(lib().cyc_table_reach(self._t, int(k_lo), int(k_hi), int(_lib.REACH_DIRECTIONS.get(direction, direction)),
                                          ctypes.c_void_p(off.ctypes.data), ctypes.c_void_p(seeds.ctypes.data), n, int(max_hops), *ptr))
        return out

    # ---- all pairs: the transitive closure and the zones (cyc_table_closure, cyc_table_zones)
    def closure(self, direction="from", k_lo=0, k_hi=None, d_out=None, want=("plane", "n_reach")):
        """cyc_table_closure: the reflexive transitive closure of adjacency()'s edges: {"plane": a bit plane [P, W] on the
        table's device, "from": row p bit q set iff a path leads from p to q, "to": from q to p (a torch int64 tensor that
        owns the plane, or with d_out, a device pointer to write the plane to, that pointer), "n_reach": i64 [P] the set
        bits of every row}."""
        k_hi = self.slots if k_hi is None else k_hi
        out, ptr = {}, None
        if d_out is not None:
            out["plane"], ptr = d_out, d_out
        elif "plane" in want:
            import torch

            out["plane"] = torch.empty((self.pods, self.words), dtype=torch.int64, device=f"cuda:{self.device}")
            # (a tensor without elements has no pointer to refuse: the count keeps the call from being without output)
            ptr = out["plane"].data_ptr() if out["plane"].numel() else None
        if "n_reach" in want or (ptr is None and "plane" in want):
            out["n_reach"] = np.zeros(self.pods, np.int64)
        n = ctypes.c_void_p(out["n_reach"].ctypes.data) if "n_reach" in out else None
        self._check(lib().cyc_table_closure(self._t, int(k_lo), int(k_hi), int(_lib.REACH_DIRECTIONS.get(direction, direction)),
                                            ctypes.c_void_p(ptr), n))
        return {x: out[x] for x in out if x in want or (x == "plane" and d_out is not None)}

    def zones(self, k_lo=0, k_hi=None, want=("zone", "n_from", "n_to")):
        """cyc_table_zones: {"zone": i32 [P] the zone of every pod (pods are in one zone iff each reaches the other; zones
        numbered by their smallest pod), "n_zones": int, "n_from": i64 [P] the pods a pod reaches, "n_to": i64 [P] the
        pods that reach it, each with the pod itself}."""
        k_hi = self.slots if k_hi is None else k_hi
        dt = {"zone": np.int32, "n_from": np.int64, "n_to": np.int64}
        out = {x: np.zeros(self.pods, dt[x]) for x in want if x in dt}
        nz = ctypes.c_int64(0)
        # (empty numpy arrays still have a data pointer: an empty output is never the NULL the library refuses)
        p = {x: ctypes.c_void_p(out[x].ctypes.data) if x in out else None for x in dt}
        self._check(lib().cyc_table_zones(self._t, int(k_lo), int(k_hi), p["zone"], ctypes.byref(nz) if "zone" in want or "n_zones" in want else None,
                                          p["n_from"], p["n_to"]))
        if "zone" in want or "n_zones" in want:
            out["n_zones"] = int(nz.value)
        return out

    # ---- how the zones are connected (cyc_table_zone_graph)
    def zone_graph(self, k_lo=0, k_hi=None, want=("zone", "rep", "size", "tier", "edges"), max_zones=None, max_edges=None):
        """cyc_table_zone_graph: the condensation of the reach graph reduced to its cover edges: {"zone": i32 [P] as
        zones(), "n_zones": int Z, "rep": i32 [Z] the smallest pod of every zone, "size": i64 [Z] its pods, "tier": i32 [Z]
        the edges of the longest chain of cover edges that ends in it, "edges": i32 [n, 2] the cover edges (a, b) in
        ascending order (a reaches b and no third zone lies between them), "n_edges": int}.  The edges take a count-only
        call first, then the listing.  "reach" (on request): the reflexive zone reach matrix as a bit plane
        [Z, ceil(Z / 64)] on the table's device (a torch int64 tensor).  With max_zones (an upper bound of Z, the pods at
        the most) the plane is allocated for that many zones and costs no call of its own; without it a first call
        learns Z, which costs a second closure.  Likewise max_edges (an upper bound of the number of edges, from an
        earlier call on the same table and slots) lists the edges without the count-only call; one that is too small is the
        library's capacity error.  With the bounds that apply the whole result is one call."""
        k_hi = self.slots if k_hi is None else k_hi
        P = self.pods
        dt = {"zone": np.int32, "rep": np.int32, "size": np.int64, "tier": np.int32}
        out = {x: np.zeros(P, dt[x]) for x in want if x in dt}
        nz, ne = ctypes.c_int64(0), ctypes.c_int64(0)
        # (empty numpy arrays still have a data pointer: an empty output is never the NULL the library refuses)
        p = [ctypes.c_void_p(out[x].ctypes.data) if x in out else None for x in ("zone", "rep", "size", "tier")]

        def call(outs, edges, cap, plane, words):
            self._check(lib().cyc_table_zone_graph(self._t, int(k_lo), int(k_hi), outs[0], ctypes.byref(nz), *outs[1:], edges, cap,
                                                   ctypes.byref(ne), plane, words))

        none = [None] * 4
        edges, plane = None, None
        if ("edges" in want and max_edges is None) or ("reach" in want and max_zones is None):
            call(none, None, 0, None, 0)  # the counts: Z and the number of edges
        if "edges" in want:
            edges = np.zeros((int(ne.value) if max_edges is None else int(max_edges), 2), np.int32)
        if "reach" in want:
            import torch

            zmax = int(nz.value) if max_zones is None else int(max_zones)
            plane = torch.zeros(zmax * ((zmax + 63) // 64), dtype=torch.int64, device=f"cuda:{self.device}")
        if out or plane is not None or edges is not None:
            call(p, ctypes.c_void_p(edges.ctypes.data) if "edges" in want else None, len(edges) if "edges" in want else 0,
                 ctypes.c_void_p(plane.data_ptr()) if plane is not None and plane.numel() else None, plane.numel() if plane is not None else 0)
        else:
            call(none, None, 0, None, 0)
        Z = int(nz.value)
        for x in ("rep", "size", "tier"):
            if x in out:
                out[x] = out[x][:Z].copy()
        if "edges" in want:
            out["edges"] = edges[:int(ne.value)]
        if plane is not None:
            out["reach"] = plane[:Z * ((Z + 63) // 64)].view(Z, (Z + 63) // 64)
        out["n_zones"], out["n_edges"] = Z, int(ne.value)
        return out

    # ---- connectivity classes (cyc_table_classes, cyc_table_cells_at)
    def classes(self, view="combined", k_lo=0, k_hi=None, want=("src", "dst"), hash_mask=None, stats=False):
        """cyc_table_classes: the pods partitioned by equal rows ("src") and equal columns ("dst") of `view`'s cell codes
        over slots [k_lo, k_hi): {"src": i32 [P] class of every pod as a source, "n_src": int, "dst": ..., "n_dst": ...}
        with the classes numbered by their smallest pod.  hash_mask (cyc_table_classes_masked): the row hash is ANDed
        with it before the pods are grouped; stats: also "stats": i64 [4] = verification rounds and failed pods for
        sources, then for destinations."""
        k_hi = self.slots if k_hi is None else k_hi
        cls = {x: np.zeros(self.pods, np.int32) for x in want}
        cnt = {x: ctypes.c_int64(0) for x in want}
        st = np.zeros(4, np.int64)
        ptr = [ctypes.c_void_p(cls[x].ctypes.data) if x in cls else None for x in ("src", "dst")]
        ptr += [ctypes.byref(cnt[x]) if x in cnt else None for x in ("src", "dst")]
        v = int(_lib.VIEWS.get(view, view))
        if hash_mask is None and not stats:
            self._check(lib().cyc_table_classes(self._t, v, int(k_lo), int(k_hi), *ptr))
        else:
            mask = (1 << 64) - 1 if hash_mask is None else int(hash_mask)
            self._check(lib().cyc_table_classes_masked(self._t, v, int(k_lo), int(k_hi), *ptr, mask, ctypes.c_void_p(st.ctypes.data) if stats else None))
        out = {}
        for x in want:
            out[x], out["n_" + x] = cls[x], int(cnt[x].value)
        if stats:
            out["stats"] = st
        return out

    def cells_at(self, sources, dests, k_lo=0, k_hi=None, want=("ingress", "egress", "combined")):
        """cyc_table_cells_at: {name: u8 [n_s, n_d, k]} of cyc_connectivity codes for the listed sources and
        destinations (pod indices in any order, duplicates allowed)."""
        k_hi = self.slots if k_hi is None else k_hi
        s, d = np.ascontiguousarray(sources, np.int32).reshape(-1), np.ascontiguousarray(dests, np.int32).reshape(-1)
        out = {n: np.zeros((len(s), len(d), max(k_hi - k_lo, 0)), np.uint8) for n in want}
        ptr = [ctypes.c_void_p(out[n].ctypes.data) if n in out else None for n in ("ingress", "egress", "combined")]
        self._check(lib().cyc_table_cells_at(self._t, ctypes.c_void_p(s.ctypes.data), len(s), ctypes.c_void_p(d.ctypes.data), len(d),
                                             int(k_lo), int(k_hi), *ptr))
        return out
