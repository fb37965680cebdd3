"""Config #3's whole table through cyc_table_counts and cyc_table_compare, against a plain read of the same planes.

    python scripts/table_counts_bench.py time [reps=3] [out=FILE]   # the table below, as text and one JSON line
    python scripts/table_counts_bench.py run counts|compare|find_count|compare_find|find_dense|group_counts|group_compare|
                                             pod_counts|pod_compare|closure|zone_graph [n=2]   # n calls of one pass (for a rocprofv3 run)
    python scripts/table_counts_bench.py group [reps=3] [out=FILE]  # the group leg alone (below)
    python scripts/table_counts_bench.py pod [reps=3] [out=FILE]    # the pod leg alone (below)
    python scripts/table_counts_bench.py reach [reps=3] [out=FILE]  # the reachability leg alone (below)
    python scripts/table_counts_bench.py classes [reps=3] [out=FILE]  # the connectivity-class leg alone (below)
    python scripts/table_counts_bench.py closure [reps=3] [out=FILE]  # the transitive-closure leg alone (below)
    python scripts/table_counts_bench.py zone_graph [reps=3] [out=FILE]  # the zone graph leg alone (below)

In one process: the table of config #3 (2 x 10 GB planes) and a second table of the same pods under policies
drawn with another seed; then, min over reps of the synchronous calls,
  counts    cyc_table_counts over every slot (reads both planes once: 20 GB)
  compare   cyc_table_compare of the two tables with d_diff (reads four planes: 40 GB, writes P x W words)
  read      the yardstick: torch.sum over the same planes viewed as int64 (20 GB, and 40 GB for the four planes)
  fill      the box's fill figure, as bench.py measures it: torch's fill kernel over two planes' bytes
and the ratios counts / read and compare / read, with the achieved GB/s of the algorithmic bytes.  Then the
listings (cyc_table_find, cyc_table_compare_find) against counts and compare as their yardsticks:
  find_count    the count-only calls (pass 1 alone): compare_find of the two tables, find of Combined == blocked
  compare_find  the sparse case: table A against a torch.clone of its planes with 64 egress bits flipped, in one page
  find_dense    the dense case: one page of find(Combined == allowed) with cap = P * K
The group leg (mode `group`): the pods' namespaces as groups (1000 for config #3), every slot, interleaved with their
ungrouped counterparts on the same tables, min over reps of each:
  group_counts   cyc_table_group_counts, all three views and no_job, against cyc_table_counts; and Combined alone
  group_compare  cyc_table_group_compare with slot_counts against cyc_table_compare without d_diff
and once, as checks, that the group results summed over the group pairs are the ungrouped results.
The pod leg (mode `pod`): every slot, interleaved with their whole-table counterparts on the same tables, min over
reps of each:
  pod_counts   cyc_table_pod_counts(Combined), both outputs, against cyc_table_counts; and by_dst alone, which
               launches the kernel cyc_table_counts launches
  pod_compare  cyc_table_pod_compare, all four outputs, against cyc_table_compare without d_diff
and once, as checks, the sum invariants: both arrays of either call summed over the pods are the whole-table results,
and dst_slots is cyc_table_compare's dst_counts.
The reachability leg (mode `reach`): every slot, interleaved with counts and the plain read, min over reps of each:
  adjacency  cyc_table_adjacency into a device plane, both directions
  reach      cyc_table_reach "from" for 1 seed set and for 64 seed sets of one random pod each, to the fixpoint: the
             steps taken, the pods reached, the device scratch, the time split (a call without steps, one without hop
             values and copy-back, the whole call) and the adjacency rows gathered against the bound of DESIGN.md
The class leg (mode `classes`): every slot, Combined view, interleaved with counts, the adjacency pass both ways and the
plain read, min over reps of each:
  classes   cyc_table_classes_masked with stats for sources only, destinations only and both; the numbers of classes,
            the verification rounds and the pods that failed one
  cells_at  cyc_table_cells_at over one representative per class (the class table)
The closure leg (mode `closure`): every slot, interleaved with counts, the adjacency pass and one cyc_table_reach of 64
single-pod seed sets, min over reps of each:
  closure   cyc_table_closure into a device plane with n_reach, both directions
  zones     cyc_table_zones, all outputs; the number of zones and the largest one
and the closure against the only other way to all rows, P / 64 reach calls of 64 sets.  The split between the panel
and the update launches comes from a rocprofv3 --kernel-trace --stats run of `run closure`.
The zone graph leg (mode `zone_graph`): every slot, interleaved with cyc_table_zones, min over reps of each:
  zone_graph  cyc_table_zone_graph, every output and the zone reach plane in one call (the bounds from a count-only call
              made once); the count-only call; the unbounded form of the Python mirror (two calls, two closures)
and the number of zones, the cover edges against the set bits of the strict zone reach matrix, the tiers.  The split
between the compress, cover and listing launches comes from a rocprofv3 --kernel-trace --stats run of `run zone_graph`.
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from cyclonus_amd import synth
from cyclonus_amd._lib import CELL_DTYPE, CONN_ALLOWED, CONN_BLOCKED
from cyclonus_amd.engine import Engine
from cyclonus_amd.flat import prepare_flat

mode = sys.argv[1] if len(sys.argv) > 1 else "time"
pos = [a for a in sys.argv[2:] if "=" not in a]
kw = dict(a.split("=") for a in sys.argv[2:] if "=" in a)
reps, n_run, config = int(kw.get("reps", 3)), int(kw.get("n", 2)), kw.get("config", "config3")
SEED_B = 20250218  # the second table's policy seed (synth's own is 20250217)

data = synth.CONFIGS[config]()
pols_b = synth.CONFIGS[config](seed=SEED_B)["policies"]
tables, planes, flipped = [], [], []
for pols in (data["policies"], pols_b):
    eng = Engine(0)
    sh = prepare_flat(eng, pols, data["resources"], data["probes"])
    P, K, W = sh["pods"], sh["slots"], sh["words"]
    d_in = torch.empty((P, K, W), dtype=torch.int64, device="cuda")
    d_eg = torch.empty((P, K, W), dtype=torch.int64, device="cuda")
    d_st = torch.empty((P, K), dtype=torch.uint8, device="cuda")
    eng.run_device(d_in.data_ptr(), d_eg.data_ptr(), d_st.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    tables.append(eng.wrap_table(d_in.data_ptr(), d_eg.data_ptr(), d_st.data_ptr()))
    planes.append((d_in, d_eg, d_st))
    if not flipped:  # table A's copy with 64 directed egress bits flipped (source i * P // 64, destination 7919 i mod P)
        c_in, c_eg = torch.clone(d_in), torch.clone(d_eg)
        for i in range(64):
            s_, d_ = i * P // 64, (7919 * i + 63) % P
            c_eg[s_, i % K, d_ // 64] ^= (1 << (d_ % 64)) - (1 << 64 if d_ % 64 == 63 else 0)
        flipped = [eng.wrap_table(c_in.data_ptr(), c_eg.data_ptr(), d_st.data_ptr()), c_in, c_eg]
    eng.close()  # (a table outlives its context; the front's scratch goes)
ta, tb = tables
plane_gb = P * K * W * 8 / 1e9
diff = torch.empty((P, W), dtype=torch.int64, device="cuda")


def timed(f, n):
    best = float("inf")
    for _ in range(n):
        torch.cuda.synchronize()
        t = time.perf_counter()
        f()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t)
    return best * 1e3


def read(n_tables):
    return sum(int(torch.sum(p)) for t in planes[:n_tables] for p in t[:2])


def fill_gbs():
    """The box's fill figure (bench.py's write ceiling): torch's fill kernel over two planes' bytes."""
    scratch = torch.empty_like(planes[0][0])
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for _ in range(3):
        e0.record()
        scratch.fill_(0)
        scratch.fill_(0)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return 2 * scratch.numel() * 8 / (min(ms) * 1e-3) / 1e9


names = sorted({p["Namespace"] for p in data["resources"]["Pods"]})
ns_at = {n: i for i, n in enumerate(names)}
groups = np.array([ns_at[p["Namespace"]] for p in data["resources"]["Pods"]], np.int32)
G = len(names)
GROUP = {"group_counts": lambda: ta.group_counts(groups, G), "group_compare": lambda: ta.group_compare(tb, groups, G, ignore_loopback=True)}

POD = {"pod_counts": lambda: ta.pod_counts("combined"), "pod_compare": lambda: ta.pod_compare(tb, ignore_loopback=True)}

tc = flipped[0]
page = np.zeros(P * K, CELL_DTYPE)  # cap = P * K always makes progress
LISTINGS = {
    "find_count": lambda: (ta.compare_find(tb, ignore_loopback=True, cap=0), ta.find("combined", (CONN_BLOCKED,), cap=0)),
    "compare_find": lambda: ta.compare_find(tc, ignore_loopback=True, out=page),
    "find_dense": lambda: ta.find("combined", (CONN_ALLOWED,), out=page),
}

ZG_ALL = ("zone", "rep", "size", "tier", "edges", "reach")


def zone_graph_single_pass():
    """Every output of cyc_table_zone_graph in one call: the bounds come from a count-only call made once."""
    if not hasattr(zone_graph_single_pass, "bounds"):
        c = ta.zone_graph(want=())
        zone_graph_single_pass.bounds = {"max_zones": c["n_zones"], "max_edges": c["n_edges"]}
    return ta.zone_graph(want=ZG_ALL, **zone_graph_single_pass.bounds)


if mode == "run":
    f = {"counts": lambda: ta.counts(), "compare": lambda: ta.compare(tb, d_diff=diff.data_ptr()), **LISTINGS, **GROUP, **POD,
         "closure": lambda: ta.closure(want=("n_reach",)), "zone_graph": zone_graph_single_pass}[pos[0]]
    for _ in range(n_run):
        f()
    sys.exit(0)

if mode == "group":
    legs = {"counts": lambda: ta.counts(), "group_counts": GROUP["group_counts"],
            "group_counts_combined": lambda: ta.group_counts(groups, G, want=("combined",)),
            "compare_nodiff": lambda: ta.compare(tb, ignore_loopback=True), "group_compare": GROUP["group_compare"]}
    gc, gp = GROUP["group_counts"](), GROUP["group_compare"]()  # (warm-up, and the checks)
    c, r = ta.counts(), ta.compare(tb, ignore_loopback=True)
    sums_ok = (all(np.array_equal(gc[n].sum(axis=(0, 1)), c[n]) for n in ("ingress", "egress", "combined")) and int(gc["no_job"].sum()) == c["no_job"]
               and np.array_equal(gp["pairs"].sum(axis=(0, 1)), r["pairs"]) and np.array_equal(gp["slots"].sum(axis=(0, 1)), r["slots"]))
    ms = {n: float("inf") for n in legs}
    for _ in range(reps):  # interleaved: every leg once per round
        for n, f in legs.items():
            ms[n] = min(ms[n], timed(f, 1))
    res = {"config": config, "pods": P, "slots": K, "words": W, "groups": G, "plane_gb": round(plane_gb, 3), "reps": reps,
           **{n + "_ms": v for n, v in ms.items()}, "sums_equal_ungrouped": bool(sums_ok),
           "group_counts_over_counts": ms["group_counts"] / ms["counts"],
           "group_counts_combined_over_counts": ms["group_counts_combined"] / ms["counts"],
           "group_compare_over_compare": ms["group_compare"] / ms["compare_nodiff"],
           "group_counts_out_mb": sum(a.nbytes for a in gc.values()) / 1e6, "group_compare_out_mb": sum(a.nbytes for a in gp.values()) / 1e6,
           "group_pairs_with_allowed": int((gc["combined"][..., CONN_ALLOWED].sum(axis=2) > 0).sum()),
           "group_pairs_that_differ": int((gp["pairs"][..., 1] > 0).sum())}
    lines = [
        f"# {config}: P {P}, K {K}, W {W}, groups = the {G} namespaces; a plane is {plane_gb:.2f} GB; min of {reps} interleaved synchronous calls",
        f"counts         {ms['counts']:9.2f} ms   group_counts  {ms['group_counts']:9.2f} ms  ratio {res['group_counts_over_counts']:.2f}  "
        f"(host outputs {res['group_counts_out_mb']:.0f} MB; Combined alone {ms['group_counts_combined']:.2f} ms, ratio {res['group_counts_combined_over_counts']:.2f})",
        f"compare        {ms['compare_nodiff']:9.2f} ms   group_compare {ms['group_compare']:9.2f} ms  ratio {res['group_compare_over_compare']:.2f}  "
        f"(compare without d_diff; host outputs {res['group_compare_out_mb']:.0f} MB)",
        f"group results summed over the group pairs equal the ungrouped results: {sums_ok}; namespace pairs with an allowed Combined cell "
        f"{res['group_pairs_with_allowed']} of {G * G}, that differ between the tables {res['group_pairs_that_differ']}",
        json.dumps(res),
    ]
    print("\n".join(lines))
    if "out" in kw:
        os.makedirs(os.path.dirname(os.path.abspath(kw["out"])), exist_ok=True)
        with open(kw["out"], "w") as f:
            f.write("\n".join(lines) + "\n")
    sys.exit(0)

if mode == "pod":
    legs = {"counts": lambda: ta.counts(), "pod_counts": POD["pod_counts"], "pod_counts_dst": lambda: ta.pod_counts("combined", want=("dst",)),
            "compare_nodiff": lambda: ta.compare(tb, ignore_loopback=True), "pod_compare": POD["pod_compare"]}
    pc, pp = POD["pod_counts"](), POD["pod_compare"]()  # (warm-up, and the checks)
    c, r = ta.counts(), ta.compare(tb, ignore_loopback=True)
    sums_ok = (all(np.array_equal(pc[n][:, :, :6].sum(axis=0), c["combined"]) and int(pc[n][:, :, 6].sum()) == c["no_job"] for n in ("src", "dst"))
               and all(np.array_equal(pp[n + "_pairs"].sum(axis=0), r["pairs"]) and np.array_equal(pp[n + "_slots"].sum(axis=0), r["slots"])
                       for n in ("src", "dst")) and np.array_equal(pp["dst_slots"], r["dst"]))
    ms = {n: float("inf") for n in legs}
    for _ in range(reps):  # interleaved: every leg once per round
        for n, f in legs.items():
            ms[n] = min(ms[n], timed(f, 1))
    reach_all = int((pc["src"][:, :, CONN_ALLOWED].sum(axis=1) == pc["src"][:, :, :6].sum(axis=(1, 2))).sum())
    res = {"config": config, "pods": P, "slots": K, "words": W, "plane_gb": round(plane_gb, 3), "reps": reps,
           **{n + "_ms": v for n, v in ms.items()}, "sums_equal_whole_table": bool(sums_ok),
           "pod_counts_over_counts": ms["pod_counts"] / ms["counts"], "pod_counts_dst_over_counts": ms["pod_counts_dst"] / ms["counts"],
           "pod_compare_over_compare": ms["pod_compare"] / ms["compare_nodiff"],
           "pod_counts_out_mb": sum(a.nbytes for a in pc.values()) / 1e6, "pod_compare_out_mb": sum(a.nbytes for a in pp.values()) / 1e6,
           "sources_that_reach_nothing": int((pc["src"][:, :, CONN_ALLOWED].sum(axis=1) == 0).sum()), "sources_that_reach_every_job": reach_all,
           "sources_with_a_different_pair": int((pp["src_pairs"][:, 1] > 0).sum()),
           "destinations_with_a_different_pair": int((pp["dst_pairs"][:, 1] > 0).sum())}
    lines = [
        f"# {config}: P {P}, K {K}, W {W}; a plane is {plane_gb:.2f} GB; min of {reps} interleaved synchronous calls",
        f"counts         {ms['counts']:9.2f} ms   pod_counts(combined) {ms['pod_counts']:9.2f} ms  ratio {res['pod_counts_over_counts']:.2f}  "
        f"(host outputs {res['pod_counts_out_mb']:.1f} MB; by_dst alone {ms['pod_counts_dst']:.2f} ms, ratio {res['pod_counts_dst_over_counts']:.2f})",
        f"compare        {ms['compare_nodiff']:9.2f} ms   pod_compare          {ms['pod_compare']:9.2f} ms  ratio {res['pod_compare_over_compare']:.2f}  "
        f"(compare without d_diff; host outputs {res['pod_compare_out_mb']:.1f} MB)",
        f"sums over the pods equal counts / compare, dst_slots equals compare's dst: {sums_ok}; sources that reach nothing "
        f"{res['sources_that_reach_nothing']}, that reach every job {reach_all}; pods with a different pair: "
        f"{res['sources_with_a_different_pair']} as source, {res['destinations_with_a_different_pair']} as destination",
        json.dumps(res),
    ]
    print("\n".join(lines))
    if "out" in kw:
        os.makedirs(os.path.dirname(os.path.abspath(kw["out"])), exist_ok=True)
        with open(kw["out"], "w") as f:
            f.write("\n".join(lines) + "\n")
    sys.exit(0)

if mode == "reach":
    # slots [0, K): the adjacency plane both ways next to counts and the plain read, then the search from 1 seed set and
    # from 64 seed sets of one random pod each, to the fixpoint.  The library frees its scratch inside the call and reports
    # no phases, so the split is taken from calls that leave a phase out: no step (max_hops = 0, levels alone), the steps
    # without hop values or copy-back (levels alone), everything.
    rng = np.random.default_rng(16)
    seeds = [[int(p)] for p in rng.integers(0, P, 64)]
    adj = torch.empty((P, W), dtype=torch.int64, device="cuda")
    pitch = (W + 15) // 16 * 16
    legs = {"counts": lambda: ta.counts(), "read2": lambda: read(1),
            "adjacency_from": lambda: ta.adjacency("from", d_out=adj.data_ptr()), "adjacency_to": lambda: ta.adjacency("to", d_out=adj.data_ptr())}
    for n in (1, 64):
        legs[f"reach{n}_no_step"] = lambda n=n: ta.reach(seeds[:n], max_hops=0, want=("levels",))
        legs[f"reach{n}_levels"] = lambda n=n: ta.reach(seeds[:n], want=("levels",))
        legs[f"reach{n}"] = lambda n=n: ta.reach(seeds[:n])
    got = {n: ta.reach(seeds[:n]) for n in (1, 64)}  # (warm-up, and the figures of the search)
    for f in legs.values():
        f()
    ms = {n: float("inf") for n in legs}
    for _ in range(reps):  # interleaved: every leg once per round
        for n, f in legs.items():
            ms[n] = min(ms[n], timed(f, 1))
    # the edges: the set bits of the plane the last leg left in adj ("to"), counted through a byte table
    ones = torch.tensor([bin(i).count("1") for i in range(256)], dtype=torch.int64, device="cuda")
    edges = sum(int(ones[adj[lo:lo + 2048].view(torch.uint8).long()].sum()) for lo in range(0, P, 2048))
    res = {"config": config, "pods": P, "slots": K, "words": W, "plane_gb": round(plane_gb, 3), "reps": reps,
           **{n + "_ms": v for n, v in ms.items()}, "adjacency_gb": P * W * 8 / 1e9, "edges_to_plane": edges,
           "adjacency_from_over_read": ms["adjacency_from"] / ms["read2"], "adjacency_to_over_read": ms["adjacency_to"] / ms["read2"],
           "adjacency_from_over_counts": ms["adjacency_from"] / ms["counts"], "adjacency_to_over_counts": ms["adjacency_to"] / ms["counts"]}
    lines = [
        f"# {config}: P {P}, K {K}, W {W}, slots [0, {K}); a plane is {plane_gb:.2f} GB, the adjacency plane {res['adjacency_gb']:.3f} GB; "
        f"min of {reps} interleaved synchronous calls",
        f"counts {ms['counts']:9.2f} ms   read of 2 planes {ms['read2']:9.2f} ms   adjacency from {ms['adjacency_from']:9.2f} ms "
        f"({res['adjacency_from_over_read']:.2f} x read, {res['adjacency_from_over_counts']:.2f} x counts, {2 * plane_gb / ms['adjacency_from'] * 1e3:.0f} GB/s of 2 planes)   "
        f"adjacency to {ms['adjacency_to']:9.2f} ms ({res['adjacency_to_over_read']:.2f} x read, {res['adjacency_to_over_counts']:.2f} x counts, "
        f"{2 * plane_gb / ms['adjacency_to'] * 1e3:.0f} GB/s); edges in the plane {edges}",
    ]
    for n in (1, 64):
        g = got[n]
        reached = [int(x) for x in (g["hops"] >= 0).sum(axis=1)]
        steps = int(g["levels"].max()) + 1  # (the last step finds nothing)
        bound_gb = sum(reached) * pitch * 8 / 1e9  # rows gathered: every reached pod's row once per set
        step_ms = ms[f"reach{n}_levels"] - ms[f"reach{n}_no_step"]
        scratch_mb = (P * pitch * 8 + 3 * n * W * 8 + n * P * 4 + n * 8 + K * W * 16) / 1e6
        res.update({f"reach{n}_steps": steps, f"reach{n}_levels_max": int(g["levels"].max()), f"reach{n}_reached_min": min(reached),
                    f"reach{n}_reached_max": max(reached), f"reach{n}_reached_sum": sum(reached), f"reach{n}_rows_gb": bound_gb,
                    f"reach{n}_bound_gb": n * P * pitch * 8 / 1e9, f"reach{n}_steps_ms": step_ms,
                    f"reach{n}_hops_and_copy_ms": ms[f"reach{n}"] - ms[f"reach{n}_levels"], f"reach{n}_scratch_mb": scratch_mb})
        lines.append(
            f"reach from {n:2d} seed set(s) of one random pod, to the fixpoint: {ms[f'reach{n}']:9.2f} ms = adjacency and seeds {ms[f'reach{n}_no_step']:.2f} "
            f"+ {steps} steps {step_ms:.2f} + hop values and copy-back {res[f'reach{n}_hops_and_copy_ms']:.2f}; pods reached {min(reached)} - {max(reached)} "
            f"per set, deepest level {int(g['levels'].max())}; rows gathered {bound_gb:.2f} GB (bound {res[f'reach{n}_bound_gb']:.2f} GB: the plane once per set), "
            f"{bound_gb / max(step_ms, 1e-9) * 1e3:.0f} GB/s over the steps; device scratch {scratch_mb:.0f} MB")
    lines.append(json.dumps(res))
    print("\n".join(lines))
    if "out" in kw:
        os.makedirs(os.path.dirname(os.path.abspath(kw["out"])), exist_ok=True)
        with open(kw["out"], "w") as f:
            f.write("\n".join(lines) + "\n")
    sys.exit(0)

if mode == "closure":
    # slots [0, K): the closure both ways into a device plane with the row counts, the zones, next to counts, the adjacency
    # pass and one search from 64 single-pod seed sets: P / 64 such calls are the other way to every row of the closure.
    rng = np.random.default_rng(16)
    seeds = [[int(p)] for p in rng.integers(0, P, 64)]
    plane = torch.empty((P, W), dtype=torch.int64, device="cuda")
    pitch = (W + 15) // 16 * 16
    legs = {"counts": lambda: ta.counts(), "adjacency_from": lambda: ta.adjacency("from", d_out=plane.data_ptr()),
            "reach64": lambda: ta.reach(seeds, want=("reach",)),
            "closure_from": lambda: ta.closure("from", d_out=plane.data_ptr()), "closure_to": lambda: ta.closure("to", d_out=plane.data_ptr()),
            "zones": lambda: ta.zones()}
    z = ta.zones()  # (warm-up, and the figures)
    n_from = ta.closure("from", want=("n_reach",))["n_reach"]
    assert np.array_equal(n_from, z["n_from"])
    # a sample of the closure's rows against the search: the rows of the 64 seed pods
    rows = ta.closure("from", want=("plane",))["plane"][[s[0] for s in seeds]].cpu().numpy().view(np.uint64)
    assert np.array_equal(rows, ta.reach(seeds, want=("reach",))["reach"]), "closure rows differ from cyc_table_reach"
    for f in legs.values():
        f()
    ms = {n: float("inf") for n in legs}
    for _ in range(reps):  # interleaved: every leg once per round
        for n, f in legs.items():
            ms[n] = min(ms[n], timed(f, 1))
    sizes = np.bincount(z["zone"])
    scratch_mb = (P * pitch * 8 + 64 * pitch * 8 + 2 * P * 8 + K * W * 16) / 1e6
    route_ms = (P + 63) // 64 * ms["reach64"]
    res = {"config": config, "pods": P, "slots": K, "words": W, "plane_gb": round(plane_gb, 3), "reps": reps,
           **{n + "_ms": v for n, v in ms.items()}, "closure_gb": P * W * 8 / 1e9, "n_zones": z["n_zones"], "largest_zone": int(sizes.max()),
           "zones_of_one": int((sizes == 1).sum()), "mean_reach": float(z["n_from"].mean()), "max_reach": int(z["n_from"].max()),
           "closure_bits": int(z["n_from"].sum()), "scratch_mb": scratch_mb, "launches": 2 * W, "reach_route_ms": route_ms,
           "closure_over_reach_route": ms["closure_from"] / route_ms, "update_bound_gb_per_pivot_word": 2 * P * pitch * 8 / 1e9}
    lines = [
        f"# {config}: P {P}, K {K}, W {W}, slots [0, {K}); a plane is {plane_gb:.2f} GB, the closure plane {res['closure_gb']:.3f} GB; "
        f"min of {reps} interleaved synchronous calls",
        f"counts {ms['counts']:9.2f} ms   adjacency from {ms['adjacency_from']:9.2f} ms   reach from 64 single-pod sets {ms['reach64']:9.2f} ms",
        f"closure from {ms['closure_from']:9.2f} ms   to {ms['closure_to']:9.2f} ms ({2 * W} launches of the pivot steps)   zones {ms['zones']:9.2f} ms   "
        f"device scratch {scratch_mb:.0f} MB",
        f"{z['n_zones']} zones of {P} pods, the largest {int(sizes.max())} pods, {res['zones_of_one']} of one pod; a pod reaches {res['mean_reach']:.1f} pods "
        f"on average, at most {res['max_reach']}; {res['closure_bits']} bits of the closure set ({res['closure_bits'] / P / P * 100:.2f} %)",
        f"every row by reach: {(P + 63) // 64} calls of 64 sets x {ms['reach64']:.2f} ms = {route_ms / 1e3:.2f} s; the closure takes "
        f"{res['closure_over_reach_route'] * 100:.2f} % of that ({'less' if ms['closure_from'] < route_ms else 'NOT less'} than the reach route)",
        json.dumps(res),
    ]
    print("\n".join(lines))
    if "out" in kw:
        os.makedirs(os.path.dirname(os.path.abspath(kw["out"])), exist_ok=True)
        with open(kw["out"], "w") as f:
            f.write("\n".join(lines) + "\n")
    sys.exit(0)

if mode == "zone_graph":
    # slots [0, K): cyc_table_zone_graph with every output in one call (the bounds known) and as the Python mirror makes it
    # without bounds (a count-only call, then the listing: two closures), interleaved with cyc_table_zones, its yardstick.
    legs = {"zones": lambda: ta.zones(), "zone_graph": zone_graph_single_pass, "zone_graph_count_only": lambda: ta.zone_graph(want=()),
            "zone_graph_unbounded": lambda: ta.zone_graph(want=ZG_ALL)}
    z, g = ta.zones(), zone_graph_single_pass()  # (warm-up, and the figures)
    assert np.array_equal(g["zone"], z["zone"]) and g["n_zones"] == z["n_zones"]
    for f in legs.values():
        f()
    ms = {n: float("inf") for n in legs}
    for _ in range(reps):  # interleaved: every leg once per round
        for n, f in legs.items():
            ms[n] = min(ms[n], timed(f, 1))
    Z, E = g["n_zones"], g["n_edges"]
    Wz = (Z + 63) // 64
    zpitch = (Wz + 15) // 16 * 16
    strict = int(np.unpackbits(g["reach"].cpu().numpy().view(np.uint8)).sum()) - Z  # the set bits of the zone reach plane without its diagonal
    tiers = np.bincount(g["tier"])
    scratch_mb = (2 * Z * zpitch * 8 + Z * 12 + E * 8) / 1e6
    res = {"config": config, "pods": P, "slots": K, "words": W, "reps": reps, **{n + "_ms": v for n, v in ms.items()}, "n_zones": Z, "zone_words": Wz,
           "cover_edges": E, "strict_reach_bits": strict, "tiers": len(tiers), "widest_tier": int(tiers.max()), "widest_tier_at": int(tiers.argmax()),
           "largest_zone": int(g["size"].max()), "zone_graph_over_zones": ms["zone_graph"] / ms["zones"], "extra_scratch_mb": scratch_mb}
    lines = [
        f"# {config}: P {P}, K {K}, W {W}, slots [0, {K}); min of {reps} interleaved synchronous calls",
        f"zones {ms['zones']:9.2f} ms   zone_graph, every output in one call {ms['zone_graph']:9.2f} ms   ratio {res['zone_graph_over_zones']:.3f} "
        f"({'less' if res['zone_graph_over_zones'] < 2 else 'NOT less'} than twice zones)",
        f"zone_graph count-only {ms['zone_graph_count_only']:9.2f} ms   count-only and listing, two closures {ms['zone_graph_unbounded']:9.2f} ms",
        f"{Z} zones of {P} pods ({Wz} words a row of the zone plane), the largest {res['largest_zone']} pods; {E} cover edges of {strict} strict reach bits "
        f"({E / max(strict, 1) * 100:.3f} %: the reduction removes {strict - E}); {len(tiers)} tiers, the widest tier {int(tiers.argmax())} with {int(tiers.max())} zones; "
        f"device scratch beyond zones' {scratch_mb:.1f} MB",
        json.dumps(res),
    ]
    print("\n".join(lines))
    if "out" in kw:
        os.makedirs(os.path.dirname(os.path.abspath(kw["out"])), exist_ok=True)
        with open(kw["out"], "w") as f:
            f.write("\n".join(lines) + "\n")
    sys.exit(0)

if mode == "classes":
    # slots [0, K), Combined: sources only, destinations only, both (with stats), the class table through cells_at, next
    # to counts, the adjacency pass both ways (one pass over the planes where a side of classes makes two per slot) and
    # the plain read.
    adj = torch.empty((P, W), dtype=torch.int64, device="cuda")
    pitch = (W + 15) // 16 * 16
    got = ta.classes("combined", stats=True)  # (warm-up, and the figures)
    reps_s, reps_d = np.unique(got["src"], return_index=True)[1], np.unique(got["dst"], return_index=True)[1]
    legs = {"counts": lambda: ta.counts(), "read2": lambda: read(1),
            "adjacency_from": lambda: ta.adjacency("from", d_out=adj.data_ptr()), "adjacency_to": lambda: ta.adjacency("to", d_out=adj.data_ptr()),
            "classes_src": lambda: ta.classes("combined", want=("src",), stats=True),
            "classes_dst": lambda: ta.classes("combined", want=("dst",), stats=True),
            "classes": lambda: ta.classes("combined", stats=True),
            "cells_at": lambda: ta.cells_at(reps_s, reps_d)}
    for f in legs.values():
        f()
    ms = {n: float("inf") for n in legs}
    for _ in range(reps):  # interleaved: every leg once per round
        for n, f in legs.items():
            ms[n] = min(ms[n], timed(f, 1))
    table = ta.cells_at(reps_s, reps_d, want=("combined",))["combined"]
    scratch_mb = (P * pitch * 8 + P * 20 + K * W * 16) / 1e6
    res = {"config": config, "pods": P, "slots": K, "words": W, "plane_gb": round(plane_gb, 3), "reps": reps,
           **{n + "_ms": v for n, v in ms.items()}, "n_src": got["n_src"], "n_dst": got["n_dst"], "stats": [int(x) for x in got["stats"]],
           "classes_over_counts": ms["classes"] / ms["counts"], "classes_src_over_counts": ms["classes_src"] / ms["counts"],
           "classes_dst_over_counts": ms["classes_dst"] / ms["counts"], "classes_over_read": ms["classes"] / ms["read2"],
           "class_table_cells": int(table.size), "class_table_allowed": int((table == CONN_ALLOWED).sum()), "scratch_mb": scratch_mb}
    lines = [
        f"# {config}: P {P}, K {K}, W {W}, slots [0, {K}), Combined; a plane is {plane_gb:.2f} GB, the view plane of a slot {P * pitch * 8 / 1e9:.3f} GB; "
        f"min of {reps} interleaved synchronous calls",
        f"counts {ms['counts']:9.2f} ms   read of 2 planes {ms['read2']:9.2f} ms   adjacency from {ms['adjacency_from']:9.2f} ms   to {ms['adjacency_to']:9.2f} ms",
        f"classes: sources {ms['classes_src']:9.2f} ms ({res['classes_src_over_counts']:.2f} x counts)   destinations {ms['classes_dst']:9.2f} ms "
        f"({res['classes_dst_over_counts']:.2f} x counts)   both {ms['classes']:9.2f} ms ({res['classes_over_counts']:.2f} x counts, {res['classes_over_read']:.2f} x read)",
        f"{got['n_src']} source classes and {got['n_dst']} destination classes of {P} pods; verification rounds and failed pods "
        f"(sources, destinations) {res['stats']}; device scratch of a side {scratch_mb:.0f} MB",
        f"cells_at over the representatives ({len(reps_s)} x {len(reps_d)} x {K} cells, three views): {ms['cells_at']:9.2f} ms; "
        f"allowed Combined cells of the class table {res['class_table_allowed']} of {res['class_table_cells']}",
        json.dumps(res),
    ]
    print("\n".join(lines))
    if "out" in kw:
        os.makedirs(os.path.dirname(os.path.abspath(kw["out"])), exist_ok=True)
        with open(kw["out"], "w") as f:
            f.write("\n".join(lines) + "\n")
    sys.exit(0)

c = ta.counts()
r = ta.compare(tb, ignore_loopback=True, d_diff=diff.data_ptr())
res = {
    "config": config, "pods": P, "slots": K, "words": W, "plane_gb": round(plane_gb, 3),
    "counts_ms": timed(lambda: ta.counts(), reps),
    "compare_ms": timed(lambda: ta.compare(tb, ignore_loopback=True, d_diff=diff.data_ptr()), reps),
    "compare_nodiff_ms": timed(lambda: ta.compare(tb, ignore_loopback=True), reps),
    "read2_ms": timed(lambda: read(1), reps), "read4_ms": timed(lambda: read(2), reps),
    "combined_allowed": int(c["combined"][:, 5].sum()), "combined_blocked": int(c["combined"][:, 4].sum()), "no_job": c["no_job"],
    "pairs_same_different_ignored": [int(x) for x in r["pairs"]],
}
res["fill_gbs"] = fill_gbs()
res["counts_over_read"] = res["counts_ms"] / res["read2_ms"]
res["compare_over_read"] = res["compare_ms"] / res["read4_ms"]
res["counts_gbs"] = 2 * plane_gb / res["counts_ms"] * 1e3
res["compare_gbs"] = (4 * plane_gb + P * W * 8 / 1e9) / res["compare_ms"] * 1e3
res["read2_gbs"] = 2 * plane_gb / res["read2_ms"] * 1e3
res["read4_gbs"] = 4 * plane_gb / res["read4_ms"] * 1e3
# the listings: pass 1 alone (the count-only calls) and whole pages, next to counts and compare above
sparse, sparse_next, sparse_total = LISTINGS["compare_find"]()
dense, dense_next, dense_total = LISTINGS["find_dense"]()
res.update({
    "compare_find_count_ms": timed(lambda: ta.compare_find(tb, ignore_loopback=True, cap=0), reps),
    "find_count_ms": timed(lambda: ta.find("combined", (CONN_BLOCKED,), cap=0), reps),
    "sparse_count_ms": timed(lambda: ta.compare_find(tc, ignore_loopback=True, cap=0), reps),
    "sparse_page_ms": timed(LISTINGS["compare_find"], reps),
    "sparse_records": len(sparse), "sparse_next": sparse_next, "sparse_total": sparse_total,
    "dense_page_ms": timed(LISTINGS["find_dense"], reps),
    "dense_count_ms": timed(lambda: ta.find("combined", (CONN_ALLOWED,), cap=0), reps),
    "dense_records": len(dense), "dense_next": dense_next, "dense_total": dense_total,
    "compare_find_total": ta.compare_find(tb, ignore_loopback=True, cap=0)[2],
    "find_blocked_total": ta.find("combined", (CONN_BLOCKED,), cap=0)[2],
})
res["compare_find_count_over_compare"] = res["compare_find_count_ms"] / res["compare_nodiff_ms"]
res["find_count_over_counts"] = res["find_count_ms"] / res["counts_ms"]
res["sparse_pass2_ms"] = res["sparse_page_ms"] - res["sparse_count_ms"]
res["dense_pass2_ms"] = res["dense_page_ms"] - res["dense_count_ms"]
find_lines = [
    f"find_count    compare_find count-only {res['compare_find_count_ms']:9.2f} ms  ({res['compare_find_count_over_compare']:.2f} x compare without d_diff, "
    f"{4 * plane_gb / res['compare_find_count_ms'] * 1e3:.0f} GB/s of 4 planes; total {res['compare_find_total']})   "
    f"find(Combined == blocked) count-only {res['find_count_ms']:9.2f} ms  ({res['find_count_over_counts']:.2f} x counts, "
    f"{2 * plane_gb / res['find_count_ms'] * 1e3:.0f} GB/s of 2 planes; total {res['find_blocked_total']})",
    f"compare_find  A against its copy with 64 egress bits flipped: page {res['sparse_page_ms']:9.2f} ms, pass 1 alone {res['sparse_count_ms']:9.2f} ms, "
    f"so pass 2 and the copies {res['sparse_pass2_ms']:.2f} ms; {res['sparse_records']} records, s_next {res['sparse_next']}",
    f"find_dense    one page of find(Combined == allowed), cap P*K = {P * K}: {res['dense_page_ms']:9.2f} ms, pass 1 alone {res['dense_count_ms']:9.2f} ms, "
    f"so pass 2 and the copies {res['dense_pass2_ms']:.2f} ms; {res['dense_records']} records ({res['dense_records'] * 16 / 1e6:.1f} MB), "
    f"s_next {res['dense_next']}, total {res['dense_total']}",
]
lines = [
    f"# {config}: P {P}, K {K}, W {W}; a plane is {plane_gb:.2f} GB; min of {reps} synchronous calls; the box's fill figure {res['fill_gbs']:.0f} GB/s",
    f"counts   {res['counts_ms']:9.2f} ms  {res['counts_gbs']:7.0f} GB/s of 2 planes   read of 2 planes {res['read2_ms']:9.2f} ms "
    f"{res['read2_gbs']:7.0f} GB/s   ratio {res['counts_over_read']:.2f}",
    f"compare  {res['compare_ms']:9.2f} ms  {res['compare_gbs']:7.0f} GB/s of 4 planes + d_diff   read of 4 planes {res['read4_ms']:9.2f} ms "
    f"{res['read4_gbs']:7.0f} GB/s   ratio {res['compare_over_read']:.2f}   (without d_diff {res['compare_nodiff_ms']:.2f} ms)",
    f"Combined allowed {res['combined_allowed']}, blocked {res['combined_blocked']}, cells without a job {res['no_job']}; "
    f"pairs same / different / ignored {res['pairs_same_different_ignored']}",
    *find_lines,
    json.dumps(res),
]
print("\n".join(lines))
if "out" in kw:
    os.makedirs(os.path.dirname(os.path.abspath(kw["out"])), exist_ok=True)
    with open(kw["out"], "w") as f:
        f.write("\n".join(lines) + "\n")
