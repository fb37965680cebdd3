"""Template-stamped problems whose whole verdict planes have a cheap exact reference.

A plane row of pod p (the ingress row of destination p, the egress row of source p) depends on p's
namespace, labels and containers and on nothing else of p: the other pods enter only as columns.  For
pods stamped from T templates, a whole plane is therefore T x (distinct probe configs) oracle rows per
direction, expanded by template:

    plane[p, k, :] = R[tpl_of[p], base_of[k], :]

`template_problem` builds such a problem, `reference_planes` the rows R and the status plane, and
`expand` the planes.  tests/test_planegen.py checks the method with the oracle alone (rows of other
pods of a template equal the first pod's; the expansion equals Oracle.probe's whole table where that
is affordable); the GPU tests of tests/test_gpu_emit_planes.py compare whole device planes with it.
"""
from __future__ import annotations

import ipaddress
import random

import numpy as np

NAMESPACES = {"x": {"ns": "x", "team": "red"}, "y": {"ns": "y", "team": "blue"}, "z": {"ns": "z", "team": "red", "zone": "1"}}
CONTAINERS = [
    {"Name": "c80", "Port": 80, "Protocol": "TCP", "PortName": "serve-80-tcp"},
    {"Name": "c81", "Port": 81, "Protocol": "UDP", "PortName": "serve-81-udp"},
    {"Name": "c53", "Port": 53, "Protocol": "UDP", "PortName": "dns"},
]
TIERS = ["web", "db", "cache"]
# served, unserved, named and wrong-protocol PortProtocol configs
BASE = [
    {"Port": 80, "Protocol": "TCP"},
    {"Port": 81, "Protocol": "UDP"},
    {"Port": 53, "Protocol": "UDP"},
    {"Port": 443, "Protocol": "TCP"},
    {"Port": "serve-80-tcp", "Protocol": "TCP"},
    {"Port": "dns", "Protocol": "UDP"},
    {"Port": 80, "Protocol": "UDP"},
]
IP0 = int(ipaddress.IPv4Address("10.64.0.1"))


def _pod_ip(n: int) -> str:
    return str(ipaddress.IPv4Address(IP0 + n))


def _layout(r: random.Random, n_templates: int, n_pods: int, layout: str):
    """tpl_of[n]: every template at least once."""
    T = n_templates
    if layout == "shuffled":
        assert n_pods >= T
        tpl_of = [r.randrange(T) for _ in range(n_pods)]
        for t, n in enumerate(r.sample(range(n_pods), T)):
            tpl_of[n] = t
        return tpl_of
    assert layout == "runs" and n_pods >= 22 * T, (layout, n_pods, T)
    unseen = list(range(T))
    r.shuffle(unseen)
    tpl_of, last = [], -1
    while len(tpl_of) < n_pods:
        rem = n_pods - len(tpl_of)
        if unseen:
            t = unseen.pop()
        else:
            t = r.choice([x for x in range(T) if x != last])
        n = min(r.randint(22, 90), rem - 22 * len(unseen))
        if 0 < rem - n < 22:  # no run shorter than 22 at the end
            n = rem if rem <= 90 else rem - 22
        tpl_of += [t] * n
        last = t
    return tpl_of


def _ports(r: random.Random):
    c = r.randrange(4)
    if c == 0:
        return None
    if c == 1:
        return [r.choice([{"port": 80, "protocol": "TCP"}, {"port": 81, "protocol": "UDP"}, {"port": 53, "protocol": "UDP"}])]
    if c == 2:
        return [r.choice([{"port": "serve-80-tcp", "protocol": "TCP"}, {"port": "serve-81-udp", "protocol": "UDP"},
                          {"port": "dns", "protocol": "UDP"}])]
    lo = r.choice([50, 53, 80])
    return [{"port": lo, "endPort": lo + r.choice([1, 30, 400]), "protocol": r.choice(["TCP", "UDP"])}]


def _peer(r: random.Random, n_templates: int, n_pods: int):
    c = r.randrange(3)
    if c == 0:
        return {"podSelector": {"matchLabels": {"tier": r.choice(TIERS)}}}
    if c == 1:
        apps = [f"t{t}" for t in r.sample(range(n_templates), min(n_templates, r.randint(1, 4)))]
        key, val = r.choice([("ns", "x"), ("ns", "y"), ("ns", "z"), ("team", "red"), ("team", "blue")])
        return {"namespaceSelector": {"matchLabels": {key: val}},
                "podSelector": {"matchExpressions": [{"key": "app", "operator": "In", "values": apps}]}}
    addr = IP0 + r.randrange(n_pods)
    net = ipaddress.ip_network((addr, r.randint(22, 27)), strict=False)
    ib = {"cidr": str(net)}
    if r.random() < 0.5:
        inside = int(net.network_address) + r.randrange(net.num_addresses)
        ib["except"] = [str(ipaddress.ip_network((inside, r.randint(28, 32)), strict=False))]
    return {"ipBlock": ib}


def template_problem(seed: int, n_templates: int, n_pods: int, n_slots: int, layout: str):
    """(policies, resources, probes, tpl_of, base_of): pod n is a copy of template tpl_of[n] (own name, own
    increasing IPv4 address), probes[k] = BASE[base_of[k]].  layout "runs": contiguous runs of 22-90 pods
    per template (<= 4 identity runs per 64-pod word: identity-set builds); "shuffled": a random template
    per pod (materialised-row builds, emit order unrelated to pod order).  Pods and policies depend on
    (seed, n_templates, n_pods, layout) only, the probes on (seed, n_slots) only."""
    T = n_templates
    r = random.Random(f"planegen {seed} {T} {n_pods} {layout}")
    ns_names = list(NAMESPACES)
    templates = []
    for t in range(T):
        conts = r.sample(CONTAINERS, r.randint(1, 3))
        templates.append({"Namespace": ns_names[t % 3] if t < 3 else r.choice(ns_names),
                          "Labels": {"app": f"t{t}", "tier": TIERS[t % 3] if t < 3 else r.choice(TIERS)},
                          "Containers": [dict(c) for c in conts]})
    tpl_of = _layout(r, T, n_pods, layout)
    pods = []
    for n, t in enumerate(tpl_of):
        tpl = templates[t]
        pods.append({"Namespace": tpl["Namespace"], "Name": f"t{t}-{n}", "Labels": tpl["Labels"], "IP": _pod_ip(n),
                     "Containers": tpl["Containers"]})
    resources = {"Namespaces": NAMESPACES, "Pods": pods}
    policies = []
    no_policy = set(r.sample(range(T), max(1, round(T / 7))))
    for t in range(T):
        if t in no_policy:
            continue
        spec = {"podSelector": {"matchLabels": {"app": f"t{t}"}}, "policyTypes": ["Ingress", "Egress"]}
        for key, pk in (("ingress", "from"), ("egress", "to")):
            rule = {pk: [_peer(r, T, n_pods) for _ in range(r.randint(1, 3))]}
            ports = _ports(r)
            if ports:
                rule["ports"] = ports
            spec[key] = [rule]
        policies.append({"apiVersion": "networking.k8s.io/v1", "kind": "NetworkPolicy",
                         "metadata": {"name": f"pol-t{t}", "namespace": templates[t]["Namespace"]}, "spec": spec})
    rk = random.Random(f"planegen probes {seed} {n_slots}")
    base_of = [rk.randrange(len(BASE)) for _ in range(n_slots)]
    probes = [dict(BASE[b]) for b in base_of]
    return policies, resources, probes, np.asarray(tpl_of, np.int64), np.asarray(base_of, np.int64)


def first_pods(tpl_of, n_templates):
    """The first pod of every template."""
    t, first = np.unique(tpl_of, return_index=True)
    assert len(t) == n_templates and np.array_equal(t, np.arange(n_templates)), "a template without pods"
    return first


def template_rows(oracle, probes, pods, base_of, bases=BASE):
    """Oracle rows and status of `pods` for every base probe: (R_in[n,B,W], R_eg[n,B,W] u64, S[n,B] u8);
    a base probe no slot uses keeps zero rows.  `bases`: the probe list base_of indexes (a problem may
    bring its own)."""
    P, K = oracle.shape(probes)
    assert K == len(base_of), (K, len(base_of))
    W = (P + 63) // 64
    slot_of = {}
    for k, b in enumerate(base_of):
        slot_of.setdefault(int(b), k)
    R_in = np.zeros((len(pods), len(bases), W), np.uint64)
    R_eg = np.zeros((len(pods), len(bases), W), np.uint64)
    S = np.zeros((len(pods), len(bases)), np.uint8)
    for i, pod in enumerate(pods):
        for b, k in slot_of.items():
            R_in[i, b] = oracle.row(probes, "ingress", int(pod), k, threads=16)
            R_eg[i, b] = oracle.row(probes, "egress", int(pod), k, threads=16)
    bs = sorted(slot_of)
    d = np.repeat(np.asarray(pods, np.int32), len(bs))
    k = np.tile(np.asarray([slot_of[b] for b in bs], np.int32), len(pods))
    cells = oracle.cells(probes, d, d, k, threads=16)
    assert not (cells & 0x40).any(), "a template problem must not panic"
    S[:, bs] = (cells & 0x0F).reshape(len(pods), len(bs))
    return R_in, R_eg, S


def reference_planes(oracle, problem):
    """(status[P,K] u8, R_in[T,B,W], R_eg[T,B,W] u64, tpl_of, base_of): the planes are
    plane[p, k, :] = R[tpl_of[p], base_of[k], :] (`expand`, or the same indexing on the device)."""
    _, _, probes, tpl_of, base_of = problem
    T = int(tpl_of.max()) + 1
    R_in, R_eg, S = template_rows(oracle, probes, first_pods(tpl_of, T), base_of)
    status = S[tpl_of][:, base_of]
    return status, R_in, R_eg, tpl_of, base_of


def expand(R, tpl_of, base_of):
    return R[tpl_of][:, base_of]


# ---- the cases tests/test_gpu_emit_planes.py runs and tests/test_planegen.py validates ----
# Target-row shapes: (K, P, expected emit kernel, layouts).  Row bytes = 8 K ceil(P / 64).
TARGET_SHAPES = [
    (3, 300, "k_emit_words", ("runs",)),                 # 120 B, odd words
    (33, 4000, "k_emit_words", ("shuffled",)),           # 16,632 B, odd, more than one pass of 256 threads
    (2, 700, "k_emit_flat<256,8>", ("shuffled",)),       # 176 B, chunk capped near EMIT_FLAT_MAX_ROWS
    (62, 2112, "k_emit_flat<256,8>", ("runs",)),         # 16,368 B, just under EMIT_WIDE_MIN, chunk 2
    (32, 4096, "k_emit_wide<256,4>", ("runs",)),         # 16,384 B, lower edge
    (4, 32768, "k_emit_wide<256,4>", ("runs", "shuffled")),   # 16,384 B, <= 4 slots at 512 words
    (34, 4000, "k_emit_wide<256,6>", ("runs",)),         # 17,136 B, rows start mid-line
    (50, 4000, "k_emit_wide<256,7>", ("shuffled",)),     # 25,200 B
    (64, 4096, "k_emit_wide<256,8>", ("runs", "shuffled")),   # 32,768 B, upper edge
    (100, 2624, "k_emit_wide<512,7>", ("runs", "shuffled")),  # 32,800 B
    (8, 32800, "k_emit_wide<512,7>", ("runs", "shuffled")),   # 32,832 B, <= 32 slots at 513 words
    (112, 4096, "k_emit_wide<512,7>", ("runs", "shuffled")),  # 57,344 B, upper edge, exactly one pass
    (104, 4416, "k_emit_wide_buf<1024,7>", ("runs", "shuffled")),  # 57,408 B, mid-line heads
    (224, 4096, "k_emit_wide_buf<1024,7>", ("runs", "shuffled")),  # 114,688 B, upper edge, exactly one pass
    (134, 6848, "k_emit_wide<1024,7>", ("runs", "shuffled")),  # 114,704 B, second pass of one chunk
    (240, 4100, "k_emit_wide<1024,7>", ("runs", "shuffled")),  # 124,800 B
]
OPTION_SHAPES = [(8, 32800), (104, 4416)]  # every path option against the reference ("runs")
ALIGN_SHAPES = [(3, 300, "runs"), (34, 4000, "runs"), (104, 4416, "runs"), (134, 6848, "runs"), (2, 700, "shuffled"),
                (4, 32768, "shuffled")]
# Source shards: (K, P, layout, [(lo, hi)] at the start, middle and end of the pods, expected emit)
UNITS = ("k_emit_units<1024,7>", 1)
SOURCE_CASES = [
    (32, 4096, "runs", [(0, 1792), (1024, 2816), (2304, 4096)], UNITS),    # wi 28: 7,168 B, flat sweep, 16 rows a unit
    (30, 4090, "runs", [(0, 1920), (1088, 3008), (2176, 4090)], UNITS),    # wi 30: 7,200 B, group path
    (32, 4096, "runs", [(0, 3584), (256, 3840), (512, 4096)], UNITS),      # wi 56: 14,336 B, group path's upper edge
    (30, 4090, "runs", [(0, 3840), (128, 3968), (256, 4090)], UNITS),      # wi 60: 14,400 B, flat sweep, 7 rows a unit
    (32, 14400, "runs", [(0, 4800), (4800, 9600), (9600, 14400)], UNITS),  # egress rows 57,600 B: one-row units
    (134, 6848, "runs", [(0, 2304), (2304, 4608), (4608, 6848)], UNITS),   # egress rows 114,704 B: two copy_row_buf passes
    (2, 700, "shuffled", [(0, 64), (320, 384), (640, 700)], UNITS),        # wi 1: 16 B slices, the 64-row unit cap
    (3, 500, "runs", [(0, 64), (128, 320), (448, 500)], ("k_emit_words + k_emit_flat<256,8>", 2)),  # odd ingress words
]


def n_templates(K, P):
    """16 templates, 24 for the two largest shapes; fewer where runs of >= 22 pods need it."""
    return 24 if K in (134, 240) else min(16, P // 25)


# The seed of every (K, P, layout): the first that meets the conditions of tests/test_planegen.py
# (distinct class rows, a template with distinct slot rows, the fraction of set bits).
SEEDS = {(2, 700, "shuffled"): 4}


def case_key(K, P, layout):
    return (SEEDS.get((K, P, layout), 0), n_templates(K, P), P, K, layout)


def all_cases():
    """Every (seed, T, P, K, layout) the GPU tests use."""
    keys = [case_key(K, P, lay) for K, P, _, lays in TARGET_SHAPES for lay in lays]
    keys += [case_key(K, P, lay) for K, P, lay in ALIGN_SHAPES]
    keys += [case_key(K, P, "runs") for K, P in OPTION_SHAPES]
    keys += [case_key(K, P, lay) for K, P, lay, _, _ in SOURCE_CASES]
    return sorted(set(keys), key=lambda c: (c[2], c[3], c[4]))
