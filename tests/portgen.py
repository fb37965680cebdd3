"""Directed port-matcher and job-descriptor problems: every entry kind of PortMatcher.Allows (portmatcher.go:10-92,
190-199) against an exact number D of job descriptors and K of job slots, laid out over the 64-destination words so
that every word class the slot words know (one common descriptor, mixed, no valid job) occurs by design.

The random generators reach ports only far from every threshold of csrc/route.hpp (D <= 4 and K <= 4, D <= 32, ingress
K <= 32, uni_desc, slot chunks of 4 and 8).  port_problem(D, K, layout) builds a problem with exactly D descriptors as
host.cpp counts them — the distinct (ResolvedPort, ResolvedPortName, Protocol) of VALID jobs, numbered in first-seen
order over configs, destinations and containers (_jobs restates that rule; meta["desc_ids"] is its prediction) — and
exactly K slots (an AllAvailable config has one per container of the pod with the most, a PortProtocol config one).

Container types: t0 100/TCP "p0" (every pod's first container), t1 140/UDP "web", t2 180/SCTP "" (an empty port name),
dev 141/UDP "web" (the same name on another number), zed 999/TCP "zed" (the last pod's alone), and extras x<e> on
consecutive numbers per protocol (TCP 101.., UDP 142.., SCTP 181..).  Container sets: S0 = t0 t1 [t2], S1 = t0 dev [t2],
FEW = t0, one set per A - 1 extras, ZSET = t0 zed.  PortProtocol configs (repeats allowed: each is a table of its own)
are numbered and named probes that resolve on some sets only; the numbered probe 140/TCP resolves protocol-blind on
t1 (140/UDP) to the VALID job (140, "web", TCP), a descriptor no container has.

Layouts.  "mixed", P = 5 * 64 + 37, by destination word: 0 all S0; 1 S0 but lane 0 (S1); 2 S0 but lanes 0-2 (FEW: no job
in the upper AllAvailable slots, the named / numbered probes fail, the first valid lane is lane 3) and lane 63 (S1);
3 all FEW (upper slots without any job); 4 and 5 cycle through every set; the last pod is ZSET.  Variant "hi" puts the
AllAvailable config last, so zed is the descriptor with id D - 1; variant "lo" probes the name "zed" first: id 0.
"uniform": every pod has the same containers and every probe resolves on them (D <= K: a slot has one descriptor).
"chunks": 65 * 64 + 37 pods (or n_pods), word w laid out as mixed word (w + 4) mod 5, the last word as word 5; the pods are
stamped from templates (group, container set), so tests take one oracle row per template (planegen.template_rows).

Pods come in runs of 16 with one label set per run (<= 4 identity runs per word: identity-set builds are possible),
run r in namespace NS[r mod 3] with tgt = g<r mod 23>.  Every matcher shape has one policy on a group of its own, the
same ports in both directions, under a pod peer, a namespace peer and an IPBlock peer (PEERLESS: a ports-only rule,
an all-peers rule), and a second rule that opens one protocol to one more group; "merge-a" and "merge-b" share one
target, so Combine orders their ports.  meta carries per policy the descriptors its ports admit and the pods its
peers select (a plain restatement: tests/test_portgen.py compares the whole oracle table with it).
"""
from __future__ import annotations

import ipaddress

import numpy as np

PROTOS = ["TCP", "UDP", "SCTP"]
NS = ["x", "y", "z"]
NAMESPACES = {"x": {"ns": "x"}, "y": {"ns": "y"}, "z": {"ns": "z"}}
RUN, GROUPS = 16, 23
P_MIXED, P_CHUNKS = 5 * 64 + 37, 65 * 64 + 37
IP0 = int(ipaddress.IPv4Address("10.64.0.1"))
NONE, VALID, BAD_NAMED, BAD_PORT_PROTOCOL = 0, 1, 2, 3


def _cont(name, port, proto, port_name):
    return {"Name": name, "Port": port, "Protocol": proto, "PortName": port_name}


T0, T1, T2 = _cont("c0", 100, "TCP", "p0"), _cont("c1", 140, "UDP", "web"), _cont("c2", 180, "SCTP", "")
DEV, ZED = _cont("c1", 141, "UDP", "web"), _cont("cz", 999, "TCP", "zed")
_EXTRA_BASE = {"TCP": 101, "UDP": 142, "SCTP": 181}


def _extra(e, A):
    proto = PROTOS[e % 3]
    return _cont(f"cx{e}", _EXTRA_BASE[proto] + e // 3, proto, "" if (A == 2 and e == 2) else f"x{e}")


def _num(port, proto):
    return {"Port": port, "Protocol": proto}


def _dummy(i):
    return {"port": 7000 + i, "protocol": "TCP"}  # no job has such a port


# ---- the matcher shapes: name -> NetworkPolicyPort list (None: the rule has no ports)
MATCHERS = {
    "all-ports": None,
    "proto-only": [{"protocol": "UDP"}],                                  # PE_PROTO
    "numbered": [{"port": 140, "protocol": "UDP"}],                       # a list of one
    "named": [{"port": "web", "protocol": "UDP"}],                        # resolves to 140 and to 141
    "range": [{"port": 101, "endPort": 102, "protocol": "TCP"}],          # TCP jobs at 100, 101, 102, 103
    "range-one": [{"port": 141, "endPort": 141, "protocol": "UDP"}],      # endPort == port
    "named-other-proto": [{"port": "web", "protocol": "TCP"}],            # a container's name on another protocol
    "lowercase": [{"port": 100, "protocol": "tcp"}],                      # the protocol is compared raw
    "no-proto": [{"port": 100}],                                          # an omitted protocol is TCP
    "blind": [{"port": 140, "protocol": "TCP"}],                          # only the protocol-blind numbered probe's job
    "empty-name": [{"port": "", "protocol": "SCTP"}],                     # PortName "" against port name ""
    "list2-first": [{"port": 140, "protocol": "UDP"}, _dummy(0)],
    "list2-last": [_dummy(0), {"port": "web", "protocol": "UDP"}],
    "list3-first": [{"port": "zed", "protocol": "TCP"}, _dummy(0), _dummy(1)],
    "list3-last": [_dummy(0), _dummy(1), {"port": 999, "protocol": "TCP"}],  # odd length, the last entry alone matches
    "list5-first": [{"port": 100, "protocol": "TCP"}] + [_dummy(i) for i in range(4)],
    "list5-last": [_dummy(i) for i in range(4)] + [{"port": 140, "endPort": 141, "protocol": "UDP"}],
    "ports-only": [{"port": 141, "protocol": "UDP"}],                     # a rule without peers: PortsForAllPeers
    "all-peers": None,                                                    # a rule without peers and ports
    "merge-a": [{"port": 180, "protocol": "SCTP"}],
    "merge-b": [{"port": 100, "protocol": "TCP"}, {"port": 140, "endPort": 140, "protocol": "UDP"}],
}
PEERLESS = ("ports-only", "all-peers")
# the group of every policy: the groups of words 4 and 5 (runs 16-22) hold every container set, word 2's (runs 8-11)
# S0, and FEW (run 8) or S1 (run 11); the last pod (zed) is of group 22; groups 0 and 5 have no policy
GROUP_OF = {"list3-last": 22, "list3-first": 21, "range": 20, "proto-only": 19, "named": 18, "list5-last": 17, "empty-name": 16,
            "numbered": 8, "list2-first": 9, "list2-last": 10, "range-one": 11, "all-ports": 1, "named-other-proto": 2,
            "lowercase": 3, "no-proto": 4, "blind": 6, "list5-first": 7, "ports-only": 12, "all-peers": 13, "merge-a": 14,
            "merge-b": 14}
# (policy, its near miss): a kernel that computes the near miss instead must change the table
NEAR_MISS = [
    ("range", [{"port": 101, "endPort": 101, "protocol": "TCP"}]),        # [a, b] -> [a, b - 1]
    ("no-proto", [{"port": 100, "protocol": "tcp"}]),                     # "TCP" -> "tcp"
    ("named", [{"port": 140, "protocol": "UDP"}]),                        # the number it resolves to on some pods only
    ("empty-name", [{"protocol": "SCTP"}]),                               # "" -> absent
]
ENTRY_ORDER = ["list2-first", "list2-last", "list3-first", "list3-last", "list5-first", "list5-last"]


def admits(ports, desc):
    """SpecificPortMatcher.Allows of a NetworkPolicyPort list for the descriptor (port, port name, protocol)."""
    if not ports:
        return True
    port, name, proto = desc
    for e in ports:
        if e.get("protocol", "TCP") != proto:
            continue
        p = e.get("port")
        if p is None or (p == name if isinstance(p, str) else (p <= port <= e["endPort"] if "endPort" in e else p == port)):
            return True
    return False


def _jobs(pods, probes):
    """host.cpp's job slots restated: (status [P, K], slot_desc [P, K] (-1: no VALID job), the descriptors in id order)."""
    maxc = max(len(p["Containers"]) for p in pods)
    K = sum(maxc if c.get("AllAvailable") else 1 for c in probes)
    status, slot_desc, ids = np.zeros((len(pods), K), np.uint8), np.full((len(pods), K), -1, np.int32), {}
    k0 = 0
    for cfg in probes:
        for d, pod in enumerate(pods):
            conts = pod["Containers"]
            if cfg.get("AllAvailable"):
                for i, c in enumerate(conts):
                    status[d, k0 + i] = VALID
                    slot_desc[d, k0 + i] = ids.setdefault((c["Port"], c["PortName"], c["Protocol"]), len(ids))
                continue
            port, proto = cfg["Port"], cfg["Protocol"]
            if isinstance(port, str):
                hit = next((c for c in conts if c["PortName"] == port), None)
                desc, bad = (hit["Port"], port, proto) if hit else None, BAD_NAMED
            else:
                hit = next((c for c in conts if c["Port"] == port), None)
                desc, bad = (port, hit["PortName"], proto) if hit else None, BAD_PORT_PROTOCOL
            status[d, k0] = VALID if hit else bad
            if hit:
                slot_desc[d, k0] = ids.setdefault(desc, len(ids))
        k0 += maxc if cfg.get("AllAvailable") else 1
    return status, slot_desc, list(ids)


def word_classes(status, slot_desc):
    """The DESCW class of every (word, slot): the common descriptor id of the word's VALID lanes, -1 mixed, -2 none."""
    P, K = status.shape
    W = (P + 63) // 64
    out = np.full((W, K), -2, np.int64)
    for w in range(W):
        for k in range(K):
            v = status[64 * w:64 * w + 64, k] == VALID
            ds = set(slot_desc[64 * w:64 * w + 64, k][v].tolist())
            if ds:
                out[w, k] = ds.pop() if len(ds) == 1 else -1
    return out


def _mixed_plan(D, K):
    """(A, the container sets, the PortProtocol configs) of the mixed and chunks layouts."""
    A = 2 if K <= 5 else 3
    N = K - A
    d_min = A + 2  # S0's types, dev and zed
    if D < d_min or N < 2:
        raise ValueError(f"mixed: D >= {d_min} and K >= {A + 2} (D {D}, K {K})")
    blind = D > d_min
    extras = [_extra(e, A) for e in range(D - d_min - blind)]
    S0, S1 = [T0, T1, T2][:A], [T0, DEV, T2][:A]
    sets = [S0, S1, [T0]] + [[T0] + extras[i:i + A - 1] for i in range(0, len(extras), A - 1)]
    assert len(sets) <= 64
    base = [_num("web", "UDP"), _num(140, "UDP"), _num(100, "TCP"), _num("p0", "TCP")]
    for e, x in enumerate(extras):
        base.append(_num(x["PortName"] if (e % 2 and x["PortName"]) else x["Port"], x["Protocol"]))
    pp = [dict(base[i % len(base)]) for i in range(N)]
    if blind:
        pp[min(2, N - 1)] = _num(140, "TCP")
    return A, sets, pp


def _set_of(word, lane, n_sets, last_word, last):
    """The container set (index; -1: ZSET) of a pod by its word's pattern."""
    if last:
        return -1
    pat = 5 if last_word else word % 5
    if pat == 1:
        return 1 if lane == 0 else 0
    if pat == 2:
        return 2 if lane < 3 else (1 if lane == 63 else 0)
    if pat == 3:
        return 2
    if pat >= 4:
        return (lane + (1 if pat == 5 else 0)) % n_sets
    return 0


def _uniform_plan(D, K):
    A = (D + 2) // 3
    N, new = K - A, D - A
    if N < new:
        raise ValueError(f"uniform: every slot has one descriptor for all pods, so D <= K (D {D}, K {K})")
    conts = ([T0, T1, T2] + [_extra(e, 3) for e in range(A)])[:A]
    cand = []
    for j, c in enumerate(conts):  # the container's number and name under the two other protocols: new descriptors
        for x, proto in enumerate(p for p in PROTOS if p != c["Protocol"]):
            cand.append(_num(c["PortName"] if ((j + x) % 2 and c["PortName"]) else c["Port"], proto))
    pp = cand[:new] + [dict((cand[:new] or [_num(100, "TCP")])[i % max(new, 1)]) for i in range(N - new)]
    return conts, pp


def _peers(i, P):
    groups = [f"g{(i + o) % GROUPS}" for o in (3, 8, 9, 17)]  # (the last pod's group, 22, is a peer of list3-first and list3-last)
    if P > 1000:
        net = ipaddress.ip_network((IP0 - 1 + 256 * (i % ((P + 255) // 256)), 24))
    else:
        net = ipaddress.ip_network((IP0 - 1 + 32 * (i % ((P + 31) // 32)), 27))
    return [{"namespaceSelector": {}, "podSelector": {"matchExpressions": [{"key": "tgt", "operator": "In", "values": groups}]}},
            {"namespaceSelector": {"matchLabels": {"ns": NS[(i + 1) % 3]}}},
            {"ipBlock": {"cidr": str(net)}}]


def _peer_mask(peers, pods):
    if peers is None:
        return np.ones(len(pods), bool)
    out = np.zeros(len(pods), bool)
    for peer in peers:
        if "ipBlock" in peer:
            net = ipaddress.ip_network(peer["ipBlock"]["cidr"])
            out |= np.array([ipaddress.ip_address(p["IP"]) in net for p in pods])
        elif "podSelector" in peer:
            groups = set(peer["podSelector"]["matchExpressions"][0]["values"])
            out |= np.array([p["Labels"]["tgt"] in groups for p in pods])
        else:
            out |= np.array([p["Namespace"] == peer["namespaceSelector"]["matchLabels"]["ns"] for p in pods])
    return out


DECOY = {"apiVersion": "networking.k8s.io/v1", "kind": "NetworkPolicy", "metadata": {"name": "decoy", "namespace": "w"},
         "spec": {"podSelector": {}, "policyTypes": ["Ingress", "Egress"], "ingress": [{"from": [{"ipBlock": {"cidr": "10.0.0.0/33"}}]}],
                  "egress": [{"to": [{"ipBlock": {"cidr": "10.0.0.0/33"}}]}]}}


LONG_LIST, LONG_GROUP = 260, 5  # more entries than pl_items keeps in LDS (256), on a group without another policy
_LONG_PORTS = [[{"port": 140, "protocol": "UDP"}], [{"port": "web", "protocol": "UDP"}], [{"port": 100, "protocol": "TCP"}],
               [{"protocol": "SCTP"}], [{"port": 141, "endPort": 141, "protocol": "UDP"}]]


def port_problem(D, K, layout, variant="hi", replace=None, decoy=False, n_pods=None, long_list=False):
    """(policies, resources, probes, meta) with exactly D descriptors and K slots.  variant: "hi" / "lo", the id of the
    last pod's own descriptor (mixed and chunks).  replace: {policy name: ports} to use in its place (the near-miss
    and entry-order checks).  decoy: one more policy with an unparsable CIDR in a namespace without pods (the run may
    panic, and no cell does).  n_pods: layout "chunks" only.  long_list: one more policy, "long-list", of LONG_LIST rules, each
    the /32 of another pod under one of five port lists in turn: a class whose entry list spills past the LDS part of
    the materialised rows, every entry with slot bits of its own."""
    if layout == "uniform":
        conts, pp = _uniform_plan(D, K)
        P = P_MIXED
        pod_sets, sets = [0] * P, [conts]
        probes = [{"AllAvailable": True}] + pp
    else:
        assert layout in ("mixed", "chunks") and variant in ("hi", "lo")
        A, sets, pp = _mixed_plan(D, K)
        P = P_MIXED if layout == "mixed" else (n_pods or P_CHUNKS)
        assert P % 64 and P > 128
        sets = sets + [[T0, ZED]]
        shift = 0 if layout == "mixed" else 4  # chunks: word 64 all FEW, word 65 mixed
        pod_sets = [_set_of(n // 64 + shift, n % 64, len(sets) - 1, n // 64 == P // 64, n == P - 1) % len(sets) for n in range(P)]
        drop = 0 if len(pp) <= 3 else len(pp) - 1  # "lo": the zed probe takes the place of a config that adds no descriptor
        probes = pp + [{"AllAvailable": True}] if variant == "hi" else \
            [_num("zed", "TCP"), {"AllAvailable": True}] + pp[:drop] + pp[drop + 1:]
    pods = []
    for n in range(P):
        r = (n // RUN) % GROUPS
        pods.append({"Namespace": NS[r % 3], "Name": f"p{n}", "Labels": {"tgt": f"g{r}"}, "IP": str(ipaddress.IPv4Address(IP0 + n)),
                     "Containers": [dict(c) for c in sets[pod_sets[n]]]})
    status, slot_desc, descs = _jobs(pods, probes)
    if len(descs) != D or status.shape[1] != K:
        raise ValueError(f"{layout}: built D {len(descs)}, K {status.shape[1]}; asked D {D}, K {K}")
    policies, info = [], []
    for i, (name, ports) in enumerate(MATCHERS.items()):
        ports = (replace or {}).get(name, ports)
        g = GROUP_OF[name]
        peers = None if name in PEERLESS else _peers(i - (name == "merge-b"), P)  # merge-b: merge-a's peers
        rules = [(peers, ports)]
        if peers is not None:  # a second rule: one more group of pods on one protocol (the three protocols in turn)
            rules.append(([{"namespaceSelector": {}, "podSelector": {"matchExpressions": [
                {"key": "tgt", "operator": "In", "values": [f"g{(i + 5) % GROUPS}"]}]}}], [{"protocol": PROTOS[i % 3]}]))
        spec = {"podSelector": {"matchLabels": {"tgt": f"g{g}"}}, "policyTypes": ["Ingress", "Egress"], "ingress": [], "egress": []}
        for rp, rports in rules:
            for key, pk in (("ingress", "from"), ("egress", "to")):
                rule = {} if rp is None else {pk: [dict(p) for p in rp]}
                if rports is not None:
                    rule["ports"] = [dict(e) for e in rports]
                spec[key].append(rule)
            info.append({"name": name, "group": g, "ports": rports, "admits": np.array([admits(rports, d) for d in descs]),
                         "peers": _peer_mask(rp, pods), "second": rp is not peers})
        policies.append({"apiVersion": "networking.k8s.io/v1", "kind": "NetworkPolicy",
                         "metadata": {"name": name, "namespace": NS[g % 3]}, "spec": spec})
    if long_list:
        spec = {"podSelector": {"matchLabels": {"tgt": f"g{LONG_GROUP}"}}, "policyTypes": ["Ingress", "Egress"], "ingress": [], "egress": []}
        for j in range(LONG_LIST):
            rp, rports = [{"ipBlock": {"cidr": pods[(5 * j + 3) % P]["IP"] + "/32"}}], _LONG_PORTS[j % 5]
            spec["ingress"].append({"from": [dict(rp[0])], "ports": [dict(e) for e in rports]})
            spec["egress"].append({"to": [dict(rp[0])], "ports": [dict(e) for e in rports]})
            info.append({"name": "long-list", "group": LONG_GROUP, "ports": rports, "admits": np.array([admits(rports, d) for d in descs]),
                         "peers": _peer_mask(rp, pods), "second": j > 0})
        policies.append({"apiVersion": "networking.k8s.io/v1", "kind": "NetworkPolicy",
                         "metadata": {"name": "long-list", "namespace": NS[LONG_GROUP % 3]}, "spec": spec})
    namespaces = {k: dict(v) for k, v in NAMESPACES.items()}
    if decoy:
        namespaces["w"] = {"ns": "w"}
        policies.append(DECOY)
    tpl_key, tpl_of = {}, []
    for n in range(P):
        tpl_of.append(tpl_key.setdefault(((n // RUN) % GROUPS, pod_sets[n]), len(tpl_key)))
    counts = np.stack([(status == s).sum(0) for s in range(4)], axis=1)
    zed = (999, "zed", "TCP")
    meta = {"D": D, "K": K, "P": P, "layout": layout, "variant": variant, "desc_ids": descs, "status": status, "slot_desc": slot_desc,
            "status_counts": counts, "policies": info, "group_of_pod": np.array([(n // RUN) % GROUPS for n in range(P)]),
            "word_class": word_classes(status, slot_desc), "tpl_of": np.asarray(tpl_of, np.int64), "T": len(tpl_key),
            "zed_id": descs.index(zed) if zed in descs else None, "uniform": layout == "uniform"}
    return policies, {"Namespaces": namespaces, "Pods": pods}, probes, meta


def model_table(meta):
    """(ingress [s, d, k], egress [s, d, k]) bool: the verdicts of the VALID cells restated from meta alone.  A pod of a
    group without policy is open; a policy's rule admits (peer, descriptor) pairs; merge-a and merge-b share a target
    with equal peers, so the target's one peer admits either's ports."""
    P, K = meta["status"].shape
    grp, sd = meta["group_of_pod"], np.maximum(meta["slot_desc"], 0)
    ok_in, ok_eg = np.zeros((P, P, K), bool), np.zeros((P, P, K), bool)
    has = np.zeros(P, bool)
    for pol in meta["policies"]:
        mine = grp == pol["group"]
        has |= mine
        adm = pol["admits"][sd]  # [pod, k]: the pod's job as destination
        ok_in[:, mine] |= pol["peers"][:, None, None] & adm[None, mine]
        ok_eg[mine] |= (pol["peers"][:, None] & adm)[None]
    ok_in[:, ~has] = True
    ok_eg[~has] = True
    valid = (meta["status"] == VALID)[None]
    return ok_in & valid, ok_eg & valid


def unpack(table):
    """Oracle.probe's (status, ingress, egress) as bool [s, d, k] arrays of the VALID cells' verdicts."""
    status, inp, egp = table
    P, K, _ = inp.shape
    bits = lambda a: np.unpackbits(a.view(np.uint8).reshape(P, K, -1), axis=2, bitorder="little")[:, :, :P].astype(bool)
    valid = (status == VALID)[None]
    return bits(inp).transpose(2, 0, 1) & valid, bits(egp).transpose(0, 2, 1) & valid


# ---- the shapes tests/test_gpu_ports.py runs and tests/test_portgen.py pins ----
# ("uniform" needs D <= K — each slot has ONE descriptor for all pods — so D = 32 beside uni_desc is (32, 32))
SHAPES = [(1, 1, "uniform"), (4, 4, "uniform"), (4, 4, "mixed"), (5, 4, "mixed"), (4, 5, "mixed"), (5, 9, "mixed"), (31, 8, "mixed"),
          (32, 8, "mixed"), (33, 8, "mixed"), (33, 4, "mixed"), (5, 33, "mixed"), (32, 32, "mixed"), (33, 33, "mixed"),
          (32, 32, "uniform"), (33, 33, "uniform"), (4, 4, "chunks")]
ORDERED_WALK = [(5, 9), (32, 8), (33, 33)]        # k_class_rows, forced by the decoy policy
CONSUMERS = [(5, 9), (32, 8), (33, 4)]            # query, target effects and batched blocks (mixed)
LONG = [(5, 9), (32, 8), (33, 33)]                # the long-list policy: ingress slot bits of the second and third slot chunk; K > 32
