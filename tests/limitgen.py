"""Directed problems that cross the capacity limits of the class-row, membership and IP-row kernels.

tests/randgen.py and tests/planegen.py give a pod a handful of policies with a few peers each, so the
fixed-size stages of the front (LDS lists, lane groups, register batches: the table in
tests/test_gpu_front_limits.py) are only ever filled part-way.  The problems here fill them to a chosen
count.  Both generators return planegen.template_problem's 5-tuple (policies, resources, probes, tpl_of,
base_of), so planegen.reference_planes is the reference and a whole plane is a few oracle rows.

class_problem: one "heavy" template that n_targets policies select, holding n_pod_peers + n_ip_peers
peers in all, every peer matching pods no other peer matches: each list entry of the heavy class decides
bits of its rows on its own, so a dropped or misplaced entry changes the table.

ip_problem: IPBlock-only policies over pods numbered in address order, the IPBlocks per direction and
the excepts of each chosen by the caller, every except the network of existing pods of its block.

tests/test_limitgen.py proves the counts and the sole-contributor property with the oracle alone.
"""
from __future__ import annotations

import ipaddress
import random

import numpy as np

from planegen import BASE, CONTAINERS, NAMESPACES

VALID_BASES = [0, 1, 2, 4, 5, 6]  # the base probes every pod with all three containers serves
RUN = 22                       # pods per identity run of layout "runs" (<= 4 runs in any 64-pod word)
HEAVY_PODS, SPARE = 3, 4       # shuffled: pods of the heavy template; identities no peer selects
LIGHT = 3                      # column identities with a small policy of their own
A0 = int(ipaddress.IPv4Address("10.64.0.0"))
RESERVED = int(ipaddress.IPv4Address("10.99.0.0"))  # ip_problem: /30 networks of chosen pod pairs

_NUMBERED = [{"port": 80, "protocol": "TCP"}, {"port": 81, "protocol": "UDP"}, {"port": 53, "protocol": "UDP"}]
_NAMED = [{"port": "serve-80-tcp", "protocol": "TCP"}, {"port": "serve-81-udp", "protocol": "UDP"},
          {"port": "dns", "protocol": "UDP"}]
_RANGED = [{"port": 50, "endPort": 60, "protocol": "UDP"}, {"port": 80, "endPort": 81, "protocol": "TCP"},
           {"port": 53, "endPort": 500, "protocol": "UDP"}]


def rule_ports(j: int):
    """The ports of the rule of entry j: none, numbered, named, ranged in turn, each kind over three values."""
    c, v = j % 4, (j // 4) % 3
    return None if c == 0 else [dict((_NUMBERED, _NAMED, _RANGED)[c - 1][v])]


def _ip(a: int) -> str:
    return str(ipaddress.IPv4Address(a))


def _netpol(name, ns, selector, ingress, egress):
    return {"apiVersion": "networking.k8s.io/v1", "kind": "NetworkPolicy", "metadata": {"name": name, "namespace": ns},
            "spec": {"podSelector": {"matchLabels": selector}, "policyTypes": ["Ingress", "Egress"], "ingress": ingress,
                     "egress": egress}}


def ip_rule_ports(j: int):
    """ip_problem's rules: none, numbered, named, ranged in turn, each admitting one of the first two base probes."""
    return (None, [dict(_NUMBERED[0])], [dict(_NAMED[1])], [dict(_RANGED[1])])[j % 4]


def _rules(key, peers, ports=rule_ports):
    out = []
    for j, peer in peers:
        rule = {key: [peer]}
        if ports(j):
            rule["ports"] = ports(j)
        out.append(rule)
    return out


DECOY = _netpol("decoy", "w", {}, [{"from": [{"ipBlock": {"cidr": "10.0.0.0/33"}}]}], [{"to": [{"ipBlock": {"cidr": "10.0.0.0/33"}}]}])


def probes_of(K: int):
    """K <= 4: distinct base probes every pod serves when all pods have all containers (one VALID descriptor
    per slot: the UNI egress variants); more: every base probe in turn (repeated bases, unserved ones among them)."""
    base_of = VALID_BASES[:K] if K <= 4 else [k % len(BASE) for k in range(K)]
    return [dict(BASE[b]) for b in base_of], np.asarray(base_of, np.int64)


def class_problem(n_targets, n_pod_peers, n_ip_peers, layout="shuffled", K=4, uniform=True, decoy=False):
    """Template 0 is the heavy one (namespace x, labels g0..g{n_targets-1}); policy i selects {g_i: "1"} and
    holds the entries j = i mod n_targets of the n_pod_peers + n_ip_peers, one per rule, the same in both
    directions.  Template 1 + e is column identity e with the label id = e: pod peer j selects id = j (every
    fifth through a namespaceSelector onto namespace y, where that identity then lives), IP peer j is the /32
    of the middle pod of identity j; SPARE more identities match no peer; LIGHT identities have a small policy
    of their own."""
    M = n_pod_peers + n_ip_peers
    assert n_targets >= 1 and M >= 1
    E = M + SPARE
    r = random.Random(f"limitgen class {n_targets} {n_pod_peers} {n_ip_peers} {layout}")
    in_y = [j < n_pod_peers and j % 5 == 3 for j in range(E)]
    heavy_conts = CONTAINERS if uniform else [CONTAINERS[0], CONTAINERS[2]]
    templates = [{"Namespace": "x", "Labels": {"app": "heavy", **{f"g{i}": "1" for i in range(n_targets)}}, "Containers": heavy_conts}]
    for e in range(E):
        templates.append({"Namespace": "y" if in_y[e] else ("z" if e >= M else "x"), "Labels": {"app": "col", "id": str(e)},
                          "Containers": CONTAINERS})
    if layout == "shuffled":
        tpl_of = [0] * HEAVY_PODS + list(range(1, E + 1))
        r.shuffle(tpl_of)
    else:
        assert layout == "runs"
        order = list(range(E + 1))
        r.shuffle(order)
        tpl_of = [t for t in order for _ in range(RUN)]
    pods, mid = [], {}
    for n, t in enumerate(tpl_of):
        tp = templates[t]
        pods.append({"Namespace": tp["Namespace"], "Name": f"t{t}-{n}", "Labels": tp["Labels"], "IP": _ip(A0 + 1 + n),
                     "Containers": [dict(c) for c in tp["Containers"]]})
    for t in range(1, E + 1):
        members = [n for n, x in enumerate(tpl_of) if x == t]
        mid[t - 1] = members[len(members) // 2]
    peers = []
    for j in range(M):
        if j >= n_pod_peers:
            peers.append((j, {"ipBlock": {"cidr": pods[mid[j]]["IP"] + "/32"}}))
        elif in_y[j]:
            peers.append((j, {"namespaceSelector": {"matchLabels": {"ns": "y"}}, "podSelector": {"matchLabels": {"id": str(j)}}}))
        else:
            peers.append((j, {"podSelector": {"matchLabels": {"id": str(j)}}}))
    policies = []
    for i in range(n_targets):
        mine = peers[i::n_targets]
        policies.append(_netpol(f"heavy-g{i}", "x", {f"g{i}": "1"}, _rules("from", mine), _rules("to", mine)))
    for e in r.sample(range(E), LIGHT):  # the heavy pods on one port, and a network around the first pods
        ns = templates[1 + e]["Namespace"]
        policies.append(_netpol(f"light-{e}", ns, {"id": str(e)},
                                [{"from": [{"namespaceSelector": {"matchLabels": {"ns": "x"}}, "podSelector": {"matchLabels": {"app": "heavy"}}}],
                                  "ports": [dict(_NUMBERED[e % 3])]}],
                                [{"to": [{"ipBlock": {"cidr": _ip(A0) + "/27", "except": [_ip(A0 + 4) + "/30"]}}]}]))
    namespaces = dict(NAMESPACES)
    if decoy:
        namespaces["w"] = {"ns": "w"}
        policies.append(DECOY)
    probes, base_of = probes_of(K)
    return policies, {"Namespaces": namespaces, "Pods": pods}, probes, np.asarray(tpl_of, np.int64), base_of


def entries(policies, prefix, direction):
    """[(policy namespace, peer, ports)] of the rules of the policies named prefix*, as written."""
    key = "from" if direction == "ingress" else "to"
    return [(pol["metadata"]["namespace"], rule[key][0], rule.get("ports")) for pol in policies
            if pol["metadata"]["name"].startswith(prefix) for rule in pol["spec"][direction]]


# ---- IPBlock-only problems ----
IP_TEMPLATES = 6  # a0, a1, a2 carry the policies; the blocks are dealt over them


def block(first, bits, excepts=0, ex_bits=32):
    """An IPBlock spec: the /bits network at address A0 + first, `excepts` of its pods excepted by their
    /ex_bits networks (every except other pods, none the network's first or last pod, no two adjacent when
    the network has room: the block's pods are then excepts + 1 intervals of the address order)."""
    return {"first": first, "bits": bits, "excepts": excepts, "ex_bits": ex_bits}


def pair(pod_a, pod_b, slot):
    """The reserved /30 number `slot` whose only pods are pod_a and pod_b (they get its addresses)."""
    return {"pair": (pod_a, pod_b), "slot": slot}


def _ipblock(spec, P, addr):
    if "pair" in spec:
        return {"cidr": _ip(RESERVED + 4 * spec["slot"]) + "/30"}
    net = ipaddress.ip_network((A0 + spec["first"], spec["bits"]))
    lo, hi = int(net.network_address) - A0, int(net.broadcast_address) - A0
    inside = [n for n in range(max(lo, 0), min(hi, P - 1) + 1) if addr[n] == A0 + n]  # (not moved to a reserved /30)
    ib = {"cidr": str(net)}
    cnt, step = spec["excepts"], 1 << (32 - spec["ex_bits"])
    if cnt:
        cells = (len(inside) - 2 * step) // step  # aligned groups of `step` pods strictly inside
        assert cells >= cnt, (spec, len(inside))
        stride = max(1, cells // cnt)
        first = (inside[0] // step + 1) * step
        ib["except"] = [f"{_ip(A0 + first + i * stride * step)}/{spec['ex_bits']}" for i in range(cnt)]
        assert first + (cnt - 1) * stride * step + step - 1 < inside[-1]
    return ib


def ip_problem(P, blocks_in, blocks_eg, K=4, decoy=False, far_from=None):
    """P pods in namespace x, pod n at address A0 + n (the pods of a `pair` at their reserved /30 instead, pods
    n >= far_from 65,536 addresses further on), template n mod IP_TEMPLATES shuffled in blocks of 64 pods.  The IPBlocks of blocks_in / blocks_eg are the
    ingress / egress peers, one per rule, dealt in turn over the policies of templates a0, a1, a2."""
    r = random.Random(f"limitgen ip {P}")
    tpl_of = []
    while len(tpl_of) < P:
        w = [n % IP_TEMPLATES for n in range(64)]
        r.shuffle(w)
        tpl_of += w
    tpl_of = tpl_of[:P]
    addr = [A0 + n + (65536 if far_from is not None and n >= far_from else 0) for n in range(P)]
    for spec in blocks_in + blocks_eg:
        if "pair" in spec:
            for u, n in enumerate(spec["pair"]):
                assert addr[n] != A0 + n + 65536 and (addr[n] == A0 + n or addr[n] == RESERVED + 4 * spec["slot"] + 1 + u), "a pod in two pairs"
                addr[n] = RESERVED + 4 * spec["slot"] + 1 + u
    pods = [{"Namespace": "x", "Name": f"a{t}-{n}", "Labels": {"app": f"a{t}"}, "IP": _ip(addr[n]),
             "Containers": [dict(c) for c in CONTAINERS]} for n, t in enumerate(tpl_of)]
    npol = 3
    peers_in = [(j, {"ipBlock": _ipblock(s, P, addr)}) for j, s in enumerate(blocks_in)]
    peers_eg = [(j + 1, {"ipBlock": _ipblock(s, P, addr)}) for j, s in enumerate(blocks_eg)]
    policies = [_netpol(f"ip-a{t}", "x", {"app": f"a{t}"}, _rules("from", peers_in[t::npol], ip_rule_ports),
                        _rules("to", peers_eg[t::npol], ip_rule_ports))
                for t in range(npol)]
    namespaces = dict(NAMESPACES)
    if decoy:
        namespaces["w"] = {"ns": "w"}
        policies.append(DECOY)
    probes, base_of = probes_of(K)
    return policies, {"Namespaces": namespaces, "Pods": pods}, probes, np.asarray(tpl_of, np.int64), base_of


# ---- the cases tests/test_gpu_front_limits.py runs and tests/test_limitgen.py proves ----
# (n_targets, n_pod_peers, n_ip_peers): materialised rows; m = pod + IP peers is the heavy class's list
PM_CASES = [
    (1, 40, 24),      # m 64: one lane group, the sorted list's upper edge
    (1, 41, 24),      # m 65: a second lane group, unsorted
    (3, 200, 55),     # m 255: the tail batch of 7, one short of the LDS part
    (3, 200, 56),     # m 256: the LDS part full
    (3, 200, 57),     # m 257: one spilled entry
    (3, 230, 90),     # m 320: the spilled lane group full
    (3, 231, 90),     # m 321: a second spilled lane group of one entry
    (63, 40, 23),     # 63 targets with one peer each
    (64, 40, 24),     # a full target chunk
    (65, 170, 133),   # a second target chunk of one target; m 303
    (130, 400, 121),  # three target chunks; m 521
]
PM_K40 = [(3, 200, 56), (3, 200, 57), (130, 400, 121)]  # also with 40 slots (no slot bit rows: the general loop)
PM_OPTIONS = PM_K40[1:]  # ... and these with every path option, a decoy and row shards
# identity sets: (n_targets, n_pod_peers, n_ip_peers, uniform)
IDO_CASES = [
    (3, 127, 0, True),     # m 127
    (3, 128, 0, True),     # m 128: the flat LDS list full
    (3, 129, 0, True),     # m 129: the direct target walk
    (3, 111, 17, True),    # m 128 flat, one IP peer past the staged ones
    (3, 129, 15, True),
    (3, 129, 16, True),    # the staged IP peers full
    (3, 129, 17, False),   # one past them; the heavy pods serve two of the three ports
    (3, 129, 33, True),
    (65, 129, 16, False),  # a second batch of membership targets
    (130, 200, 33, True),  # three
]


def pm_key(case, K=4, decoy=False):
    return ("class",) + tuple(case) + ("shuffled", K, True, decoy)


def ido_key(case):
    return ("class",) + tuple(case[:3]) + ("runs", 4, case[3], False)


def _fast_blocks(total):
    """16 disjoint /27 networks of 32 pods with `total` excepts in all: 16 each, the last one 15 / 16 / 17."""
    return [block(32 * b, 27, 16 if b < 15 else total - 240) for b in range(16)]


def _iv_blocks():
    """/25 (two words) and /26 networks with 14 / 15 / 16 excepts (15 / 16 / 17 intervals), one of each."""
    return [block(128 * b, 25, 14 + b) for b in range(3)] + [block(384 + 64 * b, 26, 14 + b) for b in range(3)]


IP_P = 512
# name -> ip_problem's arguments; the egress blocks are the ingress ones in another order
IP_CASES = {}
for _n in (255, 256, 257):
    IP_CASES[f"fast{_n}"] = dict(P=IP_P, blocks_in=_fast_blocks(_n), blocks_eg=_fast_blocks(_n)[::-1])
for _n in (191, 192, 193):  # one /24 with every except, 23 /29 networks around it
    _b = [block(0, 24, _n)] + [block(256 + 8 * b, 29) for b in range(23)]
    IP_CASES[f"batch{_n}"] = dict(P=IP_P, blocks_in=_b, blocks_eg=_b[::-1], decoy=True)
IP_IV_ROWS = 4  # (per direction: the blocks of <= 16 intervals)
IP_CASES["iv"] = dict(P=640, blocks_in=_iv_blocks(), blocks_eg=_iv_blocks()[::-1])
# pods 0..4096 at A0 + n, the other 203 far away: /20 = 4096 pods, less one /32 = 4095, /19 = 4097; and small networks
_match = [block(0, 20), block(0, 20, 1), block(0, 19), block(1024, 24, 3, 30), block(64, 26)]
IP_CASES["match"] = dict(P=4300, blocks_in=_match, blocks_eg=_match[::-1], far_from=4097)
IP_MATCH_RANGE_ROWS = 4  # (per direction: all but the /19)
# 257 words: pairs of pods 256, 255, 255 and 254 words apart (bit 63 of the window's last word among them)
_span = [pair(3, 256 * 64 + 10, 0), pair(64 + 7, 256 * 64 + 20, 1), pair(40, 255 * 64 + 63, 2), pair(2 * 64 + 9, 256 * 64 + 30, 3),
         block(8192, 24, 2)]
IP_CASES["span"] = dict(P=16448, K=2, blocks_in=_span, blocks_eg=_span[::-1])
IP_SPAN_RANGE_ROWS = 4  # (per direction: all but the pair 256 words apart)


def ip_key(name):
    return ("ip", name)


def problem(key):
    if key[0] == "class":
        return class_problem(*key[1:])
    return ip_problem(**IP_CASES[key[1]])


def all_keys():
    keys = [pm_key(c) for c in PM_CASES] + [pm_key(c, 40) for c in PM_K40] + [pm_key(c, 40, True) for c in PM_OPTIONS]
    keys += [ido_key(c) for c in IDO_CASES] + [ip_key(n) for n in IP_CASES]
    return keys
