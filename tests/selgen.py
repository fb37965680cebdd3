"""Directed selector problems: every operator and requirement shape of labelselector.go:66-86 over a chosen
number of distinct label sets, each selector in every role a NetworkPolicy gives one.

tests/randgen.py is the only other generator with every operator, and its problems stay below 120 pods and
20-odd label sets; the generators that reach large tables (planegen, limitgen) use matchLabels and one- or
two-value In only.  selector_problem(L, layout) builds a problem whose label-set table has exactly L entries as
the engine counts them (host.cpp interns pod and namespace label maps into ONE table whose entry 0 is the empty
map; nil and {} both read as entry 0), so a test can put L on either side of a kernel's block and lane edges.

Vocabulary: pod keys k0..k9 and `both` (namespaces carry `both` too, with other values), `tgt` (below),
`nsonly` that only namespaces carry and `ghost` that nothing carries (the dense label table's all-absent
column).  Values "", a..f.  Label sets: a few written out (the empty map, one key only, 8 labels, the
witnesses of the multi-requirement selectors), the rest the points n * STRIDE of a mixed-radix counter over
absent / value per key — distinct by construction, spread over every key, no randomness.

Every selector gets one policy per role, so a wrong verdict of one selector on one label set moves bits no
other policy sets:
  tgt-<s>    policy podSelector <s> (namespace x, half of the pods); its one peer is the pods of a group
  pod-<s>    peer podSelector <s>, once beside namespaceSelector {} and once alone (the policy's namespace)
  ns-<s>     peer namespaceSelector <s> alone
  nspod-<s>  peer namespaceSelector <s> with a pod selector
A policy of the last three roles targets the pods of one group, `tgt = g<i>`: every label set but the empty and
the one-key ones carries one group tag (a group per policy from L = 255 on; below that policies share groups).
Rules sit on one of the two probed ports in turn, so the two job slots differ.

Layouts: "shuffled" one pod per template in a fixed shuffled order (pod index and label-set index never
agree); "runs" every template as a run of RUN identical pods (<= 4 identity runs per 64-pod word: identity-set
builds); "stamped" n_pods pods cycling through the templates (every window of the pods holds every template), with
two more policies in whose rows only posting-built peer rows admit the last two pods (_edge_policies).
For "runs" and "stamped" the planes are the oracle table of the one-pod-per-template problem expanded by
meta["tpl_of"] (expand_rows; tests/test_selgen.py checks the method against Oracle.probe).
"""
from __future__ import annotations

import ipaddress
import json
import random

import numpy as np

# key -> what a pod may hold under it (None: absent); the counter's digits, first key fastest
POD_KEYS = [
    ("k0", [None, "", "a", "b", "c"]),
    ("k1", [None, "", "a", "b", "c", "d", "e"]),
    ("k2", [None, "a", "b"]),
    ("k3", [None, "", "a"]),
    ("k4", [None, "a", "b", "c"]),
    ("k5", [None, "a"]),
    ("k6", [None, "a", "b"]),
    ("k7", [None, "", "f"]),
    ("k8", [None, "a"]),
    ("k9", [None, "a", "b"]),
    ("both", [None, "a", "b"]),
]
PRODUCT = int(np.prod([len(v) for _, v in POD_KEYS]))  # 408,240 points
STRIDE = 252_307  # ~ PRODUCT / golden ratio, coprime to PRODUCT: n * STRIDE mod PRODUCT are distinct points
# namespace -> labels; "e" has {} and "n" has no entry (nil namespace labels): both read as the empty label set
NAMESPACES = {
    "x": {"nsonly": "a", "both": "b"},
    "y": {"nsonly": "b", "both": "c"},
    "z": {"nsonly": "", "both": "a"},
    "u": {"nsonly": "c"},
    "v": {"nsonly": "a", "both": "c"},
    "w": {"nsonly": "e"},
    "t": {"nsonly": "d", "both": "a"},
    "e": {},
}
NS_SETS = len({json.dumps(v, sort_keys=True) for v in NAMESPACES.values() if v})  # distinct non-empty namespace maps
NS_CYCLE = ["x", "y", "x", "z", "x", "u", "x", "v", "x", "e", "x", "n", "x", "w", "x", "t"]  # namespace of template i
CONTAINERS = [{"Name": "c80", "Port": 80, "Protocol": "TCP", "PortName": "serve-80-tcp"},
              {"Name": "c81", "Port": 81, "Protocol": "UDP", "PortName": "serve-81-udp"}]
PROBES = [{"Port": 80, "Protocol": "TCP"}, {"Port": 81, "Protocol": "UDP"}]
RULE_PORTS = [[{"port": 80, "protocol": "TCP"}], [{"port": 81, "protocol": "UDP"}]]
RUN = 16            # pods per template of layout "runs"; the last run is RUN + 5 (P is no multiple of 64)
EXTRA = {"shuffled": 37 + NS_SETS, "runs": 9, "stamped": 3}  # templates that reuse an earlier template's label set
MIN_L = 40
IP0 = int(ipaddress.IPv4Address("10.64.0.1"))


def _expr(key, op, *values):
    e = {"key": key, "operator": op}
    if op in ("In", "NotIn"):
        e["values"] = list(values)
    return e


def single_forms(key, vals=("a", "b", "c", "d", "e")):
    """[(form, selector)]: every one-requirement shape on `key`."""
    a, b, c, d, e = vals
    X = lambda op, *v: {"matchExpressions": [_expr(key, op, *v)]}
    return [
        ("eq", {"matchLabels": {key: a}}),
        ("eq-empty", {"matchLabels": {key: ""}}),   # REQ_EQ_EMPTY: absent or empty
        ("in1", X("In", a)),
        ("in2", X("In", a, b)),
        ("in3", X("In", a, b, c)),
        ("in5", X("In", a, b, c, d, e)),
        ("in-dup", X("In", a, a)),
        ("in-empty", X("In", "", a)),
        ("in-nopod", X("In", a, "z")),              # no label anywhere has the value z
        ("notin1", X("NotIn", a)),
        ("notin2", X("NotIn", a, b)),
        ("notin3", X("NotIn", a, b, c)),
        ("exists", X("Exists")),
        ("dne", X("DoesNotExist")),
    ]


# the 6-requirement selector (matchLabels are walked in key order, then the expressions), the label set that
# holds all six, and per position the change that makes that requirement the first to fail
SIX = {"matchLabels": {"k2": "a", "k5": "a"},
       "matchExpressions": [_expr("k1", "In", "a", "b", "c"), _expr("k4", "NotIn", "c"), _expr("k6", "Exists"),
                            _expr("k9", "DoesNotExist")]}
SIX_HOLDS = {"k2": "a", "k5": "a", "k1": "b", "k4": "a", "k6": "a"}
SIX_FAILS = [("k2", "b"), ("k5", None), ("k1", "d"), ("k4", "c"), ("k6", None), ("k9", "a")]


def six_sets():
    """SIX_HOLDS, then for each position the label set whose first failing requirement is that one."""
    out = [dict(SIX_HOLDS)]
    for key, val in SIX_FAILS:
        s = dict(SIX_HOLDS)
        if val is None:
            del s[key]
        else:
            s[key] = val
        out.append(s)
    return out


MULTI = [
    ("m-2+1", {"matchLabels": {"k2": "a", "k5": "a"}, "matchExpressions": [_expr("k1", "Exists")]}),
    ("m-3+2", {"matchLabels": {"k2": "a", "k3": "", "k6": "b"},
               "matchExpressions": [_expr("k1", "In", "a", "b"), _expr("k9", "NotIn", "a")]}),
    ("m-4+4", {"matchLabels": {"k0": "a", "k2": "b", "k5": "a", "k8": "a"},
               "matchExpressions": [_expr("k1", "NotIn", "a", "b", "c"), _expr("k4", "Exists"), _expr("k7", "DoesNotExist"),
                                    _expr("both", "In", "a", "b")]}),
    ("m-same-notin", {"matchLabels": {"k1": "a"}, "matchExpressions": [_expr("k1", "NotIn", "a")]}),  # matches nothing
    ("m-same-in", {"matchLabels": {"k1": "a"}, "matchExpressions": [_expr("k1", "In", "a", "b")]}),
    ("m-six", SIX),
    ("all", {}),
]
# label sets written out: one key only (every other key sorts below / above it), 8 labels (a binary search of
# depth 3), the witnesses of m-3+2 (k3 absent: "" by absence) and m-4+4, and SIX's seven
SPECIAL = [
    {"k0": "a"}, {"k9": "b"}, {"k4": "a"}, {"k1": ""},
    {"k0": "b", "k1": "c", "k2": "a", "k3": "", "k4": "b", "k6": "a", "k7": "f", "k9": "a"},
    {"k2": "a", "k6": "b", "k1": "b", "k9": "b"},
    {"k2": "a", "k3": "", "k6": "b", "k1": "a", "k9": "b", "k8": "a"},
    {"k0": "a", "k2": "b", "k5": "a", "k8": "a", "k1": "", "k4": "c", "both": "b"},
] + six_sets()
UNTAGGED = 4  # the first SPECIAL sets carry no group tag


def pod_selectors():
    """[(name, selector)] used as policy target, as peer pod selector and beside a namespace selector."""
    out = [(f"k1-{f}", s) for f, s in single_forms("k1")]
    out += [(f"ghost-{f}", s) for f, s in single_forms("ghost")]
    out += [("both-eq", {"matchLabels": {"both": "a"}}), ("k0-in-empty", {"matchExpressions": [_expr("k0", "In", "")]})]
    return out + MULTI


def ns_selectors():
    """[(name, selector)] used as peer namespace selector, alone and with a pod selector."""
    out = [(f"nsonly-{f}", s) for f, s in single_forms("nsonly")]
    out += [(f"nsghost-{f}", s) for f, s in single_forms("ghost")]
    out += [("nsboth-eq", {"matchLabels": {"both": "a"}}),
            ("nsk1-exists", {"matchExpressions": [_expr("k1", "Exists")]}),  # a key only pods carry
            ("ns-m", {"matchLabels": {"nsonly": "a", "both": "c"}, "matchExpressions": [_expr("ghost", "DoesNotExist")]}),
            ("ns-all", {})]
    return out


# selectors that are trivial on purpose: name -> what they match
TRIVIAL = {"all": "all", "ns-all": "all", "m-same-notin": "none", "nsk1-exists": "none"}
for _p in ("ghost", "nsghost"):
    for _f, _ in single_forms("ghost"):
        TRIVIAL[f"{_p}-{_f}"] = "all" if _f in ("eq-empty", "dne") else "none"

# (selector, its near miss, whether the two differ on some label set): a kernel that computes the near miss
# instead must change the table (tests/test_selgen.py checks that it does); In (a, a) and In (a) are the
# same selector by labelselector.go, which the check pins as well
NEAR_MISS = [
    ("k1-in3", {"matchExpressions": [_expr("k1", "In", "a", "b")]}, True),
    ("k1-eq-empty", {"matchLabels": {"k1": "a"}}, True),
    ("k1-eq-empty", {"matchExpressions": [_expr("k1", "DoesNotExist")]}, True),
    ("k1-notin1", {"matchExpressions": [_expr("k1", "DoesNotExist")]}, True),
    ("k1-in-dup", {"matchExpressions": [_expr("k1", "In", "a")]}, False),
    ("nsonly-in3", {"matchExpressions": [_expr("nsonly", "In", "a", "b")]}, True),
    ("nsonly-eq-empty", {"matchExpressions": [_expr("nsonly", "DoesNotExist")]}, True),
]


def _point(n):
    """Label map of counter point n."""
    x, out = (n * STRIDE) % PRODUCT, {}
    for key, vals in POD_KEYS:
        x, d = divmod(x, len(vals))
        if vals[d] is not None:
            out[key] = vals[d]
    return out


def label_sets(n_sets):
    """n_sets distinct non-empty pod label maps: SPECIAL, then counter points (those equal to an earlier one skipped)."""
    assert n_sets >= len(SPECIAL), n_sets
    out, seen = [], set()
    for s in SPECIAL:
        k = json.dumps(s, sort_keys=True)
        assert k not in seen
        seen.add(k)
        out.append(dict(s))
    n = 1
    while len(out) < n_sets:
        s = _point(n)
        n += 1
        k = json.dumps(s, sort_keys=True)
        if s and k not in seen:
            seen.add(k)
            out.append(s)
    return out


def count_label_sets(resources):
    """The engine's label-set count of a Resources value: the empty map, and every distinct non-empty map of a
    Namespaces entry or a pod (one table for both kinds; nil and {} are the empty map)."""
    maps = [v for v in resources["Namespaces"].values()] + [p["Labels"] for p in resources["Pods"]]
    return 1 + len({json.dumps(m, sort_keys=True) for m in maps if m})


def _netpol(name, ns, selector, peer_in, peer_eg, ports):
    return {"apiVersion": "networking.k8s.io/v1", "kind": "NetworkPolicy", "metadata": {"name": name, "namespace": ns},
            "spec": {"podSelector": selector, "policyTypes": ["Ingress", "Egress"],
                     "ingress": [{"from": [peer_in], "ports": ports}], "egress": [{"to": [peer_eg], "ports": ports}]}}


def _templates(L, layout):
    """[(namespace, labels)] of the templates, the group count and each group's namespace (its first template's)."""
    assert L >= MIN_L, L
    n_sets = L - 1 - NS_SETS
    sets = label_sets(n_sets)
    n_groups = len(pod_selectors()) * 2 + len(ns_selectors()) * 2
    G = min(n_groups, n_sets - UNTAGGED)
    for j in range(UNTAGGED, n_sets):
        sets[j]["tgt"] = f"g{(j - UNTAGGED) % G}"
    sets = [{}] + sets  # template 0: the empty label set
    tpls = [(NS_CYCLE[i % 16], s) for i, s in enumerate(sets)]
    for e in range(EXTRA[layout] + (1 if layout == "shuffled" and (len(sets) + EXTRA[layout]) % 64 == 0 else 0)):
        i = len(tpls)
        tpls.append((NS_CYCLE[(i + 1) % 16], sets[(7 * e + 3) % len(sets)]))  # a shared label set, mostly elsewhere
    group_ns = {}
    for ns, s in tpls:
        if "tgt" in s:
            group_ns.setdefault(s["tgt"], ns)
    return tpls, G, group_ns


def _policies(G, group_ns, replace):
    sel = lambda name, s: (replace or {}).get(name, s)
    group = lambda i: f"g{i % G}"
    pols, i = [], 0
    pods, nss = pod_selectors(), ns_selectors()
    for name, s in pods:  # target role: the pods of namespace x the selector matches; peers: one group, everywhere
        peer = {"namespaceSelector": {}, "podSelector": {"matchLabels": {"tgt": group(i)}}}
        pols.append(_netpol(f"tgt-{name}", "x", sel(name, s), peer, peer, RULE_PORTS[i % 2]))
        i += 1
    for name, s in pods:  # peer pod selector: every namespace in one direction, the policy's own in the other
        wide, own = {"namespaceSelector": {}, "podSelector": sel(name, s)}, {"podSelector": sel(name, s)}
        g = group(i)
        pols.append(_netpol(f"pod-{name}", group_ns[g], {"matchLabels": {"tgt": g}}, *((wide, own) if i % 4 < 2 else (own, wide)),
                            RULE_PORTS[i % 2]))
        i += 1
    for name, s in nss:
        g = group(i)
        peer = {"namespaceSelector": sel(name, s)}
        pols.append(_netpol(f"ns-{name}", group_ns[g], {"matchLabels": {"tgt": g}}, peer, peer, RULE_PORTS[i % 2]))
        i += 1
    for x, (name, s) in enumerate(nss):
        g = group(i)
        pname, ps = pods[(5 * x) % len(pods)]
        peer = {"namespaceSelector": sel(name, s), "podSelector": sel(pname, ps)}
        pols.append(_netpol(f"nspod-{name}", group_ns[g], {"matchLabels": {"tgt": g}}, peer, peer, RULE_PORTS[i % 2]))
        i += 1
    return pols


EDGE_NS = "y"  # the namespace of the stamped layout's last two pods


def _edge_policies(g_a, g_b):
    """Layout "stamped": the rows in which the last two pods (groups g_a, g_b, namespace EDGE_NS) show through
    posting-built rows alone.  The targets are the one-key label sets {k0: a} in namespace y and {k4: a} in
    namespace z, which carry no group and which no other policy targets; their peers are posting-built rows beside
    each kind of namespace matcher: every namespace (`tgt = g` twice), the policy's own (`tgt In (g_a, g_b)`: both
    posting ranges), a namespace selector."""
    assert g_a != g_b
    both = {"matchExpressions": [_expr("tgt", "In", g_a, g_b)]}
    wide = [{"namespaceSelector": {}, "podSelector": {"matchLabels": {"tgt": g}}} for g in (g_a, g_b)]
    own = [{"podSelector": both}]
    by_ns = [{"namespaceSelector": {"matchExpressions": [_expr("nsonly", "Exists")]}, "podSelector": both}]
    pol = lambda name, ns, target, p_in, p_eg: {
        "apiVersion": "networking.k8s.io/v1", "kind": "NetworkPolicy", "metadata": {"name": name, "namespace": ns},
        "spec": {"podSelector": {"matchLabels": target}, "policyTypes": ["Ingress", "Egress"],
                 "ingress": [{"from": p_in, "ports": RULE_PORTS[0]}], "egress": [{"to": p_eg, "ports": RULE_PORTS[0]}]}}
    return [pol("edge-y", EDGE_NS, {"k0": "a"}, wide, own), pol("edge-z", "z", {"k4": "a"}, by_ns, by_ns)]


def _requirements(selector):
    return [("eq" if v else "eq-empty", k, [v]) for k, v in (selector.get("matchLabels") or {}).items()] + \
           [(e["operator"], e["key"], e.get("values") or []) for e in selector.get("matchExpressions") or []]


def sparse_rows(policies, resources):
    """(posting-built, scanned) pod-peer rows of a whole-table run that builds sparse rows, each a list of (policy
    namespace, peer), by plan.hpp's rule: a row per pod peer of a target (the peers of targets with equal namespace and selector are one list, equal peers one
    peer) that is not `every pod of every namespace`; it is built from postings when its pod selector is ONE
    requirement `k = v` (v not empty) or `k In` one or two values on a key of the label table."""
    keys = {k for m in resources["Namespaces"].values() if m for k in m} | {k for p in resources["Pods"] for k in p["Labels"]}
    with_pods = {p["Namespace"] for p in resources["Pods"]}
    peers = set()
    for pol in policies:
        ns, spec = pol["metadata"]["namespace"], pol["spec"]
        if ns not in with_pods:
            continue
        for d, pk in (("ingress", "from"), ("egress", "to")):
            for rule in spec.get(d) or []:
                for peer in rule.get(pk) or []:
                    assert "ipBlock" not in peer
                    peers.add((d, ns, json.dumps(spec["podSelector"], sort_keys=True), json.dumps(peer, sort_keys=True)))
    post, scan = [], []
    for _, ns, _, peer in sorted(peers):
        peer = json.loads(peer)
        reqs = _requirements(peer.get("podSelector") or {})
        if not reqs and peer.get("namespaceSelector") == {}:
            continue  # an all-ones row: none is built
        posting = len(reqs) == 1 and reqs[0][1] in keys and (reqs[0][0] == "eq" or (reqs[0][0] == "In" and 1 <= len(reqs[0][2]) <= 2))
        (post if posting else scan).append((ns, peer))
    return post, scan


def engine_label_sets(namespaces, pod_labels):
    """Each pod's label-set index as host.cpp numbers them: 0 the empty map, then the namespaces' maps in the order of
    the Namespaces entries, then the pods' by first appearance."""
    ids = {"{}": 0}
    for m in list(namespaces.values()) + list(pod_labels):
        ids.setdefault(json.dumps(m or {}, sort_keys=True), len(ids))
    return [ids[json.dumps(m, sort_keys=True)] for m in pod_labels]


def _no_fixed_index(order, tpls):
    """The shuffled template order with no pod whose index is its label set's: the table has fewer entries than there
    are pods, so the pod index overtakes the index of a new label set somewhere; a pod with an earlier pod's label
    set is moved to that place."""
    order = list(order)
    for _ in range(len(order)):
        ls = engine_label_sets(NAMESPACES, [tpls[t][1] for t in order])
        n = next((n for n, l in enumerate(ls) if l == n), None)
        if n is None:
            return order
        if n == 0:  # the empty label set first
            order.append(order.pop(0))
            continue
        m = next(m for m in range(n + 1, len(order)) if ls[m] < n)  # (its label set is older than position n)
        order.insert(n, order.pop(m))
    raise AssertionError("no order without a pod at its label set's index")


def selector_problem(L, layout="shuffled", replace=None, n_pods=None, K=2):
    """(policies, resources, probes, meta) with exactly L label sets and K <= 2 probes.  replace: {selector name:
    selector} to use in its place in every role (the near-miss check).  n_pods: layout "stamped" only."""
    tpls, G, group_ns = _templates(L, layout)
    T = len(tpls)
    policies = _policies(G, group_ns, replace)
    order = list(range(T))
    random.Random(f"selgen {L} {layout}").shuffle(order)
    if layout == "shuffled":
        tpl_of = _no_fixed_index(order, tpls)
    elif layout == "runs":
        tpl_of = [t for t in order for _ in range(RUN)] + [order[-1]] * 5
    else:
        assert layout == "stamped" and n_pods >= 2 * T
        tpl_of = [order[n % T] for n in range(n_pods)]
        # the last two pods: the last two templates of namespace EDGE_NS that carry a group, and the policies in
        # which only posting-built rows admit them
        t_b, t_a = [t for t in range(T - 1, -1, -1) if tpls[t][0] == EDGE_NS and "tgt" in tpls[t][1]][:2]
        tpl_of[n_pods - 2], tpl_of[n_pods - 1] = t_a, t_b
        policies += _edge_policies(tpls[t_a][1]["tgt"], tpls[t_b][1]["tgt"])
    pods = [{"Namespace": tpls[t][0], "Name": f"p{n}", "Labels": tpls[t][1], "IP": str(ipaddress.IPv4Address(IP0 + n)),
             "Containers": [dict(c) for c in CONTAINERS]} for n, t in enumerate(tpl_of)]
    resources = {"Namespaces": {k: dict(v) for k, v in NAMESPACES.items()}, "Pods": pods}
    post, scan = sparse_rows(policies, resources)
    meta = {"L": L, "T": T, "tpl_of": np.asarray(tpl_of, np.int64), "groups": G, "post_rows": len(post), "scan_rows": len(scan),
            "post_peers": post,
            "pod_selectors": dict(pod_selectors()), "ns_selectors": dict(ns_selectors()), "trivial": dict(TRIVIAL),
            "near_miss": NEAR_MISS, "templates": tpls}
    return policies, resources, [dict(p) for p in PROBES[:K]], meta


def template_problem(problem):
    """The one-pod-per-template problem of a "runs" / "stamped" problem: pod t is template t."""
    policies, resources, probes, meta = problem
    pods = [{"Namespace": ns, "Name": f"t{t}", "Labels": labels, "IP": str(ipaddress.IPv4Address(IP0 + t)),
             "Containers": [dict(c) for c in CONTAINERS]} for t, (ns, labels) in enumerate(meta["templates"])]
    return policies, {"Namespaces": resources["Namespaces"], "Pods": pods}, probes


def whole_table(oracle, probes, threads=16):
    """Oracle.probe's (status, ingress, egress) from Oracle.cells over every (s, d, k), which walks the cells on
    several threads (Oracle.probe walks them on one; tests/test_selgen.py compares the two)."""
    P, K = oracle.shape(probes)
    s, d, k = (a.ravel().astype(np.int32) for a in np.meshgrid(np.arange(P), np.arange(P), np.arange(K), indexing="ij"))
    c = oracle.cells(probes, s, d, k, threads=threads).reshape(P, P, K)  # [s, d, k]
    assert not (c & 0x40).any(), "a selector problem must not panic"
    status = (c[np.arange(P), np.arange(P), :] & 0x0F).astype(np.uint8)  # a job's status is its destination's: cell (d, d)
    assert np.array_equal(c & 0x0F, np.broadcast_to(status[None], (P, P, K)))

    def pack(bits):  # [row, k, col] -> u64 [row, k, W]
        wide = np.zeros((P, K, (P + 63) // 64 * 64), np.uint8)
        wide[:, :, :P] = bits
        return np.packbits(wide, axis=2, bitorder="little").view(np.uint64).reshape(P, K, -1)

    return status, pack(((c >> 4) & 1).transpose(1, 2, 0)), pack(((c >> 5) & 1).transpose(0, 2, 1))


def expand_rows(table, tpl_of):
    """(status[T,K], R_in[T,K,W], R_eg[T,K,W]) of the P = len(tpl_of) pods' problem from the template problem's
    whole table (status, ingress, egress of Oracle.probe): row t is the plane row of every pod of template t, its
    columns expanded — bit s = the template table's bit tpl_of[s].  The planes are R[tpl_of] (the row expansion
    is left to the caller: planecheck does it on the device)."""
    status, inp, egp = table
    T, K, _ = inp.shape
    P = len(tpl_of)
    out = []
    for plane in (inp, egp):
        bits = np.unpackbits(plane.view(np.uint8).reshape(T, K, -1), axis=2, bitorder="little")[:, :, :T]
        wide = np.zeros((T, K, (P + 63) // 64 * 64), np.uint8)
        wide[:, :, :P] = bits[:, :, tpl_of]
        out.append(np.packbits(wide, axis=2, bitorder="little").view(np.uint64).reshape(T, K, -1))
    return status, out[0], out[1]


def panic_problem(kind, L=MIN_L):
    """The shuffled pods of selector_problem(L) under one policy whose selector is [k0 In (a), k1 <Bogus>], as the
    policy's podSelector (kind "target") or its peers' (kind "peer"): labelselector.go panics on the operator only
    for a label set that passes k0 In (a).  Pod 0 is not such a pod, so the first job does not panic."""
    _, resources, probes, meta = selector_problem(L, "shuffled")
    bogus = {"matchExpressions": [_expr("k0", "In", "a"), {"key": "k1", "operator": "Bogus"}]}
    pods = resources["Pods"]
    first_ok = next(n for n, p in enumerate(pods) if p["Labels"].get("k0") != "a")
    pods[0], pods[first_ok] = pods[first_ok], pods[0]
    assert any(p["Labels"].get("k0") == "a" and p["Namespace"] == "x" for p in pods)
    if kind == "target":
        peer = {"namespaceSelector": {}}
        pol = _netpol("panic-target", "x", bogus, peer, peer, RULE_PORTS[0])
    else:
        assert kind == "peer"
        peer = {"namespaceSelector": {}, "podSelector": bogus}
        pol = _netpol("panic-peer", "x", {}, peer, peer, RULE_PORTS[0])
    return [pol], resources, probes, meta


# ---- the sizes tests/test_gpu_selectors.py runs and tests/test_selgen.py pins ----
DENSE_L = [255, 256, 257, 1023, 1024, 1025]  # k_selectors_dense: lane x = 1's first label set, a chunk's last, the next chunk's first
RUNS_L = [255, 257]
SHARD_L = 1024
QUERY_L = [257, 1025]
SMALL_L = MIN_L            # the replicated instance of the expansion check
POST_L, POST_PODS = 48, 65_537  # posting rows past one LDS pass: W = 1025
