"""The directed problems of tests/limitgen.py, proved with the oracle alone, for every problem
tests/test_gpu_front_limits.py compares whole device planes with:
(a) counts: the heavy template has exactly n_targets applying targets per direction holding exactly
    n_pod_peers + n_ip_peers peers after Simplify (Oracle.query_targets + Oracle.policy_json); an IP problem
    has exactly the distinct IPBlocks and excepts per direction its case names (from the IR);
(b) every entry counts: the pods the heavy class's peers match (oracle.selector_match / ipblock_match) are
    pairwise disjoint and non-empty, every peer's ports admit some probe in use, and for every base probe and
    direction the heavy template's reference row is exactly the union of the sets of the peers whose ports
    admit the probe, with fewer than P bits; for an IP problem every except removes pods its block would match;
(c) no reference cell has the panic bit, the decoy cases included (planegen.template_rows asserts it);
(d) on the smallest problems the template expansion equals Oracle.probe's whole table."""
import ipaddress
import json

import numpy as np
import pytest

import limitgen as lg
import planegen as pg
from oracle import oracle as O

KEYS = lg.all_keys()
CLASS_KEYS = [k for k in KEYS if k[0] == "class"]
IP_KEYS = [k for k in KEYS if k[0] == "ip"]
_id = lambda k: "-".join(str(x) for x in k)


def _resolved(base, containers):
    """A base probe at a destination with `containers`: (port, name, protocol), or None where no container has
    the port's number or name (the container's protocol is not compared: pod.go:132-148)."""
    for c in containers:
        if base["Port"] in (c["Port"], c["PortName"]):
            return c["Port"], c["PortName"], base["Protocol"]
    return None


def _admits(ports, job):
    if ports is None:
        return True
    (p,), (port, name, proto) = ports, job
    if p["protocol"] != proto:
        return False
    if "endPort" in p:
        return p["port"] <= port <= p["endPort"]
    return p["port"] in (port, name)


def _bits(pods, W):
    row = np.zeros(W * 64, np.uint8)
    row[sorted(pods)] = 1
    return np.packbits(row, bitorder="little").view(np.uint64)


def _matched(peer, policy_ns, res, tpl_of, firsts):
    """The pods a peer matches, by the oracle's selector and IPBlock matchers."""
    pods = res["Pods"]
    if "ipBlock" in peer:
        ib = peer["ipBlock"]
        return {n for n, p in enumerate(pods) if O.ipblock_match(p["IP"], ib["cidr"], ib.get("except", ()))}
    tpls = set()
    for t, n in enumerate(firsts):  # (labels and namespace are the template's)
        p = pods[int(n)]
        ns_ok = (O.selector_match(res["Namespaces"][p["Namespace"]], peer["namespaceSelector"]) if "namespaceSelector" in peer
                 else p["Namespace"] == policy_ns)
        if ns_ok and O.selector_match(p["Labels"], peer["podSelector"]):
            tpls.add(t)
    return {n for n, t in enumerate(tpl_of.tolist()) if t in tpls}


def _ir_peers(ir, direction, prefix):
    """The peers of the IR's targets whose source rules are the policies named prefix*."""
    out = []
    for t in ir[direction].values():
        if all(r["metadata"]["name"].startswith(prefix) for r in t["SourceRules"]):
            out += t["Peers"]
    return out


@pytest.mark.parametrize("key", CLASS_KEYS, ids=_id)
def test_class_problem(key):
    _, n_targets, n_pod, n_ip, layout, K, uniform, decoy = key
    prob = lg.problem(key)
    pols, res, probes, tpl_of, base_of = prob
    P, T = len(res["Pods"]), int(tpl_of.max()) + 1
    W = (P + 63) // 64
    orc = O.Oracle(pols, res)
    assert orc.shape(probes) == (P, K)
    firsts = pg.first_pods(tpl_of, T)
    heavy = res["Pods"][int(firsts[0])]
    # (a) counts after Simplify
    ir = orc.policy_json()
    (tg,) = orc.query_targets([{"Namespace": heavy["Namespace"], "Labels": heavy["Labels"]}])
    for direction in ("Ingress", "Egress"):
        assert len(tg[direction]) == len(set(tg[direction])) == n_targets, direction
        peers = [p for t in tg[direction] for p in ir[direction][t]["Peers"]]
        assert len(peers) == n_pod + n_ip, (direction, len(peers))
        assert sum(p.get("Type") == "IPBlock" for p in peers) == n_ip
        assert len({json.dumps(p, sort_keys=True) for p in peers}) == len(peers)
    # (b) every entry counts
    status, R_in, R_eg, _, _ = pg.reference_planes(orc, prob)  # (c): asserts no panic bit
    assert status.shape == (P, K)
    used = sorted(set(base_of.tolist()))
    for direction, R in (("ingress", R_in), ("egress", R_eg)):
        ents = lg.entries(pols, "heavy-", direction)
        assert len(ents) == n_pod + n_ip
        sets = [_matched(peer, ns, res, tpl_of, firsts) for ns, peer, _ in ents]
        assert all(sets), "a peer that matches no pod"
        assert sum(len(s) for s in sets) == len(set().union(*sets)), "two peers match one pod"
        # ingress: the destination is the heavy pod; egress: a column pod (the heavy pods match no peer)
        conts = heavy["Containers"] if direction == "ingress" else pg.CONTAINERS
        seen = [False] * len(ents)
        for b in used:
            job = _resolved(pg.BASE[b], conts)
            want = set()
            for x, (_, _, ports) in enumerate(ents):
                if job and _admits(ports, job):
                    want |= sets[x]
                    seen[x] = True
            assert np.array_equal(R[0, b], _bits(want, W)), f"{direction} row of base probe {b}"
            assert len(want) < P
        if uniform or direction == "egress":
            assert all(seen), f"{direction}: a peer no probe in use admits"
    assert any(len({R[t, b].tobytes() for b in used}) > 1 for R in (R_in, R_eg) for t in range(1, T)), "no light policy shows"
    if layout == "runs":  # <= 4 identity runs in every 64-pod word, each identity one run
        assert (np.diff(np.nonzero(np.diff(tpl_of))[0]) >= lg.RUN).all() and P == lg.RUN * T


def _ir_blocks(ir, direction):
    return {(p["CIDR"], tuple(p["Except"] or ())) for p in _ir_peers(ir, direction, "ip-") if p.get("Type") == "IPBlock"}


@pytest.mark.parametrize("key", IP_KEYS, ids=_id)
def test_ip_problem(key):
    case = lg.IP_CASES[key[1]]
    prob = lg.problem(key)
    pols, res, probes, tpl_of, base_of = prob
    P = len(res["Pods"])
    W = (P + 63) // 64
    assert P == case["P"]
    orc = O.Oracle(pols, res)
    ir = orc.policy_json()
    T = lg.IP_TEMPLATES
    firsts = pg.first_pods(tpl_of, T)
    status, R_in, R_eg, _, _ = pg.reference_planes(orc, prob)
    assert (status == O.ST_VALID).all()
    for direction, specs, R in (("Ingress", case["blocks_in"], R_in), ("Egress", case["blocks_eg"], R_eg)):
        # (a) distinct IPBlocks and excepts, from the IR
        blocks = _ir_blocks(ir, direction)
        assert len(blocks) == len(specs), direction
        assert sorted(len(ex) for _, ex in blocks) == sorted(s.get("excepts", 0) for s in specs)
        # (b) every except lies in its block and removes pods of its own; the blocks' pods
        ents = lg.entries(pols, "ip-", direction.lower())
        assert len(ents) == len(specs)
        for _, peer, _ in ents:
            ib = peer["ipBlock"]
            net = ipaddress.ip_network(ib["cidr"])
            ex = [ipaddress.ip_network(e) for e in ib.get("except", ())]
            assert all(e.subnet_of(net) for e in ex)
            assert all(not a.overlaps(b) for i, a in enumerate(ex) for b in ex[:i])
            full = {n for n, p in enumerate(res["Pods"]) if O.ipblock_match(p["IP"], ib["cidr"], ())}
            left = {n for n, p in enumerate(res["Pods"]) if O.ipblock_match(p["IP"], ib["cidr"], ib.get("except", ()))}
            assert len(full - left) == sum(e.num_addresses for e in ex) and left, ib["cidr"]
        # the rows of the templates with a policy: the union of their admitted blocks
        for t in range(3):
            mine = lg.entries(pols, f"ip-a{t}", direction.lower())
            for b in sorted(set(base_of.tolist())):
                job = _resolved(pg.BASE[b], pg.CONTAINERS)
                want = set()
                for ns, peer, ports in mine:
                    if _admits(ports, job):
                        want |= _matched(peer, ns, res, tpl_of, firsts)
                assert np.array_equal(R[t, b], _bits(want, W)), (direction, t, b)
        for x, (_, _, ports) in enumerate(ents):
            assert any(_admits(ports, _resolved(pg.BASE[b], pg.CONTAINERS)) for b in set(base_of.tolist())), x
    # what the range and interval plans are expected to count (tests/test_gpu_front_limits.py)
    if key[1] == "match":
        n = [sum(bool(O.ipblock_match(p["IP"], pr["ipBlock"]["cidr"], pr["ipBlock"].get("except", ()))) for p in res["Pods"])
             for _, pr, _ in lg.entries(pols, "ip-", "ingress")]
        assert sorted(n)[-3:] == [4095, 4096, 4097] and sum(x <= 4096 for x in n) == lg.IP_MATCH_RANGE_ROWS
    if key[1] == "iv":  # a block's pods are excepts + 1 runs of consecutive pods (no except first, last or adjacent)
        runs = []
        for _, pr, _ in lg.entries(pols, "ip-", "ingress"):
            m = sorted(_matched(pr, "x", res, tpl_of, firsts))
            runs.append(1 + int((np.diff(m) > 1).sum()))
            assert runs[-1] == len(pr["ipBlock"]["except"]) + 1
        assert sorted(runs) == [15, 15, 16, 16, 17, 17] and sum(n <= 16 for n in runs) == lg.IP_IV_ROWS
    if key[1] == "span":
        spans = []
        for _, pr, _ in lg.entries(pols, "ip-", "ingress"):
            m = [n // 64 for n, p in enumerate(res["Pods"]) if O.ipblock_match(p["IP"], pr["ipBlock"]["cidr"], pr["ipBlock"].get("except", ()))]
            spans.append(max(m) - min(m))
        assert sorted(spans)[-4:] == [254, 255, 255, 256] and sum(s < 256 for s in spans) == lg.IP_SPAN_RANGE_ROWS
        assert W == 257


@pytest.mark.parametrize("key", [("class", 1, 40, 24, "shuffled", 4, True, False), ("class", 3, 20, 5, "shuffled", 40, False, True),
                                 ("class", 2, 5, 2, "runs", 4, True, False), ("ip", "iv")], ids=_id)
def test_expansion_equals_whole_table(key):
    """(d): the expansion against Oracle.probe's whole table."""
    prob = lg.problem(key)
    pols, res, probes, tpl_of, base_of = prob
    orc = O.Oracle(pols, res)
    st, ing, eg = orc.probe(probes)
    status, R_in, R_eg, _, _ = pg.reference_planes(orc, prob)
    assert np.array_equal(status, st)
    assert np.array_equal(pg.expand(R_in, tpl_of, base_of), ing)
    assert np.array_equal(pg.expand(R_eg, tpl_of, base_of), eg)
    assert ing.any() and eg.any()
