"""tests/selgen.py pinned with the oracle alone, for every size tests/test_gpu_selectors.py runs:
(a) the label-set count is exactly the L asked for, counted here as host.cpp interns label maps (one table for
    pods and namespaces, the empty map always entry 0), and the pods have the shapes the generator promises;
(b) every selector meant to be non-trivial matches some but not all label sets, the others all or none as declared;
    the three-value In has a pod that only its third value admits, `k = ""` one that lacks the key and one that
    holds it empty, and the 6-requirement selector a label set failing first at each position;
(c) replacing a selector by its near miss changes Oracle.probe's table at the smallest L — so a kernel that
    computes the near miss fails the GPU comparison — and In (a, a) is In (a);
(d) the expansion of the one-pod-per-template table equals the whole table of the replicated pods;
(e) the panic problems panic in the oracle, and not on the first job;
(f) the 65,537-pod problem has 1025 words, every template in the first LDS pass's window, and its last two pods in
    posting-built rows of every kind of namespace matcher — rows that alone admit them somewhere: without the
    posting-built rows of one kind, a row of the table loses the pod's bit (a second LDS pass that never ran shows)."""
import json

import numpy as np
import pytest

import selgen as sg
from oracle.oracle import Oracle, OraclePanic, selector_match

SIZES = sorted({(L, "shuffled") for L in sg.DENSE_L + sg.QUERY_L + [sg.SMALL_L]} | {(L, "runs") for L in sg.RUNS_L + [sg.SHARD_L, sg.SMALL_L]})


def _count(resources):
    maps = list(resources["Namespaces"].values()) + [p["Labels"] for p in resources["Pods"]]
    return len({frozenset(m.items()) for m in maps if m} | {frozenset()})


@pytest.mark.parametrize("L,layout", SIZES, ids=lambda x: str(x))
def test_label_sets_and_pods(L, layout):
    pols, res, probes, meta = sg.selector_problem(L, layout)
    pods, tpl_of = res["Pods"], meta["tpl_of"]
    P = len(pods)
    assert _count(res) == L == meta["L"] == sg.count_label_sets(res)
    assert P % 64 and len(tpl_of) == P and len(probes) == 2 and all(len(p["Containers"]) == 2 for p in pods)
    sets = [json.dumps(p["Labels"], sort_keys=True) for p in pods]
    assert "{}" in sets and max(len(p["Labels"]) for p in pods) >= 8
    assert {"k0": "a"} in [p["Labels"] for p in pods] and {"k9": "b"} in [p["Labels"] for p in pods]  # one key only
    assert {} in res["Namespaces"].values() and "n" not in res["Namespaces"] and {"e", "n"} <= {p["Namespace"] for p in pods}
    assert not any(k.startswith("k") or k in ("tgt", "ghost") for m in res["Namespaces"].values() for k in m)
    assert not any(k in ("nsonly", "ghost") for p in pods for k in p["Labels"])
    by_tpl = {}
    for n, t in enumerate(tpl_of):
        by_tpl.setdefault(int(t), set()).add((pods[n]["Namespace"], sets[n]))
    assert len(by_tpl) == meta["T"] and all(len(v) == 1 for v in by_tpl.values())  # a template's pods are alike
    first = {}
    for t, ((_, s),) in sorted(by_tpl.items()):
        first.setdefault(s, t)
    assert len(first) < meta["T"], "no label set shared by two templates"
    if layout == "shuffled":
        assert P in (L + 37, L + 38)
        # no pod's index is its label set's (the engine numbers them by first appearance, the namespaces' first): a
        # per-pod table read where the per-label-set one is meant, or the reverse, reads another pod's labels
        seen = {"{}": 0}
        for m in res["Namespaces"].values():
            seen.setdefault(json.dumps(m, sort_keys=True), len(seen))
        ls_of_pod = [seen.setdefault(s, len(seen)) for s in sets]
        assert len(seen) == L and ls_of_pod == sg.engine_label_sets(res["Namespaces"], [p["Labels"] for p in pods])
        assert all(l != n for n, l in enumerate(ls_of_pod))
        assert sum(pods[n]["Labels"] == pods[l]["Labels"] for n, l in enumerate(ls_of_pod) if l < P) < P // 10
    else:
        edges = np.nonzero(np.diff(tpl_of))[0] + 1
        lens = np.diff(np.concatenate(([0], edges, [P])))
        assert lens.min() >= 16
        runs = np.concatenate(([1], (np.diff(tpl_of) != 0).astype(np.int64)))
        pad = np.concatenate((runs, np.zeros(-P % 64, np.int64))).reshape(-1, 64)
        assert (pad.sum(1) - pad[:, 0] + 1).max() <= 4  # identity runs in a 64-pod word
    post, scan = sg.sparse_rows(pols, res)
    assert (len(post), len(scan)) == (meta["post_rows"], meta["scan_rows"]) and len(post) > 0 and len(scan) > 0
    # each policy keeps its own peers: no two policies share (namespace, selector) unless groups are shared
    if meta["groups"] == len(pols):
        assert len({(p["metadata"]["namespace"], json.dumps(p["spec"]["podSelector"], sort_keys=True)) for p in pols}) == len(pols)
        # two peers a policy, less the all-ones rows: pod-all's `{}` beside namespaceSelector {}, ns-ns-all's two
        assert meta["post_rows"] + meta["scan_rows"] == 2 * len(pols) - 3


def _matches(selector, maps):
    return [selector_match(m, selector) for m in maps]


@pytest.mark.parametrize("L", [sg.SMALL_L, sg.POST_L, min(sg.DENSE_L)])
def test_selectors_are_not_trivial(L):
    _, res, _, meta = sg.selector_problem(L, "shuffled")
    pod_maps = [p["Labels"] for p in res["Pods"]]
    used_ns = {p["Namespace"] for p in res["Pods"]}
    ns_maps = [res["Namespaces"].get(ns) or {} for ns in sorted(used_ns)]
    for sels, maps in ((meta["pod_selectors"], pod_maps), (meta["ns_selectors"], ns_maps)):
        for name, s in sels.items():
            n = sum(_matches(s, maps))
            want = meta["trivial"].get(name)
            if want is None:
                assert 0 < n < len(maps), (name, n, len(maps))
            else:
                assert n == (len(maps) if want == "all" else 0), (name, n, want)
    P, N = meta["pod_selectors"], meta["ns_selectors"]
    for sels, maps, key in ((P, pod_maps, "k1"), (N, ns_maps, "nsonly")):
        prefix = key if key == "nsonly" else "k1"
        in3, in2 = _matches(sels[f"{prefix}-in3"], maps), _matches(sels[f"{prefix}-in2"], maps)
        third = [m for m, a, b in zip(maps, in3, in2) if a and not b]
        assert third and all(m[key] == "c" for m in third)  # admitted by the third value only
        hit = [m for m, a in zip(maps, _matches(sels[f"{prefix}-eq-empty"], maps)) if a]
        assert any(key not in m for m in hit) and any(m.get(key) == "" for m in hit)
        assert all(m.get(key, "") == "" for m in hit)
    # the 6-requirement selector: a label set that holds all six, and one failing first at each position
    reqs = [{"matchLabels": {k: v}} for k, v in sorted(sg.SIX["matchLabels"].items())] + [{"matchExpressions": [e]} for e in sg.SIX["matchExpressions"]]
    assert len(reqs) == 6
    first_fail = set()
    for m in pod_maps:
        ok = [selector_match(m, r) for r in reqs]
        assert selector_match(m, sg.SIX) == all(ok)
        first_fail.add(ok.index(False) if not all(ok) else 6)
    assert first_fail == set(range(7)), first_fail


def _table(problem):
    pols, res, probes = problem[:3]
    return sg.whole_table(Oracle(pols, res), probes)


def test_whole_table_is_probe():
    pols, res, probes, _ = sg.selector_problem(sg.SMALL_L, "shuffled")
    orc = Oracle(pols, res)
    for a, b in zip(sg.whole_table(orc, probes, threads=3), orc.probe(probes)):
        assert a.dtype == b.dtype and np.array_equal(a, b)


def test_near_misses_change_the_table():
    L = min(sg.DENSE_L)
    base = _table(sg.selector_problem(L, "shuffled"))
    assert len(np.unique(base[1])) > 2 and len(np.unique(base[2])) > 2
    names = set()
    for name, miss, differs in sg.NEAR_MISS:
        got = _table(sg.selector_problem(L, "shuffled", replace={name: miss}))
        assert np.array_equal(got[0], base[0])
        for d, (a, b) in enumerate(zip(got[1:], base[1:])):
            assert np.array_equal(a, b) != differs, f"{name} -> {miss}: the {('ingress', 'egress')[d]} plane {'did not change' if differs else 'changed'}"
        names.add(name)
    assert {"k1-in3", "k1-eq-empty", "k1-notin1", "k1-in-dup"} <= names


@pytest.mark.parametrize("L,layout,n_pods", [(sg.SMALL_L, "runs", None), (sg.POST_L, "stamped", 333)])
def test_expansion_equals_whole_table(L, layout, n_pods):
    prob = sg.selector_problem(L, layout, n_pods=n_pods)
    tpl_of = prob[3]["tpl_of"]
    want = _table(prob)
    status, R_in, R_eg = sg.expand_rows(_table(sg.template_problem(prob)), tpl_of)
    assert np.array_equal(status[tpl_of], want[0])
    assert np.array_equal(R_in[tpl_of], want[1]) and np.array_equal(R_eg[tpl_of], want[2])
    assert set(tpl_of.tolist()) == set(range(prob[3]["T"]))


@pytest.mark.parametrize("kind", ["target", "peer"])
def test_panic_problems(kind):
    pols, res, probes, _ = sg.panic_problem(kind)
    with pytest.raises(OraclePanic) as e:
        Oracle(pols, res).probe(probes)
    assert "invalid operator" in str(e.value) and e.value.cell > 0  # not the first job
    # without the bogus requirement nothing panics: the label sets failing `k0 In (a)` never reach it
    sel = pols[0]["spec"]["podSelector"] if kind == "target" else pols[0]["spec"]["ingress"][0]["from"][0]["podSelector"]
    assert sel["matchExpressions"][1]["operator"] == "Bogus"
    n_pass = sum(p["Labels"].get("k0") == "a" for p in res["Pods"])
    assert 0 < n_pass < len(res["Pods"]) and res["Pods"][0]["Labels"].get("k0") != "a"


def test_posting_problem_shape():
    pols, res, probes, meta = sg.selector_problem(sg.POST_L, "stamped", n_pods=sg.POST_PODS, K=1)
    pods, tpl_of = res["Pods"], meta["tpl_of"]
    P = len(pods)
    assert P == 65_537 and (P + 63) // 64 == 1025 and len(probes) == 1 and _count(res) == sg.POST_L
    assert 40 <= meta["T"] <= 56 and set(tpl_of[:65_536 - 2].tolist()) == set(range(meta["T"]))  # the first pass's window
    kind_of = lambda peer: "own" if "namespaceSelector" not in peer else ("all" if peer["namespaceSelector"] == {} else "selector")
    for q in (65_535, 65_536):  # the last bit of the first pass, the lone bit of the second
        kinds = set()
        for ns, peer in meta["post_peers"]:
            nss = peer.get("namespaceSelector")
            in_ns = pods[q]["Namespace"] == ns if nss is None else selector_match(res["Namespaces"].get(pods[q]["Namespace"]) or {}, nss)
            if in_ns and selector_match(pods[q]["Labels"], peer["podSelector"]):
                kinds.add(kind_of(peer))
        assert kinds == {"own", "all", "selector"}, (q, kinds)
    # ... and a lost bit shows: without the posting-built rows of one kind of namespace matcher (their rules taken out
    # of the policies), some row of the table loses the bit of either pod — no other peer of that row admits them
    tp, tr, _ = sg.template_problem((pols, res, probes, meta))
    full = sg.whole_table(Oracle(tp, tr), probes)
    for kind in ("own", "all", "selector"):
        drop = {(ns, json.dumps(peer, sort_keys=True)) for ns, peer in meta["post_peers"] if kind_of(peer) == kind}
        less = json.loads(json.dumps(tp))
        for pol in less:
            for d, pk in (("ingress", "from"), ("egress", "to")):
                for rule in pol["spec"][d]:
                    rule[pk] = [p for p in rule[pk] if (pol["metadata"]["namespace"], json.dumps(p, sort_keys=True)) not in drop]
                pol["spec"][d] = [rule for rule in pol["spec"][d] if rule[pk]]  # (a rule without peers would admit everyone)
        part = sg.whole_table(Oracle(less, tr), probes)
        for q in (65_535, 65_536):
            c = int(tpl_of[q])
            lost = [((a[:, 0, c // 64] & ~b[:, 0, c // 64]) >> np.uint64(c % 64)) & np.uint64(1) for a, b in zip(full[1:], part[1:])]
            assert lost[0].any() or lost[1].any(), (kind, q)
