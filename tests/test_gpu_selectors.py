"""labelselector.go:66-86 through every device evaluation path, bit-exact against the oracle, with more label sets
than one block of the dense selector kernel takes.

The device restates the selector walk six times: the binary-search walk of the query path (eval_selector), the
dense table kernel (selectors_dense_blk: a block is one selector x 1024 label sets, thread t taking label sets t,
t + 256, t + 512, t + 768), the lazy walk over the label table (sel_eval over LVT) and over the per-pod table (PLVT),
the one-requirement records (req_holds, <= 2 values) and the label postings (pod_rows_post_blk, 1024 words per LDS
pass).  tests/selgen.py builds problems with every operator and requirement shape in every role and exactly L label
sets (tests/test_selgen.py pins it with the oracle alone, and shows that a kernel computing a near-miss selector
changes the table); here whole device planes are compared inside guard bands (tests/planecheck.py), twice per
context, on every route, each run asserting the route it took.

- test_dense_edges: L = 255 / 256 / 257 / 1023 / 1024 / 1025, one pod per label set in shuffled order, every route.
- test_identity_sets: every template a run of 16 pods, the one-requirement records of peer_bits_blk.
- test_source_shards_posting_rows: posting-built rows of a word window that starts past chunk 0.
- test_posting_rows_past_one_pass: 65,537 pods, 1025 words: the second LDS pass holds one bit.
- test_query_path: the binary-search walk with a label-set table of 257 / 1025 entries.
- test_panics: `[k0 In (a), k1 <Bogus>]` as target and as peer selector panics as the oracle does.
"""
import json

import numpy as np
import pytest

import selgen as sg
from cyclonus_amd import flat
from cyclonus_amd._lib import CyclonusPanic
from cyclonus_amd.engine import Engine
from cyclonus_amd.matcher import build_network_policies
from oracle.oracle import Oracle, OraclePanic
from planecheck import _expected, _run_and_check
from test_gpu_parity import Panicked, assert_same

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("gpu")]


def _case(L, layout, n_pods=None, K=2):
    """A selgen problem and its reference rows (planecheck's case dict; every problem serves one test): the whole
    oracle table for "shuffled" (every pod its own template), the one-pod-per-template table expanded otherwise."""
    prob = sg.selector_problem(L, layout, n_pods=n_pods, K=K)
    pols, res, probes, meta = prob
    P = len(res["Pods"])
    if layout == "shuffled":
        status, R_in, R_eg = sg.whole_table(Oracle(pols, res), probes)
        tpl_of = np.arange(P, dtype=np.int64)
    else:
        tp, tr, _ = sg.template_problem(prob)
        tpl_of = meta["tpl_of"]
        status, R_in, R_eg = sg.expand_rows(sg.whole_table(Oracle(tp, tr), probes), tpl_of)
    T = len(R_in)
    first = np.full(T, -1, np.int64)
    first[tpl_of[::-1]] = np.arange(P - 1, -1, -1)
    assert (first >= 0).all()
    return {"key": (f"selgen-L{L}", T, P, len(probes), layout), "policies": pols, "resources": res, "probes": probes, "meta": meta,
            "tpl_of": tpl_of, "base_of": np.arange(len(probes), dtype=np.int64), "first": first, "status": status[tpl_of],
            "R_in": R_in, "R_eg": R_eg}


def _engine(case):
    """A prepared context (the probe model through the flat tables: no JSON of the pods)."""
    eng = Engine(0)
    sh = flat.prepare_flat(eng, case["policies"], case["resources"], case["probes"])
    _, _, P, K, _ = case["key"]
    assert (sh["pods"], sh["slots"], sh["words"]) == (P, K, (P + 63) // 64), sh
    assert sh["label_sets"] == case["meta"]["L"] and not sh["may_panic"], sh
    return eng


def _routed(eng, case, exp, options, want, sparse=False, **kw):
    """Two runs with `options` set, the reported route compared with `want` ({reported name: value}) and the posting
    counters with the generator's prediction (sparse rows) or 0, then the options back at their defaults."""
    defaults = {n: eng.get_option(n) for n in options}
    for n, v in options.items():
        eng.set_option(n, v)
    _run_and_check(eng, case, exp, None, ctx=str(options), **kw)
    got = {n: eng.get_option(n) for n in want}
    assert got == want, (options, got, want)
    meta = case["meta"]
    rows = (meta["post_rows"], meta["scan_rows"]) if sparse else (0, 0)
    assert (eng.get_option("pod_post_rows"), eng.get_option("pod_scan_rows")) == rows, options
    for n, v in defaults.items():
        eng.set_option(n, v)


@pytest.mark.parametrize("L", sg.DENSE_L)
def test_dense_edges(L):
    """One pod per label set (P = L + 37) on every route.  A lane guard off by one at l0 + 256 == L, a second chunk
    that never runs, a per-pod table read by label set: each moves bits of a policy of its own."""
    case = _case(L, "shuffled")
    eng = _engine(case)
    exp = _expected(case)
    meta = case["meta"]
    assert meta["post_rows"] > 0 and meta["scan_rows"] > 0
    pm = {"pod_words": 0}
    _routed(eng, case, exp, {}, {**pm, "front_fused_active": 1, "launch": 2, "plvt_active": 0, "pl_wave_active": 1})  # auto
    _routed(eng, case, exp, {"graphs": 0, "front_fused": 0}, {**pm, "front_fused_active": 0, "launch": 0})  # eager
    for g in (1, 2):  # the two-branch DAG, replayed and enqueued
        _routed(eng, case, exp, {"front_fused": 0, "graphs": g}, {**pm, "front_fused_active": 0, "launch": g})
    # the fused front's sparse pod-peer rows: the dense table / the lazy walk, a block / a wave per chunk, with and
    # without the per-pod label table
    for lazy in (0, 1):
        for grp in (1, 8):
            for mb in (0, 1024):
                _routed(eng, case, exp, {"pod_words": 0, "sel_lazy": lazy, "pr_group": grp, "plvt_max_mb": mb},
                        {**pm, "front_fused_active": 1, "plvt_active": 1 if mb else 0, "sel_lazy": lazy, "pr_group": grp}, sparse=True)
    _routed(eng, case, exp, {"pod_rows": 0}, {**pm, "front_fused_active": 0})  # identity outcomes and word runs: the DAG
    _routed(eng, case, exp, {"pod_rows": 1}, {**pm, "front_fused_active": 1})
    for v in (0, 1):
        _routed(eng, case, exp, {"pl_wave": v}, {**pm, "front_fused_active": 1, "pl_wave_active": v})
    for v in (0, 1):
        _routed(eng, case, exp, {"member_wave": v}, {**pm, "front_fused_active": 1, "member_wave": v})
        _routed(eng, case, exp, {"member_wave": v, "front_fused": 0}, {**pm, "front_fused_active": 0, "member_wave": v})
    eng.close()


@pytest.mark.parametrize("L", sg.RUNS_L)
def test_identity_sets(L):
    """Identity-set class rows (pod_words 1): peer_bits_blk evaluates each peer's selectors through its
    one-requirement records; one and three representatives per block, the fused front and the DAG."""
    case = _case(L, "runs")
    eng = _engine(case)
    exp = _expected(case)
    ido = {"pod_words": 1}
    _routed(eng, case, exp, {}, {**ido, "front_fused_active": 1})
    for rpb in (1, 3):
        _routed(eng, case, exp, {"pod_words": 1, "class_rpb": rpb}, {**ido, "front_fused_active": 1, "class_rpb": rpb})
        _routed(eng, case, exp, {"pod_words": 1, "class_rpb": rpb, "front_fused": 0}, {**ido, "front_fused_active": 0, "class_rpb": rpb})
    eng.close()


def test_source_shards_posting_rows():
    """Posting-built rows of source shards: 16,421 pods in runs, 257 words in 5 chunks, as materialised rows per pod
    on the fused front with sparse pod-peer rows.  The ingress word window of ranks 1 and 2 of 3 starts at a chunk
    c0 > 0.  (Every shard holds pods of every namespace, so every peer's row is needed: the whole table's counts.)"""
    case = _case(sg.SHARD_L, "runs")
    eng = _engine(case)
    exp = _expected(case)
    meta = case["meta"]
    P = case["key"][2]
    for n, v in (("pod_words", 0), ("pod_rows", 1), ("pr_group", 1)):
        eng.set_option(n, v)
    shards = [eng.rows_shard(3, r, "source") for r in range(3)]
    assert shards[0][0] == 0 and shards[-1][1] == P and all(a[1] == b[0] for a, b in zip(shards, shards[1:]))
    assert shards[1][0] // 64 >= 64 and (P + 63) // 64 == 257  # rank 1's window starts past chunk 0
    for lo, hi in shards:
        _run_and_check(eng, case, exp, None, lo=lo, hi=hi, partition="source", ctx="pr_group 1")
        assert eng.get_option("front_fused_active") == 1 and eng.get_option("pod_words") == 0
        assert (eng.get_option("pod_post_rows"), eng.get_option("pod_scan_rows")) == (meta["post_rows"], meta["scan_rows"])
    eng.close()


def test_posting_rows_past_one_pass():
    """pod_rows_post_blk past PR_POST_WORDS: 65,537 pods are 1025 words, so a posting-built row takes two LDS passes
    and pod 65,536 is the lone bit of the second; pod 65,535 is the last bit of the first.  Both are selected by
    posting-built rows beside every kind of namespace matcher (tests/test_selgen.py).  The whole planes (537 MB each)
    are compared on the device with rows expanded from the template table."""
    case = _case(sg.POST_L, "stamped", sg.POST_PODS, 1)
    eng = _engine(case)
    exp = _expected(case)
    assert case["key"][2] == 65_537 and eng.shape["words"] == 1025 and eng.get_option("pod_words") == 0
    for lazy in (0, 1):
        for grp in (1, 8):
            _routed(eng, case, exp, {"pod_rows": 1, "pr_group": grp, "sel_lazy": lazy},
                    {"pod_words": 0, "front_fused_active": 1, "pr_group": grp, "sel_lazy": lazy}, sparse=True, reps=1)
    eng.close()


@pytest.mark.parametrize("L", sg.QUERY_L)
def test_query_path(L):
    """The query path's k_selectors (a binary search over each label set) with a traffic per pod of the problem: the
    query's own label-set table holds every label set of the pods and namespaces, 257 and 1025 entries."""
    pols, res, _, _ = sg.selector_problem(L, "shuffled")
    pods = res["Pods"]
    P = len(pods)

    def end(p):
        return {"Internal": {"PodLabels": p["Labels"], "NamespaceLabels": res["Namespaces"].get(p["Namespace"]), "Namespace": p["Namespace"]},
                "IP": p["IP"]}

    traffics = [{"Source": end(pods[n]), "Destination": end(pods[(7 * n + 3) % P]), "ResolvedPort": 80 + n % 2,
                 "ResolvedPortName": ("serve-80-tcp", "serve-81-udp")[n % 2], "Protocol": ("TCP", "UDP")[n % 2]} for n in range(P)]
    orc = Oracle(pols)
    want = orc.query_traffic(traffics)
    assert not any(isinstance(w, OraclePanic) for w in want)
    assert {(True, True), (False, False), (True, False), (False, True)} == set(want)  # every outcome occurs
    pol = build_network_policies(True, pols)
    assert pol.engine.query_traffic(traffics) == want
    assert pol.engine.query_traffic_tables(traffics) == want
    tpods = [{"Namespace": p["Namespace"], "Labels": p["Labels"]} for p in pods]
    want_t = orc.query_targets(tpods)
    assert len({json.dumps(w, sort_keys=True) for w in want_t}) > L // 4  # many different target lists
    assert pol.query_targets(tpods) == want_t


@pytest.mark.parametrize("graphs", [-1, 0])
@pytest.mark.parametrize("kind", ["target", "peer"])
def test_panics(kind, graphs):
    """An invalid operator behind `k0 In (a)`: the run panics with the oracle's message (the first panicking job's:
    label sets that fail the first requirement never reach the operator), on the automatic route and with graphs 0."""
    pols, res, probes, _ = sg.panic_problem(kind)
    with pytest.raises(OraclePanic) as e:
        Oracle(pols, res).probe(probes)
    want = Panicked(str(e.value))
    eng = Engine(0)
    eng.set_option("graphs", graphs)
    try:
        eng.build_policies(pols).load_resources(res)
        assert eng.prepare(probes)["may_panic"]
        got = eng.run_host()
    except CyclonusPanic as p:
        got = Panicked(p.msg)
    assert_same(want, got, f"{kind} graphs {graphs}")
    eng.close()
