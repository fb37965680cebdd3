"""connectivity.ComparisonTable (pkg/connectivity/comparisontable.go) over lazy probe.Tables: every method against
a literal restatement of the Go file written over Table.get Items (dict walks), on config #1's resources with
two policy sets of tests/golden/yaml; the tables are PlaneCells views of the oracle's planes, so no GPU is needed."""
import copy
import ctypes
import json
import os

import pytest

from cyclonus_amd import _lib
from cyclonus_amd._lib import CyclonusPanic
from cyclonus_amd.comparison import ComparisonTable, short_string
from cyclonus_amd.loader import read_policies_from_path
from cyclonus_amd.probe import PlaneCells, Resources, Table, new_all_available, new_probe_config
from cyclonus_amd.tablewriter import render
from oracle.oracle import Oracle

GOLD = os.path.join(os.path.dirname(__file__), "golden")
NIL_MAP = "assignment to entry in nil map"


def _resources(upper=False):
    """Config #1's pods; `upper`: with the container protocols the by-protocol maps exist for (config #1
    writes "tcp", for which ValueCountsByProtocol :90,102 assigns into a nil map) and one UDP container."""
    res = copy.deepcopy(json.load(open(os.path.join(GOLD, "config1.json")))["resources"])
    if upper:
        for p in res["Pods"]:
            for c in p["Containers"]:
                c["Protocol"] = c["Protocol"].upper()
        res["Pods"][4]["Containers"][1]["Protocol"] = "UDP"
    return res


POLICY_SETS = {
    "simple": lambda: read_policies_from_path(os.path.join(GOLD, "yaml", "simple-example")),
    "upstream": lambda: (read_policies_from_path(os.path.join(GOLD, "yaml", "upstream_test_cases")) +
                         read_policies_from_path(os.path.join(GOLD, "yaml", "features"))),
}
CONFIGS = {"all-available": new_all_available(), "tcp-80": new_probe_config(80, "TCP"),
           "named-udp": new_probe_config("serve-81-tcp", "UDP")}
_tables = {}


def _table(policies, config, upper=False, res=None):
    key = (policies, config, upper)
    if res is not None or key not in _tables:
        doc = res if res is not None else _resources(upper)
        cfg = CONFIGS[config]
        cells = PlaneCells(*Oracle(POLICY_SETS[policies](), doc).probe([cfg.to_json()]))
        t = Table(Resources.from_json(doc), cfg, cells, 0, cells.status.shape[1])
        if res is not None:
            return t
        _tables[key] = t
    return _tables[key]


# ---- comparisontable.go, restated over Items
def _equals_dict(l, r):  # :26-36
    if len(l) != len(r):
        return False
    return all(k in r and r[k].combined == lv.combined for k, lv in l.items())


def _item_results_by_protocol(kube, sim):  # :14-20 (Job.Protocol is the key's protocol, job.go:23-25)
    counts = {True: {}, False: {}}
    for key, kr in kube.job_results.items():
        ok, proto = kr.combined == sim.job_results[key].combined, key.split("/")[0]
        counts[ok][proto] = counts[ok].get(proto, 0) + 1
    return counts


def _items(kube, sim):
    return [(fr, to, kube.get(fr, to), sim.get(fr, to)) for fr, to in kube.keys()]


def _results_by_protocol(kube, sim):  # :69-79
    counts = {True: {}, False: {}}
    for _, _, k, s in _items(kube, sim):
        for ok, pc in _item_results_by_protocol(k, s).items():
            for proto, n in pc.items():
                counts[ok][proto] = counts[ok].get(proto, 0) + n
    return counts


def _value_counts_by_protocol(kube, sim, ignore_loopback):  # :89-107
    counts = {"TCP": {}, "SCTP": {}, "UDP": {}}
    for fr, to, k, s in _items(kube, sim):
        for ok, pc in _item_results_by_protocol(k, s).items():
            c = "ignored" if ignore_loopback and fr == to else "same" if ok else "different"
            for proto, n in pc.items():
                if proto not in counts:
                    raise CyclonusPanic(0, NIL_MAP)
                counts[proto][c] = counts[proto].get(c, 0) + n
    return counts


def _value_counts(kube, sim, ignore_loopback):  # :109-123
    counts = {}
    for fr, to, k, s in _items(kube, sim):
        c = "ignored" if ignore_loopback and fr == to else "same" if _equals_dict(k.job_results, s.job_results) else "different"
        counts[c] = counts.get(c, 0) + 1
    return counts


def _render_success_table(kube, sim):  # :125-134, truthtable.go:101-117
    rows = [[fr] + ["." if _equals_dict(kube.get(fr, to).job_results, sim.get(fr, to).job_results) else "X" for to in kube.items]
            for fr in kube.items]
    return render([""] + kube.items, rows, row_line=False)


def _outcome(f, *a):
    try:
        return f(*a)
    except CyclonusPanic as p:
        return ("panic", p.msg)


@pytest.mark.parametrize("upper", (False, True))
@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_comparison_methods_equal_the_restatement(config, upper):
    kube, sim = _table("simple", config, upper), _table("upstream", config, upper)
    ct = ComparisonTable(kube, sim)
    for loop in (False, True):
        assert ct.value_counts(loop) == _value_counts(kube, sim, loop), loop
        want = _outcome(_value_counts_by_protocol, kube, sim, loop)
        assert _outcome(ct.value_counts_by_protocol, loop) == want, loop
        if config == "all-available":  # config #1 writes its container protocols in lower case
            assert (want == ("panic", NIL_MAP)) == (not upper)
    assert ct.results_by_protocol() == _results_by_protocol(kube, sim)
    assert ct.render_success_table() == _render_success_table(kube, sim)
    assert ct.value_counts(False).get("different", 0) > 0, "the two policy sets must disagree somewhere"
    if config == "all-available" and upper:
        assert len([p for p, c in ct.value_counts_by_protocol(False).items() if c]) == 2  # TCP and UDP jobs


@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_table_against_itself_has_no_different(config):
    t = _table("simple", config, True)
    ct = ComparisonTable(t, _table("simple", config, True))
    P = len(t.items)
    assert ct.value_counts(False) == {"same": P * P}
    assert ct.value_counts(True) == {"same": P * P - P, "ignored": P}
    assert ct.results_by_protocol()[False] == {}
    assert all("different" not in c for c in ct.value_counts_by_protocol(True).values())
    assert "| X " not in ct.render_success_table()  # (the header holds the upper-cased namespace x)
    assert not ct.differs().any()


def test_plane_cells_counts_equal_a_walk_over_items():
    """PlaneCells.counts against Connectivity values counted Item by Item."""
    t = _table("simple", "all-available", True)
    got = t.src.counts()
    want = {n: {} for n in ("ingress", "egress", "combined")}
    jobs = 0
    for fr, to in t.keys():
        for r in t.get(fr, to).job_results.values():
            jobs += 1
            for n in want:
                want[n][getattr(r, n)] = want[n].get(getattr(r, n), 0) + 1
    P, K = len(t.items), len(t.slots)
    assert got["no_job"] == P * P * K - jobs
    for n in want:
        assert {_lib.CONNECTIVITY[c]: int(v) for c, v in enumerate(got[n].sum(axis=0)) if v} == want[n], n
    sub = t.src.counts(1, 2)
    assert (sub["combined"][0] == got["combined"][1]).all()


def test_mismatched_pod_sets_panic_as_the_reference():
    kube = _table("simple", "tcp-80")
    fewer = _resources()
    fewer["Pods"].pop()
    with pytest.raises(CyclonusPanic) as e:
        ComparisonTable(kube, _table("upstream", "tcp-80", res=fewer))
    assert e.value.msg == "cannot compare tables of different dimensions"
    renamed = _resources()
    renamed["Pods"][4]["Name"] = "bb"  # y/b -> y/bb: sorted index 4 of both
    with pytest.raises(CyclonusPanic) as e:
        ComparisonTable(kube, _table("upstream", "tcp-80", res=renamed))
    assert e.value.msg == "cannot compare: from keys at index 4 do not match (y/bb vs y/b)"


def test_short_strings():
    assert [short_string(c) for c in ("same", "different", "ignored")] == [".", "X", "?"]
    with pytest.raises(CyclonusPanic):
        short_string("other")


def test_null_arguments_are_refused_without_a_gpu():
    L = _lib.lib()
    out = (ctypes.c_int64 * 6)()
    pairs = (ctypes.c_int64 * 3)()
    assert L.cyc_table_counts(None, 0, 1, out, None, None, None) == _lib.ERR_ARG
    assert L.cyc_table_counts(None, 0, 1, None, None, None, None) == _lib.ERR_ARG
    assert L.cyc_table_compare(None, None, 0, 1, 0, pairs, None, None, None) == _lib.ERR_ARG
    assert L.cyc_table_compare(None, None, 0, 1, 0, None, None, None, None) == _lib.ERR_ARG
    assert L.cyc_table_error(None) == b"null table"
