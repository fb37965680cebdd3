"""Counts and comparison per pod-group pair, on the host: probe.PlaneCells.group_counts / group_compare (the
restatement cyc_table_group_counts / cyc_table_group_compare are tested against on the GPU) against a literal
triple loop over cells(), their sums over the group axes against PlaneCells.counts / compare, Table's namespace
summaries on config #1 against a direct tally of Table.get, and the C ABI's argument errors that need no device."""
import ctypes
import json
import os

import numpy as np
import pytest

from cyclonus_amd import _lib
from cyclonus_amd.comparison import COMPARISONS, ComparisonTable
from cyclonus_amd.probe import ALLOWED, PlaneCells, Resources, Table, new_all_available
from cyclonus_amd.tablewriter import render
from oracle.oracle import Oracle

GOLD = os.path.join(os.path.dirname(__file__), "golden")
VIEWS = ("ingress", "egress", "combined")
PODS = (5, 70)
K = 2


def _random_cells(P, K, seed):
    """Planes with about half the bits set (those beyond P too) and all four statuses."""
    rng = np.random.default_rng(seed)
    W = (P + 63) // 64
    st = rng.integers(0, 4, (P, K)).astype(np.uint8)
    st.reshape(-1)[:4] = [0, 1, 2, 3]
    words = lambda: rng.integers(0, 2**64, (P, K, W), dtype=np.uint64)  # noqa: E731
    return PlaneCells(st, words(), words())


def _loop_group_counts(cells, g, G, k_lo, k_hi):
    P = cells.status.shape[0]
    c = cells.cells(0, P, 0, P, k_lo, k_hi)
    out = {n: np.zeros((G, G, k_hi - k_lo, 6), np.int64) for n in VIEWS}
    out["no_job"] = np.zeros((G, G), np.int64)
    for s in range(P):
        for d in range(P):
            if g[s] < 0 or g[d] < 0:
                continue
            for k in range(k_hi - k_lo):
                for n in VIEWS:
                    code = int(c[n][s, d, k])
                    if code != _lib.CONN_NO_JOB:
                        out[n][g[s], g[d], k, code] += 1
                if int(c["combined"][s, d, k]) == _lib.CONN_NO_JOB:
                    out["no_job"][g[s], g[d]] += 1
    return out


def _loop_group_compare(a, b, g, G, k_lo, k_hi, loop):
    P = a.status.shape[0]
    ca = a.cells(0, P, 0, P, k_lo, k_hi, want=("combined",))["combined"]
    cb = b.cells(0, P, 0, P, k_lo, k_hi, want=("combined",))["combined"]
    pairs, slots = np.zeros((G, G, 3), np.int64), np.zeros((G, G, k_hi - k_lo, 3), np.int64)
    for s in range(P):
        for d in range(P):
            if g[s] < 0 or g[d] < 0:
                continue
            differs = False
            for k in range(k_hi - k_lo):
                x, y = int(ca[s, d, k]), int(cb[s, d, k])
                differs |= x != y
                if x != _lib.CONN_NO_JOB:
                    slots[g[s], g[d], k, 2 if loop and s == d else 0 if x == y else 1] += 1
            pairs[g[s], g[d], 2 if loop and s == d else 1 if differs else 0] += 1
    return {"pairs": pairs, "slots": slots}


@pytest.mark.parametrize("P", PODS)
def test_plane_cells_group_results_equal_a_triple_loop(P):
    a, b = _random_cells(P, K, 40 + P), _random_cells(P, K, 50 + P)
    g = np.random.default_rng(P).integers(-1, 4, P)
    g[:5] = [-1, 0, 1, 2, 3]
    G = 6  # groups 4 and 5 are empty
    for k_lo, k_hi in ((0, K), (1, 2), (1, 1)):
        want = _loop_group_counts(a, g, G, k_lo, k_hi)
        got = a.group_counts(g, G, k_lo, k_hi)
        for n in want:
            assert np.array_equal(got[n], want[n]), (n, k_lo, k_hi)
        assert not got["combined"][4:].any() and not got["combined"][:, 4:].any() and want["combined"].any() == (k_hi > k_lo)
        for loop in (False, True):
            want = _loop_group_compare(a, b, g, G, k_lo, k_hi, loop)
            got = a.group_compare(b, g, G, k_lo, k_hi, loop)
            for n in want:
                assert np.array_equal(got[n], want[n]), (n, k_lo, k_hi, loop)
    assert list(a.group_counts(g, G, want=("egress",))) == ["egress"]
    assert a.group_counts(np.maximum(g, 0))["combined"].shape == (4, 4, K, 6)  # n_groups defaults to max + 1
    for call, msg in ((lambda: a.group_counts(g, 0), "n_groups must be at least 1"),
                      (lambda: a.group_counts(g, 3), "group_of[4] = 3 is neither -1 nor a group in [0, 3)"),
                      (lambda: a.group_compare(b, np.where(np.arange(P) == 2, -2, g), G), "group_of[2] = -2 is neither -1 nor a group in [0, 6)")):
        with pytest.raises(_lib.CyclonusError) as e:
            call()
        assert e.value.code == _lib.ERR_ARG and e.value.msg == msg


@pytest.mark.parametrize("P", PODS)
def test_group_results_sum_to_the_whole_table(P):
    a, b = _random_cells(P, K, 60 + P), _random_cells(P, K, 70 + P)
    g = np.random.default_rng(P + 1).integers(0, 4, P)
    whole, got = a.counts(), a.group_counts(g, 6)
    for n in VIEWS:
        assert np.array_equal(got[n].sum(axis=(0, 1)), whole[n]), n
    assert int(got["no_job"].sum()) == whole["no_job"]
    for loop in (False, True):
        whole, got = a.compare(b, ignore_loopback=loop), a.group_compare(b, g, 6, ignore_loopback=loop)
        assert np.array_equal(got["pairs"].sum(axis=(0, 1)), whole["pairs"]) and np.array_equal(got["slots"].sum(axis=(0, 1)), whole["slots"])
        ignored = got["pairs"][:, :, 2]
        assert np.array_equal(ignored, np.diag(np.bincount(g, minlength=6)) * loop)  # ignored pairs land in (g, g)


def test_config1_namespace_summaries_equal_a_tally_of_the_items():
    """Config #1 over the oracle's planes, every port of every pod: namespace_counts, render_namespace_table and the
    comparison's namespace summaries against a walk over Table.get."""
    c = json.load(open(os.path.join(GOLD, "config1.json")))
    res, cfg = Resources.from_json(c["resources"]), new_all_available()
    planes = {n: Oracle(pols, c["resources"]).probe([cfg.to_json()]) for n, pols in (("all", c["policies"]), ("some", c["policies"][:3]))}
    table = Table(res, cfg, PlaneCells(*planes["all"]), 0, planes["all"][0].shape[1])
    other = Table(res, cfg, PlaneCells(*planes["some"]), 0, planes["some"][0].shape[1])
    ns_of = {p.pod_string(): p.namespace for p in res.pods}
    names = sorted(set(ns_of.values()))
    assert len(names) > 1
    for view in VIEWS:
        want = {(a, b): {} for a in names for b in names}
        for fr, to in table.keys():
            for r in table.get(fr, to).job_results.values():
                cell = want[ns_of[fr], ns_of[to]]
                cell[getattr(r, view)] = cell.get(getattr(r, view), 0) + 1
        got = table.namespace_counts(view)
        assert got == want and any(ALLOWED in v for v in got.values())
        rows = [[a] + [f"{want[a, b].get(ALLOWED, 0)}/{sum(want[a, b].values())}" for b in names] for a in names]
        assert table.render_namespace_table(view) == render([""] + names, rows, row_line=False)
    assert table.render_namespace_table() == table.render_namespace_table("combined")
    with pytest.raises(ValueError):
        table.namespace_counts("open")
    ct = ComparisonTable(table, other)
    for loop in (False, True):
        pairs, jobs = ({(a, b): {} for a in names for b in names} for _ in range(2))
        for fr, to in table.keys():
            k, s = table.get(fr, to).job_results, other.get(fr, to).job_results
            at = (ns_of[fr], ns_of[to])
            ignored = loop and fr == to
            for key, kr in k.items():
                x = COMPARISONS[2 if ignored else 0 if key in s and s[key].combined == kr.combined else 1]
                jobs[at][x] = jobs[at].get(x, 0) + 1
            same = set(k) == set(s) and all(s[key].combined == kr.combined for key, kr in k.items())
            x = COMPARISONS[2 if ignored else 0 if same else 1]
            pairs[at][x] = pairs[at].get(x, 0) + 1
        assert ct.value_counts_by_namespace(loop) == pairs and ct.job_counts_by_namespace(loop) == jobs
        assert any("different" in v for v in jobs.values())
        total = {}
        for v in pairs.values():
            for x, n in v.items():
                total[x] = total.get(x, 0) + n
        assert total == ct.value_counts(loop)
    assert ct.value_counts_by_namespace() == ct.value_counts_by_namespace(False)


def test_arguments_are_refused_without_a_gpu():
    L = _lib.lib()
    g = np.zeros(4, np.int32)
    out = np.full(4 * 6, -7, np.int64)
    assert L.cyc_table_group_counts(None, g.ctypes.data, 1, 0, 1, out.ctypes.data, out.ctypes.data, out.ctypes.data, out.ctypes.data) == _lib.ERR_ARG
    assert L.cyc_table_group_counts(None, None, 1, 0, 1, None, None, None, None) == _lib.ERR_ARG
    assert L.cyc_table_group_compare(None, None, g.ctypes.data, 1, 0, 1, 0, out.ctypes.data, out.ctypes.data) == _lib.ERR_ARG
    assert L.cyc_table_group_compare(None, None, None, 1, 0, 1, 1, None, None) == _lib.ERR_ARG
    assert (out == -7).all()
    assert ctypes.sizeof(ctypes.c_int32) == g.itemsize
