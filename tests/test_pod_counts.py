"""Counts and comparison per pod, on the host: probe.PlaneCells.pod_counts / pod_compare (the restatement
cyc_table_pod_counts / cyc_table_pod_compare are tested against on the GPU) against plain loops over cells(), their
sums over the pods against PlaneCells.counts / compare, Table's and ComparisonTable's pod summaries on config #1
against a direct tally of Table.get, and the C ABI's argument errors that need no device."""
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
K = 3
SLOT_RANGES = ((0, K), (1, 2), (2, 3), (1, 1))


def _random_cells(P, K, seed):
    """Planes with about half the bits set (those beyond P too) and all four statuses."""
    rng = np.random.default_rng(seed)
    W = (P + 63) // 64
    st = rng.integers(0, 4, (P, K)).astype(np.uint8)
    st.reshape(-1)[:4] = [0, 1, 2, 3]
    words = lambda: rng.integers(0, 2**64, (P, K, W), dtype=np.uint64)  # noqa: E731
    return PlaneCells(st, words(), words())


def _loop_pod_counts(cells, view, k_lo, k_hi):
    P = cells.status.shape[0]
    c = cells.cells(0, P, 0, P, k_lo, k_hi, want=(view,))[view]
    src, dst = (np.zeros((P, k_hi - k_lo, 7), np.int64) for _ in range(2))
    for s in range(P):
        for d in range(P):
            for k in range(k_hi - k_lo):
                code = int(c[s, d, k])
                col = 6 if code == _lib.CONN_NO_JOB else code
                src[s, k, col] += 1
                dst[d, k, col] += 1
    return {"src": src, "dst": dst}


def _loop_pod_compare(a, b, k_lo, k_hi, loop):
    P = a.status.shape[0]
    ca = a.cells(0, P, 0, P, k_lo, k_hi, want=("combined",))["combined"]
    cb = b.cells(0, P, 0, P, k_lo, k_hi, want=("combined",))["combined"]
    out = {"src_pairs": np.zeros((P, 3), np.int64), "dst_pairs": np.zeros((P, 3), np.int64),
           "src_slots": np.zeros((P, k_hi - k_lo, 3), np.int64), "dst_slots": np.zeros((P, k_hi - k_lo, 3), np.int64)}
    for s in range(P):
        for d in range(P):
            differs = False
            for k in range(k_hi - k_lo):
                x, y = int(ca[s, d, k]), int(cb[s, d, k])
                differs |= x != y
                if x != _lib.CONN_NO_JOB:
                    col = 2 if loop and s == d else 0 if x == y else 1
                    out["src_slots"][s, k, col] += 1
                    out["dst_slots"][d, k, col] += 1
            col = 2 if loop and s == d else 1 if differs else 0
            out["src_pairs"][s, col] += 1
            out["dst_pairs"][d, col] += 1
    return out


@pytest.mark.parametrize("P", PODS)
def test_plane_cells_pod_results_equal_plain_loops(P):
    a, b = _random_cells(P, K, 40 + P), _random_cells(P, K, 50 + P)
    assert {0, 1, 2, 3} <= set(a.status.reshape(-1).tolist())
    for k_lo, k_hi in SLOT_RANGES:
        for view in VIEWS:
            want, got = _loop_pod_counts(a, view, k_lo, k_hi), a.pod_counts(view, k_lo, k_hi)
            for n in want:
                assert np.array_equal(got[n], want[n]), (n, view, k_lo, k_hi)
            assert (got["src"].sum(axis=2) == P).all() and (got["dst"].sum(axis=2) == P).all()
            assert np.array_equal(a.pod_counts(_lib.VIEWS[view], k_lo, k_hi)["src"], want["src"])  # (a cyc_view too)
        for loop in (False, True):
            want, got = _loop_pod_compare(a, b, k_lo, k_hi, loop), a.pod_compare(b, k_lo, k_hi, loop)
            assert set(got) == set(want)
            for n in want:
                assert np.array_equal(got[n], want[n]), (n, k_lo, k_hi, loop)
    assert list(a.pod_counts("egress", want=("dst",))) == ["dst"]
    with pytest.raises(_lib.CyclonusError) as e:
        a.pod_counts("open")
    assert e.value.code == _lib.ERR_ARG and e.value.msg == "unknown view"
    with pytest.raises(_lib.CyclonusError) as e:
        a.pod_compare(_random_cells(P + 1, K, 1))
    assert e.value.code == _lib.ERR_ARG


@pytest.mark.parametrize("P", PODS)
def test_pod_results_sum_to_the_whole_table(P):
    a, b = _random_cells(P, K, 60 + P), _random_cells(P, K, 70 + P)
    for k_lo, k_hi in SLOT_RANGES:
        whole = a.counts(k_lo, k_hi)
        for view in VIEWS:
            got = a.pod_counts(view, k_lo, k_hi)
            for n in ("src", "dst"):
                assert np.array_equal(got[n][:, :, :6].sum(axis=0), whole[view]), (view, n, k_lo, k_hi)
                assert int(got[n][:, :, 6].sum()) == whole["no_job"], (view, n, k_lo, k_hi)
        for loop in (False, True):
            whole, got = a.compare(b, k_lo, k_hi, loop), a.pod_compare(b, k_lo, k_hi, loop)
            for n in ("src", "dst"):
                assert np.array_equal(got[n + "_pairs"].sum(axis=0), whole["pairs"]), (n, k_lo, k_hi, loop)
                assert np.array_equal(got[n + "_slots"].sum(axis=0), whole["slots"]), (n, k_lo, k_hi, loop)
            assert np.array_equal(got["dst_slots"], whole["dst"])
            assert (got["src_pairs"][:, 2] == int(loop)).all() and (got["dst_pairs"][:, 2] == int(loop)).all()


def test_config1_pod_summaries_equal_a_tally_of_the_items():
    """Config #1 over the oracle's planes, every port of every pod: pod_counts, render_pod_table and the comparison's
    pod summaries against a walk over Table.get for all 81 pairs."""
    c = json.load(open(os.path.join(GOLD, "config1.json")))
    res, cfg = Resources.from_json(c["resources"]), new_all_available()
    planes = {n: Oracle(pols, c["resources"]).probe([cfg.to_json()]) for n, pols in (("all", c["policies"]), ("some", c["policies"][:3]))}
    table = Table(res, cfg, PlaneCells(*planes["all"]), 0, planes["all"][0].shape[1])
    other = Table(res, cfg, PlaneCells(*planes["some"]), 0, planes["some"][0].shape[1])
    assert len(table.keys()) == 81
    for view in VIEWS:
        want = {p: {"as_source": {}, "as_destination": {}} for p in table.items}
        for fr, to in table.keys():
            for r in table.get(fr, to).job_results.values():
                for cell in (want[fr]["as_source"], want[to]["as_destination"]):
                    cell[getattr(r, view)] = cell.get(getattr(r, view), 0) + 1
        got = table.pod_counts(view)
        assert got == want and any(ALLOWED in v["as_source"] for v in got.values())
        cell = lambda t: f"{t.get(ALLOWED, 0)}/{sum(t.values())}"  # noqa: E731
        rows = [[p, cell(want[p]["as_source"]), cell(want[p]["as_destination"])] for p in table.items]
        text = table.render_pod_table(view)
        assert text == render(["", "as source", "as destination"], rows, row_line=False) and text == table.render_pod_table(view)
    assert table.render_pod_table() == table.render_pod_table("combined")
    assert table.items == sorted(table.items)  # (the rows above are in sorted-name order)
    with pytest.raises(ValueError):
        table.pod_counts("open")
    ct = ComparisonTable(table, other)
    for loop in (False, True):
        pairs, jobs = ({p: {"as_source": {}, "as_destination": {}} for p in table.items} for _ in range(2))
        for fr, to in table.keys():
            k, s = table.get(fr, to).job_results, other.get(fr, to).job_results
            ignored = loop and fr == to
            for key, kr in k.items():
                x = COMPARISONS[2 if ignored else 0 if key in s and s[key].combined == kr.combined else 1]
                for cell in (jobs[fr]["as_source"], jobs[to]["as_destination"]):
                    cell[x] = cell.get(x, 0) + 1
            same = set(k) == set(s) and all(s[key].combined == kr.combined for key, kr in k.items())
            x = COMPARISONS[2 if ignored else 0 if same else 1]
            for cell in (pairs[fr]["as_source"], pairs[to]["as_destination"]):
                cell[x] = cell.get(x, 0) + 1
        assert ct.value_counts_by_pod(loop) == pairs and ct.job_counts_by_pod(loop) == jobs
        assert any("different" in v["as_source"] for v in jobs.values())
        for side in ("as_source", "as_destination"):
            total = {}
            for v in pairs.values():
                for x, n in v[side].items():
                    total[x] = total.get(x, 0) + n
            assert total == ct.value_counts(loop), (side, loop)
    assert ct.value_counts_by_pod() == ct.value_counts_by_pod(False)


def test_arguments_are_refused_without_a_gpu():
    L = _lib.lib()
    out = np.full(4 * 7, -7, np.int64)
    assert _lib.POD_CODES == 7
    assert L.cyc_table_pod_counts(None, _lib.VIEW_COMBINED, 0, 1, out.ctypes.data, out.ctypes.data) == _lib.ERR_ARG
    assert L.cyc_table_pod_counts(None, 3, 0, 1, None, None) == _lib.ERR_ARG
    assert L.cyc_table_pod_compare(None, None, 0, 1, 0, out.ctypes.data, out.ctypes.data, out.ctypes.data, out.ctypes.data) == _lib.ERR_ARG
    assert L.cyc_table_pod_compare(None, None, 0, 1, 1, None, None, None, None) == _lib.ERR_ARG
    assert (out == -7).all()
