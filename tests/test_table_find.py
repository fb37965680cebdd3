"""The listings behind the counts, on the host: probe.PlaneCells.find / compare_find (the restatement that
cyc_table_find / cyc_table_compare_find are tested against on the GPU) against a literal triple loop over cells(),
their paging contract, Table.find on config #1's README table, ComparisonTable.different_jobs against a walk over
the Items (comparisontable.go:14-36), and the C ABI's argument errors that need no device."""
import copy
import ctypes
import json
import os

import numpy as np
import pytest

from cyclonus_amd import _lib
from cyclonus_amd._lib import CyclonusError
from cyclonus_amd.comparison import ComparisonTable
from cyclonus_amd.loader import read_policies_from_path
from cyclonus_amd.probe import ALLOWED, BLOCKED, PlaneCells, Resources, Table, new_all_available, new_probe_config
from oracle.oracle import Oracle

GOLD = os.path.join(os.path.dirname(__file__), "golden")
VIEWS = ("ingress", "egress", "combined")


def _random_cells(P, K, seed):
    """Planes with about half the bits set (those beyond P too) and all four statuses."""
    rng = np.random.default_rng(seed)
    W = (P + 63) // 64
    st = rng.integers(0, 4, (P, K)).astype(np.uint8)
    st.reshape(-1)[:4] = [0, 1, 2, 3]
    words = lambda: rng.integers(0, 2**64, (P, K, W), dtype=np.uint64)  # noqa: E731
    return PlaneCells(st, words(), words())


def _loop_find(cells, view, codes, k_lo, k_hi):
    """Every matching cell, by a literal loop in (s, d, k) order -> list of record tuples."""
    P = cells.status.shape[0]
    c = cells.cells(0, P, 0, P, k_lo, k_hi)
    out = []
    for s in range(P):
        for d in range(P):
            for k in range(k_hi - k_lo):
                if int(c[view][s, d, k]) in codes:
                    out.append((s, d, k + k_lo, int(c["ingress"][s, d, k]), int(c["egress"][s, d, k]), int(c["combined"][s, d, k]), 0))
    return out


def _loop_compare_find(a, b, k_lo, k_hi, loop):
    P = a.status.shape[0]
    ca, cb = a.cells(0, P, 0, P, k_lo, k_hi), b.cells(0, P, 0, P, k_lo, k_hi)
    out = []
    for s in range(P):
        for d in range(P):
            for k in range(k_hi - k_lo):
                x, y = int(ca["combined"][s, d, k]), int(cb["combined"][s, d, k])
                if x == _lib.CONN_NO_JOB or (loop and s == d) or x == y:
                    continue
                out.append((s, d, k + k_lo, int(ca["ingress"][s, d, k]), int(ca["egress"][s, d, k]), x, y))
    return out


def _tuples(recs):
    return [tuple(int(v) for v in r) for r in recs.tolist()]


def _check_paging(page, want, P):
    """page(s_from, cap) -> (records, s_next, total) against the full list `want` (record tuples in order)."""
    per = np.bincount([r[0] for r in want], minlength=P)
    starts = np.concatenate([[0], np.cumsum(per)])
    recs, s_next, total = page(0, len(want) + 1)
    assert (_tuples(recs), s_next, total) == (want, P, len(want))
    recs, s_next, total = page(0, 0)  # the count-only call
    assert (len(recs), s_next, total) == (0, 0, len(want))
    busy = [s for s in range(P) if per[s]]
    if len(busy) < 2:
        return
    mid = busy[len(busy) // 2]  # a source with matches, not the first one
    # cap = the exact size of the prefix [0, mid]: s_next runs on over the sources without matches behind it
    stop = next((s for s in range(mid + 1, P) if per[s]), P)
    recs, s_next, total = page(0, int(starts[mid + 1]))
    assert (_tuples(recs), s_next, total) == (want[:starts[mid + 1]], stop, len(want))
    # one less: the page ends before source mid
    recs, s_next, total = page(0, int(starts[mid + 1]) - 1)
    assert (_tuples(recs), s_next, total) == (want[:starts[mid]], mid, len(want))
    # continuing from there gives the rest; total counts from s_from on
    recs2, s_next2, total2 = page(mid, len(want))
    assert (_tuples(recs2), s_next2, total2) == (want[starts[mid]:], P, len(want) - int(starts[mid]))
    # cap below the first source's count (a source with two matches at least: cap 0 would be the count-only call)
    big = next(s for s in busy if per[s] >= 2)
    with pytest.raises(CyclonusError) as e:
        page(big, int(per[big]) - 1)
    assert e.value.code == _lib.ERR_ARG and e.value.total == len(want) - int(starts[big])
    assert e.value.msg == f"source {big} alone has {per[big]} matching cells, more than cap {per[big] - 1}"
    recs, s_next, total = page(P, None)
    assert (len(recs), s_next, total) == (0, P, 0)


@pytest.mark.parametrize("P", (5, 64, 70))
def test_plane_cells_find_equals_a_triple_loop(P):
    K = 3
    a = _random_cells(P, K, 10 + P)
    masks = [(c,) for c in range(6)] + [(_lib.CONN_BLOCKED, _lib.CONN_ALLOWED)]
    for view in VIEWS:
        for codes in masks:
            for k_lo, k_hi in ((0, K), (1, 2)):
                want = _loop_find(a, view, codes, k_lo, k_hi)
                recs, s_next, total = a.find(view, codes, k_lo, k_hi, cap=P * P * K)
                assert (_tuples(recs), s_next, total) == (want, P, len(want)), (view, codes, k_lo, k_hi)
    for view, codes in (("combined", (_lib.CONN_ALLOWED,)), ("egress", (_lib.CONN_UNKNOWN,)), ("ingress", (_lib.CONN_BLOCKED,))):
        _check_paging(lambda s, cap: a.find(view, codes, 0, K, s, cap), _loop_find(a, view, codes, 0, K), P)
    recs, s_next, total = a.find("combined", (_lib.CONN_ALLOWED,), 1, 1)
    assert (len(recs), s_next, total) == (0, P, 0)
    assert np.concatenate(list(a.find_all("ingress", (_lib.CONN_ALLOWED,), cap=P * K))).tolist() == \
        a.find("ingress", (_lib.CONN_ALLOWED,), cap=P * P * K)[0].tolist()
    for call, msg in ((lambda: a.find("combined", ()), "code_mask must name codes 0..5"), (lambda: a.find("combined", (6,)), "code_mask must name codes 0..5"),
                      (lambda: a.find(3, (5,)), "unknown view"), (lambda: a.find("combined", (5,), 0, K + 1), "slot range out of bounds"),
                      (lambda: a.find("combined", (5,), s_from=P + 1), "s_from outside the table's rows")):
        with pytest.raises(CyclonusError) as e:
            call()
        assert e.value.code == _lib.ERR_ARG and e.value.msg == msg


@pytest.mark.parametrize("P", (5, 64, 70))
def test_plane_cells_compare_find_equals_a_triple_loop(P):
    K = 3
    a, b = _random_cells(P, K, 20 + P), _random_cells(P, K, 30 + P)
    for loop in (False, True):
        for k_lo, k_hi in ((0, K), (2, 3)):
            want = _loop_compare_find(a, b, k_lo, k_hi, loop)
            recs, s_next, total = a.compare_find(b, k_lo, k_hi, loop, cap=P * P * K)
            assert (_tuples(recs), s_next, total) == (want, P, len(want)), (loop, k_lo, k_hi)
            assert total == int(a.compare(b, k_lo, k_hi, loop)["slots"][:, 1].sum())
        # a sparse difference: slot 0 VALID and open for ingress everywhere, and every third source's egress bits of
        # the first five destinations flipped, so that sources with several matches and sources without any exist
        st = a.status.copy()
        st[:, 0] = _lib.JOB_VALID
        x = PlaneCells(st, a.ingress.copy(), a.egress.copy())
        x.ingress[:, 0, :] = ~np.uint64(0)
        y = PlaneCells(st, x.ingress, x.egress.copy())
        y.egress[1::3, 0, 0] ^= np.uint64(0b11111)
        _check_paging(lambda s, cap: x.compare_find(y, 0, K, loop, s, cap), _loop_compare_find(x, y, 0, K, loop), P)
    assert a.compare_find(a)[2] == 0 and a.compare_find(a)[1] == P


def test_config1_find_is_the_readme_table():
    """Config #1 over the oracle's planes: find(Combined == blocked) lists exactly the X cells of the README table
    fixture (TCP/80, slot 0), find(allowed) exactly the . cells, in plane order."""
    c = json.load(open(os.path.join(GOLD, "config1.json")))
    res = Resources.from_json(c["resources"])
    cells = PlaneCells(*Oracle(c["policies"], c["resources"]).probe(c["probes"]))
    table = Table(res, new_probe_config(80, "TCP"), cells, 0, 1)
    rows = c["readme_combined_tcp80"]["rows"]
    names = [p.pod_string() for p in res.pods]
    for conn, mark in ((BLOCKED, "X"), (ALLOWED, ".")):
        want = [(fr, to) for fr in names for to in names if rows[fr][to.upper()] == mark]
        got = list(table.find(conn))
        assert [(fr, to) for fr, to, _ in got] == want and want
        assert all(r.key == "TCP/80" and r.combined == conn for _, _, r in got)
        for fr, to, r in got:
            assert table.get(fr, to).job_results["TCP/80"] == r
    assert sorted((fr, to) for fr, to, _ in table.find(ALLOWED, "ingress")) == \
        sorted((fr, to) for fr, to in table.keys() if table.get(fr, to).job_results["TCP/80"].ingress == ALLOWED)
    with pytest.raises(ValueError):
        next(table.find("open"))


POLICY_SETS = {
    "simple": lambda: read_policies_from_path(os.path.join(GOLD, "yaml", "simple-example")),
    "upstream": lambda: (read_policies_from_path(os.path.join(GOLD, "yaml", "upstream_test_cases")) +
                         read_policies_from_path(os.path.join(GOLD, "yaml", "features"))),
}


def _walk_different_jobs(kube, sim, ignore_loopback):
    """comparisontable.go:14-36 over the Items, in plane order: every job of the kube Item whose simulated
    Combined differs (a job the simulated Item lacks included), loopback Items left out when they are ignored."""
    names = [p.pod_string() for p in kube.resources.pods]
    out = []
    for fr in names:
        for to in names:
            if ignore_loopback and fr == to:
                continue
            k, s = kube.get(fr, to).job_results, sim.get(fr, to).job_results
            for key, kr in k.items():  # (Table.get builds the dict in slot order)
                sr = s.get(key)
                if sr is None or sr.combined != kr.combined:
                    out.append((fr, to, key, kr.combined, sr.combined if sr is not None else None))
    return out


@pytest.mark.parametrize("config", ("all-available", "tcp-80"))
def test_different_jobs_equal_a_walk_over_the_items(config):
    doc = copy.deepcopy(json.load(open(os.path.join(GOLD, "config1.json")))["resources"])
    cfg = new_all_available() if config == "all-available" else new_probe_config(80, "TCP")
    res = Resources.from_json(doc)
    planes = {n: Oracle(POLICY_SETS[n](), doc).probe([cfg.to_json()]) for n in POLICY_SETS}
    kube = Table(res, cfg, PlaneCells(*planes["simple"]), 0, planes["simple"][0].shape[1])
    st = planes["upstream"][0].copy()
    st[2, 0] = _lib.JOB_NONE  # a job that the simulated table lacks: every source differs there
    sim = Table(res, cfg, PlaneCells(st, *planes["upstream"][1:]), 0, st.shape[1])
    ct = ComparisonTable(kube, sim)
    for loop in (False, True):
        want = _walk_different_jobs(kube, sim, loop)
        assert list(ct.different_jobs(loop)) == want and want
        assert any(x[4] is None for x in want)
        assert len(want) == int(ct._compare(loop)["slots"][:, 1].sum())
        assert list(ct.different_jobs(loop, limit=3)) == want[:3]
    assert list(ComparisonTable(kube, kube).different_jobs(False)) == []


def test_arguments_are_refused_without_a_gpu():
    L = _lib.lib()
    n, s_next, total = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
    refs = (ctypes.byref(n), ctypes.byref(s_next), ctypes.byref(total))
    buf = np.zeros(4, _lib.CELL_DTYPE)
    assert np.dtype(_lib.CELL_DTYPE).itemsize == ctypes.sizeof(_lib.Cell) == 16
    assert (_lib.VIEW_INGRESS, _lib.VIEW_EGRESS, _lib.VIEW_COMBINED) == (0, 1, 2)
    for view, mask in ((_lib.VIEW_COMBINED, 1 << _lib.CONN_ALLOWED), (_lib.VIEW_COMBINED, 0), (_lib.VIEW_COMBINED, 64), (3, 1), (-1, 1)):
        assert L.cyc_table_find(None, view, mask, 0, 1, 0, buf.ctypes.data, 4, *refs) == _lib.ERR_ARG
    for skip in range(3):
        args = [None if i == skip else r for i, r in enumerate(refs)]
        assert L.cyc_table_find(None, _lib.VIEW_COMBINED, 32, 0, 1, 0, buf.ctypes.data, 4, *args) == _lib.ERR_ARG
        assert L.cyc_table_compare_find(None, None, 0, 1, 0, 0, buf.ctypes.data, 4, *args) == _lib.ERR_ARG
    assert L.cyc_table_compare_find(None, None, 0, 1, 0, 0, buf.ctypes.data, 4, *refs) == _lib.ERR_ARG
    assert not buf.view(np.uint8).any()
