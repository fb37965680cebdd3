"""cyc_table_pod_counts / cyc_table_pod_compare: counts and comparison per source pod and per destination pod on
the device (the SRC instantiations of k_table_tiles, csrc/dev_table.hpp), bit-exact against probe.PlaneCells'
per-cell numpy restatement.

Kernel geometry on wrapped random planes (set bits beyond P, both plane alignments, all four statuses): pod counts
around the 64-pod word and around the block tile of 16 words (at 1024 / 1025 two blocks add to one source's
counter), 1 and 3 slots with sub-ranges, all three views, both loopback settings; host outputs lie between sentinel
elements.  Then source shards, a directed orientation test that does not use PlaneCells, the engine's tables
against the oracle's planes, and arguments and lifetime."""
import json
import os

import numpy as np
import pytest

from cyclonus_amd import _lib
from cyclonus_amd._lib import CyclonusError
from cyclonus_amd.engine import Engine
from cyclonus_amd.probe import PlaneCells
from cyclonus_amd.shard import source_range
from oracle.oracle import Oracle, OraclePanic
from randgen import random_problem
from test_gpu_group_counts import SENTINEL, _Out, _check, _same
from test_gpu_table_counts import SLOT_RANGES, _bare_engine, _Planes

GOLD = os.path.join(os.path.dirname(__file__), "golden")
pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("gpu")]
VIEWS = ("ingress", "egress", "combined")
CMP_OUT = ("src_pairs", "dst_pairs", "src_slots", "dst_slots")
PARTIAL = "ingress cells need destinations inside the table's rows"


def _pod_counts(t, view, k_lo, k_hi, ctx):
    """cyc_table_pod_counts with both outputs between sentinels -> the dict DeviceTable.pod_counts returns."""
    nk = k_hi - k_lo
    out = {"src": _Out((t.row_hi - t.row_lo, nk, 7)), "dst": _Out((t.pods, nk, 7))}
    _check(t, _lib.lib().cyc_table_pod_counts(t._t, _lib.VIEWS[view], k_lo, k_hi, out["src"].ptr, out["dst"].ptr))
    return {n: o.take(ctx) for n, o in out.items()}


def _pod_compare(ta, tb, k_lo, k_hi, loop, ctx):
    nk, rows = k_hi - k_lo, ta.row_hi - ta.row_lo
    out = {"src_pairs": _Out((rows, 3)), "dst_pairs": _Out((ta.pods, 3)), "src_slots": _Out((rows, nk, 3)), "dst_slots": _Out((ta.pods, nk, 3))}
    _check(ta, _lib.lib().cyc_table_pod_compare(ta._t, tb._t, k_lo, k_hi, int(loop), *(out[n].ptr for n in CMP_OUT)))
    return {n: o.take(ctx) for n, o in out.items()}


@pytest.mark.parametrize("K", (1, 3))
@pytest.mark.parametrize("P", (1, 63, 64, 65, 129, 1023, 1024, 1025))
def test_random_planes_equal_the_cell_restatement(P, K):
    """Both entry points over every slot range of K, both plane alignments, the three views and both loopback
    settings against the cell restatement (computed once: the planes' contents do not depend on the alignment; a
    sub-range's counts are slots of the whole range's), and their sums over the pods against counts / compare."""
    eng = _bare_engine(P, K)
    want_c = {}
    want_p = {}
    for off in (0, 1):
        a, b = _Planes(P, K, 900 + P, off), _Planes(P, K, 1000 + P, off)
        assert {0, 1, 2, 3} <= set(a.h_st.reshape(-1).tolist()) or P * K < 16
        ta, tb = a.table(eng), b.table(eng)
        for k_lo, k_hi in SLOT_RANGES[K]:
            whole = ta.counts(k_lo, k_hi)
            for view in VIEWS:
                ctx = f"P {P} K {K} {view} slots [{k_lo}, {k_hi}) plane offset {off}"
                if view not in want_c:
                    want_c[view] = a.cells.pod_counts(view)
                got = _pod_counts(ta, view, k_lo, k_hi, ctx)
                _same(got, {n: w[:, k_lo:k_hi] for n, w in want_c[view].items()}, ctx)
                for n in ("src", "dst"):
                    assert np.array_equal(got[n][:, :, :6].sum(axis=0), whole[view]), f"{ctx}: {n} does not sum to counts"
                    assert int(got[n][:, :, 6].sum()) == whole["no_job"], f"{ctx}: {n} column 6 does not sum to no_job"
            for loop in (False, True):
                ctx = f"P {P} K {K} slots [{k_lo}, {k_hi}) plane offset {off} loopback {loop}"
                if (k_lo, k_hi, loop) not in want_p:
                    want_p[k_lo, k_hi, loop] = a.cells.pod_compare(b.cells, k_lo, k_hi, loop)
                got = _pod_compare(ta, tb, k_lo, k_hi, loop, ctx)
                _same(got, want_p[k_lo, k_hi, loop], ctx)
                whole_p = ta.compare(tb, k_lo, k_hi, loop)
                for n in ("src", "dst"):
                    assert np.array_equal(got[n + "_pairs"].sum(axis=0), whole_p["pairs"]), f"{ctx}: {n}_pairs do not sum to compare"
                    assert np.array_equal(got[n + "_slots"].sum(axis=0), whole_p["slots"]), f"{ctx}: {n}_slots do not sum to compare"
                assert np.array_equal(got["dst_slots"], whole_p["dst"]), f"{ctx}: dst_slots is not compare's dst"
    # the Python mirror returns the same arrays; one output alone
    _same(ta.pod_counts("combined"), want_c["combined"], f"P {P} DeviceTable.pod_counts")
    _same(ta.pod_counts(_lib.VIEW_EGRESS, want=("dst",)), {"dst": want_c["egress"]["dst"]}, f"P {P} DeviceTable.pod_counts, dst alone")
    _same(ta.pod_counts("ingress", want=("src",)), {"src": want_c["ingress"]["src"]}, f"P {P} DeviceTable.pod_counts, src alone")
    _same(ta.pod_compare(tb, ignore_loopback=True), want_p[0, K, True], f"P {P} DeviceTable.pod_compare")


@pytest.mark.parametrize("P", (129, 1025))
def test_source_shards(P):
    """Two ranks of a source partition: by_dst / dst_* add up to the whole table's, by_src / src_* are its rows."""
    K = 3
    eng = _bare_engine(P, K)
    a, b = _Planes(P, K, 1100 + P, 1), _Planes(P, K, 1200 + P, 1)
    ta, tb = a.table(eng), b.table(eng)
    whole_c = {view: ta.pod_counts(view) for view in VIEWS}
    whole_p = {loop: ta.pod_compare(tb, ignore_loopback=loop) for loop in (False, True)}
    _same(whole_c["combined"], a.cells.pod_counts("combined"), f"P {P}")
    parts_c, parts_p = {view: [] for view in VIEWS}, {False: [], True: []}
    for rank in range(2):
        lo, hi = source_range(P, 2, rank)
        sa, tsa = a.source_shard(eng, lo, hi)
        sb, tsb = b.source_shard(eng, lo, hi)
        assert (tsa.window[0] > 0) == (rank == 1)  # the second rank's ingress window starts past word 0
        for view in VIEWS:
            parts_c[view].append(_pod_counts(tsa, view, 0, K, f"P {P} {view} shard {rank}"))
        for loop in (False, True):
            parts_p[loop].append(_pod_compare(tsa, tsb, 0, K, loop, f"P {P} shard {rank} loopback {loop}"))
    for view in VIEWS:
        got = {"src": np.concatenate([p["src"] for p in parts_c[view]]), "dst": sum(p["dst"] for p in parts_c[view])}
        _same(got, whole_c[view], f"P {P} {view} source shards")
    for loop in (False, True):
        got = {n: np.concatenate([p[n] for p in parts_p[loop]]) if n.startswith("src") else sum(p[n] for p in parts_p[loop]) for n in CMP_OUT}
        _same(got, whole_p[loop], f"P {P} source shards, loopback {loop}")


def test_orientation():
    """Ingress bit (d, s) set iff s < d, egress all ones, every slot VALID: source s reaches the P - 1 - s pods
    after it, destination d is reached from the d pods before it; and the mirrored planes (egress bit (s, d) set iff
    s < d, ingress all ones) for the Egress view.  A swapped role would pass a mirrored restatement: this does not
    use PlaneCells."""
    import torch

    P, K, W = 130, 2, 3
    i = np.arange(P)
    below = np.zeros((P, K, W), np.uint64)  # row r: the bits of the pods before r
    above = np.zeros((P, K, W), np.uint64)  # row r: the bits of the pods after r (and none at or beyond P)
    for r in range(P):
        for p in range(P):
            (below if p < r else above)[r, :, p // 64] |= np.uint64(p != r) << np.uint64(p % 64)
    ones = torch.full((P, K, W), -1, dtype=torch.int64)
    zeros = torch.zeros((P, K, W), dtype=torch.int64)
    valid = torch.full((P, K), _lib.JOB_VALID, dtype=torch.uint8)
    planes = lambda ing, eg: _Planes(P, K, 0, 0, valid, ing, eg)  # noqa: E731
    by_ingress = planes(torch.from_numpy(below.view(np.int64)), ones)  # ingress[d] holds the sources s < d
    by_egress = planes(ones, torch.from_numpy(above.view(np.int64)))   # egress[s] holds the destinations d > s
    nothing = planes(zeros, zeros)
    eng = _bare_engine(P, K)
    for a, views in ((by_ingress, ("ingress", "combined")), (by_egress, ("egress", "combined"))):
        t = a.table(eng)
        for view in views:
            got = _pod_counts(t, view, 0, K, view)
            for k in range(K):
                assert np.array_equal(got["src"][:, k, _lib.CONN_ALLOWED], P - 1 - i), (view, "src")
                assert np.array_equal(got["dst"][:, k, _lib.CONN_ALLOWED], i), (view, "dst")
                assert np.array_equal(got["src"][:, k, _lib.CONN_BLOCKED], i + 1) and np.array_equal(got["dst"][:, k, _lib.CONN_BLOCKED], P - i)
            assert not got["src"][:, :, [0, 1, 2, 3, 6]].any() and not got["dst"][:, :, [0, 1, 2, 3, 6]].any()
        # against a table that allows nothing, the different jobs are the allowed cells: K per differing pair
        cmp_ = _pod_compare(t, nothing.table(eng), 0, K, False, "compare")
        assert np.array_equal(cmp_["src_pairs"][:, 1], P - 1 - i) and np.array_equal(cmp_["dst_pairs"][:, 1], i)
        assert np.array_equal(cmp_["src_pairs"][:, 0], i + 1) and np.array_equal(cmp_["dst_pairs"][:, 0], P - i)
        for k in range(K):
            assert np.array_equal(cmp_["src_slots"][:, k, 1], P - 1 - i) and np.array_equal(cmp_["dst_slots"][:, k, 1], i)
        assert not cmp_["src_pairs"][:, 2].any() and not cmp_["src_slots"][:, :, 2].any()


def _oracle_cells(pols, res, probes):
    try:
        return PlaneCells(*Oracle(pols, res).probe(probes))
    except OraclePanic:
        return None


def test_engine_tables_equal_the_oracle():
    """Config #1 and random problems (AllAvailable and named-port probes: NO_JOB and both invalid kinds occur): the
    engine's tables against the oracle's planes."""
    c = json.load(open(os.path.join(GOLD, "config1.json")))
    cases = [(c["policies"], c["policies"][:3], c["resources"], c["probes"])]
    for seed in range(8000, 8040):
        pols, res, probes = random_problem(seed)
        cases.append((pols, random_problem(seed + 500)[0], res, probes))
    need = {_lib.CONN_INVALID_NAMED_PORT, _lib.CONN_INVALID_PORT_PROTOCOL, _lib.CONN_BLOCKED, _lib.CONN_ALLOWED, 6}
    n, codes = 0, set()
    e1, e2 = Engine(0), Engine(0)
    for i, (pols_a, pols_b, res, probes) in enumerate(cases):
        wa, wb = _oracle_cells(pols_a, res, probes), _oracle_cells(pols_b, res, probes)
        if wa is None or wb is None:
            continue
        e1.build_policies(pols_a).load_resources(res)
        e2.build_policies(pols_b).load_resources(res)
        e1.prepare(probes), e2.prepare(probes)
        ta, tb = e1.table(), e2.table()
        for view in VIEWS:
            want = wa.pod_counts(view)
            _same(ta.pod_counts(view), want, f"case {i} {view}")
            codes |= {x for x in range(7) if want["src"][:, :, x].sum()}
        for loop in (False, True):
            _same(ta.pod_compare(tb, ignore_loopback=loop), wa.pod_compare(wb, ignore_loopback=loop), f"case {i} loopback {loop}")
        n += 1
        if n >= 6 and need <= codes:
            break
    assert n >= 6 and need <= codes, (n, codes)


def test_arguments_and_lifetime():
    P, K = 150, 2
    eng = _bare_engine(P, K)
    a, b = _Planes(P, K, 1300), _Planes(P, K, 1301)
    ta, tb = a.table(eng), b.table(eng)
    want_c, want_p = a.cells.pod_counts("combined"), a.cells.pod_compare(b.cells, ignore_loopback=True)
    part = eng.wrap_table(a.d_in.data_ptr(), a.d_eg.data_ptr(), a.d_st.data_ptr(), 0, 64)
    src = eng.wrap_table(a.d_in.data_ptr(), a.d_eg.data_ptr(), a.d_st.data_ptr(), 0, P, "source")
    for call, msg in (
            (lambda: ta.pod_counts("combined", want=()), "no output requested"),
            (lambda: ta.pod_counts(3), "unknown view"),
            (lambda: ta.pod_counts(-1), "unknown view"),
            (lambda: ta.pod_counts("combined", 0, K + 1), "slot range out of bounds"),
            (lambda: ta.pod_counts("ingress", 1, 0), "slot range out of bounds"),
            (lambda: ta.pod_compare(tb, -1, K), "slot range out of bounds"),
            (lambda: part.pod_counts("egress"), PARTIAL),
            (lambda: part.pod_compare(part), PARTIAL),
            (lambda: ta.pod_compare(src), "cannot compare tables of different devices, shapes, partitions or rows")):
        with pytest.raises(CyclonusError) as e:
            call()
        assert e.value.code == _lib.ERR_ARG and e.value.msg == msg
    L = _lib.lib()
    out = _Out((P, K, 7))
    assert L.cyc_table_pod_counts(ta._t, _lib.VIEW_COMBINED, 0, K, None, None) == _lib.ERR_ARG
    assert L.cyc_table_pod_counts(ta._t, 3, 0, K, out.ptr, None) == _lib.ERR_ARG
    assert L.cyc_table_pod_compare(ta._t, tb._t, 0, K, 0, None, None, None, None) == _lib.ERR_ARG
    assert L.cyc_table_pod_compare(ta._t, None, 0, K, 0, out.ptr, None, None, None) == _lib.ERR_ARG
    assert (out.buf == SENTINEL).all()
    # an empty slot range writes nothing; a source table answers alike
    empty = _pod_counts(ta, "combined", 1, 1, "empty slot range")
    assert empty["src"].shape == (P, 0, 7) and empty["dst"].shape == (P, 0, 7)
    empty = _pod_compare(ta, tb, 1, 1, True, "empty slot range")
    assert empty["src_slots"].shape == (P, 0, 3) and (empty["src_pairs"] == [P - 1, 0, 1]).all() and (empty["dst_pairs"] == [P - 1, 0, 1]).all()
    _same(src.pod_counts("combined"), want_c, "whole source table")
    eng.close()
    _same(ta.pod_counts("combined"), want_c, "after ctx destroy")
    _same(ta.pod_compare(tb, ignore_loopback=True), want_p, "after ctx destroy")
