"""cyc_table_classes / cyc_table_classes_masked / cyc_table_cells_at: the connectivity classes of a device table
(csrc/dev_classes.hpp) against probe.PlaneCells' restatement (the pods grouped by the bytes of their code rows and
columns), every comparison exact.

The view planes and the row kernels on wrapped random planes (independent of the engine): pod counts around the 64-pod
word and the 16-word block tile, 1 and 3 slots with sub-ranges, both plane alignments, all three views, set plane bits
beyond P, all four statuses.  Generated problems with real classes and every decoy planted (classgen), up to both sides
of one pass of the row kernels over a row (a wave with 16-byte loads takes 128 words: 8192 and 8193 pods), with the
defining property checked through cells_at and cyc_table_cells alone.  The hash masks ~0, 0xF and 0, which drive the
refinement rounds.  Host outputs between sentinels, each output alone, twice for identical bytes.  cells_at against
cyc_table_cells.  Then the engine's own tables against the oracle's planes, a source-row table over all rows, and
arguments and lifetime."""
import ctypes
import json
import os

import numpy as np
import pytest

from classgen import VIEWS, ClassProblem
from cyclonus_amd import _lib
from cyclonus_amd._lib import CyclonusError
from cyclonus_amd.engine import Engine
from cyclonus_amd.probe import PlaneCells, Resources, Table, new_all_available
from oracle.oracle import Oracle, OraclePanic
from randgen import random_problem
from test_gpu_reach import FILL, _Host
from test_gpu_table_counts import SLOT_RANGES, _bare_engine, _Planes

GOLD = os.path.join(os.path.dirname(__file__), "golden")
pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("gpu")]
FILL.setdefault(np.dtype(np.uint8), 0x5A)
FULL = (1 << 64) - 1
OUTPUTS = ("src", "dst", "n_src", "n_dst")
CELL_NAMES = ("ingress", "egress", "combined")


def _err(t):
    return _lib.lib().cyc_table_error(t._t).decode(errors="replace")


def _classes(t, view, k_lo=0, k_hi=None, want=OUTPUTS, mask=None, stats=False, ctx=""):
    """cyc_table_classes (mask None and no stats) or cyc_table_classes_masked with every requested output between
    sentinels -> {"src": i32 [P], "dst": ..., "n_src": int, "n_dst": int, "stats": i64 [4]}."""
    L = _lib.lib()
    k_hi = t.slots if k_hi is None else k_hi
    shape = {"src": ((t.pods,), np.int32), "dst": ((t.pods,), np.int32), "n_src": ((1,), np.int64), "n_dst": ((1,), np.int64)}
    out = {x: _Host(*shape[x]) for x in want}
    ptr = [out[x].ptr if x in out else None for x in OUTPUTS]
    v = _lib.VIEWS.get(view, view)
    if mask is None and not stats:
        rc = L.cyc_table_classes(t._t, v, k_lo, k_hi, *ptr)
    else:
        st = _Host((4,), np.int64)
        rc = L.cyc_table_classes_masked(t._t, v, k_lo, k_hi, *ptr, FULL if mask is None else mask, st.ptr if stats else None)
    if rc != _lib.OK:
        raise CyclonusError(rc, _err(t))
    got = {x: o.take(ctx) for x, o in out.items()}
    for x in ("n_src", "n_dst"):
        if x in got:
            got[x] = int(got[x][0])
    if stats:
        got["stats"] = st.take(ctx)
    return got


def _same(got, want, ctx):
    for x in got:
        if x == "stats":
            continue
        if x.startswith("n_"):
            assert got[x] == want[x], f"{ctx}: {x} {got[x]} want {want[x]}"
        else:
            bad = np.argwhere(got[x] != want[x])
            assert got[x].dtype == np.int32 and bad.size == 0, f"{ctx}: {x} differs at pods {bad[:5, 0].tolist()}: {got[x][bad[:5, 0]]} want {want[x][bad[:5, 0]]}"


# ---------------------------------------------------------------- 1. random wrapped planes
@pytest.mark.parametrize("K", (1, 3))
@pytest.mark.parametrize("P", (1, 63, 64, 65, 129, 1023, 1024, 1025))
def test_random_planes_equal_the_restatement(P, K):
    eng = _bare_engine(P, K)
    want = {}
    for off in (0, 1):
        a = _Planes(P, K, 900 + P, off)
        assert {0, 1, 2, 3} <= set(a.h_st.reshape(-1).tolist()) or P * K < 16
        t = a.table(eng)
        for k_lo, k_hi in SLOT_RANGES[K]:
            for view in VIEWS:
                ctx = f"P {P} K {K} slots [{k_lo}, {k_hi}) {view} plane offset {off}"
                if (k_lo, k_hi, view) not in want:  # (the planes' contents do not depend on the offset)
                    want[k_lo, k_hi, view] = a.cells.classes(view, k_lo, k_hi)
                _same(_classes(t, view, k_lo, k_hi, ctx=ctx), want[k_lo, k_hi, view], ctx)
    # the Python mirror
    got = t.classes("ingress", want=("dst",))
    assert set(got) == {"dst", "n_dst"}
    _same(got, want[0, K, "ingress"], f"P {P} DeviceTable.classes")


# ---------------------------------------------------------------- 2. generated problems with real classes
def _wrap(g, off=0):
    st, ing, eg = g.torch()
    return _Planes(g.P, g.K, 0, off, st, ing, eg)


def _property(t, view, k_lo, k_hi, classes, ctx):
    """On the device alone: cells_at(reps, reps)[src_class[s], dst_class[d]] == cyc_table_cells[s, d] for every cell,
    no two representative rows and no two representative columns are equal, and the ids are canonical."""
    src, dst = classes["src"], classes["dst"]
    for side, n in ((src, classes["n_src"]), (dst, classes["n_dst"])):
        first = np.full(n, len(side), np.int64)
        np.minimum.at(first, side, np.arange(len(side)))
        assert side[0] == 0 and (np.diff(first) > 0).all(), f"{ctx}: class ids are not in the order of their smallest pods"
    reps_s, reps_d = np.unique(src, return_index=True)[1], np.unique(dst, return_index=True)[1]
    table = t.cells_at(reps_s, reps_d, k_lo, k_hi, want=(view,))[view]
    cells = t.cells(0, t.pods, 0, t.pods, k_lo, k_hi, want=(view,))[view]
    assert np.array_equal(table[src][:, dst], cells), f"{ctx}: the class table does not give the cells back"
    assert len({table[i].tobytes() for i in range(len(reps_s))}) == len(reps_s), f"{ctx}: two source classes with equal rows"
    assert len({np.ascontiguousarray(table[:, j]).tobytes() for j in range(len(reps_d))}) == len(reps_d), f"{ctx}: two destination classes with equal columns"


PASS_PODS = 128 * 64  # the words of a row a wave of the row kernels takes in one pass, in pods
GENERATED = [(P, 3, view) for P in (65, 130, 1025) for view in VIEWS] + [(P, 1, view) for P in (PASS_PODS, PASS_PODS + 1) for view in ("ingress", "combined")]


@pytest.mark.parametrize("P,K,view", GENERATED)
def test_generated_problems(P, K, view):
    g = ClassProblem(P, K, 3000 + P)
    assert set(g.decoys) == {"a", "b", "c", "e", "e_dst", "f", "fe", "g", "h"} | ({"d"} if P % 64 else set())
    cells = g.cells()
    eng = _bare_engine(P, K)
    pl = _wrap(g, 1 if P == 1025 else 0)  # (a wrapped table does not own its planes)
    t = pl.table(eng)
    for k_lo, k_hi in SLOT_RANGES[K][:2]:
        ctx = f"P {P} K {K} {view} slots [{k_lo}, {k_hi})"
        want = cells.classes(view, k_lo, k_hi)
        got = _classes(t, view, k_lo, k_hi, stats=True, ctx=ctx)
        _same(got, want, ctx)
        assert 2 <= got["n_src"] <= P // 2 and 2 <= got["n_dst"] <= P // 2, ctx
        _property(t, view, k_lo, k_hi, got, ctx)
        if (k_lo, k_hi) == (0, K):
            g.check_decoys(view, got, ctx)
            assert got["stats"].tolist() == [1, 0, 1, 0], f"{ctx}: stats {got['stats'].tolist()}"  # one round, nobody failed


# ---------------------------------------------------------------- 3. the hash masks
@pytest.mark.parametrize("P", (130, 1025))
def test_hash_masks(P):
    K = 3
    g = ClassProblem(P, K, 3000 + P)
    eng = _bare_engine(P, K)
    pl = _wrap(g)
    t = pl.table(eng)
    for view in VIEWS:
        want = g.cells().classes(view)
        for mask in (FULL, 0xF, 0):
            ctx = f"P {P} {view} mask {mask:#x}"
            got = _classes(t, view, mask=mask, stats=True, ctx=ctx)
            _same(got, want, ctx)
            rs, fs, rd, fd = got["stats"].tolist()
            if mask == FULL:
                assert (rs, fs, rd, fd) == (1, 0, 1, 0), ctx
            if mask == 0:
                assert rs > 1 and rd > 1 and fs >= want["n_src"] - 1 and fd >= want["n_dst"] - 1, f"{ctx}: stats {got['stats'].tolist()}"
    # the Python mirror passes the mask and returns the stats
    got = t.classes("combined", hash_mask=0, stats=True)
    _same(got, want, "DeviceTable.classes, mask 0")
    assert got["stats"].dtype == np.int64 and got["stats"][0] > 1


# ---------------------------------------------------------------- 4. output discipline
def test_outputs_alone_twice_and_the_empty_range():
    P, K = 130, 3
    g = ClassProblem(P, K, 3000 + P)
    eng = _bare_engine(P, K)
    pl = _wrap(g, 1)
    t = pl.table(eng)
    want = g.cells().classes("combined", 1, 3)
    got = _classes(t, "combined", 1, 3)
    _same(got, want, "all outputs")
    for alone in (("src",), ("dst",), ("n_src",), ("n_dst",), ("n_src", "n_dst"), ("src", "n_dst")):
        one = _classes(t, "combined", 1, 3, want=alone, ctx=str(alone))
        assert set(one) == set(alone)
        _same(one, want, f"{alone} alone")
    again = _classes(t, "combined", 1, 3)
    assert all(np.asarray(got[x]).tobytes() == np.asarray(again[x]).tobytes() for x in got), "two calls differ"
    masked = _classes(t, "combined", 1, 3, mask=0xF0, stats=True)
    assert all(np.asarray(got[x]).tobytes() == np.asarray(masked[x]).tobytes() for x in got)
    for view in VIEWS:
        empty = _classes(t, view, 2, 2, stats=True)
        assert not empty["src"].any() and not empty["dst"].any() and (empty["n_src"], empty["n_dst"]) == (1, 1)
        assert empty["stats"].tolist() == [0, 0, 0, 0]


# ---------------------------------------------------------------- 5. cells_at
def _cells_at(t, srcs, dsts, k_lo=0, k_hi=None, want=CELL_NAMES, ctx=""):
    k_hi = t.slots if k_hi is None else k_hi
    s, d = np.ascontiguousarray(srcs, np.int32), np.ascontiguousarray(dsts, np.int32)
    out = {n: _Host((len(s), len(d), max(k_hi - k_lo, 0)), np.uint8) for n in want}
    rc = _lib.lib().cyc_table_cells_at(t._t, ctypes.c_void_p(s.ctypes.data), len(s), ctypes.c_void_p(d.ctypes.data), len(d), k_lo, k_hi,
                                       *(out[n].ptr if n in out else None for n in CELL_NAMES))
    if rc != _lib.OK:
        raise CyclonusError(rc, _err(t))
    return {n: o.take(ctx) for n, o in out.items()}


@pytest.mark.parametrize("P", (65, 1025))
def test_cells_at_equals_cells(P):
    K = 3
    eng = _bare_engine(P, K)
    rng = np.random.default_rng(P)
    for off in (0, 1):
        a = _Planes(P, K, 950 + P, off)
        t = a.table(eng)
        whole = t.cells(0, P, 0, P)
        lists = [(rng.permutation(P)[:40], rng.permutation(P)[:33]), ([P - 1, 0, P - 1, P - 1, 5], [64, 64, 0, P - 1]), ([P - 1], [0]),
                 ([], [1, 2]), ([3], []), (np.arange(P), [P - 1])]
        for s, d in lists:
            s, d = np.asarray(s, np.int64), np.asarray(d, np.int64)
            for k_lo, k_hi in SLOT_RANGES[K]:
                ctx = f"P {P} offset {off} {len(s)} x {len(d)} slots [{k_lo}, {k_hi})"
                got = _cells_at(t, s, d, k_lo, k_hi, ctx=ctx)
                for n in CELL_NAMES:
                    assert np.array_equal(got[n], whole[n][s][:, d][:, :, k_lo:k_hi]), f"{ctx}: {n}"
            for n in CELL_NAMES:
                alone = _cells_at(t, s, d, want=(n,), ctx=f"{n} alone")
                assert set(alone) == {n} and np.array_equal(alone[n], whole[n][s][:, d])
        assert np.array_equal(t.cells_at([2, 1], [0, 2], 1, 2, want=("egress",))["egress"], whole["egress"][[2, 1]][:, [0, 2]][:, :, 1:2])
    # a partial target-row table under cyc_table_cells' rules: ingress cells for its destinations, egress for its sources
    if P == 65:
        lo, hi = 10, 50
        p_in, p_eg = a._dev(a.h_in[lo:hi].contiguous()), a._dev(a.h_eg[lo:hi].contiguous())
        part = eng.wrap_table(p_in.data_ptr(), p_eg.data_ptr(), a.d_st.data_ptr(), lo, hi, "target")
        s_in, d_in = [0, 64, 20], [49, 10, 10]
        assert np.array_equal(_cells_at(part, s_in, d_in, want=("ingress",))["ingress"], whole["ingress"][s_in][:, d_in])
        s_eg, d_eg = [49, 10], [0, 64, 30]
        assert np.array_equal(_cells_at(part, s_eg, d_eg, want=("egress",))["egress"], whole["egress"][s_eg][:, d_eg])
        both = _cells_at(part, [10, 49], [49, 11])
        assert all(np.array_equal(both[n], whole[n][[10, 49]][:, [49, 11]]) for n in CELL_NAMES)
        for args, msg in ((dict(srcs=[20], dsts=[50], want=("ingress",)), "ingress cells need destinations inside the table's rows"),
                          (dict(srcs=[9], dsts=[20], want=("egress",)), "egress cells need sources inside the table's rows"),
                          (dict(srcs=[20], dsts=[20, 9], want=("combined",)), "ingress cells need destinations inside the table's rows"),
                          (dict(srcs=[20, 50], dsts=[20], want=("combined",)), "egress cells need sources inside the table's rows")):
            with pytest.raises(CyclonusError) as e:
                _cells_at(part, **args)
            assert e.value.code == _lib.ERR_ARG and e.value.msg == msg
        assert _cells_at(part, [], [50], want=("ingress",))["ingress"].shape == (0, 1, K)  # (no cell: no row rule)
        keep, shard = a.source_shard(eng, 0, 64)
        assert np.array_equal(_cells_at(shard, [63, 0], [64, 1])["combined"], whole["combined"][[63, 0]][:, [64, 1]])
        with pytest.raises(CyclonusError, match="cells of a source-row table need sources inside its rows"):
            _cells_at(shard, [64], [0], want=("ingress",))
        del keep


# ---------------------------------------------------------------- 6. the engine's own tables; refusals; lifetime
def test_engine_tables_equal_the_oracle():
    """Config #1 and random problems (AllAvailable and named-port probes: NO_JOB and both invalid kinds occur): the
    classes of the engine's table == those of the oracle's planes, for every view."""
    c = json.load(open(os.path.join(GOLD, "config1.json")))
    cases = [(c["policies"], c["resources"], c["probes"])] + [random_problem(seed) for seed in range(8000, 8012)]
    eng, n, merged = Engine(0), 0, 0
    for i, (pols, res, probes) in enumerate(cases):
        if n == 11:
            break
        try:
            want = PlaneCells(*Oracle(pols, res).probe(probes))
        except OraclePanic:
            continue
        eng.build_policies(pols).load_resources(res)
        eng.prepare(probes)
        t = eng.table()
        for view in VIEWS:
            w = want.classes(view)
            _same(_classes(t, view, ctx=f"case {i} {view}"), w, f"case {i} {view}")
            merged += w["n_src"] < t.pods or w["n_dst"] < t.pods
        _same(_classes(t, "combined", 0, 1), want.classes("combined", 0, 1), f"case {i} slot 0")
        n += 1
    assert n == 11 and merged >= 3
    # config #1 through the probe mirror: Table.classes and the class table on the device table == on the oracle's planes
    res, cfg = Resources.from_json(c["resources"]), new_all_available()
    eng.build_policies(c["policies"]).load_resources(c["resources"])
    eng.prepare([cfg.to_json()])
    dt = eng.table()
    st, ing, eg = Oracle(c["policies"], c["resources"]).probe([cfg.to_json()])
    on_dev, on_host = Table(res, cfg, dt, 0, dt.slots), Table(res, cfg, PlaneCells(st, ing, eg), 0, st.shape[1])
    for view in VIEWS:
        assert on_dev.classes(view) == on_host.classes(view)
        assert on_dev.render_class_table(view) == on_host.render_class_table(view)


@pytest.mark.parametrize("P", (65, 1025))
def test_source_table_over_all_rows(P):
    K = 3
    g = ClassProblem(P, K, 3100 + P)
    pl = _wrap(g)
    eng = _bare_engine(P, K)
    t = pl.table(eng)
    ts = eng.wrap_table(pl.d_in.data_ptr(), pl.d_eg.data_ptr(), pl.d_st.data_ptr(), 0, P, "source")
    assert ts.partition == "source" and (ts.row_lo, ts.row_hi) == (0, P)
    for view in VIEWS:
        for k_lo, k_hi in SLOT_RANGES[K]:
            _same(_classes(ts, view, k_lo, k_hi), _classes(t, view, k_lo, k_hi), f"source table P {P} {view} [{k_lo}, {k_hi})")
    _same(_classes(ts, "combined"), g.cells().classes("combined"), f"source table P {P}")
    s, d = [P - 1, 0, 3], [0, P - 1]
    assert all(np.array_equal(x, y) for x, y in zip(_cells_at(ts, s, d).values(), _cells_at(t, s, d).values()))


RP, RK = 65, 3
SLOTS = "slot range out of bounds"
BAD_SLOTS = ((-1, 2), (0, RK + 1), (2, 1))
PARTIAL = "ingress cells need destinations inside the table's rows"
I64, I32 = ctypes.c_int64, ctypes.c_int32


def _refused(t, rc, msg):
    assert rc == _lib.ERR_ARG
    assert _err(t) == msg


def test_refusals_and_lifetime():
    L = _lib.lib()
    eng = _bare_engine(RP, RK)
    a = _Planes(RP, RK, 21)
    t = a.table(eng)
    keep, shard = a.source_shard(eng, 64, RP)
    p_in, p_eg = a._dev(a.h_in[10:50].contiguous()), a._dev(a.h_eg[10:50].contiguous())
    partial = eng.wrap_table(p_in.data_ptr(), p_eg.data_ptr(), a.d_st.data_ptr(), 10, 50, "target")
    src, dst = np.full(RP, 77, np.int32), np.full(RP, 77, np.int32)
    n_src, n_dst, stats = I64(77), I64(77), (I64 * 4)(77, 77, 77, 77)
    ps, pd = ctypes.c_void_p(src.ctypes.data), ctypes.c_void_p(dst.ctypes.data)
    outs = (ps, pd, ctypes.byref(n_src), ctypes.byref(n_dst))
    call = lambda tt=t, view=2, k_lo=0, k_hi=RK, out=outs: L.cyc_table_classes(tt._t, view, k_lo, k_hi, *out)  # noqa: E731
    masked = lambda tt=t, view=2, k_lo=0, k_hi=RK, out=outs: L.cyc_table_classes_masked(tt._t, view, k_lo, k_hi, *out, 0xFF, stats)  # noqa: E731
    # ---- cyc_table_classes and its twin
    assert L.cyc_table_classes(None, 2, 0, RK, *outs) == _lib.ERR_ARG and L.cyc_table_classes_masked(None, 2, 0, RK, *outs, 0, None) == _lib.ERR_ARG
    for f in (call, masked):
        for view in (-1, 3):
            _refused(t, f(view=view), "unknown view")
        for k_lo, k_hi in BAD_SLOTS:
            _refused(t, f(k_lo=k_lo, k_hi=k_hi), SLOTS)
        _refused(t, f(out=(None, None, None, None)), "no output requested")
        for other in (partial, shard):
            _refused(other, f(tt=other), PARTIAL)
    assert (src == 77).all() and (dst == 77).all() and (n_src.value, n_dst.value) == (77, 77) and list(stats) == [77] * 4  # (a refused call writes nothing)
    assert call() == _lib.OK, _err(t)
    assert src[0] == 0 and dst[0] == 0 and n_src.value == int(src.max()) + 1 and n_dst.value == int(dst.max()) + 1
    # ---- cyc_table_cells_at
    cells = np.full(4 * 3 * RK, 77, np.uint8)
    pc = ctypes.c_void_p(cells.ctypes.data)
    srcs, dsts = (I32 * 4)(0, 64, 3, 3), (I32 * 3)(64, 0, 1)
    at = lambda tt=t, s=srcs, ns=4, d=dsts, nd=3, k_lo=0, k_hi=RK, out=(None, None, pc): L.cyc_table_cells_at(tt._t, s, ns, d, nd, k_lo, k_hi, *out)  # noqa: E731
    assert L.cyc_table_cells_at(None, srcs, 4, dsts, 3, 0, RK, None, None, pc) == _lib.ERR_ARG
    for k_lo, k_hi in BAD_SLOTS:
        _refused(t, at(k_lo=k_lo, k_hi=k_hi), SLOTS)
    _refused(t, at(ns=-1), "negative count of srcs")
    _refused(t, at(nd=-2), "negative count of dsts")
    _refused(t, at(s=None), "null srcs")
    _refused(t, at(d=None), "null dsts")
    _refused(t, at(s=(I32 * 4)(RP, 64, 3, 3)), f"srcs[0] = {RP} is not a pod in [0, {RP})")
    _refused(t, at(s=(I32 * 4)(0, 64, -1, 70)), f"srcs[2] = -1 is not a pod in [0, {RP})")
    _refused(t, at(d=(I32 * 3)(0, 1, 2**31 - 1)), f"dsts[2] = {2**31 - 1} is not a pod in [0, {RP})")
    _refused(t, at(out=(None, None, None)), "no output requested")
    _refused(partial, at(tt=partial), PARTIAL)
    assert (cells == 77).all()  # (a refused call writes nothing)
    assert at(s=None, ns=0) == _lib.OK and at(d=None, nd=0) == _lib.OK and at(k_lo=1, k_hi=1) == _lib.OK and (cells == 77).all()  # nothing to write
    assert at() == _lib.OK and (cells != 77).all()
    # the Python mirror raises the library's message
    with pytest.raises(CyclonusError, match="unknown view"):
        t.classes(3)
    with pytest.raises(CyclonusError, match=r"dsts\[1\] = 65 is not a pod"):
        t.cells_at([0], [0, RP])
    with pytest.raises(CyclonusError, match=PARTIAL):
        shard.classes()
    # ---- neither call touches the context; both outlive it
    before = _classes(t, "combined"), _cells_at(t, [64, 0], [3, 64, 3])
    eng.close()
    after = _classes(t, "combined"), _cells_at(t, [64, 0], [3, 64, 3])
    _same(after[0], before[0], "after cyc_ctx_destroy")
    assert all(np.array_equal(after[1][n], before[1][n]) for n in CELL_NAMES)
    _same(after[0], a.cells.classes("combined"), "after cyc_ctx_destroy, against the restatement")
    del keep
