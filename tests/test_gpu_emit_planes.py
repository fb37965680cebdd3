"""Whole planes of every emit kernel against the oracle, at the sizes the kernels switch at.

The pods are stamped from a few templates (tests/planegen.py), so a whole plane is a few oracle rows
expanded by template — what tests/test_planegen.py validates with the oracle alone — and the
comparison runs on the device.  Every run writes into planes that sit inside larger buffers filled
with a sentinel, guard words on either side: a row the emit never wrote keeps the sentinel, a store
before the first or past the last row breaks a guard band.  Every case asserts the kernel the emit
launched (cyc_last_emit), so a change of a threshold has to edit the tables of planegen.py, and runs
twice on one context (the second run finds the state the first one left).

- test_target_planes: the ladder of row lengths, both edges of every kernel's range, identity-set
  ("runs") and materialised-row ("shuffled") class rows, in place and from their own buffer.
- test_path_options: every path option against the same reference, row phases among them.
- test_plane_alignment: planes at 8-byte and at 16-byte offsets from the allocation (the host's
  % 16 switches, the class rows' pair stores, the wide kernels' line-aligned heads).
- test_source_shards: k_emit_units' flat sweep, 8-row groups, one-row units and unit cap, and the
  per-plane launches of a shard with odd row words.
- test_misaligned_plane_refused: a plane pointer that is not 8-byte aligned is an argument error and
  launches nothing.
"""
import functools
import json

import pytest

import planegen as pg
from planecheck import _expected, _Guarded, _run_and_check  # (with _mismatch: shared with test_gpu_front_limits.py)
from cyclonus_amd._lib import ERR_ARG, CyclonusError
from cyclonus_amd.engine import Engine
from oracle.oracle import Oracle

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("gpu")]


@functools.lru_cache(maxsize=None)
def _case(key):
    """The problem of a (seed, T, P, K, layout) and its reference rows, computed once."""
    prob = pg.template_problem(*key)
    pols, res, probes, tpl_of, base_of = prob
    status, R_in, R_eg, _, _ = pg.reference_planes(Oracle(pols, res), prob)
    return {"key": key, "policies": json.dumps(pols), "resources": json.dumps(res), "probes": probes, "tpl_of": tpl_of,
            "base_of": base_of, "first": pg.first_pods(tpl_of, key[1]), "status": status, "R_in": R_in, "R_eg": R_eg}


def _engine(case):
    eng = Engine(0).build_policies(case["policies"]).load_resources(case["resources"])
    sh = eng.prepare(case["probes"])
    _, _, P, K, _ = case["key"]
    assert (sh["pods"], sh["slots"], sh["words"]) == (P, K, (P + 63) // 64), sh
    assert not sh["may_panic"]
    return eng


def _route_checks(eng, layout, K):
    """The automatic route of a layout: identity-set class rows written in place on the fused front for
    template runs; materialised rows where the templates are shuffled, a wave per 64-word chunk for
    <= 4 slots.  (The <= 32-slot bit rows of the materialised class rows are a function of K alone.)"""
    if layout == "runs":
        assert eng.get_option("pod_words") == 1
        assert eng.get_option("front_fused_active") == 1
        assert eng.get_option("class_inplace_active") == 1
    else:
        assert eng.get_option("pod_words") == 0
        assert eng.get_option("pl_wave_active") == (1 if K <= 4 else 0)


def _force_pm_inplace(eng, K):
    """Materialised-row class rows per pod on the fused front, written into the caller's planes: with a
    few templates shuffled over the pods the automatic route is the two-branch DAG, whose class rows go
    to a buffer of the library's own.  class_inplace_active needs a run: the caller asserts it."""
    eng.set_option("pod_rows", 1)
    eng.set_option("class_inplace", 1)
    assert eng.get_option("front_fused_active") == 1
    assert eng.get_option("pl_wave_active") == (1 if K <= 4 else 0)


TARGET = [(K, P, kernel, layout) for K, P, kernel, layouts in pg.TARGET_SHAPES for layout in layouts]
BOTH_LAYOUTS = {(K, P) for K, P, _, layouts in pg.TARGET_SHAPES if len(layouts) == 2}


@pytest.mark.parametrize("K,P,kernel,layout", TARGET, ids=[f"K{K}-P{P}-{lay}" for K, P, _, lay in TARGET])
def test_target_planes(K, P, kernel, layout):
    """The ladder: every emit kernel at both edges of its range of row lengths, whole planes."""
    case = _case(pg.case_key(K, P, layout))
    eng = _engine(case)
    exp = _expected(case)
    _run_and_check(eng, case, exp, (kernel, 1))
    _route_checks(eng, layout, K)
    if layout == "shuffled" and (K, P) in BOTH_LAYOUTS:
        _force_pm_inplace(eng, K)
        _run_and_check(eng, case, exp, (kernel, 1), ctx="pod_rows 1 class_inplace 1")
        assert eng.get_option("class_inplace_active") == 1
    eng.close()


@pytest.mark.parametrize("K,P", pg.OPTION_SHAPES, ids=[f"K{K}-P{P}" for K, P in pg.OPTION_SHAPES])
def test_path_options(K, P):
    """Every path option against the reference planes (not against another run of the library): class
    rows from their own buffer, the interleaved row list, the two-branch DAG, graph replay, ordered
    eager launches, and two row phases."""
    kernel = {s[:2]: s[2] for s in pg.TARGET_SHAPES}[(K, P)]
    case = _case(pg.case_key(K, P, "runs"))
    eng = _engine(case)
    exp = _expected(case)
    _run_and_check(eng, case, exp, (kernel, 1), reps=1)
    _route_checks(eng, "runs", K)
    assert eng.get_option("emit_interleave_active") == 0 and eng.get_option("launch") == 2  # (the automatic choices)
    for name, value, default in (("class_inplace", 0, -1), ("emit_interleave", 1, -1), ("emit_interleave", 0, -1),
                                 ("front_fused", 0, 1), ("graphs", 1, -1), ("graphs", 0, -1)):
        eng.set_option(name, value)
        _run_and_check(eng, case, exp, (kernel, 1), ctx=f"{name} {value}")
        if name == "class_inplace":
            assert eng.get_option("class_inplace_active") == 0
        if name == "front_fused":
            assert eng.get_option("front_fused_active") == 0
        if name == "emit_interleave":
            assert eng.get_option("emit_interleave_active") == value
        if name == "graphs":
            assert eng.get_option("launch") == value
        eng.set_option(name, default)
    eng.set_option("row_phases", 2)
    assert eng.get_option("front_fused_active") == 1
    _run_and_check(eng, case, exp, (kernel, 2), ctx="row_phases 2")  # one emit launch per phase
    assert eng.get_option("row_phases_active") == 2
    eng.close()


OFFSETS = [(1, 1), (2, 2), (6, 6), (15, 15), (0, 1)]  # words; the last: only the egress plane offset


@pytest.mark.parametrize("K,P,layout", pg.ALIGN_SHAPES, ids=[f"K{K}-P{P}-{lay}" for K, P, lay in pg.ALIGN_SHAPES])
def test_plane_alignment(K, P, layout):
    """Planes 1, 2, 6 and 15 words past the allocation's alignment.  An odd offset is 8-byte alignment: the
    emit is k_emit_words and the class rows take their 8-byte stores.  An even offset keeps the 16-byte
    kernels, every row's head at another distance from a 128-byte line.  The planes are the same.
    In-place class rows are what meets the caller's alignment: identity-set rows on the automatic route
    of the "runs" shapes, and the wave-per-chunk materialised rows of the shuffled <= 4-slot shapes once
    forced onto the fused front in place (K = 4 / P = 32,768 has even row words, so its pair stores
    switch with the offset; K = 2 / P = 700 has 11 words a row and never pairs)."""
    kernel = {s[:2]: s[2] for s in pg.TARGET_SHAPES}[(K, P)]
    case = _case(pg.case_key(K, P, layout))
    eng = _engine(case)
    exp = _expected(case)
    for forced in (False, True) if layout == "shuffled" else (False,):
        if forced:
            # the class rows' pair-store switch reads the caller's plane only when they are written in place
            _force_pm_inplace(eng, K)
            _run_and_check(eng, case, exp, (kernel, 1), reps=1, ctx="in place")
            assert eng.get_option("class_inplace_active") == 1
        for off in OFFSETS:
            emit = "k_emit_words" if off[0] % 2 or off[1] % 2 else kernel
            _run_and_check(eng, case, exp, (emit, 1), off=off, ctx="in place" if forced else "")
        if not forced:
            _route_checks(eng, layout, K)
    eng.close()


@pytest.mark.parametrize("K,P,layout,ranks,emit", pg.SOURCE_CASES,
                         ids=[f"K{c[0]}-P{c[1]}-{c[3][0][1] - c[3][0][0]}rows" for c in pg.SOURCE_CASES])
def test_source_shards(K, P, layout, ranks, emit):
    """Source shards at the start, middle and end of the pods: the ingress plane is every destination's
    words of the shard, the egress plane the shard's rows, both inside guard bands."""
    case = _case(pg.case_key(K, P, layout))
    eng = _engine(case)
    exp = _expected(case)
    for lo, hi in ranks:
        _run_and_check(eng, case, exp, emit, lo=lo, hi=hi, partition="source")
    eng.close()


def test_misaligned_plane_refused():
    """A plane pointer that is not 8-byte aligned is CYC_ERR_ARG naming the argument, from the run and the
    table-wrap entry points; the refused call launches nothing (every buffer keeps its sentinel) and
    the context then runs normally."""
    import torch

    K, P, kernel, _ = pg.TARGET_SHAPES[0]
    case = _case(pg.case_key(K, P, "runs"))
    eng = _engine(case)
    exp = _expected(case)
    W = (P + 63) // 64
    g_in, g_eg, g_st = _Guarded(P * K * W), _Guarded(P * K * W), _Guarded(P * K, 0, torch.uint8)
    st = torch.cuda.current_stream().cuda_stream
    for d_in, d_eg, arg in ((g_in.ptr + 4, g_eg.ptr, "d_ingress"), (g_in.ptr, g_eg.ptr + 4, "d_egress"),
                            (g_in.ptr + 1, g_eg.ptr + 4, "d_ingress")):
        for part in ("target", "source"):
            with pytest.raises(CyclonusError) as e:
                eng.run_device(d_in, d_eg, g_st.ptr, st, 0, 64, part)
            assert e.value.code == ERR_ARG and arg in e.value.msg and "8-byte" in e.value.msg, e.value
            with pytest.raises(CyclonusError) as e:
                eng.wrap_table(d_in, d_eg, g_st.ptr, 0, 64, part)
            assert e.value.code == ERR_ARG and arg in e.value.msg, e.value
    torch.cuda.synchronize()
    assert g_in.untouched() and g_eg.untouched() and g_st.untouched()
    with pytest.raises(CyclonusError):  # no run yet on this prepare: the refused calls were none
        eng.last_emit()
    _run_and_check(eng, case, exp, (kernel, 1))
    eng.close()
