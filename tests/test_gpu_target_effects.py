"""cyc_probe_target_effects (csrc/dev_effects.hpp): per-target effect counts over the verdict grid, exact against
the oracle's per-cell DirectionResult target lists tallied by tests/effectcheck.py (pinned in
tests/test_target_effects.py).

Random problems at P = 1, 63, 64, 65, 130 (tail word, exact word, three words) over every slot sub-range; wide
rows (65 words) with few target pods; more targets on one pod than a wave has lanes; several class batches and
word windows forced by a small scratch cap; row shards that add up, and the BLOCKED ingress count of
cyc_table_counts; a run's state left alone; refusals; the Python layer on config #1's policies.  Host outputs
lie between sentinel elements.  The oracle's tally of a problem is computed once and shared."""
import ctypes
import functools
import json
import os
import random

import numpy as np
import pytest

import effectcheck as ec
import limitgen
import randgen
from cyclonus_amd import _lib
from cyclonus_amd.engine import Engine
from cyclonus_amd.matcher import Policy
from oracle.oracle import Oracle
from test_target_effects import THREE_PODS, THREE_POLICIES, THREE_PROBES, THREE_WANT, three_pod_targets

GOLD = os.path.join(os.path.dirname(__file__), "golden")
pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("gpu")]
PAD, SENTINEL = 64, -0x5A5A5A5A5A5A5A5B
DIRS = ("ingress", "egress")
# P -> seed of randgen.random_problem(seed, n_pods=P, n_pols=24, bad=False).  For P >= 63 the seeds are chosen so
# that the ORACLE's tally shows, per direction, each of the four counters non-zero for some target, a cell with two
# or more allowing targets and a target that applies to no pod (asserted below), with two or three job slots.  A
# single pod has one fixed set of applying targets, so P = 1 cannot show both sole counters and asserts none of it.
# (Seed 6 at P = 130, tallied with the probe's real jobs, has one slot and no ingress cell with two allowing targets.)
SEEDS = {1: 6, 63: 18, 64: 3, 65: 10, 130: 36}


class _Out:
    """A host output array of `shape` between PAD sentinel elements on either side."""

    def __init__(self, shape):
        self.shape, self.n = shape, int(np.prod(shape))
        self.buf = np.full(self.n + 2 * PAD, SENTINEL, np.int64)

    @property
    def ptr(self):
        return ctypes.c_void_p(self.buf.ctypes.data + 8 * PAD)

    def take(self, ctx):
        assert (self.buf[:PAD] == SENTINEL).all() and (self.buf[PAD + self.n:] == SENTINEL).all(), f"{ctx}: a store outside the output array"
        return self.buf[PAD:PAD + self.n].reshape(self.shape).copy()


def _call(eng, dr, lo, hi, k0, k1, ctx=""):
    """cyc_probe_target_effects with both outputs between sentinels -> (effects [T, nk, 4], applies [T])."""
    T = eng.shape["targets_eg" if dr else "targets_in"]
    eff, app = _Out((T, max(k1 - k0, 0), 4)), _Out((T,))
    rc = _lib.lib().cyc_probe_target_effects(eng._ctx, dr, lo, hi, k0, k1, eff.ptr, app.ptr)
    _lib.check(eng._ctx, rc)
    return eff.take(ctx), app.take(ctx)


def _same(got, want, ctx):
    for name, g, w in zip(("effects", "applies"), got, want):
        assert g.shape == w.shape, f"{ctx}: {name} shape {g.shape} want {w.shape}"
        bad = np.argwhere(g != w)
        assert bad.size == 0, f"{ctx}: {name} differs at {bad[:5].tolist()}: {g[tuple(bad[0])]} want {w[tuple(bad[0])]}"


def _engine(pols, res, probes):
    eng = Engine(0)
    eng.build_policies(pols).load_resources(res)
    eng.prepare(probes)
    return eng


def _keys(eng):
    ir = eng.policy_ir()
    return [list(ir["Ingress"] or {}), list(ir["Egress"] or {})]


@functools.lru_cache(maxsize=None)
def _random(P):
    pols, res, probes = randgen.random_problem(SEEDS[P], n_pods=P, n_pols=24, bad=False)
    return pols, res, probes, ec.Tally(Oracle(pols, res), res, probes)


def _covered(t, dr):
    """What the oracle's expected values must show so that a kernel missing a branch cannot pass."""
    eff, app = t.effects(dr)
    return bool((eff.sum(axis=1) > 0).any(axis=0).all()) and t.multi[dr] > 0 and bool((app == 0).any()) and bool((app > 0).any())


@pytest.mark.parametrize("P", sorted(SEEDS))
def test_random_problems_every_slot_range(P):
    pols, res, probes, t = _random(P)
    eng = _engine(pols, res, probes)
    assert (eng.shape["pods"], eng.shape["slots"], eng.shape["may_panic"]) == (P, t.K, 0)
    assert _keys(eng) == t.keys  # target index = primary-key order on both sides
    if P >= 63:
        assert 2 <= t.K <= 3
        assert _covered(t, 0) and _covered(t, 1), "the seed no longer exercises every counter: choose another (see SEEDS)"
    for dr in (0, 1):
        for k0 in range(t.K + 1):
            for k1 in range(k0, t.K + 1):
                _same(_call(eng, dr, 0, P, k0, k1, f"P={P} {DIRS[dr]} k[{k0},{k1})"), t.effects(dr, 0, P, k0, k1), f"P={P} {DIRS[dr]} k[{k0},{k1})")
        eff, app = eng.target_effects(DIRS[dr])  # the Python entry point: the same arrays
        _same((eff, app), t.effects(dr), f"P={P} {DIRS[dr]} Engine.target_effects")


# ---- wide rows, few target pods: P = 4100 is 65 words (one past a 64-word chunk) with a 4-bit tail
WIDE_P, WIDE_ROWS = 4100, ((0, 3), (60, 70), (4090, 4100))


@functools.lru_cache(maxsize=None)
def _wide():
    """IPv4 pods of randgen with at most two containers (most have one) under one AllAvailable config: two slots, the
    second without a job for most pods, and every destination word mixes several egress descriptors.  The policies
    are randgen's, IPBlock peers among them."""
    r = random.Random(4100)
    pols = [randgen.random_policy(r, i, v6=False, bad=False) for i in range(16)]
    res = randgen.random_resources(r, WIDE_P, v6=False, bad=False)
    for i, pod in enumerate(res["Pods"]):
        pod["Containers"] = pod["Containers"][:2 if i % 9 == 0 else 1]
    return pols, res, [{"AllAvailable": True}], Oracle(pols, res)


@functools.lru_cache(maxsize=None)
def _wide_engine():
    pols, res, probes, _ = _wide()
    return _engine(pols, res, probes)


@pytest.mark.parametrize("rows", WIDE_ROWS)
def test_wide_rows_few_target_pods(rows):
    pols, res, probes, oracle = _wide()
    eng = _wide_engine()
    assert (eng.shape["pods"], eng.shape["words"], eng.shape["slots"]) == (WIDE_P, 65, 2)
    assert eng.shape["ip_peers"] > 0 and eng.shape["descriptors"] > 4
    t = ec.Tally(oracle, res, probes, *rows)
    assert _keys(eng) == t.keys
    for dr in (0, 1):
        want = t.effects(dr)
        assert want[0].any() and want[1].any()
        _same(_call(eng, dr, rows[0], rows[1], 0, 2, f"rows {rows} {DIRS[dr]}"), want, f"rows {rows} {DIRS[dr]}")
        _same(_call(eng, dr, rows[0], rows[1], 1, 2, f"rows {rows} {DIRS[dr]} k1"), t.effects(dr, None, None, 1, 2), f"rows {rows} {DIRS[dr]} k[1,2)")


# ---- more targets on one pod than a wave has lanes
@functools.lru_cache(maxsize=None)
def _heavy():
    pols, res, probes, _, _ = limitgen.class_problem(70, 50, 20, K=2)
    return pols, res, probes, ec.Tally(Oracle(pols, res), res, probes)


def test_seventy_targets_on_one_pod():
    pols, res, probes, t = _heavy()
    eng = _engine(pols, res, probes)
    assert _keys(eng) == t.keys
    for dr in (0, 1):
        want = t.effects(dr)
        assert (want[1] > 0).sum() >= 70 and t.appliers[dr].max() >= 70  # 70 targets apply to the heavy pods
        assert want[0][:, :, ec.SOLE_ALLOWING].any()
        _same(_call(eng, dr, 0, t.P, 0, t.K, f"heavy {DIRS[dr]}"), want, f"heavy {DIRS[dr]}")
        assert eng.get_option("effects_batches") == 1


# ---- several batches and word windows: the scratch cap (dev_effects.hpp, EFF_SCRATCH_CAP) lowered for the process
def _batch_bytes(eng, dr, targets, words):
    """The batch buffers of `targets` targets built `words` words at a time (effects.hpp, target_effects): per target
    and word D row words, per target its population counts (D for ingress, a slot's for egress) and sole counts."""
    D, nk = max(eng.shape["descriptors"], 1), eng.shape["slots"]
    return targets * (((nk if dr else D) + nk) * 8 + D * 8 * words)


@pytest.mark.parametrize("which,factor", [("random", 1), ("random", 4), ("heavy", 1), ("heavy", 4)])
def test_batches_and_windows_give_the_same_counts(which, factor, monkeypatch):
    pols, res, probes, t = _random(130) if which == "random" else _heavy()
    eng = _engine(pols, res, probes)
    W = eng.shape["words"]
    assert W >= 2 and eng.get_option("effects_scratch_cap") == 256 << 20
    whole = {dr: _call(eng, dr, 0, t.P, 0, t.K) for dr in (0, 1)}
    assert eng.get_option("effects_batches") == 1 and eng.get_option("effects_launches") == 1
    most = [int(t.appliers[dr].max()) for dr in (0, 1)]  # the largest class's targets
    applied = [int((t.effects(dr)[1] > 0).sum()) for dr in (0, 1)]
    # the least cap (in KB) under which the largest class of either direction can be built a word at a time
    least_kb = -(-max(_batch_bytes(eng, dr, most[dr], 1) for dr in (0, 1)) // 1024)
    cap_kb = factor * least_kb
    monkeypatch.setenv("CYC_EFFECTS_SCRATCH_KB", str(cap_kb))
    assert eng.get_option("effects_scratch_cap") == cap_kb << 10
    split = False
    for dr in (0, 1):
        ctx = f"{which} cap {cap_kb} KB {DIRS[dr]}"
        got = _call(eng, dr, 0, t.P, 0, t.K, ctx)
        batches, launches = eng.get_option("effects_batches"), eng.get_option("effects_launches")
        _same(got, whole[dr], f"{ctx} ({batches} batches, {launches} launches)")
        _same(got, t.effects(dr), f"{ctx} against the oracle")
        assert launches >= batches >= 1
        assert eng.get_option("effects_scratch_bytes") > 0
        if _batch_bytes(eng, dr, most[dr], W) > cap_kb << 10:
            assert launches > batches, ctx  # the largest class does not fit whole: built a window of words at a time
        if _batch_bytes(eng, dr, applied[dr], W) > cap_kb << 10:
            assert launches > 1, ctx        # all the applying targets' rows do not fit at once
            split = True
    # (the least cap always splits; four times as much may hold a small problem whole: then only the equality)
    assert split or factor > 1, "the least cap split nothing: the test shows nothing"
    if which == "heavy":  # not even one word of the largest class: refused, not overrun
        small = (_batch_bytes(eng, 0, most[0], 1) - 1) // 1024
        assert small >= 1
        monkeypatch.setenv("CYC_EFFECTS_SCRATCH_KB", str(small))
        with pytest.raises(_lib.CyclonusError) as e:
            _call(eng, 0, 0, t.P, 0, t.K)
        assert e.value.code == _lib.ERR_OOM and "scratch cap" in e.value.msg


# ---- partition
def test_row_shards_add_up_and_blocked_ingress_count():
    pols, res, probes, t = _random(130)
    eng = _engine(pols, res, probes)
    P, K = t.P, t.K
    for dr in (0, 1):
        whole = _call(eng, dr, 0, P, 0, K)
        parts = [_call(eng, dr, lo, hi, 0, K, f"shard [{lo},{hi})") for lo, hi in ((0, 37), (37, 64), (64, P))]
        for (lo, hi), part in zip(((0, 37), (37, 64), (64, P)), parts):
            _same(part, t.effects(dr, lo, hi), f"{DIRS[dr]} shard [{lo},{hi})")
        _same((sum(p[0] for p in parts), sum(p[1] for p in parts)), whole, f"{DIRS[dr]} shards against the whole")
    # A VALID ingress cell is BLOCKED iff some target applies and none allows (policy.go:158-173).  With exactly
    # one applier that is the applier's SOLE_DENYING cell; so per slot
    #   BLOCKED = sum over t of SOLE_DENYING[t] + (cells with two or more appliers, all denying),
    # the second term from the oracle's per-cell lists.
    counts = eng.table().counts(want=("ingress",))["ingress"]
    eff, _ = _call(eng, 0, 0, P, 0, K)
    many = ((t.appliers[0] >= 2) & (t.allowers[0] == 0)).sum(axis=(0, 1))
    assert many.any()
    assert (counts[:, _lib.CONN_BLOCKED] == eff[:, :, ec.SOLE_DENYING].sum(axis=0) + many).all()
    # and ALLOWED = cells no target applies to + cells with an allower
    free = ((t.appliers[0] == 0) & (t.status == ec.VALID)[:, None, :]).sum(axis=(0, 1))
    some = (t.allowers[0] > 0).sum(axis=(0, 1))
    assert (counts[:, _lib.CONN_ALLOWED] == free + some).all()


# ---- a run's state is left alone
ACTIVE = ("pod_words", "launch", "front_fused_active", "pl_wave_active", "class_inplace_active", "emit_interleave_active",
          "plvt_active", "ip_iv_rows", "ip_range_rows", "pod_post_rows", "pod_scan_rows", "row_phases_active")


def test_runs_are_not_disturbed():
    pols, res, probes, t = _random(65)
    eng = _engine(pols, res, probes)
    first = {dr: _call(eng, dr, 0, t.P, 0, t.K, "before any run") for dr in (0, 1)}  # needs no run
    for dr in (0, 1):
        _same(first[dr], t.effects(dr), f"{DIRS[dr]} before any run")
    with pytest.raises(_lib.CyclonusError):
        eng.last_emit()  # still no run
    before = eng.run_host()
    emit, active = eng.last_emit(), {n: eng.get_option(n) for n in ACTIVE}
    for dr in (0, 1):
        _same(_call(eng, dr, 0, t.P, 0, t.K), first[dr], f"{DIRS[dr]} after a run")
        _same(_call(eng, dr, 3, 40, 0, 1), t.effects(dr, 3, 40, 0, 1), f"{DIRS[dr]} rows [3,40) after a run")
    assert eng.last_emit() == emit and {n: eng.get_option(n) for n in ACTIVE} == active
    after = eng.run_host()
    for a, b in zip(before, after):
        assert a.tobytes() == b.tobytes()
    assert eng.last_emit() == emit and {n: eng.get_option(n) for n in ACTIVE} == active
    # a partial-row run plans its range; the call in between leaves the plan's results alone too
    part = eng.run_host(10, 50)
    _call(eng, 1, 0, t.P, 0, t.K)
    for a, b in zip(part, eng.run_host(10, 50)):
        assert a.tobytes() == b.tobytes()


# ---- refusals
def _rc(eng, *args, eff=True):
    out = _Out((max(eng.shape["targets_in"], eng.shape["targets_eg"]), eng.shape["slots"], 4))
    rc = _lib.lib().cyc_probe_target_effects(eng._ctx, *args, out.ptr if eff else None, None)
    out.take("a refused call")
    if eff:
        assert (out.buf == SENTINEL).all() or rc == _lib.OK
    return rc, _lib.lib().cyc_last_error(eng._ctx).decode()


def test_refusals():
    pols, res, probes, t = _random(63)
    eng = _engine(pols, res, probes)
    P, K = t.P, t.K
    for args, word in (((2, 0, P, 0, K), "direction"), ((-1, 0, P, 0, K), "direction"), ((0, -1, P, 0, K), "row range"),
                       ((0, 0, P + 1, 0, K), "row range"), ((0, 5, 4, 0, K), "row range"), ((1, 0, P, -1, K), "slot range"),
                       ((1, 0, P, 0, K + 1), "slot range"), ((1, 0, P, 2, 1), "slot range")):
        rc, msg = _rc(eng, *args)
        assert rc == _lib.ERR_ARG and word in msg, (args, rc, msg)
    rc, msg = _rc(eng, 0, 0, P, 0, K, eff=False)
    assert rc == _lib.ERR_ARG and "effects" in msg
    # empty ranges are not errors: zeros (and the applies of the rows) are written
    for dr in (0, 1):
        eff, app = _call(eng, dr, 7, 7, 0, K, "no rows")
        assert eff.shape[1] == K and not eff.any() and not app.any()
        eff, app = _call(eng, dr, 0, P, 1, 1, "no slots")
        assert eff.size == 0 and (app == t.effects(dr)[1]).all()
    # a batched-blocks prepare
    eng.prepare_blocks(probes[:1], [P], [0])
    rc, msg = _rc(eng, 0, 0, P, 0, 1)
    assert rc == _lib.ERR_ARG and "blocks" in msg
    # a problem that can panic: the panic is cyc_probe_run's to report
    found = False
    for seed in range(1, 40):
        pols, res, probes = randgen.random_problem(seed, n_pods=12, n_pols=8, bad=True)
        e2 = Engine(0)
        try:
            e2.build_policies(pols).load_resources(res)
            shape = e2.prepare(probes)
        except _lib.CyclonusError:
            continue
        if shape["may_panic"]:
            rc, msg = _rc(e2, 0, 0, shape["pods"], 0, shape["slots"])
            assert rc == _lib.ERR_ARG and "cyc_probe_run" in msg and "panic" in msg
            found = True
            break
    assert found
    # no targets at all
    e3 = _engine([], THREE_PODS, THREE_PROBES)
    eff, app = _call(e3, 0, 0, 3, 0, 1, "no targets")
    assert eff.shape == (0, 1, 4) and app.shape == (0,)


# ---- the Python layer
def test_three_pod_case_on_the_device():
    eng = _engine(THREE_POLICIES, THREE_PODS, THREE_PROBES)
    for name, (dr, i) in three_pod_targets(_keys(eng)).items():
        eff, app = _call(eng, dr, 0, 3, 0, 1, name)
        assert (tuple(eff[i, 0]), int(app[i])) == THREE_WANT[name], name


def test_policy_target_effects_on_config1():
    c = json.load(open(os.path.join(GOLD, "config1.json")))
    pols, res, probes = c["policies"], c["resources"], c["probes"]
    t = ec.Tally(Oracle(pols, res), res, probes)
    policy = Policy(Engine(0).build_policies(pols))
    te = policy.target_effects(probes, res)
    assert [te.keys[d] for d in DIRS] == t.keys == [list(policy.ingress), list(policy.egress)]
    for dr, d in enumerate(DIRS):
        eff, app = t.effects(dr)
        _same((te.effects[d], te.applies[d]), (eff, app), f"config #1 {d}")
        by_key = te.by_key(d)
        assert list(by_key) == t.keys[dr]
        for i, k in enumerate(t.keys[dr]):
            assert by_key[k] == {"applies": int(app[i]), **{n: eff[i, :, e].tolist() for e, n in enumerate(_lib.EFFECTS)}}
        assert te.unused(d) == [k for i, k in enumerate(t.keys[dr]) if app[i] == 0]
        assert te.never_allowing(d) == [k for i, k in enumerate(t.keys[dr]) if not eff[i, :, ec.ALLOWING].any()]
        redundant = [k for i, k in enumerate(t.keys[dr]) if not eff[i, :, ec.SOLE_ALLOWING:].any()]
        assert te.redundant(d) == redundant and set(te.unused(d)) <= set(redundant)
    text = te.render()
    rows = [line for line in text.splitlines() if line.startswith("| ingress") or line.startswith("| egress")]
    assert len(rows) == len(t.keys[0]) + len(t.keys[1]) and "SOLE DENYING" in text
