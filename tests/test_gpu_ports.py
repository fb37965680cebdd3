"""PortMatcher.Allows (portmatcher.go:10-92, 190-199) and the job descriptors through every device path that restates
them, bit-exact against the oracle, at the thresholds of csrc/route.hpp.

The port table reaches the class rows through many encodings: the byte table of portok_blk, its bit rows (portbits_blk,
and portbits_direct_blk when launch A is dropped: entries two at a time, the last one clamped), the slot words of
slot_words_blk (VALID, DESCW from the first valid lane, DM for mixed words), the identity sets of class_ident_blk, the
ordered walk's class_row_word, pl_items (sorted port-bit runs, ingress slot bits for K <= 32, port_mask + DM), the
wave-per-chunk rows (D, K <= 4), the identity-set rows with and without one descriptor per slot (UNI), k_query and
k_eff_rows, and the batched blocks.  tests/portgen.py builds problems with exactly D descriptors and K slots whose
destination words have every DESCW class by design, one policy per matcher shape (tests/test_portgen.py pins it with
the oracle alone and shows that a dropped entry or a near-miss matcher changes the table); here whole device planes are
compared inside guard bands (tests/planecheck.py), twice per context, on every route, each run asserting the route it
took: port_bits_active exactly when D <= 32, uni_desc_active exactly for the uniform layouts, slot_words_active by
route.hpp's rule, pl_wave_active exactly when D <= 4 and K <= 4 on materialised rows.

- test_shapes: D and K on either side of 4, 8, 32 (portgen.SHAPES), every route.
- test_ordered_walk: k_class_rows (a policy with an unparsable CIDR in a namespace without pods: a panic is possible,
  no cell panics).
- test_long_entry_list: a class of 260 entries: pl_items' loop over the entries past its LDS part.
- test_query_path / test_target_effects / test_batched_blocks: the other consumers of the port table.

(A uniform layout has one descriptor per slot, so D <= K: D = 32 beside uni_desc is the shape (32, 32).)
"""
import functools

import numpy as np
import pytest

import effectcheck as ec
import planegen
import portgen as pg
import selgen as sg
from cyclonus_amd._lib import CyclonusPanic
from cyclonus_amd.batch import Batch
from cyclonus_amd.engine import Engine
from oracle.oracle import Oracle, OraclePanic
from planecheck import _expected, _run_and_check

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("gpu")]
ROUTE_NAMES = ("pod_words", "pl_wave_active", "port_bits_active", "slot_words_active", "uni_desc_active")


@functools.lru_cache(maxsize=None)
def _case(D, K, layout, variant="hi", decoy=False, long_list=False):
    """A portgen problem and its reference rows (planecheck's case dict): the whole oracle table, or for "chunks" one
    oracle row per template."""
    pols, res, probes, meta = pg.port_problem(D, K, layout, variant, decoy=decoy, long_list=long_list)
    P = len(res["Pods"])
    orc = Oracle(pols, res)
    base_of = np.arange(K, dtype=np.int64)
    if layout == "chunks":
        tpl_of = meta["tpl_of"]
        first = planegen.first_pods(tpl_of, meta["T"])
        R_in, R_eg, S = planegen.template_rows(orc, probes, first, base_of, bases=list(base_of))
        status = S[tpl_of]
    else:
        status, R_in, R_eg = sg.whole_table(orc, probes)
        tpl_of = np.arange(P, dtype=np.int64)
        first = tpl_of
    assert np.array_equal(status, meta["status"])
    return {"key": (f"portgen-D{D}-{variant}{'-decoy' if decoy else ''}{'-long' if long_list else ''}", len(R_in), P, K, layout), "policies": pols, "resources": res,
            "probes": probes, "meta": meta, "tpl_of": tpl_of, "base_of": base_of, "first": first, "status": status, "R_in": R_in, "R_eg": R_eg}


def _engine(case):
    eng = Engine(0).build_policies(case["policies"]).load_resources(case["resources"])
    sh = eng.prepare(case["probes"])
    _, _, P, K, _ = case["key"]
    meta = case["meta"]
    assert (sh["pods"], sh["slots"], sh["words"]) == (P, K, (P + 63) // 64), sh
    assert sh["descriptors"] == meta["D"] and sh["slots"] == meta["K"], sh
    assert sh["max_word_runs"] <= 4, sh
    return eng


def _routed(eng, case, exp, options, want, **kw):
    """Two runs with `options` set, the reported route compared with `want` and with what D, K and the layout decide,
    then the options back at their defaults."""
    defaults = {n: eng.get_option(n) for n in options}
    for n, v in options.items():
        eng.set_option(n, v)
    _run_and_check(eng, case, exp, None, ctx=str(options), **kw)
    got = {n: eng.get_option(n) for n in want}
    assert got == want, (options, got, want)
    meta = case["meta"]
    ido, plw, bits, words, uni = (eng.get_option(n) for n in ROUTE_NAMES)
    assert bits == int(meta["D"] <= 32) and uni == int(meta["uniform"]), (options, bits, uni)
    assert words == int(not uni or not (ido or plw)), (options, words, uni, ido, plw)  # route.hpp: slot_words
    if not ido and eng.get_option("pl_wave") == 1:
        assert plw == int(meta["D"] <= 4 and meta["K"] <= 4), (options, plw)
    else:
        assert plw == 0, (options, plw)
    for n, v in defaults.items():
        eng.set_option(n, v)


_id = lambda s: "-".join(map(str, s))


@pytest.mark.parametrize("shape", pg.SHAPES, ids=_id)
def test_shapes(shape):
    D, K, layout = shape
    case = _case(D, K, layout)
    eng = _engine(case)
    assert not eng.shape["may_panic"]
    exp = _expected(case)
    P = case["key"][2]
    # materialised rows on the fused front need their pod-peer rows per pod (pod_rows 1: few identities here)
    pm, ido = {"pod_words": 0, "pod_rows": 1}, {"pod_words": 1}
    _routed(eng, case, exp, {}, {"front_fused_active": 1, "launch": 2})  # automatic
    _routed(eng, case, exp, pm, {**pm, "front_fused_active": 1})
    _routed(eng, case, exp, {"pod_words": 0}, {"pod_words": 0})
    for v in (0, 1):  # materialised rows: the batched items alone / a wave per chunk where D, K <= 4
        _routed(eng, case, exp, {**pm, "pl_wave": v}, {**pm, "front_fused_active": 1})
    for rpb in (1, 3):  # identity-set rows, on the fused front and as the DAG's kernels
        _routed(eng, case, exp, {**ido, "class_rpb": rpb}, {**ido, "front_fused_active": 1, "class_rpb": rpb})
        _routed(eng, case, exp, {**ido, "class_rpb": rpb, "front_fused": 0}, {**ido, "front_fused_active": 0, "class_rpb": rpb})
    # the DAG (k_portok, then k_portbits from its bytes), eager, replayed and enqueued
    for words in (0, 1):
        _routed(eng, case, exp, {"pod_words": words, "front_fused": 0}, {"pod_words": words, "front_fused_active": 0})
        _routed(eng, case, exp, {"pod_words": words, "front_fused": 0, "graphs": 0}, {"front_fused_active": 0, "launch": 0})
    for g in (0, 1, 2):  # (a captured graph keeps launch A: the bit rows from the byte table)
        _routed(eng, case, exp, {"graphs": g}, {"front_fused_active": 1, "launch": g})
        _routed(eng, case, exp, {**pm, "graphs": g}, {**pm, "front_fused_active": 1, "launch": g})
    # no selector table: launch A is dropped, the bit rows come from the matchers (portbits_direct_blk)
    for words in (0, 1):
        _routed(eng, case, exp, {"pod_words": words, "pod_rows": 1, "sel_lazy": 1}, {"pod_words": words, "front_fused_active": 1, "sel_lazy": 1})
    for words in (0, 1):
        _routed(eng, case, exp, {"pod_words": words, "pod_rows": 1, "class_inplace": 0},
                {"pod_words": words, "front_fused_active": 1, "class_inplace_active": 0})
    # a middle shard: source rows (whole words), target rows (no multiple of 64 at either end)
    for words in (0, 1):
        for part, lo, hi in (("source", 64, (P // 64 - 1) * 64), ("target", P // 3, 2 * P // 3 + 5)):
            _routed(eng, case, exp, {"pod_words": words, "pod_rows": 1}, {"pod_words": words, "front_fused_active": 1}, lo=lo, hi=hi,
                    partition=part, reps=1)
    eng.close()
    if layout != "uniform":  # the last pod's own descriptor with id 0 instead of D - 1
        case = _case(D, K, layout, "lo")
        eng = _engine(case)
        exp = _expected(case)
        assert case["meta"]["zed_id"] == 0
        _routed(eng, case, exp, {}, {"front_fused_active": 1})
        _routed(eng, case, exp, pm, {**pm, "front_fused_active": 1})
        _routed(eng, case, exp, {**pm, "front_fused": 0}, {**pm, "front_fused_active": 0})
        eng.close()


@pytest.mark.parametrize("shape", pg.ORDERED_WALK, ids=_id)
def test_ordered_walk(shape):
    """k_class_rows (class_row_word, KC = 8: its DM loop for mixed egress words): a policy with an unparsable CIDR in a
    namespace without pods makes a panic possible, so the run walks the peers in order, and no cell panics."""
    D, K = shape
    for variant in ("hi", "lo"):
        case = _case(D, K, "mixed", variant, True)
        eng = _engine(case)
        assert eng.shape["may_panic"]
        exp = _expected(case)
        walk = {"pod_words": 0, "front_fused_active": 0}
        _routed(eng, case, exp, {}, walk)
        _routed(eng, case, exp, {"graphs": 0}, walk)
        P = case["key"][2]
        _routed(eng, case, exp, {}, walk, lo=64, hi=(P // 64 - 1) * 64, partition="source", reps=1)
        eng.close()


@pytest.mark.parametrize("shape", pg.LONG, ids=_id)
def test_long_entry_list(shape):
    """pl_items' general loop: a class of 260 entries (past the 256 kept in LDS) on materialised rows.  With K <= 32 an
    ingress entry carries its slot bits, read at k0 + kk in the second and third slot chunk; with K = 33 it carries the
    port matcher (port_mask); also the identity-set rows and the ordered walk over the same list."""
    D, K = shape
    case = _case(D, K, "mixed", long_list=True)
    eng = _engine(case)
    exp = _expected(case)
    pm = {"pod_words": 0, "pod_rows": 1}
    _routed(eng, case, exp, {}, {"front_fused_active": 1})
    _routed(eng, case, exp, pm, {**pm, "front_fused_active": 1})
    _routed(eng, case, exp, {**pm, "sel_lazy": 1}, {**pm, "front_fused_active": 1})
    _routed(eng, case, exp, {"pod_words": 0, "front_fused": 0}, {"pod_words": 0, "front_fused_active": 0})
    eng.close()


def _end(res, p):
    pod = res["Pods"][p]
    return {"Internal": {"PodLabels": pod["Labels"], "NamespaceLabels": res["Namespaces"].get(pod["Namespace"]), "Namespace": pod["Namespace"]},
            "IP": pod["IP"]}


@pytest.mark.parametrize("shape", pg.CONSUMERS, ids=_id)
def test_query_path(shape):
    """k_query's portok[port * D + desc]: one traffic per (source, destination, descriptor) for 64 pod pairs — every
    descriptor as the traffic's (ResolvedPort, ResolvedPortName, Protocol), whichever job the destination holds."""
    D, K = shape
    pols, res, _, meta = pg.port_problem(D, K, "mixed")
    P = len(res["Pods"])
    pairs = [((37 * n + 11) % P, (101 * n + P - 1) % P) for n in range(64)]
    assert (pairs[0][1] == P - 1) and len(set(pairs)) == 64
    traffics = [{"Source": _end(res, s), "Destination": _end(res, d), "ResolvedPort": port, "ResolvedPortName": name, "Protocol": proto}
                for s, d in pairs for port, name, proto in meta["desc_ids"]]
    want = Oracle(pols).query_traffic(traffics)
    assert not any(isinstance(w, OraclePanic) for w in want)
    assert {(True, True), (False, False), (True, False), (False, True)} == set(want)
    per_desc = np.array(want).reshape(64, D, 2)
    assert all((per_desc[:, j] != per_desc[:, (j + 1) % D]).any() for j in range(D))  # no two neighbouring descriptors alike
    eng = Engine(0).build_policies(pols)
    assert eng.query_traffic(traffics) == want
    assert eng.query_traffic_tables(traffics) == want
    eng.close()


@pytest.mark.parametrize("shape", pg.CONSUMERS, ids=_id)
def test_target_effects(shape):
    """k_eff_rows' portok[port * D + desc] per target: the effect counts of the rows around the words 1 / 2 edge (a
    deviating lane 63, lanes 0-2 without upper jobs) and of the last pods (the descriptor only the last pod holds)."""
    D, K = shape
    case = _case(D, K, "mixed")
    pols, res, probes = case["policies"], case["resources"], case["probes"]
    P = case["key"][2]
    eng = _engine(case)
    orc = Oracle(pols, res)
    ir = eng.policy_ir()
    for lo, hi in ((126, 132), (P - 3, P)):
        t = ec.Tally(orc, res, probes, lo, hi)
        assert [list(ir["Ingress"] or {}), list(ir["Egress"] or {})] == t.keys
        for dr, name in enumerate(("ingress", "egress")):
            want_eff, want_app = t.effects(dr, lo, hi)
            assert (want_eff.sum(axis=(0, 1))[:2] > 0).all(), "no allowing or no denying target in these rows"
            eff, app = eng.target_effects(name, lo, hi)
            assert np.array_equal(app, want_app) and np.array_equal(eff, want_eff), (name, lo, hi, np.argwhere(eff != want_eff)[:5].tolist())
    eng.close()


BLOCK_SHAPES = [(5, 3), (31, 3), (32, 2)]  # each CONSUMERS problem under AllAvailable alone: its containers' descriptors


def test_batched_blocks():
    """Three port problems as blocks of one pass (the batched blocks always take the slot words).  A block answers one
    probe config, so each runs under its AllAvailable config alone: the (5, 9), (32, 8) and (33, 4) problems' pods and
    policies with (D, K) = (5, 3), (31, 3), (32, 2), every upper slot of words 1, 2, 4 and 5 mixed.  Every block's slab
    equals its stand-alone oracle table."""
    blocks = []
    for (D, K), want in zip(pg.CONSUMERS, BLOCK_SHAPES):
        pols, res, _, _ = pg.port_problem(D, K, "mixed")
        blocks.append({"policies": pols, "resources": res, "probe": {"AllAvailable": True}})
        status, slot_desc, descs = pg._jobs(res["Pods"], [blocks[-1]["probe"]])
        assert (len(descs), status.shape[1]) == want and (pg.word_classes(status, slot_desc) == -1).sum() >= 4
    eng = Engine(0)
    got = Batch(blocks).run(eng)
    assert eng.get_option("slot_words_active") == 1 and eng.get_option("pod_words") == 0
    for blk, g in zip(blocks, got):
        assert not isinstance(g, CyclonusPanic), g
        want = Oracle(blk["policies"], blk["resources"]).probe([blk["probe"]])
        assert len(np.unique(want[2])) > 8  # (many different egress words)
        assert want[0].shape[1] == BLOCK_SHAPES[blocks.index(blk)][1]
        for name, a, b in zip(("status", "ingress", "egress"), g, want):
            assert a.shape == b.shape and np.array_equal(a, b), (name, np.argwhere(a != b)[:5].tolist())
    eng.close()
