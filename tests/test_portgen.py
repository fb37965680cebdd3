"""tests/portgen.py pinned with the oracle alone, for every shape tests/test_gpu_ports.py runs:
(a) D, K and the per-slot status counts are what the generator predicts: K and the status plane against Oracle.shape /
    Oracle.probe, D as the distinct (port, port name, protocol) of the VALID jobs recounted here from the pods and
    probes through tests/effectcheck.py's job expansion; all four statuses occur in the mixed layouts; every word of
    the mixed layout has the DESCW class it was designed for (common / mixed / none, the deviating lanes, the first
    valid lane) recomputed from the oracle's status plane and the generator's descriptor ids;
(b) the whole oracle table equals portgen.model_table — the plain restatement of "a rule admits (peer, descriptor)
    pairs" from each policy's predicted admitted descriptors and peer pods — so every matcher admits exactly the
    descriptors meta says, and at D >= 31 every matcher meant to decide admits some descriptors and not others in
    cells of both directions; removing the deciding first / last entry of a list, and each near miss, changes the
    table; the last pod's own descriptor has id D - 1 (variant "hi") or 0 ("lo") and alone decides cells in both
    directions;
(c) per direction between 5 % and 95 % of the VALID cells are allowed and there are at least D / 2 distinct slot rows;
(d) for "chunks", the template expansion equals Oracle.probe's whole table at 200 pods;
(e) a uniform layout with D > K cannot exist (each slot has one descriptor for all pods), and the generator says so."""
import numpy as np
import pytest

import effectcheck as ec
import planegen
import portgen as pg
import selgen as sg
from oracle.oracle import Oracle

SMALL = {"n_pods": 200}  # the chunks layout at a size whose whole table the oracle walks quickly
CASES = [(D, K, lay, var) for D, K, lay in pg.SHAPES for var in (("hi",) if lay == "uniform" else ("hi", "lo"))]
# matchers that admit nothing unless a probe builds their descriptor, or everything: trivial on purpose
TRIVIAL = {"all-ports", "all-peers", "lowercase", "named-other-proto", "blind"}


def _problem(D, K, layout, variant="hi", **kw):
    return pg.port_problem(D, K, layout, variant, **(SMALL if layout == "chunks" else {}), **kw)


def _table(prob):
    pols, res, probes, _ = prob
    return sg.whole_table(Oracle(pols, res), probes)


@pytest.mark.parametrize("D,K,layout,variant", CASES, ids=lambda x: str(x))
def test_shape_statuses_and_model(D, K, layout, variant):
    prob = _problem(D, K, layout, variant)
    pols, res, probes, meta = prob
    pods = res["Pods"]
    P = len(pods)
    assert Oracle(pols, res).shape(probes) == (P, K) and (meta["D"], meta["K"], meta["P"]) == (D, K, P)
    assert all(p["Containers"] for p in pods) and P % 64 and sum(bool(c.get("AllAvailable")) for c in probes) <= 1
    table = _table(prob)
    assert np.array_equal(table[0], meta["status"])
    # D recounted through the job expansion of tests/effectcheck.py, in first-seen order over configs, pods, containers
    sl = ec.slots(res, probes)
    assert len(sl) == K
    ids, k = {}, 0
    for cfg in probes:
        ks = [x for x in range(K) if sl[x][0] is cfg]
        for d in range(P):
            for x in ks:
                st, *desc = ec.job(res, probes, d, x, sl)
                assert st == meta["status"][d, x]
                if st == ec.VALID:
                    assert meta["slot_desc"][d, x] == ids.setdefault(tuple(desc), len(ids))
    assert list(ids) == meta["desc_ids"] and len(ids) == D
    counts = meta["status_counts"]
    assert counts.shape == (K, 4) and all(np.array_equal(counts[:, s], (table[0] == s).sum(0)) for s in range(4))
    # (b) the whole table is the restatement
    got_in, got_eg = pg.unpack(table)
    want_in, want_eg = pg.model_table(meta)
    assert np.array_equal(got_in, want_in) and np.array_equal(got_eg, want_eg)
    # (c) the condition on the planes
    n_valid = int((table[0] == ec.VALID).sum()) * P
    for name, cells, plane in (("ingress", got_in, table[1]), ("egress", got_eg, table[2])):
        assert 0.05 <= cells.sum() / n_valid <= 0.95, (name, cells.sum() / n_valid)
        assert len(np.unique(plane.reshape(-1, plane.shape[-1]), axis=0)) >= D / 2, name
    if layout == "uniform":
        assert (table[0] == ec.VALID).all() and (meta["word_class"] >= 0).all()
        assert all(len(set(meta["slot_desc"][:, x])) == 1 for x in range(K))
        return
    assert (counts.sum(0) > 0).all(), "a job status that never occurs"
    # the last pod's own descriptor: id D - 1 or 0, nowhere else, and it alone decides cells in both directions
    z = meta["zed_id"]
    assert z == (D - 1 if variant == "hi" else 0)
    holders = np.argwhere(meta["slot_desc"] == z)
    assert set(holders[:, 0]) == {P - 1}
    if layout == "chunks":  # (200 pods hold the first groups only; the full size: test_chunks_expansion_equals_whole_table)
        return
    for name in ("list3-first", "list3-last"):
        pol = next(p for p in meta["policies"] if p["name"] == name and not p["second"])
        assert pol["admits"].sum() == 1 and pol["admits"][z]
        src = int(np.flatnonzero(meta["group_of_pod"] == pol["group"])[0 if name == "list3-first" else -1])
        row = got_eg[src, P - 1]  # egress: the policy's pods to the last pod
        assert pol["peers"][P - 1] and row[meta["slot_desc"][P - 1] == z].all()
    last = got_in[:, P - 1]  # ingress of the last pod (list3-last's): some source is admitted in zed's slots only
    only = last[:, meta["slot_desc"][P - 1] == z].all(1) & ~last[:, (meta["slot_desc"][P - 1] != z) & (meta["status"][P - 1] == 1)].any(1)
    assert only.any()


@pytest.mark.parametrize("D,K", [(4, 4), (5, 9), (33, 8), (33, 33)])
def test_words_have_their_designed_class(D, K):
    """Word 0 common in every slot; word 1 as word 0 but lane 0 deviates; word 2: lane 63 deviates, lanes 0-2 hold no job in
    the upper AllAvailable slots (the first valid lane is 3) and fail the named / numbered probes; word 3: slot 0 common,
    every upper slot without a job; word 4 mixed in every AllAvailable slot with every descriptor but zed's; word 5 mixed."""
    pols, res, probes, meta = pg.port_problem(D, K, "mixed", "hi")
    status = Oracle(pols, res).probe(probes)[0]
    wc = pg.word_classes(status, meta["slot_desc"])
    assert np.array_equal(wc, meta["word_class"])
    A = max(len(p["Containers"]) for p in res["Pods"])
    aa = list(range(K - A, K))  # variant "hi": the AllAvailable slots are the last
    sd = meta["slot_desc"]
    assert (wc[0] != -1).all() and (wc[0, aa] >= 0).all()
    dev1 = [k for k in range(K) if wc[1, k] == -1]
    assert aa[1] in dev1 and wc[1, aa[0]] >= 0
    for k in dev1:  # exactly one deviating destination: lane 0
        lanes = sd[64:128, k]
        assert status[64, k] == ec.VALID and lanes[0] != lanes[1] and len(set(lanes[1:])) == 1
    k = aa[1]
    assert wc[2, k] == -1 and (status[128:131, k] == ec.NONE).all() and status[131, k] == ec.VALID
    lanes = sd[131:192, k]
    assert len(set(lanes[:-1])) == 1 and lanes[-1] != lanes[0]
    assert {int(s) for s in status[128:131].ravel()} == {ec.NONE, ec.VALID, ec.BAD_NAMED_PORT, ec.BAD_PORT_PROTOCOL}
    # (slot aa[0] is every pod's first container, t0: valid everywhere; without extras the third container is t2 everywhere)
    mixed = aa[1:] if D >= 31 else aa[1:2]
    assert (wc[:, aa[0]] >= 0).all() and (wc[3, aa[1:]] == -2).all() and (wc[4, mixed] == -1).all() and (wc[5, mixed] == -1).all()
    assert set(sd[256:320, aa].ravel()) - {-1} == set(sd[:, aa].ravel()) - {-1, meta["zed_id"]}  # every container type but zed
    assert (wc == -2).any() and any(wc[w, k] == -2 and wc[w + 1, k] == -1 for w in range(5) for k in range(K))  # -2 next to mixed


@pytest.mark.parametrize("D,K", [(31, 8), (33, 33)])
def test_every_matcher_decides(D, K):
    """With >= 31 descriptors every matcher not trivial on purpose admits some descriptors and refuses others, and both
    kinds occur in cells of its own pods' rows, in both directions, under each peer kind."""
    pols, res, probes, meta = pg.port_problem(D, K, "mixed", "hi")
    got_in, got_eg = pg.unpack(_table((pols, res, probes, meta)))
    sd, valid, grp = meta["slot_desc"], meta["status"] == ec.VALID, meta["group_of_pod"]
    for pol in meta["policies"]:
        if pol["second"] or pol["name"] in TRIVIAL:
            continue
        adm = pol["admits"]
        assert 0 < adm.sum() < D, pol["name"]
        mine = np.flatnonzero(grp == pol["group"])
        held = sd[mine][valid[mine]]
        if pol["name"] not in ("merge-a", "merge-b", "list5-first", "list3-first", "no-proto", "ports-only"):
            assert adm[held].any() and not adm[held].all(), f"{pol['name']}: its pods' own jobs do not tell (ingress)"
        seen = sd[pol["peers"]][valid[pol["peers"]]]
        assert adm[seen].any() and not adm[seen].all(), f"{pol['name']}: its peers' jobs do not tell (egress)"
    names = {p["name"] for p in meta["policies"]}
    assert names == set(pg.MATCHERS) and set(pg.GROUP_OF) == names
    groups = [g for n, g in pg.GROUP_OF.items() if n != "merge-b"]
    assert len(set(groups)) == len(groups) and pg.GROUP_OF["merge-a"] == pg.GROUP_OF["merge-b"]
    # each peer kind alone selects pods of every policy with peers
    for pol in pols:
        for rule in pol["spec"]["ingress"][:1]:
            if "from" in rule:
                assert ["podSelector" in p and "namespaceSelector" in p for p in rule["from"]] == [True, False, False]
                assert "ipBlock" in rule["from"][2] and rule["from"][1]["namespaceSelector"]


@pytest.mark.parametrize("D,K", pg.LONG)
def test_long_list(D, K):
    """The long-list policy: more than 256 entries on one class, the table still the restatement, and in the ingress rows
    of its pods some source is admitted in a slot past the first four and refused in the slot four below it (an entry's
    slot bit k read as bit k mod 4 changes the table)."""
    prob = pg.port_problem(D, K, "mixed", long_list=True)
    meta = prob[3]
    assert sum(p["name"] == "long-list" for p in meta["policies"]) == pg.LONG_LIST > 256
    assert len({tuple(np.flatnonzero(p["peers"])) for p in meta["policies"] if p["name"] == "long-list"}) == pg.LONG_LIST
    got_in, got_eg = pg.unpack(_table(prob))
    want_in, want_eg = pg.model_table(meta)
    assert np.array_equal(got_in, want_in) and np.array_equal(got_eg, want_eg)
    mine = np.flatnonzero(meta["group_of_pod"] == pg.LONG_GROUP)
    rows = got_in[:, mine]  # [s, d, k]
    assert any((rows[:, :, k] & ~rows[:, :, k - 4]).any() for k in range(4, K))
    assert any((rows[:, :, k - 4] & ~rows[:, :, k]).any() for k in range(4, K))


def _changed(base, prob):
    got = _table(prob)
    assert np.array_equal(got[0], base[0])
    return [not np.array_equal(a, b) for a, b in zip(got[1:], base[1:])]


@pytest.mark.parametrize("D,K", [(33, 8)])
def test_entry_order_and_near_misses_change_the_table(D, K):
    base = _table(pg.port_problem(D, K, "mixed", "hi"))
    for name in pg.ENTRY_ORDER:
        ports = pg.MATCHERS[name]
        less = ports[1:] if name.endswith("first") else ports[:-1]
        assert all(e["port"] >= 7000 for e in less)  # what stays matches no job
        # (list3-first's own pods do not hold zed, the last pod's: its ingress rows are zero either way)
        assert _changed(base, pg.port_problem(D, K, "mixed", "hi", replace={name: less})) == [name != "list3-first", True], name
    for name, miss in pg.NEAR_MISS:
        assert _changed(base, pg.port_problem(D, K, "mixed", "hi", replace={name: miss})) == [True, True], (name, miss)


def test_chunks_expansion_equals_whole_table():
    prob = _problem(4, 4, "chunks")
    pols, res, probes, meta = prob
    tpl_of, base_of = meta["tpl_of"], np.arange(4)
    orc = Oracle(pols, res)
    want = _table(prob)
    first = planegen.first_pods(tpl_of, meta["T"])
    R_in, R_eg, S = planegen.template_rows(orc, probes, first, base_of, bases=list(base_of))
    assert np.array_equal(S[tpl_of], want[0]) and np.array_equal(R_in[tpl_of], want[1]) and np.array_equal(R_eg[tpl_of], want[2])
    assert meta["T"] < len(tpl_of) // 2
    big = pg.port_problem(4, 4, "chunks")[3]  # the size the GPU test runs: a second 64-word chunk with mixed words
    assert big["P"] == 65 * 64 + 37 and (big["word_class"][64:] == -1).any() and (big["word_class"][64:] == -2).any()
    assert set(np.argwhere(big["slot_desc"] == big["zed_id"])[:, 0]) == {big["P"] - 1}


def test_uniform_needs_a_slot_per_descriptor():
    with pytest.raises(ValueError, match="D <= K"):
        pg.port_problem(32, 8, "uniform")
