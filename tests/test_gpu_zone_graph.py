"""cyc_table_zone_graph: the cover edges and tiers between the zones of a device table and the zone reach plane
(csrc/dev_zone_graph.hpp), exact against zonegen's closed forms, against probe.PlaneCells' restatement (a matrix product
over the unpacked zone matrix), against cyc_table_zones and against the closure rows gathered at the zones' first pods.

Graphs written as wrapped planes with the decoys planted (closuregen, zonegen): singleton chains, so Z = P, around the
64-zone word, the cover kernel's row tile and one zone past its column chunk, in both orders so that the pivots of a row
come before and after it; rings whose first pods lie in unrelated words; the diamond and the layers; random digraphs.
Every call is made as the protocol goes (the counts first, then exactly fitting arrays), twice for identical results,
with every host array between sentinels and the plane inside device guard bands one word off 16-byte alignment.  Then
each output alone, a source-row table, the engine's own table against the oracle's planes, the capacity protocol, and
arguments and lifetime."""
import ctypes
import json
import os

import numpy as np
import pytest

import closuregen as cg
import zonegen as zg
from cyclonus_amd import _lib
from cyclonus_amd._lib import CyclonusError
from cyclonus_amd.engine import Engine
from cyclonus_amd.probe import PlaneCells, Resources, Table, new_all_available
from oracle.oracle import Oracle
from planecheck import _Guarded
from test_gpu_closure import BAD_SLOTS, PARTIAL, SLOTS, _err, _zones
from test_gpu_reach import _Host, _wrap
from test_gpu_table_counts import _bare_engine, _Planes
from test_zone_graph import same_as_expected

GOLD = os.path.join(os.path.dirname(__file__), "golden")
pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("gpu")]
COVER_ROWS = 128             # ZC_ROWS: the rows one block of k_zone_cover owns
COVER_CHUNK_ZONES = 128 * 64  # ZC_CHUNK: the column words one block of k_zone_cover owns, in zones
HOST = {"zone": np.int32, "rep": np.int32, "size": np.int64, "tier": np.int32}
ALL = ("zone", "rep", "size", "tier", "edges", "reach")
FILL = 0x5A5A5A5A5A5A5A5A


def _raw(t, k_lo, k_hi, zone=None, n_zones=None, rep=None, size=None, tier=None, edges=None, cap=0, n_edges=None, plane=None, words=0):
    return _lib.lib().cyc_table_zone_graph(t._t, k_lo, k_hi, zone, n_zones, rep, size, tier, edges, cap, n_edges, plane, words)


def _graph(t, k_lo=0, k_hi=None, want=ALL, off=0, ctx=""):
    """cyc_table_zone_graph as its protocol goes, twice: the count-only call, then the outputs in `want` with exactly
    fitting capacities, every host array between sentinels (rep, size and tier have room for P: nothing beyond Z may
    change), the plane inside device guard bands `off` words past a 16-byte boundary -> the dict DeviceTable.zone_graph
    returns, "reach" as u64 [Z, Wz] on the host."""
    import torch

    k_hi = t.slots if k_hi is None else k_hi
    P, runs = t.pods, []
    for _ in range(2):
        nz, ne = _Host((1,), np.int64), _Host((1,), np.int64)
        rc = _raw(t, k_lo, k_hi, n_zones=nz.ptr, n_edges=ne.ptr)
        if rc != _lib.OK:
            raise CyclonusError(rc, _err(t))
        Z, E = int(nz.take(ctx)[0]), int(ne.take(ctx)[0])
        Wz = (Z + 63) // 64
        o = {x: _Host((P,), HOST[x]) for x in want if x in HOST}
        e = _Host((E, 2), np.int32) if "edges" in want else None
        g = _Guarded(Z * Wz, off) if "reach" in want else None
        nz, ne = _Host((1,), np.int64), _Host((1,), np.int64)
        torch.cuda.synchronize()  # (the sentinel fill runs on torch's stream, the call on the table's own)
        rc = _raw(t, k_lo, k_hi, *(o[x].ptr if x in o else None for x in ("zone",)), nz.ptr, *(o[x].ptr if x in o else None for x in ("rep", "size", "tier")),
                  e.ptr if e else None, E if e else 0, ne.ptr, ctypes.c_void_p(g.ptr) if g else None, Z * Wz if g else 0)
        if rc != _lib.OK:
            raise CyclonusError(rc, _err(t))
        torch.cuda.synchronize()
        assert (int(nz.take(ctx)[0]), int(ne.take(ctx)[0])) == (Z, E), f"{ctx}: the counts of the two calls differ"
        out = {"n_zones": Z, "n_edges": E}
        for x, h in o.items():
            arr, n = h.take(ctx), P if x == "zone" else Z
            assert (arr[n:] == h.fill).all(), f"{ctx}: {x} was written beyond the {n} values"
            out[x] = arr[:n]
        if e:
            out["edges"] = e.take(ctx)
        if g:
            assert g.guards_intact(), f"{ctx}: a store outside the zone reach plane (guard band changed)"
            out["reach"] = g.plane.cpu().numpy().view(np.uint64).reshape(Z, Wz)
        runs.append(out)
    assert all(np.array_equal(runs[0][x], runs[1][x]) for x in runs[0]), f"{ctx}: two calls differ"
    return runs[0]


def _check_closed(eng, case, off, ctx):
    pl = _wrap(case.g, 0, off)  # (a wrapped table does not own its planes)
    t = pl.table(eng)
    c = f"{ctx} {case.name} plane offset {off}"
    got = _graph(t, case.k_lo, case.k_hi, off=1 - off, ctx=c)
    same_as_expected(got, zg.expected(case), c)
    return t, pl, got


# ---------------------------------------------------------------- 1. Z at the kernels' edges: singleton chains
@pytest.mark.parametrize("chain", (zg.forward_chain, zg.reverse_chain), ids=("forward", "reverse"))
@pytest.mark.parametrize("P", sorted({1, 2, 63, 64, 65, 129, COVER_ROWS, COVER_ROWS + 1, COVER_CHUNK_ZONES + 1}))
def test_chains_at_the_kernel_edges(P, chain):
    """Z = P zones in a chain: the strict reach is a full triangle (the product's densest case) and all but the P - 1
    steps must go; every output equals the closed form.  The pivots of a row come after it (forward) and before it
    (reverse)."""
    eng = _bare_engine(P, 1)
    _, _, got = _check_closed(eng, chain(P), P % 2, f"P {P}")
    assert got["n_zones"] == P and got["n_edges"] == P - 1 and int(got["tier"].max()) == P - 1


# ---------------------------------------------------------------- 2. rings, the diamond, the layers, the small cases
@pytest.mark.parametrize("P", (129, 1025))
def test_ring_dag(P):
    """The zones are rings over a permutation: rep is not aligned to words and the compression gathers across them.  The
    decoy bridges stay decoys.  zone, n_zones and the sizes are cyc_table_zones'."""
    K = 3
    eng = _bare_engine(P, K)
    case = zg.ring_dag(P, 300 + P, K)
    t, pl, got = _check_closed(eng, case, 1, f"P {P}")
    assert len(set((got["rep"] // 64).tolist())) > 1 or P < 130
    z = _zones(t, case.k_lo, case.k_hi, want=("zone", "n_zones"))
    assert np.array_equal(got["zone"], z["zone"]) and got["n_zones"] == z["n_zones"]
    assert got["size"].tolist() == np.bincount(z["zone"], minlength=z["n_zones"]).tolist()
    sub = _graph(t, 1, K, ctx="the decoy slots alone")  # (no edge there: every pod its own zone)
    assert sub["n_zones"] == P and sub["n_edges"] == 0 and not sub["tier"].any() and sub["rep"].tolist() == list(range(P))


@pytest.mark.parametrize("L,n", ((7, 9), (8, 8), (5, 13), (10, 13)))
def test_layers(L, n):
    eng = _bare_engine(L * n, 1)
    _, _, got = _check_closed(eng, zg.layers(L, n, 40 + L), L % 2, f"{L} x {n}")
    assert got["n_edges"] == (L - 1) * n * n and sorted(set(got["tier"].tolist())) == list(range(L))


def test_diamond_two_slots_one_zone_and_none():
    d = zg.diamond()
    eng = _bare_engine(d.g.P, 1)
    _, _, got = _check_closed(eng, d, 1, "diamond")
    assert got["n_edges"] == 4 and sorted(got["tier"].tolist()) == [0, 1, 1, 2]
    for P in (65, 130):
        eng1 = _bare_engine(P, 1)
        _, _, one = _check_closed(eng1, zg.shuffled_ring(P, 7), 0, f"P {P}")
        assert one["n_zones"] == 1 and one["n_edges"] == 0 and one["reach"].tolist() == [[1]] and one["size"].tolist() == [P]
        _check_closed(eng1, zg.loopbacks(P), 1, f"P {P}")
        eng3 = _bare_engine(P, 3)
        a, b = zg.two_slots(P)
        _, _, first = _check_closed(eng3, a, 0, f"P {P}")
        _, _, both = _check_closed(eng3, b, 1, f"P {P}")
        assert (first["n_zones"], first["n_edges"], both["n_zones"], both["n_edges"]) == (P, 1, P - 1, 0)


# ---------------------------------------------------------------- 3. random digraphs against the restatement
@pytest.mark.parametrize("P", (129, 1025))
def test_random_sparse(P):
    """Against PlaneCells.zone_graph over the whole range and a sub-range; d_zreach against the closure's rows gathered on
    the device at rep, bit for bit; zone, n_zones and the sizes against cyc_table_zones on the same table."""
    import torch

    K = 3
    case = cg.random_sparse(P, K, 500 + P)
    pl = _wrap(case.g, 0, 1)
    eng = _bare_engine(P, K)
    t = pl.table(eng)
    cells = case.g.cells()
    for k_lo, k_hi in ((0, K), (0, 1)):
        ctx = f"P {P} [{k_lo}, {k_hi})"
        got = _graph(t, k_lo, k_hi, off=1, ctx=ctx)
        want = cells.zone_graph(k_lo, k_hi, want=ALL)
        assert got["n_zones"] == want["n_zones"] and got["n_edges"] == want["n_edges"], ctx
        for x in ALL:
            assert got[x].dtype == want[x].dtype and np.array_equal(got[x], want[x]), f"{ctx}: {x} differs at {np.argwhere(got[x] != want[x])[:5].tolist()}"
        z = _zones(t, k_lo, k_hi, want=("zone", "n_zones"))
        assert np.array_equal(got["zone"], z["zone"]) and got["n_zones"] == z["n_zones"]
        assert got["size"].tolist() == np.bincount(z["zone"], minlength=z["n_zones"]).tolist()
        rep = torch.from_numpy(got["rep"].astype(np.int64)).cuda()
        rows = t.closure("from", k_lo, k_hi, want=("plane",))["plane"][rep]
        bits = ((rows[:, rep // 64] >> (rep % 64)[None, :]) & 1).bool().cpu().numpy()
        assert np.array_equal(got["reach"], zg.pack_zone_plane(bits)), f"{ctx}: d_zreach is not the closure at the zones' first pods"
        assert not cg.unpack(got["reach"], got["n_zones"])[:, got["n_zones"]:].any()
    assert got["n_edges"] > 0 and got["tier"].max() >= 1


# ---------------------------------------------------------------- 4. outputs alone; a source-row table; the mirror
def test_each_output_alone_a_source_table_and_the_mirror():
    import torch

    P, K = 1025, 3
    case = cg.random_sparse(P, K, 34)
    pl = _wrap(case.g, 0, 1)
    eng = _bare_engine(P, K)
    t = pl.table(eng)
    ts = eng.wrap_table(pl.d_in.data_ptr(), pl.d_eg.data_ptr(), pl.d_st.data_ptr(), 0, P, "source")
    assert ts.partition == "source" and (ts.row_lo, ts.row_hi) == (0, P)
    full = _graph(t, ctx="all outputs")
    Z, E = full["n_zones"], full["n_edges"]
    same = lambda a, b: all(np.array_equal(a[x], b[x]) for x in a)  # noqa: E731
    for x in ALL:
        alone = _graph(t, want=(x,), ctx=f"{x} alone")
        assert set(alone) == {x, "n_zones", "n_edges"} and same(alone, full), f"{x} alone"
    # without n_edges: the tiers alone need the list, the plane alone needs no product; Z alone
    nz, tier = _Host((1,), np.int64), _Host((P,), np.int32)
    assert _raw(t, 0, K, n_zones=nz.ptr, tier=tier.ptr) == _lib.OK, _err(t)
    assert int(nz.take("")[0]) == Z and tier.take("")[:Z].tolist() == full["tier"].tolist()
    g = _Guarded(Z * ((Z + 63) // 64), 1)
    torch.cuda.synchronize()
    assert _raw(t, 0, K, n_zones=nz.ptr, plane=ctypes.c_void_p(g.ptr), words=g.n) == _lib.OK, _err(t)
    torch.cuda.synchronize()
    assert g.guards_intact() and np.array_equal(g.plane.cpu().numpy().view(np.uint64).reshape(full["reach"].shape), full["reach"])
    nz = _Host((1,), np.int64)
    assert _raw(t, 0, K, n_zones=nz.ptr) == _lib.OK and int(nz.take("")[0]) == Z
    for k_lo, k_hi in ((0, K), (1, 2), (2, 2)):
        assert same(_graph(ts, k_lo, k_hi), _graph(t, k_lo, k_hi)), f"source table [{k_lo}, {k_hi})"
    # the Python mirror
    m = t.zone_graph()
    assert set(m) == {"zone", "rep", "size", "tier", "edges", "n_zones", "n_edges"} and same(m, {x: full[x] for x in m})
    assert m["edges"].dtype == np.int32 and m["edges"].shape == (E, 2) and m["size"].dtype == np.int64 and len(m["rep"]) == Z
    for kw in ({}, {"max_zones": P}, {"max_zones": Z}):
        r = t.zone_graph(want=("reach", "tier"), **kw)
        assert set(r) == {"reach", "tier", "n_zones", "n_edges"} and r["reach"].dtype == torch.int64 and tuple(r["reach"].shape) == full["reach"].shape
        assert np.array_equal(r["reach"].cpu().numpy().view(np.uint64), full["reach"]) and r["tier"].tolist() == full["tier"].tolist()
    for cap in (E, E + 3):  # (the bounds known: one call)
        one = t.zone_graph(want=ALL, max_zones=Z, max_edges=cap)
        assert one["edges"].shape == (E, 2) and same({x: one[x] for x in m}, m) and np.array_equal(one["reach"].cpu().numpy().view(np.uint64), full["reach"])
    with pytest.raises(CyclonusError, match=f"edge_cap = {E - 1} is less than the {E} cover edges"):
        t.zone_graph(max_edges=E - 1)
    assert t.zone_graph(want=()) == {"n_zones": Z, "n_edges": E}
    with pytest.raises(CyclonusError, match="zreach_words = .* is less than"):
        t.zone_graph(want=("reach",), max_zones=Z - 1)


def test_the_engines_table_equals_the_oracle():
    """Config #1: the engine's own table against PlaneCells.zone_graph on the oracle's planes, and through probe.Table."""
    c = json.load(open(os.path.join(GOLD, "config1.json")))
    eng = Engine(0)
    want = PlaneCells(*Oracle(c["policies"], c["resources"]).probe(c["probes"]))
    eng.build_policies(c["policies"]).load_resources(c["resources"])
    eng.prepare(c["probes"])
    t = eng.table()
    for k_lo, k_hi in ((0, t.slots), (0, 1)):
        got, w = _graph(t, k_lo, k_hi, ctx=f"config #1 [{k_lo}, {k_hi})"), want.zone_graph(k_lo, k_hi, want=ALL)
        assert all(np.array_equal(got[x], w[x]) for x in w), f"config #1 [{k_lo}, {k_hi})"
    res, cfg = Resources.from_json(c["resources"]), new_all_available()
    eng.prepare([cfg.to_json()])
    dt = eng.table()
    st, ing, eg = Oracle(c["policies"], c["resources"]).probe([cfg.to_json()])
    on_dev, on_host = Table(res, cfg, dt, 0, dt.slots), Table(res, cfg, PlaneCells(st, ing, eg), 0, st.shape[1])
    assert on_dev.zone_graph() == on_host.zone_graph()
    assert on_dev.render_zone_graph() == on_host.render_zone_graph() and on_dev.render_zone_graph("dot") == on_host.render_zone_graph("dot")


# ---------------------------------------------------------------- 5. the capacity protocol
def test_capacities():
    import torch

    L, n = 5, 13
    case = zg.layers(L, n, 3)
    P = case.g.P
    want = zg.expected(case)
    Z, E, Wz = want["n_zones"], want["n_edges"], 2
    assert (Z, E) == (65, 4 * 169)
    pl = _wrap(case.g)
    eng = _bare_engine(P, 1)
    t = pl.table(eng)
    vp = lambda x: ctypes.c_void_p(x.ctypes.data)  # noqa: E731
    nz, ne = np.full(1, FILL, np.int64), np.full(1, FILL, np.int64)
    zone, rep, tier = (np.full(P, 0x5A5A5A5A, np.int32) for _ in range(3))
    size = np.full(P, FILL, np.int64)
    edges = np.full((E + 1, 2), 0x5A5A5A5A, np.int32)
    plane = torch.full((Z * Wz + 2,), FILL, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    d = plane.data_ptr() + 8

    def arrays_untouched():
        torch.cuda.synchronize()
        return bool((plane == FILL).all()) and (size == FILL).all() and all((x == 0x5A5A5A5A).all() for x in (zone, rep, tier, edges))

    # a count-only call
    assert _raw(t, 0, 1, n_zones=vp(nz), n_edges=vp(ne)) == _lib.OK, _err(t)
    assert (nz[0], ne[0]) == (Z, E) and arrays_untouched()
    # edge_cap one short: the total in the message and in *n_edges, nothing else written
    nz[:], ne[:] = FILL, FILL
    rc = _raw(t, 0, 1, vp(zone), vp(nz), vp(rep), vp(size), vp(tier), vp(edges), E - 1, vp(ne), ctypes.c_void_p(d), Z * Wz)
    assert rc == _lib.ERR_ARG and _err(t) == f"edge_cap = {E - 1} is less than the {E} cover edges", (rc, _err(t))
    assert (nz[0], ne[0]) == (Z, E) and arrays_untouched()
    # zreach_words one short likewise (the number of edges is not known yet)
    nz[:], ne[:] = FILL, FILL
    rc = _raw(t, 0, 1, vp(zone), vp(nz), vp(rep), vp(size), vp(tier), vp(edges), E, vp(ne), ctypes.c_void_p(d), Z * Wz - 1)
    assert rc == _lib.ERR_ARG and _err(t) == f"zreach_words = {Z * Wz - 1} is less than the {Z * Wz} words of the plane of {Z} zones", (rc, _err(t))
    assert nz[0] == Z and ne[0] == FILL and arrays_untouched()
    # exactly fitting: exactly that much is written
    rc = _raw(t, 0, 1, vp(zone), vp(nz), vp(rep), vp(size), vp(tier), vp(edges), E, vp(ne), ctypes.c_void_p(d), Z * Wz)
    assert rc == _lib.OK, _err(t)
    torch.cuda.synchronize()
    host = plane.cpu().numpy().view(np.uint64)
    assert host[0] == FILL and host[-1] == FILL and np.array_equal(host[1:-1].reshape(Z, Wz), zg.pack_zone_plane(want["reach"]))
    assert (edges[E] == 0x5A5A5A5A).all() and np.array_equal(edges[:E], want["edges"]) and (nz[0], ne[0]) == (Z, E)
    assert np.array_equal(zone, want["zone"]) and np.array_equal(rep[:Z], want["rep"]) and np.array_equal(tier[:Z], want["tier"]) and np.array_equal(size[:Z], want["size"])
    # more room than needed is fine
    assert _raw(t, 0, 1, n_zones=vp(nz), edges=vp(edges), cap=E + 1, n_edges=vp(ne)) == _lib.OK and (edges[E] == 0x5A5A5A5A).all()
    # the Python mirror carries the message
    with pytest.raises(CyclonusError, match="words of the plane of 65 zones"):
        t.zone_graph(want=("reach",), max_zones=64)


# ---------------------------------------------------------------- 6. what the call refuses; the empty cases; lifetime
RP, RK = 65, 3


def test_refusals_empty_cases_and_lifetime():
    import torch

    eng = _bare_engine(RP, RK)
    a = _Planes(RP, RK, 22)
    t = a.table(eng)
    keep, shard = a.source_shard(eng, 64, RP)
    p_in, p_eg = a._dev(a.h_in[10:50].contiguous()), a._dev(a.h_eg[10:50].contiguous())
    partial = eng.wrap_table(p_in.data_ptr(), p_eg.data_ptr(), a.d_st.data_ptr(), 10, 50, "target")
    plane = torch.full((RP * 2 + 2,), FILL, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    d = plane.data_ptr()
    vp = lambda x: ctypes.c_void_p(x.ctypes.data)  # noqa: E731
    nz, ne = np.full(1, FILL, np.int64), np.full(1, FILL, np.int64)
    zone, rep, tier = (np.full(RP, 0x5A5A5A5A, np.int32) for _ in range(3))
    size = np.full(RP, FILL, np.int64)
    edges = np.full((RP * RP, 2), 0x5A5A5A5A, np.int32)

    def call(tt=t, k_lo=0, k_hi=RK, n_zones=nz, e=edges, cap=RP * RP, n_edges=ne, dz=d, words=RP * 2):
        return _raw(tt, k_lo, k_hi, vp(zone), vp(n_zones) if n_zones is not None else None, vp(rep), vp(size), vp(tier), vp(e) if e is not None else None, cap,
                    vp(n_edges) if n_edges is not None else None, ctypes.c_void_p(dz), words)

    def untouched():
        torch.cuda.synchronize()
        return bool((plane == FILL).all()) and all((x == FILL).all() for x in (nz, ne, size)) and all((x == 0x5A5A5A5A).all() for x in (zone, rep, tier, edges))

    def refused(tt, rc, msg):
        assert rc == _lib.ERR_ARG and _err(tt) == msg, (rc, _err(tt), msg)
        assert untouched(), f"{msg}: a refused call wrote something"

    assert _lib.lib().cyc_table_zone_graph(None, 0, RK, None, vp(nz), None, None, None, None, 0, None, None, 0) == _lib.ERR_ARG and untouched()
    for k_lo, k_hi in BAD_SLOTS:
        refused(t, call(k_lo=k_lo, k_hi=k_hi), SLOTS)
    for other in (partial, shard):
        refused(other, call(tt=other), PARTIAL)
    refused(t, call(n_zones=None), "null n_zones")
    refused(t, call(n_edges=None), "edges without n_edges")
    refused(t, call(cap=-1), "negative edge_cap")
    refused(t, call(e=None), "null edges with edge_cap > 0")
    refused(t, call(dz=d + 4), "d_zreach is not 8-byte aligned")
    refused(t, call(words=-1), "negative zreach_words")
    # ---- the good call: 8-byte alignment is enough
    want = a.cells.zone_graph(want=ALL)
    Z, E = want["n_zones"], want["n_edges"]
    Wz = (Z + 63) // 64
    assert call(dz=d + 8, words=Z * Wz) == _lib.OK, _err(t)
    torch.cuda.synchronize()
    host = plane.cpu().numpy().view(np.uint64)
    assert host[0] == FILL and (host[1 + Z * Wz:] == FILL).all() and np.array_equal(host[1:1 + Z * Wz].reshape(Z, Wz), want["reach"])
    assert (nz[0], ne[0]) == (Z, E) and np.array_equal(zone, want["zone"]) and np.array_equal(edges[:E], want["edges"]) and (edges[E:] == 0x5A5A5A5A).all()
    assert np.array_equal(tier[:Z], want["tier"]) and np.array_equal(rep[:Z], want["rep"]) and np.array_equal(size[:Z], want["size"])
    # ---- an empty slot range: every pod its own zone, the identity plane
    got = _graph(t, 1, 1, off=1, ctx="empty slot range")
    assert got["n_zones"] == RP and got["n_edges"] == 0 and got["edges"].shape == (0, 2)
    assert got["zone"].tolist() == got["rep"].tolist() == list(range(RP)) and got["size"].tolist() == [1] * RP and not got["tier"].any()
    assert np.array_equal(got["reach"], cg.pack(np.eye(RP, dtype=bool)))
    # ---- no pod at all: the two counts and nothing else
    eng0 = Engine(0).build_policies([]).load_resources({"Namespaces": {"n": {}}, "Pods": []})
    eng0.prepare([{"Port": 80, "Protocol": "TCP"}])
    t0 = eng0.table()
    assert t0.pods == 0
    nz[:], ne[:] = FILL, FILL
    zone[:] = rep[:] = tier[:] = 0x5A5A5A5A
    size[:], edges[:] = FILL, 0x5A5A5A5A
    plane.fill_(FILL)
    assert call(tt=t0, k_hi=t0.slots) == _lib.OK, _err(t0)
    assert (nz[0], ne[0]) == (0, 0)
    nz[:], ne[:] = FILL, FILL
    assert untouched()
    m0 = t0.zone_graph()
    assert m0["n_zones"] == 0 and m0["n_edges"] == 0 and m0["edges"].shape == (0, 2) and len(m0["zone"]) == 0
    # the Python mirror raises the library's message
    with pytest.raises(CyclonusError, match=SLOTS):
        t.zone_graph(0, RK + 1)
    # ---- the call does not touch the context and outlives it
    before = _graph(t, ctx="before")
    eng.close()
    after = _graph(t, ctx="after cyc_ctx_destroy")
    assert all(np.array_equal(before[x], after[x]) for x in before), "after cyc_ctx_destroy"
    same_keys = {x: want[x] for x in after}
    assert all(np.array_equal(after[x], same_keys[x]) for x in after), "after cyc_ctx_destroy, against the restatement"
    del keep
