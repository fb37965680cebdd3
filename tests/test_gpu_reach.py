"""cyc_table_adjacency / cyc_table_reach: the adjacency bit plane and the multi-hop search on the device
(csrc/dev_reach.hpp), bit-exact against probe.PlaneCells' restatement (edges read off the unpacked bits, a plain queue
per seed set).

The adjacency pass on wrapped random planes (independent of the engine): pod counts around the 64-pod word and the
16-word block tile, 1 and 3 slots with sub-ranges, both plane alignments, set plane bits beyond P, all four statuses,
the output inside guard bands, both orientations and that one is the other's bit transpose.  The search on sparse
directed graphs written as planes with the decoys planted (reachgen): a path through every pod across the word
boundaries under every hop bound, random digraphs up to one pod past the 32768 pods a block of the step covers, many
seed sets at once, host outputs between sentinels, each output alone, twice for identical bytes.  Then a source-row
table over all rows, the engine's own tables against the oracle's planes, and arguments and lifetime."""
import ctypes
import json
import os

import numpy as np
import pytest

from cyclonus_amd import _lib
from cyclonus_amd._lib import CyclonusError
from cyclonus_amd.engine import Engine
from cyclonus_amd.probe import PlaneCells, Resources, Table, new_all_available
from oracle.oracle import Oracle, OraclePanic
from planecheck import _Guarded
from randgen import random_problem
from reachgen import NOT_VALID, GraphPlanes, random_digraph
from test_gpu_table_counts import SLOT_RANGES, _bare_engine, _Planes

GOLD = os.path.join(os.path.dirname(__file__), "golden")
pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("gpu")]
DIRECTIONS = ("from", "to")
PAD = 64
FILL = {np.dtype(np.uint64): 0x5A5A5A5A5A5A5A5A, np.dtype(np.int32): 0x5A5A5A5A, np.dtype(np.int64): 0x5A5A5A5A5A5A5A5A}
DTYPES = {"reach": np.uint64, "hops": np.int32, "levels": np.int64}
STEP_BLOCK_PODS = 512 * 64  # the words of a set's bitsets one block of k_reach_step owns, in pods


class _Host:
    """A host output array of `shape` between PAD sentinel elements on either side."""

    def __init__(self, shape, dtype):
        self.shape, self.n, self.fill = shape, int(np.prod(shape)), FILL[np.dtype(dtype)]
        self.buf = np.full(self.n + 2 * PAD, self.fill, dtype)

    @property
    def ptr(self):
        return ctypes.c_void_p(self.buf.ctypes.data + self.buf.itemsize * PAD)

    def take(self, ctx):
        assert (self.buf[:PAD] == self.fill).all() and (self.buf[PAD + self.n:] == self.fill).all(), f"{ctx}: a store outside the output array"
        return self.buf[PAD:PAD + self.n].reshape(self.shape).copy()


def _reach(t, sets, direction="from", k_lo=0, k_hi=None, max_hops=-1, want=("reach", "hops", "levels"), ctx=""):
    """cyc_table_reach with every requested output between sentinels -> the dict DeviceTable.reach returns."""
    k_hi = t.slots if k_hi is None else k_hi
    off, seeds = _lib.seed_arrays(sets)
    n = len(sets)
    shape = {"reach": (n, t.words), "hops": (n, t.pods), "levels": (n,)}
    out = {x: _Host(shape[x], DTYPES[x]) for x in want}
    rc = _lib.lib().cyc_table_reach(t._t, k_lo, k_hi, _lib.REACH_DIRECTIONS[direction], off.ctypes.data, seeds.ctypes.data, n, max_hops,
                                    *(out[x].ptr if x in out else None for x in ("reach", "hops", "levels")))
    if rc != _lib.OK:
        raise CyclonusError(rc, _lib.lib().cyc_table_error(t._t).decode(errors="replace"))
    return {x: o.take(ctx) for x, o in out.items()}


def _same(got, want, ctx):
    assert set(got) <= set(want), ctx
    for n in got:
        assert got[n].dtype == want[n].dtype and got[n].shape == want[n].shape, f"{ctx}: {n} {got[n].dtype} {got[n].shape}"
        bad = np.argwhere(got[n] != want[n])
        assert bad.size == 0, f"{ctx}: {n} differs at {bad[:5].tolist()}: {got[n][tuple(bad[0])]} want {want[n][tuple(bad[0])]}"


def _bit_matrix(plane, P):
    """u64 [P, W] -> bool [P, P]: [r, c] = bit c of row r (asserts that no bit at or beyond P is set)."""
    bits = np.unpackbits(np.ascontiguousarray(plane).view(np.uint8), axis=1, bitorder="little").astype(bool)
    assert not bits[:, P:].any(), "a bit at or beyond P is set"
    return bits[:, :P]


# ---------------------------------------------------------------- 1. the adjacency pass
@pytest.mark.parametrize("K", (1, 3))
@pytest.mark.parametrize("P", (1, 63, 64, 65, 129, 1023, 1024, 1025))
def test_adjacency_of_random_planes(P, K):
    import torch

    eng = _bare_engine(P, K)
    want = {}
    for off in (0, 1):
        a = _Planes(P, K, 500 + P, off)
        assert {0, 1, 2, 3} <= set(a.h_st.reshape(-1).tolist()) or P * K < 16
        t = a.table(eng)
        for k_lo, k_hi in SLOT_RANGES[K]:
            got = {}
            for direction in DIRECTIONS:
                ctx = f"P {P} K {K} slots [{k_lo}, {k_hi}) {direction} plane offset {off}"
                if (k_lo, k_hi, direction) not in want:  # (the planes' contents do not depend on the offset)
                    want[k_lo, k_hi, direction] = a.cells.adjacency(direction, k_lo, k_hi)
                g = _Guarded(P * a.W, off)
                torch.cuda.synchronize()  # (the sentinel fill runs on torch's stream, the call on the table's own)
                assert t.adjacency(direction, k_lo, k_hi, d_out=g.ptr) == g.ptr
                torch.cuda.synchronize()
                assert g.guards_intact(), f"{ctx}: a store outside the adjacency plane (guard band changed)"
                got[direction] = g.plane.cpu().numpy().view(np.uint64).reshape(P, a.W)
                bad = np.argwhere(got[direction] != want[k_lo, k_hi, direction])
                assert bad.size == 0, f"{ctx}: differs at {bad[:5].tolist()}"
            assert np.array_equal(_bit_matrix(got["to"], P), _bit_matrix(got["from"], P).T), f"P {P} K {K} slots [{k_lo}, {k_hi}) offset {off}"
            if k_hi > k_lo and P > 1:
                assert got["from"].any()
        # the Python mirror allocates the plane itself
        own = t.adjacency("to")
        assert own.dtype == torch.int64 and tuple(own.shape) == (P, a.W)
        assert np.array_equal(own.cpu().numpy().view(np.uint64), want[0, K, "to"])


# ---------------------------------------------------------------- 2. the search
def _wrap(g, seed=0, off=0):
    st, ing, eg = g.torch()
    return _Planes(g.P, g.K, seed, off, st, ing, eg)


def test_path_through_every_pod():
    """A Hamiltonian path along a seeded permutation of 130 pods (129 hops, across the word boundaries both ways), its
    edges in slot 0 of 2, the decoys in slot 1 and in the tail bits: hops are the places along the path, under every
    bound."""
    P, K = 130, 2
    order = np.random.default_rng(130).permutation(P)
    g = GraphPlanes(P, K).edge(order[:-1], order[1:], 0)
    g.ingress_only(order[-1], order[0], 0).egress_only(order[-1], order[0], 1)  # the closing edge, one bit per slot
    g.ingress_only(order[5:], order[:-5], 1).egress_only(order[7:], order[:-7], 1)  # shortcuts back, one bit each
    for i, st in enumerate(NOT_VALID):
        g.not_valid(int(order[20 + 40 * i]), 1, st)
    g.tail_bits()
    place = np.empty(P, np.int64)
    place[order] = np.arange(P)
    eng = _bare_engine(P, K)
    for off in (0, 1):
        pl = _wrap(g, 0, off)  # (a wrapped table does not own its planes)
        t = pl.table(eng)
        for max_hops in (0, 1, 64, 128, 129, -1):
            bound = P if max_hops < 0 else max_hops
            for direction, seed, dist in (("from", int(order[0]), place), ("to", int(order[-1]), P - 1 - place)):
                ctx = f"path {direction} max_hops {max_hops} plane offset {off}"
                got = _reach(t, [[seed]], direction, max_hops=max_hops, ctx=ctx)
                assert got["hops"][0].tolist() == np.where(dist <= bound, dist, -1).tolist(), ctx
                assert got["levels"].tolist() == [min(bound, P - 1)], ctx
                _same(got, g.cells().reach([[seed]], direction, max_hops=max_hops), ctx)
        # a seed in the middle, the whole path as seeds, and slot 1 alone (no edge at all)
        mid = int(order[64])
        got = _reach(t, [[mid], order.tolist(), [mid]], "from", 0, 1)
        assert got["levels"].tolist() == [P - 1 - 64, 0, P - 1 - 64] and (got["hops"][1] == 0).all()
        _same(got, g.cells().reach([[mid], order.tolist(), [mid]], "from", 0, 1), "path, three sets")
        assert _reach(t, [[mid]], "from", 1, 2)["hops"][0].tolist() == np.where(np.arange(P) == mid, 0, -1).tolist()


def _seed_sets(P, n, rng):
    """n sets that mix an empty set, all pods, duplicates with the last pod, and single seeds (the last pod among them)."""
    sets = [[int(rng.integers(P))], [], [P - 1, 0, P - 1, P - 1], list(range(P)), [P - 1]]
    sets += [[int(x)] for x in rng.integers(0, P, max(n - len(sets), 0))]
    return sets[:n]


@pytest.mark.parametrize("P,K", ((65, 3), (1025, 3), (STEP_BLOCK_PODS + 1, 1)))
def test_random_digraphs(P, K):
    """Seeded digraphs of mean out-degree 2 with the decoys planted: reach, hops and levels == PlaneCells.reach for 1, 3
    and 65 seed sets, both directions, slot sub-ranges and a hop bound; each output alone; twice for the same bytes."""
    g = random_digraph(P, K, 7000 + P)
    assert {0, 1, 2, 3} <= set(g.status.reshape(-1).tolist())
    cells = g.cells()
    eng = _bare_engine(P, K)
    pl = _wrap(g, 0, 1 if P == 1025 else 0)  # (a wrapped table does not own its planes)
    t = pl.table(eng)
    rng = np.random.default_rng(P)
    for n in (1, 3, 65):
        sets = _seed_sets(P, n, rng)
        for direction in DIRECTIONS:
            for k_lo, k_hi in SLOT_RANGES[K][:3 if n == 3 else 1]:
                for max_hops in (-1, 3) if n == 3 else (-1,):
                    ctx = f"P {P} K {K} sets {n} {direction} slots [{k_lo}, {k_hi}) max_hops {max_hops}"
                    want = cells.reach(sets, direction, k_lo, k_hi, max_hops)
                    if (k_lo, k_hi, max_hops) == (0, K, -1):
                        # not a degenerate input: some set has three hop levels or more, reached pods and unreached ones
                        assert any(len(set(h[h >= 0].tolist())) >= 3 and (h < 0).any() for h in want["hops"]), ctx
                    got = _reach(t, sets, direction, k_lo, k_hi, max_hops, ctx=ctx)
                    _same(got, want, ctx)
                    if n == 3 and max_hops < 0:
                        for x in ("reach", "hops", "levels"):
                            _same(_reach(t, sets, direction, k_lo, k_hi, max_hops, want=(x,), ctx=ctx), {x: want[x]}, f"{ctx}, {x} alone")
                        again = _reach(t, sets, direction, k_lo, k_hi, max_hops, ctx=ctx)
                        assert all(got[x].tobytes() == again[x].tobytes() for x in got), f"{ctx}: two calls differ"
    # the Python mirror
    sets = _seed_sets(P, 3, rng)
    _same(t.reach(sets, "to", max_hops=2), cells.reach(sets, "to", max_hops=2), f"P {P} DeviceTable.reach")
    assert set(t.reach(sets, want=("levels",))) == {"levels"}
    assert t.reach([])["hops"].shape == (0, P)


# ---------------------------------------------------------------- 3. a source-row table over every row
@pytest.mark.parametrize("P", (65, 1025))
def test_source_table_over_all_rows(P):
    K = 3
    g = random_digraph(P, K, 7100 + P)
    pl = _wrap(g)
    eng = _bare_engine(P, K)
    t = pl.table(eng)
    ts = eng.wrap_table(pl.d_in.data_ptr(), pl.d_eg.data_ptr(), pl.d_st.data_ptr(), 0, P, "source")
    assert ts.partition == "source" and (ts.row_lo, ts.row_hi) == (0, P)
    sets = _seed_sets(P, 5, np.random.default_rng(P))
    for direction in DIRECTIONS:
        for k_lo, k_hi in SLOT_RANGES[K]:
            assert np.array_equal(ts.adjacency(direction, k_lo, k_hi).cpu().numpy(), t.adjacency(direction, k_lo, k_hi).cpu().numpy())
            a, b = _reach(ts, sets, direction, k_lo, k_hi), _reach(t, sets, direction, k_lo, k_hi)
            _same(a, b, f"source table P {P} {direction} [{k_lo}, {k_hi})")
    _same(_reach(ts, sets), g.cells().reach(sets), f"source table P {P}")


# ---------------------------------------------------------------- 4. the engine's own tables
def test_engine_tables_equal_the_oracle():
    """Config #1 and random problems (AllAvailable and named-port probes: NO_JOB and both invalid kinds occur): the
    adjacency planes and the search from every pod and from all of them, on the engine's table == on the oracle's planes."""
    c = json.load(open(os.path.join(GOLD, "config1.json")))
    cases = [(c["policies"], c["resources"], c["probes"])] + [random_problem(seed) for seed in range(8000, 8012)]
    eng, n, deepest = Engine(0), 0, 0
    for i, (pols, res, probes) in enumerate(cases):
        try:
            want = PlaneCells(*Oracle(pols, res).probe(probes))
        except OraclePanic:
            continue
        eng.build_policies(pols).load_resources(res)
        eng.prepare(probes)
        t = eng.table()
        P = t.pods
        sets = [[p] for p in range(P)] + [list(range(P)), []]
        for direction in DIRECTIONS:
            assert np.array_equal(t.adjacency(direction).cpu().numpy().view(np.uint64), want.adjacency(direction)), f"case {i} {direction}"
            w = want.reach(sets, direction)
            _same(_reach(t, sets, direction), w, f"case {i} {direction}")
            deepest = max(deepest, int(w["levels"].max()))
        _same(_reach(t, sets, "from", 0, 1, 1), want.reach(sets, "from", 0, 1, 1), f"case {i} slot 0, one hop")
        n += 1
    assert n >= 6 and deepest >= 2
    # config #1 through the probe mirror: Table.reach on the device table == on the oracle's planes
    res, cfg = Resources.from_json(c["resources"]), new_all_available()
    eng.build_policies(c["policies"]).load_resources(c["resources"])
    eng.prepare([cfg.to_json()])
    dt = eng.table()
    st, ing, eg = Oracle(c["policies"], c["resources"]).probe([cfg.to_json()])
    on_dev, on_host = Table(res, cfg, dt, 0, dt.slots), Table(res, cfg, PlaneCells(st, ing, eg), 0, st.shape[1])
    for pod in on_host.items:
        for direction in DIRECTIONS:
            assert on_dev.reach(pod, direction) == on_host.reach(pod, direction)
            assert on_dev.reach(pod, direction, 1) == on_host.reach(pod, direction, 1)


# ---------------------------------------------------------------- 5. what the two calls refuse; lifetime
RP, RK = 65, 3
SLOTS = "slot range out of bounds"
BAD_SLOTS = ((-1, 2), (0, RK + 1), (2, 1))
PARTIAL = "ingress cells need destinations inside the table's rows"
LIMIT = "n_sets * words exceeds the limit of 16777216 (2^24)"
I64, I32 = ctypes.c_int64, ctypes.c_int32


def _err(t):
    return _lib.lib().cyc_table_error(t._t).decode()


def _refused(t, rc, msg):
    assert rc == _lib.ERR_ARG
    assert _err(t) == msg


def test_refusals_and_lifetime():
    import torch

    L = _lib.lib()
    eng = _bare_engine(RP, RK)
    a = _Planes(RP, RK, 21)
    t = a.table(eng)
    keep, shard = a.source_shard(eng, 64, RP)
    p_in, p_eg = a._dev(a.h_in[10:50].contiguous()), a._dev(a.h_eg[10:50].contiguous())
    partial = eng.wrap_table(p_in.data_ptr(), p_eg.data_ptr(), a.d_st.data_ptr(), 10, 50, "target")
    W = a.W
    adj = torch.zeros(RP * W + 1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    d_adj = adj.data_ptr()
    off = (I64 * 4)(0, 2, 2, 4)
    seeds = (I32 * 4)(0, 64, 3, 3)
    reach, hops, levels = np.zeros(3 * W, np.uint64), np.full(3 * RP, 77, np.int32), np.zeros(3, np.int64)
    r, h, lv = (ctypes.c_void_p(x.ctypes.data) for x in (reach, hops, levels))
    call = lambda tt=t, k_lo=0, k_hi=RK, d=0, o=off, s=seeds, n=3, m=-1, out=(r, h, lv): L.cyc_table_reach(tt._t, k_lo, k_hi, d, o, s, n, m, *out)  # noqa: E731
    # ---- the good calls
    assert L.cyc_table_adjacency(t._t, 0, RK, 0, d_adj) == _lib.OK, _err(t)
    assert call() == _lib.OK, _err(t)
    assert call(out=(None, None, lv)) == _lib.OK and call(out=(r, None, None)) == _lib.OK and call(out=(None, h, None)) == _lib.OK
    assert L.cyc_table_adjacency(None, 0, RK, 0, d_adj) == _lib.ERR_ARG and L.cyc_table_reach(None, 0, RK, 0, off, seeds, 3, -1, r, h, lv) == _lib.ERR_ARG
    # ---- cyc_table_adjacency
    for d in (-1, 2):
        _refused(t, L.cyc_table_adjacency(t._t, 0, RK, d, d_adj), "unknown direction")
    for k_lo, k_hi in BAD_SLOTS:
        _refused(t, L.cyc_table_adjacency(t._t, k_lo, k_hi, 0, d_adj), SLOTS)
    _refused(t, L.cyc_table_adjacency(t._t, 0, RK, 0, d_adj + 4), "d_adj is not 8-byte aligned")
    _refused(t, L.cyc_table_adjacency(t._t, 0, RK, 0, None), "null d_adj")
    for other in (partial, shard):
        _refused(other, L.cyc_table_adjacency(other._t, 0, RK, 0, d_adj), PARTIAL)
    assert L.cyc_table_adjacency(t._t, 0, RK, 1, d_adj + 8) == _lib.OK  # (8-byte alignment is enough)
    # ---- cyc_table_reach
    hops[:] = 77
    for d in (-1, 2):
        _refused(t, call(d=d), "unknown direction")
    for k_lo, k_hi in BAD_SLOTS:
        _refused(t, call(k_lo=k_lo, k_hi=k_hi), SLOTS)
    for other in (partial, shard):
        _refused(other, call(tt=other), PARTIAL)
    _refused(t, call(o=None), "null seed_off")
    _refused(t, call(s=None), "null seeds")
    assert call(o=(I64 * 4)(0, 0, 0, 0), s=None, out=(None, None, lv)) == _lib.OK and levels.tolist() == [-1] * 3  # (no set has a seed)
    _refused(t, call(n=-1), "negative n_sets")
    for bad in ((1, 2, 2, 4), (0, 2, 1, 4), (0, 2, 2, 1)):
        _refused(t, call(o=(I64 * 4)(*bad)), "seed_off must start at 0 and never decrease")
    _refused(t, call(s=(I32 * 4)(RP, 64, 3, 3)), f"seeds[0] = {RP} is not a pod in [0, {RP})")
    _refused(t, call(s=(I32 * 4)(0, 64, -1, 70)), f"seeds[2] = -1 is not a pod in [0, {RP})")
    _refused(t, call(s=(I32 * 4)(0, 64, 3, 2**31 - 1)), f"seeds[3] = {2**31 - 1} is not a pod in [0, {RP})")
    _refused(t, call(out=(None, None, None)), "no output requested")
    big = (1 << 24) // W + 1  # (seed_off alone is read: every set empty)
    _refused(t, call(o=(I64 * (big + 1))(), n=big), LIMIT)
    assert (hops == 77).all()  # (a refused call writes nothing)
    assert call(n=0, out=(None, h, None)) == _lib.OK and (hops == 77).all()  # n_sets == 0 writes nothing
    # the Python mirror raises the library's message
    with pytest.raises(CyclonusError, match="unknown direction"):
        t.reach([[0]], 2)
    with pytest.raises(CyclonusError, match=r"seeds\[1\] = 65 is not a pod"):
        t.reach([[0, RP]])
    with pytest.raises(CyclonusError, match="d_adj is not 8-byte aligned"):
        t.adjacency("from", d_out=d_adj + 4)
    # ---- neither call touches the context; both outlive it
    before = _reach(t, [[0], [64, 3]]), t.adjacency("from").cpu().numpy()
    eng.close()
    after = _reach(t, [[0], [64, 3]]), t.adjacency("from").cpu().numpy()
    _same(after[0], before[0], "after cyc_ctx_destroy")
    assert np.array_equal(after[1], before[1])
    _same(after[0], a.cells.reach([[0], [64, 3]]), "after cyc_ctx_destroy, against the restatement")
    del keep
