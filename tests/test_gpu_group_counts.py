"""cyc_table_group_counts / cyc_table_group_compare: counts and comparison per pod-group pair on the device
(k_table_group_tiles, csrc/dev_table.hpp), bit-exact against probe.PlaneCells' per-cell numpy restatement.

Kernel geometry on wrapped random planes (set bits beyond P, both plane alignments, all four statuses) under five
group layouts: one group; contiguous runs whose boundaries fall inside 64-pod words and on them; i % 70, which puts
64 groups into every word and 70 into every block (past the capacity of the block's LDS table: the direct path);
random groups with left-out pods and empty groups; and a boundary on the 16-word block tile.  Host outputs lie
between sentinel elements.  Then a directed transposition test that does not use PlaneCells, source shards, the
engine's tables against the oracle's planes with the namespaces as groups, and arguments and lifetime."""
import json
import os

import numpy as np
import pytest

from cyclonus_amd import _lib
from cyclonus_amd._lib import CyclonusError
from cyclonus_amd.engine import Engine
from cyclonus_amd.probe import PlaneCells, Resources, Table, new_all_available
from cyclonus_amd.shard import source_range
from oracle.oracle import Oracle, OraclePanic
from randgen import random_problem
from test_gpu_table_counts import _bare_engine, _Planes

GOLD = os.path.join(os.path.dirname(__file__), "golden")
pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("gpu")]
VIEWS = ("ingress", "egress", "combined")
PAD, SENTINEL = 64, -0x5A5A5A5A5A5A5A5B
RUNS = (1, 37, 64, 100, 27)
SLOT_RANGES = {1: ((0, 1),), 3: ((0, 3), (1, 2), (2, 3), (1, 1))}


def _layout(name, P):
    """(int32 group id per pod, n_groups)."""
    i = np.arange(P)
    if name == "one":
        return np.zeros(P, np.int32), 1
    if name == "runs":  # runs start at pods 0, 1, 38, 102, 202, 229, 230, ...: runs inside a word and over two and three
        g, at = np.zeros(P, np.int32), 0
        n = 0
        while at < P:
            g[at:at + RUNS[n % len(RUNS)]] = n
            at += RUNS[n % len(RUNS)]
            n += 1
        return g, n
    if name == "mod70":
        return (i % 70).astype(np.int32), 70
    if name == "holes":
        return np.random.default_rng(P).integers(-1, 9, P).astype(np.int32), 12
    if name == "split":
        return (i >= 1024).astype(np.int32), 2
    raise KeyError(name)


class _Out:
    """A host output array of `shape` between PAD sentinel elements on either side."""

    def __init__(self, shape):
        self.shape, self.n = shape, int(np.prod(shape))
        self.buf = np.full(self.n + 2 * PAD, SENTINEL, np.int64)

    @property
    def ptr(self):
        return self.buf.ctypes.data + 8 * PAD

    def take(self, ctx):
        assert (self.buf[:PAD] == SENTINEL).all() and (self.buf[PAD + self.n:] == SENTINEL).all(), f"{ctx}: a store outside the output array"
        return self.buf[PAD:PAD + self.n].reshape(self.shape).copy()


def _check(t, rc):
    if rc != _lib.OK:
        raise CyclonusError(rc, _lib.lib().cyc_table_error(t._t).decode(errors="replace"))


def _group_counts(t, g, G, k_lo, k_hi, ctx):
    """cyc_table_group_counts with every output between sentinels -> the dict DeviceTable.group_counts returns."""
    nk = k_hi - k_lo
    out = {n: _Out((G, G, nk, 6)) for n in VIEWS}
    out["no_job"] = _Out((G, G))
    g = np.ascontiguousarray(g, np.int32)
    _check(t, _lib.lib().cyc_table_group_counts(t._t, g.ctypes.data, G, k_lo, k_hi, *(out[n].ptr for n in VIEWS + ("no_job",))))
    return {n: o.take(ctx) for n, o in out.items()}


def _group_compare(ta, tb, g, G, k_lo, k_hi, loop, ctx):
    out = {"pairs": _Out((G, G, 3)), "slots": _Out((G, G, k_hi - k_lo, 3))}
    g = np.ascontiguousarray(g, np.int32)
    _check(ta, _lib.lib().cyc_table_group_compare(ta._t, tb._t, g.ctypes.data, G, k_lo, k_hi, int(loop), out["pairs"].ptr, out["slots"].ptr))
    return {n: o.take(ctx) for n, o in out.items()}


def _same(got, want, ctx):
    assert set(got) == set(want), ctx
    for n in want:
        bad = np.argwhere(got[n] != want[n])
        assert bad.size == 0, f"{ctx}: {n} differs at {bad[:5].tolist()}: {got[n][tuple(bad[0])]} want {want[n][tuple(bad[0])]}"


def _check_layout(P, K, layout):
    """Both entry points over every slot range of K, both plane alignments and loopback settings, against the cell
    restatement (computed once: the planes' contents do not depend on the alignment)."""
    eng = _bare_engine(P, K)
    g, G = _layout(layout, P)
    want_c, want_p = {}, {}
    for off in (0, 1):
        a, b = _Planes(P, K, 300 + P, off), _Planes(P, K, 400 + P, off)
        assert {0, 1, 2, 3} <= set(a.h_st.reshape(-1).tolist()) or P * K < 16
        ta, tb = a.table(eng), b.table(eng)
        for k_lo, k_hi in SLOT_RANGES[K]:
            ctx = f"P {P} K {K} layout {layout} slots [{k_lo}, {k_hi}) plane offset {off}"
            if (k_lo, k_hi) not in want_c:
                want_c[k_lo, k_hi] = a.cells.group_counts(g, G, k_lo, k_hi)
            got = _group_counts(ta, g, G, k_lo, k_hi, ctx)
            _same(got, want_c[k_lo, k_hi], ctx)
            if (g >= 0).all():
                whole = ta.counts(k_lo, k_hi)
                for n in VIEWS:
                    assert np.array_equal(got[n].sum(axis=(0, 1)), whole[n]), f"{ctx}: {n} does not sum to counts"
                assert int(got["no_job"].sum()) == whole["no_job"], ctx
            for loop in (False, True):
                if (k_lo, k_hi, loop) not in want_p:
                    want_p[k_lo, k_hi, loop] = a.cells.group_compare(b.cells, g, G, k_lo, k_hi, loop)
                got = _group_compare(ta, tb, g, G, k_lo, k_hi, loop, ctx)
                _same(got, want_p[k_lo, k_hi, loop], f"{ctx} loopback {loop}")
                if (g >= 0).all():
                    whole = ta.compare(tb, k_lo, k_hi, loop)
                    assert np.array_equal(got["pairs"].sum(axis=(0, 1)), whole["pairs"]), f"{ctx}: pairs do not sum to compare"
                    assert np.array_equal(got["slots"].sum(axis=(0, 1)), whole["slots"]), f"{ctx}: slots do not sum to compare"
    # the Python mirror returns the same arrays
    _same(ta.group_counts(g, G), want_c[0, K], f"P {P} layout {layout} DeviceTable.group_counts")
    _same(ta.group_compare(tb, g, G, ignore_loopback=True), want_p[0, K, True], f"P {P} layout {layout} DeviceTable.group_compare")


@pytest.mark.parametrize("layout", ("runs", "mod70"))
@pytest.mark.parametrize("P", (1, 63, 64, 65, 129, 1023, 1024, 1025))
def test_one_slot_around_the_word_and_the_block_tile(P, layout):
    _check_layout(P, 1, layout)


@pytest.mark.parametrize("layout", ("one", "runs", "mod70", "holes", "split"))
@pytest.mark.parametrize("P", (65, 1025))
def test_three_slots_and_their_sub_ranges(P, layout):
    _check_layout(P, 3, layout)


@pytest.mark.parametrize("P", (129, 1025))
def test_transposition_by_group(P):
    """ingress = all ones, egress[s][k] = the single bit d = (s * 7 + k) % P (test_gpu_table_counts.test_transposition)
    under the `runs` layout: Combined is allowed for exactly the cells (s, (s * 7 + k) % P, k), so per slot the matrix
    is an np.add.at over P cells; Ingress is allowed everywhere: |gs| * |gd|.  Independent of PlaneCells."""
    import torch

    K, W = 3, (P + 63) // 64
    s, k = np.arange(P)[:, None], np.arange(K)[None, :]
    d = (s * 7 + k) % P
    eg = np.zeros((P, K, W), np.uint64)
    eg[s, k, d // 64] = np.uint64(1) << (d % 64).astype(np.uint64)
    ones = torch.full((P, K, W), -1, dtype=torch.int64)
    valid = torch.full((P, K), _lib.JOB_VALID, dtype=torch.uint8)
    a = _Planes(P, K, 0, 0, valid, ones, torch.from_numpy(eg.view(np.int64)))
    b = _Planes(P, K, 0, 0, valid, ones, torch.zeros((P, K, W), dtype=torch.int64))
    eng = _bare_engine(P, K)
    g, G = _layout("runs", P)
    got = _group_counts(a.table(eng), g, G, 0, K, f"P {P}")
    want = np.zeros((G, G, K), np.int64)
    np.add.at(want, (g[np.broadcast_to(s, d.shape)], g[d], np.broadcast_to(k, d.shape)), 1)
    size = np.bincount(g, minlength=G)
    assert np.array_equal(got["combined"][..., _lib.CONN_ALLOWED], want)
    assert np.array_equal(got["egress"][..., _lib.CONN_ALLOWED], want)
    assert np.array_equal(got["ingress"][..., _lib.CONN_ALLOWED], np.broadcast_to(np.outer(size, size)[:, :, None], (G, G, K)))
    assert np.array_equal(got["combined"][..., _lib.CONN_BLOCKED], np.outer(size, size)[:, :, None] - want)
    assert not got["no_job"].any() and not got["combined"][..., :_lib.CONN_BLOCKED].any()
    # b allows nothing: the `different` jobs are a's allowed cells; a pair differs iff one of its three slots does
    cmp_ = _group_compare(a.table(eng), b.table(eng), g, G, 0, K, False, f"P {P}")
    assert np.array_equal(cmp_["slots"][..., 1], want)
    pair = np.zeros((P, P), bool)
    pair[np.broadcast_to(s, d.shape), d] = True
    want_pairs = np.zeros((G, G), np.int64)
    np.add.at(want_pairs, (g[:, None].repeat(P, 1)[pair], g[None, :].repeat(P, 0)[pair]), 1)
    assert np.array_equal(cmp_["pairs"][..., 1], want_pairs) and np.array_equal(cmp_["pairs"][..., 0], np.outer(size, size) - want_pairs)


@pytest.mark.parametrize("P", (129, 1025))
def test_source_shards_add_up(P):
    K = 3
    eng = _bare_engine(P, K)
    a, b = _Planes(P, K, 500 + P, 1), _Planes(P, K, 600 + P, 1)
    ta, tb = a.table(eng), b.table(eng)
    for layout in ("runs", "holes"):
        g, G = _layout(layout, P)
        whole_c = ta.group_counts(g, G)
        whole_p = {loop: ta.group_compare(tb, g, G, ignore_loopback=loop) for loop in (False, True)}
        _same(whole_c, a.cells.group_counts(g, G), f"P {P} {layout}")
        tot_c, tot_p = None, {False: None, True: None}
        for rank in range(2):
            lo, hi = source_range(P, 2, rank)
            sa, tsa = a.source_shard(eng, lo, hi)
            sb, tsb = b.source_shard(eng, lo, hi)
            c = _group_counts(tsa, g, G, 0, K, f"P {P} {layout} shard {rank}")
            tot_c = c if tot_c is None else {n: tot_c[n] + c[n] for n in c}
            for loop in (False, True):
                p = _group_compare(tsa, tsb, g, G, 0, K, loop, f"P {P} {layout} shard {rank}")
                tot_p[loop] = p if tot_p[loop] is None else {n: tot_p[loop][n] + p[n] for n in p}
        _same(tot_c, whole_c, f"P {P} {layout} source shards")
        for loop in (False, True):
            _same(tot_p[loop], whole_p[loop], f"P {P} {layout} source shards, loopback {loop}")


def _oracle_cells(pols, res, probes):
    try:
        return PlaneCells(*Oracle(pols, res).probe(probes))
    except OraclePanic:
        return None


def test_engine_tables_equal_the_oracle_by_namespace():
    """Config #1 and random problems (AllAvailable and named-port probes: NO_JOB and both invalid kinds occur), the
    namespaces as groups: the engine's tables against the oracle's planes, and Table.namespace_counts both ways."""
    c = json.load(open(os.path.join(GOLD, "config1.json")))
    cases = [(c["policies"], c["policies"][:3], c["resources"], c["probes"])]
    for seed in range(8000, 8040):
        pols, res, probes = random_problem(seed)
        cases.append((pols, random_problem(seed + 500)[0], res, probes))
    need = {_lib.CONN_INVALID_NAMED_PORT, _lib.CONN_INVALID_PORT_PROTOCOL, _lib.CONN_BLOCKED, _lib.CONN_ALLOWED, 255}
    n, codes = 0, set()
    e1, e2 = Engine(0), Engine(0)
    for i, (pols_a, pols_b, res, probes) in enumerate(cases):
        wa, wb = _oracle_cells(pols_a, res, probes), _oracle_cells(pols_b, res, probes)
        if wa is None or wb is None:
            continue
        e1.build_policies(pols_a).load_resources(res)
        e2.build_policies(pols_b).load_resources(res)
        K = e1.prepare(probes)["slots"]
        e2.prepare(probes)
        ta, tb = e1.table(), e2.table()
        r = Resources.from_json(res)
        dev, ora = Table(r, new_all_available(), ta, 0, K), Table(r, new_all_available(), wa, 0, K)
        names, g = dev._namespaces()
        want = wa.group_counts(g, len(names))
        _same(ta.group_counts(g, len(names)), want, f"case {i}")
        codes |= {x for x in range(6) if want["combined"][..., x].sum()} | ({255} if want["no_job"].any() else set())
        for loop in (False, True):
            _same(ta.group_compare(tb, g, len(names), ignore_loopback=loop), wa.group_compare(wb, g, len(names), ignore_loopback=loop),
                  f"case {i} loopback {loop}")
        for view in VIEWS:
            assert dev.namespace_counts(view) == ora.namespace_counts(view), (i, view)
        n += 1
        if n >= 8 and need <= codes:
            break
    assert n >= 8 and need <= codes, (n, codes)


def test_arguments_and_lifetime():
    P, K = 150, 2
    eng = _bare_engine(P, K)
    a, b = _Planes(P, K, 700), _Planes(P, K, 701)
    ta, tb = a.table(eng), b.table(eng)
    g, G = _layout("holes", P)
    want_c, want_p = a.cells.group_counts(g, G), a.cells.group_compare(b.cells, g, G, ignore_loopback=True)
    part = eng.wrap_table(a.d_in.data_ptr(), a.d_eg.data_ptr(), a.d_st.data_ptr(), 0, 64)
    src = eng.wrap_table(a.d_in.data_ptr(), a.d_eg.data_ptr(), a.d_st.data_ptr(), 0, P, "source")
    bad_hi, bad_lo = g.copy(), g.copy()
    bad_hi[7], bad_lo[140] = G, -2
    limit = "n_groups^2 * slots exceeds the limit of 134217728 (2^27)"
    for call, msg in (
            (lambda: part.group_counts(g, G), "ingress cells need destinations inside the table's rows"),
            (lambda: part.group_compare(part, g, G), "ingress cells need destinations inside the table's rows"),
            (lambda: ta.group_counts(bad_hi, G), f"group_of[7] = {G} is neither -1 nor a group in [0, {G})"),
            (lambda: ta.group_compare(tb, bad_lo, G), f"group_of[140] = -2 is neither -1 nor a group in [0, {G})"),
            (lambda: ta.group_counts(np.full(P, -1, np.int32), 0), "n_groups must be at least 1"),
            (lambda: ta.group_compare(tb, np.full(P, -1, np.int32), 0), "n_groups must be at least 1"),
            (lambda: ta.group_counts(g, 11586, 0, 1), limit),  # 11586^2 = 2^27 + 17668
            (lambda: ta.group_counts(g, 8193, 0, 2), limit),   # 8192^2 * 2 = 2^27 would be inside the limit
            (lambda: ta.group_compare(tb, g, 8193), limit),
            (lambda: ta.group_counts(g, G, 0, K + 1), "slot range out of bounds"),
            (lambda: ta.group_compare(tb, g, G, 1, 0), "slot range out of bounds"),
            (lambda: ta.group_counts(g, G, want=()), "no output requested"),
            (lambda: ta.group_compare(src, g, G), "cannot compare tables of different devices, shapes, partitions or rows")):
        with pytest.raises(CyclonusError) as e:
            call()
        assert e.value.code == _lib.ERR_ARG and e.value.msg == msg
    L, gp = _lib.lib(), g.ctypes.data
    out = _Out((G, G, K, 6))
    assert L.cyc_table_group_counts(ta._t, None, G, 0, K, out.ptr, None, None, None) == _lib.ERR_ARG
    assert L.cyc_table_group_compare(ta._t, tb._t, gp, G, 0, K, 0, None, None) == _lib.ERR_ARG
    assert L.cyc_table_group_compare(ta._t, None, gp, G, 0, K, 0, out.ptr, None) == _lib.ERR_ARG
    assert (out.buf == SENTINEL).all()
    # an empty slot range writes zeros
    empty = _group_counts(ta, g, G, 1, 1, "empty slot range")
    assert empty["combined"].shape == (G, G, 0, 6) and not empty["no_job"].any()
    _same(ta.group_counts(g, G, want=("combined",)), {"combined": want_c["combined"]}, "one output")
    eng.close()
    _same(ta.group_counts(g, G), want_c, "after ctx destroy")
    _same(ta.group_compare(tb, g, G, ignore_loopback=True), want_p, "after ctx destroy")
