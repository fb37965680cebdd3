"""cyc_table_find / cyc_table_compare_find: the cells behind cyc_table_counts' and cyc_table_compare's numbers,
listed on the device (csrc/dev_table.hpp) in (s, d, k) order, byte for byte against probe.PlaneCells' per-cell
numpy restatement (itself checked against a literal loop in tests/test_table_find.py).

Kernel geometry on wrapped random planes (independent of the engine): pod counts around the 64-pod word, both
sides of the 16-word block tile (1023 / 1024 / 1025 pods) with directed sparse differences, slot sub-ranges,
planes one word off 16-byte alignment, set plane bits beyond P, all four job statuses, the paging contract, and
more slots than the emit kernel keeps in the LDS.  Then consistency with the merged entry points, source shards
and the engine's own tables against the oracle's planes."""
import ctypes
import json
import os

import numpy as np
import pytest

from cyclonus_amd import _lib
from cyclonus_amd._lib import CELL_DTYPE, CyclonusError
from cyclonus_amd.engine import Engine
from cyclonus_amd.probe import PlaneCells
from cyclonus_amd.shard import row_range, source_range
from oracle.oracle import Oracle, OraclePanic
from randgen import random_problem

GOLD = os.path.join(os.path.dirname(__file__), "golden")
pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("gpu")]
VIEWS = ("ingress", "egress", "combined")
ALLOWED, BLOCKED = _lib.CONN_ALLOWED, _lib.CONN_BLOCKED
VALID, NONE, BNP, BPP = _lib.JOB_VALID, _lib.JOB_NONE, _lib.JOB_BAD_NAMED_PORT, _lib.JOB_BAD_PORT_PROTOCOL


def _bare_engine(P, K):
    """A context prepared for P pods and K slots (K numbered probes), without policies."""
    res = {"Namespaces": {"n": {}}, "Pods": [{"Namespace": "n", "Name": f"p{i}", "Labels": {}, "IP": f"10.{i >> 16}.{(i >> 8) & 255}.{i & 255}",
                                             "Containers": [{"Name": "c", "Port": 80, "Protocol": "TCP", "PortName": "w"}]}
                                            for i in range(P)]}
    eng = Engine(0).build_policies([]).load_resources(res)
    sh = eng.prepare([{"Port": 80 + k, "Protocol": "TCP"} for k in range(K)])
    assert (sh["pods"], sh["slots"], sh["words"]) == (P, K, (P + 63) // 64)
    return eng


class _Planes:
    """Host planes (u64 [P, K, W] ingress and egress, u8 [P, K] status) on the device, each plane `off` words
    past a 16-byte boundary, with PlaneCells over the host copies."""

    def __init__(self, status, ingress, egress, off=0):
        import torch

        self.off = off
        self.cells = PlaneCells(status, ingress, egress)
        self.d_in, self.d_eg = self._dev(ingress), self._dev(egress)
        self.d_st = torch.from_numpy(status).cuda()

    def _dev(self, h):
        import torch

        buf = torch.empty(h.size + 2, dtype=torch.int64, device="cuda")
        v = buf[self.off:self.off + h.size]
        assert v.data_ptr() % 16 == 8 * self.off
        v.copy_(torch.from_numpy(np.ascontiguousarray(h).view(np.int64).reshape(-1)))
        return v

    def table(self, eng):
        return eng.wrap_table(self.d_in.data_ptr(), self.d_eg.data_ptr(), self.d_st.data_ptr())


def _random(P, K, seed, off=0):
    """About half the bits set, the bits beyond P too, all four statuses."""
    rng = np.random.default_rng(seed)
    W = (P + 63) // 64
    words = lambda: rng.integers(0, 2**64, (P, K, W), dtype=np.uint64)  # noqa: E731
    return _Planes(rng.integers(0, 4, (P, K)).astype(np.uint8), words(), words(), off)


def _listing(page):
    """page(s_from, cap, out) -> (records, s_next, total): the count-only call, then everything in one page."""
    _, s_next, total = page(None, 0, None)
    recs, s_end, total2 = page(None, max(total, 1), None)
    assert total2 == total == len(recs), (total, total2, len(recs))
    return recs, s_end


def _same(got, want, ctx):
    assert got.dtype == np.dtype(CELL_DTYPE) and want.dtype == got.dtype
    if got.tobytes() != want.tobytes():
        n = min(len(got), len(want))
        bad = np.nonzero(got[:n] != want[:n])[0]
        at = int(bad[0]) if len(bad) else n
        pytest.fail(f"{ctx}: {len(got)} records, want {len(want)}; first difference at {at}: "
                    f"got {got[at:at + 3].tolist()} want {want[at:at + 3].tolist()}")


SLOT_RANGES = {1: ((0, 1),), 3: ((0, 3), (1, 2), (2, 3), (1, 1))}
MASKS = [(c,) for c in range(6)] + [(BLOCKED, ALLOWED)]


@pytest.mark.parametrize("K", (1, 3))
@pytest.mark.parametrize("P", (1, 63, 64, 65, 129))
def test_dense_random_planes(P, K):
    """Every view and mask, compare_find for both loopback settings, both plane alignments, slot sub-ranges; the
    same call twice gives the same bytes."""
    eng = _bare_engine(P, K)
    want = {}
    for off in (0, 1):
        a, b = _random(P, K, 300 + P, off), _random(P, K, 400 + P, off)
        ta, tb = a.table(eng), b.table(eng)
        for k_lo, k_hi in SLOT_RANGES[K]:
            big = P * P * max(k_hi - k_lo, 1)
            for view in VIEWS:
                for codes in MASKS:
                    key = (view, codes, k_lo, k_hi)
                    if key not in want:  # (the planes' contents do not depend on the offset)
                        want[key] = a.cells.find(view, codes, k_lo, k_hi, cap=big)
                    got, s_end = _listing(lambda s, cap, out: ta.find(view, codes, k_lo, k_hi, s, cap, out))
                    _same(got, want[key][0], f"P {P} K {K} {key} offset {off}")
                    assert s_end == P
            for loop in (False, True):
                key = ("compare", loop, k_lo, k_hi)
                if key not in want:
                    want[key] = a.cells.compare_find(b.cells, k_lo, k_hi, loop, cap=big)
                got, s_end = _listing(lambda s, cap, out: ta.compare_find(tb, k_lo, k_hi, loop, s, cap, out))
                _same(got, want[key][0], f"P {P} K {K} {key} offset {off}")
                again, _ = _listing(lambda s, cap, out: ta.compare_find(tb, k_lo, k_hi, loop, s, cap, out))
                assert again.tobytes() == got.tobytes(), "two runs differ"
                assert s_end == P


def test_more_slots_than_the_lds_holds():
    """40 slots: the emit kernel keeps its words in global scratch instead of the LDS."""
    P, K = 70, 40
    eng = _bare_engine(P, K)
    a, b = _random(P, K, 11), _random(P, K, 12)
    ta, tb = a.table(eng), b.table(eng)
    got, _ = _listing(lambda s, cap, out: ta.find("combined", (ALLOWED,), 0, K, s, cap, out))
    _same(got, a.cells.find("combined", (ALLOWED,), cap=P * P * K)[0], "find, 40 slots")
    got, _ = _listing(lambda s, cap, out: ta.compare_find(tb, 3, K, True, s, cap, out))
    _same(got, a.cells.compare_find(b.cells, 3, K, True, cap=P * P * K)[0], "compare_find, 37 slots")


def _directed_cells(P, rng, n_random):
    """(s, d) pairs on the edges of the pod range, of a 64-pod word and of a 16-word block on both axes, a loopback
    cell, and random ones."""
    edge = sorted({0, 1, 62, 63, 64, 65, 1022, 1023, 1024, P - 2, P - 1} & set(range(P)))
    cells = {(s, d) for s in edge for d in (0, 63, 64, 500, 1007, 1008, 1023, 1024, P - 1) if d < P}
    cells |= {(s, d) for d in edge for s in (0, 63, 64, 500, 1007, 1008, 1023, 1024, P - 1) if s < P}
    cells |= {(500, 500), (0, 0), (P - 1, P - 1)}
    cells |= {(int(s), int(d)) for s, d in rng.integers(0, P, (n_random, 2))}
    return sorted(cells)


@pytest.mark.parametrize("P", (1023, 1024, 1025))
def test_both_sides_of_the_block_tile(P):
    """Sparse listings around the 16-word (1024-pod) block tile: table B is table A with about 200 plane bits
    flipped (directed ones on every edge, a loopback cell, flips in only the ingress plane, random ones), one
    status that differs (every source differs there) and one job that B lacks; and find(Combined == allowed) on
    planes that are zero except directed cells."""
    K = 2
    rng = np.random.default_rng(P)
    W = (P + 63) // 64
    eng = _bare_engine(P, K)
    st = np.full((P, K), VALID, np.uint8)
    st[7, 0], st[P - 1, 1], st[64, 1] = BNP, BPP, NONE
    words = lambda: rng.integers(0, 2**64, (P, K, W), dtype=np.uint64)  # noqa: E731
    a = _Planes(st, words(), words(), 1)
    stb = st.copy()
    stb[300, 1], stb[P - 2, 0], stb[7, 0] = BPP, NONE, BPP  # a status that differs, a job B lacks, invalid against invalid
    ing, eg = a.cells.ingress.copy(), a.cells.egress.copy()
    cells = _directed_cells(P, rng, 100)
    for i, (s, d) in enumerate(cells):
        k = i % K
        if i % 3 != 1:
            eg[s, k, d // 64] ^= np.uint64(1) << np.uint64(d % 64)
        if i % 3 != 0:  # (i % 3 == 1: only the ingress plane, so Combined changes only where the egress bit is set)
            ing[d, k, s // 64] ^= np.uint64(1) << np.uint64(s % 64)
    b = _Planes(stb, ing, eg, 1)
    ta, tb = a.table(eng), b.table(eng)
    for loop in (False, True):
        want, s_next, total = a.cells.compare_find(b.cells, 0, K, loop, cap=P * P * K)
        got, s_end = _listing(lambda s, cap, out: ta.compare_find(tb, 0, K, loop, s, cap, out))
        _same(got, want, f"P {P} compare_find loopback {loop}")
        assert s_end == P and 3 * (P - 1) <= len(got) <= 3 * P + 400
        assert int((got["other"] == _lib.CONN_NO_JOB).sum()) == P - loop  # the job B lacks, for every source
    # from the last source on: at 1025 pods pass 1 starts at its second block of 16 source words
    s0 = min(1024, P - 1)
    got, s_next, total = ta.compare_find(tb, 0, K, False, s0, cap=P * K)
    want, _, want_total = a.cells.compare_find(b.cells, 0, K, False, s0, cap=P * K)
    _same(got, want, f"P {P} compare_find from source {s0}")
    assert (s_next, total) == (P, want_total) and (got["s"] >= s0).all() and len(got) >= 3
    # zero planes except directed cells: allowed there and nowhere else
    zi, ze = np.zeros((P, K, W), np.uint64), np.zeros((P, K, W), np.uint64)
    for i, (s, d) in enumerate(cells):
        zi[d, i % K, s // 64] |= np.uint64(1) << np.uint64(s % 64)
        ze[s, i % K, d // 64] |= np.uint64(1) << np.uint64(d % 64)
    z = _Planes(st, zi, ze, 0)
    tz = z.table(eng)
    got, s_end = _listing(lambda s, cap, out: tz.find("combined", (ALLOWED,), 0, K, s, cap, out))
    _same(got, z.cells.find("combined", (ALLOWED,), cap=P * P * K)[0], f"P {P} find allowed")
    valid = [(s, d, i % K) for i, (s, d) in enumerate(cells) if st[d, i % K] == VALID]
    assert sorted(zip(got["s"].tolist(), got["d"].tolist(), got["k"].tolist())) == sorted(valid) and s_end == P
    again, _ = _listing(lambda s, cap, out: tz.find("combined", (ALLOWED,), 0, K, s, cap, out))
    assert again.tobytes() == got.tobytes(), "two runs differ"


def test_paging():
    """cap at the exact size of a prefix of sources, one less, P * nk, and below the first source's count; the pages
    concatenated equal the one-call result; s_next jumps over sources without matches; records beyond n keep the
    sentinel; the count-only call."""
    P, K = 200, 2
    eng = _bare_engine(P, K)
    rng = np.random.default_rng(5)
    W = (P + 63) // 64
    st = np.full((P, K), VALID, np.uint8)
    st[9, 1] = NONE
    ing = np.full((P, K, W), ~np.uint64(0), np.uint64)
    eg = np.zeros((P, K, W), np.uint64)
    busy = sorted({3, 4, 70, 71, 128, 199} | {int(s) for s in rng.integers(0, P, 20)})
    for s in busy:  # sources with 5 to 40 allowed cells; the others have none
        for d in rng.integers(0, P, int(rng.integers(5, 41))):
            eg[s, int(rng.integers(0, K)), d // 64] |= np.uint64(1) << np.uint64(d % 64)
    a = _Planes(st, ing, eg)
    t = a.table(eng)
    want, _, total = a.cells.find("combined", (ALLOWED,), cap=P * P * K)
    per = np.bincount(want["s"], minlength=P)
    starts = np.concatenate([[0], np.cumsum(per)])
    assert [s for s in range(P) if per[s]] == busy and total == len(want)
    find = lambda s, cap, out=None: t.find("combined", (ALLOWED,), 0, K, s, cap, out)  # noqa: E731
    assert find(0, 0)[1:] == (0, total) and len(find(0, 0)[0]) == 0  # count-only
    for i in (1, len(busy) // 2, len(busy) - 1):
        mid, nxt = busy[i], (busy[i + 1] if i + 1 < len(busy) else P)
        out = np.zeros(int(starts[mid + 1]) + 7, CELL_DTYPE)
        out.view(np.uint8)[:] = 0x5A
        # the exact size of the prefix [0, mid]: the page runs on over the sources without matches behind it
        got, s_next, tot = find(0, int(starts[mid + 1]), out)
        assert (s_next, tot, len(got)) == (nxt, total, starts[mid + 1])
        _same(np.array(got), want[:starts[mid + 1]], f"prefix up to {mid}")
        assert (out.view(np.uint8)[16 * len(got):] == 0x5A).all(), "records beyond n were written"
        # one less: the page stops before source mid
        got, s_next, tot = find(0, int(starts[mid + 1]) - 1)
        assert (s_next, tot) == (mid, total)
        _same(got, want[:starts[mid]], f"prefix before {mid}")
        # from the middle of a word on
        got, s_next, tot = find(mid, P * K)
        assert tot == total - starts[mid] and s_next > mid
        _same(got, want[starts[mid]:starts[s_next]], f"from {mid}")
    for cap in (P * K, 41, 64):
        pages = list(t.find_all("combined", (ALLOWED,), cap=cap))
        _same(np.concatenate(pages), want, f"pages of cap {cap}")
        assert all(len(p) <= cap for p in pages) and (cap != 41 or len(pages) > 5)
    first = busy[0]
    with pytest.raises(CyclonusError) as e:
        find(first, int(per[first]) - 1)
    assert e.value.code == _lib.ERR_ARG and e.value.total == total
    assert e.value.msg == f"source {first} alone has {per[first]} matching cells, more than cap {per[first] - 1}"
    assert find(P, 10)[1:] == (P, 0)
    got, s_next, tot = t.find("combined", (ALLOWED,), 1, 1, 0, 10)  # an empty slot range
    assert (len(got), s_next, tot) == (0, P, 0)
    L = _lib.lib()
    n, sn, to = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
    refs = [ctypes.byref(n), ctypes.byref(sn), ctypes.byref(to)]
    buf = np.zeros(4, CELL_DTYPE)
    for args, msg in (((2, 0, 0, K, 0, buf.ctypes.data, 4, *refs), "code_mask must name codes 0..5"),
                      ((2, 64, 0, K, 0, buf.ctypes.data, 4, *refs), "code_mask must name codes 0..5"),
                      ((3, 32, 0, K, 0, buf.ctypes.data, 4, *refs), "unknown view"),
                      ((2, 32, 0, K + 1, 0, buf.ctypes.data, 4, *refs), "slot range out of bounds"),
                      ((2, 32, 1, 0, 0, buf.ctypes.data, 4, *refs), "slot range out of bounds"),
                      ((2, 32, 0, K, P + 1, buf.ctypes.data, 4, *refs), "s_from outside the table's rows"),
                      ((2, 32, 0, K, -1, buf.ctypes.data, 4, *refs), "s_from outside the table's rows"),
                      ((2, 32, 0, K, 0, None, 4, *refs), "null cells"),
                      ((2, 32, 0, K, 0, buf.ctypes.data, -1, *refs), "negative cap"),
                      ((2, 32, 0, K, 0, buf.ctypes.data, 4, None, refs[1], refs[2]), "null n, s_next or total"),
                      ((2, 32, 0, K, 0, buf.ctypes.data, 4, refs[0], None, refs[2]), "null n, s_next or total"),
                      ((2, 32, 0, K, 0, buf.ctypes.data, 4, refs[0], refs[1], None), "null n, s_next or total")):
        assert L.cyc_table_find(t._t, *args) == _lib.ERR_ARG and L.cyc_table_error(t._t).decode() == msg, msg


def test_consistency_with_counts_cells_and_compare():
    """Independent of PlaneCells: total == cyc_table_counts' count of the view and code; total == the sum of
    cyc_table_compare's slot_counts[.][different]; cyc_table_cells of every 97th record's cell returns its codes;
    the (s, d) of the compare_find records are bits of d_diff."""
    P, K = 300, 2
    eng = _bare_engine(P, K)
    a, b = _random(P, K, 21), _random(P, K, 22)
    ta, tb = a.table(eng), b.table(eng)
    counts = ta.counts()
    for view in VIEWS:
        for c in range(6):
            recs, _ = _listing(lambda s, cap, out: ta.find(view, (c,), 0, K, s, cap, out))
            assert len(recs) == counts[view][:, c].sum(), (view, c)
            assert (recs[view] == c).all()
            for r in recs[::97]:
                s, d, k = int(r["s"]), int(r["d"]), int(r["k"])
                cell = ta.cells(s, s + 1, d, d + 1, k, k + 1)
                assert tuple(int(cell[n][0, 0, 0]) for n in VIEWS) == tuple(int(r[n]) for n in VIEWS) and r["other"] == 0
    for loop in (False, True):
        cmp_ = ta.compare(tb, 0, K, loop, want_diff=True)
        recs, _ = _listing(lambda s, cap, out: ta.compare_find(tb, 0, K, loop, s, cap, out))
        assert len(recs) == cmp_["slots"][:, 1].sum()
        diff = cmp_["diff"].cpu().numpy().view(np.uint64)
        s, d = recs["s"].astype(np.int64), recs["d"].astype(np.int64)
        assert ((diff[d, s // 64] >> (s % 64).astype(np.uint64)) & np.uint64(1)).all()
        for r in recs[::97]:
            s, d, k = int(r["s"]), int(r["d"]), int(r["k"])
            assert int(tb.cells(s, s + 1, d, d + 1, k, k + 1, want=("combined",))["combined"][0, 0, 0]) == r["other"] != r["combined"]


def _oracle_cells(pols, res, probes):
    try:
        return PlaneCells(*Oracle(pols, res).probe(probes))
    except OraclePanic:
        return None


def test_source_shards_partial_tables_and_lifetime():
    """A 150-pod problem at worlds 2 and 3: the source shards' listings concatenated in rank order equal the whole
    table's, record for record; a partial target-row table and tables of different shapes are refused; a table
    that outlives its context still answers."""
    pols, res, probes = random_problem(6100, n_pods=150, n_pols=30)
    pols_b = random_problem(6101, n_pods=150, n_pols=30)[0]
    wa, wb = _oracle_cells(pols, res, probes), _oracle_cells(pols_b, res, probes)
    e1 = Engine(0).build_policies(pols).load_resources(res)
    e2 = Engine(0).build_policies(pols_b).load_resources(res)
    sh = e1.prepare(probes)
    e2.prepare(probes)
    P, K = sh["pods"], sh["slots"]
    big = P * P * K
    want_f = wa.find("combined", (BLOCKED,), cap=big)[0]
    want_c = wa.compare_find(wb, ignore_loopback=True, cap=big)[0]
    assert len(want_f) and len(want_c)
    for world in (2, 3):
        got_f, got_c = [], []
        for rank in range(world):
            lo, hi = source_range(P, world, rank)
            ta, tb = e1.table(lo, hi, "source"), e2.table(lo, hi, "source")
            got_f += list(ta.find_all("combined", (BLOCKED,)))
            got_c += list(ta.compare_find_all(tb, ignore_loopback=True))
            recs, s_next, total = ta.find("combined", (BLOCKED,), s_from=hi)
            assert (len(recs), s_next, total) == (0, hi, 0)
            with pytest.raises(CyclonusError) as e:
                ta.find("combined", (BLOCKED,), s_from=lo - 1 if lo else hi + 1)
            assert e.value.msg == "s_from outside the table's rows"
        _same(np.concatenate(got_f), want_f, f"world {world} find")
        _same(np.concatenate(got_c), want_c, f"world {world} compare_find")
        for rank in range(world):  # target-row shards
            lo, hi = row_range(P, world, rank)
            t = e1.table(lo, hi)
            for call in (lambda: t.find("ingress", (ALLOWED,), s_from=lo), lambda: t.compare_find(t, s_from=lo), lambda: t.find("egress", (ALLOWED,), cap=0)):
                with pytest.raises(CyclonusError) as e:
                    call()
                assert e.value.code == _lib.ERR_ARG and e.value.msg == "ingress cells need destinations inside the table's rows"
    whole, other = e1.table(), e2.table()
    with pytest.raises(CyclonusError) as e:
        whole.compare_find(e2.table(0, P, "source"))
    assert e.value.code == _lib.ERR_ARG and e.value.msg == "cannot compare tables of different devices, shapes, partitions or rows"
    e1.close(), e2.close()
    _same(whole.find("combined", (BLOCKED,), cap=big)[0], want_f, "after ctx destroy")
    _same(whole.compare_find(other, ignore_loopback=True, cap=big)[0], want_c, "after ctx destroy")


def test_engine_tables_equal_the_oracle():
    """Config #1 and random problems (AllAvailable and named-port probes: NO_JOB and both invalid kinds occur): find
    for every code of every view == PlaneCells over the oracle's planes; two policy sets compared; a table against
    itself lists nothing and its page runs to row_hi."""
    c = json.load(open(os.path.join(GOLD, "config1.json")))
    cases = [(c["policies"], c["policies"][:3], c["resources"], c["probes"])]
    for seed in range(8000, 8040):
        pols, res, probes = random_problem(seed)
        cases.append((pols, random_problem(seed + 500)[0], res, probes))
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
        P, K = ta.pods, ta.slots
        big = max(P * P * K, 1)
        for view in VIEWS:
            for code in range(6):
                want = wa.find(view, (code,), cap=big)[0]
                _same(ta.find(view, (code,), cap=big)[0], want, f"case {i} {view} {code}")
                if len(want) and view == "combined":
                    codes.add(code)
        if (wa.status == NONE).any():
            codes.add(255)
        for loop in (False, True):
            got, s_next, total = ta.compare_find(tb, ignore_loopback=loop, cap=big)
            _same(got, wa.compare_find(wb, ignore_loopback=loop, cap=big)[0], f"case {i} compare loopback {loop}")
            assert s_next == P and total == len(got)
        me, s_next, total = ta.compare_find(ta, cap=big)
        assert (len(me), s_next, total) == (0, P, 0), i
        n += 1
        if n >= 11:
            break
    assert n >= 11
    assert {_lib.CONN_INVALID_NAMED_PORT, _lib.CONN_INVALID_PORT_PROTOCOL, BLOCKED, ALLOWED, 255} <= codes, codes
