"""cyc_table_counts / cyc_table_compare: the whole-table verdict counts and the table comparison computed on the
device (csrc/dev_table.hpp), bit-exact against probe.PlaneCells' per-cell numpy restatement.

Kernel geometry is checked on wrapped random planes (independent of the engine): pod counts around the 64-pod
word and around the tile kernel's block tile of 16 words (1023 / 1024 / 1025 pods), 1 and 3 slots with
sub-ranges, planes one word off 16-byte alignment, set plane bits beyond P, all four job statuses, and d_diff
inside sentinel guard bands.  Then the engine's tables against the oracle's planes, and row shards."""
import json
import os

import numpy as np
import pytest

from cyclonus_amd import _lib
from cyclonus_amd._lib import CyclonusError
from cyclonus_amd.engine import Engine
from cyclonus_amd.probe import PlaneCells
from cyclonus_amd.shard import row_range, source_range
from oracle.oracle import Oracle, OraclePanic
from planecheck import _Guarded
from randgen import random_problem

GOLD = os.path.join(os.path.dirname(__file__), "golden")
pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("gpu")]


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
    """Random planes (about half the bits set, the bits beyond P too) and statuses on the device, each
    plane `off` words past a 16-byte boundary, with their host copies as PlaneCells."""

    def __init__(self, P, K, seed, off=0, status=None, ingress=None, egress=None):
        import torch

        g = torch.Generator(device="cpu").manual_seed(seed)
        W = (P + 63) // 64
        rnd = lambda: torch.randint(-2**63, 2**63 - 1, (P, K, W), dtype=torch.int64, generator=g)  # noqa: E731
        self.h_in = rnd() if ingress is None else ingress
        self.h_eg = rnd() if egress is None else egress
        self.h_st = torch.randint(0, 4, (P, K), dtype=torch.uint8, generator=g) if status is None else status
        self.P, self.K, self.W, self.off = P, K, W, off
        self.d_in, self.d_eg = self._dev(self.h_in), self._dev(self.h_eg)
        self.d_st = self.h_st.cuda()
        self.cells = PlaneCells(self.h_st.numpy(), self.h_in.numpy().view(np.uint64), self.h_eg.numpy().view(np.uint64))

    def _dev(self, h):
        import torch

        buf = torch.empty(h.numel() + 2, dtype=torch.int64, device="cuda")
        v = buf[self.off:self.off + h.numel()]
        assert v.data_ptr() % 16 == 8 * self.off
        v.copy_(h.reshape(-1))
        return v

    def table(self, eng):
        return eng.wrap_table(self.d_in.data_ptr(), self.d_eg.data_ptr(), self.d_st.data_ptr())

    def source_shard(self, eng, lo, hi):
        """The source-row planes of sources [lo, hi): every destination's ingress words of the shard, the
        shard's egress rows."""
        w0, w1 = lo // 64, (hi + 63) // 64
        sh = _Planes.__new__(_Planes)
        sh.off = self.off
        sh.d_in, sh.d_eg, sh.d_st = sh._dev(self.h_in[:, :, w0:w1].contiguous()), sh._dev(self.h_eg[lo:hi].contiguous()), self.d_st
        sh.keep = self
        return sh, eng.wrap_table(sh.d_in.data_ptr(), sh.d_eg.data_ptr(), sh.d_st.data_ptr(), lo, hi, "source")


def _same_counts(got, want, ctx):
    for n in want:
        assert np.array_equal(got[n], want[n]), f"{ctx}: {n} counts {np.asarray(got[n]).tolist()} want {np.asarray(want[n]).tolist()}"


def _same_compare(got, want, ctx):
    for n in ("pairs", "slots", "dst"):
        bad = np.argwhere(got[n] != want[n])
        assert bad.size == 0, f"{ctx}: {n} differs at {bad[:5].tolist()}: {got[n][tuple(bad[0])]} want {want[n][tuple(bad[0])]}"


def _compare_guarded(ta, tb, k_lo, k_hi, loop, shape, off):
    """compare with d_diff inside guard bands, `off` words past a 16-byte boundary -> (result, diff u64 array)."""
    import torch

    g = _Guarded(shape[0] * shape[1], off)
    got = ta.compare(tb, k_lo, k_hi, loop, d_diff=g.ptr if g.n else None)
    torch.cuda.synchronize()
    assert g.guards_intact(), "a store outside the d_diff plane (guard band changed)"
    return got, g.plane.cpu().numpy().view(np.uint64).reshape(shape)


SLOT_RANGES = {1: ((0, 1),), 3: ((0, 3), (1, 2), (2, 3), (1, 1))}


@pytest.mark.parametrize("K", (1, 3))
@pytest.mark.parametrize("P", (1, 63, 64, 65, 129, 1023, 1024, 1025))
def test_random_planes_equal_the_cell_restatement(P, K):
    """Wrapped random planes and statuses: counts, compare (pairs, slots, dst, d_diff) == PlaneCells, for both
    plane alignments and loopback settings; the shards of a source partition add up to the whole table."""
    eng = _bare_engine(P, K)
    want_counts, want_cmp = {}, {}
    for off in (0, 1):
        a, b = _Planes(P, K, 100 + P, off), _Planes(P, K, 200 + P, off)
        ta, tb = a.table(eng), b.table(eng)
        for k_lo, k_hi in SLOT_RANGES[K]:
            ctx = f"P {P} K {K} slots [{k_lo}, {k_hi}) plane offset {off}"
            if (k_lo, k_hi) not in want_counts:  # (the planes' contents do not depend on the offset)
                want_counts[k_lo, k_hi] = a.cells.counts(k_lo, k_hi)
            _same_counts(ta.counts(k_lo, k_hi), want_counts[k_lo, k_hi], ctx)
            for loop in (False, True):
                if (k_lo, k_hi, loop) not in want_cmp:
                    want_cmp[k_lo, k_hi, loop] = a.cells.compare(b.cells, k_lo, k_hi, loop, want_diff=True)
                want = want_cmp[k_lo, k_hi, loop]
                got, diff = _compare_guarded(ta, tb, k_lo, k_hi, loop, (P, a.W), off)
                _same_compare(got, want, f"{ctx} loopback {loop}")
                assert np.array_equal(diff, want["diff"]), f"{ctx}: d_diff differs at {np.argwhere(diff != want['diff'])[:5].tolist()}"
        if P >= 129:  # source shards: an ingress window that starts past word 0
            for loop in (False, True):
                tot_c, tot_p = None, None
                for rank in range(2):
                    lo, hi = source_range(P, 2, rank)
                    sa, tsa = a.source_shard(eng, lo, hi)
                    sb, tsb = b.source_shard(eng, lo, hi)
                    c = tsa.counts(0, K)
                    got, diff = _compare_guarded(tsa, tsb, 0, K, loop, (P, tsa.window[1]), off)
                    w0 = tsa.window[0]
                    assert np.array_equal(diff, want_cmp[0, K, loop]["diff"][:, w0:w0 + tsa.window[1]]), (P, K, rank, "shard d_diff")
                    tot_c = c if tot_c is None else {n: tot_c[n] + c[n] for n in c}
                    tot_p = got if tot_p is None else {n: tot_p[n] + got[n] for n in got}
                _same_counts(tot_c, want_counts[0, K], f"P {P} K {K} source shards, offset {off}")
                _same_compare(tot_p, want_cmp[0, K, loop], f"P {P} K {K} source shards, offset {off}, loopback {loop}")


@pytest.mark.parametrize("P", (129, 1025))
def test_transposition(P):
    """ingress = all ones, egress[s][k] = the single bit d = (s * 7 + k) % P: Combined is allowed for exactly P
    cells per slot, one source on each destination (7 is coprime to both pod counts).  An error in any stage of
    the bit transpose moves or loses bits."""
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
    ta, tb = a.table(eng), b.table(eng)
    c = ta.counts()
    assert c["combined"][:, _lib.CONN_ALLOWED].tolist() == [P] * K and c["combined"][:, _lib.CONN_BLOCKED].tolist() == [P * P - P] * K
    assert c["egress"][:, _lib.CONN_ALLOWED].tolist() == [P] * K and c["ingress"][:, _lib.CONN_ALLOWED].tolist() == [P * P] * K
    got = ta.compare(tb, 0, K, False, want_diff=True)  # b allows nothing: `different` are a's allowed cells
    assert (got["dst"][:, :, 1] == 1).all() and (got["dst"][:, :, 0] == P - 1).all()
    diff = got["diff"].cpu().numpy().view(np.uint64)
    want = np.zeros((P, W), np.uint64)
    np.bitwise_or.at(want, (d, np.broadcast_to(s // 64, d.shape)), np.broadcast_to(np.uint64(1) << (s % 64).astype(np.uint64), d.shape))
    assert np.array_equal(diff, want)
    _same_counts(c, a.cells.counts(), "transposition planes")


def _oracle_cells(pols, res, probes):
    try:
        return PlaneCells(*Oracle(pols, res).probe(probes))
    except OraclePanic:
        return None


def test_engine_tables_equal_the_oracle():
    """Config #1 and random problems (AllAvailable and named-port probes: NO_JOB and both invalid kinds occur):
    counts of the engine's table == counts of the oracle's planes; compare of two policy sets over the same
    resources == PlaneCells.compare; a table against itself has no `different` and an all-zero d_diff."""
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
        want = wa.counts()
        _same_counts(ta.counts(), want, f"case {i}")
        codes |= {x for x in range(6) if want["combined"][:, x].sum()} | ({255} if want["no_job"] else set())
        for loop in (False, True):
            got = ta.compare(tb, ignore_loopback=loop, want_diff=True)
            w = wa.compare(wb, ignore_loopback=loop, want_diff=True)
            _same_compare(got, w, f"case {i} loopback {loop}")
            assert np.array_equal(got["diff"].cpu().numpy().view(np.uint64), w["diff"]), i
        me = ta.compare(ta, ignore_loopback=False, want_diff=True)
        assert me["pairs"][1] == 0 and not me["slots"][:, 1].any() and not me["diff"].any().item(), i
        n += 1
        if n >= 21:
            break
    assert n >= 21
    assert {_lib.CONN_INVALID_NAMED_PORT, _lib.CONN_INVALID_PORT_PROTOCOL, _lib.CONN_BLOCKED, _lib.CONN_ALLOWED, 255} <= codes, codes


def test_shards_partial_tables_and_lifetime():
    """A 150-pod problem: every CYC_ROWS_SOURCE shard's counts and compare results sum to the whole table's; a
    partial target-row table counts Ingress over its destinations and Egress over its sources and refuses Combined
    and compare; bad arguments are CYC_ERR_ARG; a table outliving its context still answers."""
    pols, res, probes = random_problem(6100, n_pods=150, n_pols=30)
    pols_b = random_problem(6101, n_pods=150, n_pols=30)[0]
    wa, wb = _oracle_cells(pols, res, probes), _oracle_cells(pols_b, res, probes)
    e1 = Engine(0).build_policies(pols).load_resources(res)
    e2 = Engine(0).build_policies(pols_b).load_resources(res)
    sh = e1.prepare(probes)
    e2.prepare(probes)
    P, K = sh["pods"], sh["slots"]
    want_c = wa.counts()
    want_p = {loop: wa.compare(wb, ignore_loopback=loop) for loop in (False, True)}
    for world in (2, 3):
        tot_c, tot_p = None, {False: None, True: None}
        for rank in range(world):
            lo, hi = source_range(P, world, rank)
            ta, tb = e1.table(lo, hi, "source"), e2.table(lo, hi, "source")
            c = ta.counts()
            tot_c = c if tot_c is None else {n: tot_c[n] + c[n] for n in c}
            for loop in (False, True):
                g = ta.compare(tb, ignore_loopback=loop)
                tot_p[loop] = g if tot_p[loop] is None else {n: tot_p[loop][n] + g[n] for n in g}
        _same_counts(tot_c, want_c, f"world {world}")
        for loop in (False, True):
            _same_compare(tot_p[loop], want_p[loop], f"world {world} loopback {loop}")
        for rank in range(world):  # target-row shards
            lo, hi = row_range(P, world, rank)
            t = e1.table(lo, hi)
            got = t.counts(want=("ingress", "egress"))
            ci = wa.cells(0, P, lo, hi, 0, K, want=("ingress",))["ingress"]
            ce = wa.cells(lo, hi, 0, P, 0, K, want=("egress",))["egress"]
            for x in range(6):
                assert np.array_equal(got["ingress"][:, x], (ci == x).sum(axis=(0, 1))), (world, rank, "ingress", x)
                assert np.array_equal(got["egress"][:, x], (ce == x).sum(axis=(0, 1))), (world, rank, "egress", x)
            for call in (lambda: t.counts(), lambda: t.counts(want=("combined",)), lambda: t.counts(want=("no_job",)),
                         lambda: t.compare(t)):
                with pytest.raises(CyclonusError) as e:
                    call()
                assert e.value.code == _lib.ERR_ARG and e.value.msg == "ingress cells need destinations inside the table's rows"
    whole, other = e1.table(), e2.table()
    for call, msg in ((lambda: whole.counts(0, K + 1), "slot range out of bounds"), (lambda: whole.counts(want=()), "no output requested"),
                      (lambda: whole.compare(other, d_diff=12), "d_diff is not 8-byte aligned"),
                      (lambda: whole.compare(e2.table(0, P, "source")), "cannot compare tables of different devices, shapes, partitions or rows")):
        with pytest.raises(CyclonusError) as e:
            call()
        assert e.value.code == _lib.ERR_ARG and e.value.msg == msg
    assert _lib.lib().cyc_table_compare(whole._t, other._t, 0, K, 0, None, None, None, None) == _lib.ERR_ARG
    e1.close(), e2.close()
    _same_counts(whole.counts(), want_c, "after ctx destroy")
    _same_compare(whole.compare(other, ignore_loopback=True), want_p[True], "after ctx destroy")
