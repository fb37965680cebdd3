"""The template expansion of tests/planegen.py, validated with the oracle alone, for every
(seed, T, P, K, layout) tests/test_gpu_emit_planes.py compares whole device planes with:
(a) the oracle rows of the last pod and of a random middle pod of every template equal its first pod's,
    for every base probe and both directions (and so does their status);
(b) the planes are not trivial, so a wrong row copied into the right place cannot pass: each plane has
    >= T/2 distinct class rows, some template has >= 2 distinct slot rows, and the fraction of set bits
    lies in [0.05, 0.95] — conditions on the inputs: a seed that fails them is replaced (planegen.SEEDS);
(c) at P = 200, K = 9 the expanded planes and status equal Oracle.probe's whole table bit for bit."""
import random

import numpy as np
import pytest

import planegen as pg
from oracle.oracle import Oracle


@pytest.mark.parametrize("case", pg.all_cases(), ids=lambda c: "s{}-T{}-P{}-K{}-{}".format(*c))
def test_template_rows_and_conditions(case):
    seed, T, P, K, layout = case
    prob = pg.template_problem(*case)
    pols, res, probes, tpl_of, base_of = prob
    assert len(res["Pods"]) == P and len(probes) == K and len(tpl_of) == P
    orc = Oracle(pols, res)
    assert orc.shape(probes) == (P, K)  # one slot per PortProtocol config
    status, R_in, R_eg, _, _ = pg.reference_planes(orc, prob)
    assert status.shape == (P, K)
    # (a) any pod of a template has its first pod's rows
    r = random.Random(seed)
    others = []
    for t in range(T):
        members = np.nonzero(tpl_of == t)[0]
        middle = members[1:-1] if len(members) >= 3 else members  # (neither its first nor its last pod)
        others += [int(members[-1]), int(middle[r.randrange(len(middle))])]
    O_in, O_eg, O_st = pg.template_rows(orc, probes, others, base_of)
    for i, pod in enumerate(others):
        t = i // 2
        assert np.array_equal(O_in[i], R_in[t]), f"ingress rows of pod {pod} differ from its template {t}'s first pod"
        assert np.array_equal(O_eg[i], R_eg[t]), f"egress rows of pod {pod} differ from its template {t}'s first pod"
        assert np.array_equal(O_st[i][base_of], status[pod]), f"status of pod {pod} differs from its template {t}'s"
    # (b) non-trivial planes
    count = np.bincount(tpl_of, minlength=T)
    slot_rows = 0
    for name, R in (("ingress", R_in), ("egress", R_eg)):
        rows = R[:, base_of]  # [T, K, W]: a class row per template
        assert len({rows[t].tobytes() for t in range(T)}) * 2 >= T, f"{name}: too few distinct class rows"
        slot_rows = max(slot_rows, max(len({rows[t, k].tobytes() for k in range(K)}) for t in range(T)))
        bits = sum(int(count[t]) * int(np.unpackbits(rows[t].view(np.uint8)).sum()) for t in range(T))
        assert 0.05 <= bits / (float(P) * K * P) <= 0.95, f"{name}: fraction of set bits {bits / (float(P) * K * P)}"
    assert slot_rows >= 2, "no template with two distinct slot rows"
    if layout == "runs":  # <= 4 identity runs in every 64-pod word
        runs = np.concatenate(([1], (np.diff(tpl_of) != 0).astype(np.int64)))
        pad = np.concatenate((runs, np.zeros(-P % 64, np.int64))).reshape(-1, 64)
        starts = pad.sum(1) - pad[:, 0] + 1
        assert starts.max() <= 4, starts.max()


@pytest.mark.parametrize("layout", ["runs", "shuffled"])
@pytest.mark.parametrize("seed", range(3))
def test_expansion_equals_whole_table(seed, layout):
    """(c): the expansion against Oracle.probe's whole table."""
    prob = pg.template_problem(seed, 6, 200, 9, layout)
    pols, res, probes, tpl_of, base_of = prob
    orc = Oracle(pols, res)
    st, ing, eg = orc.probe(probes)
    status, R_in, R_eg, _, _ = pg.reference_planes(orc, prob)
    assert np.array_equal(status, st)
    assert np.array_equal(pg.expand(R_in, tpl_of, base_of), ing)
    assert np.array_equal(pg.expand(R_eg, tpl_of, base_of), eg)
    assert ing.any() and eg.any() and len(set(st.ravel().tolist())) >= 2


def test_layouts_and_addresses():
    """Every template occurs, runs are 22 to 90 pods, addresses are valid and increase with the pod."""
    import ipaddress

    for layout in ("runs", "shuffled"):
        for seed in range(5):
            _, res, _, tpl_of, _ = pg.template_problem(seed, 16, 4000 + seed, 5, layout)
            assert set(tpl_of.tolist()) == set(range(16))
            ips = [int(ipaddress.IPv4Address(p["IP"])) for p in res["Pods"]]
            assert all(b > a for a, b in zip(ips, ips[1:]))
            if layout == "runs":
                edges = np.nonzero(np.diff(tpl_of))[0] + 1
                lens = np.diff(np.concatenate(([0], edges, [len(tpl_of)])))
                assert lens.min() >= 22 and lens.max() <= 90, (lens.min(), lens.max())


def test_shape_tables():
    """The row bytes 8 K ceil(P / 64) of the target shapes, and the ingress slice bytes 8 K wi and egress
    row bytes of the source cases (what decides the emit kernel and the k_emit_units path), written out:
    a shape swapped by mistake fails here."""
    row_bytes = [120, 16632, 176, 16368, 16384, 16384, 17136, 25200, 32768, 32800, 32832, 57344, 57408, 114688, 114704, 124800]
    assert [8 * K * ((P + 63) // 64) for K, P, _, _ in pg.TARGET_SHAPES] == row_bytes
    want = [(7168, 16384), (7200, 15360), (14336, 16384), (14400, 15360), (19200, 57600), (38592, 114704), (16, 176), (24, 192)]
    assert len(want) == len(pg.SOURCE_CASES)
    for (K, P, _, ranks, _), (b_in, b_eg) in zip(pg.SOURCE_CASES, want):
        assert 8 * K * ((P + 63) // 64) == b_eg, (K, P)
        wis = [(hi + 63) // 64 - lo // 64 for lo, hi in ranks]
        assert 8 * K * wis[0] == b_in, (K, P, wis)
        if b_in in (7168, 7200, 14336, 14400, 19200, 16):
            assert len(set(wis)) == 1, (K, P, wis)
        assert all(lo % 64 == 0 and (hi % 64 == 0 or hi == P) for lo, hi in ranks)
        assert ranks[0][0] == 0 and ranks[-1][1] == P and 0 < ranks[1][0] and ranks[1][1] < P
