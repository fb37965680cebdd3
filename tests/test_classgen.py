"""classgen on the CPU, pinned with probe.PlaneCells.classes alone: every decoy splits or does not split as the
definition says, per view and side, and the generated problems have real classes (at least 2 and at most P / 2 on each
side; templates may merge, so the counts are the restatement's, never the number of templates)."""
import numpy as np
import pytest

from classgen import VIEWS, ClassProblem
from cyclonus_amd import _lib

CASES = ((65, 1, 11), (65, 3, 12), (130, 2, 13), (130, 3, 14))


@pytest.mark.parametrize("P,K,seed", CASES)
def test_decoys_and_class_counts(P, K, seed):
    g = ClassProblem(P, K, seed)
    assert set(g.decoys) == {"a", "b", "c", "d", "e", "e_dst", "f", "fe", "g", "h"}
    assert {0, 1, 2, 3} <= set(g.status.reshape(-1).tolist())
    tail = np.uint64((1 << 64) - (1 << (P % 64)))
    assert (g.ingress[:, :, -1] & tail).any() and (g.egress[:, :, -1] & tail).any()
    cells = g.cells()
    for view in VIEWS:
        c = cells.classes(view)
        g.check_decoys(view, c, f"P {P} K {K}")
        for side in ("src", "dst"):
            n = c["n_" + side]
            assert 2 <= n <= P // 2, (view, side, n)
            assert c[side].dtype == np.int32 and c[side][0] == 0 and int(c[side].max()) == n - 1
            # canonical: a class's id is the number of classes that start before its first pod
            first = {}
            for p, x in enumerate(c[side].tolist()):
                first.setdefault(x, p)
            assert sorted(first, key=first.get) == list(range(n))
            # class members are not neighbours (templates that merge under a view may put two side by side)
            assert (c[side][1:] != c[side][:-1]).mean() > 0.5


def test_a_decoy_is_one_planted_difference():
    """Decoy a: the two pods' code rows differ in the cell (., P - 1, K - 1) alone; decoy g: the two destinations'
    statuses differ in one slot alone."""
    g = ClassProblem(130, 3, 14)
    codes = g.cells().cells(0, 130, 0, 130, 0, 3, want=("combined",))["combined"]
    p, q = g.decoys["a"]["pair"]
    assert np.argwhere(codes[p] != codes[q]).tolist() == [[129, 2]]
    p, q = g.decoys["c"]["pair"]
    assert np.argwhere(codes[p] != codes[q]).tolist() == [[p, 1]]
    d1, d2 = g.decoys["g"]["pair"]
    assert np.argwhere(g.status[d1] != g.status[d2]).tolist() == [[1]]
    assert {int(g.status[d1, 1]), int(g.status[d2, 1])} == {_lib.JOB_BAD_NAMED_PORT, _lib.JOB_BAD_PORT_PROTOCOL}
