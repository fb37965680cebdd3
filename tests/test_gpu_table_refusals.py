"""What the table entry points refuse (csrc/table.hpp): for each of the eleven, every bad argument alone, with the
status code and the exact text of cyc_table_error (cyc_table_run_rows / cyc_table_wrap_rows have no table yet: their
text is cyc_last_error's).  One 65-pod, 3-slot table over wrapped random planes, a table of another shape, a partial
target-row table and a source shard; each entry point first answers a good call with the same base arguments."""
import ctypes

import numpy as np
import pytest

from cyclonus_amd import _lib
from cyclonus_amd.engine import Engine
from test_gpu_table_counts import _bare_engine, _Planes

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("gpu")]
P, K = 65, 3
SLOTS = "slot range out of bounds"
BAD_SLOTS = ((-1, 2), (0, K + 1), (2, 1))
PARTIAL = "ingress cells need destinations inside the table's rows"
DIFFERENT = "cannot compare tables of different devices, shapes, partitions or rows"
NO_OUT = "no output requested"
I64 = ctypes.c_int64


class _Env:
    def __init__(self):
        self.eng, self.eng2 = _bare_engine(P, K), _bare_engine(64, K)
        self.a, self.b, self.c = _Planes(P, K, 11), _Planes(P, K, 12), _Planes(64, K, 13)
        self.ta, self.tb, self.other = self.a.table(self.eng), self.b.table(self.eng), self.c.table(self.eng2)
        self.keep = [self.a.source_shard(self.eng, 64, P), self.b.source_shard(self.eng, 64, P)]
        self.shard, self.shard_b = self.keep[0][1], self.keep[1][1]
        self.partial, self.partial_b = self._partial(self.a), self._partial(self.b)
        self.buf = np.zeros(P * P * K * 7 + 64, np.int64)  # any host output fits
        self.out = self.buf.ctypes.data
        self.groups = np.ascontiguousarray(np.arange(P) % 3, np.int32)
        self.g = self.groups.ctypes.data

    def _partial(self, pl, lo=10, hi=50):
        d_in, d_eg = pl._dev(pl.h_in[lo:hi].contiguous()), pl._dev(pl.h_eg[lo:hi].contiguous())
        self.__dict__.setdefault("planes", []).extend((d_in, d_eg))
        return self.eng.wrap_table(d_in.data_ptr(), d_eg.data_ptr(), pl.d_st.data_ptr(), lo, hi, "target")


@pytest.fixture(scope="module")
def env():
    return _Env()


def _err(t):
    return _lib.lib().cyc_table_error(t._t).decode()


def _ok(t, rc):
    assert rc == _lib.OK, _err(t)


def _refused(t, rc, msg):
    assert rc == _lib.ERR_ARG
    assert _err(t) == msg


def test_null_tables(env):
    L, o, n = _lib.lib(), env.out, I64()
    r = ctypes.byref(n)
    assert L.cyc_table_cells(None, 0, 1, 0, 1, 0, 1, o, o, o) == _lib.ERR_ARG
    assert L.cyc_table_counts(None, 0, K, o, o, o, o) == _lib.ERR_ARG
    assert L.cyc_table_pod_counts(None, 0, 0, K, o, o) == _lib.ERR_ARG
    assert L.cyc_table_compare(None, env.tb._t, 0, K, 0, o, None, None, None) == _lib.ERR_ARG
    assert L.cyc_table_pod_compare(None, env.tb._t, 0, K, 0, o, None, None, None) == _lib.ERR_ARG
    assert L.cyc_table_group_counts(None, env.g, 3, 0, K, o, None, None, None) == _lib.ERR_ARG
    assert L.cyc_table_group_compare(None, env.tb._t, env.g, 3, 0, K, 0, o, None) == _lib.ERR_ARG
    assert L.cyc_table_find(None, 0, 1, 0, K, 0, None, 0, r, r, r) == _lib.ERR_ARG
    assert L.cyc_table_compare_find(None, env.tb._t, 0, K, 0, 0, None, 0, r, r, r) == _lib.ERR_ARG
    assert L.cyc_table_error(None) == b"null table"


def test_cells(env):
    L, o, t = _lib.lib(), env.out, env.ta
    _ok(t, L.cyc_table_cells(t._t, 0, P, 0, P, 0, K, o, o, o))
    for s_lo, s_hi, d_lo, d_hi, k_lo, k_hi in ((-1, P, 0, P, 0, K), (0, P + 1, 0, P, 0, K), (2, 1, 0, P, 0, K), (0, P, -1, P, 0, K),
                                               (0, P, 0, P + 1, 0, K), (0, P, 2, 1, 0, K), (0, P, 0, P, -1, K), (0, P, 0, P, 0, K + 1),
                                               (0, P, 0, P, 2, 1)):
        _refused(t, L.cyc_table_cells(t._t, s_lo, s_hi, d_lo, d_hi, k_lo, k_hi, o, o, o), "cell range out of bounds")
    t = env.partial  # rows [10, 50)
    _ok(t, L.cyc_table_cells(t._t, 0, P, 10, 50, 0, K, o, None, None))
    _ok(t, L.cyc_table_cells(t._t, 10, 50, 0, P, 0, K, None, o, None))
    _refused(t, L.cyc_table_cells(t._t, 0, P, 9, 50, 0, K, o, None, None), PARTIAL)
    _refused(t, L.cyc_table_cells(t._t, 0, P, 10, 51, 0, K, o, None, None), PARTIAL)
    _refused(t, L.cyc_table_cells(t._t, 10, 50, 9, 50, 0, K, None, None, o), PARTIAL)
    _refused(t, L.cyc_table_cells(t._t, 9, 50, 0, P, 0, K, None, o, None), "egress cells need sources inside the table's rows")
    _refused(t, L.cyc_table_cells(t._t, 10, 51, 10, 50, 0, K, None, None, o), "egress cells need sources inside the table's rows")
    t = env.shard  # sources [64, 65)
    _ok(t, L.cyc_table_cells(t._t, 64, P, 0, P, 0, K, o, o, o))
    for want in ((o, None, None), (None, o, None), (None, None, o)):
        _refused(t, L.cyc_table_cells(t._t, 63, P, 0, P, 0, K, *want), "cells of a source-row table need sources inside its rows")


def test_counts(env):
    L, o, t = _lib.lib(), env.out, env.ta
    _ok(t, L.cyc_table_counts(t._t, 0, K, o, o, o, o))
    for k_lo, k_hi in BAD_SLOTS:
        _refused(t, L.cyc_table_counts(t._t, k_lo, k_hi, o, o, o, o), SLOTS)
    _refused(t, L.cyc_table_counts(t._t, 0, K, None, None, None, None), NO_OUT)
    t = env.partial
    _ok(t, L.cyc_table_counts(t._t, 0, K, o, o, None, None))
    _refused(t, L.cyc_table_counts(t._t, 0, K, o, o, o, None), PARTIAL)
    _refused(t, L.cyc_table_counts(t._t, 0, K, o, o, None, o), PARTIAL)


def test_pod_counts(env):
    L, o, t = _lib.lib(), env.out, env.ta
    _ok(t, L.cyc_table_pod_counts(t._t, 2, 0, K, o, o))
    for view in (-1, 3):
        _refused(t, L.cyc_table_pod_counts(t._t, view, 0, K, o, o), "unknown view")
    for k_lo, k_hi in BAD_SLOTS:
        _refused(t, L.cyc_table_pod_counts(t._t, 2, k_lo, k_hi, o, o), SLOTS)
    _refused(t, L.cyc_table_pod_counts(t._t, 2, 0, K, None, None), NO_OUT)
    _refused(env.partial, L.cyc_table_pod_counts(env.partial._t, 2, 0, K, o, o), PARTIAL)


def test_compare(env):
    L, o, t, tb = _lib.lib(), env.out, env.ta, env.tb._t
    _ok(t, L.cyc_table_compare(t._t, tb, 0, K, 1, o, o, o, None))
    _refused(t, L.cyc_table_compare(t._t, None, 0, K, 1, o, o, o, None), "null table")
    _refused(t, L.cyc_table_compare(t._t, tb, 0, K, 1, None, o, o, None), "null pair_counts")
    for other in (env.other, env.shard, env.partial):
        _refused(t, L.cyc_table_compare(t._t, other._t, 0, K, 1, o, o, o, None), DIFFERENT)
    for k_lo, k_hi in BAD_SLOTS:
        _refused(t, L.cyc_table_compare(t._t, tb, k_lo, k_hi, 1, o, o, o, None), SLOTS)
    _refused(t, L.cyc_table_compare(t._t, tb, 0, K, 1, o, o, o, ctypes.c_void_p(env.a.d_in.data_ptr() + 4)), "d_diff is not 8-byte aligned")
    _refused(env.partial, L.cyc_table_compare(env.partial._t, env.partial_b._t, 0, K, 1, o, o, o, None), PARTIAL)
    _ok(env.shard, L.cyc_table_compare(env.shard._t, env.shard_b._t, 0, K, 1, o, o, o, None))


def test_pod_compare(env):
    L, o, t, tb = _lib.lib(), env.out, env.ta, env.tb._t
    _ok(t, L.cyc_table_pod_compare(t._t, tb, 0, K, 1, o, o, o, o))
    _refused(t, L.cyc_table_pod_compare(t._t, None, 0, K, 1, o, o, o, o), "null table")
    for other in (env.other, env.shard, env.partial):
        _refused(t, L.cyc_table_pod_compare(t._t, other._t, 0, K, 1, o, o, o, o), DIFFERENT)
    for k_lo, k_hi in BAD_SLOTS:
        _refused(t, L.cyc_table_pod_compare(t._t, tb, k_lo, k_hi, 1, o, o, o, o), SLOTS)
    _refused(t, L.cyc_table_pod_compare(t._t, tb, 0, K, 1, None, None, None, None), NO_OUT)
    _refused(env.partial, L.cyc_table_pod_compare(env.partial._t, env.partial_b._t, 0, K, 1, o, o, o, o), PARTIAL)


def _bad_groups(env, call):
    """The group arguments both group entry points check alike; call(group_of, n_groups, k_lo, k_hi) -> rc."""
    t = env.ta
    _refused(t, call(None, 3, 0, K), "null group_of")
    for k_lo, k_hi in BAD_SLOTS:
        _refused(t, call(env.g, 3, k_lo, k_hi), SLOTS)
    for G in (0, -1):
        _refused(t, call(env.g, G, 0, K), "n_groups must be at least 1")
    for G, k_hi in ((1 << 27) + 1, K), (1 << 40, K), (11586, 1), (8192, K):  # 11586^2 > 2^27 >= 11585^2; 8192^2 * 3 > 2^27
        _refused(t, call(env.g, G, 0, k_hi), "n_groups^2 * slots exceeds the limit of 134217728 (2^27)")
    _refused(t, call(env.g, 2, 0, K), "group_of[2] = 2 is neither -1 nor a group in [0, 2)")
    low = np.ascontiguousarray(np.where(np.arange(P) == 7, -2, 0), np.int32)
    _refused(t, call(low.ctypes.data, 3, 0, K), "group_of[7] = -2 is neither -1 nor a group in [0, 3)")


def test_group_counts(env):
    L, o, t = _lib.lib(), env.out, env.ta
    _ok(t, L.cyc_table_group_counts(t._t, env.g, 3, 0, K, o, o, o, o))
    _bad_groups(env, lambda g, G, k_lo, k_hi: L.cyc_table_group_counts(t._t, g, G, k_lo, k_hi, o, o, o, o))
    _refused(t, L.cyc_table_group_counts(t._t, env.g, 3, 0, K, None, None, None, None), NO_OUT)
    _refused(env.partial, L.cyc_table_group_counts(env.partial._t, env.g, 3, 0, K, o, o, o, o), PARTIAL)


def test_group_compare(env):
    L, o, t, tb = _lib.lib(), env.out, env.ta, env.tb._t
    _ok(t, L.cyc_table_group_compare(t._t, tb, env.g, 3, 0, K, 1, o, o))
    _refused(t, L.cyc_table_group_compare(t._t, None, env.g, 3, 0, K, 1, o, o), "null table")
    _refused(t, L.cyc_table_group_compare(t._t, tb, env.g, 3, 0, K, 1, None, o), NO_OUT)
    for other in (env.other, env.shard, env.partial):
        _refused(t, L.cyc_table_group_compare(t._t, other._t, env.g, 3, 0, K, 1, o, o), DIFFERENT)
    _bad_groups(env, lambda g, G, k_lo, k_hi: L.cyc_table_group_compare(t._t, tb, g, G, k_lo, k_hi, 1, o, o))
    _refused(env.partial, L.cyc_table_group_compare(env.partial._t, env.partial_b._t, env.g, 3, 0, K, 1, o, o), PARTIAL)


def _bad_find(env, call, ta, shard, partial):
    """What table_find checks for both find entry points; call(t, k_lo, k_hi, s_from, cells, cap, n, s_next, total) -> rc."""
    o = env.out
    n, s_next, total = I64(), I64(), I64()
    r = (ctypes.byref(n), ctypes.byref(s_next), ctypes.byref(total))
    _ok(ta, call(ta, 0, K, 0, o, P * P * K, *r))
    assert s_next.value == P and 0 < n.value == total.value
    for i in range(3):
        _refused(ta, call(ta, 0, K, 0, o, P * P * K, *(None if j == i else r[j] for j in range(3))), "null n, s_next or total")
    for k_lo, k_hi in BAD_SLOTS:
        _refused(ta, call(ta, k_lo, k_hi, 0, o, P * P * K, *r), SLOTS)
    _refused(partial, call(partial, 0, K, 10, o, P * P * K, *r), PARTIAL)
    for s_from in (-1, P + 1):
        _refused(ta, call(ta, 0, K, s_from, o, P * P * K, *r), "s_from outside the table's rows")
    _refused(shard, call(shard, 0, K, 63, o, P * P * K, *r), "s_from outside the table's rows")
    _refused(ta, call(ta, 0, K, 0, o, -1, *r), "negative cap")
    _refused(ta, call(ta, 0, K, 0, None, 1, *r), "null cells")
    _ok(ta, call(ta, 0, K, P - 1, None, 0, *r))  # count only, the last source: its matches
    alone = total.value
    assert alone > 1 and (n.value, s_next.value) == (0, P - 1)
    _refused(ta, call(ta, 0, K, P - 1, o, alone - 1, *r), f"source {P - 1} alone has {alone} matching cells, more than cap {alone - 1}")
    assert (n.value, s_next.value, total.value) == (0, P - 1, alone)


def test_find(env):
    L = _lib.lib()
    find = lambda t, k_lo, k_hi, s_from, cells, cap, *r, view=2, mask=0x30: L.cyc_table_find(t._t, view, mask, k_lo, k_hi, s_from, cells, cap, *r)  # noqa: E731
    _bad_find(env, find, env.ta, env.shard, env.partial)
    n = I64()
    r = (ctypes.byref(n),) * 3
    for view in (-1, 3):
        _refused(env.ta, find(env.ta, 0, K, 0, env.out, P * P * K, *r, view=view), "unknown view")
    for mask in (0, 64, 0x130):
        _refused(env.ta, find(env.ta, 0, K, 0, env.out, P * P * K, *r, mask=mask), "code_mask must name codes 0..5")


def test_compare_find(env):
    L = _lib.lib()
    other_of = {env.ta._t.value: env.tb, env.shard._t.value: env.shard_b, env.partial._t.value: env.partial_b}
    find = lambda t, k_lo, k_hi, s_from, cells, cap, *r: L.cyc_table_compare_find(t._t, other_of[t._t.value]._t, k_lo, k_hi, 1, s_from, cells, cap, *r)  # noqa: E731
    _bad_find(env, find, env.ta, env.shard, env.partial)
    n = I64()
    r = (ctypes.byref(n),) * 3
    _refused(env.ta, L.cyc_table_compare_find(env.ta._t, None, 0, K, 1, 0, env.out, P * P * K, *r), "null table")
    for other in (env.other, env.shard, env.partial):
        _refused(env.ta, L.cyc_table_compare_find(env.ta._t, other._t, 0, K, 1, 0, env.out, P * P * K, *r), DIFFERENT)


def _ctx_refused(eng, rc, msg, t):
    assert rc == _lib.ERR_ARG and not t.value
    assert _lib.lib().cyc_last_error(eng._ctx).decode() == msg


ROW_REFUSALS = ((2, 0, P, "unknown partition"), (-1, 0, P, "unknown partition"), (0, -1, P, "row range out of bounds"),
                (0, 0, P + 1, "row range out of bounds"), (0, 2, 1, "row range out of bounds"),
                (1, 1, P, "source rows: row_lo must be a multiple of 64, row_hi too unless it is the pod count"),
                (1, 0, 63, "source rows: row_lo must be a multiple of 64, row_hi too unless it is the pod count"))


def test_run_rows(env):
    L, eng, t = _lib.lib(), env.eng, ctypes.c_void_p()
    for part, lo, hi in ((0, 0, P), (1, 64, P)):
        assert L.cyc_table_run_rows(eng._ctx, part, lo, hi, ctypes.byref(t)) == _lib.OK and t.value
        L.cyc_table_destroy(t)
    assert L.cyc_table_run_rows(None, 0, 0, P, ctypes.byref(t)) == _lib.ERR_ARG
    assert L.cyc_table_run_rows(eng._ctx, 0, 0, P, None) == _lib.ERR_ARG
    for part, lo, hi, msg in ROW_REFUSALS:
        _ctx_refused(eng, L.cyc_table_run_rows(eng._ctx, part, lo, hi, ctypes.byref(t)), msg, t)
    raw = Engine(0)
    _ctx_refused(raw, L.cyc_table_run_rows(raw._ctx, 0, 0, P, ctypes.byref(t)), "cyc_probe_prepare first", t)


def test_wrap_rows(env):
    L, eng, t = _lib.lib(), env.eng, ctypes.c_void_p()
    d_in, d_eg, d_st = env.a.d_in.data_ptr(), env.a.d_eg.data_ptr(), env.a.d_st.data_ptr()
    assert L.cyc_table_wrap_rows(eng._ctx, d_in, d_eg, d_st, 0, 0, P, ctypes.byref(t)) == _lib.OK and t.value
    L.cyc_table_destroy(t)
    assert L.cyc_table_wrap_rows(None, d_in, d_eg, d_st, 0, 0, P, ctypes.byref(t)) == _lib.ERR_ARG
    assert L.cyc_table_wrap_rows(eng._ctx, d_in, d_eg, d_st, 0, 0, P, None) == _lib.ERR_ARG
    for part, lo, hi, msg in ROW_REFUSALS:
        _ctx_refused(eng, L.cyc_table_wrap_rows(eng._ctx, d_in, d_eg, d_st, part, lo, hi, ctypes.byref(t)), msg, t)
    for planes in ((None, d_eg, d_st), (d_in, None, d_st), (d_in, d_eg, None)):
        _ctx_refused(eng, L.cyc_table_wrap_rows(eng._ctx, *planes, 0, 0, P, ctypes.byref(t)), "null plane", t)
    _ctx_refused(eng, L.cyc_table_wrap_rows(eng._ctx, d_in + 4, d_eg, d_st, 0, 0, P, ctypes.byref(t)), "d_ingress is not 8-byte aligned", t)
    _ctx_refused(eng, L.cyc_table_wrap_rows(eng._ctx, d_in, d_eg + 4, d_st, 0, 0, P, ctypes.byref(t)), "d_egress is not 8-byte aligned", t)
    raw = Engine(0)
    _ctx_refused(raw, L.cyc_table_wrap_rows(raw._ctx, d_in, d_eg, d_st, 0, 0, P, ctypes.byref(t)), "cyc_probe_prepare first", t)
