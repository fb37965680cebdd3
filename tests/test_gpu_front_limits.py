"""Whole planes of the front's kernels against the oracle at the sizes where their fixed-size stages fill up.

The class-row, membership and IP-row kernels stage a fixed number of entries in LDS or registers and take a
second code path past it.  tests/limitgen.py builds problems with exactly the counts on either side of each
limit (tests/test_limitgen.py proves the counts, and that every entry decides bits of its own, with the
oracle alone); here whole device planes and the status plane are compared with the template-expanded oracle
rows inside guard bands (tests/planecheck.py), twice per context.

| constant              | kernel                                   | cases                                          |
| PL_LDS 256            | class_rows_pl_blk, pl_items, pl_wave_chunks | m 255 / 256 / 257 / 320 / 321 / 521         |
| 64-entry lane groups  | pl_wave_chunks, the sort of pl_items     | m 63 / 64 / 65                                 |
| PL_BATCH 8            | pl_items' tail batch                     | m 255                                          |
| PL_TGT 64             | class_rows_pl_blk's target chunks        | 63 / 64 / 65 / 130 targets                     |
| CI_LDS 128            | class_ident_blk                          | m 127 / 128 / 129, 3 / 65 / 130 targets        |
| IDO_IPL 16            | class_rows_ido_blk                       | 15 / 16 / 17 / 33 IP peers                     |
| MB 8, 64 per wave     | member_blk, member_wave_blk              | 65 / 130 targets in the namespace              |
| IP_EX_LDS 256         | ip_rows_fast_blk, the items              | 16 IPBlocks with 255 / 256 / 257 excepts       |
| IPB_EX_LDS 192        | k_ip_rows<true>                          | an IPBlock with 191 / 192 / 193 excepts        |
| IPV_MAX 16            | plan.hpp iv_rows, ip_rows_iv_rows        | 15 / 16 / 17 intervals                         |
| IPR_MAX_MATCH 4096    | plan.hpp range_rows, ip_rows_range_blk   | 4095 / 4096 / 4097 matching pods               |
| IPR_SPAN 256          | ... and its LDS window                   | matching pods 254 / 255 / 256 words apart      |

(k_ip_rows<true> takes one IPBlock per block of threads on problems of this size — its batch grows only
with the word count — so the except list that crosses IPB_EX_LDS is one IPBlock's.)
"""
import functools
import json

import pytest

import limitgen as lg
import planegen as pg
from cyclonus_amd.engine import Engine
from oracle.oracle import Oracle
from planecheck import _expected, _run_and_check

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("gpu")]


@functools.lru_cache(maxsize=None)
def _case(key):
    """The problem of a limitgen key and its reference rows, computed once."""
    prob = lg.problem(key)
    pols, res, probes, tpl_of, base_of = prob
    status, R_in, R_eg, _, _ = pg.reference_planes(Oracle(pols, res), prob)
    T, P = int(tpl_of.max()) + 1, len(res["Pods"])
    return {"key": ("-".join(map(str, key)), T, P, len(probes), key[0]), "policies": json.dumps(pols), "resources": json.dumps(res),
            "probes": probes, "tpl_of": tpl_of, "base_of": base_of, "first": pg.first_pods(tpl_of, T), "status": status,
            "R_in": R_in, "R_eg": R_eg}


def _engine(case, may_panic=False):
    eng = Engine(0).build_policies(case["policies"]).load_resources(case["resources"])
    sh = eng.prepare(case["probes"])
    _, _, P, K, _ = case["key"]
    assert (sh["pods"], sh["slots"], sh["words"]) == (P, K, (P + 63) // 64), sh
    assert bool(sh["may_panic"]) == may_panic
    return eng


def _with(eng, case, exp, name, value, default, **kw):
    """A run with one option changed, then the option back at its default."""
    eng.set_option(name, value)
    _run_and_check(eng, case, exp, None, ctx=f"{name} {value}", **kw)
    assert eng.get_option(name) == value
    eng.set_option(name, default)


_ids = lambda cases: ["-".join(map(str, c)) for c in cases]


@pytest.mark.parametrize("shape", lg.PM_CASES, ids=_ids(lg.PM_CASES))
def test_class_lists_four_slots(shape):
    """Materialised class rows of the heavy class with 4 slots and <= 4 descriptors: a wave per 64-word chunk
    with the entries in 64-entry lane groups (pl_wave_chunks), then the batched items (pl_items)."""
    case = _case(lg.pm_key(shape))
    eng = _engine(case)
    exp = _expected(case)
    assert 1 <= eng.shape["descriptors"] <= 4, eng.shape
    assert eng.get_option("pod_words") == 0 and eng.get_option("pl_wave_active") == 1
    _run_and_check(eng, case, exp, None)
    eng.set_option("pl_wave", 0)
    assert eng.get_option("pl_wave_active") == 0
    _run_and_check(eng, case, exp, None, ctx="pl_wave 0")
    eng.close()


@pytest.mark.parametrize("shape", lg.PM_K40, ids=_ids(lg.PM_K40))
def test_class_lists_forty_slots(shape):
    """40 slots of repeated base probes: ingress has no slot bit rows (K > 32) and takes pl_items' general
    loop, which reads the spilled entries; two of the cases under every path option, and as row shards."""
    case = _case(lg.pm_key(shape, 40))
    eng = _engine(case)
    exp = _expected(case)
    assert eng.get_option("pod_words") == 0 and eng.get_option("pl_wave_active") == 0
    _run_and_check(eng, case, exp, None)
    if shape in lg.PM_OPTIONS:
        P = case["key"][2]
        for name, value, default in (("front_fused", 0, 1), ("class_inplace", 0, -1), ("graphs", 1, -1)):
            _with(eng, case, exp, name, value, default)
        lo, hi = 64, min(192, P - 64)  # a middle row range
        _run_and_check(eng, case, exp, None, lo=lo, hi=hi, partition="source")
        _run_and_check(eng, case, exp, None, lo=lo, hi=hi, partition="target")
    eng.close()


@pytest.mark.parametrize("shape", lg.PM_OPTIONS, ids=_ids(lg.PM_OPTIONS))
def test_class_lists_may_panic(shape):
    """The same lists on the ordered walk (k_class_rows, k_ip_rows<true>, k_first_error): a policy with an
    invalid CIDR in a namespace without pods makes a panic possible, and no cell panics."""
    case = _case(lg.pm_key(shape, 40, True))
    eng = _engine(case, may_panic=True)
    _run_and_check(eng, case, _expected(case), None)
    eng.close()


@pytest.mark.parametrize("shape", lg.IDO_CASES, ids=_ids(lg.IDO_CASES))
def test_identity_set_lists(shape):
    """Identity-set class rows (every identity a run of 22 pods): the flat LDS list of class_ident_blk and
    its direct target walk, the staged IP peers of class_rows_ido_blk and the walk past them, one and four
    representatives per block, the DAG's kernels, and both membership kernels."""
    case = _case(lg.ido_key(shape))
    eng = _engine(case)
    exp = _expected(case)
    assert eng.get_option("pod_words") == 1
    _run_and_check(eng, case, exp, None)
    assert eng.get_option("front_fused_active") == 1
    for name, value, default in (("class_rpb", 1, 0), ("class_rpb", 4, 0), ("front_fused", 0, 1), ("member_wave", 0, -1),
                                 ("member_wave", 1, -1)):
        _with(eng, case, exp, name, value, default)
    eng.set_option("front_fused", 0)  # the stand-alone membership kernels
    for value in (0, 1):
        _with(eng, case, exp, "member_wave", value, -1)
    eng.close()


# name -> (options, expected counter, source shard whose word window cuts a block's span)
FAST = {"ip_iv": 0, "ip_range": 0, "ip_items": 0}
IP_RUNS = {
    **{f"fast{n}": (FAST, None, (64, 192)) for n in (255, 256, 257)},
    **{f"batch{n}": ({}, None, (64, 192)) for n in (191, 192, 193)},
    "iv": ({}, ("ip_iv_rows", 2 * lg.IP_IV_ROWS), (64, 192)),
    "match": ({"ip_iv": 0, "ip_range": 1}, ("ip_range_rows", 2 * lg.IP_MATCH_RANGE_ROWS), (1024, 3072)),
    "span": ({"ip_iv": 0, "ip_range": 1}, ("ip_range_rows", 2 * lg.IP_SPAN_RANGE_ROWS), (6400, 16448)),
}


@pytest.mark.parametrize("name", list(lg.IP_CASES))
def test_ip_rows(name):
    """IP rows: the fast groups' and the panic path's staged except lists, and the interval- and range-built
    rows at the limits of what the plan builds that way (the plan's own counts asserted)."""
    opts, counter, (lo, hi) = IP_RUNS[name]
    case = _case(lg.ip_key(name))
    eng = _engine(case, may_panic=bool(lg.IP_CASES[name].get("decoy")))
    exp = _expected(case)
    for k, v in opts.items():
        eng.set_option(k, v)
    _run_and_check(eng, case, exp, None, ctx=str(opts))
    if counter:
        assert eng.get_option(counter[0]) == counter[1], (counter, eng.get_option(counter[0]))
    if "ip_items" in opts:
        eng.set_option("ip_items", -1)
        _run_and_check(eng, case, exp, None, ctx="ip_items auto")
    _run_and_check(eng, case, exp, None, lo=lo, hi=hi, partition="source", ctx=str(opts))
    if counter:
        assert eng.get_option(counter[0]) == counter[1], (counter, eng.get_option(counter[0]))
    eng.close()
