"""tests/effectcheck.py, the oracle tally cyc_probe_target_effects is checked against (test_gpu_target_effects.py),
pinned on the CPU: its job expansion and Traffic builder against the oracle's own planes, a three-pod case whose
counters are written out, and the entry point's refusals that need no device."""
import ctypes

import numpy as np
import pytest

import effectcheck as ec
from cyclonus_amd import _lib
from cyclonus_amd.engine import Engine
from oracle.oracle import Oracle
from randgen import random_problem


@pytest.mark.parametrize("seed,n_pods", [(1, 9), (2, 17), (3, 12), (6, 20), (11, 14)])
def test_traffic_builder_matches_job_expansion(seed, n_pods):
    """Per VALID cell and direction, IsAllowed of the helper's Traffic equals the bit of Oracle.probe's planes,
    and the helper's job statuses are the oracle's: the helper's cells are the probe's jobs."""
    pols, res, probes = random_problem(seed, n_pods=n_pods, n_pols=10, bad=False)
    o = Oracle(pols, res)
    status, inp, egp = o.probe(probes)
    t = ec.Tally(o, res, probes)
    P, K = status.shape
    assert (t.P, t.K) == (P, K)
    assert (t.status == status).all()
    assert (status == ec.VALID).any()
    # ingress plane [d, k, s/64] bit s%64; egress plane [s, k, d/64] bit d%64 (include/cyclonus_hip.h)
    bits_in = np.unpackbits(inp.view(np.uint8).reshape(P, K, -1), axis=2, bitorder="little")[:, :, :P].astype(bool)
    bits_eg = np.unpackbits(egp.view(np.uint8).reshape(P, K, -1), axis=2, bitorder="little")[:, :, :P].astype(bool)
    valid_in = np.broadcast_to((status == ec.VALID)[:, None, :], (P, P, K))  # [d, s, k]: the destination's job
    valid_eg = np.broadcast_to((status == ec.VALID)[None, :, :], (P, P, K))  # [s, d, k]
    got_in, got_eg = t.allowed[0], t.allowed[1]  # [target pod, other pod, k]
    assert (got_in[valid_in] == bits_in.transpose(0, 2, 1)[valid_in]).all()
    assert (got_eg[valid_eg] == bits_eg.transpose(0, 2, 1)[valid_eg]).all()
    # a direction is allowed iff no target applies or some target allows (policy.go:158-173)
    for dr, valid in ((0, valid_in), (1, valid_eg)):
        assert (t.allowed[dr][valid] == ((t.appliers[dr] == 0) | (t.allowers[dr] > 0))[valid]).all()
        assert not t.appliers[dr][~valid].any()


def _pod(name, app):
    return {"Namespace": "x", "Name": name, "Labels": {"app": app}, "IP": f"10.0.0.{ord(app) - 96}",
            "Containers": [{"Name": "c", "Port": 80, "Protocol": "TCP", "PortName": "serve-80-tcp"}]}


def _pol(name, selector, **spec):
    return {"apiVersion": "networking.k8s.io/v1", "kind": "NetworkPolicy", "metadata": {"name": name, "namespace": "x"},
            "spec": {"podSelector": selector, **spec}}


THREE_PODS = {"Namespaces": {"x": {"ns": "x"}}, "Pods": [_pod("a", "a"), _pod("b", "b"), _pod("c", "c")]}
THREE_PROBES = [{"Port": 80, "Protocol": "TCP"}]
_IN_BC = {"podSelector": {"matchExpressions": [{"key": "app", "operator": "In", "values": ["b", "c"]}]}}
THREE_POLICIES = [
    # T1 applies to a and allows b
    _pol("t1", {"matchLabels": {"app": "a"}}, policyTypes=["Ingress"], ingress=[{"from": [{"podSelector": {"matchLabels": {"app": "b"}}}]}]),
    # T2 applies to a and b and allows b and c
    _pol("t2", {"matchExpressions": [{"key": "app", "operator": "In", "values": ["a", "b"]}]}, policyTypes=["Ingress"],
         ingress=[{"from": [_IN_BC]}]),
    # T3 applies to c and allows nothing
    _pol("t3", {"matchLabels": {"app": "c"}}, policyTypes=["Ingress"], ingress=[]),
    # E1 applies to a and allows b
    _pol("e1", {"matchLabels": {"app": "a"}}, policyTypes=["Egress"], egress=[{"to": [{"podSelector": {"matchLabels": {"app": "b"}}}]}]),
]
# target -> (ALLOWING, DENYING, SOLE_ALLOWING, SOLE_DENYING), applies, over the 3 x 3 cells of the one slot:
#   destination a (T1, T2): from a both deny; from b both allow; from c T1 denies, T2 alone allows
#   destination b (T2):     from a T2 alone denies; from b, c it allows
#   destination c (T3):     T3 alone denies all three
#   source a (E1):          to b it allows; to a, c it alone denies
THREE_WANT = {"T1": ((1, 2, 0, 0), 1), "T2": ((4, 2, 1, 1), 2), "T3": ((0, 3, 0, 3), 1), "E1": ((1, 2, 0, 2), 1)}


def three_pod_targets(keys):
    """Name -> (direction, index) of the case's targets among the primary keys."""
    ing, eg = keys
    assert len(ing) == 3 and len(eg) == 1
    t2 = next(i for i, k in enumerate(ing) if "MatchExpression" in k and "operator" in k)
    t1 = next(i for i, k in enumerate(ing) if i != t2 and "app: a" in k)
    t3 = next(i for i, k in enumerate(ing) if i != t2 and "app: c" in k)
    assert sorted((t1, t2, t3)) == [0, 1, 2]
    return {"T1": (0, t1), "T2": (0, t2), "T3": (0, t3), "E1": (1, 0)}


def test_three_pod_case_counters():
    o = Oracle(THREE_POLICIES, THREE_PODS)
    t = ec.Tally(o, THREE_PODS, THREE_PROBES)
    assert (t.status == ec.VALID).all() and t.K == 1
    for name, (dr, i) in three_pod_targets(t.keys).items():
        eff, app = t.effects(dr)
        assert (tuple(eff[i, 0]), int(app[i])) == THREE_WANT[name], name
    assert t.multi == [1, 0]  # b -> a: T1 and T2 both allow
    # rows add up
    for dr in (0, 1):
        whole = t.effects(dr)
        parts = [t.effects(dr, lo, hi) for lo, hi in ((0, 1), (1, 3))]
        assert (whole[0] == parts[0][0] + parts[1][0]).all() and (whole[1] == parts[0][1] + parts[1][1]).all()


def test_slots_and_statuses_of_every_probe_kind():
    res = {"Namespaces": {}, "Pods": [
        {"Namespace": "x", "Name": "a", "Labels": None, "IP": "10.0.0.1",
         "Containers": [{"Name": "c0", "Port": 80, "Protocol": "TCP", "PortName": "http"},
                        {"Name": "c1", "Port": 53, "Protocol": "UDP", "PortName": "dns"}]},
        {"Namespace": "y", "Name": "b", "Labels": {}, "IP": "10.0.0.2",
         "Containers": [{"Name": "c0", "Port": 81, "Protocol": "TCP", "PortName": "alt"}]}]}
    probes = [{"AllAvailable": True}, {"Port": 80, "Protocol": "UDP"}, {"Port": "alt", "Protocol": "TCP"}]
    assert len(ec.slots(res, probes)) == 4
    assert ec.job(res, probes, 0, 1) == (ec.VALID, 53, "dns", "UDP")
    assert ec.job(res, probes, 1, 1)[0] == ec.NONE
    assert ec.job(res, probes, 0, 2) == (ec.VALID, 80, "http", "UDP")  # the probe's protocol, the container's name
    assert ec.job(res, probes, 1, 2) == (ec.BAD_PORT_PROTOCOL, 80, "", "UDP")
    assert ec.job(res, probes, 0, 3) == (ec.BAD_NAMED_PORT, -1, "alt", "TCP")
    assert ec.job(res, probes, 1, 3) == (ec.VALID, 81, "alt", "TCP")
    assert ec.traffic(res, probes, 0, 1, 2) is None
    tr = ec.traffic(res, probes, 1, 0, 0)
    assert tr["Source"]["Internal"] == {"PodLabels": {}, "NamespaceLabels": None, "Namespace": "y"}
    assert (tr["Destination"]["IP"], tr["ResolvedPort"], tr["ResolvedPortName"], tr["Protocol"]) == ("10.0.0.1", 80, "http", "TCP")
    status, _, _ = Oracle([], res).probe(probes)
    assert (status == np.array([[ec.job(res, probes, d, k)[0] for k in range(4)] for d in range(2)])).all()


def test_refusals_that_need_no_device():
    L = _lib.lib()
    out = (ctypes.c_int64 * 8)()
    assert L.cyc_probe_target_effects(None, 0, 0, 0, 0, 0, out, None) == _lib.ERR_ARG
    e = Engine(0)
    e.build_policies(THREE_POLICIES).load_resources(THREE_PODS)
    assert L.cyc_probe_target_effects(e._ctx, 0, 0, 0, 0, 0, out, None) == _lib.ERR_ARG
    assert b"prepare" in L.cyc_last_error(e._ctx)
    with pytest.raises(_lib.CyclonusError, match="prepare"):
        e.target_effects("ingress")
    assert _lib.DIRECTIONS == {"ingress": 0, "egress": 1}
    assert _lib.EFFECTS == ("allowing", "denying", "sole_allowing", "sole_denying")
