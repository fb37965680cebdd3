"""Whole device planes against template-expanded oracle rows, inside guard bands: the helpers of
tests/test_gpu_emit_planes.py and tests/test_gpu_front_limits.py.

A case is a dict: "key" (a 5-tuple with P and K at [2] and [3]), "tpl_of", "base_of", "first" (the first pod
of every template), and the reference rows "R_in", "R_eg" [T, B, W] u64 and "status" [P, K] u8 of
planegen.reference_planes."""
import numpy as np
import pytest

G = 4096  # guard words on either side of a plane (guard bytes of the status plane)
SENTINEL = 0x5A5A5A5A5A5A5A5A


def _expected(case):
    """(ingress[P,K,W], egress[P,K,W], status[P,K]) on the device: plane[p, k] = R[tpl_of[p], base_of[k]]."""
    import torch

    tpl = torch.as_tensor(case["tpl_of"], device="cuda")
    base = torch.as_tensor(case["base_of"], device="cuda")
    planes = [torch.from_numpy(case[n].view(np.int64)).cuda()[:, base][tpl].contiguous() for n in ("R_in", "R_eg")]
    return planes[0], planes[1], torch.from_numpy(case["status"]).cuda()


class _Guarded:
    """A plane of n elements inside a larger sentinel-filled buffer: G guard elements, `off` more
    (the plane's offset from the allocation's alignment), the plane, G guard elements."""

    def __init__(self, n, off=0, dtype=None):
        import torch

        self.dtype = dtype or torch.int64
        self.fill = SENTINEL if self.dtype == torch.int64 else 0x5A
        self.lo, self.n = G + off, n
        self.buf = torch.empty(self.lo + n + G, dtype=self.dtype, device="cuda")
        assert self.buf.data_ptr() % 128 == 0
        self.refill()

    def refill(self):
        self.buf.fill_(self.fill)

    @property
    def ptr(self):
        return self.buf.data_ptr() + self.buf.element_size() * self.lo

    @property
    def plane(self):
        return self.buf[self.lo:self.lo + self.n]

    def guards_intact(self):
        return bool((self.buf[:self.lo] == self.fill).all()) and bool((self.buf[self.lo + self.n:] == self.fill).all())

    def untouched(self):
        return bool((self.buf == self.fill).all())


def _mismatch(case, name, got, want, row_lo):
    """The first five differing (row, slot, word) triples, each with the pod's template and whether
    the row is the first pod of its template (an in-place class row)."""
    bad = (got != want).nonzero()
    out = [f"{name} plane: {bad.shape[0]} of {want.numel()} words differ"]
    for r, k, w in bad[:5].tolist():
        pod = r + row_lo
        t = int(case["tpl_of"][pod])
        out.append(f"  (row {r} = pod {pod}, slot {k}, word {w}): got {int(got[r, k, w]) & (2**64 - 1):#018x} want "
                   f"{int(want[r, k, w]) & (2**64 - 1):#018x}; template {t}, "
                   f"{'the first pod of its template' if int(case['first'][t]) == pod else 'not its first pod'}")
    return "\n".join(out)


def _run_and_check(eng, case, exp, emit, off=(0, 0), lo=0, hi=None, partition="target", reps=2, ctx=""):
    """Run rows [lo, hi) into guarded planes `off` words past the allocation's alignment, `reps` times on
    this context, and compare guard bands, both planes, the status plane and the emit with the reference
    (emit None: whichever emit kernel the run chose)."""
    import torch

    _, _, P, K, _ = case["key"]
    hi = P if hi is None else hi
    ri, wi, re_, we, w0 = eng.layout(lo, hi, partition)
    exp_in, exp_eg, exp_st = exp
    if partition == "source":
        want_in, lo_in = exp_in[:, :, w0:w0 + wi], 0  # every destination's words of the shard
    else:
        want_in, lo_in = exp_in[lo:hi], lo
    want_eg = exp_eg[lo:hi]
    assert tuple(want_in.shape) == (ri, K, wi) and tuple(want_eg.shape) == (re_, K, we)
    g_in, g_eg = _Guarded(ri * K * wi, off[0]), _Guarded(re_ * K * we, off[1])
    g_st = _Guarded(P * K, 0, torch.uint8)
    for rep in range(reps):
        where = f"{case['key']} {partition} rows [{lo}, {hi}) offsets {off} {ctx} run {rep}"
        if rep:
            for g in (g_in, g_eg, g_st):
                g.refill()
        eng.run_device(g_in.ptr, g_eg.ptr, g_st.ptr, torch.cuda.current_stream().cuda_stream, lo, hi, partition)
        torch.cuda.synchronize()
        assert emit is None or eng.last_emit() == emit, f"{where}: emit {eng.last_emit()}, expected {emit}"
        for name, g in (("ingress", g_in), ("egress", g_eg), ("status", g_st)):
            assert g.guards_intact(), f"{where}: a store outside the {name} plane (guard band changed)"
        for name, g, want, row_lo in (("ingress", g_in, want_in, lo_in), ("egress", g_eg, want_eg, lo)):
            got = g.plane.view(want.shape)
            if not torch.equal(got, want):
                pytest.fail(f"{where}\n" + _mismatch(case, name, got, want, row_lo))
        got_st = g_st.plane.view(P, K)
        if not torch.equal(got_st, exp_st):
            bad = (got_st != exp_st).nonzero()
            pytest.fail(f"{where}: status plane: {bad.shape[0]} cells differ, first (pod, slot) {bad[:5].tolist()}")
