"""cyc_probe_target_effects on the synth configs, next to the same process's cyc_probe_run step.

    python scripts/target_effects_bench.py [configs=config2,config3,config4] [reps=3] [steps=5] [out=FILE]

Per config, in one process: prepare (flat tables), `steps` table steps into device planes (the min of their
times between two events on the stream), then per direction the min over `reps` of the synchronous call over the whole
table (every row, every slot), with how the call was batched and the device scratch it held at its peak
(cyc_get_option "effects_batches", "effects_launches", "effects_scratch_bytes"), and the ratio of the call to the
table step.  The box's fill figure, as bench.py measures it, is printed with the numbers.  With CYC_TRACE_PREPARE=1
the library prints each call's host phases and kernel times on stderr (the kernels are then synchronised one by
one, so the totals are a little higher).
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from cyclonus_amd import synth
from cyclonus_amd.engine import Engine
from cyclonus_amd.flat import prepare_flat

kw = dict(a.split("=") for a in sys.argv[1:] if "=" in a)
configs = kw.get("configs", "config2,config3,config4").split(",")
reps, steps = int(kw.get("reps", 3)), int(kw.get("steps", 5))


def fill_gbs(nbytes):
    """The box's fill figure (bench.py's write ceiling): torch's fill kernel over `nbytes`, twice."""
    scratch = torch.empty(nbytes // 8, dtype=torch.int64, device="cuda")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for _ in range(3):
        e0.record()
        scratch.fill_(0)
        scratch.fill_(0)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return 2 * scratch.numel() * 8 / (min(ms) * 1e-3) / 1e9


lines, results = [], []
for config in configs:
    data = synth.CONFIGS[config]()
    eng = Engine(0)
    sh = prepare_flat(eng, data["policies"], data["resources"], data["probes"])
    P, K, W = sh["pods"], sh["slots"], sh["words"]
    d_in = torch.empty((P, K, W), dtype=torch.int64, device="cuda")
    d_eg = torch.empty((P, K, W), dtype=torch.int64, device="cuda")
    d_st = torch.empty((P, K), dtype=torch.uint8, device="cuda")
    step_ms = float("inf")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(steps):
        e0.record()
        eng.run_device(d_in.data_ptr(), d_eg.data_ptr(), d_st.data_ptr(), torch.cuda.current_stream().cuda_stream)
        e1.record()
        torch.cuda.synchronize()
        step_ms = min(step_ms, e0.elapsed_time(e1))
    res = {"config": config, "pods": P, "slots": K, "words": W, "descriptors": sh["descriptors"], "targets_in": sh["targets_in"],
           "targets_eg": sh["targets_eg"], "step_ms": step_ms, "plane_gb": P * K * W * 8 / 1e9, "reps": reps}
    res["fill_gbs"] = fill_gbs(min(P * K * W * 8, 4 << 30))
    for d in ("ingress", "egress"):
        best = float("inf")
        for _ in range(reps):
            torch.cuda.synchronize()
            t = time.perf_counter()
            eff, app = eng.target_effects(d)
            best = min(best, (time.perf_counter() - t) * 1e3)
        sole = eff[:, :, 2:].sum(axis=(1, 2))
        res[d] = {"ms": best, "over_step": best / step_ms, "batches": eng.get_option("effects_batches"),
                  "row_builds": eng.get_option("effects_launches"), "scratch_mb": eng.get_option("effects_scratch_bytes") / 2**20,
                  "unused": int((app == 0).sum()), "never_allowing": int((eff[:, :, 0].sum(axis=1) == 0).sum()),
                  "redundant": int((sole == 0).sum()), "sole_allowing": int(eff[:, :, 2].sum()), "sole_denying": int(eff[:, :, 3].sum())}
    lines.append(f"# {config}: P {P}, K {K}, W {W}, D {sh['descriptors']}, targets {sh['targets_in']} / {sh['targets_eg']}; table step "
                 f"{step_ms:.3f} ms (min of {steps}; planes 2 x {res['plane_gb']:.2f} GB); the box's fill figure {res['fill_gbs']:.0f} GB/s")
    for d in ("ingress", "egress"):
        r = res[d]
        lines.append(f"{d:8s} {r['ms']:9.2f} ms  = {r['over_step']:7.1f} x step   {r['batches']} batches, {r['row_builds']} row builds, scratch "
                     f"{r['scratch_mb']:.1f} MB   targets unused {r['unused']}, never allowing {r['never_allowing']}, redundant {r['redundant']}; "
                     f"sole-allowing cells {r['sole_allowing']}, sole-denying cells {r['sole_denying']}")
    results.append(res)
    del d_in, d_eg, d_st
    eng.close()
    torch.cuda.empty_cache()
lines.append(json.dumps(results))
print("\n".join(lines))
if "out" in kw:
    os.makedirs(os.path.dirname(os.path.abspath(kw["out"])), exist_ok=True)
    with open(kw["out"], "w") as f:
        f.write("\n".join(lines) + "\n")
