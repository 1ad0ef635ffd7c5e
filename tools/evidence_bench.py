"""What the `evidence` option costs at BASELINE config 2 (d = 30, 65 536 walkers; the default ladder
of five radii beside every moment snapshot) -- the source of profiles/r14_evidence.txt.

  python tools/evidence_bench.py ab        whole-job time per launch (host clock around work that
                                           ends in a device synchronise) with the option off / on,
                                           two samplers alternated in one process
  rocprofv3 --kernel-trace --stats -- python tools/evidence_bench.py trace
                                           one run with `evidence` on: evidence_kernel,
                                           evidence_group_kernel and the moment kernels in the same
                                           trace (no counters)
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import bench  # noqa: E402
from cobaya_amd.model import ProblemSpec  # noqa: E402
from cobaya_amd.sampler import MCMCHip  # noqa: E402

D, W = 30, 65536
mean, cov = bench.target(D)
names = [f"a__{i}" for i in range(D)]


def sampler(evidence):
    info = bench.make_info(D, mean, cov, W, None, None)
    info["sampler"]["mcmc_hip"]["evidence"] = evidence
    s = MCMCHip(info["sampler"]["mcmc_hip"], ProblemSpec.from_info(info))
    s._next_ckpt = s._checkpoint_steps()
    return s


def timed(s, n):
    s.engine.sync()
    t0 = time.perf_counter()
    for _ in range(n):
        s.advance()
    if s._ckpt_pending:
        s._finish_checkpoint()
        s._after_checkpoint()
    s.engine.sync()
    return 1e3 * (time.perf_counter() - t0) / n


def main():
    mode = sys.argv[1]
    on = True
    if mode == "trace":
        s = sampler(on)
        for _ in range(30):
            s.advance()
        ms = timed(s, 100)
        e = s.products()["evidence"]
        print(json.dumps({"mode": mode, "ms_per_launch": ms, "spl": int(s.steps_per_launch),
                          "kernel": s.engine.last_step_kernel(), "n_acc": int(e.n_acc.sum()),
                          "lnZ": e.lnZ, "stderr": e.stderr, "radius": e.radius,
                          "lnZ_by_radius": e.lnZ_by_radius().tolist(),
                          "inside": e.inside_fraction().tolist(), "clamped": e.clamped}), flush=True)
        s.close()
        return
    kinds = ("off", "on")
    ss = {"off": sampler(None), "on": sampler(on)}
    for s in ss.values():
        for _ in range(60):
            s.advance()
        s.engine.sync()
    res = {k: [] for k in kinds}
    for rep in range(6):
        for k in kinds:
            res[k].append(timed(ss[k], 150))
        print(json.dumps({"rep": rep, **{k: res[k][-1] for k in kinds}}), flush=True)
    out = {k: {"ms_per_launch_median": float(np.median(v)), "min": min(v), "max": max(v)} for k, v in res.items()}
    out["on_over_off"] = out["on"]["ms_per_launch_median"] / out["off"]["ms_per_launch_median"]
    out["spl"] = int(ss["on"].steps_per_launch)
    out["kernel"] = ss["on"].engine.last_step_kernel()
    print(json.dumps(out), flush=True)
    for s in ss.values():
        s.close()


main()
