"""What the `bestfit` option costs at BASELINE config 2 (d = 30, 65 536 walkers; both records and the
profiles of all 30 parameters at 64 bins) -- the source of profiles/r13_bestfit.txt.

  python tools/bestfit_bench.py ab         whole-job time per launch (host clock around work that
                                           ends in a device synchronise) with the option off / on,
                                           two samplers alternated in one process
  rocprofv3 --kernel-trace --stats -- python tools/bestfit_bench.py trace
                                           one run with `bestfit` on AND `marginals` on 30 parameters
                                           x 64 bins (no pairs): bestfit_kernel, bestfit_commit_kernel
                                           and marginals_kernel in the same trace
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


def sampler(bestfit, marginals=None):
    info = bench.make_info(D, mean, cov, W, None, None)
    info["sampler"]["mcmc_hip"]["bestfit"] = bestfit
    info["sampler"]["mcmc_hip"]["marginals"] = marginals
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
    on = {"params": "all", "bins": 64}
    if mode == "trace":
        s = sampler(on, {"params": "all", "bins": 64})
        for _ in range(30):
            s.advance()
        ms = timed(s, 100)
        b = s.products()["bestfit"]
        print(json.dumps({"mode": mode, "ms_per_launch": ms, "spl": int(s.steps_per_launch),
                          "kernel": s.engine.last_step_kernel(), "n_acc": b.n_accumulations,
                          "bestfit_chi2": b.bestfit.chi2, "filled_bins": int(np.count_nonzero(b.slab)),
                          "interval_a0": b.interval(names[0])}), flush=True)
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
