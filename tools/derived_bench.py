"""What function-derived parameters cost at BASELINE config 2 (d = 30, 65 536 walkers; four derived
parameters, cross-moments with all 30 sampled ones, beside every moment snapshot) -- the source of
profiles/r15_derived.txt.

  python tools/derived_bench.py ab         whole-job time per launch (host clock around work that
                                           ends in a device synchronise) without / with the derived
                                           parameters, two samplers alternated in one process; and
                                           the host time of queueing the four functions
  rocprofv3 --kernel-trace --stats -- python tools/derived_bench.py trace
                                           one run with them: derived_group_kernel, derived_pool_kernel,
                                           the moment kernels and (with `marginals`) marginals_kernel
                                           in the same trace (no counters)
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (before the first engine: one HIP runtime for both)

import bench  # noqa: E402
from cobaya_amd.model import ProblemSpec  # noqa: E402
from cobaya_amd.sampler import MCMCHip  # noqa: E402

D, W = 30, 65536
mean, cov = bench.target(D)
DERIVED = {"s01": {"derived": "lambda a__0, a__1: a__0 + a__1"},
           "p23": {"derived": "lambda a__2, a__3: a__2 * a__3"},
           "q": {"derived": "lambda a__4, a__5, a__6: a__4 * a__5 ** 2 / (1.0 + a__6 ** 2)"},
           "r": {"derived": "lambda s01, p23: torch.sqrt(s01 ** 2 + p23 ** 2)"}}


def sampler(on, marginals=False):
    info = bench.make_info(D, mean, cov, W, None, None)
    if on:
        info["params"].update(DERIVED)
        if marginals:
            info["sampler"]["mcmc_hip"]["marginals"] = {"params": ["a__0", "s01", "r"],
                                                        "ranges": {"s01": [-10.0, 10.0], "r": [0.0, 10.0]}}
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


def host_eval_us(s, n=200):
    """Host time of queueing the functions of one snapshot (nothing is waited for)."""
    s.engine.sync()
    t0 = time.perf_counter()
    for _ in range(n):
        s._derived.evaluate(force=True)
    t = 1e6 * (time.perf_counter() - t0) / n
    s.engine.sync()
    return t


def main():
    mode = sys.argv[1]
    if mode == "trace":
        s = sampler(True, marginals=True)
        for _ in range(30):
            s.advance()
        ms = timed(s, 100)
        dv = s.products()["derived"]
        print(json.dumps({"mode": mode, "ms_per_launch": ms, "spl": int(s.steps_per_launch),
                          "kernel": s.engine.last_step_kernel(), "n_used": dv.n_used, "n_samples": dv.n_samples,
                          "mean": {n: dv.mean(n) for n in dv.names}, "std": {n: dv.std(n) for n in dv.names}}),
              flush=True)
        s.close()
        return
    kinds = ("off", "on")
    ss = {"off": sampler(False), "on": sampler(True)}
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
    out["host_us_per_evaluation_of_four_functions"] = host_eval_us(ss["on"])
    print(json.dumps(out), flush=True)
    for s in ss.values():
        s.close()


main()
