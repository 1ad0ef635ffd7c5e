"""What the `marginals` option costs at BASELINE config 2 (d = 30, 65 536 walkers; all 30
parameters at 128 bins plus ten pairs at 32 x 32) -- the source of profiles/r09_marginals.txt.

  python tools/marginals_bench.py ab       whole-job time per launch (host clock around work that
                                           ends in a device synchronise) with the option off / on /
                                           peaked, three samplers alternated in one process
  rocprofv3 --kernel-trace --stats -- python tools/marginals_bench.py trace
                                           one run with the option on: kernel times from the trace
  ... marginals_bench.py peaked            the same with ranges of 1000 sigma, off centre: nearly all
                                           walkers of a parameter share ONE bin (atomic contention)
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
PAIRS = [[names[i], names[i + 1]] for i in range(10)]


def option(kind):
    if kind == "off":
        return None
    opt = {"params": "all", "pairs": PAIRS, "bins": 128, "bins2d": 32}
    if kind == "peaked":
        sd = np.sqrt(np.diag(cov))
        opt["ranges"] = {n: [float(mean[i] - 400 * sd[i]), float(mean[i] + 600 * sd[i])]
                         for i, n in enumerate(names)}
    return opt


def sampler(kind):
    info = bench.make_info(D, mean, cov, W, None, None)
    info["sampler"]["mcmc_hip"]["marginals"] = option(kind)
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
    if mode in ("trace", "peaked"):
        s = sampler("on" if mode == "trace" else "peaked")
        for _ in range(30):
            s.advance()
        ms = timed(s, 100)
        m = s.products()["marginals"]
        print(json.dumps({"mode": mode, "ms_per_launch": ms, "spl": int(s.steps_per_launch),
                          "kernel": s.engine.last_step_kernel(), "n_acc": m.n_accumulations,
                          "max_bin_share": float(m.counts(names[0]).max() / max(1, m.counts(names[0]).sum())),
                          "outside0": m.outside(names[0])}), flush=True)
        s.close()
        return
    kinds = ("off", "on", "peaked")
    ss = {k: sampler(k) for k in kinds}
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
    out["peaked_over_off"] = out["peaked"]["ms_per_launch_median"] / out["off"]["ms_per_launch_median"]
    out["spl"] = int(ss["on"].steps_per_launch)
    out["kernel"] = ss["on"].engine.last_step_kernel()
    print(json.dumps(out), flush=True)
    for s in ss.values():
        s.close()


main()
