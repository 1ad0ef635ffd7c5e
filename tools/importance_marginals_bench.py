"""What the reweighted marginal histograms cost at BASELINE config 2 (d = 30, 65 536 walkers; `marginals` of
30 parameters x 128 bins and ten 32 x 32 pairs; 1 or 4 importance alternatives with `marginals: True`, beside
every moment snapshot) -- the source of profiles/r17_importance_marginals.txt.

  python tools/importance_marginals_bench.py ab N     whole-job time per launch (host clock around work that ends
                                                      in a device synchronise) with N alternatives and the run's
                                                      marginals, the key off / on: two samplers alternated in
                                                      one process
  rocprofv3 --kernel-trace --stats -- python tools/importance_marginals_bench.py trace N
                                                      one run with the key on: importance_hist_weights_kernel and
                                                      importance_hist_kernel beside marginals_kernel and
                                                      importance_group_kernel in the same trace (no counters)
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402,F401
import torch  # noqa: E402,F401  (before the first engine: one HIP runtime for both)

import bench  # noqa: E402
from cobaya_amd.model import ProblemSpec  # noqa: E402
from cobaya_amd.sampler import MCMCHip  # noqa: E402
from tools.importance_bench import ALTERNATIVES, D, W, cov, mean, timed  # noqa: E402

PAIRS = [["a__%d" % i, "a__%d" % (i + 1)] for i in range(0, 20, 2)]
MARGINALS = {"params": "all", "pairs": PAIRS, "bins": 128, "bins2d": 32}


def sampler(n_alt, key):
    info = bench.make_info(D, mean, cov, W, None, None)
    o = info["sampler"]["mcmc_hip"]
    o["marginals"] = MARGINALS
    o["importance"] = {k: dict(v, marginals=key) for k, v in list(ALTERNATIVES.items())[:n_alt]}
    s = MCMCHip(o, ProblemSpec.from_info(info))
    s._next_ckpt = s._checkpoint_steps()
    return s


def main():
    mode, n_alt = sys.argv[1], int(sys.argv[2])
    if mode == "trace":
        s = sampler(n_alt, True)
        for _ in range(30):
            s.advance()
        ms = timed(s, 100)
        iw = s.products()["importance"]
        print(json.dumps({"mode": mode, "n_alt": n_alt, "ms_per_launch": ms, "spl": int(s.steps_per_launch),
                          "kernel": s.engine.last_step_kernel(), "n_samples": iw.n_samples,
                          "hist_layout": s.engine.importance_hist_layout(),
                          "saturated": [iw.saturated(n) for n in iw.names],
                          "median_of_a__0": [iw.marginals(n).quantile("a__0", 0.5) for n in iw.names]}))
        s.close()
        return
    off, on = sampler(n_alt, False), sampler(n_alt, True)
    for s in (off, on):
        for _ in range(30):
            s.advance()
    t_off, t_on = [], []
    for _ in range(6):
        t_off.append(timed(off, 150))
        t_on.append(timed(on, 150))
    print(json.dumps({"mode": mode, "n_alt": n_alt, "spl": int(on.steps_per_launch),
                      "ms_per_launch_off": t_off, "ms_per_launch_on": t_on,
                      "ratio_of_medians": float(np.median(t_on) / np.median(t_off))}))
    off.close()
    on.close()


if __name__ == "__main__":
    main()
