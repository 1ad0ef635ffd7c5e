"""What importance reweighting costs at BASELINE config 2 (d = 30, 65 536 walkers; 1 or 4 alternatives
with `cov: True`, beside every moment snapshot) -- the source of profiles/r16_importance.txt.

  python tools/importance_bench.py ab N      whole-job time per launch (host clock around work that ends
                                             in a device synchronise) without / with N alternatives, two
                                             samplers alternated in one process; and the host time of
                                             queueing the N functions
  rocprofv3 --kernel-trace --stats -- python tools/importance_bench.py trace N
                                             one run with them: importance_group_kernel,
                                             importance_max_kernel and the moment kernels in the same
                                             trace (no counters)
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

D, W = 30, 65536
mean, cov = bench.target(D)
ALTERNATIVES = {"bao": {"function": "lambda a__0: -0.5 * ((a__0 - 0.1) * 2.0) ** 2", "cov": True},
                "prior": {"function": "lambda a__1, a__2: -0.125 * (a__1 * a__1 + a__2 * a__2)", "cov": True},
                "tilt": {"function": "lambda a__3: 0.25 * a__3", "cov": True},
                "wall": {"function": "lambda a__4: torch.where(a__4 > -1.0, 0.0 * a__4, -math.inf + 0.0 * a__4)",
                         "cov": True}}


def sampler(n_alt):
    info = bench.make_info(D, mean, cov, W, None, None)
    if n_alt:
        info["sampler"]["mcmc_hip"]["importance"] = dict(list(ALTERNATIVES.items())[:n_alt])
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


def accumulator(s):
    return next(p for p in s._products if p.name == "importance")


def host_eval_us(s, n=200):
    """Host time of queueing the functions of one snapshot (nothing is waited for)."""
    s.engine.sync()
    t0 = time.perf_counter()
    for _ in range(n):
        accumulator(s).evaluate()
    t = 1e6 * (time.perf_counter() - t0) / n
    s.engine.sync()
    return t


def main():
    mode, n_alt = sys.argv[1], int(sys.argv[2])
    if mode == "trace":
        s = sampler(n_alt)
        for _ in range(30):
            s.advance()
        ms = timed(s, 100)
        iw = s.products()["importance"]
        print(json.dumps({"mode": mode, "n_alt": n_alt, "ms_per_launch": ms, "spl": int(s.steps_per_launch),
                          "group_size": int(s.group_size), "kernel": s.engine.last_step_kernel(),
                          "n_samples": iw.n_samples, "ess_fraction": [iw.ess_fraction(n) for n in iw.names],
                          "log_ratio": [iw.log_ratio(n) for n in iw.names]}))
        s.close()
        return
    off, on = sampler(0), sampler(n_alt)
    for s in (off, on):
        for _ in range(30):
            s.advance()
    t_off, t_on = [], []
    for _ in range(6):
        t_off.append(timed(off, 150))
        t_on.append(timed(on, 150))
    print(json.dumps({"mode": mode, "n_alt": n_alt, "spl": int(on.steps_per_launch), "group_size": int(on.group_size),
                      "ms_per_launch_off": t_off, "ms_per_launch_on": t_on,
                      "ratio_of_medians": float(np.median(t_on) / np.median(t_off)),
                      "host_eval_us_per_snapshot": host_eval_us(on)}))
    off.close()
    on.close()


if __name__ == "__main__":
    main()
