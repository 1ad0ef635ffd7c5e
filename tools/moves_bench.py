#!/usr/bin/env python3
"""What the mixtures of ensemble moves cost and buy (profiles/r20_moves.txt).

A. The kernels: 65 536 walkers, a function that only zeroes the engine's result buffer, at d = 2
   (group_size 64), 30 (128) and 64 (256).  Per HALF-UPDATE, from the engine's event timing:
   stretch_kernel (`move: stretch`) and ensemble_move_kernel with each kind alone, in one session;
   the ratio of each to stretch_kernel.  Under `rocprofv3 --kernel-trace --stats` the same run gives
   the times per kernel name (the kind is the kernel's second template argument).

B. The banana at d = 2: `run(info)` with 16 384 walkers and `autocorr` on for `move: stretch`,
   `moves: de` and `moves: de + snooker` -- acceptance, the integrated autocorrelation time in steps,
   which are FUNCTION EVALUATIONS per walker (every kind evaluates every walker once per step),
   steps and wall time to Rminus1_stop 0.01.

    python tools/moves_bench.py [--steps 400] [--dims 2,30,64] [--skip-kernel] [--skip-job]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch  # noqa: F401  (before the engine: one HIP runtime)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KINDS = {"stretch": None, "moves:stretch": [["stretch", 1]], "moves:de": [["de", 1]],
         "moves:snooker": [["snooker", 1]]}
JOBS = {"stretch": {"move": "stretch"}, "de": {"moves": [["de", 1]]},
        "de+snooker": {"moves": [["de", 0.8], ["snooker", 0.2]]}}


def zero_function(p, out):
    return out.zero_()


def banana(p):
    return -0.5 * (p[:, 0] ** 2 + ((p[:, 1] - 0.5 * p[:, 0] ** 2) / 0.5) ** 2)


def time_engine(d, gs, W, which, steps, warmup):
    from cobaya_amd.engine import Engine
    eng = Engine(d, W, group_size=gs, device=0, seed=1, max_tries=1e12)
    eng.set_prior(np.zeros(d, np.int32), np.full(d, -30.0), np.full(d, 30.0))
    eng.set_target_function(zero_function, pass_out=True)
    if KINDS[which] is None:
        eng.set_move("stretch", 2.0)
    else:
        eng.set_moves(KINDS[which])
    eng.set_state(np.random.default_rng(0).normal(0.0, 0.5, (W, d)))
    eng.step(warmup)
    eng.sync()
    eng.enable_timing(True)
    eng.kernel_times(reset=True)
    t0 = time.perf_counter()
    eng.step(steps)
    eng.sync()
    wall = time.perf_counter() - t0
    kt = eng.kernel_times()
    name = eng.last_step_kernel()
    acc = eng.counters()["accepted"] / float((steps + warmup) * W)
    eng.close()
    return {"d": d, "group_size": gs, "move": which, "kernel": name, "launches": kt["step_launches"],
            "kernel_us_per_half_update": 1e3 * kt["step_ms"] / kt["step_launches"],
            "wall_us_per_step": 1e6 * wall / steps, "acceptance": acc}


def job(label, n_walkers):
    from cobaya_amd import run
    opts = {"n_walkers": n_walkers, "seed": 11, "Rminus1_stop": 0.01, "max_samples": n_walkers * 200000,
            # (one lag of `autocorr` is one launch of 20 steps, as tools/stretch_bench.py has it)
            "autocorr": {"params": "all", "lags": 64}, "steps_per_launch": 20, "max_tries": "400d", **JOBS[label]}
    info = {"likelihood": {"banana": {"class": "device_function", "function": banana}},
            "params": {"a": {"prior": {"min": -8, "max": 8}, "ref": {"dist": "norm", "loc": 0, "scale": 1}},
                       "b": {"prior": {"min": -6, "max": 30}, "ref": {"dist": "norm", "loc": 0.5, "scale": 1}}},
            "sampler": {"mcmc_hip": opts}}
    t0 = time.perf_counter()
    _, smp = run(info)
    wall = time.perf_counter() - t0
    ac = smp.products()["autocorr"]
    names = ("a", "b")
    out = {"moves": label, "converged": bool(smp.converged), "steps": int(smp.n_steps_raw), "wall_s": wall,
           "acceptance": smp._accepted_total / float(smp.n_steps_raw * n_walkers),
           "tau_steps": {n: float(ac.tau_steps(n)) for n in names},
           "tau_window_closed": {n: bool(ac.converged(n)) for n in names},
           "kernel": smp.engine.last_step_kernel()}
    smp.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--walkers", type=int, default=65536)
    ap.add_argument("--dims", default="2,30,64", help="the d of part A (group_size 64 / 128 / 256 by d)")
    ap.add_argument("--skip-kernel", action="store_true")
    ap.add_argument("--skip-job", action="store_true")
    a = ap.parse_args()
    if not a.skip_kernel:
        for d in (int(v) for v in a.dims.split(",")):
            gs = 64 if 4 * d <= 64 else (128 if 4 * d <= 128 else 256)
            base = None
            for which in KINDS:
                r = time_engine(d, gs, a.walkers, which, a.steps, a.warmup)
                base = r["kernel_us_per_half_update"] if base is None else base
                r["over_stretch_kernel"] = r["kernel_us_per_half_update"] / base
                print(json.dumps(r), flush=True)
    if not a.skip_job:
        for label in JOBS:
            print(json.dumps(job(label, 16384)), flush=True)


if __name__ == "__main__":
    main()
