#!/usr/bin/env python3
"""What the stretch move costs and buys (profiles/r19_stretch_move.txt).

A. The kernel: 65 536 walkers, a function that only zeroes the engine's result buffer, at d = 2
   (group_size 64), 30 (128) and 64 (256).  Per HALF-UPDATE, from the engine's event timing:
   stretch_kernel, beside fn_walker_kernel per step at the same d in the same session, and its ratio
   to the byte floor -- one read of the active and the partner states plus one write of the trial
   rows, 3 x 8 d W / 2 bytes, over the HBM rate (8 TB/s).  Wall time per step (two half-updates, two
   calls of the function) with that function.

B. The banana at d = 2: wall time per step of both moves at 65 536 walkers; and `run(info)` with
   16 384 walkers and `autocorr` on for both moves -- acceptance, the integrated autocorrelation time
   in steps and in FUNCTION EVALUATIONS per walker (a stretch step evaluates every walker once, as a
   Metropolis step does: two calls of half the rows), steps and wall time to Rminus1_stop 0.01.

    python tools/stretch_bench.py [--steps 400] [--skip-kernel] [--skip-job]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch  # noqa: F401  (before the engine: one HIP runtime)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_BYTES_PER_S = 8.0e12


def zero_function(p, out):
    return out.zero_()


def banana(p):
    return -0.5 * (p[:, 0] ** 2 + ((p[:, 1] - 0.5 * p[:, 0] ** 2) / 0.5) ** 2)


def time_engine(label, d, gs, W, move, fn, steps, warmup, pass_out):
    from cobaya_amd.engine import Engine
    eng = Engine(d, W, group_size=gs, device=0, seed=1, max_tries=1e12)
    eng.set_prior(np.zeros(d, np.int32), np.full(d, -30.0), np.full(d, 30.0))
    eng.set_target_function(fn, pass_out=pass_out)
    eng.set_move(move, 2.0)
    eng.set_proposal_cov(np.eye(d) * 0.25)
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
    launches = kt["step_launches"]
    out = {"case": label, "d": d, "group_size": gs, "move": move, "kernel": name, "launches": launches,
           "kernel_us_per_launch": 1e3 * kt["step_ms"] / launches, "kernel_us_per_step": 1e3 * kt["step_ms"] / steps,
           "wall_us_per_step": 1e6 * wall / steps, "acceptance": acc}
    if move == "stretch":
        floor_us = 1e6 * 3 * 8 * d * (W // 2) / HBM_BYTES_PER_S
        out["byte_floor_us_per_half_update"] = floor_us
        out["kernel_over_floor"] = out["kernel_us_per_launch"] / floor_us
    return out


def job(move, n_walkers):
    from cobaya_amd import run
    ref = ({"a": {"dist": "norm", "loc": 0, "scale": 1}, "b": {"dist": "norm", "loc": 0.5, "scale": 1}}
           if move == "stretch" else {"a": 0, "b": 0.5})
    opts = {"n_walkers": n_walkers, "seed": 11, "Rminus1_stop": 0.01, "max_samples": n_walkers * 200000,
            # (one lag of `autocorr` is one launch of 20 steps: Sokal's window closes within 64 lags for both)
            "autocorr": {"params": "all", "lags": 64}, "steps_per_launch": 20}
    if move == "stretch":
        opts["move"] = "stretch"
    else:
        opts["max_tries"] = "2000d"
    info = {"likelihood": {"banana": {"class": "device_function", "function": banana}},
            "params": {"a": {"prior": {"min": -8, "max": 8}, "ref": ref["a"], "proposal": 1},
                       "b": {"prior": {"min": -6, "max": 30}, "ref": ref["b"], "proposal": 1}},
            "sampler": {"mcmc_hip": opts}}
    t0 = time.perf_counter()
    _, smp = run(info)
    wall = time.perf_counter() - t0
    ac = smp.products()["autocorr"]
    lag_steps = int(smp.steps_per_launch) * max(1, int(smp.moments_every))
    names = ("a", "b")
    out = {"move": move, "converged": bool(smp.converged), "steps": int(smp.n_steps_raw), "wall_s": wall,
           "acceptance": smp._accepted_total / float(smp.n_steps_raw * n_walkers),
           "steps_per_lag": lag_steps, "tau_lags": {n: float(ac.tau(n)) for n in names},
           # one evaluation per walker and step under both moves: tau in steps IS tau in evaluations
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
    ap.add_argument("--skip-kernel", action="store_true")
    ap.add_argument("--skip-job", action="store_true")
    a = ap.parse_args()
    if not a.skip_kernel:
        for d, gs in ((2, 64), (30, 128), (64, 256)):
            for move in ("metropolis", "stretch", "metropolis"):
                print(json.dumps(time_engine("zero", d, gs, a.walkers, move, zero_function, a.steps, a.warmup, True)),
                      flush=True)
        for move in ("metropolis", "stretch"):
            print(json.dumps(time_engine("banana", 2, 64, a.walkers, move, banana, a.steps, a.warmup, False)),
                  flush=True)
    if not a.skip_job:
        for move in ("metropolis", "stretch"):
            print(json.dumps(job(move, 16384)), flush=True)


if __name__ == "__main__":
    main()
