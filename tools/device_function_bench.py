#!/usr/bin/env python3
"""What a function target costs per step (profiles/r08_device_function.txt).

65 536 walkers, d in {2, 30, 100}; the function is (a) `out.zero_()` into the engine's own result
buffer, (b) the banana of the README.  Reported per step: the propose + accept kernel
(fn_walker_kernel, one launch per step) from the engine's event timing, and the wall time of
the whole step loop -- one ctypes callback and the function's torch launches per step.  Two
yardsticks, neither of them the code under test:

  * pl_walker_kernel<true, true> of the plik-lite target at d = 27, W = 65 536
    (`Engine.binned_kernel_times`): the same work fused, without the transposition;
  * the byte floor: 4 x 8 d W bytes per step (x in, trial out; trial in, x out) at the measured
    HBM copy rate of the MI355X, 6.29 TB/s.

    python tools/device_function_bench.py [--steps 400] [--walkers 65536]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch  # noqa: F401  (before the engine's library: one HIP runtime in the process)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_BYTES_PER_S = 6.29e12


def zero_function(p, out):
    return out.zero_()


def banana(p):
    return -0.5 * (p[:, 0] ** 2 + ((p[:, 1] - 0.5 * p[:, 0] ** 2) / 0.5) ** 2)


def time_function_target(d, W, fn, steps, warmup, pass_out=False):
    from cobaya_amd.engine import Engine
    # (max_tries out of the way: among 65 536 walkers one always meets 40 d rejections in a row)
    eng = Engine(d, W, group_size=256, device=0, seed=1, max_tries=1e12)
    eng.set_prior(np.zeros(d, np.int32), np.full(d, -8.0), np.full(d, 8.0))
    eng.set_target_function(fn, pass_out=pass_out)
    eng.set_proposal_cov(np.eye(d))
    eng.set_state(np.random.default_rng(0).normal(0.0, 0.5, (W, d)))
    eng.step(warmup)
    eng.sync()
    eng.enable_timing(True)
    eng.kernel_times(reset=True)
    t0 = time.perf_counter()
    eng.step(steps)
    t_queued = time.perf_counter() - t0
    eng.sync()
    wall = time.perf_counter() - t0
    kt = eng.kernel_times()
    name = eng.last_step_kernel()
    eng.close()
    floor_us = 4 * 8 * d * W / HBM_BYTES_PER_S * 1e6
    return {"d": d, "walkers": W, "kernel": name,
            "kernel_us_per_step": 1e3 * kt["step_ms"] / steps,
            "basis_us_per_step": 1e3 * kt["basis_ms"] / steps,
            "wall_us_per_step": 1e6 * wall / steps,
            "host_queue_us_per_step": 1e6 * t_queued / steps,
            "byte_floor_us": floor_us}


def time_pl_walker(W, steps, warmup):
    """The parent's fused walker kernel on the plik-lite-shaped target (d = 27)."""
    from cobaya_amd import pliklite as P
    from cobaya_amd.engine import Engine
    d = 27
    target = P.BinnedGaussian.from_dataset(P.synthetic_dataset(1))
    emu = P.synthetic_emulator(d - 1, target.lmax)
    # uniform boxes of +- 8 posterior sigmas on the emulator parameters, the reference's normal
    # prior on the calibration; the Fisher estimate of the posterior as proposal covariance
    C = P.fisher_covariance(target, emu)
    sig = np.sqrt(np.diag(C))
    kinds = np.array([0] * (d - 1) + [1], dtype=np.int32)
    lo = np.concatenate((emu.theta0 - 8.0 * sig[:d - 1], [1.0]))
    hi = np.concatenate((emu.theta0 + 8.0 * sig[:d - 1], [0.0025]))
    eng = Engine(d, W, group_size=256, device=0, seed=1)
    eng.set_prior(kinds, lo, hi)
    eng.set_target_binned_gaussian(target, emu, d - 1)
    eng.set_proposal_cov(C)
    rng = np.random.default_rng(0)
    x0 = np.concatenate((emu.theta0, [1.0])) + 0.5 * sig * rng.standard_normal((W, d))
    eng.set_state(x0)
    eng.step(warmup)
    eng.sync()
    eng.enable_timing(True)
    eng.binned_kernel_times(reset=True)
    eng.step(steps)
    eng.sync()
    bt = eng.binned_kernel_times()
    eng.close()
    return {"d": d, "walkers": W, "kernel": "mcmc::pl_walker_kernel<true, true>",
            "kernel_us_per_launch": 1e3 * bt["walker_ms"] / max(bt["launches"][0], 1),
            "byte_floor_us": 2 * 8 * d * W / HBM_BYTES_PER_S * 1e6}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--walkers", type=int, default=65536)
    ap.add_argument("--no-yardstick", action="store_true", help="skip the plik-lite walker kernel")
    args = ap.parse_args()
    rows = []
    for d in (2, 30, 100):
        for label, fn in (("zero", zero_function), ("banana", banana)):
            r = time_function_target(d, args.walkers, fn, args.steps, args.warmup,
                                     pass_out=fn is zero_function)
            r["function"] = label
            rows.append(r)
            print(json.dumps(r), flush=True)
    if not args.no_yardstick:
        r = time_pl_walker(args.walkers, min(args.steps, 100), 10)
        print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
