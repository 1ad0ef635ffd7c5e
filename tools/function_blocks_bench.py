#!/usr/bin/env python3
"""What several device functions over parameter blocks cost and save
(profiles/r18_function_blocks.txt).

A. The kernel: d = 30, 65 536 walkers, functions that only zero their result.  Per step, from the
   engine's event timing: fn_walker_kernel with one function (the yardstick, in the same session),
   fn_blocked_walker_kernel with two functions slow(10 parameters) and fast(all 30) -- without
   blocks (both due at every slot) and with blocks 10 + 20, factors 1 and 4 (slow due at 10 of 90
   slots).  Beside the ratio: what the added bytes explain -- the gathered inputs written once,
   8 W (sum of the due d_c), and their x read once more, on top of the 4 x 8 d W of fn_walker_kernel.

B. The whole job: `run(info)` with a deliberately slow function of (a, b) -- a chain of float64
   matmuls, about a millisecond per call of 4 096 rows -- beside a trivial fast one of (b, c, e),
   with oversample_power 0 and 1: wall time per step and the calls of each function.

    python tools/function_blocks_bench.py [--steps 400] [--skip-job]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def zero_function(p, out):
    return out.zero_()


def time_kernel(label, d, W, inputs, blocks, factors, steps, warmup):
    from cobaya_amd.engine import Engine
    eng = Engine(d, W, group_size=256, device=0, seed=1, max_tries=1e12)
    eng.set_prior(np.zeros(d, np.int32), np.full(d, -8.0), np.full(d, 8.0))
    if inputs is None:
        eng.set_target_function(zero_function, pass_out=True)
    else:
        eng.set_target_functions([zero_function] * len(inputs), inputs, pass_out=True)
    if blocks:
        eng.set_blocking(blocks, factors)
    eng.set_proposal_cov(np.eye(d))
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
    eng.close()
    L = sum(len(b) * f for b, f in zip(blocks, factors)) if blocks else d
    # bytes written for the due functions, averaged over the slots of a cycle
    if inputs is None:
        gathered = 0.0
    elif not blocks:
        gathered = float(sum(len(i) for i in inputs))
    else:
        block_of = {i: b for b, blk in enumerate(blocks) for i in blk}
        last = [max(block_of[i] for i in idx) for idx in inputs]
        gathered = sum(len(blk) * f * sum(len(idx) for idx, lb in zip(inputs, last) if lb >= b)
                       for b, (blk, f) in enumerate(zip(blocks, factors))) / L
    base = 4 * 8 * d * W
    return {"case": label, "kernel": name, "kernel_us_per_step": 1e3 * kt["step_ms"] / steps,
            "basis_us_per_step": 1e3 * kt["basis_ms"] / steps, "wall_us_per_step": 1e6 * wall / steps,
            # (the full trial is fn_walker_kernel's own buffer; the gathered inputs are written once and
            # their x read once more, from L2)
            "bytes_ratio_explained": (base + 2 * 8 * W * gathered) / base,
            "mean_due_inputs_per_step": gathered}


CALLS = {"slow": 0, "fast": 0}   # (module level: `run` copies the input, instances included)


class Slow:
    """A chain of float64 matmuls on (n, 2) inputs; counts its calls."""

    def __init__(self, n_mm, width=512):
        g = torch.Generator(device="cpu").manual_seed(1)
        self.A = torch.randn(2, width, generator=g, dtype=torch.float64).cuda()
        self.M = (torch.randn(width, width, generator=g, dtype=torch.float64) / np.sqrt(width)).cuda()
        self.n_mm = n_mm

    def __call__(self, p):
        CALLS["slow"] += 1
        h = p @ self.A
        for _ in range(self.n_mm):
            h = torch.tanh(h @ self.M)
        return -0.5 * (p ** 2).sum(1) + 1e-30 * h.sum(1)


class Fast:
    def __call__(self, p):
        CALLS["fast"] += 1
        return -0.5 * (p ** 2).sum(1)


def time_job(power, n_mm, W, max_samples):
    from cobaya_amd import run
    slow, fast = Slow(n_mm), Fast()
    x = torch.zeros(W, 2, dtype=torch.float64, device="cuda")
    slow(x)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(10):
        slow(x)
    torch.cuda.synchronize()
    call_ms = 1e3 * (time.perf_counter() - t0) / 10
    CALLS.update(slow=0, fast=0)
    info = {"likelihood": {"slow": {"class": "device_function", "function": slow, "speed": 1,
                                    "input_params": ["a", "b"]},
                           "fast": {"class": "device_function", "function": fast, "speed": 50,
                                    "input_params": ["b", "c", "e"]}},
            "params": {p: {"prior": {"min": -12, "max": 12}, "ref": {"dist": "norm", "loc": 0, "scale": 0.5},
                           "proposal": 1} for p in "abce"},
            "sampler": {"mcmc_hip": {"n_walkers": W, "group_size": 64, "seed": 1, "oversample_power": power,
                                     "Rminus1_stop": 0.0, "max_samples": max_samples}}}
    t0 = time.perf_counter()
    _, smp = run(info)
    smp.engine.sync()
    wall = time.perf_counter() - t0
    out = {"oversample_power": power, "slow_call_ms": call_ms, "blocks": smp.blocks,
           "factors": [int(f) for f in smp.oversampling_factors], "cycle": int(smp.cycle_length),
           "steps": int(smp.n_steps_raw), "wall_s": wall, "wall_us_per_step": 1e6 * wall / smp.n_steps_raw,
           "calls_slow": CALLS["slow"], "calls_fast": CALLS["fast"], "kernel": smp.engine.last_step_kernel()}
    smp.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--walkers", type=int, default=65536)
    ap.add_argument("--matmuls", type=int, default=40)
    ap.add_argument("--skip-job", action="store_true")
    ap.add_argument("--skip-kernel", action="store_true")
    args = ap.parse_args()
    d, W = 30, args.walkers
    slow, fast = list(range(10)), list(range(30))
    cases = (("one function (fn_walker_kernel)", None, None, None),
             ("two functions, one block", [slow, fast], None, None),
             ("two functions, blocks 10 + 20, factors 1 and 4", [slow, fast],
              [list(range(10)), list(range(10, 30))], [1, 4]),
             ("one function (fn_walker_kernel), again", None, None, None))
    rows = []
    for label, inputs, blocks, factors in (() if args.skip_kernel else cases):
        rows.append(time_kernel(label, d, W, inputs, blocks, factors, args.steps, args.warmup))
        print(json.dumps(rows[-1]), flush=True)
    base = 0.5 * (rows[0]["kernel_us_per_step"] + rows[-1]["kernel_us_per_step"]) if rows else 0.0
    for r in rows[1:-1]:
        print("%s: %.2f x fn_walker_kernel (the added bytes explain %.2f x)" % (
            r["case"], r["kernel_us_per_step"] / base, r["bytes_ratio_explained"]), flush=True)
    if not args.skip_job:
        for power in (0.0, 1.0):
            print(json.dumps(time_job(power, args.matmuls, 4096, 4096 * 1500)), flush=True)


if __name__ == "__main__":
    main()
