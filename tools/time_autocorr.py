"""What the `autocorr` option costs at BASELINE config 2 (d = 30, 65 536 walkers, all 30 parameters,
`lags: 16`) -- the source of profiles/r11_autocorr.txt.

  python tools/time_autocorr.py kernel [lags]   one accumulation at a full ring: host clock around 200
                                                queued accumulations that end in a device synchronise
                                                (and the two moment kernels the same way), against
                                                the byte floor (lags + 2) d W 8 B at 6.29 TB/s
  python tools/time_autocorr.py ab              whole-job time per launch with the option off / on,
                                                two samplers alternated in one process
  python tools/time_autocorr.py off             the whole job with the option off only (the same
                                                command on the parent commit gives the noise)
  rocprofv3 --kernel-trace --stats -- python tools/time_autocorr.py trace
                                                one run with the option on: kernel times from the trace
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
COPY_RATE = 6.29e12      # B/s: the measured device copy rate the floor is stated at
mean, cov = bench.target(D)


def sampler(option):
    info = bench.make_info(D, mean, cov, W, None, None)
    if option is not None:
        info["sampler"]["mcmc_hip"]["autocorr"] = option
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


def queued(eng, call, n=200):
    eng.sync()
    t0 = time.perf_counter()
    for _ in range(n):
        call()
    eng.sync()
    return 1e6 * (time.perf_counter() - t0) / n


def kernel(lags):
    s = sampler({"params": "all", "lags": lags})
    eng = s.engine
    for _ in range(3):
        s.advance()
    for _ in range(lags + 1):          # fill the ring
        eng.accumulate_autocorr()
    assert eng.autocorr_layout()["held"] == lags + 1
    us = [queued(eng, eng.accumulate_autocorr) for _ in range(5)]
    mom = [queued(eng, eng.accumulate_moments) for _ in range(5)]
    floor = (lags + 2) * D * W * 8 / COPY_RATE * 1e6
    print(json.dumps({"mode": "kernel", "lags": lags, "group_size": int(s.group_size),
                      "us_per_accumulation_median": float(np.median(us)), "min": min(us), "max": max(us),
                      "us_per_moment_snapshot_median": float(np.median(mom)),
                      "floor_us": floor, "over_floor": float(np.median(us)) / floor,
                      "ring_MB": (lags + 1) * D * W * 8 / 1e6}), flush=True)
    s.close()


def main():
    mode = sys.argv[1]
    if mode == "kernel":
        kernel(int(sys.argv[2]) if len(sys.argv) > 2 else 16)
        return
    if mode == "trace":
        s = sampler(True)
        for _ in range(30):
            s.advance()
        ms = timed(s, 100)
        ac = s.products()["autocorr"]
        print(json.dumps({"mode": mode, "ms_per_launch": ms, "spl": int(s.steps_per_launch),
                          "kernel": s.engine.last_step_kernel(), "n_pairs": ac.n_pairs.tolist()}), flush=True)
        s.close()
        return
    kinds = ("off",) if mode == "off" else ("off", "on")
    ss = {k: sampler(None if k == "off" else True) for k in kinds}
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
    if "on" in out:
        out["on_over_off"] = out["on"]["ms_per_launch_median"] / out["off"]["ms_per_launch_median"]
        ac = ss["on"].products()["autocorr"]
        worst = ac.worst()
        out["worst"] = {"param": worst[0], "tau_snapshots": worst[1], "converged": worst[2],
                        "interval_steps": ac.interval_steps}
    out["spl"] = int(ss["off"].steps_per_launch)
    out["kernel"] = ss["off"].engine.last_step_kernel()
    print(json.dumps(out), flush=True)
    for s in ss.values():
        s.close()


main()
