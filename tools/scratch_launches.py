#!/usr/bin/env python3
"""Does a change of the host side launch the from-scratch step kernels as before?

    rocprofv3 --kernel-trace -d <dir> -o t -- python tools/scratch_launches.py run
    python tools/scratch_launches.py list <dir> > launches.txt

`run` steps a fixed list of shapes with `evaluation: full`, one per kernel family of csrc/scratch_choice.h, plus 65 792
walkers (257 workgroups of 256: two per compute unit) at d = 14 and d = 100, where the placement request of the
two-wave and the matrix-core kernel is no longer the one-workgroup-per-CU value.  `list` prints, from the profiler's
database, one line per dispatch of a step kernel in launch order: kernel name, grid, workgroup, LDS bytes, scratch
bytes.  The lists of two trees (or two libraries, MCMC_HIP_LIB) are compared with diff."""
import glob
import os
import sqlite3
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# name: d, W, group_size, then keyword options (K modes, own basis, drag)
SHAPES = [
    ("step", 8, 512, 64, {}),
    ("step_own", 8, 512, 64, {"own": True}),
    ("pair", 30, 512, 64, {}),
    ("mfma", 64, 512, 64, {}),
    ("big_reg", 40, 320, 64, {}),
    ("general", 40, 256, 64, {"K": 2}),
    ("drag", 8, 512, 64, {"drag": True}),
    ("general_drag", 40, 256, 64, {"drag": True}),
    ("pair_257", 14, 65792, 256, {}),
    ("mfma_257", 100, 65792, 256, {}),
]


def run():
    from cobaya_amd.engine import Engine
    for name, d, W, gs, opt in SHAPES:
        K = opt.get("K", 1)
        rng = np.random.default_rng(d)
        means = rng.uniform(0.35, 0.65, size=(K, d))
        covs = np.array([np.diag(rng.uniform(0.5, 1.5, size=d) * 0.05) ** 2 for _ in range(K)])
        eng = Engine(d, W, group_size=gs, seed=7, incremental=False, shared_basis=not opt.get("own"))
        eng.set_prior([0] * d, [0.0] * d, [1.0] * d)
        eng.set_target_gaussian_mixture(means, covs)
        if opt.get("drag"):
            eng.set_blocking([list(range(d // 2)), list(range(d // 2, d))], [1, 1], 0, 2)
        eng.set_proposal_cov(covs[0])
        eng.set_state(np.clip(means[0] + rng.normal(size=(W, d)) * np.sqrt(np.diag(covs[0])), 1e-3, 1 - 1e-3))
        eng.step(d + 3)
        eng.step(2 * d)
        eng.sync()
        print(f"{name}: {eng.last_step_kernel()}", flush=True)
        eng.close()


def dispatches(directory):
    db = sqlite3.connect(glob.glob(os.path.join(directory, "**", "*_results.db"), recursive=True)[0])
    cur = db.execute("select * from kernels order by start")
    cols = [c[0].lower() for c in cur.description]

    def col(*words):
        return next(i for i, c in enumerate(cols) if all(w in c for w in words))
    name = col("name")
    grid = [col("grid", a) for a in "xyz"]
    wg = [col("workgroup", a) for a in "xyz"]
    lds, scratch = col("lds"), col("scratch")
    for r in cur:
        if "step_" in r[name] or "drag_" in r[name]:
            yield (r[name], tuple(r[i] for i in grid), tuple(r[i] for i in wg), r[lds], r[scratch])


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run()
    else:
        for n, g, w, lds, scratch in dispatches(sys.argv[2]):
            print(f"{n} grid {g} workgroup {w} lds {lds} scratch {scratch}")
