"""Writes tests/golden/inc_supported_parent.npz: the answers of mcmc_hip_incremental_supported over
a grid of shapes, as packed bits.

The committed file was generated from a library BUILT AT THE PARENT of the commit that moved the
rule into cobaya_amd/csrc/inc_choice.h (a scratch checkout of that parent, selected with
MCMC_HIP_LIB): tests/test_host_logic.py asserts that the library of this tree gives the same
table, shape by shape.  Regenerate it only from a library whose rule is known to be right:

    MCMC_HIP_LIB=/path/to/libmcmc_hip.so python tests/golden/make_golden_inc_supported.py

The grid (n_periodic = -1 stands for "all d parameters"):
    d in 1..129, K in {0, 1..8, 16, 17, 64, 65}, n_periodic in {0, 1, 8, 16, 17, d},
    n_drag in {0, 1, 4, 7, 15}, (n_walkers, basis_group_size) in {(65536, 256), (65536, 4096), (256, 64)}
in C order of (d, K, n_periodic, n_drag, ensemble).  No device is touched."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(ROOT, "tests", "golden", "inc_supported_parent.npz")

AXES = dict(
    d=np.arange(1, 130, dtype=np.int32),
    n_modes=np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, 16, 17, 64, 65], dtype=np.int32),
    n_periodic=np.array([0, 1, 8, 16, 17, -1], dtype=np.int32),
    n_drag=np.array([0, 1, 4, 7, 15], dtype=np.int32),
    ensemble=np.array([[65536, 256], [65536, 4096], [256, 64]], dtype=np.int32),
)


def shapes(axes=AXES):
    """Every (d, n_modes, n_periodic, n_drag, n_walkers, basis_group_size) of the grid, in order."""
    for d in axes["d"]:
        for K in axes["n_modes"]:
            for per in axes["n_periodic"]:
                for nd in axes["n_drag"]:
                    for W, bgs in axes["ensemble"]:
                        yield int(d), int(K), int(d if per < 0 else per), int(nd), int(W), int(bgs)


def table(lib, axes=AXES):
    return np.array([lib.mcmc_hip_incremental_supported(*s) for s in shapes(axes)], dtype=np.uint8)


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    from cobaya_amd import engine as E
    answers = table(E.load_library())
    np.savez_compressed(OUT, bits=np.packbits(answers), n=np.int64(answers.size), **AXES)
    print(f"{OUT}: {answers.size} shapes, {int(answers.sum())} served, {os.path.getsize(OUT)} bytes")
