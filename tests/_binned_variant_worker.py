"""Worker of tests/test_gpu_binned_geometries.py::test_round3_kernels_in_a_child: the binned
Gaussian target with one of the library's developer switches set.  The library reads a switch once
per process, so every variant runs in a child of its own, started with the switch in its
environment:

    MCMC_HIP_PL_SCALAR_RESIDUAL=1 python tests/_binned_variant_worker.py scalar
    MCMC_HIP_PL_UNFUSED=1         python tests/_binned_variant_worker.py unfused

-> one line `RESULT {"complete": ..., "cases": [{"case": [...], "equal": ..., ...}, ...]}` on
stdout.  A case whose comparison fails is reported and the list goes on; anything else (an error
of the HIP runtime among them) ends the list there, `complete` false."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.dont_write_bytecode = True
sys.path[:0] = [ROOT]

SWITCH = {"scalar": "MCMC_HIP_PL_SCALAR_RESIDUAL", "unfused": "MCMC_HIP_PL_UNFUSED"}


def scalar_case(case):
    """`evaluate` through pl_residual_kernel<nlp> at 1, 64 and 65 points."""
    import numpy as np

    from tests import binned_cases as BC
    from tests.test_gpu_parity import assert_bit_equal
    from tests.test_gpu_pliklite import make
    n_bins, n_lin, calib = case
    target, emu = BC.target_of(n_bins), BC.emulator_of(n_lin, n_bins)
    eng, prob, B, C = make(target, emu, calib=calib)
    x = BC.start_points(emu, C, calib, 65, seed=500 + n_lin)
    olp, oll = prob.evaluate(x)
    try:
        for n in (1, 64, 65):
            lp, ll = eng.evaluate(x[:n])
            assert_bit_equal(ll, oll[:n], f"loglike of {n} points")
            assert_bit_equal(lp, olp[:n], f"logprior of {n} points")
        assert np.all(np.isfinite(oll))
    finally:
        eng.close()
    return {"nlp": BC.geometry(n_bins, n_lin)["nlp"]}


def unfused_case(case):
    """Nine steps through pl_walker_kernel, pl_residual_mfma_kernel and pl_chi2_kernel."""
    from tests import binned_cases as BC
    from tests.test_gpu_binned_geometries import run_steps
    acc, kernel = run_steps(tuple(case), BC.UNFUSED_CALLS, "pl_chi2_kernel")
    return {"accepted": acc, "kernel": kernel}


def main(variant):
    from tests import binned_cases as BC
    assert os.environ.get(SWITCH[variant]), f"{SWITCH[variant]} is not set"
    other = SWITCH["unfused" if variant == "scalar" else "scalar"]
    assert other not in os.environ, f"{other} is set too"
    cases, run = ((BC.SCALAR_CASES, scalar_case) if variant == "scalar" else (BC.UNFUSED_CASES, unfused_case))
    out, complete = [], True
    for case in cases:
        rec = {"case": list(case), "equal": False}
        out.append(rec)
        try:
            rec.update(run(case))
            rec["equal"] = True
        except AssertionError as e:
            rec["why"] = str(e)[:300]
        except Exception as e:       # the device or the runtime: nothing more is started on it
            rec["why"] = f"{type(e).__name__}: {e}"[:300]
            complete = False
            break
    print("RESULT " + json.dumps({"complete": complete, "cases": out}))
    return 0 if complete else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
