"""The binned Gaussian (plik-lite) target on the device at EVERY kernel geometry, bit for bit against
the oracle: all 20 `pl_fused_kernel<NG, NP>`, every shift of the row-tile deal, `n_bins` from 1 to
the limit 640, the calibration parameter first, in the middle and last, two sets of walkers per
workgroup (`batches = 2`), the evaluate path (`pl_residual_mfma_kernel<np>` -> `pl_chi2_kernel<ntw>`)
at the same shapes, extreme calibration values, the refusals at the limits, and -- each in a child
process of its own -- the round-3 kernels behind MCMC_HIP_PL_SCALAR_RESIDUAL and MCMC_HIP_PL_UNFUSED.
The cases and what they cover: tests/binned_cases.py (asserted in tests/test_binned_cases_host.py,
where the oracle itself is pinned against a longdouble reference at every shape)."""
import contextlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from cobaya_amd import engine as E  # noqa: E402
from cobaya_amd import pliklite as P  # noqa: E402
from oracle import cbind as O  # noqa: E402
from tests import binned_cases as BC  # noqa: E402
from tests.test_gpu_parity import assert_bit_equal, compare_state  # noqa: E402
from tests.test_gpu_pliklite import make  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
SWEPT = [c for c in BC.STEP_CASES if c not in BC.HELD_BACK]


def run_steps(case, calls, kernel):
    """One engine and one oracle problem of `case`; a state around the fiducial point; `calls`
    step calls with the whole state compared after each.  Returns the accepted count and the
    kernel's name."""
    n_bins, n_lin, calib, W, gs = case
    target, emu = BC.target_of(n_bins), BC.emulator_of(n_lin, n_bins)
    eng, prob, B, C = make(target, emu, W=W, gs=gs, seed=BC.STEP_SEED, calib=calib)
    with contextlib.closing(eng):      # (a failing case does not keep its engine for the rest of the session)
        x0 = BC.start_points(emu, C, calib, W)
        eng.set_state(x0)
        st = O.State(prob, x0)
        compare_state(eng, st)
        for n in calls:   # a call ends on an accept-only launch, the next starts with a propose-only one
            eng.step(n)
            eng.sync()
            st.run(n, n_threads=4)
            compare_state(eng, st)
            assert kernel in eng.last_step_kernel(), eng.last_step_kernel()
        c = eng.counters()
        acc = int(st.n_accept.sum())
        assert c["steps"] == sum(calls) and c["accepted"] == acc
        # no acceptance band (one bin and 31 parameters: most directions are held by the prior
        # alone), but a run that only accepts or only rejects shows nothing
        assert 0 < acc < W * sum(calls), acc
        return acc, eng.last_step_kernel()


@pytest.mark.parametrize("case", SWEPT, ids=BC.case_id)
def test_steps_bit_exact(case):
    g = BC.geometry(case[0], case[1])
    run_steps(case, BC.calls_of(case), f"pl_fused_kernel<{g['NG']}>")


def spectra(emu, theta):
    """D_l of the emulator for many points at once: [n][3][lmax + 1]."""
    return emu.D0[None] + np.einsum("tlp,np->ntl", emu.J, theta - emu.theta0)


def check_evaluations(eng, prob, B, emu, calib, x, counts):
    olp, oll = prob.evaluate(x)
    for n in counts:      # (the lanes that pad a set of 64 repeat point 0)
        lp, ll = eng.evaluate(x[:n])
        assert_bit_equal(ll, oll[:n], f"loglike of {n} points")
        assert_bit_equal(lp, olp[:n], f"logprior of {n} points")
    theta, A = np.delete(x, calib, axis=1), x[:, calib]
    cl = spectra(emu, theta)
    for L0 in (0, 2):     # get_chi_squared's own arguments; at L0 = 2 the rows start at l = 2
        part = np.ascontiguousarray(cl[:, :, L0:])
        assert_bit_equal(eng.evaluate_binned(L0, part, A), B.chi2_of_cl(L0, part, A), f"L0 = {L0}")


@pytest.mark.parametrize("shape", BC.shapes(SWEPT), ids=lambda s: "-".join(map(str, s)))
def test_evaluate_every_geometry(shape):
    """pl_prior_kernel -> pl_residual_mfma_kernel<np> -> pl_chi2_kernel<ntw> -> pl_combine_kernel, and
    pl_bin_kernel in front of the chi2 for explicit spectra.  (`make` compares Bc0 and BJ of the
    library with the oracle's collapse, bit for bit.)"""
    n_bins, n_lin, calib = shape
    target, emu = BC.target_of(n_bins), BC.emulator_of(n_lin, n_bins)
    eng, prob, B, C = make(target, emu, calib=calib)
    with contextlib.closing(eng):
        x = BC.start_points(emu, C, calib, 65, seed=300 + n_bins)
        check_evaluations(eng, prob, B, emu, calib, x, (1, 63, 64, 65))


def test_evaluate_in_batches():
    """16 449 points: 16 512 lanes, 258 sets of 64, `batches = 2` in pl_chi2_kernel (129 workgroups
    of two sets each).  A data set of its own (l <= 600): the explicit spectra of so many points at
    lmax = 2508 would be 1 GB."""
    ds = P.synthetic_dataset(seed=3, lmin=30, lmax=600, nbin_pol=30, band=4)
    assert ds.nbins >= 129
    for n_bins, n_lin, calib in ((88, 5, 5), (129, 9, 0)):
        target, emu = BC.first_bins(ds, n_bins), P.synthetic_emulator(n_lin, ds.lmax)
        eng, prob, B, C = make(target, emu, calib=calib)
        with contextlib.closing(eng):
            x = BC.start_points(emu, C, calib, BC.BATCH_W + 1, seed=41)
            check_evaluations(eng, prob, B, emu, calib, x, (BC.BATCH_W + 1,))


def test_calibration_values():
    """`evaluate` at calibrations far from 1, the calibration parameter under a flat prior over
    +-1e300 (under the reference's N(1, 0.0025) the log-prior itself overflows to -inf at 1e200 and
    the likelihood is skipped: the last lines).  The sign of A does not matter (A * A); at 1e-3 and
    1e3 chi2 is large and finite.  A = 1e200: A * A overflows, 1 / A^2 is +0 and delta = X exactly.
    A = 1e-160: A * A underflows to 0, 1 / A^2 is +inf, the residuals are +-inf and the triangular
    product mixes their signs.  There device and oracle must agree on finite / infinite / NaN, and
    bit for bit wherever the value is a number.  Observed on the MI355X: docs/KERNELS.md, "Every
    geometry once"."""
    n_bins, n_lin, calib = 65, 8, 3
    d = n_lin + 1
    target, emu = BC.target_of(n_bins), BC.emulator_of(n_lin, n_bins)
    kinds, a, b, C = BC.permuted_problem(target, emu, calib)
    kinds[calib], a[calib], b[calib] = 0, -1e300, 1e300
    eng = E.Engine(d, 64, seed=BC.STEP_SEED)
    with contextlib.closing(eng):
        eng.set_prior(kinds, a, b)
        eng.set_target_binned_gaussian(target, emu, calib_index=calib)
        eng.set_proposal_cov(C)
        B = O.Binned(target.bin_table(), target.weights, target.X_data, Linv=eng.binned_constants()["Linv"],
                     theta0=emu.theta0, D0=emu.D0, J=emu.J, calib=calib)
        prob = O.Problem(d, kinds, a, b, T=eng.get_proposal_transform(), seed=BC.STEP_SEED,
                         derived=eng.derived_constants(), binned=B)
        A = np.array([1.0, -1.0, 1e-3, 1e3, 1e200, 1e-160])
        fid = BC.fiducial(emu, calib)
        off = BC.start_points(emu, 4.0 * C, calib, 1, seed=9)[0]
        for name, point in (("fiducial", fid), ("off-centre", off)):
            x = np.tile(point, (len(A), 1))
            x[:, calib] = A
            lp, ll = eng.evaluate(x)
            olp, oll = prob.evaluate(x)
            print(f"{name}: A = {A.tolist()}\n  device loglike {ll.tolist()}\n  oracle loglike {oll.tolist()}")
            assert_bit_equal(lp, olp, "logprior")
            assert np.all(np.isfinite(lp))
            for kind in (np.isnan, np.isposinf, np.isneginf):
                assert np.array_equal(kind(ll), kind(oll)), (name, ll, oll)
            ok = ~np.isnan(oll)
            assert_bit_equal(ll[ok], oll[ok], "loglike where it is a number")
            assert_bit_equal(ll[1:2], ll[0:1], "A = -1 against A = 1")
            assert np.all(np.isfinite(ll[:5])) and np.all(ll[:5] < 0)
            # 1 / A^2 = 0: chi2 of delta = X, whatever theta is
            assert_bit_equal(ll[4:5], -0.5 * B.chi2_of_delta(target.X_data), "A = 1e200")
    # the reference's prior on the calibration: at 1e200 its log-density overflows to -inf, and
    # the likelihood of such a point is skipped (model.py:650-653), as outside the support
    eng, prob, B, C = make(target, emu, calib=calib)
    with contextlib.closing(eng):
        x = np.tile(fid, (2, 1))
        x[1, calib] = 1e200
        lp, ll = eng.evaluate(x)
        assert np.isfinite(lp[0]) and np.isfinite(ll[0]) and np.isneginf(lp[1]) and np.isneginf(ll[1])


def test_limits():
    """n_bins 640 and n_lin 31 (d = 32) are served (and stepped: STEP_CASES); 641 bins, a calibration
    index outside 0..d-1 and d = 33 are refused."""
    emu = BC.emulator_of(31)
    eng, prob, B, C = make(BC.target_of(640), emu, calib=31)
    with contextlib.closing(eng):
        assert eng.n_bins == 640 and eng.d == 32
        with pytest.raises(E.EngineError, match=r"1\.\.640"):
            eng.set_target_binned_gaussian(BC.target_of(641), emu, calib_index=31)
        for bad in (-1, 32):
            with pytest.raises(E.EngineError, match="calibration"):
                eng.set_target_binned_gaussian(BC.target_of(16), emu, calib_index=bad)
    wide = P.LinearClEmulator(theta0=np.zeros(32), D0=emu.D0,
                              J=np.concatenate((emu.J, emu.J[:, :, :1]), axis=2), names=[])
    with contextlib.closing(E.Engine(33, 64)) as big:
        big.set_prior(np.zeros(33, np.int32), -np.ones(33), np.ones(33))
        with pytest.raises(E.EngineError, match="d <= 32"):
            big.set_target_binned_gaussian(BC.target_of(16), wide, calib_index=32)


def run_variant(variant, switch):
    """The worker in a fresh child with `switch` set (the library reads it once per process).  The
    return code is looked at before anything else: a child that faulted, aborted or ran out of
    time fails the test here, and the caller starts no other child."""
    env = dict(os.environ)
    env.pop("MCMC_HIP_PL_SCALAR_RESIDUAL", None)
    env.pop("MCMC_HIP_PL_UNFUSED", None)
    env[switch] = "1"
    out = subprocess.run([sys.executable, os.path.join(HERE, "_binned_variant_worker.py"), variant],
                         capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0, f"{variant}: return code {out.returncode}\n" + out.stdout[-2000:] + out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")]
    assert lines, out.stdout[-2000:] + out.stderr[-3000:]
    return json.loads(lines[-1][len("RESULT "):])


def test_round3_kernels_in_a_child():
    """`pl_residual_kernel<4 .. 32>` (evaluate) and the step through `pl_residual_mfma_kernel` +
    `pl_chi2_kernel` instead of the fused kernel: shipped, reachable through two developer
    switches, and run by nothing else.  One child per switch, one after the other."""
    assert "MCMC_HIP_PL_SCALAR_RESIDUAL" not in os.environ and "MCMC_HIP_PL_UNFUSED" not in os.environ
    r = run_variant("scalar", "MCMC_HIP_PL_SCALAR_RESIDUAL")
    assert r["complete"] and [tuple(c["case"]) for c in r["cases"]] == BC.SCALAR_CASES
    assert all(c["equal"] for c in r["cases"]), [c for c in r["cases"] if not c["equal"]]
    r = run_variant("unfused", "MCMC_HIP_PL_UNFUSED")
    assert r["complete"] and [tuple(c["case"]) for c in r["cases"]] == BC.UNFUSED_CASES
    assert all(c["equal"] for c in r["cases"]), [c for c in r["cases"] if not c["equal"]]
    for c in r["cases"]:
        assert f"pl_chi2_kernel<{BC.geometry(c['case'][0], c['case'][1])['ntw']}>" in c["kernel"], c
