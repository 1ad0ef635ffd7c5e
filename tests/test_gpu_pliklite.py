"""GPU parity of the binned-bandpower Gaussian likelihood (planck_pliklite.py:143-155) through the
C ABI: against golden G13 (the reference's own `get_chi_squared` run on a synthetic
plik-lite-shaped data set -- the Planck data is not available offline) at rtol 1e-12, and BIT-EXACT
against the oracle (oracle/mcmc_oracle.c: orc_binned) for evaluations and Metropolis steps."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from cobaya_amd import engine as E  # noqa: E402
from cobaya_amd import pliklite as P  # noqa: E402
from oracle import cbind as O  # noqa: E402
from tests.binned_cases import permuted_problem  # noqa: E402
from tests.pliklite_common import load_g13, sampling_problem, small_dataset  # noqa: E402
from tests.test_gpu_parity import assert_bit_equal, compare_state  # noqa: E402

RTOL = 1e-12   # the tolerance of the verdict's G13 bar (summation orders differ from numpy's BLAS)


def make(target, emu, W=64, gs=64, seed=5, T=1.0, max_tries=None, calib=None):
    """Engine and oracle problem of one target; `calib`: position of the calibration parameter
    among the sampled ones (default: last)."""
    d = emu.n + 1
    calib = emu.n if calib is None else calib
    kinds, a, b, C = permuted_problem(target, emu, calib)     # (calib = emu.n: sampling_problem's own)
    eng = E.Engine(d, W, group_size=gs, seed=seed, temperature=T, max_tries=max_tries)
    eng.set_prior(kinds, a, b)
    eng.set_target_binned_gaussian(target, emu, calib_index=calib)
    eng.set_proposal_cov(C * T)
    k = eng.binned_constants()
    B = O.Binned(target.bin_table(), target.weights, target.X_data, Linv=k["Linv"],
                 theta0=emu.theta0, D0=emu.D0, J=emu.J, calib=calib)
    # the library's binned response is the oracle's, bit for bit (host fma chains both)
    assert_bit_equal(k["Bc0"], B.Bc0, "Bc0")
    assert_bit_equal(k["BJ"], B.BJ, "BJ")
    prob = O.Problem(d, kinds, a, b, T=eng.get_proposal_transform(), group_size=gs, seed=seed,
                     temperature=T, max_tries=max_tries, derived=eng.derived_constants(), binned=B)
    return eng, prob, B, C


def test_chi2_against_reference_golden_g13():
    g, ds = load_g13()
    target = P.BinnedGaussian.from_dataset(ds)
    emu = P.synthetic_emulator(26, ds.lmax)
    eng, prob, B, _ = make(target, emu)
    # the inverse Cholesky factor the library derived (functions.py:81-89 of cov)
    np.testing.assert_allclose(eng.binned_constants()["Linv"],
                               np.linalg.inv(np.linalg.cholesky(target.cov)), rtol=1e-9, atol=1e-13)
    # (a) explicit spectra, L0 = 0 and L0 = 2: get_chi_squared's own signature
    raw = g["raw_cl"].astype(np.float64)
    for L0 in (0, 2):
        sel = g["raw_L0"] == L0
        got = eng.evaluate_binned(L0, raw[sel][:, :, L0:], g["raw_A"][sel])
        np.testing.assert_allclose(got, g["raw_chi2"][sel], rtol=RTOL)
        assert_bit_equal(got, B.chi2_of_cl(L0, raw[sel][:, :, L0:], g["raw_A"][sel]), "raw vs oracle")
    # (b) 64 parameter points of the emulator: explicit spectra and the sampler's own path
    cl = np.array([emu.cl(t) for t in g["emu_theta"]])
    assert np.array_equal(cl.sum(axis=2), g["emu_clsum"])   # the inputs the reference saw
    np.testing.assert_allclose(eng.evaluate_binned(0, cl, g["emu_A"]), g["emu_chi2"], rtol=RTOL)
    x = np.column_stack((g["emu_theta"], g["emu_A"]))
    lp, ll = eng.evaluate(x)
    np.testing.assert_allclose(-2.0 * ll, g["emu_chi2"], rtol=RTOL)
    olp, oll = prob.evaluate(x)
    assert_bit_equal(ll, oll, "loglike vs oracle")
    assert_bit_equal(lp, olp, "logprior vs oracle")
    # outside the prior support the likelihood is skipped (model.py:650-653)
    xo = x[:3].copy()
    xo[:, 0] = 1e3
    lp, ll = eng.evaluate(xo)
    assert np.all(np.isneginf(lp)) and np.all(np.isneginf(ll))


@pytest.mark.parametrize("tag,kw", [
    ("tt", dict(use_cl=["tt"])),
    ("bins", dict(use_bins=list(range(10, 120, 3)))),
    ("lrange", dict(use_cl=["te", "ee"], bins_for_L_range=[500, 1200]))])
def test_bin_and_spectrum_selections_against_g13(tag, kw):
    """planck_pliklite.py:84-125 (`use_cl`, `use_bins`, `bins_for_L_range`): other bin counts,
    i.e. other tile geometries of the chi2 kernel (215, 111 and 156 bins)."""
    g, ds = load_g13()
    target = P.BinnedGaussian.from_dataset(ds, **kw)
    assert np.array_equal(target.used_indices, g[f"sel_{tag}_used_indices"])
    emu = P.synthetic_emulator(26, ds.lmax)
    eng, prob, B, _ = make(target, emu)
    x = np.column_stack((g["emu_theta"][:8], g["emu_A"][:8]))
    lp, ll = eng.evaluate(x)
    np.testing.assert_allclose(-2.0 * ll, g[f"sel_{tag}_chi2"], rtol=RTOL)
    assert_bit_equal(ll, prob.evaluate(x)[1], "loglike vs oracle")


@pytest.mark.parametrize("case,W,gs,steps,T", [
    ("small", 256, 64, 45, 1.0), ("small", 128, 128, 30, 2.0), ("full", 128, 64, 12, 1.0),
    ("330", 64, 64, 9, 1.0), ("414", 128, 64, 9, 1.0)])
def test_binned_steps_bit_exact(case, W, gs, steps, T):
    """(88, 613, 330 and 414 bins: one, five, three and four row tiles per wave of the chi2 kernel)"""
    kw = {}
    if case == "small":
        ds = small_dataset()
        n_lin = 5
    else:
        _, ds = load_g13()
        n_lin = 26 if case == "full" else 7
        kw = {"330": dict(use_bins=list(range(110))), "414": dict(use_cl=["tt", "te"])}.get(case, {})
    target = P.BinnedGaussian.from_dataset(ds, **kw)
    assert target.n_bins == {"small": 88, "full": 613}.get(case) or target.n_bins == int(case)
    emu = P.synthetic_emulator(n_lin, ds.lmax)
    eng, prob, B, C = make(target, emu, W=W, gs=gs, T=T)
    rng = np.random.default_rng(77)
    x0 = np.concatenate((emu.theta0, [1.0])) + rng.standard_normal((W, emu.n + 1)) @ np.linalg.cholesky(C).T
    eng.set_state(x0)
    st = O.State(prob, x0)
    compare_state(eng, st)
    for n in (1, steps // 3, steps - steps // 3 - 1):   # launches that start and stop mid-cycle
        eng.step(n)
        eng.sync()
        st.run(n, n_threads=4)
        compare_state(eng, st)
    c = eng.counters()
    assert c["steps"] == steps and c["accepted"] == int(st.n_accept.sum())
    assert 0.05 < c["accepted"] / (W * steps) < 0.9
    assert "pl_fused_kernel" in eng.last_step_kernel()


def test_binned_target_refuses_what_it_does_not_cover():
    ds = small_dataset()
    target = P.BinnedGaussian.from_dataset(ds)
    emu = P.synthetic_emulator(5, ds.lmax)
    kinds, a, b, C = sampling_problem(target, emu)
    inc = E.Engine(6, 64, incremental=True)
    inc.set_prior(kinds, a, b)
    with pytest.raises(E.EngineError, match="from scratch"):
        inc.set_target_binned_gaussian(target, emu, calib_index=5)
    eng = E.Engine(6, 64)
    eng.set_prior(kinds, a, b)
    bad = P.BinnedGaussian.from_dataset(ds)
    bad.cov = bad.cov.copy()
    bad.cov[0, 0] = -1.0
    with pytest.raises(E.NotPositiveDefinite):
        eng.set_target_binned_gaussian(bad, emu, calib_index=5)
    with pytest.raises(ValueError, match="shape"):   # d - 1 emulator parameters, no other count
        eng.set_target_binned_gaussian(target, P.synthetic_emulator(4, ds.lmax), calib_index=4)
    with pytest.raises(E.EngineError, match="calibration"):
        eng.set_target_binned_gaussian(target, emu, calib_index=9)


def test_binned_target_posterior_on_the_device_at_the_baseline_size():
    """VERDICT r3 item 9 (Tier C for the plik-lite target, so far on the CPU oracle only): 65 536
    walkers on the 613-bin target through the sampler; the posterior of (theta, A_planck) is
    Gaussian to a very good approximation (Cl linear in theta, the calibration pinned by its
    0.25 % prior): the pooled ensemble must reproduce the EXACT posterior moments (theta integrated
    out in closed form, A on a grid) to 1 % of sigma / 1.5 % -- the north star's bar."""
    from cobaya_amd import pliklite as Pk
    from cobaya_amd.model import ProblemSpec
    from cobaya_amd.sampler import MCMCHip
    ds = Pk.synthetic_dataset(0)
    target = Pk.BinnedGaussian.from_dataset(ds)
    emu = Pk.synthetic_emulator(26, ds.lmax)
    C = Pk.fisher_covariance(target, emu)
    sig = np.sqrt(np.diag(C))
    params = {n: {"prior": {"min": float(emu.theta0[i] - 8 * sig[i]), "max": float(emu.theta0[i] + 8 * sig[i])},
                  "ref": {"dist": "norm", "loc": float(emu.theta0[i]), "scale": float(sig[i])}}
              for i, n in enumerate(emu.names)}
    params["A_planck"] = {"prior": {"dist": "norm", "loc": 1.0, "scale": 0.0025},
                          "ref": {"dist": "norm", "loc": 1.0, "scale": 0.002}}
    info = {"likelihood": {"plik": {"class": "planck_pliklite", "dataset": ds, "cl_emulator": emu}},
            "params": params}
    s = MCMCHip({"seed": 12, "n_walkers": 65536, "steps_per_launch": 54, "covmat": C,
                 "covmat_params": list(params), "learn_proposal": False, "Rminus1_stop": 0.0,
                 "snapshot_every": 540, "max_samples": 65536 * 540 * 10 * 0.4, "max_rows": 1 << 21},
                ProblemSpec.from_info(info))
    s.run()
    assert "pl_fused_kernel<5>" in s.engine.last_step_kernel()
    coll = s.products(skip_samples=0.45)["sample"]
    assert len(coll) >= 4 * 65536
    # EXACT reference moments: given A the posterior is Gaussian in theta (Cl is linear in theta), so
    # theta is integrated out in closed form -- its conditional mean th(A), covariance F^-1 A^4 and
    # the marginal p(A) ~ A^(2n) exp(-chi2_min(A) / 2) N(A; 1, 0.0025) (the A^(2n) is the volume of
    # the conditional: it moves <A> by 2 n sigma_A^2 = 0.13 sigma, which a Gaussian approximation
    # at the fiducial point misses) -- and A on a grid
    n = emu.n
    tab = target.bin_table()
    Bm = np.zeros((target.n_bins, n))
    cl0 = np.zeros(target.n_bins)
    for ib, (tp, a_, b_) in enumerate(tab):
        wv = target.weights[a_:b_ + 1]
        Bm[ib] = wv @ emu.J[tp, a_:b_ + 1, :]
        cl0[ib] = wv @ emu.D0[tp, a_:b_ + 1]
    Si = np.linalg.inv(target.cov)
    F = Bm.T @ Si @ Bm
    Fi = np.linalg.inv(F)
    grid = 1.0 + 0.0025 * np.linspace(-7, 7, 561)
    logp, th = np.empty(len(grid)), np.empty((len(grid), n))
    for k, A in enumerate(grid):
        sc = 1.0 / (A * A)
        r0 = target.X_data - sc * cl0
        g = Bm.T @ (Si @ r0)
        th[k] = emu.theta0 + (Fi @ g) / sc
        logp[k] = -0.5 * (r0 @ Si @ r0 - g @ Fi @ g) + 2 * n * np.log(A) - 0.5 * ((A - 1.0) / 0.0025) ** 2
    pA = np.exp(logp - logp.max())
    pA /= pA.sum()
    mA = pA @ grid
    mth = pA @ th
    mean = np.concatenate((mth, [mA]))
    cov = np.zeros((n + 1, n + 1))
    cov[:n, :n] = Fi * (pA @ grid ** 4) + (th - mth).T @ ((th - mth) * pA[:, None])
    cov[:n, n] = cov[n, :n] = (th - mth).T @ (pA * (grid - mA))
    cov[n, n] = pA @ (grid - mA) ** 2
    sig = np.sqrt(np.diag(cov))
    acc = s.engine.counters()
    assert 0.1 < acc["accepted"] / (acc["steps"] * 65536) < 0.5
    assert np.max(np.abs(coll.mean() - mean) / sig) < 0.01
    assert np.max(np.abs(coll.cov() - cov) / np.outer(sig, sig)) < 0.015
    s.close()
