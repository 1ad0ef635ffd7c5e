"""One mode with TWO lanes per walker (step_inc_duo_kernel, incremental_duo.hip, round 7): the
incremental Metropolis step of one Gaussian mode on the box [0, hi], reported as
`step_inc_kernel<dq, 0, .., two lanes>`, walker for walker against the C oracle, bit for bit --
at the bench geometry (where the launcher takes it by itself), forced on small ensembles
(MCMC_HIP_DUO=1) over the dimensions around every padding case, at the wall of the box, through
burn-in and the stuck test, and on both sides of the ensemble size from which the launcher takes it."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from cobaya_amd import engine as E  # noqa: E402
from oracle import cbind as O  # noqa: E402
from tests.test_gpu_bench_geometry import _compare, _pair  # noqa: E402
from tests.test_gpu_parity import assert_bit_equal, compare_state, make_pair  # noqa: E402

TWO = "two lanes"
DUO1_MIN_WALKERS = 65536   # inc_choice.h: kDuo1MinWalkers


@pytest.mark.parametrize("offset", [0, 7 * 65536], ids=["rank0", "rank7-of-configs2"])
def test_config2_geometry_runs_on_two_lanes_bit_exact(offset):
    """BASELINE config 2 as bench.py runs it: 65 536 walkers, basis groups of 4 096, 1 200 steps per
    launch; three calls, the last one holding two launches (one direction set, the second launch
    refreshes y itself: anchor & 2, col0 > 0), a proposal refresh between the calls."""
    d, W, gs, bgs, spl = 30, 65536, 256, 4096, 1200
    threads = O.max_threads()
    eng, prob, st, mean, cov = _pair(d, W, gs, bgs, offset)
    for call in range(3):
        n = spl if call < 2 else 2 * spl
        eng.step(n)
        eng.sync()
        st.run(n, walker0=offset, n_threads=threads)
        _compare(eng, st, f"call {call}")
        kernel = eng.last_step_kernel()
        assert "step_inc_kernel" in kernel and TWO in kernel, kernel
        if call < 2:
            eng.set_proposal_cov(np.cov(st.x.T))
            prob.set_T(eng.get_proposal_transform())
    eng.close()


def _run_case(eng, st, d, steps):
    for n in steps:
        eng.step(n)
        eng.sync()
        st.run(n, n_threads=8)
        compare_state(eng, st)
        assert_bit_equal(eng.get_full_state()["y"], st.y, "carried whitened residual")
    c = eng.counters()
    assert c["steps"] == st.step and c["accepted"] == int(st.n_accept.sum())
    kernel = eng.last_step_kernel()
    assert "step_inc_kernel" in kernel and TWO in kernel, kernel
    return c


@pytest.mark.parametrize("d", [2, 3, 5, 8, 15, 16, 17, 29, 30, 31, 32])
def test_forced_small_ensembles_bit_exact(d, monkeypatch):
    """Launches that end mid-octet and mid-cycle, and one call across the refresh at 40 d steps (the
    launch inside the call refreshes y in the kernel)."""
    monkeypatch.setenv("MCMC_HIP_DUO", "1")
    W, gs = (256, 128) if d % 2 else (384, 128)
    eng, prob, st = make_pair(d, W, gs, incremental=True, rng=np.random.default_rng(9100 + d))
    compare_state(eng, st)
    R = 40 * d
    c = _run_case(eng, st, d, (1, 2, 7, d + 3, R - (d + 13) - 1, 5, 2 * d + 1))
    assert st.step > R
    assert 0.03 < c["accepted"] / (W * st.step) < 0.9
    eng.close()


@pytest.mark.parametrize("d", [5, 30])
def test_walkers_at_the_wall_take_the_exact_box_test(d, monkeypatch):
    """A posterior against both walls of [0, 1]: most trials of the walkers there leave the box, the
    high-word test cannot decide them and the exact comparisons run."""
    monkeypatch.setenv("MCMC_HIP_DUO", "1")
    W, gs = 256, 128
    eng = E.Engine(d, W, group_size=gs, seed=3, incremental=True)
    eng.set_prior([0] * d, [0.0] * d, [1.0] * d)
    rng = np.random.default_rng(77 + d)
    mean = np.where(np.arange(d) % 2 == 0, 0.015, 0.985)
    A = rng.normal(size=(d, d))
    cov = (A @ A.T / d + np.eye(d)) * 0.02 ** 2
    eng.set_target_gaussian_mixture([mean], [cov])
    eng.set_proposal_cov(cov)
    prob = O.Problem(d, [0] * d, [0.0] * d, [1.0] * d, means=mean, covs=cov,
                     T=eng.get_proposal_transform(), group_size=gs, seed=3,
                     derived=eng.derived_constants(), incremental=True)
    x0 = np.clip(mean + rng.normal(size=(W, d)) * 0.01, 1e-4, 1 - 1e-4)
    eng.set_state(x0)
    st = O.State(prob, x0)
    _run_case(eng, st, d, (3, 40 * d - 3, 17))
    assert int(st.prior_rej.sum()) > 0
    eng.close()


def test_burn_in_and_temperature_bit_exact(monkeypatch):
    monkeypatch.setenv("MCMC_HIP_DUO", "1")
    d = 30
    eng, prob, st = make_pair(d, 256, 128, incremental=True, burn_in=3, T=1.7,
                              rng=np.random.default_rng(4242))
    _run_case(eng, st, d, (1, 5, 37, 40 * d))
    eng.close()


def test_stuck_chain_is_reported_on_two_lanes(monkeypatch):
    """mcmc.py:717-743: a proposal far too wide trips max_tries."""
    monkeypatch.setenv("MCMC_HIP_DUO", "1")
    d = 3
    eng = E.Engine(d, 128, group_size=128, max_tries=20, incremental=True)
    eng.set_prior([0] * d, [0.0] * d, [1.0] * d)
    eng.set_target_gaussian_mixture([[0.5] * d], [np.eye(d) * 1e-8])
    eng.set_proposal_cov(np.eye(d) * 0.05)
    eng.set_state(np.full((128, d), 0.5))
    eng.step(400)
    with pytest.raises(E.ChainStuck):
        eng.sync()
    assert TWO in eng.last_step_kernel(), eng.last_step_kernel()


@pytest.mark.parametrize("W,two", [(DUO1_MIN_WALKERS - 16384, False), (DUO1_MIN_WALKERS, True)])
def test_the_launcher_takes_two_lanes_for_one_mode_from_the_measured_size_on(W, two):
    d, gs, bgs = 30, 256, 1024
    eng, prob, st, mean, cov = _pair(d, W, gs, bgs, 0)
    for n in (1, 75):
        eng.step(n)
        eng.sync()
        st.run(n, n_threads=O.max_threads())
        _compare(eng, st, f"{W} walkers")
    kernel = eng.last_step_kernel()
    assert "step_inc_kernel" in kernel and (TWO in kernel) == two, kernel
    eng.close()


def test_the_developer_switch_forces_four_lanes(monkeypatch):
    monkeypatch.setenv("MCMC_HIP_DUO", "0")
    d, W, gs, bgs = 30, 65536, 256, 4096
    eng, prob, st, mean, cov = _pair(d, W, gs, bgs, 0)
    eng.step(40)
    eng.sync()
    st.run(40, n_threads=O.max_threads())
    _compare(eng, st, "MCMC_HIP_DUO=0")
    kernel = eng.last_step_kernel()
    assert "step_inc_kernel" in kernel and TWO not in kernel, kernel
    eng.close()
