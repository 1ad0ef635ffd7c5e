"""The commit of step_inc_duo_kernel (incremental_duo.hip: one mode, two lanes per walker) runs on the accepting lanes
alone (round 20): x takes the step's trial, y moves on with r, the carried values and the bookkeeping are written under
the accept mask, and a rejecting lane is not touched -- what the oracle does (step_core_inc -> commit).  Every case is
the C oracle's state bit for bit on the forced two-lane kernel (MCMC_HIP_DUO=1), 256 walkers in groups of 128: x, y,
logpost, logprior, loglike, weight, prior_rej, n_accept, burn_left, the accept total and the stuck flag.  What a case
is meant to exercise is first checked on the oracle's own numbers (it accepts nothing / nearly everything / as
bench.py does)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from cobaya_amd import engine as E  # noqa: E402
from oracle import cbind as O  # noqa: E402
from tests.test_gpu_parity import assert_bit_equal, compare_state  # noqa: E402

TWO = "two lanes"
W, GS = 256, 128
# NE = 1, 2, 15, 15, 16, 16 dimensions per lane: 3, 29 and 31 pad a row of lane 1.  (d = 1 has no incremental evaluation
# at all -- test_one_dimension_is_not_stepped_incrementally --, so the smallest walker of this kernel has d = 2.)
DIMS = [2, 3, 29, 30, 31, 32]
C30 = 60                           # incremental_duo.hip: duo1_chunk(8), the columns of a chunk at d = 30


def lengths(d):
    """launches of 1, 7, 8 and 9 steps; at d = 30 also a chunk - 1, a chunk + 1 and two chunks + 1"""
    return (1, 7, 8, 9) + ((C30 - 1, C30 + 1, 2 * C30 + 1) if d == 30 else ())


def target(d, sigma=0.05, seed=0):
    """one Gaussian mode in the middle of [0, 1]^d"""
    rng = np.random.default_rng(2000 + 10 * d + seed)
    mean = rng.uniform(0.4, 0.6, size=d)
    A = rng.normal(size=(d, d))
    cov = (A @ A.T / d + np.eye(d) * 0.5) * sigma ** 2
    x0 = np.clip(mean + rng.normal(size=(W, d)) * np.sqrt(np.diag(cov)), 1e-3, 1 - 1e-3)
    return mean, cov, x0


def _pair(d, mean, cov, pcov, x0, hi=1.0, seed=5, T=1.0, burn_in=0, max_tries=None):
    eng = E.Engine(d, W, group_size=GS, seed=seed, temperature=T, burn_in=burn_in, max_tries=max_tries,
                   incremental=True)
    eng.set_prior([0] * d, [0.0] * d, [hi] * d)
    eng.set_target_gaussian_mixture([mean], [cov])
    eng.set_proposal_cov(pcov)
    prob = O.Problem(d, [0] * d, [0.0] * d, [hi] * d, means=mean, covs=cov, T=eng.get_proposal_transform(),
                     group_size=GS, seed=seed, temperature=T, max_tries=max_tries,
                     derived=eng.derived_constants(), incremental=True)
    eng.set_state(x0)
    return eng, prob, O.State(prob, x0, burn_in=burn_in)


def _check(eng, st):
    compare_state(eng, st)   # x, logpost, logprior, loglike, weight
    s = eng.get_full_state()
    assert_bit_equal(s["y"], st.y, "carried whitened residual")
    assert np.array_equal(s["prior_rej"], st.prior_rej)
    assert np.array_equal(s["n_accept"], st.n_accept)
    assert np.array_equal(s["burn_left"], st.burn_left)
    c = eng.counters()
    assert c["steps"] == st.step and c["accepted"] == int(st.n_accept.sum())


def _call(eng, st, n, unit_t=True):
    """one launch on both sides -> (the engine reported a stuck chain, the oracle did)"""
    eng.step(n)
    try:
        eng.sync()
        stuck = False
    except E.ChainStuck:
        stuck = True
    st.run(n, n_threads=8)
    name = eng.last_step_kernel()
    assert "step_inc_kernel" in name and TWO in name and (", true," in name) == unit_t, name
    return stuck, bool(st.stuck[0] != 0)


def _run(eng, st, d, unit_t=True):
    _check(eng, st)
    for n in lengths(d):
        assert _call(eng, st, n, unit_t) == (False, False)
        _check(eng, st)


def test_one_dimension_is_not_stepped_incrementally(monkeypatch):
    """the engine refuses incremental evaluation at d = 1: no launch of this kernel has a walker of one dimension"""
    monkeypatch.setenv("MCMC_HIP_DUO", "1")
    with pytest.raises(E.EngineError, match="d >= 2"):
        E.Engine(1, W, group_size=GS, seed=5, incremental=True)


# ---------------------------------------------------------------- no lane accepts
FAR = 1.0e16   # the proposal's variance: a trial is ~10^8 box widths away


def _never(d, x0, mean, cov):
    eng, prob, st = _pair(d, mean, cov, np.eye(d) * FAR, x0)
    _run(eng, st, d)
    # (the oracle's own numbers: nothing accepted, every trial outside the box, x untouched)
    assert int(st.n_accept.sum()) == 0
    assert np.all(st.prior_rej == st.step) and np.all(st.weight == 1 + st.step)
    assert_bit_equal(st.x, x0, "the oracle's x")
    assert_bit_equal(eng.get_state()["x"], x0, "x")
    eng.close()


@pytest.mark.parametrize("d", DIMS)
def test_a_wave_without_an_accepting_lane_changes_nothing(d, monkeypatch):
    monkeypatch.setenv("MCMC_HIP_DUO", "1")
    mean, cov, x0 = target(d)
    _never(d, x0, mean, cov)


@pytest.mark.parametrize("d", DIMS)
def test_a_rejecting_lane_keeps_minus_zero_and_a_coordinate_on_hi(d, monkeypatch):
    """x = -0.0 is inside [0, hi] and so is x = hi.  A commit that adds 0 * v to the coordinates of a rejecting lane
    turns -0.0 into +0.0 at the first v > 0; the oracle leaves it alone."""
    monkeypatch.setenv("MCMC_HIP_DUO", "1")
    mean, cov, x0 = target(d, seed=1)
    x0[:, 0] = -0.0
    x0[:, d - 1] = 1.0
    assert np.signbit(x0[0, 0]) and x0[1, d - 1] == 1.0
    _never(d, x0, mean, cov)


# ---------------------------------------------------------------- nearly every lane accepts
@pytest.mark.parametrize("d", DIMS)
def test_nearly_every_lane_accepts_at_a_very_high_temperature(d, monkeypatch):
    """T = 10^8 (the UNIT_T = false instantiation) with a proposal a tenth of the target's width: the trials stay
    inside and Ea > delta / T nearly always."""
    monkeypatch.setenv("MCMC_HIP_DUO", "1")
    mean, cov, x0 = target(d, seed=2)
    eng, prob, st = _pair(d, mean, cov, cov * 0.01, x0, T=1.0e8)
    _run(eng, st, d, unit_t=False)
    assert int(st.n_accept.sum()) >= 0.95 * W * st.step   # (of ALL trials, so of the inside ones)
    eng.close()


# ---------------------------------------------------------------- the benchmark's regime
@pytest.mark.parametrize("d", DIMS)
def test_the_benchmarks_regime(d, monkeypatch):
    """the proposal is the target's covariance: the oracle's acceptance is inside bench.py's gate"""
    monkeypatch.setenv("MCMC_HIP_DUO", "1")
    mean, cov, x0 = target(d, seed=3)
    eng, prob, st = _pair(d, mean, cov, cov, x0)
    _run(eng, st, d)
    rate = int(st.n_accept.sum()) / (W * st.step)
    assert 0.15 <= rate <= 0.5, rate
    eng.close()


# ---------------------------------------------------------------- burn-in
@pytest.mark.parametrize("d", [3, 30])
def test_burn_in_ends_inside_a_launch(d, monkeypatch):
    """burn_left = 6: a walker's burn-in ends with its sixth accepted step, at another step for every walker"""
    monkeypatch.setenv("MCMC_HIP_DUO", "1")
    mean, cov, x0 = target(d, seed=4)
    eng, prob, st = _pair(d, mean, cov, cov, x0, burn_in=5)
    assert np.all(st.burn_left == 6)
    _check(eng, st)
    seen = []
    for n in (1, 7, 8, 9, C30 - 1, C30 + 1):
        assert _call(eng, st, n) == (False, False)
        _check(eng, st)
        seen.append(int(np.count_nonzero(st.burn_left > 0)))
    assert any(0 < k < W for k in seen) and seen[-1] < seen[0]
    eng.close()


# ---------------------------------------------------------------- the limit of tries
def test_the_limit_of_tries_is_passed_inside_the_first_chunk(monkeypatch):
    """max_tries = 3 in the benchmark's regime: launches of 3 steps until the oracle raises its flag -- the engine
    raises its own in the same launch, not before"""
    monkeypatch.setenv("MCMC_HIP_DUO", "1")
    d = 30
    mean, cov, x0 = target(d, seed=5)
    eng, prob, st = _pair(d, mean, cov, cov, x0, max_tries=3)
    for k in range(20):
        got, want = _call(eng, st, 3)
        assert got == want, (k, got, want)
        if want:
            break
        _check(eng, st)
    assert want
    eng.close()


def test_the_limit_of_tries_is_passed_in_a_later_chunk_only(monkeypatch):
    """max_tries = 100.  Two chunks + 1 steps in the benchmark's regime end every walker's burn-in (its limit is ten
    times as high until then) and leave every wt - prej far below the limit; then a proposal twenty times as wide as
    the target, inside the box: nearly every trial is inside and rejected, wt - prej grows by one per step.  A launch
    of two chunks + 1 steps then passes the limit, and not in its first chunk: wt - prej grows by at most one per step
    and starts at most a chunk below the limit."""
    monkeypatch.setenv("MCMC_HIP_DUO", "1")
    d = 30
    mean, cov, x0 = target(d, sigma=0.002, seed=6)
    eng, prob, st = _pair(d, mean, cov, cov, x0, max_tries=100)
    assert _call(eng, st, 2 * C30 + 1) == (False, False)
    _check(eng, st)
    assert not np.any(st.burn_left > 0) and int((st.weight - st.prior_rej).max()) <= 100 - C30
    eng.set_proposal_cov(cov * 400.0)
    prob.set_T(eng.get_proposal_transform())
    got, want = _call(eng, st, 2 * C30 + 1)
    assert want and got
    eng.close()
