"""The step loop of step_inc_duo_kernel (incremental_duo.hip: one mode, two lanes per walker) after round 17: the
support test decided on the high words wherever they decide it (the exact comparisons only for a wave with a lane in
doubt), the steps taken octet by octet of the global step index inside a chunk, the stuck test gathered into a mask that
is looked at once per chunk, the burn-in bookkeeping behind the loop, |u|^2 staged into LDS with the chunk's columns.
None of it changes a result: every case is the C oracle's state bit for bit -- x, y, logpost, logprior, loglike,
weight, prior_rej, n_accept, burn_left -- on the forced two-lane kernel (MCMC_HIP_DUO=1), 256 walkers in groups of 128."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from cobaya_amd import engine as E  # noqa: E402
from oracle import cbind as O  # noqa: E402
from tests.test_gpu_parity import assert_bit_equal, compare_state, make_pair  # noqa: E402

TWO = "two lanes"
W, GS = 256, 128


def duo1_chunk(dq):   # incremental_duo.hip: duo1_chunk (test_gpu_staging_waits.py holds the formula to the source)
    return min(((80 * 1024 - 16896 - 2048) // (2 * 64 * dq)) & ~3, 64)


def _check(eng, st):
    compare_state(eng, st)
    s = eng.get_full_state()
    assert_bit_equal(s["y"], st.y, "carried whitened residual")
    assert np.array_equal(s["prior_rej"], st.prior_rej)
    assert np.array_equal(s["n_accept"], st.n_accept)
    assert np.array_equal(s["burn_left"], st.burn_left)


def _call(eng, st, n):
    eng.step(n)
    eng.sync()
    st.run(n, n_threads=8)
    _check(eng, st)
    name = eng.last_step_kernel()
    assert "step_inc_kernel" in name and TWO in name, name


def _box_pair(d, hi, mean, cov, x0, seed=3, **kw):
    """engine and oracle on the box [0, hi]^d with one Gaussian mode, the proposal its covariance"""
    eng = E.Engine(d, W, group_size=GS, seed=seed, incremental=True, **kw)
    eng.set_prior([0] * d, [0.0] * d, [hi] * d)
    eng.set_target_gaussian_mixture([mean], [cov])
    eng.set_proposal_cov(cov)
    prob = O.Problem(d, [0] * d, [0.0] * d, [hi] * d, means=mean, covs=cov, T=eng.get_proposal_transform(),
                     group_size=GS, seed=seed, derived=eng.derived_constants(), incremental=True, **kw)
    eng.set_state(x0)
    return eng, O.State(prob, x0)


# ---------------------------------------------------------------- walls
@pytest.mark.parametrize("d", [5, 30, 32])   # NE = 3, 15 and 16 dimensions per lane
def test_waves_with_lanes_inside_and_outside(d, monkeypatch):
    """The target's mean one sigma from the wall at 0 in the even coordinates and one sigma from hi in the odd ones:
    most wave-steps hold lanes inside and lanes outside the box, which the high words now decide without the exact
    comparisons.  300 steps in launches of odd lengths."""
    monkeypatch.setenv("MCMC_HIP_DUO", "1")
    rng = np.random.default_rng(1700 + d)
    sig = 0.02
    mean = np.where(np.arange(d) % 2 == 0, sig, 1.0 - sig)
    A = rng.normal(size=(d, d))
    cov = (A @ A.T / d + np.eye(d)) * (sig ** 2 / 2)
    x0 = np.clip(mean + rng.normal(size=(W, d)) * 0.01, 1e-4, 1 - 1e-4)
    eng, st = _box_pair(d, 1.0, mean, cov, x0)
    _check(eng, st)
    lengths = (1, 1, 37, 61, 75, 125)
    assert sum(lengths) == 300 and all(n % 2 for n in lengths)
    for n in lengths:
        _call(eng, st, n)
    assert int(st.prior_rej.sum()) > 0 and int(st.n_accept.sum()) > 0
    eng.close()


# ---------------------------------------------------------------- high words in doubt
def _doubt_case(hi, centre, sigma, inward, seed):
    """d = 5; coordinate 0 of the target and of the starting points centred on `centre` (a wall) with `sigma`, the
    other coordinates in the middle of the box"""
    d = 5
    rng = np.random.default_rng(seed)
    mean = np.full(d, 0.5)
    mean[0] = centre
    sd = np.full(d, 0.05)
    sd[0] = sigma
    cov = np.diag(sd ** 2)
    x0 = mean + rng.normal(size=(W, d)) * sd * 0.5
    x0[:, 0] = centre + inward * np.abs(rng.normal(size=W)) * sigma   # (the walkers start inside the box)
    assert np.all((x0 >= 0.0) & (x0 <= hi))
    return _box_pair(d, hi, mean, cov, x0, seed=11)


def _hi_word(v):
    return (np.asarray(v, dtype=np.float64).view(np.uint64) >> np.uint64(32)).astype(np.uint32)


def test_trials_whose_high_word_is_that_of_hi(monkeypatch):
    """hi = 1 + 2^-21 has the high word of 1.0: a trial in [1, 1 + 2^-20) is inside or outside by its LOW word.  One
    coordinate sits at hi with sigma = 2^-22, so a large share of the trials land in that slice on both sides of hi."""
    monkeypatch.setenv("MCMC_HIP_DUO", "1")
    hi = 1.0 + 2.0 ** -21
    assert _hi_word(hi) == _hi_word(1.0) == 0x3FF00000
    eng, st = _doubt_case(hi, hi, 2.0 ** -22, -1.0, 1721)
    assert np.mean(_hi_word(st.x[:, 0]) == 0x3FF00000) > 0.9   # (the walkers start in the slice)
    _check(eng, st)
    for n in (1, 7, 41, 64, 87):
        _call(eng, st, n)
    assert int(st.prior_rej.sum()) > 0 and int(st.n_accept.sum()) > 0
    assert np.mean(_hi_word(st.x[:, 0]) == 0x3FF00000) > 0.5   # (and stay in it)
    eng.close()


def test_trials_at_the_wall_at_zero(monkeypatch):
    """One coordinate at the wall 0 with sigma = 2^-40: the trials beyond the wall carry the sign bit."""
    monkeypatch.setenv("MCMC_HIP_DUO", "1")
    eng, st = _doubt_case(1.0, 0.0, 2.0 ** -40, 1.0, 1722)
    _check(eng, st)
    for n in (1, 7, 41, 64, 87):
        _call(eng, st, n)
    assert int(st.prior_rej.sum()) > 0 and int(st.n_accept.sum()) > 0
    eng.close()


# ---------------------------------------------------------------- stuck and burn-in
def _stuck_both(eng, st, n):
    """one call of n steps on both sides -> (the engine reported a stuck chain, the oracle did)"""
    eng.step(n)
    try:
        eng.sync()
        stuck = False
    except E.ChainStuck:
        stuck = True
    st.run(n, n_threads=8)
    name = eng.last_step_kernel()
    assert "step_inc_kernel" in name and TWO in name, name
    return stuck, bool(st.stuck[0] != 0)


def test_a_stuck_chain_is_reported_when_the_oracle_reports_it(monkeypatch):
    """max_tries = 3: launches of one step until the oracle raises its flag -- the engine raises its own in the same
    launch, not before (the mask of the lanes over the limit is looked at at the end of every chunk, so of every launch)."""
    monkeypatch.setenv("MCMC_HIP_DUO", "1")
    d = 30
    eng, prob, st = make_pair(d, W, GS, incremental=True, max_tries=3, rng=np.random.default_rng(1731))
    for k in range(60):
        got, want = _stuck_both(eng, st, 1)
        assert got == want, (k, got, want)
        if want:
            break
        _check(eng, st)
    # (a walker's limit is ten times as high until its first accepted step: an accept, then three rejections)
    assert want and k >= 3
    eng.close()


@pytest.mark.parametrize("d", [30, 5], ids=["dq8-C60", "dq2-C64"])
def test_a_chain_stuck_in_the_first_chunk_of_three_is_reported(d, monkeypatch):
    """A launch of 2 C + 1 steps whose limit is first exceeded in its first chunk: the walker may have accepted since."""
    monkeypatch.setenv("MCMC_HIP_DUO", "1")
    C = duo1_chunk((d + 3) // 4)
    eng, prob, st = make_pair(d, W, GS, incremental=True, max_tries=3, rng=np.random.default_rng(1732 + d))
    got, want = _stuck_both(eng, st, 2 * C + 1)
    assert want and got
    eng.close()


def test_no_flag_below_a_large_limit(monkeypatch):
    monkeypatch.setenv("MCMC_HIP_DUO", "1")
    d = 30
    C = duo1_chunk(8)
    eng, prob, st = make_pair(d, W, GS, incremental=True, max_tries=100000, rng=np.random.default_rng(1733))
    for n in (3, 2 * C + 1, C):
        got, want = _stuck_both(eng, st, n)
        assert not want and not got
        _check(eng, st)
    assert eng.counters()["stuck"] == 0
    eng.close()


@pytest.mark.parametrize("burn", [5, 70])
def test_burn_in_ends_inside_a_chunk_lane_by_lane(burn, monkeypatch):
    """burn_left = 5 and 70: a walker's burn-in ends with its burn-th accepted step -- inside a chunk, and at another
    step for every walker of a wave; the wave leaves the burning bookkeeping when its last walker has."""
    monkeypatch.setenv("MCMC_HIP_DUO", "1")
    d = 30
    C = duo1_chunk(8)
    eng, prob, st = make_pair(d, W, GS, incremental=True, burn_in=burn - 1, rng=np.random.default_rng(1740 + burn))
    _check(eng, st)
    assert np.all(st.burn_left == burn)
    seen = set()
    for n in (3, 9, 9, C + 1, 2 * C + 1, C - 1, 2 * C + 1, 2 * C + 1):
        _call(eng, st, n)
        seen.add(int(np.count_nonzero(st.burn_left > 0)))
    assert len(seen) > 1 and any(0 < k < W for k in seen)   # (walkers finished at different steps)
    if burn == 5:
        assert not np.any(st.burn_left > 0)
    eng.close()


# ---------------------------------------------------------------- geometry
@pytest.mark.parametrize("d", [30, 5], ids=["dq8-C60", "dq2-C64"])
def test_launches_of_every_length_from_inside_an_octet(d, monkeypatch):
    """Launches of 1, 7, 8, 9, C - 1, C, C + 1 and 2 C + 1 steps, each starting inside an octet of the global step index
    (the octet of the last launch's end is continued, a chunk ends inside one), some at an odd column of their
    direction set (|u|^2 is then 8-byte aligned only), and one call across the refresh of y at 40 d steps."""
    monkeypatch.setenv("MCMC_HIP_DUO", "1")
    monkeypatch.delenv("MCMC_HIP_ACCEPT_SLACK", raising=False)
    C = duo1_chunk((d + 3) // 4)
    assert C == (60 if d == 30 else 64)
    R = 40 * d
    eng, prob, st = make_pair(d, W, GS, incremental=True, rng=np.random.default_rng(1750 + d))
    _check(eng, st)
    _call(eng, st, 3)
    odd_starts = 0
    for n in (1, 7, 8, 9, C - 1, C, C + 1, 2 * C + 1):
        if st.step % 8 == 0:
            _call(eng, st, 1)
        assert st.step % 8 != 0
        odd_starts += (st.step % R) % 2
        _call(eng, st, n)
    assert odd_starts >= 2
    if st.step % 8 == 0:
        _call(eng, st, 1)
    before = st.step // R
    _call(eng, st, R - st.step % R + C + 1)
    assert st.step // R == before + 1
    c = eng.counters()
    assert c["steps"] == st.step and c["accepted"] == int(st.n_accept.sum())
    eng.close()
