"""Lagged cross-products of the ensemble on the MI355X (autocorr_kernels.hip, mcmc_hip_autocorr_*):
the accumulators equal the rule of DESIGN.md section 2 ("Autocorrelation") -- `Rule` of
tests/autocorr_ref.py: numpy with the kernel's own chains -- BIT FOR BIT, at the smallest shapes at
which the kernels can still go wrong; the read-out is stream-ordered and keeps the ring; the
sampler's product holds exactly the snapshots of its window."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402,F401  (before the first Engine: one HIP runtime for both)

from cobaya_amd import run  # noqa: E402
from cobaya_amd.autocorr import AutoCorr  # noqa: E402
from cobaya_amd.engine import ERR_ARG, ERR_STATE, Engine, EngineError  # noqa: E402
from tests.autocorr_ref import Rule, rule_window  # noqa: E402


def _gauss_engine(d, W, gs, seed=11, incremental=False, walker_offset=0, x0=None, target="gaussian"):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((d, d)) / np.sqrt(d)
    cov = 0.004 * (0.5 * A @ A.T + 0.5 * np.eye(d))
    mean = 0.5 + 0.02 * rng.standard_normal(d)
    eng = Engine(d, W, group_size=gs, device=0, seed=seed, incremental=incremental,
                 walker_offset=walker_offset)
    eng.set_prior([0] * d, [0.0] * d, [1.0] * d)
    if target == "one":
        eng.set_target_one()
    else:
        eng.set_target_gaussian_mixture([mean], [cov])
    eng.set_proposal_cov(cov)
    if x0 is None:
        x0 = np.clip(mean + rng.standard_normal((W, d)) * np.sqrt(np.diag(cov)), 0.01, 0.99)
    eng.set_state(x0)
    eng.set_moment_shift(x0.mean(0))
    return eng, mean, cov, x0


def _same(got, rule):
    sums, n_pairs = got
    return (np.array_equal(n_pairs, rule.n_pairs) and sums.shape == rule.sums.shape
            and np.array_equal(sums.view(np.uint64), rule.sums.view(np.uint64)))


SHAPES = [   # (d, W, group, lags, incremental, dims)
    (1, 64, 64, 1, False, None),
    (2, 256, 64, 3, False, None),
    (30, 512, 128, 4, False, None),
    (33, 256, 256, 2, False, None),             # the d > 32 state path; one group of 256
    (128, 128, 64, 2, False, None),
    (30, 512, 128, 4, True, None),              # the incremental step kernels write x as well
    (5, 192, 64, 3, False, [4, 0, 2]),          # a subset in non-ascending order; W no multiple of 256
    (130, 256, 64, 2, True, None),              # d > 128: huge_kernels.hip keeps x as [d][W] too
]


@pytest.mark.parametrize("d, W, gs, L, inc, dims", SHAPES,
                         ids=[f"d{s[0]}-W{s[1]}-g{s[2]}-L{s[3]}" + ("-inc" if s[4] else "") + ("-subset" if s[5] else "")
                              for s in SHAPES])
def test_accumulators_equal_the_rule_bit_for_bit(d, W, gs, L, inc, dims):
    """Seven accumulations with steps between them: the ring is partly filled at first and wraps
    afterwards.  Fails without the feature: the entry points do not exist."""
    eng, _, _, x0 = _gauss_engine(d, W, gs, incremental=inc)
    dims = list(range(d)) if dims is None else dims
    eng.configure_autocorr(dims, L)
    assert eng.autocorr_layout() == {"n_dims": len(dims), "lags": L, "n_doubles": 3 * (L + 1) * len(dims), "held": 0}
    rule = Rule(dims, L, gs, x0.mean(0))
    for t in range(7):
        eng.step(2)
        eng.accumulate_autocorr()
        rule.accumulate(eng.get_state()["x"])
        assert eng.autocorr_layout()["held"] == min(t + 1, L + 1)
    eng.request_autocorr()
    got = eng.fetch_autocorr()
    assert got[1].tolist() == [7 - k for k in range(L + 1)]
    assert _same(got, rule)
    assert np.array_equal(got[0][1, 0], got[0][2, 0])          # lag 0: accA == accB
    assert np.all(got[0][0, 0] > 0)                              # ... and accP is a second moment
    eng.close()


def _crafted_engine(d, W, gs, lo=-100.0, hi=100.0):
    eng = Engine(d, W, group_size=gs, device=0, seed=3)
    eng.set_prior([0] * d, [lo] * d, [hi] * d)
    eng.set_target_one()
    eng.set_proposal_cov(0.01 * np.eye(d))
    return eng


def test_the_same_snapshot_three_times_gives_rho_of_exactly_one():
    """Walkers and shift are small integers: every product and sum is exact, P, A, B of lag k are
    N[k] times those of one snapshot, the quotients by n_k = N[k] W are the same real numbers for
    every k, hence C_k == C_0 to the bit.  `lags` exceeds the snapshots ever taken: the unused lags
    stay at zero with n_pairs == 0."""
    d, W, gs, L = 2, 256, 64, 5
    rng = np.random.default_rng(3)
    x = rng.integers(-40, 41, size=(W, d)).astype(np.float64)
    eng = _crafted_engine(d, W, gs)
    eng.set_state(x)
    eng.set_moment_shift([3.0, -2.0])
    eng.configure_autocorr([0, 1], L)
    rule = Rule([0, 1], L, gs, [3.0, -2.0])
    for _ in range(3):
        eng.set_state(x)                  # (set_state keeps the ring)
        eng.accumulate_autocorr()
        rule.accumulate(x)
    assert eng.autocorr_layout()["held"] == 3
    eng.request_autocorr()
    sums, n_pairs = eng.fetch_autocorr()
    assert n_pairs.tolist() == [3, 2, 1, 0, 0, 0] and _same((sums, n_pairs), rule)
    assert not sums[:, 3:].any()
    ac = AutoCorr(["u", "v"], L, 1, W, sums, n_pairs)
    for n in ac.params:
        rho = ac.rho(n)
        assert np.all(rho[:3] == 1.0) and np.all(np.isnan(rho[3:]))
    eng.close()


def test_a_shift_a_million_sigma_away_still_matches_the_rule():
    """a = x - shift loses most of x's digits and a * b is ~1e6 times the signal: only the same
    separate roundings in the same order give the same bits (a fused multiply-add would not)."""
    d, W, gs, L = 3, 128, 64, 2
    rng = np.random.default_rng(5)
    sigma = 1e-3
    eng = _crafted_engine(d, W, gs, lo=-5000.0, hi=5000.0)
    shift = np.array([0.5 + 1e6 * sigma, 0.5 - 1e6 * sigma, 0.5 + 1e6 * sigma])
    snaps = [0.5 + sigma * rng.standard_normal((W, d)) for _ in range(4)]
    eng.set_state(snaps[0])
    eng.set_moment_shift(shift)
    eng.configure_autocorr([2, 0, 1], L)
    rule = Rule([2, 0, 1], L, gs, shift)
    for x in snaps:
        eng.set_state(x)
        eng.accumulate_autocorr()
        rule.accumulate(x)
    eng.request_autocorr()
    got = eng.fetch_autocorr()
    assert got[1].tolist() == [4, 3, 2] and _same(got, rule)
    eng.close()


def test_two_walker_shards_against_the_whole_ensemble():
    """The shards pool their own groups and the host adds the two sums: another order of the same
    G terms per accumulation.  Two orders of one sum differ by at most (terms - 1) 2^-52 sum|term|
    (twice the classical (m - 1) u sum|t|, u = 2^-53); the bound asserted is G 2^-52 times the
    accumulated sum of |P_g| (|S_g| for A and B), G the groups of the whole ensemble."""
    d, W, gs, L = 5, 256, 64, 2
    whole, _, _, x0 = _gauss_engine(d, W, gs, seed=19)
    shift = x0.mean(0)
    parts = [_gauss_engine(d, W // 2, gs, seed=19, walker_offset=k * (W // 2),
                           x0=x0[k * (W // 2):(k + 1) * (W // 2)])[0] for k in range(2)]
    rule = Rule(range(d), L, gs, shift)
    out = []
    for eng in [whole] + parts:
        eng.set_moment_shift(shift)
        eng.configure_autocorr(range(d), L)
        for _ in range(4):
            eng.step(3)
            eng.accumulate_autocorr()
            if eng is whole:
                rule.accumulate(eng.get_state()["x"])
        eng.request_autocorr()
        out.append(eng.fetch_autocorr())
    assert np.array_equal(np.vstack([p.get_state()["x"] for p in parts]), whole.get_state()["x"])
    assert _same(out[0], rule)
    assert np.array_equal(out[0][1], out[1][1]) and np.array_equal(out[0][1], out[2][1])
    G = W // gs
    bound = G * 2.0 ** -52 * rule.abs_sums
    err = np.abs(out[1][0] + out[2][0] - out[0][0])
    print("largest error / bound:", np.max(err / bound))
    assert np.all(err <= bound)
    for eng in [whole] + parts:
        eng.close()


def test_request_keeps_the_ring_set_continues_and_reset_empties_it():
    d, W, gs, L = 3, 128, 64, 3
    eng, _, _, x0 = _gauss_engine(d, W, gs, seed=23)
    shift = x0.mean(0)
    with pytest.raises(EngineError) as ei:        # not configured yet
        eng.accumulate_autocorr()
    assert ei.value.code == ERR_STATE
    eng.configure_autocorr([0, 1, 2], L)
    with pytest.raises(EngineError) as ei:
        eng.fetch_autocorr()
    assert ei.value.code == ERR_STATE
    rule = Rule([0, 1, 2], L, gs, shift)
    for _ in range(3):
        eng.step(2)
        eng.accumulate_autocorr()
        rule.accumulate(eng.get_state()["x"])
    eng.request_autocorr()
    first = rule.read_and_zero()
    for _ in range(2):                            # queued AFTER the request: the next fetch's
        eng.step(2)
        eng.accumulate_autocorr()
        rule.accumulate(eng.get_state()["x"])
    got = eng.fetch_autocorr()
    assert got[1].tolist() == [3, 2, 1, 0] and np.array_equal(got[0], first[0])
    eng.request_autocorr()
    got = eng.fetch_autocorr()
    # the ring was kept: the lags of the two later snapshots reach back across the request
    assert got[1].tolist() == [2, 2, 2, 2] and _same(got, rule)
    second = rule.read_and_zero()
    eng.request_autocorr()
    got = eng.fetch_autocorr()
    assert not got[0].any() and not got[1].any()
    # resume: open sums go back, the next accumulation adds to them (the ring still holds 4)
    eng.autocorr_set(first[0], first[1])
    rule.set(*first)
    eng.step(1)
    eng.accumulate_autocorr()
    rule.accumulate(eng.get_state()["x"])
    assert eng.autocorr_layout()["held"] == 4
    eng.autocorr_reset()
    rule.reset()
    assert eng.autocorr_layout()["held"] == 0
    eng.step(1)
    eng.accumulate_autocorr()                     # pairs with itself only
    rule.accumulate(eng.get_state()["x"])
    eng.request_autocorr()
    got = eng.fetch_autocorr()
    assert got[1].tolist() == [5, 3, 2, 1] and _same(got, rule) and not np.array_equal(got[0], second[0])
    with pytest.raises(EngineError) as ei:
        eng.autocorr_set(first[0].reshape(-1)[:-1], first[1])
    assert ei.value.code == ERR_ARG and "sums" in str(ei.value)
    # a change of the moment shift empties the ring and zeroes the sums; the same shift does not
    eng.accumulate_autocorr()
    eng.accumulate_moments()
    eng.read_moments(reset=True)
    eng.set_moment_shift(shift)
    assert eng.autocorr_layout()["held"] == 2
    eng.set_moment_shift(shift + 1.0)
    assert eng.autocorr_layout()["held"] == 0
    eng.request_autocorr()
    got = eng.fetch_autocorr()
    assert not got[0].any() and not got[1].any()
    # a bad configuration names its argument and leaves the old one alone
    for kw, word in ((dict(lags=0), "lags"), (dict(lags=65), "lags"), (dict(dims=[3]), "dims[0]"),
                     (dict(dims=[0, -1]), "dims[1]"), (dict(dims=[1, 2, 1]), "duplicate")):
        a = dict(dims=[0, 1, 2], lags=L)
        a.update(kw)
        with pytest.raises(EngineError) as ei:
            eng.configure_autocorr(**a)
        assert ei.value.code == ERR_ARG and word in str(ei.value), (word, str(ei.value))
    assert eng.autocorr_layout()["n_doubles"] == 3 * 4 * 3
    eng.configure_autocorr()                      # nothing listed: off, the ring is freed
    assert eng.autocorr_layout() == {"n_dims": 0, "lags": 0, "n_doubles": 0, "held": 0}
    with pytest.raises(EngineError):
        eng.accumulate_autocorr()
    eng.close()


def test_around_the_one_likelihood_and_a_device_function():
    eng, _, _, x0 = _gauss_engine(4, 128, 64, seed=29, target="one")
    eng.configure_autocorr([3, 1], 2)
    rule = Rule([3, 1], 2, 64, x0.mean(0))
    for _ in range(4):
        eng.step(5)
        eng.accumulate_autocorr()
        rule.accumulate(eng.get_state()["x"])
    eng.request_autocorr()
    assert _same(eng.fetch_autocorr(), rule)
    eng.close()

    def banana(p):                      # the banana of tests/test_gpu_function_target.py
        return -0.5 * (p[:, 0] ** 2 + ((p[:, 1] - 0.5 * p[:, 0] ** 2) / 0.5) ** 2)

    eng = Engine(2, 128, group_size=64, device=0, seed=31)
    eng.set_prior([0, 0], [-8.0, -6.0], [8.0, 30.0])
    eng.set_target_function(banana)
    eng.set_proposal_cov(np.eye(2))
    rng = np.random.default_rng(31)
    x0 = np.column_stack((rng.normal(0, 1, 128), rng.normal(0.5, 0.5, 128)))
    eng.set_state(x0)
    eng.set_moment_shift(x0.mean(0))
    eng.configure_autocorr([0, 1], 2)
    rule = Rule([0, 1], 2, 64, x0.mean(0))
    for _ in range(4):
        eng.step(4)
        eng.accumulate_autocorr()
        rule.accumulate(eng.get_state()["x"])
    assert eng.last_step_kernel().startswith("mcmc::fn_walker_kernel")
    eng.request_autocorr()
    assert _same(eng.fetch_autocorr(), rule)
    eng.close()


# ------------------------------------------------------------------------------ end to end
def _quickstart(**opts):
    o = {"n_walkers": 4096, "seed": 7, "Rminus1_stop": 0.0, "max_samples": 3.0e6,
         "steps_per_launch": 40, "moments_every": 1, "snapshot_every": 40, "max_rows": 1 << 22}
    o.update(opts)
    return {"likelihood": {"gaussian_mixture": {"means": [0.2, 0], "covs": [[0.1, 0.05], [0.05, 0.2]]}},
            "params": {"a": {"prior": {"min": -0.5, "max": 3}},
                       "b": {"prior": {"dist": "norm", "loc": 0, "scale": 1}, "ref": 0, "proposal": 0.5}},
            "sampler": {"mcmc_hip": o}}


def test_run_holds_the_window_exactly_as_the_rule_on_the_stored_rows():
    """README quickstart with `autocorr: True`: every accumulated snapshot is also stored
    (moments_every 1, snapshot_every = one launch, max_rows large enough), so the product must equal
    the rule applied to the stored rows, read out where the window's intervals begin -- exactly."""
    W = 4096
    _, s = run(_quickstart(autocorr=True))
    prod = s.products()
    ac = prod["autocorr"]
    counts = [iv[0] for iv in s._intervals]
    n_window = sum(counts) + s._snaps_in_interval
    assert 0 < s._dropped_snapshots and ac.n_pairs[0] == n_window
    assert (ac.params, ac.lags, ac.interval_steps, ac.n_walkers) == (["a", "b"], 16, 40, W)
    x = prod["sample"].data[["a", "b"]].to_numpy()
    n_all = s._dropped_snapshots + n_window
    assert len(x) == n_all * W                                           # nothing was thinned away
    snaps = x.reshape(n_all, W, 2)
    sums, n_pairs = rule_window(snaps, [0, 1], 16, int(s.group_size), s._shift, s._dropped_snapshots, counts)
    assert np.array_equal(ac.n_pairs, n_pairs)
    assert np.array_equal(ac.sums.view(np.uint64), sums.view(np.uint64))
    for name in ac.params:
        rho = ac.rho(name)
        print(name, "tau", ac.tau(name), "window", ac.window(name), "converged", ac.converged(name),
              "ess", ac.ess(name), "rho[1:4]", rho[1:4])
        assert rho[0] == 1.0 and np.all(np.abs(rho[1:]) < 1.0)
        assert np.isfinite(ac.tau(name)) and (ac.converged(name) or ac.window(name) == 16)
    assert ac.thin()[1] == ac.thin()[0] * 40
    s.close()
    assert s._products[-1].product(s._intervals) == ac           # the sums outlive the engine


def test_without_the_option_nothing_exists_and_the_chain_is_the_same():
    _, off = run(_quickstart(max_samples=4.0e5))
    assert "autocorr" not in off.products()
    assert off.engine.autocorr_layout() == {"n_dims": 0, "lags": 0, "n_doubles": 0, "held": 0}
    with pytest.raises(EngineError) as ei:       # (the launch needs the ring the option allocates)
        off.engine.accumulate_autocorr()
    assert ei.value.code == ERR_STATE
    _, on = run(_quickstart(max_samples=4.0e5, autocorr={"params": ["b"], "lags": 2}))
    assert on.engine.last_step_kernel() == off.engine.last_step_kernel()
    a, b = off.engine.get_state(), on.engine.get_state()
    assert np.array_equal(a["x"], b["x"]) and np.array_equal(a["logpost"], b["logpost"])
    assert np.array_equal(off.engine.get_proposal_cov(), on.engine.get_proposal_cov())
    cols = ["N", "acceptance_rate", "Rminus1"]   # the moment path: the same R-1 at every checkpoint
    assert len(off.progress) > 0 and off.progress[cols].equals(on.progress[cols])
    off.close()
    on.close()
