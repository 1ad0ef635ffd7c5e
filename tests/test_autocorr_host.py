"""Autocorrelation times, host side (no GPU): the `AutoCorr` product, the parsing of the sampler
option `autocorr`, the estimator on an AR(1) ensemble with known answers, and the window and resume
bookkeeping of the sampler on an oracle-backed engine double that serves the seven autocorrelation
methods from the rule in numpy (tests/autocorr_ref.py)."""
import os

import numpy as np
import pytest

from cobaya_amd.autocorr import AutoCorr, AutoCorrError, parse_option
from cobaya_amd.model import ProblemSpec
from cobaya_amd.sampler import LoggedError, MCMCHip
from tests.autocorr_ref import AcOracleEngine, rule_window
from tests.oracle_engine import OracleEngine
from tests.test_host_logic import QUICK


class OnDouble(MCMCHip):
    _engine_factory = staticmethod(AcOracleEngine)


def make(prefix=None, max_samples=30000, resume=False, **opts):
    o = {"seed": 21, "n_walkers": 128, "group_size": 64, "steps_per_launch": 40,
         "max_samples": max_samples, "Rminus1_stop": 0.0, "learn_every": "20d",
         "snapshot_every": 40, "autocorr": {"params": ["b", "a"], "lags": 3}}
    o.update(opts)
    return OnDouble(o, ProblemSpec.from_info(QUICK), output=prefix, resume=resume)


def acc(s):
    """The sampler's `AutoCorrAccumulator` (None: the option is off)."""
    return next((p for p in s._products if p.name == "autocorr"), None)


# ------------------------------------------------------------------------------- the option
def test_every_shorthand_of_the_option():
    names = ["a", "b", "c"]
    assert parse_option(None, names) is None and parse_option(False, names) is None
    t = parse_option(True, names)
    assert t == {"params": names, "lags": 16}
    assert parse_option({}, names) == t and parse_option({"params": "all"}, names) == t
    assert parse_option({"params": "all", "lags": 64}, names) == {"params": names, "lags": 64}
    assert parse_option({"params": ["c", "a"], "lags": 1}, names) == {"params": ["c", "a"], "lags": 1}
    s = make(autocorr=True)
    assert acc(s).cfg == {"params": ["a", "b"], "lags": 16, "interval_steps": 40}
    assert s.engine.autocorr_layout() == {"n_dims": 2, "lags": 16, "n_doubles": 3 * 17 * 2, "held": 0}
    s = make(autocorr={"params": ["b"], "lags": 5}, moments_every=3)
    assert acc(s).cfg["interval_steps"] == 120 and s.engine._acr.dims == [1]
    off = make(autocorr=None)
    assert acc(off) is None and off.engine._acr is None
    off.run()
    assert "autocorr" not in off.products() and not hasattr(off.engine, "ac_snapshots")


class NeverBuilt(AcOracleEngine):
    def __init__(self, *a, **k):
        raise AssertionError("the option must be refused before the engine is created")


class Refusing(MCMCHip):
    _engine_factory = staticmethod(NeverBuilt)


@pytest.mark.parametrize("opt, match", [
    ({"lags": 0}, r"autocorr: lags must be an integer in 1\.\.64, got 0"),
    ({"lags": 65}, r"autocorr: lags must be an integer in 1\.\.64, got 65"),
    ({"lags": 2.5}, "autocorr: lags must be an integer"),
    ({"lags": True}, "autocorr: lags must be an integer"),
    ({"params": ["a", "nope"]}, r"autocorr: unknown parameter name\(s\) \['nope'\]"),
    ({"params": ["a", "b", "a"]}, r"autocorr: params lists \['a'\] twice"),
    ({"params": []}, "autocorr: params lists nothing"),
    ({"params": "some"}, "autocorr: params must be a list of names or 'all'"),
    ({"lag": 3}, r"autocorr: unknown key\(s\) \['lag'\]"),
    ("all", "autocorr: expected True, None or a dict"),
])
def test_refusals_by_name_before_the_engine_is_created(opt, match):
    with pytest.raises(LoggedError, match=match):
        Refusing({"n_walkers": 128, "group_size": 64, "autocorr": opt}, ProblemSpec.from_info(QUICK))


def test_an_engine_without_the_entry_points_is_refused():
    class Old(MCMCHip):
        _engine_factory = staticmethod(OracleEngine)    # (no autocorrelation entry points)
    with pytest.raises(LoggedError, match="autocorr: this engine has no lagged cross-products"):
        Old({"n_walkers": 128, "group_size": 64, "autocorr": True}, ProblemSpec.from_info(QUICK))
    Old({"n_walkers": 128, "group_size": 64}, ProblemSpec.from_info(QUICK))   # off: served as before


# ------------------------------------------------------------------------------- the estimator
def _double(d, W, gs, lags, shift):
    eng = AcOracleEngine(d, W, group_size=gs, seed=1)
    eng.set_prior([0] * d, [-1e6] * d, [1e6] * d)
    eng.set_target_one()
    eng.set_proposal_cov(np.eye(d))
    eng.set_moment_shift(shift)
    eng.configure_autocorr(range(d), lags)
    return eng


PHI = np.array([0.0, 0.5, 0.9])
AR_W, AR_T, AR_L = 4096, 64, 32


@pytest.fixture(scope="module")
def ar1():
    """x_{t+1} = phi x_t + sqrt(1 - phi^2) xi around the offset +1, stationary from the start: 64
    snapshots of 4096 walkers through the double, lags: 32."""
    rng = np.random.default_rng(20261018)
    eng = _double(3, AR_W, 64, AR_L, np.full(3, 0.75))
    z = rng.standard_normal((AR_W, 3))
    for _ in range(AR_T):
        eng.set_state(1.0 + z)
        eng.accumulate_autocorr()
        z = PHI * z + np.sqrt(1.0 - PHI ** 2) * rng.standard_normal((AR_W, 3))
    eng.request_autocorr()
    sums, n_pairs = eng.fetch_autocorr()
    return AutoCorr(["white", "half", "slow"], AR_L, 10, AR_W, sums, n_pairs)


def test_ar1_autocorrelations_lie_within_six_bartlett_errors(ar1):
    assert np.array_equal(ar1.n_pairs, AR_T - np.arange(AR_L + 1))
    k = np.arange(1, AR_L + 1)
    for name, phi in zip(ar1.params, PHI):
        rho = ar1.rho(name)
        assert rho[0] == 1.0 and rho.shape == (AR_L + 1,)
        p2 = phi * phi
        se2 = ((1 + p2) * (1 - p2 ** k) / (1 - p2) - 2 * k * p2 ** k) / (ar1.n_pairs[1:] * AR_W)
        dev = np.abs(rho[1:] - phi ** k) / np.sqrt(se2)
        print(f"{name}: worst deviation {dev.max():.2f} standard errors at lag {k[dev.argmax()]}")
        assert np.all(dev <= 6.0), (name, dev.max())


def test_ar1_windows_and_taus(ar1):
    def six_se(M, tau):    # Sokal: se^2 = 2 (2 M + 1) tau^2 / (snapshots x walkers)
        return 6.0 * np.sqrt(2.0 * (2 * M + 1) * tau * tau / (AR_T * AR_W))
    for name in ar1.params:
        print(f"{name}: tau {ar1.tau(name):.4f} at M = {ar1.window(name)}, converged {ar1.converged(name)}")
    assert ar1.converged("half") and ar1.window("half") in range(13, 19)
    assert six_se(15, 3.0) == pytest.approx(0.277, abs=1e-3)
    assert abs(ar1.tau("half") - 3.0) <= six_se(ar1.window("half"), 3.0)
    assert ar1.converged("white") and abs(ar1.tau("white") - 1.0) <= six_se(ar1.window("white"), 1.0)
    # phi = 0.9: tau = 19 needs M >= 95 > lags: flagged, and the reported tau is a lower bound
    assert not ar1.converged("slow") and ar1.window("slow") == AR_L
    tau_L = 1.0 + 2.0 * np.sum(0.9 ** np.arange(1, AR_L + 1))       # 18.38 < 19
    assert abs(ar1.tau("slow") - tau_L) <= six_se(AR_L, tau_L) and tau_L + six_se(AR_L, tau_L) < 2 * 19.0
    assert ar1.tau_steps("half") == ar1.tau("half") * 10
    assert ar1.ess("half") == AR_T * AR_W / ar1.tau("half")
    assert ar1.thin("half") == (int(np.ceil(ar1.tau("half"))), 10 * int(np.ceil(ar1.tau("half"))))
    assert ar1.thin() == ar1.thin("slow") and ar1.worst()[0] == "slow" and ar1.worst()[2] is False


def test_identical_snapshots_give_rho_of_exactly_one():
    """The walkers and the shift are small integers, so every product and every sum is exact: P, A
    and B of lag k are N[k] times those of one snapshot, the quotients by n_k = N[k] W are the
    same real numbers for every k, and C_k == C_0 to the bit."""
    rng = np.random.default_rng(3)
    x = rng.integers(-40, 41, size=(256, 2)).astype(np.float64)
    eng = _double(2, 256, 64, 4, [3.0, -2.0])
    for _ in range(3):
        eng.set_state(x)
        eng.accumulate_autocorr()
    eng.request_autocorr()
    ac = AutoCorr(["u", "v"], 4, 1, 256, *eng.fetch_autocorr())
    assert ac.n_pairs.tolist() == [3, 2, 1, 0, 0] and ac.held() == 2
    for n in ac.params:
        rho = ac.rho(n)
        assert np.all(rho[:3] == 1.0) and np.all(np.isnan(rho[3:]))
        assert ac.tau(n) == 5.0 and not ac.converged(n)      # 1 + 2 (1 + 1): a lower bound


# ------------------------------------------------------------------------------- AutoCorr
def _hand_made():
    """rho_k = 2^-k for `p`, 0 for `q`, from sums written by hand: W = 4, one accumulation per lag
    count below; mean 0 (A = B = 0), P[k] = n_k C_k."""
    L, W = 8, 4
    n_pairs = np.arange(20, 20 - (L + 1), -1)
    sums = np.zeros((3, L + 1, 2))
    sums[0, :, 0] = n_pairs * W * 2.0 * 0.5 ** np.arange(L + 1)
    sums[0, 0, 1] = n_pairs[0] * W * 7.0
    return AutoCorr(["p", "q"], L, 25, W, sums, n_pairs)


def test_thin_ess_and_window_of_a_hand_made_object():
    ac = _hand_made()
    assert np.array_equal(ac.rho("p"), 0.5 ** np.arange(9)) and np.array_equal(ac.rho("q")[1:], np.zeros(8))
    # tau(M) = 1 + 2 (1 - 2^-M): 2, 2.5, 2.75, ...; the first M >= 5 tau(M) does not exist below 9
    assert not ac.converged("p") and ac.tau("p") == 1 + 2 * (1 - 0.5 ** 8) and ac.window("p") == 8
    assert ac.converged("p", c=1.0) and ac.window("p", c=1.0) == 3 and ac.tau("p", c=1.0) == 2.75
    assert ac.converged("q") and ac.tau("q") == 1.0 and ac.window("q") == 5
    assert ac.ess("q") == 80.0 and ac.ess("p") == 80.0 / ac.tau("p")
    assert ac.thin("q") == (1, 25) and ac.thin("p") == (3, 75) and ac.thin() == (3, 75)
    assert ac.tau_steps("q") == 25.0 and ac.n_samples() == 80
    with pytest.raises(KeyError, match="no autocorrelation of 'z'"):
        ac.rho("z")


def test_sum_refuses_other_layouts_and_files_round_trip(tmp_path):
    ac = _hand_made()
    two = ac + ac
    assert np.array_equal(two.sums, 2 * ac.sums) and np.array_equal(two.n_pairs, 2 * ac.n_pairs)
    assert np.array_equal(two.rho("p"), ac.rho("p"))
    for other in (AutoCorr(["p", "q"], 7, 25, 4), AutoCorr(["q", "p"], 8, 25, 4),
                  AutoCorr(["p", "q"], 8, 50, 4), AutoCorr(["p", "q"], 8, 25, 8)):
        with pytest.raises(AutoCorrError, match="same layout"):
            ac + other
    with pytest.raises(AutoCorrError, match="lags must be"):
        AutoCorr(["p"], 65, 1, 4)
    with pytest.raises(AutoCorrError, match="holds 54 sums"):
        AutoCorr(["p", "q"], 8, 25, 4, np.zeros(10))
    path = str(tmp_path / "x.autocorr.npz")
    ac.save(path)
    back = AutoCorr.load(path)
    assert back == ac and back.params == ["p", "q"] and back.interval_steps == 25 and back.n_walkers == 4
    assert back.n_pairs.dtype == np.int64 and not os.path.exists(path + ".npz")
    z = np.load(path)
    assert np.array_equal(z["tau"], [ac.tau("p"), 1.0]) and z["converged"].tolist() == [False, True]


# ------------------------------------------------------------------------------- the window
def _expected(snapshots, s, n_first_ring=None):
    eng = s.engine
    return rule_window(snapshots, eng._acr.dims, eng._acr.lags, eng.group_size, s._shift,
                       s._dropped_snapshots, [iv[0] for iv in s._intervals], n_first_ring)


def test_products_hold_the_window_of_the_moments_and_nothing_older():
    s = make(max_samples=60000)
    s.run()
    assert len(s.progress) >= 5 and s._dropped_snapshots > 0 and s._iv0 > 0   # intervals were dropped
    assert len(acc(s).ivs) == len(s._intervals)
    ac = s.products()["autocorr"]
    snaps = s.engine.ac_snapshots
    n_window = sum(iv[0] for iv in s._intervals) + s._snaps_in_interval
    assert n_window == len(snaps) - s._dropped_snapshots < len(snaps)
    sums, n_pairs = _expected(snaps, s)
    assert np.array_equal(ac.n_pairs, n_pairs) and np.array_equal(ac.sums, sums)
    # the ring outlives a read-out: every lag of the window's first snapshots reaches back into
    # the dropped intervals, so every lag has as many pairs as the window has snapshots
    assert ac.n_pairs.tolist() == [n_window] * 4
    assert ac.params == ["b", "a"] and ac.lags == 3 and ac.interval_steps == 40 and ac.n_walkers == 128
    assert all(ac.rho(n)[0] == 1.0 and np.isfinite(ac.tau(n)) for n in ac.params)
    again = s.products(combined=True)["autocorr"]     # reading the open sums does not disturb them
    assert again == ac
    s.close()
    assert acc(s).product(s._intervals) == ac     # (the open sums were kept at close)


def test_a_resume_in_mid_interval_restores_the_sums_and_refills_the_ring(tmp_path):
    one = make(str(tmp_path / "a"), 40000)
    one.run()
    p = str(tmp_path / "b")
    b1 = make(p, 20000)
    b1.run()
    z = np.load(p + ".1.state.npz")
    assert int(z["ac_open_pairs"][0]) > 0 and np.abs(z["ac_open"]).sum() > 0     # stopped in mid-interval
    assert z["ac_iv"].shape == (len(z["iv_n"]), 3, 4, 2) and z["ac_iv_pairs"].shape == (len(z["iv_n"]), 4)
    assert z["ac_params"].tolist() == ["b", "a"] and z["ac_geometry"].tolist() == [3, 40]
    first = AutoCorr.load(p + ".autocorr.npz")
    assert first == b1.products()["autocorr"]
    n1 = len(b1.engine.ac_snapshots)
    b2 = make(p, 40000, resume=True)
    assert np.array_equal(b2.engine._acr.sums, z["ac_open"])          # the open sums are back, exactly
    assert np.array_equal(b2.engine._acr.n_pairs, z["ac_open_pairs"]) and b2.engine._acr.held == 0
    b2.run()
    got, ref = b2.products()["autocorr"], one.products()["autocorr"]
    snaps = one.engine.ac_snapshots       # (the states of a resumed run are those of the whole run)
    assert all(np.array_equal(a, b) for a, b in zip(snaps[n1:], b2.engine.ac_snapshots))
    assert len(snaps) == n1 + len(b2.engine.ac_snapshots)
    # the whole run: the rule with one ring; the resumed run: two separately started rings
    sums, n_pairs = _expected(snaps, one)
    assert np.array_equal(ref.sums, sums) and np.array_equal(ref.n_pairs, n_pairs)
    sums2, n_pairs2 = _expected(snaps, b2, n_first_ring=n1)
    assert np.array_equal(got.n_pairs, n_pairs2) and np.array_equal(got.sums, sums2)
    assert n1 > one._dropped_snapshots        # the resume point lies in the window: pairs are missing
    assert (ref.n_pairs - got.n_pairs).tolist() == [0, 1, 2, 3]
    assert AutoCorr.load(p + ".autocorr.npz") == got
    for n in got.params:      # a valid estimate all the same
        assert got.rho(n)[0] == 1.0 and abs(got.rho(n)[1] - ref.rho(n)[1]) < 0.05
    with pytest.raises(LoggedError, match="autocorr: cannot resume -- the run was written with params"):
        make(p, 50000, resume=True, autocorr={"params": ["b", "a"], "lags": 4})
    with pytest.raises(LoggedError, match="autocorr: cannot resume -- the run was written with params"):
        make(p, 50000, resume=True, autocorr={"params": ["a", "b"], "lags": 3})
    make(str(tmp_path / "c"), 1000, autocorr=None).run()
    with pytest.raises(LoggedError, match="autocorr: cannot resume -- the run was written without"):
        make(str(tmp_path / "c"), 50000, resume=True)


def test_the_output_file_is_cleaned_with_the_other_files(tmp_path):
    p = str(tmp_path / "c")
    make(p, 5000).run()
    assert os.path.exists(p + ".autocorr.npz")
    OnDouble({"n_walkers": 128, "group_size": 64, "seed": 1}, ProblemSpec.from_info(QUICK), output=p,
             force=True)
    assert not os.path.exists(p + ".autocorr.npz")
