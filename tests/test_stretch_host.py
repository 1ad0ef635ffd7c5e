"""The stretch move (`move: stretch`; DESIGN.md section 2, "Stretch move"), the parts that need no
device: the variates of the reference (tests/stretch_ref.py) against their laws, the reference
driven to exact moments on the host, option parsing, every refusal of the sampler by message, and
the resume guard of the state file."""
import numpy as np
import pytest

from cobaya_amd.model import ProblemSpec
from cobaya_amd.sampler import HIP_DEFAULTS, LoggedError, MCMCHip
from tests import stretch_ref as SR
from tests.oracle_engine import OracleEngine
from tests.test_host_logic import QUICK

BETA, S = 0.5, 0.5


def banana_np(p):
    return -0.5 * (p[:, 0] ** 2 + ((p[:, 1] - BETA * p[:, 0] ** 2) / S) ** 2)


def _uniform_problem(d, lo, hi, gs, seed=5, temperature=1.0):
    return SR.problem(d, np.zeros(d, np.int32), np.full(d, float(lo)), np.full(d, float(hi)),
                      group_size=gs, seed=seed, temperature=temperature)


# ------------------------------------------------------------------------------ 1. the variates
@pytest.mark.parametrize("a", [2.0, 1.5])
def test_z_follows_its_cdf(a):
    """z = ((a - 1) u + 1)^2 / a has the density ~ 1 / sqrt(z) on [1 / a, a], whose CDF is
    (sqrt z - 1 / sqrt a) / (sqrt a - 1 / sqrt a).  Kolmogorov-Smirnov with N = 20 000 draws: the
    statistic exceeds 1.95 / sqrt(N) with probability 0.001 under the law."""
    N = 20000
    _, z, _ = SR.variates(seed=77, gid=np.arange(N), step=3, group_size=64, a=a)
    assert z.min() >= 1 / a and z.max() <= a
    z = np.sort(z)
    F = (np.sqrt(z) - 1 / np.sqrt(a)) / (np.sqrt(a) - 1 / np.sqrt(a))
    emp = np.arange(1, N + 1) / N
    D = max(np.max(emp - F), np.max(F - (emp - 1.0 / N)))
    print("a = %g: KS statistic %.5f, bound %.5f" % (a, D, 1.95 / np.sqrt(N)))
    assert D < 1.95 / np.sqrt(N)


def test_accept_variate_is_exponential():
    N = 20000
    _, _, Ea = SR.variates(seed=78, gid=np.arange(N), step=1 << 33, group_size=128)
    Ea = np.sort(Ea)
    F = 1 - np.exp(-Ea)
    emp = np.arange(1, N + 1) / N
    D = max(np.max(emp - F), np.max(F - (emp - 1.0 / N)))
    assert Ea.min() > 0 and D < 1.95 / np.sqrt(N)


@pytest.mark.parametrize("gs", [64, 128, 256])
def test_partners_are_uniform_and_in_the_other_half_of_the_own_group(gs):
    d, G, hg = 2, 3, gs // 2
    W = G * gs
    prob = _uniform_problem(d, 0, 1, gs)
    x0 = np.random.default_rng(1).uniform(0.2, 0.8, (W, d))
    ref = SR.StretchRef(prob, x0, lambda p: np.zeros(len(p)), walker0=2 * gs)
    counts = np.zeros(hg)
    n_half = 40 * 64 // hg
    for _ in range(n_half):
        ref.propose()
        act, par = ref.active(), ref.partner.astype(np.int64)
        assert np.array_equal(act // gs, par // gs)                   # the own group
        assert np.all((par % gs) // hg == 1 - ref.half)                 # the other half
        assert np.all((act % gs) // hg == ref.half)
        counts += np.bincount(par % hg, minlength=hg)
        ref.accept(np.zeros(W // 2))
    # chi-square of the member counts: hg - 1 degrees of freedom, mean hg - 1, variance 2 (hg - 1);
    # six standard deviations above the mean
    n = counts.sum()
    chi2 = np.sum((counts - n / hg) ** 2 / (n / hg))
    assert n == n_half * W // 2
    assert chi2 < (hg - 1) + 6 * np.sqrt(2 * (hg - 1)), (chi2, hg)


def test_q_is_exactly_zero_at_d1_and_log_z_to_the_power_elsewhere():
    for d in (1, 3):
        prob = _uniform_problem(d, 0, 1, 64)
        x0 = np.random.default_rng(2).uniform(0.2, 0.8, (128, d))
        ref = SR.StretchRef(prob, x0, lambda p: np.zeros(len(p)))
        ref.propose()
        _, z, Ea = SR.variates(prob.seed, ref.active(), 0, 64)
        if d == 1:
            assert np.all(ref.q == 0.0)
        else:
            np.testing.assert_allclose(ref.q, (d - 1) * np.log(z), rtol=1e-14)
            assert np.all(ref.q != 0.0)
        assert np.array_equal(ref.Ea, Ea)
        # the trial lies on the line through the partner: t = p + z (x - p)
        np.testing.assert_allclose(ref.t, ref.x[ref.partner] + z[:, None] * (ref.x[ref.active()] - ref.x[ref.partner]),
                                   rtol=1e-13, atol=1e-15)


# ------------------------------------------------------------------------------ 2. exact moments
def _se_checks(x, mean, var, mu4):
    """(name, got, want, standard error of N independent draws) of mean and variance per column."""
    N = len(x)
    out = []
    for i in range(x.shape[1]):
        out.append(("E x%d" % i, x[:, i].mean(), mean[i], np.sqrt(var[i] / N)))
        out.append(("Var x%d" % i, x[:, i].var(ddof=1), var[i], np.sqrt((mu4[i] - var[i] ** 2) / N)))
    return out


def _assert_within_6se(checks):
    for name, got, want, se in checks:
        print("%s: got %.5f want %.5f  (%.2f standard errors)" % (name, got, want, (got - want) / se))
    for name, got, want, se in checks:
        assert abs(got - want) < 6 * se, (name, got, want, se)


def test_reference_samples_the_banana():
    """64 groups of 64 walkers from an over-dispersed start, 600 steps: the final ensemble's exact
    moments within 6 standard errors of 4 096 independent draws (the bar of _check_banana_moments).
    The box is [-8, 8] x [-6, 30]: more than 6 sigma beyond the mass on every side."""
    gs, G = 64, 64
    prob = SR.problem(2, np.zeros(2, np.int32), np.array([-8.0, -6.0]), np.array([8.0, 30.0]),
                      group_size=gs, seed=31)
    x0 = np.random.default_rng(3).normal([0.0, 0.5], [1.0, 1.0], (G * gs, 2))
    ref = SR.StretchRef(prob, x0, banana_np)
    acc = ref.run(600, banana_np)
    rate = acc / (600.0 * G * gs)
    print("acceptance %.3f" % rate)
    assert 0.4 < rate < 0.9
    assert ref.stuck[0] == 0 and ref.bad[0] == 0
    var_b, mu4_b = 2 * BETA ** 2 + S ** 2, 60 * BETA ** 4 + 12 * BETA ** 2 * S ** 2 + 3 * S ** 4
    _assert_within_6se(_se_checks(ref.x, [0.0, BETA], [1.0, var_b], [3.0, mu4_b]))


def test_reference_samples_a_gaussian_in_d8_at_group_size_128():
    """Host only (the reference is too slow to converge the device case): d = 8, group_size 128,
    independent N(0.5 + 0.1 i, s_i^2) with s_i = 0.05 (1 + i), uniform priors on [-20, 20] (>= 25 sigma
    wide on each side), 32 groups, 1 500 steps from a start twice as wide as the target."""
    d, gs, G = 8, 128, 32
    mu, sig = 0.5 + 0.1 * np.arange(d), 0.05 * (1 + np.arange(d))

    def f(p):
        return -0.5 * (((p - mu) / sig) ** 2).sum(1)

    prob = _uniform_problem(d, -20, 20, gs, seed=32)
    x0 = np.random.default_rng(4).normal(mu, 2 * sig, (G * gs, d))
    ref = SR.StretchRef(prob, x0, f)
    acc = ref.run(1500, f)
    rate = acc / (1500.0 * G * gs)
    print("acceptance %.3f" % rate)
    assert 0.25 < rate < 0.8
    _assert_within_6se(_se_checks(ref.x, mu, sig ** 2, 3 * sig ** 4))


def test_tempered_reference_samples_the_tempered_gaussian():
    """temperature 2 flattens the posterior (variance x 2) and leaves the Jacobian z^(d - 1) alone:
    tempering it as well would sample another law."""
    d, gs, G = 3, 64, 64

    def f(p):
        return -0.5 * ((p / 0.1) ** 2).sum(1)

    prob = _uniform_problem(d, -5, 5, gs, seed=33, temperature=2.0)
    x0 = np.random.default_rng(5).normal(0, 0.2, (G * gs, d))
    ref = SR.StretchRef(prob, x0, f)
    ref.run(600, f)
    _assert_within_6se(_se_checks(ref.x, np.zeros(d), np.full(d, 0.02), np.full(d, 3 * 0.02 ** 2)))


# ------------------------------------------------------------------------------ 3. the sampler's side
def module_level_function(p):
    return -0.5 * (p ** 2).sum(1)


def _info(ref_a=None, ref_b=None, **like):
    ref_a = {"dist": "norm", "loc": 0, "scale": 1} if ref_a is None else ref_a
    ref_b = {"dist": "norm", "loc": 0.5, "scale": 1} if ref_b is None else ref_b
    return {"likelihood": {"banana": {"class": "device_function", "function": module_level_function, **like}},
            "params": {"a": {"prior": {"min": -8, "max": 8}, "ref": ref_a, "proposal": 1},
                       "b": {"prior": {"min": -6, "max": 30}, "ref": ref_b, "proposal": 1}}}


def no_engine(*a, **k):
    raise AssertionError("the engine must not be created")


no_engine.max_dim = lambda: 256


class NoEngine(MCMCHip):
    _engine_factory = staticmethod(no_engine)


BASE = {"seed": 1, "n_walkers": 128, "group_size": 64, "max_samples": 100, "move": "stretch"}


def test_option_defaults_and_parsing():
    assert HIP_DEFAULTS["move"] is None and HIP_DEFAULTS["stretch_a"] == 2.0
    import mcmc_hip
    assert mcmc_hip.MCMCHip.move is None and mcmc_hip.MCMCHip.stretch_a == 2.0
    with pytest.raises(LoggedError, match="move must be None, 'metropolis' or 'stretch', got 'walk'"):
        NoEngine({**BASE, "move": "walk"}, ProblemSpec.from_info(_info()))
    # None and "metropolis" are today's path: they reach the engine (which this double refuses to make)
    for move in (None, "metropolis"):
        with pytest.raises(AssertionError, match="the engine must not be created"):
            NoEngine({**BASE, "move": move}, ProblemSpec.from_info(_info()))
    # ... and so does a served stretch configuration
    with pytest.raises(AssertionError, match="the engine must not be created"):
        NoEngine({**BASE, "stretch_a": "1.5"}, ProblemSpec.from_info(_info()))


def test_sampler_refuses_unserved_options_by_name_before_the_engine():
    def refused(match, info=None, **opts):
        with pytest.raises(LoggedError, match=match):
            NoEngine({**BASE, **opts}, ProblemSpec.from_info(info or _info()))

    refused("move: stretch: likelihood 'gaussian_mixture' is not served", info=QUICK)
    two = _info()
    two["likelihood"] = {"f": {"class": "device_function", "function": module_level_function, "input_params": ["a"]},
                         "g": {"class": "device_function", "function": module_level_function,
                               "input_params": ["a", "b"]}}
    refused("move: stretch: several device_function likelihoods are not served", info=two)
    refused("drag: True is not served", drag=True, blocking=[[1, ["a"]], [10, ["b"]]])
    refused("parameter blocks", blocking=[[1, ["a"]], [2, ["b"]]])
    info = _info()
    info["params"]["a"]["periodic"] = True
    refused("periodic parameters are not served", info=info)
    refused("emit: chains is not served", emit="chains")
    refused("evaluation: incremental is not served", evaluation="incremental")
    for a in (1.0, 0.5, float("inf"), float("nan")):
        refused("move: stretch: stretch_a must be finite and > 1", stretch_a=a)
    refused("stretch_a must be a number > 1", stretch_a="wide")
    # group_size < 4 d: the message gives the remedy
    wide = {"likelihood": {"f": {"class": "device_function", "function": module_level_function}},
            "params": {"p%02d" % i: {"prior": {"min": 0, "max": 1}, "proposal": 0.1} for i in range(17)}}
    refused(r"group_size: 64 < 4 d = 68.*use a larger group_size \(256 serves d <= 64\)", info=wide)
    with pytest.raises(AssertionError, match="the engine must not be created"):
        NoEngine({**BASE, "n_walkers": 256, "group_size": 128}, ProblemSpec.from_info(wide))
    # a fixed `ref` point (the README's Metropolis example has "ref": 0): named, with the remedy
    refused(r"move: stretch: `ref` of \['a'\] is a fixed point.*give `ref` as a pdf", info=_info(ref_a=0))
    refused(r"`ref` of \['a', 'b'\] is a fixed point", info=_info(ref_a=0, ref_b=0.5))


class MoveDouble(OracleEngine):
    """The oracle-backed engine double; `set_move` is accepted (the resume guard is the sampler's)."""

    def set_move(self, move, stretch_a=2.0):
        pass


class OnDouble(MCMCHip):
    _engine_factory = staticmethod(MoveDouble)


class ForcedStretch(OnDouble):
    """Says `move: stretch` whatever the likelihood: only the state file's guard is under test."""

    def _check_move(self, spec, d):
        self.stretch, self.stretch_a = True, float(self.stretch_a)


def test_resume_with_another_move_is_refused(tmp_path):
    opts = {"seed": 21, "n_walkers": 128, "group_size": 64, "steps_per_launch": 40, "max_samples": 20000,
            "Rminus1_stop": 0.0, "learn_every": "20d"}
    spec = ProblemSpec.from_info(QUICK)
    # written by the default move: no key (the file of today's runs is unchanged) ...
    p = str(tmp_path / "m")
    s = OnDouble(opts, spec, output=p)
    s.run()
    s.close()
    assert "move" not in np.load(p + ".1.state.npz").files
    OnDouble({**opts, "max_samples": 30000}, spec, output=p, resume=True).close()
    with pytest.raises(LoggedError, match=r"cannot resume -- the run was written with move: metropolis and now "
                                          r"has move: stretch \(stretch_a: 2\)"):
        ForcedStretch(opts, spec, output=p, resume=True)
    # ... written by the stretch move: the key says so
    q = str(tmp_path / "s")
    s = ForcedStretch(opts, spec, output=q)
    s.run()
    s.close()
    assert np.load(q + ".1.state.npz")["move"].tolist() == [1.0, 2.0]
    ForcedStretch({**opts, "max_samples": 30000}, spec, output=q, resume=True).close()
    with pytest.raises(LoggedError, match=r"cannot resume -- the run was written with move: stretch \(stretch_a: 2\) "
                                          r"and now has move: metropolis"):
        OnDouble(opts, spec, output=q, resume=True)
    with pytest.raises(LoggedError, match=r"written with move: stretch \(stretch_a: 2\) and now has move: stretch "
                                          r"\(stretch_a: 1.5\)"):
        ForcedStretch({**opts, "stretch_a": 1.5}, spec, output=q, resume=True)
