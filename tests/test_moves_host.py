"""Mixtures of ensemble moves (`moves`; DESIGN.md section 2, "Ensemble move mixtures"), the parts
that need no device: partners, variates and the choice of kind of the reference
(tests/moves_ref.py) against their laws, the reference driven on the host -- it carries walkers
between two modes 20 sigma apart where the stretch move cannot, and the snooker update samples a
Gaussian with the right Jacobian power --, option parsing, every refusal of the sampler by message,
and the resume guard of the state file."""
import numpy as np
import pytest

from cobaya_amd.model import ProblemSpec
from cobaya_amd.sampler import HIP_DEFAULTS, LoggedError, MCMCHip
from tests import moves_ref as MR
from tests import stretch_ref as SR
from tests.oracle_engine import OracleEngine
from tests.test_host_logic import QUICK

HOP = [["de", 0.8], ["de", 0.2, {"gamma": 1.0}]]


def _uniform_problem(d, lo, hi, gs, seed=5, temperature=1.0):
    return MR.problem(d, np.zeros(d, np.int32), np.full(d, float(lo)), np.full(d, float(hi)),
                      group_size=gs, seed=seed, temperature=temperature)


def _flat(p):
    return np.zeros(len(p))


# ------------------------------------------------------------------------------ 1. partners
@pytest.mark.parametrize("gs", [64, 128, 256])
@pytest.mark.parametrize("kind", ["de", "snooker"])
def test_partners_are_distinct_uniform_and_in_the_other_half_of_the_own_group(gs, kind):
    d, G, hg = 2, 2, gs // 2
    W = G * gs
    n_members = {"de": 2, "snooker": 3}[kind]
    prob = _uniform_problem(d, 0, 1, gs)
    x0 = np.random.default_rng(1).uniform(0.2, 0.8, (W, d))
    ref = MR.MovesRef(prob, x0, _flat, [[kind, 1.0]], walker0=3 * gs)
    counts = np.zeros((n_members, hg))
    n_half = 600 * 64 // hg
    for _ in range(n_half):
        ref.propose()
        act, par = ref.active(), ref.partner.astype(np.int64)
        assert np.all(par[:, n_members:] == -1)
        par = par[:, :n_members]
        assert np.all((act % gs) // hg == ref.half)
        assert np.array_equal(par // gs, np.repeat(act[:, None] // gs, n_members, 1))   # the own group
        assert np.all((par % gs) // hg == 1 - ref.half)                               # the other half
        for a in range(n_members):
            for b in range(a + 1, n_members):
                assert np.all(par[:, a] != par[:, b])                                   # pairwise distinct
            counts[a] += np.bincount(par[:, a] % hg, minlength=hg)
        ref.accept(np.zeros(W // 2))
    assert ref.step == n_half // 2
    # chi-square of the member counts: hg - 1 degrees of freedom, mean hg - 1, variance 2 (hg - 1);
    # six standard deviations above the mean (the bound of the stretch partner test)
    for a in range(n_members):
        n = counts[a].sum()
        chi2 = np.sum((counts[a] - n / hg) ** 2 / (n / hg))
        assert n == n_half * W // 2
        assert chi2 < (hg - 1) + 6 * np.sqrt(2 * (hg - 1)), (a, chi2, hg)


def test_the_second_de_partner_is_uniform_over_the_other_members():
    """m1 - m0 - 1 mod hg is the multiply-shift draw of hg - 1 values: each equally often."""
    hg, N = 32, 31 * 2000
    m, _, _ = MR.variates(seed=3, gid=np.arange(N), step=9, group_size=64, kind=MR.DE)
    r = (m[:, 1] - m[:, 0] - 1) % hg
    assert r.max() == hg - 2
    counts = np.bincount(r, minlength=hg - 1)
    chi2 = np.sum((counts - N / (hg - 1)) ** 2 / (N / (hg - 1)))
    assert chi2 < (hg - 2) + 6 * np.sqrt(2 * (hg - 2))


# ------------------------------------------------------------------------------ 2. variates, snooker factor
def _ks(sample, cdf):
    s = np.sort(sample)
    F, N = cdf(s), len(s)
    emp = np.arange(1, N + 1) / N
    return max(np.max(emp - F), np.max(F - (emp - 1.0 / N)))


def test_gamma_jitter_has_mean_gamma0_and_deviation_gamma0_sigma():
    """gamma = gamma0 (1 + sigma n), n standard normal: 20 000 draws, mean and deviation within 5
    standard errors (deviation of a normal sample: s / sqrt(2 N)), and the law itself by
    Kolmogorov-Smirnov at the 0.001 level (1.95 / sqrt N)."""
    from math import erf
    N, g0, sig = 20000, 0.7, 0.1
    _, gam, _ = MR.variates(seed=11, gid=np.arange(N), step=5, group_size=64, kind=MR.DE, p0=g0, p1=sig)
    assert abs(gam.mean() - g0) < 5 * g0 * sig / np.sqrt(N)
    assert abs(gam.std(ddof=1) - g0 * sig) < 5 * g0 * sig / np.sqrt(2 * N)
    n = (gam / g0 - 1) / sig
    D = _ks(n, lambda s: np.array([0.5 * (1 + erf(v / np.sqrt(2))) for v in s]))
    assert D < 1.95 / np.sqrt(N)
    # sigma = 0: no jitter at all
    _, gam0, _ = MR.variates(seed=11, gid=np.arange(50), step=5, group_size=64, kind=MR.DE, p0=g0, p1=0.0)
    assert np.all(gam0 == g0)


@pytest.mark.parametrize("kind", [MR.DE, MR.SNOOKER])
def test_accept_variate_is_exponential(kind):
    N = 20000
    _, _, Ea = MR.variates(seed=78, gid=np.arange(N), step=(1 << 33) + 1, group_size=128, kind=kind)
    assert Ea.min() > 0 and _ks(Ea, lambda s: 1 - np.exp(-s)) < 1.95 / np.sqrt(N)


def test_the_kinds_draw_from_streams_of_their_own():
    gid = np.arange(64)
    Ea = [MR.variates(1, gid, 4, 64, kind, p0=2.0)[2] for kind in (MR.STRETCH, MR.DE, MR.SNOOKER)]
    assert not np.any(Ea[0] == Ea[1]) and not np.any(Ea[1] == Ea[2]) and not np.any(Ea[0] == Ea[2])
    # ... and the stretch member's are those of `move: stretch`
    m, z, ea = MR.variates(1, gid, 4, 64, MR.STRETCH, p0=2.0)
    ms, zs, eas = SR.variates(1, gid, 4, 64, a=2.0)
    assert np.array_equal(m[:, 0], ms) and np.array_equal(z, zs) and np.array_equal(ea, eas)


def test_snooker_q_is_exactly_zero_at_d1_and_the_log_ratio_to_the_power_elsewhere():
    for d in (1, 3, 40):
        gs = 64 if d < 40 else 256
        prob = _uniform_problem(d, 0, 1, gs)
        x0 = np.random.default_rng(2).uniform(0.2, 0.8, (2 * gs, d))
        ref = MR.MovesRef(prob, x0, _flat, [["snooker", 1.0]])
        ref.propose()
        x, z = ref.x[ref.active()], ref.x[ref.partner[:, 0]]
        z1, z2 = ref.x[ref.partner[:, 1]], ref.x[ref.partner[:, 2]]
        dl = x - z
        c = 1.7 * (dl * (z1 - z2)).sum(1) / (dl * dl).sum(1)
        # the trial is x moved along the line through z by the projected difference of z1 and z2
        np.testing.assert_allclose(ref.t, x + c[:, None] * dl, rtol=1e-12, atol=1e-14)
        if d == 1:
            assert np.all(ref.q == 0.0)
        else:
            want = (d - 1) * np.log(np.linalg.norm(ref.t - z, axis=1) / np.linalg.norm(dl, axis=1))
            np.testing.assert_allclose(ref.q, want, rtol=1e-11, atol=1e-13)
            assert np.all(ref.q != 0.0)
        assert np.all(ref.whole == 1)


def test_a_snooker_walker_on_its_partner_makes_a_void_trial():
    """n2 = 0: t = x, q = -inf, lp_t = -inf; rejected, and no prior rejection."""
    d, gs = 2, 64
    prob = _uniform_problem(d, 0, 1, gs)
    x0 = np.random.default_rng(3).uniform(0.2, 0.8, (gs, d))
    ref = MR.MovesRef(prob, x0, _flat, [["snooker", 1.0]])
    ref.propose()
    k = 5
    ref.x[ref.active()[k]] = ref.x[ref.partner[k, 0]]      # walker k sits on its partner
    ref.half, ref.step = 0, 0
    ref.propose()
    w = ref.active()[k]
    assert ref.whole[k] == 0 and ref.q[k] == -np.inf and ref.lp_t[k] == -np.inf
    assert np.array_equal(ref.t[k], ref.x[w])
    ref.accept(np.zeros(gs // 2))
    assert ref.weight[w] == 2 and ref.prior_rej[w] == 0 and ref.n_accept[w] == 0


# ------------------------------------------------------------------------------ 3. the choice of kind
def test_kind_follows_the_weights():
    """20 000 steps: every member's count within 5 binomial standard deviations."""
    mix = MR.members([["stretch", 1], ["de", 1], ["snooker", 1], ["de", 0.5, {"gamma": 1.0}]], 3)
    assert [m[1] for m in mix] == [1 / 3.5, 1 / 3.5, 1 / 3.5, 0.5 / 3.5]
    N = 20000
    counts = np.bincount([MR.choose(mix, 21, s) for s in range(N)], minlength=4)
    for c, m in zip(counts, mix):
        assert abs(c - N * m[1]) < 5 * np.sqrt(N * m[1] * (1 - m[1])), (counts, m)
    # a one-member mixture draws nothing
    assert MR.choose(mix[:1], 21, 7) == 0
    # the high word of the step counts
    a = [MR.choose(mix, 21, s) for s in range(64)]
    b = [MR.choose(mix, 21, (1 << 32) + s) for s in range(64)]
    assert a != b


def test_kind_is_one_for_every_walker_offset_and_any_number_of_walkers():
    moves = [["stretch", 1], ["de", 1], ["snooker", 1]]
    made = []
    for W, walker0 in ((64, 0), (64, 4096), (256, 64)):
        prob = _uniform_problem(2, 0, 1, 64, seed=8)
        x0 = np.random.default_rng(1).uniform(0.2, 0.8, (W, 2))
        ref = MR.MovesRef(prob, x0, _flat, moves, walker0=walker0)
        ref.run(40, _flat)
        made.append(ref.kinds_made)
    assert made[0] == made[1] == made[2]
    assert set(made[0]) == {0, 1, 2}
    assert made[0][0::2] == made[0][1::2]       # both halves of a step make the same kind


# ------------------------------------------------------------------------------ 4. physics
X0, W_HEAVY = 10.0, 0.7


def two_modes(p):
    """Two unit Gaussians at x0 = -10 (weight 0.3) and +10 (weight 0.7), d = 2."""
    r2 = p[:, 1] ** 2
    return np.logaddexp(np.log(1 - W_HEAVY) - 0.5 * ((p[:, 0] + X0) ** 2 + r2),
                        np.log(W_HEAVY) - 0.5 * ((p[:, 0] - X0) ** 2 + r2))


def _two_mode_start(G, gs, seed):
    """Half of every group -- alternating walkers, so half of each half-group -- in each mode."""
    x0 = np.random.default_rng(seed).normal(0.0, 1.0, (G * gs, 2))
    x0[:, 0] += np.where(np.arange(G * gs) % 2 == 0, -X0, X0)
    return x0


def test_the_mixture_with_gamma_1_finds_the_weights_of_two_modes_and_the_stretch_move_does_not():
    """64 groups of 64, 300 steps.  The occupancy of the heavy mode, averaged over the snapshots of
    the last 100 steps, within 6 standard errors of 0.7; the standard error is that of the mean of
    the 64 groups' own time averages (independent ensembles).  The stretch reference from the same
    start stays at 0.5 +- 0.01: no trial on a line through a partner with z in [1/2, 2] lands in the
    other mode."""
    gs, G = 64, 64
    prob = _uniform_problem(2, -40, 40, gs, seed=41)
    x0 = _two_mode_start(G, gs, 6)
    ref = MR.MovesRef(prob, x0, two_modes, HOP)
    occ = []
    ref.run(300, two_modes, each=lambda r: occ.append((r.x[:, 0] > 0).reshape(G, gs).mean(1)))
    assert ref.stuck[0] == 0 and ref.bad[0] == 0
    per_group = np.mean(occ[-100:], axis=0)
    mean, se = per_group.mean(), per_group.std(ddof=1) / np.sqrt(G)
    one = np.std(occ[-1], ddof=1) / np.sqrt(G)
    print("occupancy %.4f +- %.4f (one snapshot: %.4f +- %.4f), (%.2f standard errors)" % (
        mean, se, np.mean(occ[-1]), one, (mean - W_HEAVY) / se))
    assert abs(mean - W_HEAVY) < 6 * se
    assert se < 0.01
    stretch = SR.StretchRef(prob, x0, two_modes)
    stretch.run(300, two_modes)
    got = (stretch.x[:, 0] > 0).mean()
    print("stretch: occupancy %.4f" % got)
    assert abs(got - 0.5) <= 0.01
    assert abs(got - W_HEAVY) > 6 * max(se, one)


@pytest.mark.parametrize("d", [3, 6])
@pytest.mark.parametrize("moves", [[["snooker", 1.0]], [["snooker", 0.5], ["de", 0.5]]], ids=["snooker", "snooker+de"])
def test_snooker_samples_a_unit_gaussian(moves, d):
    """64 groups of 64 from a stationary start, 250 steps, the last 150 kept: every parameter's
    variance -- its mean square about the known mean 0, which is unbiased whatever the correlation
    between the walkers of a group -- within 6 standard errors of 1, the standard error from the
    spread of the 64 groups' own time averages.  A Jacobian power other than d - 1 samples another
    law (a radial density off by a power of |x - z|)."""
    gs, G = 64, 64

    def f(p):
        return -0.5 * (p ** 2).sum(1)

    prob = _uniform_problem(d, -15, 15, gs, seed=43)
    x0 = np.random.default_rng(7).normal(0.0, 1.0, (G * gs, d))
    ref = MR.MovesRef(prob, x0, f, moves)
    sq = []
    acc = ref.run(250, f, each=lambda r: sq.append((r.x ** 2).reshape(G, gs, d).mean(1)))
    rate = acc / (250.0 * G * gs)
    per_group = np.mean(sq[-150:], axis=0)            # [G][d]
    var, se = per_group.mean(0), per_group.std(0, ddof=1) / np.sqrt(G)
    print("d = %d: acceptance %.3f, variances %s, standard errors %s" % (d, rate, np.round(var, 4), np.round(se, 4)))
    assert rate > 0.1 and ref.stuck[0] == 0
    assert np.all(np.abs(var - 1.0) < 6 * se), (var, se)
    assert np.all(se < 0.02)


# ------------------------------------------------------------------------------ 5. the sampler's side
def module_level_function(p):
    return -0.5 * (p ** 2).sum(1)


def _info(ref_a=None, ref_b=None, **like):
    ref_a = {"dist": "norm", "loc": 0, "scale": 1} if ref_a is None else ref_a
    ref_b = {"dist": "norm", "loc": 0.5, "scale": 1} if ref_b is None else ref_b
    return {"likelihood": {"f": {"class": "device_function", "function": module_level_function, **like}},
            "params": {"a": {"prior": {"min": -8, "max": 8}, "ref": ref_a, "proposal": 1},
                       "b": {"prior": {"min": -6, "max": 30}, "ref": ref_b, "proposal": 1}}}


def no_engine(*a, **k):
    raise AssertionError("the engine must not be created")


no_engine.max_dim = lambda: 256


class NoEngine(MCMCHip):
    _engine_factory = staticmethod(no_engine)


BASE = {"seed": 1, "n_walkers": 128, "group_size": 64, "max_samples": 100, "moves": HOP}


def test_option_defaults_and_parsing():
    assert "moves" in HIP_DEFAULTS and HIP_DEFAULTS["moves"] is None
    import mcmc_hip
    assert mcmc_hip.MCMCHip.moves is None
    from cobaya_amd.moves import normalised, parse
    got = parse([["stretch", 2], ["de", 1], ["snooker", 1.0, {}], ["de", 4, {"gamma": 1.0, "sigma": 0}]], 2)
    assert got == [(0, 2.0, 2.0, 0.0), (1, 1.0, 2.38 / np.sqrt(4.0), 1e-5), (2, 1.0, 1.7, 0.0), (1, 4.0, 1.0, 0.0)]
    assert [m[1] for m in normalised(got)] == [0.25, 0.125, 0.125, 0.5]
    # the reference fills in the same defaults and normalises alike
    assert normalised(got) == MR.members([["stretch", 2], ["de", 1], ["snooker", 1.0, {}],
                                          ["de", 4, {"gamma": 1.0, "sigma": 0}]], 2)
    # a served mixture reaches the engine (which this double refuses to make), tuples or lists
    for moves in (HOP, (("snooker", "1"),), [["stretch", 1, {"a": 1.5}]]):
        with pytest.raises(AssertionError, match="the engine must not be created"):
            NoEngine({**BASE, "moves": moves}, ProblemSpec.from_info(_info()))
    # ... and without the option nothing of it is in force
    s = MCMCHip.__new__(MCMCHip)
    assert s.moves is None and s.mixture is None


def test_sampler_refuses_by_name_before_the_engine():
    def refused(match, info=None, **opts):
        with pytest.raises(LoggedError, match=match):
            NoEngine({**BASE, **opts}, ProblemSpec.from_info(info or _info()))

    # the option itself
    refused("moves and move: 'stretch' are both given", move="stretch")
    refused("moves and move: 'metropolis' are both given", move="metropolis")
    refused(r"moves must be a list of 1 \.\. 8 members", moves=[])
    refused(r"moves must be a list of 1 \.\. 8 members", moves=[["de", 1]] * 9)
    refused(r"moves must be a list of 1 \.\. 8 members", moves="de")
    refused(r"moves\[1\] must be \[kind, weight\] or \[kind, weight, \{params\}\]", moves=[["de", 1], ["de"]])
    refused(r"moves\[1\]: unknown kind 'walk'", moves=[["de", 1], ["walk", 1]])
    refused(r"moves\[0\]: unknown kind 'metropolis'", moves=[["metropolis", 1]])
    for w in (0, -1.0, float("inf"), float("nan")):
        refused(r"moves\[1\] \(de\): the weight must be positive and finite", moves=[["de", 1], ["de", w]])
    refused(r"moves\[0\]: the weight must be a number, got 'much'", moves=[["de", "much"]])
    for a in (1.0, 0.5, float("inf"), float("nan")):
        refused(r"moves\[0\] \(stretch\): a must be finite and > 1", moves=[["stretch", 1, {"a": a}]])
    for g in (0.0, -1.0, float("inf"), float("nan")):
        refused(r"moves\[0\] \(de\): gamma must be finite and > 0", moves=[["de", 1, {"gamma": g}]])
        refused(r"moves\[1\] \(snooker\): gamma must be finite and > 0", moves=[["de", 1], ["snooker", 1, {"gamma": g}]])
    for sg in (-1e-9, float("nan"), float("inf")):
        refused(r"moves\[0\] \(de\): sigma must be finite and >= 0", moves=[["de", 1, {"sigma": sg}]])
    refused(r"moves\[0\] \(snooker\): unknown parameter 'sigma'", moves=[["snooker", 1, {"sigma": 0.1}]])
    refused(r"moves\[0\] \(de\): the parameters must be a dict", moves=[["de", 1, 0.5]])
    # the limits of move: stretch, each by name
    refused("moves: likelihood 'gaussian_mixture' is not served", info=QUICK)
    two = _info()
    two["likelihood"] = {"f": {"class": "device_function", "function": module_level_function, "input_params": ["a"]},
                         "g": {"class": "device_function", "function": module_level_function,
                               "input_params": ["a", "b"]}}
    refused("moves: several device_function likelihoods are not served", info=two)
    refused("drag: True is not served", drag=True, blocking=[[1, ["a"]], [10, ["b"]]])
    refused("parameter blocks", blocking=[[1, ["a"]], [2, ["b"]]])
    info = _info()
    info["params"]["a"]["periodic"] = True
    refused("periodic parameters are not served", info=info)
    refused("emit: chains is not served", emit="chains")
    refused("evaluation: incremental is not served", evaluation="incremental")
    wide = {"likelihood": {"f": {"class": "device_function", "function": module_level_function}},
            "params": {"p%02d" % i: {"prior": {"min": 0, "max": 1}, "proposal": 0.1} for i in range(17)}}
    refused(r"moves: group_size: 64 < 4 d = 68.*use a larger group_size \(256 serves d <= 64\)", info=wide)
    with pytest.raises(AssertionError, match="the engine must not be created"):
        NoEngine({**BASE, "n_walkers": 256, "group_size": 128}, ProblemSpec.from_info(wide))
    refused(r"moves: `ref` of \['a'\] is a fixed point.*give `ref` as a pdf", info=_info(ref_a=0))


def test_no_proposal_is_learned_and_one_log_line_says_so(caplog):
    import logging

    class Stop(Exception):
        pass

    def stop(*a, **k):
        raise Stop()

    stop.max_dim = lambda: 256

    class Probe(MCMCHip):
        _engine_factory = staticmethod(stop)

        def _fail(self, *a, **k):       # (whatever follows the factory's failure is not under test)
            raise Stop()

    seen = {}

    class Keep(Probe):
        def _check_move(self, spec, d):
            super()._check_move(spec, d)
            seen["learn"], seen["mixture"] = self.learn_proposal, self.mixture

    with caplog.at_level(logging.INFO):
        with pytest.raises(Stop):
            Keep({**BASE}, ProblemSpec.from_info(_info()))
    assert seen["learn"] is False
    assert [m[0] for m in seen["mixture"]] == [1, 1] and [m[1] for m in seen["mixture"]] == [0.8, 0.2]
    lines = [r.getMessage() for r in caplog.records if "no proposal covariance is learned" in r.getMessage()]
    assert len(lines) == 1 and lines[0].startswith("moves")


class MoveDouble(OracleEngine):
    """The oracle-backed engine double; `set_moves` is accepted (the resume guard is the sampler's)."""

    def set_moves(self, moves):
        pass


class OnDouble(MCMCHip):
    _engine_factory = staticmethod(MoveDouble)


class ForcedMixture(OnDouble):
    """Says `moves` whatever the likelihood: only the state file's guard is under test."""

    def _check_move(self, spec, d):
        from cobaya_amd.moves import normalised, parse
        self.stretch = False
        self.mixture = normalised(parse(self.moves, d)) if self.moves is not None else None


def test_resume_with_another_mixture_is_refused(tmp_path):
    opts = {"seed": 21, "n_walkers": 128, "group_size": 64, "steps_per_launch": 40, "max_samples": 20000,
            "Rminus1_stop": 0.0, "learn_every": "20d"}
    spec = ProblemSpec.from_info(QUICK)
    d = len(spec.sampled)
    # written without the option: no key (the file of today's runs is unchanged) ...
    p = str(tmp_path / "m")
    s = OnDouble(opts, spec, output=p)
    s.run()
    s.close()
    assert "moves" not in np.load(p + ".1.state.npz").files
    OnDouble({**opts, "max_samples": 30000}, spec, output=p, resume=True).close()
    with pytest.raises(LoggedError, match=r"cannot resume -- the run was written with moves: None and now has moves: "
                                          r"\[de 0.8 \(gamma: [0-9.]+, sigma: 1e-05\), de 0.2 \(gamma: 1, sigma: 1e-05\)\]"):
        ForcedMixture({**opts, "moves": HOP}, spec, output=p, resume=True)
    # ... written with a mixture: kinds, normalised weights and parameters
    q = str(tmp_path / "s")
    s = ForcedMixture({**opts, "moves": HOP}, spec, output=q)
    s.run()
    s.close()
    assert np.load(q + ".1.state.npz")["moves"].tolist() == [[1.0, 0.8, 2.38 / np.sqrt(2.0 * d), 1e-5],
                                                             [1.0, 0.2, 1.0, 1e-5]]
    # (weights are compared normalised: 4 : 1 is the same mixture)
    ForcedMixture({**opts, "max_samples": 30000, "moves": [["de", 4], ["de", 1, {"gamma": 1.0}]]}, spec, output=q,
                  resume=True).close()
    with pytest.raises(LoggedError, match=r"written with moves: \[de 0.8 .*\] and now has moves: None"):
        OnDouble(opts, spec, output=q, resume=True)
    with pytest.raises(LoggedError, match=r"and now has moves: \[de 0.8 .*, snooker 0.2 \(gamma: 1.7\)\]"):
        ForcedMixture({**opts, "moves": [["de", 0.8], ["snooker", 0.2]]}, spec, output=q, resume=True)
    with pytest.raises(LoggedError, match=r"and now has moves: \[de 0.8 .*, de 0.2 \(gamma: 0.9, sigma: 1e-05\)\]"):
        ForcedMixture({**opts, "moves": [["de", 0.8], ["de", 0.2, {"gamma": 0.9}]]}, spec, output=q, resume=True)
