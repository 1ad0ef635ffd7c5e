"""128 < d <= 256 on the MI355X (huge_kernels.hip): the sampler runs such models on the target, the
kernels equal the oracle (evaluation, moments) and the d-agnostic restatement of its step
(tests/huge_step_ref.c) bit for bit, walker shards compose, and every unserved option is refused
by name."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from cobaya_amd import run  # noqa: E402
from cobaya_amd.engine import ChainStuck, Engine, EngineError, max_dim  # noqa: E402
from cobaya_amd.model import ProblemSpec  # noqa: E402
from cobaya_amd.sampler import LoggedError, MCMCHip  # noqa: E402
from oracle import cbind as O  # noqa: E402
from tests import huge_ref  # noqa: E402


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def kl_norm(m1, S1, m2, S2):
    """KL(N1 || N2), cobaya/tools.py:732-743."""
    d = len(m1)
    S2i = np.linalg.inv(S2)
    return 0.5 * (np.trace(S2i @ S1) + (m1 - m2) @ S2i @ (m1 - m2) - d
                  + np.linalg.slogdet(S2)[1] - np.linalg.slogdet(S1)[1])


def _model(d, K, seed, normal=True):
    rng = np.random.default_rng(seed)
    kinds = np.array([1 if (normal and i % 3 == 1) else 0 for i in range(d)], np.int32)
    a = np.where(kinds == 1, 0.5, 0.0)
    b = np.where(kinds == 1, 0.4, 1.0)
    means, covs = [], []
    for _ in range(max(K, 1)):
        A = rng.standard_normal((d, d)) / np.sqrt(d)
        covs.append(0.0025 * (0.5 * A @ A.T + 0.5 * np.eye(d)))
        means.append(0.5 + 0.02 * rng.standard_normal(d))
    return kinds, a, b, means[:K], covs[:K], rng


def _engine(d, K, W, gs, seed, bgs=None, walker_offset=0, **kw):
    kinds, a, b, means, covs, rng = _model(d, K, seed, normal=kw.pop("normal", True))
    eng = Engine(d, W, group_size=gs, device=0, seed=seed, incremental=True, basis_group_size=bgs,
                 walker_offset=walker_offset, **kw)
    eng.set_prior(kinds, a, b)
    if K:
        eng.set_target_gaussian_mixture(means, covs)
    else:
        eng.set_target_one()
    eng.set_proposal_cov(covs[0] if K else 0.0025 * np.eye(d))
    return eng, kinds, a, b, means, covs, rng


def test_max_dim():
    assert max_dim() == 256


def test_sampler_runs_d200():
    """Fails without the feature: a d = 200 Gaussian was refused at initialize."""
    info, mean, cov = huge_ref.gaussian_info(200, seed=3)
    info["sampler"] = {"mcmc_hip": {"seed": 5, "n_walkers": 4096, "group_size": 64,
                                    "max_samples": 4096 * 400, "Rminus1_stop": 0.0}}
    _, sampler = run(info)
    df = sampler.products()["sample"].data
    assert sum(c.startswith("p") for c in df.columns) == 200
    assert len(df) > 0
    name = sampler.engine.last_step_kernel()
    assert name.startswith("mcmc::huge_step_kernel"), name


def test_real_run_d200_targets_the_distribution():
    """d = 200, one random correlated Gaussian, 16 384 walkers, default options (learning
    checkpoints, R-1 of the means) with Rminus1_stop 0.05, run for 6e4 steps per walker: the
    checkpoint runs in the mode auto chose for one process (the solve on the host:
    device_checkpoint False), and the final ensemble's Gaussian fit is within KL 1.0 of the target
    -- the sampling floor of a fit from N = 16 384 points is d (d + 1) / (4 N) = 0.61.  The stop
    rule itself is NOT reached here: with 256 chains in 200 dimensions the R-1 estimate fell to
    0.22 after 1.5e5 steps and 0.087 after 4.1e5, not to 0.05 (profiles/r07_huge_dim.txt)."""
    d, W = 200, 16384
    info, mean, cov = huge_ref.gaussian_info(d, seed=8)
    sd = np.sqrt(np.diag(cov))
    for i in range(d):   # walkers start spread around the mean, not on one point
        info["params"]["p%d" % i]["ref"] = {"dist": "norm", "loc": float(mean[i]), "scale": float(sd[i])}
    info["sampler"] = {"mcmc_hip": {"seed": 13, "n_walkers": W, "Rminus1_stop": 0.05,
                                    "max_samples": W * 60000}}
    _, sampler = run(info)
    assert sampler.device_checkpoint is False and not sampler._device_ckpt
    assert np.isfinite(sampler.Rminus1_last)   # (the convergence checkpoints ran)
    assert sampler.engine.last_step_kernel().startswith("mcmc::huge_step_kernel")
    x = sampler.engine.get_state()["x"]
    kl = kl_norm(x.mean(axis=0), np.cov(x.T), mean, cov)
    assert kl < 1.0, (kl, sampler.Rminus1_last)


def test_one_likelihood_runs_d150():
    """The `one` likelihood (prior only) at d = 150 through the sampler."""
    d = 150
    info = {"likelihood": {"one": None},
            "params": {"p%d" % i: ({"prior": {"dist": "norm", "loc": 0.0, "scale": 1.0}} if i % 2 else
                                   {"prior": {"min": -1.0, "max": 1.0}}) for i in range(d)},
            "sampler": {"mcmc_hip": {"seed": 4, "n_walkers": 1024, "group_size": 64,
                                     "max_samples": 1024 * 300, "Rminus1_stop": 0.0}}}
    _, sampler = run(info)
    assert sampler.engine.last_step_kernel().startswith("mcmc::huge_step_kernel")
    x = sampler.engine.get_state()["x"]
    assert np.all(np.abs(x[:, 0::2]) <= 1.0)
    assert len(sampler.products()["sample"].data) > 0


@pytest.mark.parametrize("d", [129, 131, 192, 256])
@pytest.mark.parametrize("K", [0, 1, 3])
def test_evaluate_equals_oracle(d, K):
    eng, kinds, a, b, means, covs, rng = _engine(d, K, 64, 64, 7)
    x = np.clip(0.5 + 0.1 * rng.standard_normal((200, d)), 0.001, 0.999)
    x[3, 5] = 1.5   # outside
    lp, ll = eng.evaluate(x)[:2]
    prob = O.Problem(d, kinds, a, b, means=means if K else None, covs=covs if K else None,
                     derived=eng.derived_constants())
    plp, pll = prob.evaluate(x)
    eng.close()
    assert np.array_equal(_bits(lp), _bits(plp)) and np.array_equal(_bits(ll), _bits(pll))


# (d, K, W, group_size, case): temperature 1.5 with two modes, burn-in with one; "edge": walkers
# start against a bound so that trials leave the prior (prior_rej); "stuck": and max_tries = 3
@pytest.mark.parametrize("d,K,W,gs,case", [(129, 1, 256, 64, ""), (160, 2, 1024, 256, ""),
                                           (256, 4, 256, 64, ""), (160, 1, 1024, 64, "edge"),
                                           (160, 0, 1024, 256, "edge"), (129, 0, 256, 64, ""),
                                           (131, 1, 256, 64, "stuck")])
def test_steps_equal_restatement(d, K, W, gs, case):
    seed = 100 + d + K
    temperature = 1.5 if K == 2 else 1.0
    burn_in = 3 if K == 1 else 0
    max_tries = 3.0 if case == "stuck" else None
    eng, kinds, a, b, means, covs, rng = _engine(d, K, W, gs, seed, temperature=temperature,
                                                 burn_in=burn_in, max_tries=max_tries)
    m0 = means[0] if K else np.full(d, 0.5)
    sd = np.sqrt(np.diag(covs[0])) if K else np.full(d, 0.05)
    x0 = np.clip(m0 + 0.5 * rng.standard_normal((W, d)) * sd, 0.001, 0.999)
    if case:
        x0[:, 0] = 0.9999   # a uniform [0, 1] coordinate against its upper bound
    eng.set_state(x0)
    n = 2 * d + 3
    eng.step(n // 2)
    eng.step(n - n // 2)
    try:   # (the stuck report is raised by the sync after the steps have run)
        eng.sync()
        stuck = 0
    except ChainStuck:
        stuck = 1
    s = eng.get_full_state()
    kern = eng.last_step_kernel()
    prob = O.Problem(d, kinds, a, b, means=means if K else None, covs=covs if K else None,
                     T=eng.get_proposal_transform(), group_size=gs, seed=seed,
                     temperature=temperature, incremental=K > 0,
                     max_tries=max_tries if max_tries is not None else 40 * d,
                     derived=eng.derived_constants())
    eng.close()
    ref = huge_ref.fresh_state(prob, x0, burn_in=burn_in)
    huge_ref.run(prob, ref, n)
    assert kern.startswith("mcmc::huge_step_kernel")
    assert np.array_equal(_bits(s["x"]), _bits(ref["x"]))
    for k in ("logpost", "logprior", "loglike"):
        assert np.array_equal(_bits(s[k]), _bits(ref[k])), k
    for k in ("weight", "n_accept", "burn_left", "prior_rej"):
        assert np.array_equal(s[k], ref[k]), k
    assert 0 < ref["n_accept"].sum() < W * n
    if case == "edge" and K == 0:   # (flat in that coordinate: walkers stay at the bound)
        assert ref["prior_rej"].max() > 0
    # (which walker reports first is a race on the device; whether one does is not)
    assert (stuck != 0) == (ref["stuck"][0] != 0)
    assert (stuck != 0) == (case == "stuck")


def test_moments_equal_oracle():
    d, W, gs = 200, 512, 64
    eng, kinds, a, b, means, covs, rng = _engine(d, 1, W, gs, 9)
    x0 = np.clip(means[0] + 0.5 * rng.standard_normal((W, d)) * np.sqrt(np.diag(covs[0])), 0.001, 0.999)
    eng.set_state(x0)
    eng.step(20)
    xa = eng.get_state()["x"]
    eng.accumulate_moments()
    eng.step(7)
    eng.accumulate_moments()
    n, gsum, S = eng.read_moments()
    x1 = eng.get_state()["x"]
    eng.close()
    assert n == 2
    gs_ref = np.zeros((W // gs, d))
    S_ref = np.zeros((d, d))
    O.moments(xa, gs, group_sum=gs_ref, pooled=S_ref)   # the two snapshots, in order
    O.moments(x1, gs, group_sum=gs_ref, pooled=S_ref)
    assert np.array_equal(_bits(gsum), _bits(gs_ref))
    assert np.array_equal(_bits(S), _bits(S_ref))


def test_walker_shards_compose():
    d, W, gs, n = 160, 512, 64, 170
    full, kinds, a, b, means, covs, rng = _engine(d, 1, W, gs, 21)
    x0 = np.clip(means[0] + 0.5 * rng.standard_normal((W, d)) * np.sqrt(np.diag(covs[0])), 0.001, 0.999)
    full.set_state(x0)
    full.step(n)
    sf = full.get_state()
    full.close()
    for half in (0, 1):
        e, *_ = _engine(d, 1, W // 2, gs, 21, walker_offset=half * W // 2)
        e.set_state(x0[half * W // 2:(half + 1) * W // 2])
        e.step(n)
        s = e.get_state()
        e.close()
        assert np.array_equal(_bits(s["x"]), _bits(sf["x"][half * W // 2:(half + 1) * W // 2]))
        assert np.array_equal(_bits(s["logpost"]), _bits(sf["logpost"][half * W // 2:(half + 1) * W // 2]))


def _sampler(d, K=1, **opts):
    info, _, _ = huge_ref.gaussian_info(d, K=K, seed=2)
    o = {"seed": 1, "n_walkers": 1024, "group_size": 64, "max_samples": 1024 * 10}
    o.update(opts)
    return MCMCHip(o, ProblemSpec.from_info(info))


_HALVES = [["p%d" % i for i in range(100)], ["p%d" % i for i in range(100, 200)]]


@pytest.mark.parametrize("opts,needle", [
    ({"evaluation": "full"}, "evaluation: full"),
    ({"shared_basis": False}, "shared_basis: False"),
    ({"emit": "chains"}, "emit: chains"),
    ({"device_checkpoint": True}, "device_checkpoint"),
    ({"blocking": [[1, _HALVES[0]], [2, _HALVES[1]]]}, "parameter blocks"),
    ({"drag": True, "blocking": [[1, _HALVES[0]], [4, _HALVES[1]]]}, "drag: True"),
])
def test_refusals_name_the_option(opts, needle):
    with pytest.raises(LoggedError, match=needle):
        _sampler(200, **opts)


def test_refuses_periodic_parameters():
    info, _, _ = huge_ref.gaussian_info(200, seed=2)
    info["params"]["p7"]["periodic"] = True
    with pytest.raises(LoggedError, match="periodic parameters"):
        MCMCHip({"seed": 1, "n_walkers": 1024, "group_size": 64, "max_samples": 10240},
                ProblemSpec.from_info(info))


def test_refuses_k5_and_d257():
    with pytest.raises(LoggedError, match="5 mixture modes"):
        _sampler(200, K=5)
    with pytest.raises(LoggedError, match="at most 256 parameters"):
        _sampler(257)
    with pytest.raises(EngineError, match="largest dimension"):
        Engine(257, 256, group_size=64, device=0, incremental=True)
    with pytest.raises(EngineError, match="incremental"):
        Engine(200, 256, group_size=64, device=0, incremental=False)
    # the process is healthy: a served shape runs after the refusals
    e, *_ = _engine(130, 1, 256, 64, 3)
    e.set_state(np.full((256, 130), 0.5))
    e.step(3)
    e.close()


# the kernels these shapes ran on before d > 128 was served (the parent commit's launcher choices)
SMALL_D_KERNELS = {30: "mcmc::step_inc_kernel<8, 0, true> (d=30)",
                   100: "mcmc::step_inc_kernel<25, 0, true> (d=100)",
                   128: "mcmc::step_inc_kernel<32, 0, true> (d=128)"}


@pytest.mark.parametrize("d", [30, 100, 128])
def test_small_d_keeps_its_kernels(d):
    e, kinds, a, b, means, covs, rng = _engine(d, 1, 1024, 64, 4, normal=False)
    e.set_state(np.clip(means[0] + 0.01 * rng.standard_normal((1024, d)), 0.001, 0.999))
    e.step(5)
    k = e.last_step_kernel()
    e.close()
    assert k == SMALL_D_KERNELS[d]
