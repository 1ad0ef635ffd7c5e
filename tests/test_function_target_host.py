"""Function targets (likelihood class `device_function`), the parts that need no device:
parsing, the reference of the step (tests/function_ref.py) tied to the oracle's own from-scratch
step of the `one` likelihood, and golden G14 -- the reference's `Model.logposterior` of a model
with an external Python likelihood function."""
import numpy as np
import pytest

from cobaya_amd.model import ProblemSpec, UnsupportedModel
from oracle import cbind as O
from tests import function_ref as FR


def banana_np(p, beta=0.5, s=0.5):
    return -0.5 * (p[:, 0] ** 2 + ((p[:, 1] - beta * p[:, 0] ** 2) / s) ** 2)


def module_level_function(p):   # resolved as "tests.test_function_target_host:module_level_function"
    return -0.5 * (p ** 2).sum(1)


def _info(function=module_level_function, **like):
    return {"likelihood": {"banana": {"class": "device_function", "function": function, **like}},
            "params": {"a": {"prior": {"min": -8, "max": 8}, "ref": 0, "proposal": 1},
                       "b": {"prior": {"min": -6, "max": 30}, "ref": 0.5, "proposal": 1}}}


# ------------------------------------------------------------------------------ 1. parsing
def test_from_info_accepts_a_callable_and_a_module_name_string():
    spec = ProblemSpec.from_info(_info())
    assert spec.like_kind == "device_function" and spec.like_name == "banana"
    assert spec.n_modes == 0 and spec.d == 2 and spec.function is module_level_function
    assert not spec.has_derived and spec.components[0]["idx"] == [0, 1]
    spec = ProblemSpec.from_info(_info("tests.test_function_target_host:module_level_function"))
    assert callable(spec.function) and spec.function.__name__ == "module_level_function"
    assert spec.function.__module__ == "tests.test_function_target_host"
    # routing as for the Gaussians: an explicit list or a prefix, every sampled parameter in order
    spec = ProblemSpec.from_info(_info(input_params=["a", "b"]))
    assert spec.like_kind == "device_function"


def test_from_info_rejects_by_name():
    with pytest.raises(UnsupportedModel, match="`function` must be a callable"):
        ProblemSpec.from_info(_info(function=3.5))
    with pytest.raises(UnsupportedModel, match="`function` must be a callable"):
        ProblemSpec.from_info(_info(function=None))
    with pytest.raises(UnsupportedModel, match="package.module:name"):
        ProblemSpec.from_info(_info(function="no_colon_here"))
    with pytest.raises(UnsupportedModel, match="could not be resolved"):
        ProblemSpec.from_info(_info(function="tests.test_function_target_host:absent"))
    info = _info()
    info["params"]["chi"] = {"latex": "x"}          # a derived parameter
    with pytest.raises(UnsupportedModel, match="no derived parameters"):
        ProblemSpec.from_info(info)
    info = _info()
    info["likelihood"]["other"] = {"class": "one"}  # a second likelihood beside it
    with pytest.raises(UnsupportedModel, match="must be the only likelihood"):
        ProblemSpec.from_info(info)
    with pytest.raises(UnsupportedModel, match="all sampled parameters"):
        ProblemSpec.from_info(_info(input_params=["a"]))
    with pytest.raises(UnsupportedModel, match="all sampled parameters"):
        ProblemSpec.from_info(_info(input_params=["b", "a"]))     # not in sampled order
    with pytest.raises(UnsupportedModel, match="all sampled parameters"):
        ProblemSpec.from_info(_info(input_params_prefix="a"))
    with pytest.raises(UnsupportedModel, match="unknown options"):
        ProblemSpec.from_info(_info(means=[0, 0]))


def test_sampler_refuses_unserved_options_by_name_before_the_engine():
    from cobaya_amd.sampler import LoggedError, MCMCHip

    def no_engine(*a, **k):
        raise AssertionError("the engine must not be created")
    no_engine.max_dim = lambda: 256     # (the HIP engine's cap: d = 129 passes the general one)

    class NoEngine(MCMCHip):
        _engine_factory = staticmethod(no_engine)

    base = {"seed": 1, "n_walkers": 128, "group_size": 64, "max_samples": 100}

    def refused(match, info=None, **opts):
        with pytest.raises(LoggedError, match=match):
            NoEngine({**base, **opts}, ProblemSpec.from_info(info or _info()))

    refused("emit: chains is not served", emit="chains")
    refused("shared_basis: False is not served", shared_basis=False)
    refused("evaluation: incremental is not served", evaluation="incremental")
    refused("drag: True is not served", drag=True, blocking=[[1, ["a"]], [10, ["b"]]])
    refused("parameter blocks", blocking=[[1, ["a"]], [2, ["b"]]])
    info = _info()
    info["params"]["a"]["periodic"] = True
    refused("periodic parameters are not served", info=info)
    big = {"likelihood": {"f": {"class": "device_function", "function": module_level_function}},
           "params": {"p%03d" % i: {"prior": {"min": 0, "max": 1}, "ref": 0.5, "proposal": 0.1}
                      for i in range(129)}}
    refused("d = 129 > 128", info=big)


# ------------------------------------------------------------------------------ 2. the reference
def _mixed_problem(d, rng, gs=64, seed=11, temperature=1.5, max_tries=None):
    kinds = np.array([1 if i % 3 == 1 else 0 for i in range(d)], np.int32)
    a = np.where(kinds == 1, 0.5, 0.0)
    b = np.where(kinds == 1, 0.3, 1.0)
    A = rng.standard_normal((d, d)) / np.sqrt(d)
    cov = 0.01 * (A @ A.T + np.eye(d))
    T = np.linalg.cholesky(cov) * (2.4 / np.sqrt(d))
    return FR.problem(d, kinds, a, b, T, group_size=gs, seed=seed, temperature=temperature,
                      max_tries=max_tries), cov


def _assert_equal_states(ref, st):
    assert np.array_equal(ref.x.view(np.uint64), st.x.view(np.uint64))
    for k in ("logpost", "logprior", "loglike"):
        assert np.array_equal(getattr(ref, k).view(np.uint64), getattr(st, k).view(np.uint64)), k
    for k in ("weight", "prior_rej", "burn_left", "n_accept"):
        assert np.array_equal(getattr(ref, k), getattr(st, k)), k


@pytest.mark.parametrize("d", [1, 2, 30, 33, 100, 128])
def test_reference_with_zero_function_equals_the_oracle_on_one(d):
    """f = 0: the function target IS the `one` likelihood.  State, the three log-densities,
    weight, prior_rej, burn_left and n_accept equal oracle.cbind.State.run (from scratch) bit for
    bit over three uneven launches; temperature 1.5, burn-in 3, mixed uniform / normal priors,
    walkers started against a bound (prior_rej > 0)."""
    rng = np.random.default_rng(100 + d)
    prob, cov = _mixed_problem(d, rng)
    W = 128
    x0 = np.clip(0.5 + 0.3 * rng.standard_normal((W, d)) * np.sqrt(np.diag(cov)), 0.01, 0.99)
    x0[::4, 0] = 0.001          # against the lower bound of the first (uniform) parameter
    st = O.State(prob, x0, burn_in=3)
    ref = FR.FunctionRef(prob, x0, np.zeros(W), burn_in=3)
    _assert_equal_states(ref, st)
    zero = lambda t: np.zeros(len(t))   # noqa: E731
    seen_rej = 0
    for n in (d + 3, 1, 2 * d + 5):
        acc_o = st.run(n, n_threads=2)
        acc_r = ref.run(n, zero)
        seen_rej += int(ref.prior_rej.sum())
        assert acc_o == acc_r
        _assert_equal_states(ref, st)
    assert ref.n_accept.sum() > 0 and seen_rej > 0
    assert (ref.burn_left < 4).any()
    assert not st.stuck[0] and not ref.stuck[0] and not ref.bad[0]


def test_reference_reports_stuck_like_the_oracle():
    d = 2
    rng = np.random.default_rng(3)
    prob, cov = _mixed_problem(d, rng, max_tries=2.0)
    W = 64
    x0 = np.clip(0.5 + 0.3 * rng.standard_normal((W, d)) * np.sqrt(np.diag(cov)), 0.01, 0.99)
    st = O.State(prob, x0)          # burn_in 0: burn_left 1, ten times max_tries until the first accept
    ref = FR.FunctionRef(prob, x0, np.zeros(W))
    # a wide proposal: most trials leave the box or the normal prior's bulk
    prob.set_T(np.eye(d) * 5.0)
    st.run(60, n_threads=1)
    ref.run(60, lambda t: np.zeros(len(t)))
    _assert_equal_states(ref, st)
    assert st.stuck[0] and ref.stuck[0]


def test_reference_rejects_minus_inf_and_flags_nan_inside_the_support():
    d = 2
    rng = np.random.default_rng(4)
    prob, cov = _mixed_problem(d, rng, temperature=1.0)
    W = 64
    x0 = np.clip(0.5 + 0.2 * rng.standard_normal((W, d)) * np.sqrt(np.diag(cov)), 0.05, 0.95)
    ref = FR.FunctionRef(prob, x0, np.zeros(W))
    x_before = ref.x.copy()
    t = ref.propose().copy()
    ll = np.where(np.arange(W) % 2 == 0, -np.inf, 0.0)
    ll[np.isinf(ref.lp_t)] = np.nan          # NaN outside the support is ignored
    ref.accept(ll)
    assert np.array_equal(ref.x[::2], x_before[::2])           # -inf: an ordinary rejection
    assert not ref.bad[0]
    acc = ref.n_accept == 1                  # accepted: the state is the trial; else it stayed
    assert acc.any() and not acc[::2].any() and not acc[np.isinf(ref.lp_t)].any()
    assert np.array_equal(ref.x[acc], t[acc]) and np.array_equal(ref.x[~acc], x_before[~acc])
    assert np.array_equal(ref.weight, np.where(acc, 1, 2))
    ref.propose()
    ll = np.zeros(W)
    first = int(np.flatnonzero(np.isfinite(ref.lp_t))[0])
    ll[first] = np.nan
    ref.accept(ll)
    assert ref.bad[0] == 1 + first


# ------------------------------------------------------------------------------ 3. golden G14
def test_g14_external_function_logposterior(golden):
    """The reference's Model.logposterior with an external Python likelihood function (the banana,
    mixed uniform / normal priors) at 52 points, six of them on or outside the bounds: the
    restatement's evaluation reproduces log-prior and log-likelihood to rtol 1e-12 (the bar of
    G4 / G5) and the -inf pattern exactly."""
    g = golden("g14_external_function")
    pts = g["points"]
    beta, s, c_loc, c_scale = (float(g[k]) for k in ("beta", "s", "c_loc", "c_scale"))

    def f(p):
        return (-0.5 * (p[:, 0] ** 2 + ((p[:, 1] - beta * p[:, 0] ** 2) / s) ** 2)
                - 0.5 * ((p[:, 2] - c_loc) / c_scale) ** 2)

    prob = FR.problem(3, g["kinds"], g["a"], g["b"], np.eye(3))
    lp, ll = FR.evaluate(prob, pts, f)
    assert np.array_equal(np.isinf(lp), np.isinf(g["logprior"]))
    assert np.array_equal(np.isinf(ll), np.isinf(g["loglike"]))
    assert np.isinf(g["logprior"]).sum() == 4
    ok = np.isfinite(lp)
    np.testing.assert_allclose(lp[ok], g["logprior"][ok], rtol=1e-12, atol=0)
    np.testing.assert_allclose(ll[ok], g["loglike"][ok], rtol=1e-12, atol=0)
