"""The d-agnostic restatement of the incremental step (tests/huge_step_ref.c) against the oracle's
orc_run where both run (d <= 128): state, log-posterior, weights and accept counts bit for bit.  It
is the reference of the d > 128 kernels (tests/test_gpu_huge_dim.py).  And the sampler on the CPU
oracle keeps its cap of 128: a d = 129 model is refused with a message, before orc_run sees it."""
import numpy as np
import pytest

from oracle import cbind as O
from tests import huge_ref


def _problem(d, K, rng, gs=64, seed=11, temperature=1.0):
    """K = 0: the `one` likelihood, which orc_run steps from scratch (incremental = False)."""
    kinds = np.array([1 if i % 3 == 1 else 0 for i in range(d)], np.int32)
    a = np.where(kinds == 1, 0.5, 0.0)
    b = np.where(kinds == 1, 0.3, 1.0)
    means = [0.5 + 0.05 * rng.standard_normal(d) for _ in range(max(K, 1))]
    covs = []
    for _ in range(max(K, 1)):
        A = rng.standard_normal((d, d)) / np.sqrt(d)
        covs.append(0.01 * (A @ A.T + np.eye(d)))
    cov = covs[0]
    T = np.linalg.cholesky(cov) * (2.4 / np.sqrt(d))
    return O.Problem(d, kinds, a, b, means=means if K else None, covs=covs if K else None, T=T,
                     group_size=gs, seed=seed, temperature=temperature,
                     incremental=K > 0), means[0], cov


@pytest.mark.parametrize("d", [2, 31, 64, 100, 128])
@pytest.mark.parametrize("K", [0, 1, 3])
def test_restatement_equals_orc_run(d, K):
    rng = np.random.default_rng(d * 10 + K)
    prob, mean, cov = _problem(d, K, rng)
    W, n = 128, 2 * d + 3
    x0 = np.clip(mean + 0.3 * rng.standard_normal((W, d)) * np.sqrt(np.diag(cov)), 0.01, 0.99)
    st = O.State(prob, x0)
    st.run(n, n_threads=2)
    ref = huge_ref.fresh_state(prob, x0)
    huge_ref.run(prob, ref, n)
    assert np.array_equal(ref["x"].view(np.uint64), st.x.view(np.uint64))
    for k in ("logpost", "logprior", "loglike"):
        assert np.array_equal(ref[k].view(np.uint64), getattr(st, k).view(np.uint64)), k
    assert np.array_equal(ref["weight"], st.weight)
    assert np.array_equal(ref["n_accept"], st.n_accept)
    assert np.array_equal(ref["prior_rej"], st.prior_rej)
    assert ref["n_accept"].sum() > 0


def test_restatement_crosses_the_refresh_of_y():
    """Steps across a multiple of refresh_every (40 d) from a mid-run state: equal to orc_run."""
    d, K = 31, 1
    rng = np.random.default_rng(5)
    prob, mean, cov = _problem(d, K, rng)
    W, n0 = 64, 40 * d - 5
    x0 = np.clip(mean + 0.3 * rng.standard_normal((W, d)) * np.sqrt(np.diag(cov)), 0.01, 0.99)
    st = O.State(prob, x0)
    st.run(n0, n_threads=2)
    ref = {"x": st.x.copy(), "y": np.asarray(st.y).reshape(W, K, d).copy(),
           "logpost": st.logpost.copy(), "logprior": st.logprior.copy(), "loglike": st.loglike.copy(),
           "weight": st.weight.copy(), "prior_rej": st.prior_rej.copy(),
           "burn_left": st.burn_left.copy(), "n_accept": st.n_accept.copy(), "stuck": np.zeros(1, np.int32)}
    st.run(12, n_threads=2)
    huge_ref.run(prob, ref, 12, step0=n0, anchor=False)
    assert np.array_equal(ref["x"].view(np.uint64), st.x.view(np.uint64))
    assert np.array_equal(ref["logpost"].view(np.uint64), st.logpost.view(np.uint64))
    assert np.array_equal(ref["n_accept"], st.n_accept)


def test_sampler_on_oracle_refuses_d_129():
    """The oracle engine has no max_dim(): the sampler's cap stays 128 there, and a d = 129 model
    fails in initialize with the reason -- it never reaches orc_run's 128-element arrays."""
    from cobaya_amd.model import ProblemSpec
    from cobaya_amd.sampler import LoggedError, MCMCHip
    from tests.oracle_engine import OracleEngine

    class OnOracle(MCMCHip):
        _engine_factory = staticmethod(OracleEngine)

    info, _, _ = huge_ref.gaussian_info(129, seed=1)
    with pytest.raises(LoggedError, match="at most 128 parameters"):
        OnOracle({"seed": 1, "n_walkers": 128, "group_size": 64, "max_samples": 1000},
                 ProblemSpec.from_info(info))
