"""Pins oracle/mcmc_oracle.c (flavour b: C restatement on a Philox stream) to the reference:
known answers for the generator, libm for the fixed-order math, golden vectors G4/G5 for the
log-posterior, and a step-by-step replay of reference chains with the reference's own random
draws injected (through oracle/ref_numpy.py, itself pinned to golden G6)."""
import json
import os
import math

import numpy as np
import pytest

from oracle import cbind as O
from oracle import ref_numpy as R
from tests.test_oracle_numpy import PRIORS, replay


def ulp_diff(a, b):
    return abs(a - b) / math.ulp(b) if b != 0 else abs(a - b)


def test_philox_known_answers():
    """Random123 kat_vectors for philox4x32-10."""
    assert O.philox(0, 0, 0, 0, 0, 0) == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    f = 0xFFFFFFFF
    assert O.philox(f, f, f, f, f, f) == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
    assert O.philox(0xA4093822, 0x299F31D0, 0x243F6A88, 0x85A308D3, 0x13198A2E,
                    0x03707344) == [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]


def test_dlog_dexp_sincos_against_libm():
    rng = np.random.default_rng(0)
    xs = np.concatenate([rng.uniform(0, 1, 4000), 10 ** rng.uniform(-300, 300, 2000),
                         [2.0 ** -53, 1 - 2.0 ** -53, 1.0, 0.5, math.sqrt(0.5), 1e-16]])
    assert max(ulp_diff(O.dlog(x), math.log(x)) for x in xs) <= 1.0
    es = np.concatenate([-rng.uniform(0, 40, 4000), -(10 ** rng.uniform(-10, 2.8, 2000)),
                         [0.0, -1e-300, -707.9]])
    assert max(ulp_diff(O.dexp(x), math.exp(x)) for x in es) <= 1.0
    assert O.dexp(-709.0) == 0.0 and O.dexp(-np.inf) == 0.0
    ks = np.concatenate([rng.integers(0, 2 ** 52, 5000), [0, 2 ** 52 - 1, 2 ** 49, 2 ** 51]])
    for k in ks:
        u = (2 * int(k) + 1) * 2.0 ** -53
        s, c = O.sincos2pi(int(k))
        # mpmath-free reference: reduce exactly in integers first
        assert abs(s - math.sin(2 * math.pi * u)) < 5e-16 + 4e-16 * 2 * math.pi * u
        assert abs(c - math.cos(2 * math.pi * u)) < 5e-16 + 4e-16 * 2 * math.pi * u
        assert abs(s * s + c * c - 1) < 5e-16


def test_haar_matches_numpy_restatement():
    class FixedNormals:
        def __init__(self, z):
            self.z = z

        def standard_normal(self, size):
            assert size == len(self.z)
            return self.z.copy()

    rng = np.random.default_rng(1)
    for d in (2, 3, 7, 30, 33, 100):   # d > 32: four interleaved chains per projection
        z = rng.standard_normal((d + 2) * (d - 1) // 2)
        H = O.haar_from_normals(d, z)
        Href = R.haar_so_n(d, FixedNormals(z))
        np.testing.assert_allclose(H, Href, rtol=0, atol=5e-15)
        np.testing.assert_allclose(H @ H.T, np.eye(d), atol=1e-14)
        assert np.linalg.det(H) == pytest.approx(1.0, abs=1e-12)


def test_basis_is_T_times_haar_and_streams_differ():
    d = 5
    cov = np.diag([1.0, 4.0, 0.25, 9.0, 1.0]) + 0.1
    T = O.proposal_transform(cov, 2.4)
    p = O.Problem(d, [0] * d, [0.0] * d, [1.0] * d, T=T, seed=11)
    V = p.basis(3, 7)
    Rm = np.linalg.solve(T, V.T)  # V[c] = T R[:, c]
    np.testing.assert_allclose(Rm @ Rm.T, np.eye(d), atol=1e-12)
    assert np.linalg.det(Rm) == pytest.approx(1.0, abs=1e-10)
    assert not np.allclose(V, p.basis(3, 8)) and not np.allclose(V, p.basis(4, 7))
    np.testing.assert_array_equal(V, p.basis(3, 7))


def test_g4_prior_and_periodic(golden):
    g = golden("g4_prior")
    kinds = g["kinds"]
    a = np.where(kinds == 0, g["bounds"][:, 0], g["loc"])
    b = np.where(kinds == 0, g["bounds"][:, 1], g["scale"])
    p = O.Problem(5, kinds, a, b)
    lp, ll = p.evaluate(g["points"])
    ref = g["logprior"]
    assert np.array_equal(np.isinf(lp), np.isinf(ref))
    m = ~np.isinf(ref)
    np.testing.assert_allclose(lp[m], ref[m], rtol=4e-16)
    assert np.all(ll[m] == 0.0) and np.all(np.isinf(ll[~m]))


def test_g5_loglike(golden):
    g = golden("g5_loglike")
    for tag in ("gm_d2_K1", "gm_d3_K1", "gm_d3_K3", "gm_d4_K2", "gm_d30_K1", "gm_d30_K3",
                "gm_d100_K1"):
        means = g[tag + "_means"]
        K, d = means.shape
        p = O.Problem(d, [0] * d, [0.0] * d, [1.0] * d, means=means, covs=g[tag + "_covs"],
                      weights=g[tag + "_weights"] if K > 1 else None)
        lp, ll, der = p.evaluate(g[tag + "_points"], derived=True)
        np.testing.assert_allclose(ll, g[tag + "_loglike"], rtol=1e-12, atol=1e-11)
        np.testing.assert_allclose(der, g[tag + "_derived"], rtol=1e-9, atol=1e-10)
    for tag in ("gauss_d3_norm1", "gauss_d27_norm1", "gauss_d27_norm0"):
        mean = g[tag + "_mean"]
        d = len(mean)
        p = O.Problem(d, [0] * d, [-10.0] * d, [10.0] * d, means=mean, covs=g[tag + "_cov"],
                      normalized=tag.endswith("1"))
        lp, ll = p.evaluate(g[tag + "_points"])
        np.testing.assert_allclose(ll, g[tag + "_loglike"], rtol=1e-12, atol=1e-11)


@pytest.mark.parametrize("name,learn", [("quick_nolearn", False), ("fixed3_T2", True),
                                        ("d30_covmat", False), ("d4_K2", True)])
def test_injected_replay_of_reference_chains(golden, name, learn):
    """Tier-A link of the C oracle: fed the reference's own draws (direction*r*scale and the
    Exp(1) accept variate, in the reference's consumption order), orc_step_injected reproduces
    the reference chain: identical accept/reject sequence and weights, values to a few ulp,
    across proposal-covariance updates."""
    g = golden("g6_traces")
    chain = replay(g, name, learn, record_draws=True)
    key = lambda k: g[f"{name}__{k}"]  # noqa: E731
    pri = PRIORS[name.split("_")[0]]
    d = len(pri["kinds"])
    T = float(key("temperature"))
    prob = O.Problem(d, pri["kinds"], pri["a"], pri["b"], means=key("means"),
                     covs=key("covs"), weights=key("weights") if len(key("weights")) > 1 else None,
                     temperature=T, max_tries=float(key("max_tries")),
                     T=O.proposal_transform(key("cov0"), 1.0))
    st = O.State(prob, key("x0")[None, :], burn_in=int(key("burn_in")), row_cap=1000)
    assert st.logpost[0] == pytest.approx(float(key("logpost0")), rel=1e-13)
    # proposal updates happen when the reference learned: replay them at the same row counts
    learn_every = int(key("learn_every"))
    learned = list(g[f"{name}__learned_covs"]) if learn else []
    prog_R = list(g[f"{name}__progress_Rminus1"])
    i_check = 0
    for vec, e in chain.draws:
        before = int(st.n_rows[0])
        st.step_injected(vec, e)  # vec already carries r * proposal_scale
        n = int(st.n_rows[0])
        if learn and n != before and n % learn_every == 0 and i_check < len(prog_R):
            # the reference refreshes the proposal when 0 <= R-1 <= 30 here
            if np.isfinite(prog_R[i_check]) and prog_R[i_check] <= 30.0 and learned:
                prob.set_T(O.proposal_transform(learned.pop(0), 1.0))
            i_check += 1
    rows = st.drain()
    data = key("data")
    cols = [str(c) for c in key("columns")]
    assert len(rows) == len(data)
    assert np.array_equal(rows[:, 1], data[:, cols.index("weight")])
    np.testing.assert_allclose(rows[:, 5:], data[:, 2:2 + d], rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(-rows[:, 2] / T, data[:, cols.index("minuslogpost")],
                               rtol=1e-11, atol=1e-11)
    np.testing.assert_allclose(-rows[:, 3], data[:, cols.index("minuslogprior")],
                               rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(-2 * rows[:, 4], data[:, cols.index("chi2")], rtol=1e-11,
                               atol=1e-10)


def _g10_chain(g, name, learn):
    key = lambda k: g[f"{name}__{k}"]  # noqa: E731
    rng = np.random.Generator(np.random.PCG64())
    rng.bit_generator.state = json.loads(str(key("rng_state")))
    prior = R.Prior(kinds=[0] * 5, a=[0.0] * 5, b=[1.0] * 5)
    target = R.GaussianMixtureTarget(g["means"], g["covs"])
    sizes, flat = key("block_sizes"), key("block_params").tolist()
    blocks = [flat[sum(sizes[:i]):sum(sizes[:i + 1])] for i in range(len(sizes))]
    chain = R.BlockedRefChain(
        prior, target, key("cov0"), key("x0"), rng, blocks,
        oversampling=key("oversampling").tolist(), drag_last_slow=int(key("drag_last_slow")),
        drag_interp_steps=int(key("drag_interp_steps")), output_thin=1,
        temperature=float(key("temperature")), proposal_scale=float(key("proposal_scale")),
        burn_in=int(key("burn_in")), max_tries=float(key("max_tries")), learn_proposal=learn,
        learn_every=int(key("learn_every")), learn_Rminus1_max=30.0, record_draws=True)
    for _ in range(int(key("n_steps_raw"))):
        chain.step()
    return chain, blocks


@pytest.mark.parametrize("name", ["over_nothin", "blocks_1d", "drag"])
def test_injected_replay_of_blocked_and_dragging_chains(golden, name):
    """Tier-A link of the C step and dragging cores ((f)1): fed the increments and accept
    variates the reference drew (as restated by BlockedRefChain, itself pinned to golden
    G10), orc_step_injected_delta / orc_drag_injected reproduce the reference chain:
    identical weights, values to a few ulp."""
    g = golden("g10_blocked")
    key = lambda k: g[f"{name}__{k}"]  # noqa: E731
    if name == "over_nothin":  # learning changes the proposal only: draws carry it already
        chain, blocks = _g10_chain(g, name, True)
    else:
        chain, blocks = _g10_chain(g, name, False)
    n_drag = int(key("drag_interp_steps"))
    prob = O.Problem(5, [0] * 5, [0.0] * 5, [1.0] * 5, means=g["means"], covs=g["covs"],
                     max_tries=float(key("max_tries")), blocks=blocks,
                     oversampling=key("oversampling").tolist(),
                     drag_last_slow=int(key("drag_last_slow")), drag_steps=n_drag)
    st = O.State(prob, key("x0")[None, :], burn_in=int(key("burn_in")), row_cap=1000)
    for rec in chain.draws:
        if n_drag:
            fast = np.zeros((n_drag, 5))
            e = np.full(n_drag + 1, np.nan)
            if rec["fast"]:
                fast[:] = np.array(rec["fast"])
                e[1:] = rec["e"]
                e[0] = rec["e0"]
            st.drag_injected(rec["slow"], fast, e)
        else:
            st.step_injected_delta(*rec)
    rows = st.drain()
    data = key("data")
    cols = [str(c) for c in key("columns")]
    assert len(rows) == len(data)
    assert np.array_equal(rows[:, 1], data[:, cols.index("weight")])
    np.testing.assert_allclose(rows[:, 5:], data[:, 2:7], rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(-rows[:, 2], data[:, cols.index("minuslogpost")], rtol=1e-11,
                               atol=1e-11)
    np.testing.assert_allclose(st.x[0], key("final_x"), rtol=1e-12)
    assert int(st.weight[0]) == int(key("final_weight"))


def test_blocked_schedule_and_directions():
    """Every block appears oversample * n_b times per cycle; the k-th use of a block takes
    column k % n_b of its basis k / n_b; each basis is orthonormal, so the n_b directions of
    one basis reproduce T_b T_b^T; directions only move the block and faster parameters."""
    d = 7
    rng = np.random.default_rng(3)
    A = rng.normal(size=(d, d))
    cov = A @ A.T / d + np.eye(d) * 0.1
    blocks = [[5, 0], [3], [1, 6, 2, 4]]
    over = [1, 2, 3]
    T = O.blocked_transform(cov, blocks, 1.0)
    prob = O.Problem(d, [0] * d, [0.0] * d, [1.0] * d, T=T, blocks=blocks, oversampling=over,
                     seed=9)
    L = prob.cycle_length()
    assert L == 2 * 1 + 1 * 2 + 4 * 3
    i_of_j = np.array([i for b in blocks for i in b])
    for cycle in (0, 1, 5):
        blk, bas, col = prob.schedule(3, cycle)
        assert np.bincount(blk, minlength=3).tolist() == [2, 2, 12]
        V, flag = prob.basis_blocked(3, cycle)
        assert flag.tolist() == (blk == 1).astype(int).tolist()
        for b, (jb, n) in enumerate([(0, 2), (2, 1), (3, 4)]):
            for q in range(over[b]):
                sel = [s for s in range(L) if blk[s] == b and bas[s] == q]
                assert sorted(col[sel].tolist()) == list(range(n))
                Vs = V[sel][:, i_of_j]            # sorted order
                assert np.all(Vs[:, :jb] == 0.0)  # slower parameters untouched
                Tb = T[:, jb:jb + n]
                np.testing.assert_allclose(Vs.T @ Vs, Tb @ Tb.T, rtol=1e-11, atol=1e-14)
    b0, _, _ = prob.schedule(3, 0)
    b1, _, _ = prob.schedule(3, 1)
    b2, _, _ = prob.schedule(4, 0)
    assert not np.array_equal(b0, b1) and not np.array_equal(b0, b2)


def test_radial_law_of_the_philox_stream():
    """G3: P(exponential branch) = 0.33, and the mixture's moments (proposal.py:71-82):
    E r = 0.33*1 + 0.67*sqrt(pi/2), E r^2 = 0.33*2 + 0.67*2."""
    n = 200_000
    r = np.empty(n)
    expo = np.empty(n, bool)
    for i in range(n):
        w = O.philox(5, 6, i, 0, 0, 0)
        kr = (w[1] << 20) | (w[2] >> 12)
        E = -O.dlog((2 * kr + 1) * 2.0 ** -53)
        expo[i] = (w[0] >> 8) < 5536481
        r[i] = E if expo[i] else math.sqrt(2 * E)
    assert abs(expo.mean() - 0.33) < 4 * math.sqrt(0.33 * 0.67 / n)
    assert r.mean() == pytest.approx(0.33 + 0.67 * math.sqrt(math.pi / 2), abs=0.01)
    assert (r ** 2).mean() == pytest.approx(2.0, abs=0.03)


def test_ensemble_recovers_gaussian_target():
    """Tier C on the CPU: posterior mean/cov of the d=3 target of tests/common_sampler.py and
    KL(truth || sample) <= 0.07, the reference's own bar (common_sampler.py:18,152-161)."""
    mean = np.array([-0.48591462, 0.10064559, 0.64406749])
    cov = np.array([[0.00078333, 0.00033134, -0.0002923],
                    [0.00033134, 0.00218118, -0.00170728],
                    [-0.0002923, -0.00170728, 0.00676922]])
    d, W = 3, 1024
    prob = O.Problem(d, [0] * d, [-1.0] * d, [1.0] * d, means=mean, covs=cov,
                     T=O.proposal_transform(cov, 2.4), seed=42)
    rng = np.random.default_rng(0)
    x0 = mean + rng.standard_normal((W, d)) * np.sqrt(np.diag(cov))
    st = O.State(prob, x0)
    st.run(300, n_threads=4)
    gs, S, n = None, None, 0
    for _ in range(60):
        st.run(3 * d, n_threads=4)
        gs, S = O.moments(st.x, 64, group_sum=gs, pooled=S)
        n += W
    m = gs.sum(0) / n
    c = S / n - np.outer(m, m)
    acc = st.n_accept.sum() / (W * st.step)
    assert 0.15 < acc < 0.5
    assert np.all(np.abs(m - mean) < 4 * np.sqrt(np.diag(cov) / (n / 10)))
    kl = 0.5 * (np.trace(np.linalg.solve(c, cov)) + (m - mean) @ np.linalg.solve(c, m - mean)
                - d + np.linalg.slogdet(c)[1] - np.linalg.slogdet(cov)[1])
    assert kl < 0.07 and kl < 0.005
    np.testing.assert_allclose(c, cov, rtol=0.08, atol=2e-5)


def test_moments_fixed_order_matches_numpy():
    rng = np.random.default_rng(2)
    x = rng.normal(size=(256, 5))
    shift = x.mean(0)
    gs, S = O.moments(x, 64, shift=shift)
    xc = x - shift
    np.testing.assert_allclose(gs, xc.reshape(4, 64, 5).sum(1), rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(S, xc.T @ xc, rtol=1e-13)
    gs2, S2 = O.moments(x, 64, shift=shift, group_sum=gs.copy(), pooled=S.copy())
    np.testing.assert_allclose(S2, 2 * S, rtol=1e-15)


# ------------------------------------------------------------------ incremental evaluation
def _inc_pair(d, W, gs, seed, golden, normal=False):
    from oracle import cbind as O
    t = golden("targets")
    if f"mean_d{d}" in t.files:
        mean, cov = t[f"mean_d{d}"], t[f"cov_d{d}"]
    else:
        rng = np.random.default_rng(d)
        A = rng.normal(size=(d, d))
        cov = (A @ A.T / d + np.eye(d)) * 0.002
        mean = np.full(d, 0.5)
    kinds = [0] * d
    a, b = [0.0] * d, [1.0] * d
    if normal:
        for i in range(0, d, 3):
            kinds[i], a[i], b[i] = 1, 0.5, 0.3
    T = O.proposal_transform(cov, 2.4)
    mk = lambda inc: O.Problem(d, kinds, a, b, means=mean, covs=cov, T=T, group_size=gs,
                               seed=seed, incremental=inc, paired_variates=False)
    rng = np.random.default_rng(seed)
    x0 = np.clip(rng.multivariate_normal(mean, cov, size=W), 1e-6, 1 - 1e-6)
    return mk(False), mk(True), x0, mean, cov


@pytest.mark.parametrize("d,normal", [(2, False), (7, True), (30, False), (45, True), (100, False)])
def test_incremental_evaluation_is_the_same_posterior(golden, d, normal):
    """Incremental mode carries y = L^-1 (x - mu) and moves it along the whitened direction.
    Its log-posterior of the CURRENT point must be the from-scratch one of the same x
    (eval_point: what golden G5 pins to the reference) to rounding at every step -- drift is
    bounded by the refresh every 40 d steps -- and y must stay L^-1 (x - mu)."""
    from oracle import cbind as O
    full, inc, x0, mean, cov = _inc_pair(d, 128, 64, 11, golden, normal)
    st = O.State(inc, x0)
    worst = 0.0
    # (d = 100 is BASELINE config 4, the golden target: fewer, longer launches there)
    for _ in range(12 if d < 100 else 4):
        st.run(17 * d + 3, n_threads=4)      # launches end anywhere, refreshes fall inside
        lp, ll = full.evaluate(st.x)
        np.testing.assert_allclose(st.logprior, lp, rtol=1e-13, atol=1e-13)
        np.testing.assert_allclose(st.loglike, ll, rtol=2e-13, atol=1e-11)
        np.testing.assert_allclose(st.logpost, lp + ll, rtol=2e-13, atol=1e-11)
        y = full.whiten(st.x)
        worst = max(worst, np.max(np.abs(st.y - y)))
        np.testing.assert_allclose(st.y, y, rtol=0, atol=1e-11)
    assert st.step % (17 * d + 3) == 0 and 0.05 < st.n_accept.sum() / (128 * st.step) < 0.7
    assert worst > 0.0   # it IS a different arithmetic (else this test would be vacuous)


@pytest.mark.parametrize("d,steps", [(30, 400), (100, 250)])
def test_incremental_and_full_evaluation_walk_the_same_chains(golden, d, steps):
    """Same seed, same proposal stream: the two modes differ by rounding in the trial
    log-posterior only, so over a short run every accept decision coincides and the states
    agree to rounding; statistically they are the same sampler.  (d = 30 and d = 100: the two
    BASELINE dimensions.)"""
    from oracle import cbind as O
    full, inc, x0, mean, cov = _inc_pair(d, 256, 64, 3, golden)
    a, b = O.State(full, x0), O.State(inc, x0)
    a.run(steps, n_threads=4)
    b.run(steps, n_threads=4)
    assert np.array_equal(a.weight, b.weight) and np.array_equal(a.n_accept, b.n_accept)
    np.testing.assert_allclose(a.x, b.x, rtol=0, atol=1e-12)
    np.testing.assert_allclose(a.logpost, b.logpost, rtol=1e-12, atol=1e-10)


def test_whitened_directions_are_linv_times_v(golden):
    from oracle import cbind as O
    full, inc, x0, mean, cov = _inc_pair(30, 64, 64, 5, golden)
    V = inc.basis(3, 7)
    U = inc.whiten_directions(V)
    Linv = np.linalg.inv(np.linalg.cholesky(cov))
    np.testing.assert_allclose(U, V @ Linv.T, rtol=1e-11, atol=1e-12 * np.abs(U).max())


@pytest.mark.parametrize("carry", [False, True])
@pytest.mark.parametrize("d,K", [(4, 3), (30, 2), (9, 4), (30, 8)])
def test_incremental_mixture_is_the_same_posterior(d, K, carry):
    """K > 1 in incremental mode: one carried residual y_k and one whitened direction u_k per
    mode, log-sum-exp as in eval_point (gaussian_mixture.py:158-163).  carry (round 5): the
    log-density a_k of every mode is carried as well (step_inc_mix_kernel): it stays within
    rounding of the evaluated one between refreshes and is re-anchored where y is."""
    from oracle import cbind as O
    rng = np.random.default_rng(40 + d)
    means = rng.uniform(0.4, 0.6, size=(K, d))
    covs = []
    for _ in range(K):
        A = rng.normal(size=(d, d))
        covs.append((A @ A.T / d + np.eye(d)) * 0.003)
    covs = np.array(covs)
    w = rng.uniform(0.5, 1.5, K)
    w /= w.sum()
    T = O.proposal_transform(covs[0], 2.4)
    mk = lambda inc: O.Problem(d, [0] * d, [0.0] * d, [1.0] * d, means=means, covs=covs,
                               weights=w, T=T, group_size=64, seed=9, incremental=inc,
                               paired_variates=False, carry_modes=carry and inc)
    full, inc = mk(False), mk(True)
    assert inc.c.carry_modes == int(carry)
    x0 = np.clip(means[0] + rng.normal(size=(128, d)) * 0.03, 1e-6, 1 - 1e-6)
    a, b = O.State(full, x0), O.State(inc, x0)
    assert b.y.shape == (128, K * d)
    for _ in range(6):
        b.run(23 * d + 1, n_threads=4)
        lp, ll = full.evaluate(b.x)
        np.testing.assert_allclose(b.loglike, ll, rtol=2e-13, atol=1e-11)
        np.testing.assert_allclose(b.y, full.whiten(b.x), rtol=0, atol=1e-11)
        if carry:   # the carried a_k against -(c_k + |y_k|^2) / 2 of the carried residuals
            yk = b.y.reshape(128, K, d)
            np.testing.assert_allclose(b.amode, -0.5 * (inc.cnorm + (yk ** 2).sum(2)),
                                       rtol=2e-13, atol=1e-11)
    if carry:
        # exactly re-anchored where y is refreshed: one step past a refresh the carried values
        # of the walkers that did not move are the anchored ones
        b2 = O.State(inc, x0)
        b2.run(inc.refresh_every, n_threads=4)
        before = b2.n_accept.copy()
        b2.run(1, n_threads=4)
        still = b2.n_accept == before
        yk = b2.y.reshape(128, K, d)[still]
        q = np.zeros((still.sum(), K, 4))
        for i in range(d):
            q[:, :, i & 3] = np.fma(yk[:, :, i], yk[:, :, i], q[:, :, i & 3]) if hasattr(np, "fma") \
                else q[:, :, i & 3] + yk[:, :, i] ** 2
        if hasattr(np, "fma"):
            chi2 = (q[..., 0] + q[..., 1]) + (q[..., 2] + q[..., 3])
            assert np.array_equal(b2.amode[still], -0.5 * (inc.cnorm + chi2))
        assert still.sum() > 40
    a.run(300, n_threads=4)
    c = O.State(inc, x0)
    c.run(300, n_threads=4)
    assert np.array_equal(a.weight, c.weight) and np.array_equal(a.n_accept, c.n_accept)
    np.testing.assert_allclose(a.x, c.x, rtol=0, atol=1e-12)


def test_incremental_with_blocks_is_the_same_posterior():
    """Blocks and oversampling in incremental mode: same accept decisions as the from-scratch
    evaluation of the same blocked proposal stream."""
    from oracle import cbind as O
    d = 9
    rng = np.random.default_rng(3)
    A = rng.normal(size=(d, d))
    cov = (A @ A.T / d + np.eye(d)) * 0.003
    mean = np.full(d, 0.5)
    blocks, over = [[0, 1, 2, 3], [4, 5, 6, 7, 8]], [1, 3]
    T = O.blocked_transform(cov, blocks, 2.4)
    mk = lambda inc: O.Problem(d, [0] * d, [0.0] * d, [1.0] * d, means=mean, covs=cov, T=T,
                               group_size=64, seed=2, blocks=blocks, oversampling=over,
                               incremental=inc, paired_variates=False)
    full, inc = mk(False), mk(True)
    assert inc.refresh_every == 40 * 19
    x0 = np.clip(mean + rng.normal(size=(128, d)) * 0.03, 1e-6, 1 - 1e-6)
    a, b = O.State(full, x0), O.State(inc, x0)
    a.run(900, n_threads=4)
    b.run(900, n_threads=4)
    assert np.array_equal(a.weight, b.weight) and np.array_equal(a.n_accept, b.n_accept)
    np.testing.assert_allclose(a.x, b.x, rtol=0, atol=1e-12)
    np.testing.assert_allclose(b.y, full.whiten(b.x), rtol=0, atol=1e-11)


@pytest.mark.parametrize("K", [1, 2])
def test_incremental_with_one_parameter_blocks_is_the_same_sampler(K):
    """Columns of a one-parameter block draw the RandProposer1D variates (proposal.py:85-93) in
    incremental mode too: with un-paired variates the incremental and the from-scratch run take
    the same decisions; with paired ones the 1-D columns still use the un-paired stream.  One
    Gaussian mode and a mixture of two."""
    from oracle import cbind as O
    d = 7
    rng = np.random.default_rng(5)
    A = rng.normal(size=(d, d))
    cov = (A @ A.T / d + np.eye(d)) * 0.003
    mean = np.full(d, 0.5)
    blocks, over = [[3], [0, 1, 2], [4, 5, 6]], [1, 1, 3]
    T = O.blocked_transform(cov, blocks, 2.4)
    tgt = (dict(means=mean, covs=cov) if K == 1 else
           dict(means=[mean, mean + 0.04], covs=[cov, 1.5 * cov], weights=[0.4, 0.6]))
    mk = lambda inc, paired: O.Problem(d, [0] * d, [0.0] * d, [1.0] * d, **tgt,
                                       T=T, group_size=64, seed=4, blocks=blocks,
                                       oversampling=over, incremental=inc, paired_variates=paired)
    full, inc = mk(False, False), mk(True, False)
    x0 = np.clip(mean + rng.normal(size=(128, d)) * 0.03, 1e-6, 1 - 1e-6)
    a, b = O.State(full, x0), O.State(inc, x0)
    a.run(700, n_threads=4)
    b.run(700, n_threads=4)
    assert np.array_equal(a.weight, b.weight) and np.array_equal(a.n_accept, b.n_accept)
    np.testing.assert_allclose(a.x, b.x, rtol=0, atol=1e-12)
    # paired: a run restricted to the steps of 1-D columns moves only parameter 3, by the same
    # amounts as the full run does on those steps when both start from the same points
    pair = mk(True, True)
    c = O.State(pair, x0)
    c.run(700, n_threads=4)
    lp, ll = full.evaluate(c.x)
    np.testing.assert_allclose(c.logpost, lp + ll, rtol=2e-13, atol=1e-11)
    assert 0.05 < c.n_accept.sum() / (128 * 700) < 0.8


def test_incremental_dragging_is_the_same_sampler():
    """Dragging (mcmc.py:564-668) in incremental mode: the whitened residuals of the start and
    end points are carried through the interpolation steps -- same accept decisions as
    drag_core evaluating every point from scratch, y stays L^-1 (x - mu)."""
    from oracle import cbind as O
    d = 9
    rng = np.random.default_rng(8)
    A = rng.normal(size=(d, d))
    cov = (A @ A.T / d + np.eye(d)) * 0.003
    mean = np.full(d, 0.5)
    blocks, over = [[0, 1, 2], [3, 4, 5, 6, 7, 8]], [1, 3]
    kinds = [0] * d
    kinds[4] = 1
    a_, b_ = [0.0] * d, [1.0] * d
    a_[4], b_[4] = 0.5, 0.2
    T = O.blocked_transform(cov, blocks, 2.4)
    mk = lambda inc: O.Problem(d, kinds, a_, b_, means=mean, covs=cov, T=T, group_size=64, seed=4,
                               blocks=blocks, oversampling=over, drag_last_slow=0, drag_steps=5,
                               incremental=inc)
    full, inc = mk(False), mk(True)
    assert inc.refresh_every == 40 * 3
    x0 = np.clip(mean + rng.normal(size=(128, d)) * 0.03, 1e-6, 1 - 1e-6)
    a, b = O.State(full, x0), O.State(inc, x0)
    for n in (50, 131, 200):
        a.run(n, n_threads=4)
        b.run(n, n_threads=4)
        assert np.array_equal(a.weight, b.weight) and np.array_equal(a.n_accept, b.n_accept)
        np.testing.assert_allclose(a.x, b.x, rtol=0, atol=1e-12)
        np.testing.assert_allclose(a.logpost, b.logpost, rtol=1e-12, atol=1e-10)
        np.testing.assert_allclose(b.y, full.whiten(b.x), rtol=0, atol=1e-11)
    assert 0.05 < a.n_accept.sum() / (128 * 381) < 0.9


def test_paired_variates_have_the_specified_law():
    """Incremental kernels draw the variates of two steps from one Philox block
    (walker_variates_pair): |r| is Exp(1) with probability 676/2048 and chi(2) otherwise, its
    sign is fair, E_a is Exp(1); and a chain on that stream samples the same posterior."""
    from oracle import cbind as O
    d = 6
    rng = np.random.default_rng(1)
    A = rng.normal(size=(d, d))
    cov = (A @ A.T / d + np.eye(d)) * 0.004
    mean = np.full(d, 0.5)
    p = O.Problem(d, [0] * d, [0.0] * d, [1.0] * d, means=mean, covs=cov,
                  T=O.proposal_transform(cov, 2.4), group_size=64, seed=12, incremental=True)
    assert p.paired_variates
    st = O.State(p, np.tile(mean, (4096, 1)))
    xs = []
    for _ in range(60):
        st.run(4 * d, n_threads=8)
        xs.append(st.x.copy())
    x = np.vstack(xs[10:])
    sig = np.sqrt(np.diag(cov))
    assert np.max(np.abs(x.mean(0) - mean) / sig) < 0.02
    assert np.max(np.abs(np.cov(x.T) - cov) / np.outer(sig, sig)) < 0.03
    acc = st.n_accept.sum() / (4096 * st.step)
    assert 0.2 < acc < 0.45


def test_short_argument_logarithm_and_its_table():
    """The logarithm of the paired variates (orc_neg_log_short): within 4e-16 max(1, t) of libm on
    20 000 sampled arguments and the edges of its domain (odd n < 2^b, b = 25 and 29) -- the whole
    domain is swept in tests/test_math_domains_host.py (the oracle against an 80-bit logarithm) and
    tests/test_gpu_math_domains.py (the device against the oracle); the table the kernels and the
    oracle compile is the one tools/make_short_log_table.py writes (one file, two places)."""
    import importlib.util
    import math
    from oracle import cbind as O
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    a = open(os.path.join(root, "oracle", "short_log_table.h")).read()
    b = open(os.path.join(root, "cobaya_amd", "csrc", "short_log_table.h")).read()
    assert a == b
    spec = importlib.util.spec_from_file_location(
        "make_short_log_table", os.path.join(root, "tools", "make_short_log_table.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    rows = gen.table()
    for j, (rc, lrc) in enumerate(rows):
        assert "{ %s, %s }" % (rc.hex(), lrc.hex()) in a
        assert rc == float(np.float32(rc))                       # 24 significant bits
        c = 0.5 + (j + 0.5) / 256
        assert abs(rc * c - 1) < 2.0 ** -23 and abs(lrc - math.log(rc)) <= 2.3e-16 * lrc
    rng = np.random.default_rng(0)
    for nb in (25, 29):
        ks = np.concatenate([rng.integers(0, 2 ** (nb - 1), 20000),
                             [0, 1, 2, 3, 2 ** (nb - 1) - 1, 2 ** (nb - 1) - 2, 2 ** (nb - 2),
                              2 ** (nb - 2) - 1]])
        for k in ks:
            n = 2 * int(k) + 1
            v, t = O.neg_log_short(n, nb), -math.log(n * 2.0 ** -nb)
            assert abs(v - t) <= 4e-16 * max(1.0, t), (n, nb, v, t)


def test_short_variates_lowest_bin_is_redrawn_at_full_width():
    """the 24-bit radial and the 28-bit accept uniform of the paired stream stand,
    in their lowest bin, for u in (0, 2^-b): that bin is redrawn at full width from a Philox
    block of its own, -log u = b ln 2 - log u' -- the variates there exceed the old cut-offs
    (17.3 / 20.1) and are b ln 2 + an Exp(1) variate."""
    import math
    for which, b in ((0, 24), (1, 28)):
        hits = []
        g0 = 0
        while len(hits) < (6 if which == 0 else 2):
            h = O.find_short_tail(11, g0, 1 << 16, 0, 2048, which)
            assert h is not None
            hits.append(h)
            g0 = h[0] + 1 if h[0] + 1 < (1 << 30) else 0
            if g0 % (1 << 16):      # continue behind the hit, then the next block of walkers
                g0 = ((h[0] >> 16) + 1) << 16
        for gid, step in hits:
            r, Ea = O.pair_variates(11, gid, step)
            v = abs(r) if which == 0 else Ea
            if which == 0 and v * v / 2.0 > b * math.log(2.0) - 1e-9 and v < b * math.log(2.0):
                v = v * v / 2.0          # the chi(2) branch: |r| = sqrt(2 E)
            assert v > b * math.log(2.0), (which, gid, step, v)
            assert v - b * math.log(2.0) < 40.0


def test_paired_variates_follow_the_reference_laws():
    """r and E_a of the paired stream, drawn directly: E_a is Exp(1); |r| is Exp(1) with
    probability 676/2048 and chi(2) otherwise (proposal.py:71-82 for n >= 2); the sign is fair
    and independent; r and E_a are uncorrelated; the two halves of a block differ."""
    from scipy import stats
    from oracle import cbind as O
    n = 40000
    v = np.array([O.pair_variates(77, 3 + (i % 7), i) for i in range(n)])
    r, ea = v[:, 0], v[:, 1]
    assert stats.kstest(ea, "expon").pvalue > 1e-3
    p = 676 / 2048
    cdf = lambda t: p * (1 - np.exp(-t)) + (1 - p) * (1 - np.exp(-0.5 * t * t))
    assert stats.kstest(np.abs(r), cdf).pvalue > 1e-3
    assert abs(np.mean(r > 0) - 0.5) < 4 * 0.5 / np.sqrt(n)
    assert abs(np.corrcoef(np.abs(r), ea)[0, 1]) < 0.02
    assert abs(np.corrcoef(r[0::2], r[1::2])[0, 1]) < 0.02
    assert abs(np.corrcoef(ea[0::2], ea[1::2])[0, 1]) < 0.02


@pytest.mark.parametrize("blocked", [False, True])
def test_incremental_with_periodic_parameters_is_the_same_sampler(blocked, carry=False):
    """Periodic parameters (prior.py:675) in incremental mode: the coordinate is the wrapped one,
    and a wrap that changes the winding number moves the carried residual by the wrap times a
    column of L^-1.  With un-paired variates the incremental and the from-scratch run take the
    same decisions, the wrapped coordinates agree, and the carried residual stays L^-1 (x - mu)
    to rounding -- on a target that straddles the boundary, so that walkers wrap all the time."""
    from oracle import cbind as O
    d = 6
    rng = np.random.default_rng(8)
    A = rng.normal(size=(d, d))
    cov = (A @ A.T / d + np.eye(d)) * 0.004
    mean = np.array([0.02, 0.5, 0.97, 0.5, 0.4, 0.6])     # parameters 0 and 2 sit at the seam
    periodic = [1, 0, 1, 0, 0, 1]
    kw = {}
    if blocked:
        blocks, over = [[2], [0, 1, 3], [4, 5]], [1, 1, 2]
        kw = dict(T=O.blocked_transform(cov, blocks, 2.4), blocks=blocks, oversampling=over)
    else:
        kw = dict(T=O.proposal_transform(cov, 2.4))
    mk = lambda inc, paired: O.Problem(d, [0] * d, [0.0] * d, [1.0] * d, periodic=periodic,
                                       means=mean, covs=cov, group_size=64, seed=9,
                                       incremental=inc, paired_variates=paired,
                                       carry_periodic=carry and inc, **kw)
    full, inc = mk(False, False), mk(True, False)
    assert inc.c.carry_periodic == int(carry)
    x0 = (mean + rng.normal(size=(128, d)) * 0.05) % 1.0
    a, b = O.State(full, x0), O.State(inc, x0)
    wraps = 0
    for _ in range(6):
        xa = a.x.copy()
        a.run(150, n_threads=4)
        b.run(150, n_threads=4)
        wraps += int(np.sum(np.abs(a.x - xa)[:, [0, 2, 5]] > 0.5))
        assert np.array_equal(a.weight, b.weight) and np.array_equal(a.n_accept, b.n_accept)
        np.testing.assert_allclose(a.x, b.x, rtol=0, atol=1e-12)
        Linv = np.linalg.inv(np.linalg.cholesky(cov))
        np.testing.assert_allclose(b.y.reshape(128, d), (b.x - mean) @ Linv.T, rtol=0, atol=1e-9)
    assert wraps > 50          # the seam was crossed for real
    assert np.all((b.x >= 0) & (b.x <= 1))
    # paired variates (what the kernels draw): still the posterior's log-density at the points
    c = O.State(mk(True, True), x0)
    c.run(900, n_threads=4)
    lp, ll = full.evaluate(c.x)
    np.testing.assert_allclose(c.logpost, lp + ll, rtol=2e-13, atol=1e-9)


@pytest.mark.parametrize("blocked", [False, True])
def test_incremental_periodic_with_the_carried_loglikelihood(blocked):
    """Round 5 (step_inc_kernel<.., periodic>): a periodic coordinate is wrapped only where the trial
    leaves [lo, hi) and the log-likelihood is carried, re-summed from the moved residual at a step
    that wraps -- still the same sampler as the from-scratch run on a target at the seam (same
    decisions, coordinates to rounding: inside the interval the from-scratch run passes x through
    ((x - a) / (b - a)) % 1 * (b - a) + a, prior.py:675, which returns x up to its own rounding)."""
    test_incremental_with_periodic_parameters_is_the_same_sampler(blocked, carry=True)


@pytest.mark.parametrize("seed", list(range(8)))
def test_incremental_periodic_random_shapes_walk_the_same_chains(seed):
    """Random shapes of the periodic branch of step_core_inc (dimension, which parameters are
    periodic and on which interval, normal priors on others, temperature, parameter blocks with a
    one-parameter block): with un-paired variates the incremental and the from-scratch oracle
    take the same decisions and keep the same wrapped coordinates, and the carried residual
    stays L^-1 (x - mu)."""
    from oracle import cbind as O
    rng = np.random.default_rng(4400 + seed)
    d = int(rng.integers(2, 14))
    A = rng.normal(size=(d, d))
    sd = rng.uniform(0.02, 0.06, d)
    c = A @ A.T / d + np.eye(d)
    cov = c / np.sqrt(np.outer(np.diag(c), np.diag(c))) * np.outer(sd, sd)
    mean = rng.uniform(0.4, 0.6, d)
    periodic = (rng.random(d) < 0.4).astype(int)
    periodic[int(rng.integers(0, d))] = 1
    kinds = [int(not p and rng.random() < 0.3) for p in periodic]
    half = rng.uniform(1.0, 3.0, d) * sd                     # periodic: a few sigma wide
    a = [float(mean[i] - half[i]) if periodic[i] else (0.5 if kinds[i] else -0.5) for i in range(d)]
    b = [float(mean[i] + half[i]) if periodic[i] else (float(rng.uniform(0.2, 0.5)) if kinds[i] else 1.5)
         for i in range(d)]
    T = float(rng.choice([1.0, 1.0, 1.8]))
    kw = {}
    if d >= 4 and rng.random() < 0.5:
        perm = rng.permutation(d).tolist()
        blocks, over = [perm[:1], perm[1:d // 2 + 1], perm[d // 2 + 1:]], [1, 2, 3]
        blocks = [bl for bl in blocks if bl]
        over = over[:len(blocks)]
        kw = dict(T=O.blocked_transform(cov * T, blocks, 2.4), blocks=blocks, oversampling=over)
    else:
        kw = dict(T=O.proposal_transform(cov * T, 2.4))
    mk = lambda inc: O.Problem(d, kinds, a, b, periodic=periodic.tolist(), means=mean, covs=cov,
                               group_size=64, seed=seed + 1, temperature=T, incremental=inc,
                               paired_variates=False, **kw)
    full, inc = mk(False), mk(True)
    x0 = mean + rng.normal(size=(64, d)) * sd
    for i in range(d):
        if periodic[i]:
            x0[:, i] = a[i] + (x0[:, i] - a[i]) % (b[i] - a[i])
    sa, sb = O.State(full, x0), O.State(inc, x0)
    Linv = np.linalg.inv(np.linalg.cholesky(cov))
    moved = 0
    for n in (1, 37, 400, 163):
        before = sa.x.copy()
        sa.run(n, n_threads=2)
        sb.run(n, n_threads=2)
        assert np.array_equal(sa.weight, sb.weight) and np.array_equal(sa.n_accept, sb.n_accept)
        np.testing.assert_allclose(sa.x, sb.x, rtol=0, atol=1e-12)
        np.testing.assert_allclose(sb.y.reshape(64, d), (sb.x - mean) @ Linv.T, rtol=0, atol=1e-9)
        per = np.flatnonzero(periodic)
        moved += int(np.sum(np.abs(sa.x - before)[:, per] > 0.8 * (np.array(b) - np.array(a))[per]))
        assert np.all(sb.x[:, per] >= np.array(a)[per]) and np.all(sb.x[:, per] <= np.array(b)[per])
    assert sa.n_accept.sum() > 64 * 20


@pytest.mark.parametrize("d,K,n_per", [(5, 6, 0), (12, 16, 0), (72, 2, 0), (9, 3, 2), (30, 5, 3),
                                       (20, 1, 12)])
def test_incremental_general_shapes_walk_the_same_chains(d, K, n_per):
    """What the general incremental kernel serves (step_inc_any_kernel): more than four modes, a
    mixture above d = 64, periodic parameters together with a mixture, more than eight periodic
    parameters -- the oracle's step_core_inc against its from-scratch step on the same
    (un-paired) proposal stream: same decisions, same wrapped coordinates, and every carried
    residual stays L_k^-1 (x - mu_k)."""
    from oracle import cbind as O
    rng = np.random.default_rng(5200 + 10 * d + K)
    sd = rng.uniform(0.02, 0.05, d)
    means = 0.5 + rng.normal(size=(K, d)) * sd * 0.7
    covs = []
    for _ in range(K):
        A = rng.normal(size=(d, d))
        c = A @ A.T / d + np.eye(d)
        covs.append(c / np.sqrt(np.outer(np.diag(c), np.diag(c))) * np.outer(sd, sd) * rng.uniform(0.7, 1.4))
    covs = np.array(covs)
    w = rng.uniform(0.5, 1.5, K)
    w /= w.sum()
    periodic = np.zeros(d, dtype=int)
    periodic[rng.choice(d, n_per, replace=False)] = 1
    half = rng.uniform(1.0, 2.0, d) * sd                     # periodic: a few sigma wide
    a = [float(0.5 - half[i]) if periodic[i] else -0.5 for i in range(d)]
    b = [float(0.5 + half[i]) if periodic[i] else 1.5 for i in range(d)]
    tgt = dict(means=means, covs=covs, weights=w) if K > 1 else dict(means=means[0], covs=covs[0])
    mk = lambda inc: O.Problem(d, [0] * d, a, b, periodic=periodic.tolist() if n_per else None,
                               T=O.proposal_transform(covs[0], 2.4), group_size=64, seed=11,
                               incremental=inc, paired_variates=False, **tgt)
    full, inc = mk(False), mk(True)
    x0 = means[0] + rng.normal(size=(64, d)) * sd
    per = np.flatnonzero(periodic)
    for i in per:
        x0[:, i] = a[i] + (x0[:, i] - a[i]) % (b[i] - a[i])
    sa, sb = O.State(full, x0), O.State(inc, x0)
    assert sb.y.shape == (64, K * d)
    Linv = [np.linalg.inv(np.linalg.cholesky(c)) for c in covs]
    moved = 0
    for n in (1, 40 * d - 7, 90, 23):      # across the refresh
        before = sa.x.copy()
        sa.run(n, n_threads=4)
        sb.run(n, n_threads=4)
        assert np.array_equal(sa.weight, sb.weight) and np.array_equal(sa.n_accept, sb.n_accept)
        np.testing.assert_allclose(sa.x, sb.x, rtol=0, atol=1e-12)
        np.testing.assert_allclose(sa.logpost, sb.logpost, rtol=1e-12, atol=1e-9)
        y = sb.y.reshape(64, K, d)
        for k in range(K):
            np.testing.assert_allclose(y[:, k], (sb.x - means[k]) @ Linv[k].T, rtol=0, atol=1e-9)
        if n_per:
            moved += int(np.sum(np.abs(sa.x - before)[:, per] > 0.6 * (np.array(b) - np.array(a))[per]))
            assert np.all(sb.x[:, per] >= np.array(a)[per]) and np.all(sb.x[:, per] <= np.array(b)[per])
    assert sa.n_accept.sum() > 64 * 20 and (not n_per or moved > 10), moved


def test_binned_gaussian_oracle_against_reference_golden_g13():
    """§8f-4: the oracle's restatement of planck_pliklite.py:143-155 (orc_binned: binned response,
    triangular whitening, 32 interleaved chains) against the reference's own `get_chi_squared`,
    run on a synthetic plik-lite-shaped data set (golden G13; the Planck data is unavailable)."""
    from cobaya_amd import pliklite as P
    from tests.pliklite_common import load_g13
    g, ds = load_g13()
    t = P.BinnedGaussian.from_dataset(ds)
    # the host mirror of init_params leaves what the reference's leaves (planck_pliklite.py:32-141)
    assert np.array_equal(t.weights, g["ref_weights"]) and np.array_equal(t.X_data, g["ref_X_data"])
    assert np.array_equal(t.used_indices, g["ref_used_indices"])
    assert np.array_equal(t.blmin, g["ref_blmin"]) and np.array_equal(t.blmax, g["ref_blmax"])
    inv = np.linalg.inv(t.cov)
    np.testing.assert_allclose(np.diag(inv), g["ref_invcov_diag"], rtol=1e-10)
    np.testing.assert_allclose(inv[300], g["ref_invcov_row300"], rtol=1e-8, atol=1e-12)
    emu = P.synthetic_emulator(26, ds.lmax)
    B = O.Binned(t.bin_table(), t.weights, t.X_data, cov=t.cov, theta0=emu.theta0, D0=emu.D0,
                 J=emu.J, calib=26)
    x = np.column_stack((g["emu_theta"], g["emu_A"]))
    np.testing.assert_allclose(B.chi2_of_delta(B.delta(x)), g["emu_chi2"], rtol=1e-12)
    cl = np.array([emu.cl(th) for th in g["emu_theta"]])
    assert np.array_equal(cl.sum(axis=2), g["emu_clsum"])
    np.testing.assert_allclose(B.chi2_of_cl(0, cl, g["emu_A"]), g["emu_chi2"], rtol=1e-12)
    raw = g["raw_cl"].astype(np.float64)
    for k in range(len(raw)):
        L0 = int(g["raw_L0"][k])
        np.testing.assert_allclose(B.chi2_of_cl(L0, raw[k:k + 1, :, L0:], g["raw_A"][k:k + 1]),
                                   g["raw_chi2"][k:k + 1], rtol=1e-12)
    for tag, kw in (("tt", dict(use_cl=["tt"])), ("bins", dict(use_bins=list(range(10, 120, 3)))),
                    ("lrange", dict(use_cl=["te", "ee"], bins_for_L_range=[500, 1200]))):
        s = P.BinnedGaussian.from_dataset(ds, **kw)
        assert np.array_equal(s.used_indices, g[f"sel_{tag}_used_indices"])
        Bs = O.Binned(s.bin_table(), s.weights, s.X_data, cov=s.cov, theta0=emu.theta0, D0=emu.D0,
                      J=emu.J, calib=26)
        np.testing.assert_allclose(Bs.chi2_of_delta(Bs.delta(x[:8])), g[f"sel_{tag}_chi2"], rtol=1e-12)
    # the plain numpy statement of the same lines (cobaya_amd.pliklite) agrees too
    np.testing.assert_allclose(t.chi_squared(0, cl[3][0], cl[3][1], cl[3][2], g["emu_A"][3]),
                               g["emu_chi2"][3], rtol=1e-12)


def write_pliklite_files(folder, ds, binary=True, dataset_name="plik_lite_synth.dataset", extra=""):
    """The data set in the reference's own file formats (what planck_pliklite.py:44-73 reads):
    text tables, the covariance as ONE Fortran sequential record written by scipy's FortranFile
    with -1 in the upper triangle (which the reader must drop), and the .dataset file."""
    import os
    from scipy.io import FortranFile
    np.savetxt(os.path.join(folder, "data.txt"), ds.data, fmt="%.17g")
    np.savetxt(os.path.join(folder, "blmin.txt"), ds.blmin, fmt="%d")
    np.savetxt(os.path.join(folder, "blmax.txt"), ds.blmax, fmt="%d")
    np.savetxt(os.path.join(folder, "weights.txt.gz"), ds.weights, fmt="%.17g")
    if binary:
        f = FortranFile(os.path.join(folder, "cov.bin"), "w")
        f.write_record(np.tril(ds.cov) + np.triu(np.full(ds.cov.shape, -1.0), 1))
        f.close()
    else:
        np.savetxt(os.path.join(folder, "cov.txt"), ds.cov, fmt="%.17g")
    path = os.path.join(folder, dataset_name)
    with open(path, "w") as f:
        f.write(f"""# a plik-lite-shaped synthetic data set (the layout of plik_lite_v22.dataset)
use_cl = TT TE EE     # spectra in the data vector
nbintt = {ds.nbintt}
nbinte = {ds.nbinte}
nbinee={ds.nbinee}
lmax = {ds.lmax}
bin_lmin_offset = {ds.bin_lmin_offset}

data = data.txt
blmin = blmin.txt
blmax = blmax.txt
weights = weights.txt.gz
cov_file = cov.txt
cov_file_binary = cov.bin
{extra}""")
    return path


def test_pliklite_files_are_read_like_the_reference_reads_them(tmp_path):
    """VERDICT r3 missing 2: `PlikLiteDataset.from_files` = the input side of
    planck_pliklite.py:44-73 (.dataset keys, loadtxt tables, the Fortran-binary covariance with
    the `tril` symmetrisation).  The files are written here in the reference's formats from the
    G13 arrays; what the reader + `from_dataset` leave equals what the REFERENCE left after
    reading the same contents (golden G13 `ref_*`, and `bin_chi2` = its chi2 with the binary
    covariance), and the options of the .dataset file / `dataset_params` select as there."""
    from cobaya_amd import pliklite as P
    from cobaya_amd.model import ProblemSpec, UnsupportedModel
    from tests.pliklite_common import load_g13
    g, ds0 = load_g13()
    path = write_pliklite_files(str(tmp_path), ds0)
    raw = np.fromfile(tmp_path / "cov.bin", dtype=np.uint8)
    assert len(raw) == 8 + 8 * ds0.nbins ** 2          # one record: marker, payload, marker
    ds = P.PlikLiteDataset.from_files(path)
    assert np.array_equal(ds.cov, ds0.cov) and np.array_equal(ds.data, ds0.data)
    assert ds.options == {"use_cl": ["tt", "te", "ee"], "use_bins": [], "bins_for_L_range": [],
                          "calibration_param": "A_planck"}
    t = P.BinnedGaussian.from_dataset(ds, **ds.options)
    assert np.array_equal(t.weights, g["ref_weights"]) and np.array_equal(t.X_data, g["ref_X_data"])
    assert np.array_equal(t.used_indices, g["ref_used_indices"])
    assert np.array_equal(t.blmin, g["ref_blmin"]) and np.array_equal(t.blmax, g["ref_blmax"])
    emu = P.synthetic_emulator(26, ds.lmax)
    B = O.Binned(t.bin_table(), t.weights, t.X_data, cov=t.cov, theta0=emu.theta0, D0=emu.D0,
                 J=emu.J, calib=26)
    x = np.column_stack((g["emu_theta"], g["emu_A"]))[:8]
    np.testing.assert_allclose(B.chi2_of_delta(B.delta(x)), g["bin_chi2"], rtol=1e-12)
    # without the binary file the text covariance is used (planck_pliklite.py:66-67)
    os.remove(tmp_path / "cov.bin")
    with pytest.raises(OSError):
        P.PlikLiteDataset.from_files(path)
    write_pliklite_files(str(tmp_path), ds0, binary=False)
    assert np.array_equal(P.PlikLiteDataset.from_files(str(tmp_path / "plik_lite_synth")).cov, ds0.cov)
    # through the input: `dataset_file` + `path`, `dataset_params` overriding the file's keys
    # (TT_lite_native.yaml: `dataset_params: {use_cl: tt}`), options of the .dataset file itself
    params = {n: {"prior": {"min": -1, "max": 1}} for n in emu.names}
    params["A_planck"] = {"prior": {"dist": "norm", "loc": 1, "scale": 0.0025}}

    def spec(**like):
        return ProblemSpec.from_info({"likelihood": {"plik": {
            "class": "planck_pliklite", "cl_emulator": emu, **like}}, "params": params})
    full = spec(dataset_file="plik_lite_synth.dataset", path=str(tmp_path))
    assert np.array_equal(full.components[0]["binned"].used_indices, g["ref_used_indices"])
    tt = spec(dataset_file=path, dataset_params={"use_cl": "tt"})
    assert np.array_equal(tt.components[0]["binned"].used_indices, g["sel_tt_used_indices"])
    both = spec(dataset_file=path, use_cl="te ee", dataset_params={"use_cl": "tt", "bins_for_L_range": "500 1200"})
    assert np.array_equal(both.components[0]["binned"].used_indices, g["sel_lrange_used_indices"])
    write_pliklite_files(str(tmp_path), ds0, binary=False, dataset_name="bins.dataset",
                         extra="use_bins = " + " ".join(map(str, range(10, 120, 3))) + "\n")
    sel = spec(dataset_file="bins", path=str(tmp_path))
    assert np.array_equal(sel.components[0]["binned"].used_indices, g["sel_bins_used_indices"])
    with pytest.raises(UnsupportedModel, match="could not be read"):
        spec(dataset_file="nowhere.dataset", path=str(tmp_path))
    with open(tmp_path / "cov.bin", "wb") as f:
        f.write(b"\x10\x00\x00\x00" + b"\x00" * 12)       # a record without its closing marker
    with pytest.raises(ValueError, match="sequential unformatted"):
        P.read_fortran_reals(str(tmp_path / "cov.bin"))


def test_binned_gaussian_steps_sample_the_posterior():
    """The oracle's Metropolis steps on the binned target (small case, 6 parameters): mean and
    covariance of the walkers agree with the Gaussian (Fisher) approximation of the posterior --
    exact in theta for fixed calibration, and the calibration prior is narrow."""
    from cobaya_amd import pliklite as P
    from tests.pliklite_common import sampling_problem, small_dataset
    ds = small_dataset()
    t = P.BinnedGaussian.from_dataset(ds)
    emu = P.synthetic_emulator(5, ds.lmax)
    kinds, a, b, C = sampling_problem(t, emu)
    B = O.Binned(t.bin_table(), t.weights, t.X_data, cov=t.cov, theta0=emu.theta0, D0=emu.D0,
                 J=emu.J, calib=5)
    prob = O.Problem(6, kinds, a, b, T=O.proposal_transform(C, 2.4), group_size=64, seed=11, binned=B)
    rng = np.random.default_rng(5)
    W = 512
    x0 = np.concatenate((emu.theta0, [1.0])) + rng.standard_normal((W, 6)) @ np.linalg.cholesky(C).T
    st = O.State(prob, x0)
    acc = st.run(400, n_threads=O.max_threads())
    assert 0.1 < acc / (W * 400) < 0.6
    # the posterior mean: maximum of the binned chi2 in theta at A = 1 (linear least squares)
    Bm = np.column_stack((B.BJ, -2.0 * B.Bc0))
    F = Bm.T @ np.linalg.solve(t.cov, Bm)
    F[5, 5] += 1.0 / 0.0025 ** 2
    best = np.linalg.solve(F, Bm.T @ np.linalg.solve(t.cov, t.X_data - B.Bc0))
    mean = st.x.mean(axis=0) - np.concatenate((emu.theta0, [1.0]))
    sig = np.sqrt(np.diag(C))
    assert np.all(np.abs(mean - best) < 5 * sig / np.sqrt(W / 8)), (mean - best) / sig
    ratio = st.x.std(axis=0) / sig
    assert np.all((ratio > 0.8) & (ratio < 1.25)), ratio


def test_carried_loglikelihood_follows_the_evaluated_one_and_is_re_anchored():
    """Round 4 (step_inc_kernel, oracle step_core_inc `carry`): with ONE mode and no periodic
    parameter the log-likelihood is carried, ll_t = fma(-r/2, fma(r, |u|^2, 2 y.u), ll), instead of
    being formed from the trial's residual.  (i) |u|^2 is the four-chain sum of squares of the
    whitened direction; (ii) between two refreshes the carried value stays within rounding of the
    log-likelihood evaluated from scratch at the same point; (iii) where y is refreshed from x
    (every 40 cycles) it is re-anchored: -chi2(y)/2 in the four-chain pattern, logpost = logprior +
    loglike, exactly; (iv) a mixture keeps the two-chain form (no anchor: its state is untouched
    by a refresh)."""
    from oracle import cbind as O
    d = 11
    rng = np.random.default_rng(17)
    A = rng.normal(size=(d, d))
    cov = (A @ A.T / d + np.eye(d)) * 0.002
    mean = np.full(d, 0.5)
    T = O.proposal_transform(cov, 2.4)
    p = O.Problem(d, [0] * d, [0.0] * d, [1.0] * d, means=mean, covs=cov, T=T, group_size=64,
                  seed=6, incremental=True)
    assert p.refresh_every == 40 * d
    # (i)
    V = p.basis(3, 5)
    U = p.whiten_directions(V)
    ref = np.array([(u[0::4] ** 2).sum() + (u[1::4] ** 2).sum() + (u[2::4] ** 2).sum()
                    + (u[3::4] ** 2).sum() for u in U])
    np.testing.assert_allclose(p.direction_norms(U), ref, rtol=1e-14)
    x0 = np.clip(mean + rng.normal(size=(128, d)) * 0.03, 1e-6, 1 - 1e-6)
    st = O.State(p, x0)
    # (ii) just before the first refresh after the start: 40 d - 1 carried steps
    st.run(40 * d - 1, n_threads=4)
    lp, ll = p.evaluate(st.x)
    assert st.n_accept.sum() > 128 * 40         # (the walkers did move)
    assert np.max(np.abs(st.loglike - ll)) < 1e-10 and np.max(np.abs(st.loglike - ll)) > 0
    np.testing.assert_allclose(st.logpost, lp + ll, rtol=0, atol=1e-10)
    # (iii) step 40 d is a refresh: take ONE step and undo nothing -- instead predict the anchor
    # for the walkers that reject it (their point is the refreshed one)
    before = st.n_accept.copy()
    st.run(1, n_threads=1)
    stay = st.n_accept == before
    assert stay.sum() > 20
    y = p.whiten(st.x)
    anchored = np.empty(len(y))
    for w in range(len(y)):
        s4 = [0.0, 0.0, 0.0, 0.0]
        for i in range(d):
            s4[i & 3] = float(np.float64(y[w, i]) * np.float64(y[w, i]) + s4[i & 3])   # (no fma: to rounding)
        anchored[w] = -0.5 * (p.cnorm[0] + ((s4[0] + s4[1]) + (s4[2] + s4[3])))
    np.testing.assert_allclose(st.loglike[stay], anchored[stay], rtol=1e-14)
    assert np.array_equal(st.logpost[stay], st.logprior[stay] + st.loglike[stay])
    # (iv)
    pm = O.Problem(d, [0] * d, [0.0] * d, [1.0] * d, means=[mean, mean + 0.03], covs=[cov, cov],
                   weights=[0.5, 0.5], T=T, group_size=64, seed=6, incremental=True)
    sm = O.State(pm, x0)
    ll0 = sm.loglike.copy()
    sm.run(1, n_threads=1)                      # (step 0 is a refresh)
    keep = sm.n_accept == 0
    assert keep.sum() > 20 and np.array_equal(sm.loglike[keep], ll0[keep])


def test_carried_logprior_follows_the_evaluated_one_and_is_re_anchored():
    """Round 5 (step_inc_kernel MODE 2, oracle step_core_inc `carry_p`): with ONE mode, no periodic
    parameter and some NORMAL priors the log-prior is carried along the direction,
    lp_t = fma(-r/2, fma(r, v.w, 2 (x.w - loc.w)), lp) with w_i = (v_i / s_i) / s_i, instead of
    being summed from the trial (prior.py:733-763 is what both evaluate).  (i) between two
    refreshes the carried value stays within rounding of the log-prior evaluated from scratch at
    the same point, also with a location four orders of magnitude above its scale; (ii) at a
    refresh it is re-anchored on x."""
    from oracle import cbind as O
    d = 11
    rng = np.random.default_rng(23)
    A = rng.normal(size=(d, d))
    cov = (A @ A.T / d + np.eye(d)) * 0.002
    mean = np.full(d, 0.5)
    mean[7] = 1000.5
    T = O.proposal_transform(cov, 2.4)
    kinds = [0, 1, 1, 0, 1, 0, 1, 1, 0, 1, 1]
    a = [0.0 if k == 0 else 0.5 for k in kinds]
    b = [1.0 if k == 0 else 0.07 + 0.01 * i for i, k in enumerate(kinds)]
    a[7] = 1000.5
    p = O.Problem(d, kinds, a, b, means=mean, covs=cov, T=T, group_size=64, seed=6,
                  incremental=True)
    x0 = mean + rng.normal(size=(128, d)) * 0.03
    x0[:, [0, 3, 5, 8]] = np.clip(x0[:, [0, 3, 5, 8]], 1e-6, 1 - 1e-6)
    st = O.State(p, x0)
    st.run(40 * d - 1, n_threads=4)
    lp, ll = p.evaluate(st.x)
    assert st.n_accept.sum() > 128 * 40
    err = np.max(np.abs(st.logprior - lp))
    assert 0 < err < 1e-9, err
    np.testing.assert_allclose(st.logpost, lp + ll, rtol=0, atol=2e-9)
    pf = O.Problem(d, kinds, a, b, means=mean, covs=cov, T=T, group_size=64, seed=6,
                   incremental=False)
    st.run(1, n_threads=1)                      # (step 40 d - 1, the last one before the refresh)
    before = st.n_accept.copy()
    st.run(1, n_threads=1)                      # step 40 d: a refresh, then one step
    stay = st.n_accept == before
    assert stay.sum() > 20
    # (ii) re-anchored: the incremental form of the normal terms (reciprocal of the scale), four
    # chains over i mod 4 -- within rounding of eval_point's division form, and logpost exact
    lp1, _ = pf.evaluate(st.x)
    np.testing.assert_allclose(st.logprior[stay], lp1[stay], rtol=1e-14)
    assert np.array_equal(st.logpost[stay], st.logprior[stay] + st.loglike[stay])
    sc = np.zeros((128, 4))
    for i in range(d):
        if kinds[i]:
            q = (st.x[:, i] - a[i]) * (1.0 / b[i])
            sc[:, i & 3] += -0.5 * q * q + p.mls[i]
    anchored = p.uniform_logp + ((sc[:, 0] + sc[:, 1]) + (sc[:, 2] + sc[:, 3]))
    np.testing.assert_allclose(st.logprior[stay], anchored[stay], rtol=1e-15)


@pytest.mark.parametrize("incremental", [True, False])
def test_run_is_invariant_to_the_thread_split(golden, incremental):
    """orc_run cuts a wide basis group (one Haar basis for 1 024 walkers here, 4 096 at the
    benchmark geometry) into runs of >= 64 walkers when there are fewer groups than threads; each
    run forms the group's bases itself.  The result does not depend on the cut (1, 4, 16 threads)
    nor on how the ensemble is handed over (whole, or one group at a time with `walker0`)."""
    from oracle import cbind as O
    d, W, gs = 30, 2048, 1024
    t = golden("targets")
    mean, cov = t["mean_d30"], t["cov_d30"]
    prob = O.Problem(d, [0] * d, [0.0] * d, [1.0] * d, means=mean, covs=cov,
                     T=O.proposal_transform(cov, 2.4), group_size=gs, seed=11,
                     incremental=incremental)
    rng = np.random.default_rng(5)
    x0 = np.clip(rng.multivariate_normal(mean, cov, size=W), 1e-6, 1 - 1e-6)
    runs = []
    for nt in (1, 4, 16):
        st = O.State(prob, x0)
        acc = st.run(2 * d + 7, walker0=3 * gs, n_threads=nt)
        st.run(d, walker0=3 * gs, n_threads=nt)
        runs.append((st, acc))
    a = runs[0][0]
    assert 0.1 < a.n_accept.sum() / (W * a.step) < 0.7
    for st, acc in runs[1:]:
        assert acc == runs[0][1]
        assert np.array_equal(st.x.view(np.uint64), a.x.view(np.uint64))
        assert np.array_equal(st.logpost.view(np.uint64), a.logpost.view(np.uint64))
        assert np.array_equal(st.weight, a.weight) and np.array_equal(st.n_accept, a.n_accept)
        if incremental:
            assert np.array_equal(st.y.view(np.uint64), a.y.view(np.uint64))
    for g in range(2):    # one group at a time
        st = O.State(prob, x0[g * gs:(g + 1) * gs])
        st.run(2 * d + 7, walker0=(3 + g) * gs, n_threads=8)
        st.run(d, walker0=(3 + g) * gs, n_threads=8)
        assert np.array_equal(st.x.view(np.uint64), a.x[g * gs:(g + 1) * gs].view(np.uint64))
        assert np.array_equal(st.weight, a.weight[g * gs:(g + 1) * gs])


def test_table_driven_exp_and_log_of_the_log_sum_exp():
    """Round 5: the incremental mixtures take their log-sum-exp with a table-driven exp and log
    without divisions (orc_dexp_tab / orc_dlog_tab = dexp_tab / dlog_tab of det_math.h; the tables are
    generated with 60-digit decimal arithmetic into the ONE header both sides compile).  Against libm:
    exp within 2 ulp on [-708, 0] (0 below); log within 1 ulp + 3e-16 absolute -- what a sum of
    weighted terms in [w_max, 1] needs (the logarithm of a number next to 1 is tiny and the bar is
    absolute there)."""
    rng = np.random.default_rng(5)
    xs = np.concatenate([-rng.uniform(0, 40, 6000), -(10 ** rng.uniform(-12, 2.85, 4000)),
                         [0.0, -1e-300, -707.9, -0.010830424696249145 / 2, -0.0108304246962491]])
    worst = 0.0
    for x in xs:
        got, ref = O.dexp_tab(x), math.exp(x)
        worst = max(worst, abs(got - ref) / math.ulp(ref))
    assert worst <= 2.0, worst
    assert O.dexp_tab(-709.0) == 0.0 and O.dexp_tab(-np.inf) == 0.0 and O.dexp_tab(0.0) == 1.0
    ys = np.concatenate([rng.uniform(0.01, 1.0, 6000), 10 ** rng.uniform(-300, 300, 3000),
                         1 - 10 ** rng.uniform(-16, -1, 1000), [1.0, 0.5, 0.25, 2.0, 1e-300]])
    for y in ys:
        got, ref = O.dlog_tab(y), math.log(y)
        assert abs(got - ref) <= 3e-16 + math.ulp(ref), (y, got, ref)
    assert abs(O.dlog_tab(1.0)) < 1e-16     # (not exactly 0: the bar near 1 is absolute)
