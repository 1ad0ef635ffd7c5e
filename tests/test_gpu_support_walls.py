"""The prior-support test of every step kernel AT THE WALLS and on off-scale bounds: targets
pressed against their box (tests/support_cases.py: about a third of all trials leave the support;
the conditions on the cases are checked on the oracle alone in tests/test_support_cases_host.py),
on boxes that single precision cannot hold -- narrower than two float ulps, beyond FLT_MAX, below
the float subnormals, entirely negative --, device against oracle BIT FOR BIT across the refresh.
Each kernel answers "inside for certain" with a cheap test of its own and falls back on the exact
comparisons: a cheap test that says "inside" for a trial that has left the box fails here.

And the host linear algebra (L^-1, the log-normalisations) and the evaluator at these scales
against a long-double reference, at a tolerance measured on the numpy recipe's own error."""
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from cobaya_amd import engine as E  # noqa: E402
from cobaya_amd import pliklite as P  # noqa: E402
from oracle import cbind as O  # noqa: E402
from tests import support_cases as S  # noqa: E402
from tests.pliklite_common import sampling_problem, small_dataset  # noqa: E402
from tests.test_gpu_parity import assert_bit_equal  # noqa: E402

SEED = 3


def make_wall_pair(c, cap=0):
    """Engine and oracle of a case on ONE set of constants (the engine's), like make_pair of
    tests/test_gpu_parity.py."""
    kinds, a, b, periodic, blocking, means, covs, x0 = S.case_problem(c)
    scratch = "scratch" in (c.variant or "")
    eng = E.Engine(c.d, c.W, group_size=c.gs, seed=SEED, incremental=not scratch, emit_capacity=cap)
    eng.set_prior(kinds.tolist(), a.tolist(), b.tolist(),
                  None if periodic is None else periodic.tolist())
    eng.set_target_gaussian_mixture(means, covs, None)
    kw = {}
    if blocking is not None:
        blocks, over, last_slow, n_drag = blocking
        eng.set_blocking(blocks, over, last_slow, n_drag)
        kw = dict(blocks=blocks, oversampling=over, drag_last_slow=last_slow, drag_steps=n_drag)
    eng.set_proposal_cov(covs[0])
    prob = O.Problem(c.d, kinds.tolist(), a.tolist(), b.tolist(), periodic=periodic, means=means,
                     covs=covs, T=eng.get_proposal_transform(), group_size=c.gs, seed=SEED,
                     derived=eng.derived_constants(), incremental=not scratch,
                     carry_modes=eng.carries_modes(), carry_periodic=eng.carries_periodic(), **kw)
    eng.set_state(x0)
    st = O.State(prob, x0, row_cap=cap)
    return eng, prob, st, kinds, a, b, periodic


def compare_everything(eng, st, what=""):
    s = eng.get_full_state()
    for k in ("x", "logpost", "logprior", "loglike"):
        assert_bit_equal(s[k], getattr(st, k), f"{what}{k}")
    for k in ("weight", "prior_rej", "n_accept"):
        assert np.array_equal(s[k], getattr(st, k)), f"{what}{k}"
    if eng.incremental:
        assert_bit_equal(s["y"], st.y, f"{what}carried whitened residual")
        if eng.carries_modes() and st.step > 0:
            assert st.p.c.carry_modes == 1
            assert_bit_equal(s["amode"], st.amode, f"{what}carried mode log-densities")
    return s


@pytest.mark.parametrize("c", S.CASES, ids=S.case_id)
def test_steps_at_the_walls_bit_exact(c, monkeypatch):
    if c.variant == "duo":
        monkeypatch.setenv("MCMC_HIP_DUO", "1")
    emit = c.variant == "emit"
    eng, prob, st, kinds, a, b, periodic = make_wall_pair(c, cap=600 if emit else 0)
    L = eng.cycle_length()
    compare_everything(eng, st, "start: ")
    per = [] if periodic is None else np.flatnonzero(periodic).tolist()
    out = wraps = 0
    for n in S.case_launches(c, L):
        before, rej = st.x.copy(), st.prior_rej.copy()
        eng.step(n)
        eng.sync()
        st.run(n, n_threads=8)
        compare_everything(eng, st, f"after {st.step} steps: ")
        out += int(np.sum(st.prior_rej > rej))
        if per:
            wraps += int(np.sum(np.abs(st.x - before)[:, per] > 0.08))
        if emit:
            rows, ref = eng.drain_samples(), st.drain()
            assert rows.shape == ref.shape
            assert_bit_equal(rows, ref, "emitted rows")
    kernel = eng.last_step_kernel()
    print(f"{S.case_id(c)}: {kernel}; {st.step} steps, acceptance "
          f"{st.n_accept.sum() / (c.W * st.step):.3f}, walkers rejected outside the support in {out} launches x walkers")
    counters = eng.counters()
    assert counters["steps"] == st.step and counters["accepted"] == int(st.n_accept.sum())
    assert counters["dropped_rows"] == 0
    x = eng.get_full_state()["x"]
    uni = kinds == 0
    assert np.all((x[:, uni] >= a[uni]) & (x[:, uni] <= b[uni]))
    # the intended path ran ...
    assert c.path
    for word in c.path:
        assert word in kernel, kernel
    if "scratch" in (c.variant or ""):
        assert "inc" not in kernel, kernel
    else:
        assert st.step > 40 * L
    if c.mode is not None:
        m = re.search(r"step_inc_kernel<(\d+), (\d),", kernel)
        assert m, kernel
        assert int(m.group(2)) == c.mode, kernel
        if c.dq is not None:
            assert int(m.group(1)) == c.dq, kernel
    # ... on trials that did leave the support (a silently centred case fails here).  A dragging
    # step whose slow trial leaves the support is not counted in prior_rej (mcmc.py:590-592): there
    # the walkers themselves must sit at the walls
    if c.variant in ("drag", "scratch drag"):
        assert S.near_wall(st.x, a, b, kinds, periodic).mean() > 0.15
    else:
        assert out > 0.15 * c.W
    if per:
        assert wraps > 20
    eng.close()


def test_binned_likelihood_steps_at_a_moved_wall_bit_exact():
    """plik-lite (pl_fused_kernel): one wall of the box moved to 0.3 sigma from the fiducial point
    on two emulator parameters."""
    ds = small_dataset()
    target = P.BinnedGaussian.from_dataset(ds)
    emu = P.synthetic_emulator(5, ds.lmax)
    d, W, gs = emu.n + 1, 256, 64
    kinds, a, b, C = sampling_problem(target, emu)
    sig = np.sqrt(np.diag(C))
    a[0] = emu.theta0[0] - 0.3 * sig[0]
    b[3] = emu.theta0[3] + 0.3 * sig[3]
    eng = E.Engine(d, W, group_size=gs, seed=SEED)
    eng.set_prior(kinds, a, b)
    eng.set_target_binned_gaussian(target, emu, calib_index=emu.n)
    eng.set_proposal_cov(C)
    k = eng.binned_constants()
    B = O.Binned(target.bin_table(), target.weights, target.X_data, Linv=k["Linv"],
                 theta0=emu.theta0, D0=emu.D0, J=emu.J, calib=emu.n)
    prob = O.Problem(d, kinds, a, b, T=eng.get_proposal_transform(), group_size=gs, seed=SEED,
                     derived=eng.derived_constants(), binned=B)
    rng = np.random.default_rng(77)
    x0 = np.concatenate((emu.theta0, [1.0])) + rng.standard_normal((W, d)) @ np.linalg.cholesky(C).T
    x0[:, 0] = np.maximum(x0[:, 0], a[0] + 1e-3 * sig[0])
    x0[:, 3] = np.minimum(x0[:, 3], b[3] - 1e-3 * sig[3])
    eng.set_state(x0)
    st = O.State(prob, x0)
    compare_everything(eng, st, "start: ")
    out = 0
    for n in (1, 14, 30):
        rej = st.prior_rej.copy()
        eng.step(n)
        eng.sync()
        st.run(n, n_threads=4)
        compare_everything(eng, st, f"after {st.step} steps: ")
        out += int(np.sum(st.prior_rej > rej))
    assert st.step == 45 and eng.counters()["accepted"] == int(st.n_accept.sum())
    assert "pl_fused_kernel" in eng.last_step_kernel()
    x = eng.get_state()["x"]
    assert np.all((x[:, :emu.n] >= a[:emu.n]) & (x[:, :emu.n] <= b[:emu.n]))
    assert out > 0.15 * W
    eng.close()


# ------------------------------------------------------------------ constants and evaluator
def _wide_box(a, b):
    """A support that holds the points 30 sigma out (sigma is 0.028 of the box's width)."""
    w = b - a
    return (a - 2.0 * w).tolist(), (b + 2.0 * w).tolist()


@pytest.mark.parametrize("scale", S.EVAL_SCALES)
@pytest.mark.parametrize("d,K", S.EVAL_SHAPES)
def test_constants_and_evaluator_against_long_double(d, K, scale):
    """host_linalg.cpp and the evaluator against the long-double reference at off-scale boxes.  The
    bound is measured, not chosen: 4 x the error of the float64 numpy recipe (the reference's own
    arithmetic) against the same long-double values -- two backward-stable solves may differ in
    their elimination and summation order, not in the algorithm --, and no less than the
    summation-order floor (d + 8) 2^-53 max(1, |value|) of tests/test_gpu_drift.py."""
    a, b, means, covs, pts = S.eval_problem(d, K, scale)
    lo, hi = _wide_box(a, b)
    ref = S.loglike_ref(pts, means, covs)
    scale_of = np.maximum(1.0, np.abs(ref.astype(np.float64)))
    err_np = np.max(S.relative_error(S.loglike_numpy(pts, means, covs), ref))
    bound = S.eval_bound(err_np, d, ref)

    eng = E.Engine(d, 64, group_size=64, seed=1)
    eng.set_prior([0] * d, lo, hi)
    eng.set_target_gaussian_mixture(means, covs, None)
    lp, ll = eng.evaluate(pts)
    assert np.all(np.isfinite(lp)) and np.all(np.isfinite(ll))
    err_dev = np.abs(ll - ref).astype(np.float64)
    print(f"[evaluator] d={d} K={K} {scale}: numpy recipe {err_np:.2e}, device "
          f"{np.max(err_dev / scale_of):.2e} (relative to max(1, |loglike|))")
    assert np.all(err_dev <= bound), np.max(err_dev / bound)

    # L^-1 and d log(2 pi) + log det: entry (i, j) of L^-1 multiplies a residual of the size of
    # sigma_j, so the errors are weighed by sigma_j
    dc = eng.derived_constants()
    for k in range(K):
        sig = np.sqrt(np.diag(covs[k]))
        Lld = S.cholesky_ld(covs[k])
        Linv_ld = S.inverse_lower_ld(Lld)
        Lnp = np.linalg.cholesky(covs[k])
        e_np = np.max(np.abs(np.linalg.inv(Lnp) - Linv_ld).astype(np.float64) * sig)
        e_dev = np.max(np.abs(dc["Linv"][k] - Linv_ld).astype(np.float64) * sig)
        size = np.max(np.abs(Linv_ld).astype(np.float64) * sig)
        assert e_dev <= max(4.0 * e_np, (d + 8) * 2.0 ** -53 * size), (k, e_dev, e_np)
        assert np.array_equal(np.triu(dc["Linv"][k], 1), np.zeros((d, d)))
        cn = S.cnorm_ld(Lld)
        c_np = abs(float(d * np.log(2 * np.pi) + 2 * np.sum(np.log(np.diag(Lnp))) - cn))
        c_dev = abs(float(dc["cnorm"][k] - cn))
        assert c_dev <= max(4.0 * c_np, (d + 8) * 2.0 ** -53 * max(1.0, abs(float(cn)))), (k, c_dev, c_np)
        print(f"[constants] d={d} K={K} {scale} mode {k}: L^-1 numpy {e_np:.2e} device {e_dev:.2e}; "
              f"cnorm numpy {c_np:.2e} device {c_dev:.2e}")
    eng.close()

    # the log-likelihood the INCREMENTAL step kernel holds after one step of length ~0 (the trick
    # of test_incremental_kernels_reproduce_the_reference_values_of_g5)
    w = b - a
    inc = E.Engine(d, 64, group_size=64, seed=1, incremental=True)
    inc.set_prior([0] * d, lo, hi)
    inc.set_target_gaussian_mixture(means, covs, None)
    inc.set_proposal_cov(np.diag(1e-40 * w * w))
    inc.set_state(pts[:64])
    inc.step(1)
    inc.sync()
    s = inc.get_full_state()
    assert np.max(np.abs(s["x"] - pts[:64]) / w) <= 1e-18
    moved = s["n_accept"] == 1
    assert moved.sum() >= 56, int(moved.sum())
    err_inc = np.abs(s["loglike"] - ref[:64]).astype(np.float64)
    print(f"[step kernel] d={d} K={K} {scale}: {inc.last_step_kernel()}: device "
          f"{np.max((err_inc / scale_of[:64])[moved]):.2e}")
    assert np.all(err_inc[moved] <= bound[:64][moved]), np.max((err_inc / bound[:64])[moved])
    inc.close()
