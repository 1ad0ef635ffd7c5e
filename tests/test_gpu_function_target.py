"""Function targets on the MI355X (function_kernels.hip; likelihood class `device_function`): the
sampler samples a user's batched device function, the step equals its reference
(tests/function_ref.py) bit for bit by record and replay, evaluation reproduces golden G14, walker
shards compose, the banana's exact moments come out, checkpoints and resume work, and every
failure path is an error message, not a fault."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402

from cobaya_amd import run  # noqa: E402
from cobaya_amd.engine import (ERR_ARG, ERR_CALLBACK, ERR_TARGET, ChainStuck, Engine,  # noqa: E402
                               EngineError, TargetError)
from cobaya_amd.model import ProblemSpec  # noqa: E402
from cobaya_amd.sampler import LoggedError, MCMCHip  # noqa: E402
from tests import function_ref as FR  # noqa: E402

KERNEL = "mcmc::fn_walker_kernel"
BETA, S = 0.5, 0.5


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def banana(p):                      # p: (n, >= 2) device tensor
    return -0.5 * (p[:, 0] ** 2 + ((p[:, 1] - BETA * p[:, 0] ** 2) / S) ** 2)


def banana30(p):                    # the banana in the first two of 30, N(0.5, 0.1^2) in the rest
    return banana(p) - 0.5 * (((p[:, 2:] - 0.5) / 0.1) ** 2).sum(1)


def banana_info(n_walkers=16384, **opts):
    # max_tries: the default (40 d = 80 rejections in a row) is the reference's rule for ONE chain;
    # in the banana's arms the acceptance rate of a Gaussian proposal is a few per cent, and among
    # thousands of walkers over thousands of steps one of them meets 80 rejections in a row (seen:
    # "stuck for 80 attempts (walker 1782)" at 4 096 walkers).  Nothing else differs from the defaults.
    opts = {"max_tries": "2000d", **opts}
    return {"likelihood": {"banana": {"class": "device_function", "function": banana}},
            "params": {"a": {"prior": {"min": -8, "max": 8}, "ref": 0, "proposal": 1},
                       "b": {"prior": {"min": -6, "max": 30}, "ref": 0.5, "proposal": 1}},
            "sampler": {"mcmc_hip": {"n_walkers": n_walkers, **opts}}}


# ------------------------------------------------------------------------------ 4. the sampler
def test_run_samples_the_banana_on_the_new_kernel():
    """Fails without the feature: the class `device_function` was refused by ProblemSpec."""
    info = banana_info(2048, seed=3, group_size=64, max_samples=2048 * 300, Rminus1_stop=0.0)
    updated, sampler = run(info)
    assert sampler.engine.last_step_kernel().startswith(KERNEL), sampler.engine.last_step_kernel()
    assert sampler.incremental is False
    df = sampler.products()["sample"].data
    assert len(df) > 0 and "chi2__banana" in df.columns
    x = df[["a", "b"]].to_numpy()
    ll = banana(torch.as_tensor(x)).numpy()
    np.testing.assert_allclose(df["chi2__banana"].to_numpy(), -2 * ll, rtol=1e-12, atol=1e-12)
    assert updated["likelihood"]["banana"]["function"] is banana


# ------------------------------------------------------------------------------ 5. bit parity
class Recorder:
    """The test's function: a separable Gaussian bowl, -inf on part of the support (first
    parameter above `cut`); records, per call while `on`, the points it was given and the values
    it returned, copied to the host."""

    def __init__(self, cut=0.6):
        self.cut, self.on, self.calls = cut, False, []

    def __call__(self, p):
        ll = -0.5 * (((p - 0.45) / 0.2) ** 2).sum(1)
        ll = torch.where(p[:, 0] > self.cut, torch.full_like(ll, -float("inf")), ll)
        if self.on:
            self.calls.append((p.cpu().numpy().copy(), ll.cpu().numpy().copy()))
        return ll


def _mixed(d, seed):
    rng = np.random.default_rng(seed)
    kinds = np.array([1 if i % 3 == 1 else 0 for i in range(d)], np.int32)
    a = np.where(kinds == 1, 0.5, 0.0)
    b = np.where(kinds == 1, 0.3, 1.0)
    A = rng.standard_normal((d, d)) / np.sqrt(d)
    cov = 0.01 * (A @ A.T + np.eye(d))
    return kinds, a, b, cov, rng


def _pair(d, W, gs, f, seed=7, burn_in=3, temperature=1.5, max_tries=None, cov_scale=1.0,
          walker_offset=0, x0=None):
    kinds, a, b, cov, rng = _mixed(d, seed)
    cov = cov * cov_scale
    eng = Engine(d, W, group_size=gs, device=0, seed=seed, burn_in=burn_in, temperature=temperature,
                 max_tries=max_tries, walker_offset=walker_offset)
    eng.set_prior(kinds, a, b)
    eng.set_target_function(f)
    eng.set_proposal_cov(cov)
    if x0 is None:
        x0 = np.clip(0.45 + 0.3 * rng.standard_normal((W, d)) * np.sqrt(np.diag(cov)), 0.01, 0.55)
        x0[::4, 0] = 0.001          # against the lower bound of the first (uniform) parameter
        x0[1::4, 0] = 0.5999        # ... and just below the Recorder's cut (-inf above it)
    eng.set_state(x0)
    prob = FR.problem(d, kinds, a, b, eng.get_proposal_transform(), group_size=gs, seed=seed,
                      temperature=temperature, max_tries=max_tries, derived=eng.derived_constants())
    ref = FR.FunctionRef(prob, x0, eng.get_state()["loglike"], burn_in=burn_in, walker0=walker_offset)
    return eng, ref


def _assert_states_equal(eng, ref):
    st = eng.get_full_state()
    assert np.array_equal(_bits(st["x"]), _bits(ref.x))
    for k in ("logpost", "logprior", "loglike"):
        assert np.array_equal(_bits(st[k]), _bits(getattr(ref, k))), k
    for k in ("weight", "prior_rej", "burn_left", "n_accept"):
        assert np.array_equal(st[k], getattr(ref, k)), k
    assert int(st["step"]) == ref.step
    return st


@pytest.mark.parametrize("d,W,gs", [(1, 256, 64), (2, 1024, 256), (30, 512, 64), (33, 256, 64),
                                     (100, 256, 64), (128, 512, 128)])
def test_step_equals_the_reference_by_record_and_replay(d, W, gs):
    """Proposal, prior, accept rule and bookkeeping, independent of the rounding of the function:
    the reference is stepped with the values the function returned on the device.  At every
    step the points the function was given equal the reference's trials bit for bit; at the end of
    each of three uneven launches the whole state is equal.  Temperature 1.5, burn-in 3, walkers
    started against a bound (prior_rej > 0), -inf on part of the support."""
    rec = Recorder()
    eng, ref = _pair(d, W, gs, rec)
    _assert_states_equal(eng, ref)
    seen_rej = seen_inf = 0
    rec.on = True
    for n in (d + 3, 1, 2 * d + 5):
        rec.calls.clear()
        eng.step(n)
        eng.sync()
        assert len(rec.calls) == n
        for pts, ll in rec.calls:
            t = ref.propose()
            assert np.array_equal(_bits(pts), _bits(t)), (d, ref.step)
            seen_inf += int(np.sum(np.isinf(ll) & np.isfinite(ref.lp_t)))
            ref.accept(ll)
            seen_rej += int(ref.prior_rej.sum())
        _assert_states_equal(eng, ref)
    assert eng.last_step_kernel().startswith(KERNEL)
    assert ref.n_accept.sum() > 0 and seen_rej > 0 and (ref.burn_left < 4).any()
    assert seen_inf > 0
    assert eng.counters()["accepted"] == int(ref.n_accept.sum())
    eng.close()


def test_stuck_is_reported_as_by_the_reference():
    rec = Recorder()
    eng, ref = _pair(2, 256, 64, rec, max_tries=2.0, cov_scale=2500.0, burn_in=0, temperature=1.0)
    rec.on = True
    eng.step(60)
    with pytest.raises(ChainStuck, match="stuck"):
        eng.sync()
    for pts, ll in rec.calls:
        assert np.array_equal(_bits(pts), _bits(ref.propose()))
        ref.accept(ll)
    assert ref.stuck[0] != 0
    _assert_states_equal(eng, ref)
    eng.close()


# ------------------------------------------------------------------------------ 6. G14
def test_g14_through_engine_evaluate(golden):
    g = golden("g14_external_function")
    c_loc, c_scale = float(g["c_loc"]), float(g["c_scale"])

    def f(p):
        return banana(p) - 0.5 * ((p[:, 2] - c_loc) / c_scale) ** 2

    eng = Engine(3, 64, group_size=64, device=0, seed=1)
    eng.set_prior(g["kinds"], g["a"], g["b"])
    eng.set_target_function(f)
    lp, ll = eng.evaluate(g["points"])
    assert np.array_equal(np.isinf(lp), np.isinf(g["logprior"]))
    assert np.array_equal(np.isinf(ll), np.isinf(g["loglike"]))
    ok = np.isfinite(lp)
    np.testing.assert_allclose(lp[ok], g["logprior"][ok], rtol=1e-12, atol=0)
    np.testing.assert_allclose(ll[ok], g["loglike"][ok], rtol=1e-12, atol=0)
    # ... and the log-prior is, bit for bit, the one of the `one` target and of the oracle
    prob = FR.problem(3, g["kinds"], g["a"], g["b"], np.eye(3), derived=eng.derived_constants())
    assert np.array_equal(_bits(lp), _bits(prob.evaluate(g["points"])[0]))
    eng.set_target_one()
    assert np.array_equal(_bits(eng.evaluate(g["points"])[0]), _bits(lp))
    eng.close()


# ------------------------------------------------------------------------------ 7. shards
@pytest.mark.parametrize("d,gs", [(2, 64), (40, 128)])
def test_walker_shards_compose(d, gs):
    """Two engines with walker_offset 0 and W / 2 equal the halves of one (a pointwise function
    of +, -, x on columns)."""
    def f(p):
        q = p - 0.45
        return -(q * q).sum(1) * 12.5

    W = 4 * gs
    whole, ref = _pair(d, W, gs, f, seed=9)
    x0 = ref.x.copy()
    halves = [_pair(d, W // 2, gs, f, seed=9, walker_offset=o, x0=x0[o:o + W // 2])[0]
              for o in (0, W // 2)]
    for n in (d + 2, 3 * d + 1):
        for e in [whole] + halves:
            e.step(n)
            e.sync()
    st = whole.get_full_state()
    assert st["n_accept"].sum() > 0
    for o, e in zip((0, W // 2), halves):
        sh = e.get_full_state()
        for k in ("x", "logpost", "logprior", "loglike"):
            assert np.array_equal(_bits(sh[k]), _bits(st[k][o:o + W // 2])), k
        for k in ("weight", "prior_rej", "burn_left", "n_accept"):
            assert np.array_equal(sh[k], st[k][o:o + W // 2]), k
        e.close()
    whole.close()


# ------------------------------------------------------------------------------ 8. posterior
def _check_banana_moments(x):
    """Exact moments of a ~ N(0, 1), b | a ~ N(beta a^2, s^2), beta = s = 0.5: E a = 0, Var a = 1,
    E b = beta, Var b = 2 beta^2 + s^2 = 0.75, mu4(b) = 60 beta^4 + 12 beta^2 s^2 + 3 s^4 = 4.6875;
    standard errors of N independent draws: sigma / sqrt(N) for the means,
    sqrt((mu4 - sigma^4) / N) for the variances."""
    N = len(x)
    var_b, mu4_b = 2 * BETA ** 2 + S ** 2, 60 * BETA ** 4 + 12 * BETA ** 2 * S ** 2 + 3 * S ** 4
    checks = {"E a": (x[:, 0].mean(), 0.0, np.sqrt(1.0 / N)),
              "Var a": (x[:, 0].var(ddof=1), 1.0, np.sqrt((3.0 - 1.0) / N)),
              "E b": (x[:, 1].mean(), BETA, np.sqrt(var_b / N)),
              "Var b": (x[:, 1].var(ddof=1), var_b, np.sqrt((mu4_b - var_b ** 2) / N))}
    for name, (got, want, se) in checks.items():
        print("%s: got %.5f want %.5f  (%.2f standard errors)" % (name, got, want, (got - want) / se))
    for name, (got, want, se) in checks.items():
        assert abs(got - want) < 6 * se, (name, got, want, se)


def test_posterior_banana_moments_d2():
    """16 384 walkers, default learning, to Rminus1_stop 0.01: the final ensemble's means and
    variances lie within 6 standard errors (of 16 384 independent draws) of the exact values."""
    info = banana_info(16384, seed=11, Rminus1_stop=0.01, max_samples=16384 * 200000)
    _, sampler = run(info)
    assert sampler.converged, sampler.Rminus1_last
    assert sampler.engine.last_step_kernel().startswith(KERNEL)
    _check_banana_moments(sampler.engine.get_state()["x"])


def test_posterior_banana_moments_d30():
    """The same banana in the first two of 30 parameters, independent N(0.5, 0.1^2) Gaussians in
    the rest (uniform priors on [0, 1]): the same bar."""
    info = banana_info(16384, seed=12, Rminus1_stop=0.01, max_samples=16384 * 400000)
    info["likelihood"] = {"banana30": {"class": "device_function", "function": banana30}}
    for i in range(28):
        info["params"]["g%02d" % i] = {"prior": {"min": 0, "max": 1}, "ref": 0.5, "proposal": 0.1}
    _, sampler = run(info)
    assert sampler.converged, sampler.Rminus1_last
    x = sampler.engine.get_state()["x"]
    _check_banana_moments(x)
    N = len(x)
    assert np.all(np.abs(x[:, 2:].mean(0) - 0.5) < 6 * 0.1 / np.sqrt(N))
    assert np.all(np.abs(x[:, 2:].var(0, ddof=1) - 0.01) < 6 * 0.01 * np.sqrt(2.0 / N))


# ------------------------------------------------------------------------------ 9. checkpoints, resume
@pytest.mark.parametrize("mode", [False, "reduce"])
def test_learn_and_convergence_checkpoints(mode):
    info = banana_info(4096, seed=5, group_size=64, Rminus1_stop=0.05, device_checkpoint=mode,
                       max_samples=4096 * 100000, bounds_snapshots=8)
    _, sampler = run(info)
    assert bool(sampler._device_ckpt) == bool(mode)
    assert np.isfinite(sampler.Rminus1_last) and sampler.converged
    x = sampler.engine.get_state()["x"]
    assert abs(x[:, 0].mean()) < 0.2 and abs(x[:, 1].mean() - BETA) < 0.2
    assert sampler.engine.last_step_kernel().startswith(KERNEL)


def test_resume_continues_bit_identically(tmp_path):
    """The state file does not describe the function: a resumed run takes it from the new input,
    and continues bit-identically to an uninterrupted one."""
    def make(prefix, resume, max_samples):
        opts = {"seed": 21, "n_walkers": 512, "group_size": 64, "steps_per_launch": 40,
                "max_samples": max_samples, "Rminus1_stop": 0.0, "learn_every": "20d"}
        return MCMCHip(opts, ProblemSpec.from_info(banana_info()), output=prefix, resume=resume)

    a = make(str(tmp_path / "a"), False, 60000)
    a.run()
    ref = a.engine.get_full_state()
    steps_total = a.n_steps_raw
    a.close()
    b1 = make(str(tmp_path / "b"), False, 30000)
    b1.run()
    assert b1.n_steps_raw < steps_total
    b1.close()
    b2 = make(str(tmp_path / "b"), True, 60000)
    assert b2.n_steps_raw == b1.n_steps_raw
    b2.run()
    got = b2.engine.get_full_state()
    assert b2.n_steps_raw == steps_total
    for k in ("x", "logpost", "logprior", "loglike", "weight", "n_accept", "burn_left", "prior_rej"):
        assert np.array_equal(got[k], ref[k]), k
    assert int(got["step"]) == int(ref["step"])
    b2.close()


# ------------------------------------------------------------------------------ generic engine services
def test_generic_services_work_around_a_function_target():
    """Moments (read and request / fetch), the bounds ring, get / set_full_state and timing."""
    rec = Recorder()
    eng, ref = _pair(5, 256, 64, rec, seed=4)
    eng.enable_timing(True)
    eng.bounds_configure(2)
    eng.step(12)
    eng.accumulate_moments()
    eng.bounds_snapshot(0)
    st = eng.get_full_state()
    n, gsum, S = eng.read_moments()
    assert n == 1
    np.testing.assert_allclose(gsum.sum(0), st["x"].sum(0), rtol=1e-12)
    assert np.array_equal(_bits(eng.bounds_get_slot(0)), _bits(st["x"]))
    eng.request_moments()
    n2, gsum2, _, c = eng.fetch_moments()
    assert n2 == 1 and c["steps"] == 12 and c["accepted"] == int(st["n_accept"].sum())
    times = eng.kernel_times()
    assert times["step_launches"] == 12 and times["step_ms"] > 0
    # a second engine continues from the saved state exactly as the first
    other, _ = _pair(5, 256, 64, rec, seed=4)
    other.set_full_state(st)
    for e in (eng, other):
        e.step(9)
        e.sync()
    a, b = eng.get_full_state(), other.get_full_state()
    for k in ("x", "logpost", "n_accept", "weight"):
        assert np.array_equal(a[k], b[k]), k
    assert int(a["step"]) == int(b["step"]) == 21
    eng.close()
    other.close()


def test_pass_out_hands_the_result_buffer_to_the_function():
    """`pass_out=True`: the function writes into the engine's own (n,) buffer; the steps equal
    those of the same function returning a fresh tensor.  A function with a parameter that merely
    is NAMED `out` is called with the points alone."""
    seen = []

    def plain(p, out=None):
        seen.append(out)
        return -((p - 0.5) ** 2).sum(1) * 50.0

    def into(p, out):
        assert out.shape == (len(p),) and out.dtype == torch.float64 and out.device == p.device
        torch.sum((p - 0.5) ** 2, 1, out=out)
        return out.mul_(-50.0)

    states = []
    for fn, kw in ((plain, {}), (into, {"pass_out": True})):
        eng = Engine(3, 128, group_size=64, device=0, seed=6)
        eng.set_prior(np.zeros(3, np.int32), np.zeros(3), np.ones(3))
        eng.set_target_function(fn, **kw)
        eng.set_proposal_cov(0.01 * np.eye(3))
        eng.set_state(_x0(128, 3))
        eng.step(25)
        eng.sync()
        states.append(eng.get_full_state())
        eng.close()
    assert seen and all(o is None for o in seen)
    assert states[0]["n_accept"].sum() > 0
    for k in ("x", "logpost", "loglike", "n_accept", "weight"):
        assert np.array_equal(states[0][k], states[1][k]), k


# ------------------------------------------------------------------------------ 10. failure paths
def _small(f, d=2, W=128, **kw):
    eng = Engine(d, W, group_size=64, device=0, seed=2, **kw)
    eng.set_prior(np.zeros(d, np.int32), np.zeros(d), np.ones(d))
    eng.set_target_function(f)
    eng.set_proposal_cov(0.01 * np.eye(d))
    return eng


def _x0(W=128, d=2):
    return np.random.default_rng(0).uniform(0.3, 0.7, (W, d))


def test_an_exception_in_the_function_is_the_cause_and_the_engine_stays_usable():
    state = {"fail": False}

    def f(p):
        if state["fail"]:
            raise ValueError("boom at the user's side")
        return -((p - 0.5) ** 2).sum(1) * 50.0

    eng = _small(f)
    eng.set_state(_x0())
    eng.step(3)
    eng.sync()
    before = eng.get_full_state()
    state["fail"] = True
    with pytest.raises(EngineError) as ei:
        eng.step(5)
    assert ei.value.code == ERR_CALLBACK
    assert isinstance(ei.value.__cause__, ValueError) and "boom" in str(ei.value.__cause__)
    eng.sync()
    after = eng.get_full_state()
    assert int(after["step"]) == 3          # the pending trial was dropped
    assert np.array_equal(_bits(after["x"]), _bits(before["x"]))
    with pytest.raises(EngineError) as ei:
        eng.evaluate(_x0())
    assert isinstance(ei.value.__cause__, ValueError)
    state["fail"] = False
    eng.step(4)
    eng.sync()
    assert int(eng.get_full_state()["step"]) == 7
    eng.close()


@pytest.mark.parametrize("bad,match", [
    (lambda p: p[:, 0:1] * 0.0, r"shape \(128,\), got shape \(128, 1\)"),
    (lambda p: (p[:, 0] * 0.0).float(), "dtype torch.float64, got dtype torch.float32"),
    (lambda p: (p[:, 0] * 0.0).cpu(), "device cuda:0, got device cpu"),
    (lambda p: [0.0] * len(p), "must return a torch.Tensor, got list"),
])
def test_a_wrong_result_is_refused_by_name(bad, match):
    eng = _small(bad)
    with pytest.raises(EngineError) as ei:
        eng.set_state(_x0())
    assert ei.value.code == ERR_CALLBACK
    assert ei.value.__cause__ is not None
    import re
    assert re.search(match, str(ei.value.__cause__)), str(ei.value.__cause__)
    eng.close()


def test_nan_inside_the_support_is_an_error_of_the_target_outside_it_is_ignored():
    mode = {"nan": "none"}

    def f(p):
        ll = -((p - 0.5) ** 2).sum(1) * 50.0
        outside = ((p < 0) | (p > 1)).any(1)
        if mode["nan"] == "outside":
            ll = torch.where(outside, torch.full_like(ll, float("nan")), ll)
        elif mode["nan"] == "walker 70":
            ll[70] = float("nan")
        elif mode["nan"] == "inf":
            ll[5] = float("inf")
        return ll

    eng = _small(f)
    eng.set_proposal_cov(0.5 * np.eye(2))     # wide: many trials leave the unit box
    eng.set_state(_x0())
    mode["nan"] = "outside"
    eng.step(20)
    eng.sync()                                 # NaN only outside the support: runs clean
    st = eng.get_full_state()
    assert st["prior_rej"].sum() > 0 or st["n_accept"].sum() > 0
    assert np.all(np.isfinite(st["logpost"]))
    eng.set_proposal_cov(1e-6 * np.eye(2))    # narrow: every trial stays inside
    mode["nan"] = "walker 70"
    eng.step(2)
    with pytest.raises(TargetError, match=r"walker 70\b") as ei:
        eng.sync()
    assert ei.value.code == ERR_TARGET
    eng.request_moments()
    with pytest.raises(TargetError, match=r"walker 70\b"):
        eng.fetch_moments()
    # evaluate reports it at once; a fresh state clears the flag
    with pytest.raises(TargetError, match="point 70"):
        eng.evaluate(_x0())
    mode["nan"] = "none"
    eng.set_state(_x0())
    eng.step(2)
    eng.sync()
    mode["nan"] = "inf"
    eng.step(1)
    with pytest.raises(TargetError, match=r"walker 5\b"):
        eng.sync()
    eng.close()


def test_the_global_walker_id_is_named_with_a_walker_offset():
    mode = {"nan": False}

    def f(p):
        ll = -((p - 0.5) ** 2).sum(1)
        if mode["nan"]:
            ll[3] = float("nan")
        return ll

    eng = _small(f, walker_offset=640)
    eng.set_proposal_cov(1e-6 * np.eye(2))
    eng.set_state(_x0())
    mode["nan"] = True
    eng.step(1)
    with pytest.raises(TargetError, match=r"walker 643\b"):
        eng.sync()
    eng.close()


def test_unserved_configurations_are_refused_by_name_and_a_served_one_runs_after():
    f = lambda p: -((p - 0.5) ** 2).sum(1) * 50.0   # noqa: E731
    d = 4
    kinds, lo, hi = np.zeros(d, np.int32), np.zeros(d), np.ones(d)

    def engine(**kw):
        eng = Engine(d, 128, group_size=64, device=0, seed=2, **kw)
        eng.set_prior(kinds, lo, hi)
        return eng

    def refused(eng, match, call=None):
        with pytest.raises(EngineError, match=match) as ei:
            (call or (lambda: eng.set_target_function(f)))()
        assert ei.value.code == ERR_ARG
        # the engine stays healthy after a refusal
        eng.set_target_one()
        lp, ll = eng.evaluate(np.full((3, d), 0.5))
        assert np.all(ll == 0.0) and np.all(np.isfinite(lp))
        eng.close()

    refused(engine(incremental=True), "MCMC_HIP_FLAG_INCREMENTAL")
    refused(engine(shared_basis=False), "MCMC_HIP_FLAG_OWN_BASIS")
    refused(engine(emit_capacity=4), "emit_capacity > 0")
    eng = engine()
    eng.set_blocking([[0, 1], [2, 3]], [1, 2])
    refused(eng, "parameter blocks")
    eng = engine()
    eng.set_blocking([[0, 1], [2, 3]], [1, 1], drag_last_slow=0, drag_steps=2)
    refused(eng, "dragging")
    eng = Engine(d, 128, group_size=64, device=0, seed=2)
    eng.set_prior(kinds, lo, hi, np.array([0, 1, 0, 0], np.int32))
    refused(eng, "periodic parameters")
    # set after the target: refused by the step
    eng = engine()
    eng.set_target_function(f)
    eng.set_blocking([[0, 1], [2, 3]], [1, 2])
    eng.set_proposal_cov(0.01 * np.eye(d))
    eng.set_state(np.full((128, d), 0.5))
    refused(eng, "parameter blocks", call=lambda: eng.step(1))
    # d > 128: the engine exists only with incremental evaluation, which the target refuses
    big = Engine(130, 128, group_size=64, device=0, seed=2, incremental=True)
    with pytest.raises(EngineError, match="d <= 128") as ei:
        big.set_target_function(f)
    assert ei.value.code == ERR_ARG
    big.close()
    with pytest.raises(EngineError, match="callable"):
        engine().set_target_function(3)
    # the sampler refuses by the option's name (more in tests/test_function_target_host.py)
    with pytest.raises(LoggedError, match="emit: chains is not served"):
        run(banana_info(128, seed=1, group_size=64, emit="chains"))
    # ... and a served shape runs after all of them
    eng = engine()
    eng.set_target_function(f)
    eng.set_proposal_cov(0.01 * np.eye(d))
    eng.set_state(np.full((128, d), 0.5))
    eng.step(8)
    eng.sync()
    assert eng.last_step_kernel().startswith(KERNEL)
    assert eng.get_full_state()["n_accept"].sum() > 0
    eng.close()
