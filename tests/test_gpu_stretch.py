"""The stretch move on the MI355X (stretch_kernels.hip; `move: stretch`, mcmc_hip_set_move): the
two half-updates of a step equal their reference (tests/stretch_ref.py) bit for bit by record and
replay -- and differ from the reference with the wrong ordering --, launches split, walker shards
compose, the full state round-trips, step indices beyond 2^32 work, every failure path is an error
message, and the sampler runs the banana to convergence with the default max_tries."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402

from cobaya_amd import run  # noqa: E402
from cobaya_amd.engine import (ERR_ARG, ERR_CALLBACK, ERR_STATE, ERR_TARGET, Engine,  # noqa: E402
                               EngineError, TargetError)
from cobaya_amd.model import ProblemSpec  # noqa: E402
from cobaya_amd.sampler import MCMCHip  # noqa: E402
from tests import stretch_ref as SR  # noqa: E402
from tests.products_together import PRODUCTS, same_as_replayed  # noqa: E402
from tests.test_gpu_function_target import _check_banana_moments, banana  # noqa: E402
from tests.test_gpu_products_together import _info as products_info  # noqa: E402

KERNEL = "mcmc::stretch_kernel"


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


class Recorder:
    """The test's function: a wide separable Gaussian bowl, -inf on part of the support (first
    parameter above `cut`); records, per call while `on`, the points it was given and the values it
    returned, copied to the host."""

    def __init__(self, cut=0.93):
        self.cut, self.on, self.calls = cut, False, []

    def __call__(self, p):
        ll = -0.5 * (((p - 0.45) / 0.5) ** 2).sum(1)
        ll = torch.where(p[:, 0] > self.cut, torch.full_like(ll, -float("inf")), ll)
        if self.on:
            self.calls.append((p.cpu().numpy().copy(), ll.cpu().numpy().copy()))
        return ll


def _priors(d):
    """Uniform on the unit box, N(0.5, 0.3^2) on every third dimension."""
    kinds = np.array([1 if i % 3 == 1 else 0 for i in range(d)], np.int32)
    return kinds, np.where(kinds == 1, 0.5, 0.0), np.where(kinds == 1, 0.3, 1.0)


def _start(W, d, seed):
    """Spread over the whole unit box: about a tenth of the trials leave it per uniform dimension."""
    x0 = np.random.default_rng(seed).uniform(0.02, 0.98, (W, d))
    x0[:, 0] *= 0.93 / 0.98     # (below the Recorder's cut)
    return x0


def _pair(d, W, gs, f, seed=7, burn_in=3, temperature=1.0, a=2.0, max_tries=None, walker_offset=0, x0=None,
          stale=False):
    kinds, pa, pb = _priors(d)
    eng = Engine(d, W, group_size=gs, device=0, seed=seed, burn_in=burn_in, temperature=temperature,
                 max_tries=max_tries, walker_offset=walker_offset)
    eng.set_prior(kinds, pa, pb)
    eng.set_target_function(f)
    eng.set_move("stretch", a)
    if x0 is None:
        x0 = _start(W, d, seed)
    eng.set_state(x0)           # (no proposal covariance: the move needs none)
    prob = SR.problem(d, kinds, pa, pb, group_size=gs, seed=seed, temperature=temperature,
                      max_tries=max_tries, derived=eng.derived_constants())
    ref = SR.StretchRef(prob, x0, eng.get_state()["loglike"], a=a, burn_in=burn_in, walker0=walker_offset,
                        stale_partners=stale)
    return eng, ref


def _states_differ(eng, ref):
    """Names of the parts of the full state in which engine and reference differ."""
    st = eng.get_full_state()
    out = [k for k in ("x", "logpost", "logprior", "loglike") if not np.array_equal(_bits(st[k]), _bits(getattr(ref, k)))]
    out += [k for k in ("weight", "prior_rej", "burn_left", "n_accept") if not np.array_equal(st[k], getattr(ref, k))]
    if int(st["step"]) != ref.step:
        out.append("step")
    return out


def _replay(eng, ref, rec, n_steps, check_rows=True):
    """Steps the engine, then the reference with the values the device's function returned."""
    rec.calls.clear()
    rec.on = True
    eng.step(n_steps)
    eng.sync()
    rec.on = False
    assert len(rec.calls) == 2 * n_steps
    n_out = n_inf = 0
    for pts, ll in rec.calls:
        t = ref.propose()
        assert pts.shape == t.shape == (ref.W // 2, ref.d)
        if check_rows:
            assert np.array_equal(_bits(pts), _bits(t)), (ref.d, ref.step, ref.half)
        n_out += int(np.sum(np.isinf(ref.lp_t)))
        n_inf += int(np.sum(np.isinf(ll) & np.isfinite(ref.lp_t)))
        ref.accept(ll)
    return n_out, n_inf


# ------------------------------------------------------------------------------ 1. bit parity
# d on both sides of the 32-dimension tile and of the one-chain / four-chain prior sum; 2 to 4 groups
# (3 groups of 64: the last workgroup holds one group, 32 active lanes); temperature, a and
# walker_offset vary over the cases
CASES = [(1, 64, 3, 1.0, 2.0, 0), (2, 64, 4, 2.0, 1.5, 128), (16, 64, 3, 2.0, 2.0, 64),
         (31, 128, 2, 1.0, 1.5, 256), (32, 128, 3, 2.0, 2.0, 0), (33, 256, 2, 1.0, 2.0, 512),
         (64, 256, 2, 2.0, 1.5, 0)]


@pytest.mark.parametrize("d,gs,G,temperature,a,offset", CASES)
def test_step_equals_the_reference_by_record_and_replay(d, gs, G, temperature, a, offset):
    """State, log-values, weights, prior_rej, accept counters and the rows of every call, bit for bit,
    over three uneven launches.  From d = 16 up at least a fifth of the trials leave the box."""
    rec = Recorder()
    eng, ref = _pair(d, G * gs, gs, rec, temperature=temperature, a=a, walker_offset=offset)
    assert _states_differ(eng, ref) == []
    n_out = n_inf = n_trials = 0
    for n in (3, 1, 4):
        o, i = _replay(eng, ref, rec, n)
        n_out, n_inf, n_trials = n_out + o, n_inf + i, n_trials + n * G * gs
        assert _states_differ(eng, ref) == []
    print("d = %d: %.3f of the trials left the box, %d met -inf inside it, acceptance %.3f" % (
        d, n_out / n_trials, n_inf, ref.n_accept.sum() / n_trials))
    assert eng.last_step_kernel().startswith(KERNEL)
    assert ref.n_accept.sum() > 0 and n_out > 0 and ref.prior_rej.sum() > 0 and (ref.burn_left < 4).any()
    assert n_out >= 0.2 * n_trials or d < 16
    assert n_inf > 0 or d > 16
    assert eng.counters()["accepted"] == int(ref.n_accept.sum()) and eng.counters()["steps"] == 8
    eng.close()


@pytest.mark.parametrize("d,gs", [(2, 64), (33, 256)])
def test_half_1_reads_the_partners_half_0_has_just_committed(d, gs):
    """The power of the replay: the reference whose half 1 reads the partners of BEFORE the step is
    a different chain; the device must be the right one, and not this one."""
    rec = Recorder()
    eng, right = _pair(d, 2 * gs, gs, rec)
    spare, wrong = _pair(d, 2 * gs, gs, rec, stale=True)
    spare.close()
    rec.calls.clear()
    rec.on = True
    eng.step(3)
    eng.sync()
    rec.on = False
    differ = 0
    for pts, ll in rec.calls:
        assert np.array_equal(_bits(pts), _bits(right.propose()))
        differ += int(np.any(_bits(pts) != _bits(wrong.propose()), axis=1).sum())
        right.accept(ll)
        wrong.accept(ll)
    assert _states_differ(eng, right) == []
    assert differ > 0 and "x" in _states_differ(eng, wrong)
    eng.close()


# ------------------------------------------------------------------------------ 2. launches, shards, state
def _smooth(p):
    q = p - 0.45
    return -(q * q).sum(1) * 2.0


def _same_full_state(a, b, lo=0, hi=None):
    for k in ("x", "logpost", "logprior", "loglike"):
        assert np.array_equal(_bits(a[k][lo:hi]), _bits(b[k])), k
    for k in ("weight", "prior_rej", "burn_left", "n_accept"):
        assert np.array_equal(a[k][lo:hi], b[k]), k


@pytest.mark.parametrize("d,gs", [(3, 64), (40, 256)])
def test_one_call_of_2n_steps_equals_2n_calls_of_one(d, gs):
    one, _ = _pair(d, 2 * gs, gs, _smooth)
    many, _ = _pair(d, 2 * gs, gs, _smooth)
    one.step(6)
    for _ in range(6):
        many.step(1)
    one.sync()
    many.sync()
    a, b = one.get_full_state(), many.get_full_state()
    assert a["n_accept"].sum() > 0 and int(a["step"]) == int(b["step"]) == 6
    _same_full_state(a, b)
    one.close()
    many.close()


@pytest.mark.parametrize("d,gs", [(2, 64), (40, 256)])
def test_walker_shards_compose(d, gs):
    """Two engines with walker_offset 0 and W / 2 equal the halves of one: partners never leave the
    group (a pointwise function of +, -, x on columns)."""
    W = 4 * gs
    whole, ref = _pair(d, W, gs, _smooth, seed=9)
    x0 = ref.x.copy()
    halves = [_pair(d, W // 2, gs, _smooth, seed=9, walker_offset=o, x0=x0[o:o + W // 2])[0] for o in (0, W // 2)]
    for n in (2, 3):
        for e in [whole] + halves:
            e.step(n)
            e.sync()
    st = whole.get_full_state()
    assert st["n_accept"].sum() > 0
    for o, e in zip((0, W // 2), halves):
        _same_full_state(st, e.get_full_state(), o, o + W // 2)
        e.close()
    whole.close()


def test_full_state_round_trip():
    rec = Recorder()
    eng, ref = _pair(5, 256, 64, rec, seed=4)
    _replay(eng, ref, rec, 4)
    st = eng.get_full_state()
    other, _ = _pair(5, 256, 64, rec, seed=4)
    other.set_full_state(st)
    for e in (eng, other):
        e.step(5)
        e.sync()
    a, b = eng.get_full_state(), other.get_full_state()
    _same_full_state(a, b)
    assert int(a["step"]) == int(b["step"]) == 9 and a["n_accept"].sum() > st["n_accept"].sum()
    eng.close()
    other.close()


def test_replay_across_step_2_to_the_32():
    """The step enters the Philox counter as two words: a replay from 2^32 - 2 crosses the carry."""
    rec = Recorder()
    eng, ref = _pair(3, 128, 64, rec, seed=5)
    _replay(eng, ref, rec, 2)
    fs = eng.get_full_state()
    fs["step"] = np.uint64((1 << 32) - 2)
    eng.set_full_state(fs)
    ref.step = (1 << 32) - 2
    _replay(eng, ref, rec, 5)
    assert _states_differ(eng, ref) == [] and ref.step == (1 << 32) + 3
    # ... and the trials there are not those of the low word alone: the same state at step 3
    fs = eng.get_full_state()
    low, _ = _pair(3, 128, 64, rec, seed=5)
    low.set_full_state(dict(fs, step=np.uint64(3)))
    for e in (eng, low):
        e.step(1)
        e.sync()
    assert not np.array_equal(_bits(low.get_full_state()["x"]), _bits(eng.get_full_state()["x"]))
    eng.close()
    low.close()


# ------------------------------------------------------------------------------ 3. failure paths
def _small(f, d=2, W=128, gs=64, move=True, box=(0.0, 1.0), **kw):
    eng = Engine(d, W, group_size=gs, device=0, seed=2, **kw)
    eng.set_prior(np.zeros(d, np.int32), np.full(d, box[0]), np.full(d, box[1]))
    eng.set_target_function(f)
    if move:
        eng.set_move("stretch", 2.0)
    return eng


def _x0(W=128, d=2):
    return np.random.default_rng(0).uniform(0.3, 0.7, (W, d))


def test_nan_inside_the_support_names_the_walker():
    mode = {"row": None}

    def f(p):
        ll = -((p - 0.5) ** 2).sum(1) * 0.5
        if mode["row"] is not None:
            ll[mode["row"]] = float("nan")
        return ll

    eng = _small(f, walker_offset=640, box=(-50.0, 50.0))    # (no trial leaves this box)
    eng.set_state(_x0())
    eng.step(2)
    eng.sync()
    assert eng.get_full_state()["prior_rej"].sum() == 0
    # row 37 of half-update 0 is walker 32 + 5 of group 1's half 0: local 64 + 5, global 640 + 69
    mode["row"] = 37
    eng.step(1)
    with pytest.raises(TargetError, match=r"walker 709\b") as ei:
        eng.sync()
    assert ei.value.code == ERR_TARGET
    eng.close()


def test_a_failing_callback_leaves_the_documented_state():
    """The step counter is that of the last completed step; the engine refuses to step until a state
    is set again (half 0 of the interrupted step may be committed)."""
    state = {"calls": 0, "fail_at": None}

    def f(p):
        state["calls"] += 1
        if state["fail_at"] is not None and state["calls"] == state["fail_at"]:
            raise ValueError("boom at the user's side")
        return -((p - 0.5) ** 2).sum(1) * 0.5

    eng, good = _small(f), _small(lambda p: -((p - 0.5) ** 2).sum(1) * 0.5)
    for e in (eng, good):
        e.set_state(_x0())
        e.step(3)
        e.sync()
    state["fail_at"] = state["calls"] + 4       # half 1 of the second step of the next call
    with pytest.raises(EngineError) as ei:
        eng.step(5)
    assert ei.value.code == ERR_CALLBACK and isinstance(ei.value.__cause__, ValueError)
    eng.sync()
    after = eng.get_full_state()
    assert int(after["step"]) == 4              # one step was completed, the second interrupted
    # half 0 of the interrupted step is committed, half 1 is as the completed step left it
    good.step(1)
    good.sync()
    s4 = good.get_full_state()
    good.step(1)
    good.sync()
    s5 = good.get_full_state()
    half0 = (np.arange(128) % 64) < 32
    for k in ("x", "logpost", "weight", "n_accept"):
        assert np.array_equal(after[k][~half0], s4[k][~half0]), k
        assert np.array_equal(after[k][half0], s5[k][half0]), k
    assert not np.array_equal(s4["x"][half0], s5["x"][half0])
    good.close()
    with pytest.raises(EngineError, match="set a state again") as ei:
        eng.step(1)
    assert ei.value.code == ERR_STATE
    state["fail_at"] = None
    eng.set_full_state(after)
    eng.step(2)
    eng.sync()
    assert int(eng.get_full_state()["step"]) == 6
    eng.close()


def test_the_c_entry_refuses_by_name_and_a_served_shape_runs_after():
    f = lambda p: -((p - 0.5) ** 2).sum(1) * 0.5   # noqa: E731
    d = 4
    kinds, lo, hi = np.zeros(d, np.int32), np.zeros(d), np.ones(d)
    x0 = _x0(128, d)

    def refused(eng, match, code=ERR_ARG, call=None):
        with pytest.raises(EngineError, match=match) as ei:
            (call or (lambda: eng.step(1)))()
        assert ei.value.code == code
        eng.close()

    def gaussian(**kw):
        eng = Engine(d, 128, group_size=64, device=0, seed=2, **kw)
        eng.set_prior(kinds, lo, hi)
        eng.set_target_gaussian(np.full(d, 0.5), 0.01 * np.eye(d))
        eng.set_proposal_cov(0.01 * np.eye(d))
        eng.set_move("stretch", 2.0)
        eng.set_state(x0)
        return eng

    # the option itself
    eng = _small(f, d, move=False)
    refused(eng, "stretch_a > 1, got 1", call=lambda: eng.set_move("stretch", 1.0))
    eng = _small(f, d, move=False)
    refused(eng, "stretch_a > 1, got inf", call=lambda: eng.set_move("stretch", float("inf")))
    eng = _small(f, d, move=False)
    refused(eng, "'metropolis' or 'stretch'", call=lambda: eng.set_move("walk"))
    # targets
    refused(gaussian(), "serves one device_function target")
    refused(gaussian(incremental=True), "MCMC_HIP_FLAG_INCREMENTAL")
    refused(gaussian(emit_capacity=4), "emit_capacity > 0")
    eng = Engine(d, 128, group_size=64, device=0, seed=2)
    eng.set_prior(kinds, lo, hi)
    eng.set_target_functions([f, f], [[0, 1], [0, 1, 2, 3]])
    eng.set_move("stretch", 2.0)
    eng.set_state(x0)
    refused(eng, "several-functions target")
    # blocks, dragging (set after the target: refused by the step)
    eng = _small(f, d)
    eng.set_state(x0)
    eng.set_blocking([[0, 1], [2, 3]], [1, 2])
    refused(eng, "parameter blocks, oversampling and dragging")
    eng = _small(f, d)
    eng.set_state(x0)
    eng.set_blocking([[0, 1], [2, 3]], [1, 1], drag_last_slow=0, drag_steps=2)
    refused(eng, "parameter blocks, oversampling and dragging")
    # periodic parameters: a prior set after the target is refused by the step ...
    eng = _small(f, d)
    eng.set_prior(kinds, lo, hi, np.array([0, 1, 0, 0], np.int32))
    eng.set_state(x0)
    refused(eng, "the stretch move does not serve periodic parameters")
    # ... and one set before it by the target itself, before a move is set
    eng = Engine(d, 128, group_size=64, device=0, seed=2)
    eng.set_prior(kinds, lo, hi, np.array([0, 1, 0, 0], np.int32))
    refused(eng, "periodic parameters", call=lambda: eng.set_target_function(f))
    # group_size < 4 d, with the remedy
    eng = _small(f, 17)
    eng.set_state(_x0(128, 17))
    refused(eng, r"group_size >= 4 d.*use a larger group_size \(256 serves d <= 64\)")
    # a half-group flat in one parameter: walkers 32..63 share the value of parameter 2
    flat = x0.copy()
    flat[32:64, 2] = 0.5
    eng = _small(f, d, walker_offset=256)
    eng.set_state(flat)
    refused(eng, r"parameter 2 has the same value \(0.5\) in every walker of the half-group at walker 288.*"
                 r"give `ref` as a pdf")
    # Metropolis steps still need their covariance; the stretch move does not, and runs after all of these
    eng = _small(f, d, move=False)
    eng.set_state(x0)
    refused(eng, "set_proposal_cov must precede step", code=ERR_STATE)
    eng = _small(f, d)
    eng.set_state(x0)
    eng.step(4)
    eng.sync()
    assert eng.last_step_kernel().startswith(KERNEL) and eng.get_full_state()["n_accept"].sum() > 0
    # ... and back to Metropolis steps on the same engine
    eng.set_move("metropolis")
    eng.set_proposal_cov(0.01 * np.eye(d))
    eng.step(4)
    eng.sync()
    assert eng.last_step_kernel().startswith("mcmc::fn_walker_kernel")
    eng.close()


# ------------------------------------------------------------------------------ 4. the sampler
def banana_info(n_walkers=16384, **opts):
    """The banana of tests/test_gpu_function_target.py with `move: stretch`: the DEFAULT max_tries,
    and `ref` given as pdfs."""
    return {"likelihood": {"banana": {"class": "device_function", "function": banana}},
            "params": {"a": {"prior": {"min": -8, "max": 8}, "ref": {"dist": "norm", "loc": 0, "scale": 1}},
                       "b": {"prior": {"min": -6, "max": 30}, "ref": {"dist": "norm", "loc": 0.5, "scale": 1}}},
            "sampler": {"mcmc_hip": {"n_walkers": n_walkers, "move": "stretch", **opts}}}


def test_posterior_banana_moments_with_the_default_max_tries():
    """16 384 walkers to Rminus1_stop 0.01 without ChainStuck: the final ensemble's means and variances
    within 6 standard errors (of 16 384 independent draws) of the exact values."""
    info = banana_info(16384, seed=11, Rminus1_stop=0.01, max_samples=16384 * 200000)
    _, sampler = run(info)
    assert sampler.converged, sampler.Rminus1_last
    assert sampler.max_tries == 80 and sampler.stretch and not sampler.learn_proposal
    assert sampler.engine.last_step_kernel().startswith(KERNEL)
    rate = sampler._accepted_total / (sampler.n_steps_raw * 16384.0)
    print("steps %d, acceptance %.3f" % (sampler.n_steps_raw, rate))
    assert rate > 0.3
    _check_banana_moments(sampler.engine.get_state()["x"])
    sampler.close()


def test_resume_continues_bit_identically(tmp_path):
    def make(prefix, resume, max_samples, **more):
        opts = {"seed": 21, "n_walkers": 512, "group_size": 64, "steps_per_launch": 40,
                "max_samples": max_samples, "Rminus1_stop": 0.0, "learn_every": "20d", **more}
        info = banana_info(**opts)
        return MCMCHip(info["sampler"]["mcmc_hip"], ProblemSpec.from_info(info), output=prefix, resume=resume)

    a = make(str(tmp_path / "a"), False, 300000)
    a.run()
    ref = a.engine.get_full_state()
    steps_total = a.n_steps_raw
    a.close()
    b1 = make(str(tmp_path / "b"), False, 100000)
    b1.run()
    assert b1.n_steps_raw < steps_total
    b1.close()
    from cobaya_amd.sampler import LoggedError
    with pytest.raises(LoggedError, match="cannot resume -- the run was written with move: stretch"):
        make(str(tmp_path / "b"), True, 300000, move=None, max_tries="2000d")
    b2 = make(str(tmp_path / "b"), True, 300000)
    assert b2.n_steps_raw == b1.n_steps_raw
    b2.run()
    got = b2.engine.get_full_state()
    assert b2.n_steps_raw == steps_total
    for k in ("x", "logpost", "logprior", "loglike", "weight", "n_accept", "burn_left", "prior_rej"):
        assert np.array_equal(got[k], ref[k]), k
    assert int(got["step"]) == int(ref["step"])
    b2.close()


def test_the_six_products_beside_the_move_replay_from_the_stored_snapshots():
    info = products_info("device_function", move="stretch", max_tries="40d", max_samples=1500000)
    _, smp = run(info)
    assert smp.engine.last_step_kernel().startswith(KERNEL)
    assert [p.name for p in smp._products] == list(PRODUCTS)
    assert len(smp._intervals) >= 2
    assert same_as_replayed(smp) == {name: len(smp._intervals) + 1 for name in PRODUCTS}
    smp.close()
