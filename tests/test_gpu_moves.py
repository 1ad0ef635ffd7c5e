"""Mixtures of ensemble moves on the MI355X (ensemble_move_kernels.hip; `moves`, mcmc_hip_set_moves):
every kind alone and a four-member mixture equal their reference (tests/moves_ref.py) bit for bit
by record and replay -- and differ from references with a wrong partner rule --, the stretch member
is `move: stretch` bit for bit, launches split, walker shards compose, the full state round-trips,
step indices beyond 2^32 work, every failure path is an error message, and the sampler finds the
weights of two modes 20 sigma apart."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402

from cobaya_amd import run  # noqa: E402
from cobaya_amd.engine import (ERR_ARG, ERR_CALLBACK, ERR_STATE, ERR_TARGET, Engine,  # noqa: E402
                               EngineError, TargetError)
from cobaya_amd.model import ProblemSpec  # noqa: E402
from cobaya_amd.sampler import LoggedError, MCMCHip  # noqa: E402
from tests import moves_ref as MR  # noqa: E402
from tests.products_together import PRODUCTS, same_as_replayed  # noqa: E402
from tests.test_gpu_products_together import _info as products_info  # noqa: E402

KERNEL = "mcmc::ensemble_move_kernel"
MIX = [["stretch", 1], ["de", 1], ["snooker", 1], ["de", 0.5, {"gamma": 1.0}]]
HOP = [["de", 0.8], ["de", 0.2, {"gamma": 1.0}]]
ALONE = {"stretch": [["stretch", 1.0, {"a": 1.5}]], "de": [["de", 1.0, {"sigma": 0.05}]],
         "snooker": [["snooker", 2.0]], "mix": MIX}


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
    """Uniform on the unit box -- walls the trials of a start spread over it leave --, N(0.5, 0.3^2)
    on every third dimension."""
    kinds = np.array([1 if i % 3 == 1 else 0 for i in range(d)], np.int32)
    return kinds, np.where(kinds == 1, 0.5, 0.0), np.where(kinds == 1, 0.3, 1.0)


def _start(W, d, seed):
    x0 = np.random.default_rng(seed).uniform(0.02, 0.98, (W, d))
    x0[:, 0] *= 0.93 / 0.98     # (below the Recorder's cut)
    return x0


def _pair(d, W, gs, f, moves, seed=7, burn_in=3, temperature=1.0, max_tries=None, walker_offset=0, x0=None,
          flaw=0):
    kinds, pa, pb = _priors(d)
    eng = Engine(d, W, group_size=gs, device=0, seed=seed, burn_in=burn_in, temperature=temperature,
                 max_tries=max_tries, walker_offset=walker_offset)
    eng.set_prior(kinds, pa, pb)
    eng.set_target_function(f)
    eng.set_moves(moves)
    if x0 is None:
        x0 = _start(W, d, seed)
    eng.set_state(x0)           # (no proposal covariance: the moves need none)
    prob = MR.problem(d, kinds, pa, pb, group_size=gs, seed=seed, temperature=temperature,
                      max_tries=max_tries, derived=eng.derived_constants())
    ref = MR.MovesRef(prob, x0, eng.get_state()["loglike"], moves, burn_in=burn_in, walker0=walker_offset,
                      flaw=flaw)
    return eng, ref


def _states_differ(eng, ref):
    """Names of the parts of the full state in which engine and reference differ."""
    st = eng.get_full_state()
    out = [k for k in ("x", "logpost", "logprior", "loglike") if not np.array_equal(_bits(st[k]), _bits(getattr(ref, k)))]
    out += [k for k in ("weight", "prior_rej", "burn_left", "n_accept") if not np.array_equal(st[k], getattr(ref, k))]
    if int(st["step"]) != ref.step:
        out.append("step")
    return out


def _replay(eng, ref, rec, n_steps):
    """Steps the engine, then the reference with the values the device's function returned."""
    rec.calls.clear()
    rec.on = True
    eng.step(n_steps)
    eng.sync()
    rec.on = False
    assert len(rec.calls) == 2 * n_steps
    n_out = 0
    for pts, ll in rec.calls:
        t = ref.propose()
        assert pts.shape == t.shape == (ref.W // 2, ref.d)
        assert np.array_equal(_bits(pts), _bits(t)), (ref.d, ref.step, ref.half, ref.kind)
        n_out += int(np.sum(np.isinf(ref.lp_t)))
        ref.accept(ll)
    return n_out


# ------------------------------------------------------------------------------ 1. bit parity
# (d, gs, G, temperature, walker offset): d = 1; an odd number of 64-groups (the last workgroup holds
# 32 active walkers); d below, just above (four chains, a second tile of one dimension) and twice the tile
SHAPES = [(1, 64, 2, 1.0, 0), (2, 64, 3, 2.0, 128), (30, 128, 2, 1.0, 256), (33, 256, 1, 2.0, 512),
          (64, 256, 2, 1.0, 0)]


@pytest.mark.parametrize("d,gs,G,temperature,offset", SHAPES)
@pytest.mark.parametrize("which", list(ALONE))
def test_step_equals_the_reference_by_record_and_replay(which, d, gs, G, temperature, offset):
    """State, log-values, weights, prior_rej, accept counters and the rows of every call, bit for bit,
    over three uneven launches of 14 steps in all."""
    rec = Recorder()
    eng, ref = _pair(d, G * gs, gs, rec, ALONE[which], temperature=temperature, walker_offset=offset)
    assert _states_differ(eng, ref) == []
    n_out = 0
    for n in (5, 1, 8):
        n_out += _replay(eng, ref, rec, n)
        assert _states_differ(eng, ref) == []
    n_trials = 14 * G * gs
    print("%s d = %d: %.3f of the trials left the support, acceptance %.3f, kinds %s" % (
        which, d, n_out / n_trials, ref.n_accept.sum() / n_trials, ref.kinds_made[0::2]))
    assert eng.last_step_kernel().startswith(KERNEL)
    assert ref.n_accept.sum() > 0 and ref.stuck[0] == 0
    assert n_out > 0 and ref.prior_rej.sum() > 0
    assert eng.counters()["accepted"] == int(ref.n_accept.sum()) and eng.counters()["steps"] == 14
    if which == "mix":
        made = ref.kinds_made[0::2]
        assert set(made) == {0, 1, 2}
        # a launch accepts one kind while it proposes another: the kind changes between two steps
        assert sum(a != b for a, b in zip(made, made[1:])) >= 3
    eng.close()


@pytest.mark.parametrize("which,flaw,d,gs", [("de", 1, 2, 64), ("de", 1, 33, 256), ("snooker", 2, 2, 64),
                                             ("snooker", 2, 33, 256)])
def test_the_replay_fails_against_a_wrong_partner_rule(which, flaw, d, gs):
    """The power of the replay: DE whose second partner is drawn without the + 1 shift (p1 = p2 is
    allowed), and snooker with z and z1 exchanged, are different chains; the device must be the
    right one, and not these."""
    rec = Recorder()
    eng, right = _pair(d, 2 * gs, gs, rec, ALONE[which])
    spare, wrong = _pair(d, 2 * gs, gs, rec, ALONE[which], flaw=flaw)
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


# ------------------------------------------------------------------------------ 2. the stretch member
def _smooth(p):
    q = p - 0.45
    return -(q * q).sum(1) * 2.0


def _same_full_state(a, b, lo=0, hi=None):
    for k in ("x", "logpost", "logprior", "loglike"):
        assert np.array_equal(_bits(a[k][lo:hi]), _bits(b[k])), k
    for k in ("weight", "prior_rej", "burn_left", "n_accept"):
        assert np.array_equal(a[k][lo:hi], b[k]), k


@pytest.mark.parametrize("d,gs", [(2, 64), (40, 256)])
def test_a_stretch_mixture_is_move_stretch_bit_for_bit(d, gs):
    """`moves: [["stretch", 1.0, {"a": 2.0}]]` draws from the stretch stream unchanged."""
    W = 2 * gs
    rec_a, rec_b = Recorder(), Recorder()
    mixed, _ = _pair(d, W, gs, rec_a, [["stretch", 1.0, {"a": 2.0}]])
    kinds, pa, pb = _priors(d)
    plain = Engine(d, W, group_size=gs, device=0, seed=7, burn_in=3)
    plain.set_prior(kinds, pa, pb)
    plain.set_target_function(rec_b)
    plain.set_move("stretch", 2.0)
    plain.set_state(_start(W, d, 7))
    rec_a.on = rec_b.on = True
    for e in (mixed, plain):
        e.step(6)
        e.sync()
    assert mixed.last_step_kernel().startswith(KERNEL)
    assert plain.last_step_kernel().startswith("mcmc::stretch_kernel")
    assert len(rec_a.calls) == len(rec_b.calls) == 12
    for (pa_, la), (pb_, lb) in zip(rec_a.calls, rec_b.calls):
        assert np.array_equal(_bits(pa_), _bits(pb_)) and np.array_equal(_bits(la), _bits(lb))
    a, b = mixed.get_full_state(), plain.get_full_state()
    assert a["n_accept"].sum() > 0 and a["prior_rej"].sum() > 0
    _same_full_state(a, b)
    mixed.close()
    plain.close()


# ------------------------------------------------------------------------------ 3. launches, shards, state
@pytest.mark.parametrize("d,gs", [(3, 64), (40, 256)])
def test_one_call_of_2n_steps_equals_2n_calls_of_one(d, gs):
    one, _ = _pair(d, 2 * gs, gs, _smooth, MIX)
    many, _ = _pair(d, 2 * gs, gs, _smooth, MIX)
    one.step(8)
    for _ in range(8):
        many.step(1)
    one.sync()
    many.sync()
    a, b = one.get_full_state(), many.get_full_state()
    assert a["n_accept"].sum() > 0 and int(a["step"]) == int(b["step"]) == 8
    _same_full_state(a, b)
    one.close()
    many.close()


@pytest.mark.parametrize("d,gs", [(2, 64), (40, 256)])
def test_walker_shards_compose(d, gs):
    """Two engines with walker_offset 0 and W / 2 equal the halves of one: partners never leave the
    group, and the kind of a step is the same for every shard."""
    W = 4 * gs
    whole, ref = _pair(d, W, gs, _smooth, MIX, seed=9)
    x0 = ref.x.copy()
    halves = [_pair(d, W // 2, gs, _smooth, MIX, seed=9, walker_offset=o, x0=x0[o:o + W // 2])[0] for o in (0, W // 2)]
    for n in (3, 5):
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
    eng, ref = _pair(5, 256, 64, rec, MIX, seed=4)
    _replay(eng, ref, rec, 4)
    st = eng.get_full_state()
    other, _ = _pair(5, 256, 64, rec, MIX, seed=4)
    other.set_full_state(st)
    for e in (eng, other):
        e.step(6)
        e.sync()
    a, b = eng.get_full_state(), other.get_full_state()
    _same_full_state(a, b)
    assert int(a["step"]) == int(b["step"]) == 10 and a["n_accept"].sum() > st["n_accept"].sum()
    eng.close()
    other.close()


def test_replay_across_step_2_to_the_32():
    """The step enters the Philox counters -- the kind's and the walkers' -- as two words: a replay
    from 2^32 - 2 crosses the carry."""
    rec = Recorder()
    eng, ref = _pair(3, 128, 64, rec, MIX, seed=5)
    _replay(eng, ref, rec, 2)
    fs = eng.get_full_state()
    fs["step"] = np.uint64((1 << 32) - 2)
    eng.set_full_state(fs)
    ref.step = (1 << 32) - 2
    _replay(eng, ref, rec, 6)
    assert _states_differ(eng, ref) == [] and ref.step == (1 << 32) + 4
    # ... and the trials there are not those of the low word alone: the same state at step 4
    fs = eng.get_full_state()
    low, _ = _pair(3, 128, 64, rec, MIX, seed=5)
    low.set_full_state(dict(fs, step=np.uint64(4)))
    for e in (eng, low):
        e.step(1)
        e.sync()
    assert not np.array_equal(_bits(low.get_full_state()["x"]), _bits(eng.get_full_state()["x"]))
    eng.close()
    low.close()


# ------------------------------------------------------------------------------ 4. failure paths
def _small(f, d=2, W=128, gs=64, moves=MIX, box=(0.0, 1.0), **kw):
    eng = Engine(d, W, group_size=gs, device=0, seed=2, **kw)
    eng.set_prior(np.zeros(d, np.int32), np.full(d, box[0]), np.full(d, box[1]))
    eng.set_target_function(f)
    if moves:
        eng.set_moves(moves)
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
    with pytest.raises(EngineError, match="an ensemble-move step: set a state again") as ei:
        eng.step(1)
    assert ei.value.code == ERR_STATE
    state["fail_at"] = None
    eng.set_full_state(after)
    eng.step(2)
    eng.sync()
    assert int(eng.get_full_state()["step"]) == 6
    eng.close()


def test_the_c_entry_refuses_by_name_and_a_served_shape_runs_after():
    import ctypes as C
    f = lambda p: -((p - 0.5) ** 2).sum(1) * 0.5   # noqa: E731
    d = 4
    kinds, lo, hi = np.zeros(d, np.int32), np.zeros(d), np.ones(d)
    x0 = _x0(128, d)

    def refused(eng, match, code=ERR_ARG, call=None):
        with pytest.raises(EngineError, match=match) as ei:
            (call or (lambda: eng.step(1)))()
        assert ei.value.code == code

    def raw(eng, kinds_, weights, p0, p1, n=None):
        """mcmc_hip_set_moves itself, past the checks of Engine.set_moves."""
        k, w = np.array(kinds_, np.int32), np.array(weights, np.float64)
        a, b = np.array(p0, np.float64), np.array(p1, np.float64)
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
        eng._check(eng._lib.mcmc_hip_set_moves(eng._h, len(k) if n is None else n, k.ctypes.data_as(ip),
                                               w.ctypes.data_as(dp), a.ctypes.data_as(dp), b.ctypes.data_as(dp)))

    # the option itself: Engine.set_moves and the C entry each name the offender
    eng = _small(f, d, moves=None)
    refused(eng, r"moves\[0\]: unknown kind 'walk'", call=lambda: eng.set_moves([["walk", 1]]))
    refused(eng, r"moves\[1\] \(de\): the weight must be positive", call=lambda: eng.set_moves([["de", 1], ["de", 0]]))
    refused(eng, r"1 \.\. 8 members \(0: off\), got n=9", call=lambda: raw(eng, [1] * 9, [1] * 9, [1] * 9, [0] * 9))
    refused(eng, r"got n=-1", call=lambda: raw(eng, [1], [1], [1], [0], n=-1))
    refused(eng, r"member 1 of the mixture: the kind must be .*got 3", call=lambda: raw(eng, [1, 3], [1, 1], [1, 1], [0, 0]))
    for w in (0.0, -1.0, float("inf"), float("nan")):
        refused(eng, r"member 0 of the mixture: the weight must be positive and finite",
                call=lambda: raw(eng, [1], [w], [1], [0]))
    refused(eng, r"member 0 of the mixture \(stretch\): needs a finite a > 1, got 1", call=lambda: raw(eng, [0], [1], [1.0], [0]))
    for g in (0.0, -2.0, float("inf"), float("nan")):
        refused(eng, r"member 0 of the mixture \(de\): needs a finite gamma > 0", call=lambda: raw(eng, [1], [1], [g], [0]))
        refused(eng, r"member 1 of the mixture \(snooker\): needs a finite gamma > 0",
                call=lambda: raw(eng, [1, 2], [1, 1], [1, g], [0, 0]))
    refused(eng, r"member 0 of the mixture \(de\): needs a finite sigma >= 0, got -0.5",
            call=lambda: raw(eng, [1], [1], [1], [-0.5]))
    # (nothing of the refused calls is in force: Metropolis steps still want their covariance)
    eng.set_state(x0)
    refused(eng, "set_proposal_cov must precede step", code=ERR_STATE)
    # a mixture and move: stretch together
    eng.set_moves(MIX)
    eng.set_move("stretch", 2.0)
    refused(eng, "mcmc_hip_set_moves and mcmc_hip_set_move.* are both in force")
    eng.close()

    # the limits of the stretch move, in C
    def gaussian(**kw):
        eng = Engine(d, 128, group_size=64, device=0, seed=2, **kw)
        eng.set_prior(kinds, lo, hi)
        eng.set_target_gaussian(np.full(d, 0.5), 0.01 * np.eye(d))
        eng.set_proposal_cov(0.01 * np.eye(d))
        eng.set_moves(MIX)
        eng.set_state(x0)
        return eng

    for eng, match in ((gaussian(), "a mixture of ensemble moves serves one device_function target"),
                       (gaussian(incremental=True), "MCMC_HIP_FLAG_INCREMENTAL"),
                       (gaussian(emit_capacity=4), "emit_capacity > 0")):
        refused(eng, match)
        eng.close()
    eng = Engine(d, 128, group_size=64, device=0, seed=2)
    eng.set_prior(kinds, lo, hi)
    eng.set_target_functions([f, f], [[0, 1], [0, 1, 2, 3]])
    eng.set_moves(MIX)
    eng.set_state(x0)
    refused(eng, "several-functions target")
    eng.close()
    eng = _small(f, d)
    eng.set_state(x0)
    eng.set_blocking([[0, 1], [2, 3]], [1, 2])
    refused(eng, "a mixture of ensemble moves moves all parameters at once")
    eng.close()
    eng = _small(f, d)
    eng.set_prior(kinds, lo, hi, np.array([0, 1, 0, 0], np.int32))
    eng.set_state(x0)
    refused(eng, "a mixture of ensemble moves does not serve periodic parameters")
    eng.close()
    eng = _small(f, 17)
    eng.set_state(_x0(128, 17))
    refused(eng, r"a mixture of ensemble moves needs group_size >= 4 d.*use a larger group_size \(256 serves d <= 64\)")
    eng.close()
    flat = x0.copy()
    flat[32:64, 2] = 0.5
    eng = _small(f, d, walker_offset=256)
    eng.set_state(flat)
    refused(eng, r"a mixture of ensemble moves cannot start here: parameter 2 has the same value \(0.5\) in every "
                 r"walker of the half-group at walker 288.*give `ref` as a pdf")
    eng.close()
    # a served shape runs after all of these ...
    eng = _small(f, d)
    eng.set_state(x0)
    eng.step(6)
    eng.sync()
    assert eng.last_step_kernel().startswith(KERNEL) and eng.get_full_state()["n_accept"].sum() > 0
    # ... n = 0 switches the mixture off: back to Metropolis steps on the same engine
    eng.set_moves(None)
    eng.set_proposal_cov(0.01 * np.eye(d))
    eng.step(4)
    eng.sync()
    assert eng.last_step_kernel().startswith("mcmc::fn_walker_kernel")
    eng.close()


# ------------------------------------------------------------------------------ 5. the sampler
X0, W_HEAVY = 10.0, 0.7
LOG_LIGHT, LOG_HEAVY = float(np.log(1 - W_HEAVY)), float(np.log(W_HEAVY))


def two_modes(p):
    """Two unit Gaussians at a = -10 (weight 0.3) and a = +10 (weight 0.7)."""
    r2 = p[:, 1] ** 2
    return torch.logaddexp(LOG_LIGHT - 0.5 * ((p[:, 0] + X0) ** 2 + r2), LOG_HEAVY - 0.5 * ((p[:, 0] - X0) ** 2 + r2))


def two_modes_info(n_walkers=4096, **opts):
    """The README's bimodal posterior: the start (`ref`) spans both modes."""
    return {"likelihood": {"two_modes": {"class": "device_function", "function": two_modes}},
            "params": {"a": {"prior": {"min": -40, "max": 40}, "ref": {"dist": "norm", "loc": 0, "scale": 5}},
                       "b": {"prior": {"min": -40, "max": 40}, "ref": {"dist": "norm", "loc": 0, "scale": 1}}},
            "sampler": {"mcmc_hip": {"n_walkers": n_walkers, "group_size": 64, "moves": HOP, "max_tries": "400d",
                                     **opts}}}


def _group_checks(x, gs):
    """(name, got, want, standard error) of the occupancy of the heavy mode and of each mode's means
    and variances (about the known means: unbiased whatever the correlation inside a group); the
    standard errors are those of the mean over the groups, measured from their spread."""
    G = len(x) // gs
    xg = x.reshape(G, gs, 2)
    heavy = xg[:, :, 0] > 0

    def over_groups(name, per_group, want):
        per_group = np.asarray(per_group)
        return name, per_group.mean(), want, per_group.std(ddof=1) / np.sqrt(G)

    out = [over_groups("occupancy", heavy.mean(1), W_HEAVY)]
    for mode, sel, centre in (("heavy", heavy, X0), ("light", ~heavy, -X0)):
        n = np.maximum(sel.sum(1), 1)
        da, b = xg[:, :, 0] - centre, xg[:, :, 1]
        out.append(over_groups("E a | " + mode, (da * sel).sum(1) / n + centre, centre))
        out.append(over_groups("E b | " + mode, (b * sel).sum(1) / n, 0.0))
        out.append(over_groups("Var a | " + mode, (da ** 2 * sel).sum(1) / n, 1.0))
        out.append(over_groups("Var b | " + mode, (b ** 2 * sel).sum(1) / n, 1.0))
    return out


def test_the_sampler_finds_the_weights_of_two_modes():
    """4 096 walkers to the default Rminus1_stop: the final ensemble's occupancy of the heavy mode
    and the means and variances of each mode within 6 of their measured standard errors."""
    info = two_modes_info(4096, seed=11, max_samples=4096 * 100000)
    _, sampler = run(info)
    assert sampler.converged, sampler.Rminus1_last
    assert sampler.mixture and not sampler.stretch and not sampler.learn_proposal
    assert sampler.engine.last_step_kernel().startswith(KERNEL)
    rate = sampler._accepted_total / (sampler.n_steps_raw * 4096.0)
    checks = _group_checks(sampler.engine.get_state()["x"], 64)
    print("steps %d, acceptance %.3f" % (sampler.n_steps_raw, rate))
    for name, got, want, se in checks:
        print("%s: got %.5f want %.5f  (%.2f standard errors of %.5f)" % (name, got, want, (got - want) / se, se))
    assert rate > 0.1
    for name, got, want, se in checks:
        assert abs(got - want) < 6 * se, (name, got, want, se)
    assert checks[0][3] < 0.012      # (about 0.007: the check has power against 0.5)
    sampler.close()


def test_resume_continues_bit_identically(tmp_path):
    def make(prefix, resume, max_samples, **more):
        opts = {"seed": 21, "n_walkers": 512, "steps_per_launch": 40, "max_samples": max_samples,
                "Rminus1_stop": 0.0, "learn_every": "20d", **more}
        info = two_modes_info(**opts)
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
    with pytest.raises(LoggedError, match=r"cannot resume -- the run was written with moves: \[de 0.8 .*\] and now "
                                          r"has moves: \[de 1 "):
        make(str(tmp_path / "b"), True, 300000, moves=[["de", 1.0]])
    b2 = make(str(tmp_path / "b"), True, 300000)
    assert b2.n_steps_raw == b1.n_steps_raw
    b2.run()
    got = b2.engine.get_full_state()
    assert b2.n_steps_raw == steps_total
    for k in ("x", "logpost", "logprior", "loglike", "weight", "n_accept", "burn_left", "prior_rej"):
        assert np.array_equal(got[k], ref[k]), k
    assert int(got["step"]) == int(ref["step"])
    b2.close()


def test_the_six_products_beside_a_mixture_replay_from_the_stored_snapshots():
    info = products_info("device_function", moves=[["de", 1], ["snooker", 1], ["stretch", 1]], max_tries="40d",
                         max_samples=1500000)
    _, smp = run(info)
    assert smp.engine.last_step_kernel().startswith(KERNEL)
    assert [p.name for p in smp._products] == list(PRODUCTS)
    assert len(smp._intervals) >= 2
    assert same_as_replayed(smp) == {name: len(smp._intervals) + 1 for name in PRODUCTS}
    smp.close()
