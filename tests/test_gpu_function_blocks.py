"""Several `device_function` likelihoods over parameter blocks on the MI355X
(fn_blocked_walker_kernel, mcmc_hip_set_target_functions): the step equals its reference
(tests/function_blocks_ref.py) bit for bit by record and replay -- state, log-values, weights, the
carried ll_c and the accept counters --, every function is called exactly once per due slot, launches
and walker shards compose, failures are error messages, and the sampler resumes in mid-cycle, fills
the chi2 columns, runs its device products and finds exact moments."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402

from cobaya_amd import run  # noqa: E402
from cobaya_amd.engine import ERR_CALLBACK, Engine, EngineError, TargetError  # noqa: E402
from cobaya_amd.model import ProblemSpec  # noqa: E402
from cobaya_amd.sampler import MCMCHip  # noqa: E402
from tests import function_blocks_ref as FB  # noqa: E402

KERNEL = "mcmc::fn_blocked_walker_kernel"


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


class Recorder:
    """A separable Gaussian bowl of its inputs; NaN where its first input is outside [0, 1] when
    `nan_outside` (rows outside the prior support: ignored); -inf where its first input is above
    `cut`.  Counts its calls and records, while `on`, (inputs, values) copied to the host."""

    def __init__(self, centre, cut=None, nan_outside=False):
        self.centre, self.cut, self.nan_outside = centre, cut, nan_outside
        self.on, self.calls, self.n_calls, self.fail_at = False, [], 0, None

    def __call__(self, p):
        self.n_calls += 1
        if self.n_calls == self.fail_at:
            raise RuntimeError("boom")
        ll = -0.5 * (((p - self.centre) / 0.2) ** 2).sum(1)
        if self.cut is not None:
            ll = torch.where(p[:, 0] > self.cut, torch.full_like(ll, -float("inf")), ll)
        if self.nan_outside:
            ll = torch.where((p[:, 0] < 0) | (p[:, 0] > 1), torch.full_like(ll, float("nan")), ll)
        if self.on:
            self.calls.append((p.cpu().numpy().copy(), ll.cpu().numpy().copy()))
        return ll


def _problem(d, seed, cov_scale=1.0, all_uniform=False):
    rng = np.random.default_rng(seed)
    kinds = np.array([0 if all_uniform else (1 if i % 3 == 1 else 0) for i in range(d)], np.int32)
    a = np.where(kinds == 1, 0.5, 0.0)
    b = np.where(kinds == 1, 0.3, 1.0)
    A = rng.standard_normal((d, d)) / np.sqrt(d)
    cov = 0.01 * cov_scale * (A @ A.T + np.eye(d))
    return kinds, a, b, cov, rng


# name: (d, W, group size, blocks (sampler indices, slow -> fast), factors, inputs of the functions,
#        proposal scale, which functions return NaN outside [0, 1])
LAYOUTS = {
    # blocks 1 + 2, factors 1 and 3, two groups: group 1's own schedule differs from the shared one
    "d3": (3, 128, 64, [[1], [2, 0]], [1, 3], [[1], [1, 0, 2]], 1.0, ()),
    # three blocks 2 + 1 + 2, overlapping footprints, a one-parameter block, normal priors; wide
    # proposal: about a third of the trials leave the box, where the functions return NaN
    "d5": (5, 128, 64, [[3, 0], [2], [4, 1]], [1, 2, 3], [[0, 3], [3, 2, 0], [1, 4, 2]], 60.0, (0, 1)),
    # blocks 33 + 7: the d > 32 direction kernel, the four-chain log-prior, a tile boundary
    "d40": (40, 128, 64, [list(range(7, 40)), list(range(7))], [1, 2],
            [list(range(7, 40)), list(range(39, -1, -1)), [3, 5]], 1.0, ()),
    # no blocks at all: two overlapping functions, both due at every slot, the plain Haar columns
    "d2-one-block": (2, 128, 64, None, None, [[1, 0], [1]], 1.0, ()),
    # d = 1 without blocks: the RandProposer1D variates come from d itself, two functions of the one parameter
    "d1": (1, 128, 64, None, None, [[0], [0]], 1.0, ()),
    # blocks 64 + 64 with factor 1, one group
    "d128": (128, 64, 64, [list(range(64, 128)), list(range(64))], [1, 1],
             [list(range(64, 128)), list(range(128))], 1.0, ()),
}


def _pair(name, seed=7, burn_in=3, temperature=1.5, walker_offset=0, x0=None, W=None, fns=None,
          max_tries=None):
    d, W0, gs, blocks, over, inputs, scale, nan_fns = LAYOUTS[name]
    W = W or W0
    kinds, a, b, cov, rng = _problem(d, seed, cov_scale=scale)
    if fns is None:
        fns = [Recorder(0.4 + 0.05 * c, cut=0.6 if c == 0 else None, nan_outside=c in nan_fns)
               for c in range(len(inputs))]
    eng = Engine(d, W, group_size=gs, device=0, seed=seed, burn_in=burn_in, temperature=temperature,
                 walker_offset=walker_offset, max_tries=max_tries)
    eng.set_prior(kinds, a, b)
    eng.set_target_functions(fns, inputs)
    if blocks is not None:
        eng.set_blocking(blocks, over)
    eng.set_proposal_cov(cov)
    if x0 is None:
        x0 = np.clip(0.45 + 0.3 * rng.standard_normal((W, d)) * np.sqrt(np.diag(cov) / scale), 0.01, 0.55)
        x0[::4, inputs[0][0]] = 0.001      # against a lower bound (where the parameter is uniform)
        x0[1::4, inputs[0][0]] = 0.5999    # ... and just below function 0's cut (-inf above it)
    eng.set_state(x0)
    prob = FB.problem(d, kinds, a, b, eng.get_proposal_transform(), blocks=blocks, oversampling=over,
                      group_size=gs, seed=seed, temperature=temperature, max_tries=max_tries,
                      derived=eng.derived_constants())
    ref = FB.FunctionBlocksRef(prob, x0, inputs, eng.get_component_loglikes(), blocks=blocks,
                               burn_in=burn_in, walker0=walker_offset)
    return eng, ref, fns


def _assert_states_equal(eng, ref):
    st = eng.get_full_state()
    assert np.array_equal(_bits(st["x"]), _bits(ref.x))
    for k in ("logpost", "logprior", "loglike", "ll_c"):
        assert np.array_equal(_bits(st[k]), _bits(getattr(ref, k))), k
    for k in ("weight", "prior_rej", "burn_left", "n_accept"):
        assert np.array_equal(st[k], getattr(ref, k)), k
    assert int(st["step"]) == ref.step
    return st


def _replay(eng, ref, fns, n):
    """n steps on the engine, then the reference through the same slots with the values the
    functions returned on the device; the inputs each due function was given equal the
    reference's, bit for bit, and no other function was called."""
    for f in fns:
        f.on = True
        f.calls.clear()
    eng.step(n)
    eng.sync()
    taken = [0] * len(fns)
    outside = 0
    for _ in range(n):
        ref.propose()
        outside += int(np.sum(np.isinf(ref.lp_t)))
        new = {}
        for c in ref.due:
            pts, ll = fns[c].calls[taken[c]]
            taken[c] += 1
            assert np.array_equal(_bits(pts), _bits(ref.gather(c))), (c, ref.step)
            new[c] = ll
        ref.accept(new)
    assert taken == [len(f.calls) for f in fns]      # exactly once per due slot, never else
    for f in fns:
        f.on = False
    return outside


# ------------------------------------------------------------------------------ 1. bit parity
@pytest.mark.parametrize("name", list(LAYOUTS))
def test_step_equals_the_reference_by_record_and_replay(name):
    eng, ref, fns = _pair(name)
    W = ref.W
    L = ref.p.cycle_length()
    assert eng.cycle_length() == L
    if name == "d3":   # group 1's own schedule is not the shared one
        assert any(not np.array_equal(ref.p.schedule(0, c)[0], ref.p.schedule(1, c)[0]) for c in range(2))
    _assert_states_equal(eng, ref)
    assert [f.n_calls for f in fns] == [1] * len(fns)   # the initial state: every function once
    outside = 0
    for n in (L + 3, 1, L + 2):                      # three uneven launches, more than two cycles
        outside += _replay(eng, ref, fns, n)
        _assert_states_equal(eng, ref)
    n_steps = 2 * L + 6
    assert eng.last_step_kernel().startswith(KERNEL), eng.last_step_kernel()
    assert [f.n_calls - 1 for f in fns] == ref.calls  # counted on both sides
    assert max(ref.calls) == n_steps
    assert (min(ref.calls) < n_steps) == (ref.blocks is not None)   # a function was spared on fast slots
    assert ref.n_accept.sum() > 0 and (ref.weight > 1).any()
    assert eng.counters()["accepted"] == int(ref.n_accept.sum())
    if name == "d5":   # about a third of the trials outside the box, NaN there, and a 1-D block
        frac = outside / (n_steps * W)
        assert 0.15 < frac < 0.6, frac
        assert any(len(b) == 1 for b in ref.blocks)
    eng.close()


def test_calls_per_function_are_exactly_the_due_slots():
    """Over two whole cycles function c is called at the slots of the blocks up to its last one."""
    eng, ref, fns = _pair("d5")
    L = ref.p.cycle_length()
    assert L == 2 * 1 + 1 * 2 + 2 * 3
    eng.step(2 * L)
    eng.sync()
    # inputs end in block 0, 1, 2: slots of block 0 | blocks 0-1 | all
    assert [f.n_calls - 1 for f in fns] == [2 * 2, 2 * (2 + 2), 2 * L]
    eng.close()


def test_one_call_of_2L_steps_equals_2L_calls_of_one_step():
    a, ref, _ = _pair("d5")
    b, _, _ = _pair("d5", x0=ref.x.copy())
    L = ref.p.cycle_length()
    a.step(2 * L)
    a.sync()
    for _ in range(2 * L):
        b.step(1)
    b.sync()
    sa, sb = a.get_full_state(), b.get_full_state()
    assert sa["n_accept"].sum() > 0
    for k in ("x", "logpost", "logprior", "loglike", "ll_c"):
        assert np.array_equal(_bits(sa[k]), _bits(sb[k])), k
    for k in ("weight", "prior_rej", "burn_left", "n_accept", "step"):
        assert np.array_equal(sa[k], sb[k]), k
    a.close()
    b.close()


@pytest.mark.parametrize("name", ["d3", "d40"])
def test_walker_shards_compose(name):
    """Two engines with walker_offset 0 and W / 2 equal the halves of one: the schedule is the one
    of GLOBAL group 0 on every shard."""
    def fns():
        return [lambda p, c=c: -(((p - 0.4 - 0.05 * c) ** 2).sum(1)) * 12.5 for c in range(3)]

    n_fn = len(LAYOUTS[name][5])
    W = 256
    whole, ref, _ = _pair(name, seed=9, W=W, fns=fns()[:n_fn])
    x0 = ref.x.copy()
    halves = [_pair(name, seed=9, W=W // 2, walker_offset=o, x0=x0[o:o + W // 2], fns=fns()[:n_fn])[0]
              for o in (0, W // 2)]
    L = ref.p.cycle_length()
    for n in (L + 2, L + 1):
        for e in [whole] + halves:
            e.step(n)
            e.sync()
    st = whole.get_full_state()
    assert st["n_accept"].sum() > 0
    for o, e in zip((0, W // 2), halves):
        sh = e.get_full_state()
        for k in ("x", "logpost", "logprior", "loglike"):
            assert np.array_equal(_bits(sh[k]), _bits(st[k][o:o + W // 2])), k
        assert np.array_equal(_bits(sh["ll_c"]), _bits(st["ll_c"][:, o:o + W // 2]))
        for k in ("weight", "prior_rej", "burn_left", "n_accept"):
            assert np.array_equal(sh[k], st[k][o:o + W // 2]), k
        e.close()
    whole.close()


def test_full_state_round_trip_and_a_state_without_ll_c():
    """set_full_state with ll_c resumes bit-identically in mid-cycle; without it every function is
    called on the state at the next launch, and the run is the same."""
    a, ref, _ = _pair("d5")
    L = ref.p.cycle_length()
    a.step(L + 3)
    a.sync()
    st = a.get_full_state()
    b, _, fb = _pair("d5", x0=ref.x.copy())
    c, _, fc = _pair("d5", x0=ref.x.copy())
    b.set_full_state(st)
    c.set_full_state({k: v for k, v in st.items() if k != "ll_c"})
    calls_b, calls_c = [f.n_calls for f in fb], [f.n_calls for f in fc]
    for e in (a, b, c):
        e.step(L + 1)
        e.sync()
    sa = a.get_full_state()
    for e in (b, c):
        se = e.get_full_state()
        for k in sa:
            same = _bits if np.asarray(sa[k]).dtype == np.float64 else np.asarray
            assert np.array_equal(same(sa[k]), same(se[k])), k
    # c formed its components again: one more call of every function than b
    assert [f.n_calls - n for f, n in zip(fc, calls_c)] == [f.n_calls - n + 1 for f, n in zip(fb, calls_b)]
    for e in (a, b, c):
        e.close()


# ------------------------------------------------------------------------------ 2. failures
def test_nan_inside_the_support_from_a_due_function_names_the_walker():
    d, W, gs = 3, 128, 64
    kinds, a, b, cov, rng = _problem(d, 5, all_uniform=True)
    x0 = np.full((W, d), 0.5) + 0.01 * rng.standard_normal((W, d))
    state = {"arm": False}

    def good(p):
        return -0.5 * ((p - 0.5) ** 2).sum(1)

    def bad(p):
        ll = good(p)
        if state["arm"]:
            ll = ll.clone()
            ll[77] = float("nan")
        return ll

    eng = Engine(d, W, group_size=gs, device=0, seed=5)
    eng.set_prior(kinds, a, b)
    eng.set_target_functions([good, bad], [[0, 1], [1, 2]])
    eng.set_blocking([[0], [1, 2]], [1, 2])
    eng.set_proposal_cov(cov * 1e-4)         # tiny steps: every trial inside the support
    eng.set_state(x0)
    eng.step(3)
    eng.sync()
    state["arm"] = True
    eng.step(1)                               # function 1 is due at every slot
    with pytest.raises(TargetError, match=r"NaN or \+inf inside the prior support \(walker 77\)"):
        eng.sync()
    eng.close()


def test_a_failing_callback_leaves_the_last_completed_step():
    eng, ref, fns = _pair("d3")
    L = ref.p.cycle_length()
    eng.step(L + 1)
    eng.sync()
    st = eng.get_full_state()
    fns[1].fail_at = fns[1].n_calls + 2          # the second call from here (function 1 is always due)
    with pytest.raises(EngineError, match="boom") as ei:
        eng.step(5)
    assert ei.value.code == ERR_CALLBACK
    fns[1].fail_at = None
    eng.sync()
    s2 = eng.get_full_state()
    assert int(s2["step"]) == int(st["step"]) + 1    # the step before the failing one completed
    # ... and the engine goes on from there exactly as if nothing had happened
    ref_eng, _, _ = _pair("d3", x0=ref.x.copy())
    ref_eng.step(L + 1 + 1 + 4)
    ref_eng.sync()
    eng.step(4)
    eng.sync()
    sa, sb = eng.get_full_state(), ref_eng.get_full_state()
    for k in ("x", "logpost", "loglike", "ll_c"):
        assert np.array_equal(_bits(sa[k]), _bits(sb[k])), k
    assert np.array_equal(sa["weight"], sb["weight"]) and int(sa["step"]) == int(sb["step"])
    eng.close()
    ref_eng.close()


def test_the_c_entry_refuses_by_name():
    d, W = 3, 64
    eng = Engine(d, W, group_size=64, device=0, seed=1)
    eng.set_prior([0] * d, [0.0] * d, [1.0] * d)
    f = lambda p: p.sum(1)   # noqa: E731
    with pytest.raises(EngineError, match="feeds no function"):
        eng.set_target_functions([f, f], [[0], [1]])
    with pytest.raises(EngineError, match="1..8 functions"):
        eng.set_target_functions([f] * 9, [[0, 1, 2]] * 9)
    with pytest.raises(EngineError, match="not a sampled parameter"):
        eng.set_target_functions([f], [[0, 1, 3]])
    eng.set_target_functions([f, f], [[0, 1], [1, 2]])
    eng.set_blocking([[0], [1, 2]], [1, 2], 0, 2)          # dragging
    eng.set_proposal_cov(np.eye(d) * 0.01)
    eng.set_state(np.full((W, d), 0.5))
    with pytest.raises(EngineError, match="dragging is not served"):
        eng.step(1)
    # the singular entry with blocks stays refused as it was
    eng.set_blocking([[0], [1, 2]], [1, 2])
    with pytest.raises(EngineError, match="one parameter block"):
        eng.set_target_function(f)
    eng.close()


# ------------------------------------------------------------------------------ 3. the sampler
def slow_ab(p):      # N(0, C) in (a, b)
    return -0.5 * (p[:, 0] ** 2 + ((p[:, 1] - 0.5 * p[:, 0]) / 0.8) ** 2)


def fast_bce(p):     # Gaussians that tie b to c and e
    return -0.5 * (((p[:, 1] - p[:, 0]) / 0.7) ** 2 + ((p[:, 2] + 0.5 * p[:, 0]) / 1.1) ** 2
                   + (p[:, 1] / 1.5) ** 2 + (p[:, 2] / 1.3) ** 2)


NAMES = ["a", "b", "c", "e"]
# -2 log of the product = x^T P x: the exact joint precision
_P = np.zeros((4, 4))
for _v, _s in (((1, 0, 0, 0), 1.0), ((-0.5, 1, 0, 0), 0.8), ((0, -1, 1, 0), 0.7), ((0, 0.5, 0, 1), 1.1),
               ((0, 0, 1, 0), 1.5), ((0, 0, 0, 1), 1.3)):
    _P += np.outer(_v, _v) / _s ** 2
EXACT_COV = np.linalg.inv(_P)


def two_function_info(n_walkers, output=None, **opts):
    info = {"likelihood": {"slow": {"class": "device_function", "function": slow_ab, "speed": 1,
                                    "input_params": ["a", "b"]},
                           "fast": {"class": "device_function", "function": fast_bce, "speed": 50,
                                    "input_params": ["b", "c", "e"]}},
            "params": {p: {"prior": {"min": -12, "max": 12}, "ref": {"dist": "norm", "loc": 0, "scale": 0.5},
                           "proposal": 1} for p in NAMES},
            "sampler": {"mcmc_hip": {"n_walkers": n_walkers, "group_size": 64, "oversample_power": 0.4,
                                     **opts}}}
    if output:
        info["output"] = output
    return info


def test_run_fills_the_chi2_columns_from_the_functions():
    info = two_function_info(256, seed=3, max_samples=256 * 60, Rminus1_stop=0.0)
    updated, sampler = run(info)
    assert sampler.engine.last_step_kernel().startswith(KERNEL), sampler.engine.last_step_kernel()
    assert [len(b) for b in sampler.blocks] == [1, 1, 2] and sampler.oversampling_factors[-1] > 1
    df = sampler.products()["sample"].data
    assert len(df) > 0
    x = torch.as_tensor(df[NAMES].to_numpy())
    for name, f, cols in (("slow", slow_ab, [0, 1]), ("fast", fast_bce, [1, 2, 3])):
        np.testing.assert_allclose(df["chi2__" + name].to_numpy(), -2 * f(x[:, cols]).numpy(),
                                   rtol=1e-12, atol=1e-12)


def test_run_resumes_bit_identically_in_mid_cycle(tmp_path):
    """A run stopped at a step that is no multiple of the cycle and resumed from its state file
    (which carries ll_c) ends in the state of the run that was never stopped."""
    def make(prefix, resume, max_samples):
        opts = {"seed": 21, "n_walkers": 512, "group_size": 64, "steps_per_launch": 11, "oversample_power": 0.4,
                "max_samples": max_samples, "Rminus1_stop": 0.0, "learn_every": "20d"}
        return MCMCHip(opts, ProblemSpec.from_info(two_function_info(512)), output=prefix, resume=resume)

    a = make(str(tmp_path / "a"), False, 60000)
    a.run()
    ref = a.engine.get_full_state()
    steps_total = a.n_steps_raw
    a.close()
    b1 = make(str(tmp_path / "b"), False, 30000)
    b1.run()
    assert b1.n_steps_raw < steps_total and b1.n_steps_raw % b1.cycle_length != 0
    assert "ll_c" in np.load(b1._state_file())
    b1.close()
    b2 = make(str(tmp_path / "b"), True, 60000)
    assert b2.n_steps_raw == b1.n_steps_raw
    b2.run()
    got = b2.engine.get_full_state()
    assert b2.n_steps_raw == steps_total
    for k in ("x", "logpost", "logprior", "loglike", "ll_c", "weight", "n_accept", "burn_left", "prior_rej"):
        assert np.array_equal(got[k], ref[k]), k
    assert int(got["step"]) == int(ref["step"])
    b2.close()


def test_the_six_device_products_together_on_a_two_function_run():
    from tests.products_together import PRODUCTS, all_options, derived_params

    info = two_function_info(512, seed=7, Rminus1_stop=0.0, max_samples=100000, steps_per_launch=40,
                             moments_every=1, snapshot_every=40, learn_every="20d", **all_options(NAMES))
    info["params"].update(derived_params(NAMES))
    _, smp = run(info)
    assert smp.engine.last_step_kernel().startswith(KERNEL)
    assert [p.name for p in smp._products] == list(PRODUCTS)
    prod = smp.products()
    assert prod["derived"].n_samples > 0 and prod["marginals"].n_accumulations > 0
    best = prod["bestfit"].bestfit
    x = torch.as_tensor(best.x[None, :4], device="cuda")
    stored = float((slow_ab(x[:, [0, 1]]) + fast_bce(x[:, [1, 2, 3]]))[0])
    assert best.loglike == stored, (best.loglike, stored)
    smp.close()
    assert smp.products()["bestfit"].bestfit.loglike == stored    # kept at close()


def test_posterior_moments_of_two_gaussian_functions():
    """4 096 walkers to the default stop: every mean lies within 6 standard errors of 0, the error
    estimated from exact draws of the joint Gaussian on the CPU."""
    info = two_function_info(4096, seed=11, oversample_power=1.0, max_samples=4096 * 200000)
    _, sampler = run(info)
    assert sampler.converged, sampler.Rminus1_last
    assert sampler.engine.last_step_kernel().startswith(KERNEL)
    x = sampler.engine.get_state()["x"]
    rng = np.random.default_rng(0)
    draws = rng.multivariate_normal(np.zeros(4), EXACT_COV, size=(200, 4096))
    se = draws.mean(axis=1).std(axis=0, ddof=1)                 # of the mean of 4 096 exact draws
    np.testing.assert_allclose(se, np.sqrt(np.diag(EXACT_COV) / 4096), rtol=0.25)
    for i, p in enumerate(NAMES):
        print("E %s: got %.5f  (%.2f standard errors)" % (p, x[:, i].mean(), x[:, i].mean() / se[i]))
    for i, p in enumerate(NAMES):
        assert abs(x[:, i].mean()) < 6 * se[i], (p, x[:, i].mean(), se[i])
