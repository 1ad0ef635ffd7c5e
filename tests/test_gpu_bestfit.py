"""Best fit, MAP and profile likelihoods on the MI355X (bestfit_kernels.hip, mcmc_hip_bestfit_*): the
slab of keys and the two records equal the rule of DESIGN.md section 2 ("Best fit and profiles") --
tests/bestfit_ref.py, numpy -- bit for bit, on keys and integers, at the smallest shapes at which
the kernels can still go wrong; the read-out is stream-ordered; shards merge to the whole; the
sampler's product re-evaluates to itself.  Every test fails without the feature: the entry points
and the option do not exist."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402,F401  (before the first Engine: one HIP runtime for both)

from cobaya_amd import run  # noqa: E402
from cobaya_amd.bestfit import BestFit, key_of, merge_records  # noqa: E402
from cobaya_amd.engine import ERR_ARG, ERR_STATE, Engine, EngineError  # noqa: E402
from tests.bestfit_ref import Rule, rule_key, rule_over  # noqa: E402


def _same(got, want):
    """(slab, records) of the engine against the rule's, bit for bit."""
    assert got[0].dtype == np.uint64 and got[1].dtype == np.uint64
    assert got[0].shape == want[0].shape and np.array_equal(got[0], want[0])
    assert np.array_equal(got[1], want[1]), (got[1][:, :6], want[1][:, :6])


# ------------------------------------------------------------------------------ crafted states
def _crafted(W, d, B, rng, step):
    """A state on [-1, 2]^d with profile ranges [0, 1]: coordinates on every interior edge k / B (as
    far as W allows), one ulp on either side of some, on lo, on hi, outside on both sides; values
    with NaN, -inf, +-0 and 1e300 (loglike, logprior; set_full_state takes finite logpost only: +-0,
    +-1e300 there)."""
    x = rng.uniform(-0.25, 1.25, (W, d))
    edges = [k / B for k in range(1, B)][:W // 4]
    col = ([0.0, 1.0, np.nextafter(0.0, -1.0), np.nextafter(1.0, 2.0), -0.5, 1.5] + edges
           + [np.nextafter(e, -1.0) for e in edges[:8]] + [np.nextafter(e, 2.0) for e in edges[:8]])[:W - 8]
    for i in {0, d - 1}:
        x[8:8 + len(col), i] = col           # (walkers 0..7 keep random coordinates: the special values below)
    ll = rng.normal(-5.0, 3.0, W)
    lpr = rng.normal(-1.0, 0.5, W)
    lp = rng.normal(-6.0, 3.0, W)
    ll[0], ll[1], ll[2], ll[4] = np.nan, -np.inf, -0.0, 0.0
    lpr[0], lpr[5] = -np.inf, np.nan
    lp[2], lp[4], lp[6] = 0.0, -0.0, -1e300
    ll[W - 1] = np.nan                       # the last walker of the (ragged) last slice
    z = np.zeros(W, np.int32)
    return {"x": x, "logpost": lp, "logprior": lpr, "loglike": ll, "weight": z + 1, "prior_rej": z,
            "burn_left": z, "n_accept": np.zeros(W, np.int64), "step": np.uint64(step)}


@pytest.mark.parametrize("W, d, B", [(64, 1, 1), (192, 3, 5), (4160, 33, 1024), (4160, 3, 5)])
def test_crafted_states_over_several_accumulations(W, d, B):
    """W = 64: less than the workgroup; 192: no multiple of it; 4160: several slices with a ragged
    last one of 64 walkers.  Duplicated maxima in two walkers (the lowest id wins), an equal maximum
    in a later accumulation (does not replace the record), then a strictly greater one in the last
    slice (replaces it)."""
    rng = np.random.default_rng(100 + W + d)
    eng = Engine(d, W, group_size=64, device=0, seed=3)
    eng.set_prior([0] * d, [-1.0] * d, [2.0] * d)
    eng.set_target_one()
    eng.set_proposal_cov(0.01 * np.eye(d))
    A, Bs, Cs = _crafted(W, d, B, rng, 5), _crafted(W, d, B, rng, 9), _crafted(W, d, B, rng, 12)
    hi_w, lo_w = W - 3, 3
    A["loglike"][[hi_w, lo_w]] = 1e300       # twice the maximum: the lowest id wins
    A["logpost"][[hi_w - 1, lo_w + 2]] = 1e300
    Bs["loglike"][1] = 1e300                 # equal, later, lower id: no replacement
    Bs["logpost"][0] = 1e300
    Cs["loglike"][W - 2] = np.nextafter(1e300, np.inf)   # strictly greater, in the last slice
    lo, hi = np.zeros(d), np.ones(d)
    dims = sorted({0, d - 1, d // 2})
    for quantity, n_dims in (("loglike", dims), ("logpost", dims), ("loglike", [])):
        eng.configure_bestfit(n_dims, B, lo, hi, quantity)
        lay = eng.bestfit_layout()
        assert lay == {"on": 1, "n": len(n_dims), "bins": B if n_dims else 0, "quantity": quantity,
                       "n_slab": len(n_dims) * B, "n_records": 2 * (6 + d)}
        for st in (A, Bs):
            eng.set_full_state(st)
            eng.accumulate_bestfit()
        eng.request_bestfit()
        slab, rec, n = eng.fetch_bestfit()
        assert n == 2
        _same((slab, rec), rule_over([A, Bs], d, n_dims, B, lo, hi, quantity)[:2])
        # ... by hand: the duplicated maximum went to the lowest id at the FIRST accumulation
        assert (int(rec[1, 1]), int(rec[1, 2]), int(rec[1, 0])) == (lo_w, 5, int(rule_key([1e300])[0]))
        assert (int(rec[0, 1]), int(rec[0, 2])) == (lo_w + 2, 5)
        assert np.array_equal(rec[1, 6:].view(np.float64), A["x"][lo_w])
        assert np.array_equal(rec[1, 3:6], np.array([A[k][lo_w] for k in ("logpost", "logprior", "loglike")]).view(np.uint64))
        if n_dims:
            # x == hi is in the last bin, x == lo in the first, what lies outside nowhere: the rule, by hand
            val = (A[quantity], Bs[quantity])
            for e, i in enumerate(n_dims):
                inb = [(st["x"][:, i] >= 0) & (st["x"][:, i] <= 1) & ~np.isnan(v) for st, v in zip((A, Bs), val)]
                assert np.count_nonzero(slab[e]) <= sum(int(m.sum()) for m in inb)
                top = max(v[m].max() for v, m in zip(val, inb))
                assert int(slab[e].max()) == int(key_of([top])[0])
        # the read-out emptied the device; set puts the interval back and the next accumulation goes on
        eng.request_bestfit()
        s0, r0, n0 = eng.fetch_bestfit()
        assert n0 == 0 and not s0.any() and not r0.any()
        eng.bestfit_set(slab, rec, n)
        eng.set_full_state(Cs)
        eng.accumulate_bestfit()
        eng.request_bestfit()
        slab, rec, n = eng.fetch_bestfit()
        assert n == 3
        _same((slab, rec), rule_over([A, Bs, Cs], d, n_dims, B, lo, hi, quantity)[:2])
        assert (int(rec[1, 1]), int(rec[1, 2])) == (W - 2, 12)      # the strictly greater key replaced it
        assert (int(rec[0, 1]), int(rec[0, 2])) == (lo_w + 2, 5)    # ... and the map record stayed
    eng.close()


def test_special_values_fill_their_bins_and_nan_is_skipped():
    """One walker per bin of 8: -inf, -0.0, +0.0, NaN, 1e300 alone in their bins; -0.0 and +0.0
    together in one (the +0.0 wins); a NaN next to a number (the number stays)."""
    d, W, B = 1, 64, 8
    eng = Engine(d, W, group_size=64, device=0, seed=3)
    eng.set_prior([0], [-1.0], [2.0])
    eng.set_target_one()
    eng.set_proposal_cov(0.01 * np.eye(d))
    z = np.zeros(W, np.int32)
    x = np.full((W, 1), 1.5)                  # everyone else: outside
    ll = np.full(W, 7.0)                      # (7.0 sits outside the range: it must not show in any bin)
    centres = (np.arange(8) + 0.5) / 8
    vals = [-np.inf, -0.0, 0.0, np.nan, 1e300]
    x[:5, 0], ll[:5] = centres[:5], vals
    x[5:7, 0], ll[5:7] = centres[5], [0.0, -0.0]
    x[7:9, 0], ll[7:9] = centres[6], [np.nan, -3.0]
    st = {"x": x, "logpost": -1.0 - np.arange(W), "logprior": np.zeros(W), "loglike": ll,
          "weight": z + 1, "prior_rej": z, "burn_left": z, "n_accept": np.zeros(W, np.int64), "step": np.uint64(1)}
    eng.set_full_state(st)
    eng.configure_bestfit([0], B, [0.0], [1.0])
    eng.accumulate_bestfit()
    eng.request_bestfit()
    slab, rec, n = eng.fetch_bestfit()
    want = np.array([0x000FFFFFFFFFFFFF, 0x7FFFFFFFFFFFFFFF, 0x8000000000000000, 0, int(rule_key([1e300])[0]),
                     0x8000000000000000, int(rule_key([-3.0])[0]), 0], np.uint64)
    assert np.array_equal(slab[0], want)
    _same((slab, rec), rule_over([st], d, [0], B, [0.0], [1.0])[:2])
    assert int(rec[1, 1]) == 4 and int(rec[0, 1]) == 0           # bestfit: 1e300 (in or out of range alike); map: walker 0
    b = BestFit(["p"], ["p"], B, {"p": (0.0, 1.0)}, "loglike", slab, rec, n, n * W)
    p = b.profile("p")
    assert p[0] == -np.inf and np.signbit(p[1]) and p[1] == 0 and not np.signbit(p[2]) and np.isnan(p[3]) and np.isnan(p[7])
    eng.close()


# ------------------------------------------------------------------------------ services, shards
def _gauss_engine(d, W, gs, seed=11, incremental=False, walker_offset=0, x0=None, modes=1):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((d, d)) / np.sqrt(d)
    cov = 0.004 * (0.5 * A @ A.T + 0.5 * np.eye(d))
    mean = 0.5 + 0.02 * rng.standard_normal(d)
    eng = Engine(d, W, group_size=gs, device=0, seed=seed, incremental=incremental, walker_offset=walker_offset)
    eng.set_prior([0] * d, [0.0] * d, [1.0] * d)
    means = [mean + 0.03 * k for k in range(modes)]
    eng.set_target_gaussian_mixture(means, [cov] * modes)
    eng.set_proposal_cov(cov)
    if x0 is None:
        x0 = np.clip(mean + rng.standard_normal((W, d)) * np.sqrt(np.diag(cov)), 0.01, 0.99)
    eng.set_state(x0)
    return eng, mean, cov, x0


def _ranges(mean, cov):
    """Asymmetric and narrower than where the walkers go: some walkers fall outside."""
    sd = np.sqrt(np.diag(cov))
    return mean - 1.1 * sd, mean + 1.7 * sd


def _live(eng, d, dims, bins, lo, hi, quantity="loglike", launches=3, steps=3):
    """A few launches with an accumulation after each: (what the engine reads out, the rule over
    the states read back)."""
    eng.configure_bestfit(dims, bins, lo, hi, quantity)
    states = []
    for _ in range(launches):
        eng.step(steps)
        eng.accumulate_bestfit()
        states.append(eng.get_full_state())
    eng.request_bestfit()
    slab, rec, n = eng.fetch_bestfit()
    assert n == launches
    return (slab, rec), rule_over(states, d, dims, bins, lo, hi, quantity, eng.walker_offset)[:2], states


def test_request_empties_in_stream_order_set_restores_and_errors_are_codes():
    d, W = 3, 128
    eng, mean, cov, _ = _gauss_engine(d, W, 64, seed=23)
    lo, hi = _ranges(mean, cov)
    assert eng.bestfit_layout()["on"] == 0
    for call in (eng.accumulate_bestfit, eng.request_bestfit,
                 lambda: eng.bestfit_set(np.zeros(0, np.uint64), np.zeros(18, np.uint64), 0)):
        with pytest.raises(EngineError) as ei:        # before configure: nothing is allocated or launched
            call()
        assert ei.value.code == ERR_STATE and "bestfit_configure must precede" in str(ei.value)
    cfg = ([0, 1, 2], 12, lo, hi)
    eng.configure_bestfit(*cfg)
    with pytest.raises(EngineError) as ei:
        eng.fetch_bestfit()
    assert ei.value.code == ERR_STATE
    eng.step(2)
    eng.accumulate_bestfit()
    first = rule_over([eng.get_full_state()], d, *cfg)
    eng.request_bestfit()
    with pytest.raises(EngineError) as ei:
        eng.request_bestfit()
    assert ei.value.code == ERR_STATE and "pending" in str(ei.value)
    eng.step(2)
    eng.accumulate_bestfit()                      # queued AFTER the request: the next fetch's
    second = rule_over([eng.get_full_state()], d, *cfg)
    slab, rec, n = eng.fetch_bestfit()
    assert n == 1
    _same((slab, rec), first[:2])
    eng.request_bestfit()
    got = eng.fetch_bestfit()
    assert got[2] == 1
    _same(got[:2], second[:2])
    assert not np.array_equal(first[0], second[0])
    eng.request_bestfit()
    got = eng.fetch_bestfit()
    assert got[2] == 0 and not got[0].any() and not got[1].any()
    # resume: an unfinished interval goes back, the next accumulation goes on from it
    eng.bestfit_set(slab, rec, 3)
    eng.step(1)
    eng.accumulate_bestfit()
    r = Rule(d, *cfg)
    r.set(slab, rec, 3)
    r.accumulate(eng.get_full_state())
    eng.request_bestfit()
    got = eng.fetch_bestfit()
    assert got[2] == 4
    _same(got[:2], (r.slab, r.records))
    for s_, r_, word in ((slab.reshape(-1)[:-1], rec, "slab"), (slab, rec.reshape(-1)[:-1], "records")):
        with pytest.raises(EngineError) as ei:
            eng.bestfit_set(s_, r_, 1)
        assert ei.value.code == ERR_ARG and word in str(ei.value)
    with pytest.raises(EngineError) as ei:
        eng.bestfit_set(slab, rec, -1)
    assert ei.value.code == ERR_ARG and "n_accumulations" in str(ei.value)
    # a bad configuration names its argument and leaves the old layout alone
    for kw, word in ((dict(dims=[3]), "dims"), (dict(dims=[-1]), "dims"), (dict(bins=1025), "bins"), (dict(bins=0), "bins"),
                     (dict(hi=np.array([np.inf, 1, 1])), "hi"), (dict(lo=hi), "lo"), (dict(quantity="chi2"), "quantity")):
        a = dict(dims=[0, 1, 2], bins=12, lo=lo, hi=hi, quantity="loglike")
        a.update(kw)
        with pytest.raises(EngineError) as ei:
            eng.configure_bestfit(**a)
        assert ei.value.code == ERR_ARG and word in str(ei.value), (word, str(ei.value))
    assert eng.bestfit_layout()["n_slab"] == 36
    eng.close()


def test_two_shards_merge_to_the_whole_ensemble():
    d, W = 5, 256
    whole, mean, cov, x0 = _gauss_engine(d, W, 64, seed=19)
    lo, hi = _ranges(mean, cov)
    parts = [_gauss_engine(d, W // 2, 64, seed=19, walker_offset=k * (W // 2),
                           x0=x0[k * (W // 2):(k + 1) * (W // 2)])[0] for k in range(2)]
    out = []
    for eng in [whole] + parts:
        eng.configure_bestfit([0, 2, 4], 16, lo, hi)
        for _ in range(2):
            eng.step(4)
            eng.accumulate_bestfit()
        eng.request_bestfit()
        out.append(eng.fetch_bestfit())
    assert np.array_equal(np.vstack([p.get_state()["x"] for p in parts]), whole.get_state()["x"])
    assert np.array_equal(np.maximum(out[1][0], out[2][0]), out[0][0]) and out[0][0].any()
    assert np.array_equal(merge_records(out[1][1], out[2][1]), out[0][1])
    assert np.array_equal(merge_records(out[2][1], out[1][1]), out[0][1])
    assert all(W // 2 <= int(out[2][1][r, 1]) < W and int(out[1][1][r, 1]) < W // 2 for r in (0, 1))   # global ids
    for eng in [whole] + parts:
        eng.close()


# ------------------------------------------------------------------------------ live paths
@pytest.mark.parametrize("d, inc, modes", [(30, True, 1), (8, True, 2), (5, False, 1), (130, True, 1)],
                         ids=["one-mode-incremental-d30", "two-modes-d8", "full-d5", "d130"])
def test_live_paths_equal_the_rule_on_the_states_read_back(d, inc, modes):
    W = 256
    eng, mean, cov, _ = _gauss_engine(d, W, 64, seed=31 + d, incremental=inc, modes=modes)
    lo, hi = _ranges(mean, cov)
    dims = sorted({0, d // 2, d - 1})
    got, want, states = _live(eng, d, dims, 7, lo, hi)
    print(eng.last_step_kernel())
    _same(got, want)
    assert got[0].all() and got[1][:, 0].all()            # every bin and both records are filled
    assert states[0]["step"] == 3 and int(got[1][1, 2]) in (3, 6, 9)
    got, want, _ = _live(eng, d, dims[:1], 1024, lo, hi, "logpost", launches=2)
    _same(got, want)
    eng.close()


def test_live_function_target():
    def banana(p):                      # the banana of tests/test_gpu_function_target.py
        return -0.5 * (p[:, 0] ** 2 + ((p[:, 1] - 0.5 * p[:, 0] ** 2) / 0.5) ** 2)

    eng = Engine(2, 128, group_size=64, device=0, seed=31)
    eng.set_prior([0, 0], [-8.0, -6.0], [8.0, 30.0])
    eng.set_target_function(banana)
    eng.set_proposal_cov(np.eye(2))
    rng = np.random.default_rng(31)
    eng.set_state(np.column_stack((rng.normal(0, 1, 128), rng.normal(0.5, 0.5, 128))))
    lo, hi = np.array([-1.5, -0.5]), np.array([1.5, 2.0])
    got, want, _ = _live(eng, 2, [0, 1], 32, lo, hi, steps=4)
    assert eng.last_step_kernel().startswith("mcmc::fn_walker_kernel")
    _same(got, want)
    assert got[0].any() and got[1][:, 0].all()
    eng.close()


# ------------------------------------------------------------------------------ end to end
def test_run_on_the_quickstart_gaussian(tmp_path):
    """`evaluation: full`, `bestfit: True`, 4096 walkers.  The records re-evaluate to themselves bit
    for bit; the best fit is within t / 2 of the mode's log-likelihood with t = 2 ln(1e9) / W: ONE
    converged snapshot of W independent draws in d = 2 has all chi2 above t with probability
    exp(-t / 2)^W = 1e-9 (chi2 of two degrees of freedom: P(chi2 > t) = exp(-t / 2)); the file loads
    to an equal product."""
    W = 4096
    o = {"n_walkers": W, "seed": 7, "Rminus1_stop": 0.0, "max_samples": 3.0e6, "steps_per_launch": 40,
         "moments_every": 1, "evaluation": "full", "bestfit": True}
    prefix = str(tmp_path / "q")
    info = {"likelihood": {"gaussian_mixture": {"means": [0.2, 0], "covs": [[0.1, 0.05], [0.05, 0.2]]}},
            "params": {"a": {"prior": {"min": -0.5, "max": 3}},
                       "b": {"prior": {"dist": "norm", "loc": 0, "scale": 1}, "ref": 0, "proposal": 0.5}},
            "sampler": {"mcmc_hip": o}, "output": prefix}
    _, s = run(info)
    b = s.products()["bestfit"]
    assert b.n_accumulations == sum(iv[0] for iv in s._intervals) + s._snaps_in_interval > 0
    assert b.n_samples == b.n_accumulations * W and b.params == ["a", "b"] and b.bins == 64
    assert b.ranges == {"a": (-0.5, 3.0), "b": (-5.0, 5.0)} and b.quantity == "loglike"
    for r in (b.map, b.bestfit):
        lp, ll = s.engine.evaluate(r.x[None, :])
        assert lp.view(np.uint64)[0] == np.float64(r.logprior).view(np.uint64)
        assert ll.view(np.uint64)[0] == np.float64(r.loglike).view(np.uint64)
        assert 0 <= r.walker < W and 0 < r.step <= s.n_steps_raw and r.point == {"a": r.x[0], "b": r.x[1]}
    assert b.map.logpost >= b.bestfit.logpost and b.bestfit.loglike >= b.map.loglike
    ll_mode = s.engine.evaluate(np.array([[0.2, 0.0]]))[1][0]
    t = 2.0 * np.log(1.0e9) / W
    print("loglike(bestfit)", b.bestfit.loglike, "loglike(mode)", ll_mode, "t / 2", t / 2)
    assert b.bestfit.loglike >= ll_mode - t / 2
    assert b.bestfit.loglike <= ll_mode                      # (nothing lies above the mode)
    for name in ("a", "b"):
        assert np.nanmax(b.profile(name)) == b.bestfit.loglike     # the best fit is in range: it tops both profiles
        lo_, hi_ = b.interval(name)
        assert lo_ < b.bestfit.point[name] < hi_
    assert BestFit.load(prefix + ".bestfit.npz") == b
    s.close()
    _, s = run({**info, "output": None, "sampler": {"mcmc_hip": {**o, "bestfit": None, "max_samples": 4.0e5}}})
    assert "bestfit" not in s.products() and s.engine.bestfit_layout()["on"] == 0
    s.close()
