"""Reweighted marginal histograms of the importance alternatives, host side (no GPU): the per-alternative
key `marginals` and its refusals by name, `WeightedMarginals` on crafted 128-bit words, the merge of shards,
files, and the window bookkeeping of the sampler on an oracle-backed engine double that serves the four new
methods in numpy (tests/importance_hist_ref.py: THE REFERENCE, the rule of DESIGN.md section 2 "Importance
marginals").  Every test fails without the feature: the key, the class and the methods do not exist."""
import math
import os
from fractions import Fraction
from types import SimpleNamespace

import numpy as np
import pytest

from cobaya_amd.importance import Importance, ImportanceAccumulator, ImportanceError, hist_value, parse_option
from cobaya_amd.marginals import Marginals, MarginalsError, WeightedMarginals, slab_size
from cobaya_amd.model import ProblemSpec
from cobaya_amd.sampler import LoggedError, MCMCHip
from tests.importance_hist_ref import HistOracleEngine, HistRule, rule_add, rule_q, words
from tests.importance_ref import ImOracleEngine, Rule, rule_c, rule_e
from tests.test_host_logic import QUICK
from tests.test_marginals_host import MargOracleEngine

# (products and differences only: torch on the CPU and numpy round them alike)
BAO = "lambda a: -0.5 * ((a - 0.31) * 5.0) * ((a - 0.31) * 5.0)"
OPT = {"bao": {"function": BAO, "marginals": True},
       "tight": {"function": "lambda a, b: -2.0 * b * b + 0.0 * a", "cov": False},
       "tilt": {"function": "lambda b: 0.75 * b", "cov": False, "marginals": True}}
MARG = {"params": "all", "pairs": [["b", "a"]], "bins": 16, "bins2d": 4}


class Recording(HistOracleEngine):
    """Keeps the state and the log-weights of every accumulation, for the replay."""

    def accumulate_importance(self, delta):
        self.seen = getattr(self, "seen", []) + [(self._state.x.copy(), delta.numpy().copy())]
        super().accumulate_importance(delta)


class OnDouble(MCMCHip):
    _engine_factory = staticmethod(Recording)


def acc(s):
    return next((p for p in s._products if p.name == "importance"), None)


def make(prefix=None, max_samples=30000, resume=False, **opts):
    o = {"seed": 21, "n_walkers": 128, "group_size": 64, "steps_per_launch": 40, "max_samples": max_samples,
         "Rminus1_stop": 0.0, "learn_every": "20d", "snapshot_every": 40, "importance": OPT, "marginals": MARG}
    o.update(opts)
    return OnDouble(o, ProblemSpec.from_info(QUICK), output=prefix, resume=resume)


# ------------------------------------------------------------------------------- the option
def test_the_key_parses_to_a_flag_per_alternative():
    cfg = parse_option({"x": {"function": BAO, "marginals": True}, "y": {"function": BAO, "marginals": False},
                        "z": {"function": BAO, "marginals": None}, "w": {"function": BAO}}, ["a", "b"])
    assert [c["marginals"] for c in cfg] == [True, False, False, False]
    with pytest.raises(ImportanceError, match="importance: alternative 'x': marginals must be True, False or None, got 1"):
        parse_option({"x": {"function": BAO, "marginals": 1}}, ["a", "b"])
    with pytest.raises(ImportanceError, match="importance: alternative 'x': marginals must be True, False or None"):
        parse_option({"x": {"function": BAO, "marginals": {"bins": 3}}}, ["a", "b"])


class NeverBuilt(HistOracleEngine):
    def __init__(self, *a, **k):
        raise AssertionError("the option must be refused before the engine is created")


class Refusing(MCMCHip):
    _engine_factory = staticmethod(NeverBuilt)


def test_refusals_by_name_before_the_engine_is_created():
    spec, base = ProblemSpec.from_info(QUICK), {"n_walkers": 128, "group_size": 64}
    with pytest.raises(LoggedError, match="importance: alternative 'x': marginals must be True, False or None"):
        Refusing(dict(base, importance={"x": {"function": BAO, "marginals": "yes"}}, marginals=MARG), spec)
    with pytest.raises(LoggedError, match="importance: alternative 'bao': marginals: True needs the sampler option "
                                          "`marginals`"):
        Refusing(dict(base, importance=OPT), spec)

    class OldDouble(ImOracleEngine, MargOracleEngine):      # (both products, none of the four new methods)
        def __init__(self, *a, **k):
            raise AssertionError("the option must be refused before the engine is created")

    class Old(MCMCHip):
        _engine_factory = staticmethod(OldDouble)
    with pytest.raises(LoggedError, match="importance: alternative 'bao': marginals: True: this engine keeps no "
                                          r"reweighted marginal histograms \(its library predates "
                                          r"mcmc_hip_importance_hist_\*\)"):
        Old(dict(base, importance=OPT, marginals=MARG), spec)
    # the slab: 60 parameters x 128 bins and all pairs x 64^2 bins fit as uint64 counters, not as 128-bit ones
    d = 60
    info = {"likelihood": {"one": None}, "params": {f"p{i}": {"prior": {"min": 0, "max": 1}} for i in range(d)}}
    assert 8 * slab_size(d, 128, 1770, 64) <= 64 << 20 < 16 * slab_size(d, 128, 1770, 64)
    with pytest.raises(LoggedError, match="importance: marginals: True for 1 alternatives takes .* above the 67108864 allowed"):
        Refusing(dict(base, importance={"x": {"function": "lambda p0: p0", "marginals": True}},
                      marginals={"pairs": "all", "bins2d": 64}), ProblemSpec.from_info(info))


# ------------------------------------------------------------------------------- WeightedMarginals
def test_weighted_marginals_on_crafted_weights():
    w = WeightedMarginals(["t"], [], 4, 1, {"t": (0.0, 4.0)}, [0.5, 0.25, 1.0, 0.0, 3.0, 6.0], 2, 200, saturated=3,
                          log_scale=-2.5)
    assert np.isclose(w.density("t").sum() * 1.0, 1.0, rtol=1e-15) and w.outside("t") == (0.5, 0.25)
    assert w.weights("t").tolist() == [1.0, 0.0, 3.0, 6.0] and w.weights("t").dtype == np.float64
    assert w.quantile("t", 0.05) == pytest.approx(0.5) and w.quantile("t", 0.10) == pytest.approx(1.0)
    assert w.quantile("t", 0.25) == pytest.approx(2.5) and w.quantile("t", 0.70) == pytest.approx(3.5)
    np.testing.assert_allclose(w.quantile("t", [0.4, 0.1]), [3.0, 1.0])
    assert w.mean("t") == pytest.approx((1 * 0.5 + 3 * 2.5 + 6 * 3.5) / 10)
    assert np.array_equal(w.edges("t"), np.linspace(0.0, 4.0, 5))
    assert (w.saturated, w.n_accumulations, w.n_samples, w.log_scale) == (3, 2, 200, -2.5)
    # the same arithmetic as the unweighted histogram of ten times the counts
    m = Marginals(["t"], [], 4, 1, {"t": (0.0, 4.0)}, np.array([0, 0, 10, 0, 30, 60], np.uint64), 1, 100)
    assert np.array_equal(w.density("t"), m.density("t")) and w.quantile("t", 0.33) == m.quantile("t", 0.33)
    with pytest.raises(MarginalsError, match="quantile"):
        w.quantile("t", -0.1)
    with pytest.raises(MarginalsError, match="this layout holds 6 weights, got 5"):
        WeightedMarginals(["t"], [], 4, 1, {"t": (0.0, 4.0)}, np.zeros(5))
    with pytest.raises(MarginalsError, match="no sample of 't' inside its range"):
        WeightedMarginals(["t"], [], 4, 1, {"t": (0.0, 4.0)}).density("t")


def test_weighted_marginals_merge_at_the_common_scale_compare_and_round_trip(tmp_path):
    rng = np.random.default_rng(2)
    lay = (["a", "b"], [("b", "a")], 6, 3, {"a": (0.0, 1.0), "b": (-1.0, 1.0)})
    n = slab_size(2, 6, 1, 3)
    a = WeightedMarginals(*lay, rng.uniform(0, 4, n), 3, 300, 1, 0.0)
    b = WeightedMarginals(*lay, rng.uniform(0, 4, n), 3, 300, 2, math.log(4.0))
    both = a.merge(b)
    assert both.log_scale == math.log(4.0) and both.saturated == 3 and both.n_samples == 600 and both.n_accumulations == 3
    np.testing.assert_allclose(both.slab, 0.25 * a.slab + b.slab, rtol=1e-15)
    assert (a + b) == both and both != a and a != "weights"
    area = (1.0 / 3) * (2.0 / 3)
    assert np.isclose(both.density2d("b", "a").sum() * area, 1.0, rtol=1e-14) and both.weights2d("b", "a").shape == (3, 3)
    assert both.outside("b", "a") == both.slab[2 * 8]
    with pytest.raises(MarginalsError, match="only weighted histograms of one run"):
        a.merge(WeightedMarginals(["a", "b"], [("b", "a")], 6, 3, {"a": (0.0, 2.0), "b": (-1.0, 1.0)}, None, 3))
    with pytest.raises(MarginalsError, match="only weighted histograms of one run"):
        a.merge(Marginals(*lay))
    p = str(tmp_path / "w.npz")
    both.save(p)
    back = WeightedMarginals.load(p)
    assert back == both and back.slab.dtype == np.float64 and back.ranges == both.ranges and back.saturated == 3


def _part(c, lo, hi, sat=0, n_acc=1, s1=1.0, n=64):
    """A read-out of ONE alternative at d = 1, one group, without the covariance, with histograms."""
    return {"sums": np.array([s1, s1, 0.0, 0.0]), "n": np.array([[n]], np.uint64), "counters": np.zeros((1, 3), np.uint64),
            "c": np.array([c]), "n_acc": n_acc,
            "hist": {"lo": np.array([lo], np.uint64), "hi": np.array([hi], np.uint64), "saturated": np.array([sat], np.uint64),
                     "n_acc": n_acc}}


MARG1 = {"params": ["a"], "pairs": [], "bins": 2, "bins2d": 1, "ranges": {"a": (0.0, 1.0)}, "on": [True]}


def test_words_with_a_high_part_are_converted_and_intervals_meet_at_the_common_scale():
    one = 1 << 32                  # the word of a weight of 1.0
    assert hist_value([one, 0, 3], [0, 1, 2]).tolist() == [1.0, 2.0 ** 32, (2 * 2.0 ** 64 + 3) * 2.0 ** -32]
    # [under, over, bin 0, bin 1]
    parts = [_part(0.5, [0, one, 3 * one, one // 2], [0, 0, 0, 5], sat=2),
             _part(0.5 + math.log(2.0), [one, 0, one, one], [0, 0, 0, 0], sat=1)]
    iw = Importance.from_parts(["x"], ["a"], [0.0], [False], 64, parts, marg=MARG1)
    wm = iw.marginals("x")
    half = math.exp(0.5 - (0.5 + math.log(2.0)))
    assert wm.log_scale == iw.C[0] == 0.5 + math.log(2.0)
    want = half * np.array([0.0, 1.0, 3.0, 5 * 2.0 ** 32 + 0.5]) + np.array([1.0, 0.0, 1.0, 1.0])
    assert np.array_equal(wm.slab, want) and wm.saturated == iw.saturated("x") == 3
    assert (wm.n_accumulations, wm.n_samples) == (2, 128) and wm.outside("a") == (want[0], want[1])
    assert np.isclose(wm.density("a").sum() * 0.5, 1.0, rtol=1e-15)
    assert any("saturated" in t for t in iw.warnings("x")) and "saturated" in iw.summary() and "WARNING" in iw.summary()
    # an interval without an accumulation is skipped, its words included
    assert Importance.from_parts(["x"], ["a"], [0.0], [False], 64, parts + [_part(99.0, [7] * 4, [7] * 4, n_acc=0)],
                                 marg=MARG1) == iw
    # different weights are a different product; one without histograms says so by name
    other = Importance.from_parts(["x"], ["a"], [0.0], [False], 64, [parts[0], _part(0.5 + math.log(2.0), [one, 0, one + 1, one], [0] * 4, sat=1)],
                                  marg=MARG1)
    assert other != iw
    plain = Importance.from_parts(["x"], ["a"], [0.0], [False], 64, parts)
    assert plain != iw and plain.saturated("x") == 0 and plain.marg is None
    with pytest.raises(ImportanceError, match="importance: alternative 'x' keeps no reweighted marginals"):
        plain.marginals("x")


def test_centring_constants_1400_apart_stay_finite():
    one = 1 << 32
    small, big = _part(-700.0, [0, 0, 5 * one, 7 * one], [0] * 4), _part(700.0, [0, 0, 2 * one, 6 * one], [0] * 4)
    for parts in ([small, big], [big, small]):
        wm = Importance.from_parts(["x"], ["a"], [0.0], [False], 64, parts, marg=MARG1).marginals("x")
        assert wm.log_scale == 700.0 and wm.slab.tolist() == [0.0, 0.0, 2.0, 6.0]       # exp(-1400) = 0.0 exactly
        assert np.all(np.isfinite([*wm.density("a"), wm.mean("a"), wm.quantile("a", 0.5)]))
        assert wm.quantile("a", 0.25) == pytest.approx(0.5)


def test_save_and_load_of_the_product_with_and_without_histograms(tmp_path):
    one = 1 << 32
    parts = [_part(0.5, [0, one, 3 * one, one // 2], [0, 0, 0, 5], sat=2, n_acc=2)]
    iw = Importance.from_parts(["x"], ["a"], [0.25], [False], 64, parts, marg=MARG1)
    p = str(tmp_path / "i.npz")
    iw.save(p)
    back = Importance.load(p)
    assert back == iw and back.marginals("x") == iw.marginals("x") and back.saturated("x") == 2
    z = np.load(p)
    assert {"hist_on", "hist_weights", "hist_saturated", "marg_params", "marg_ranges"} <= set(z.files)
    plain = Importance.from_parts(["x"], ["a"], [0.25], [False], 64, [{k: v for k, v in parts[0].items() if k != "hist"}])
    plain.save(p)
    z = np.load(p)         # without histograms the file is what it always was
    assert not [k for k in z.files if k.startswith("hist_") or k.startswith("marg_")] and Importance.load(p) == plain


# ------------------------------------------------------------------------------- shards
MG = dict(dims1=[0, 1], bins1=8, pairs=[(1, 0)], bins2=4, lo=np.array([-1.0, -1.0]), hi=np.array([1.0, 1.0]))


def _host(W, size=1, rank=0, reduce=None):
    return SimpleNamespace(fail=None, n_walkers=W, size=size, rank=rank, temperature=1.0, snapshot_steps=40,
                           all_reduce_sum=reduce)


def _states(W, d, seeds):
    out = []
    for s in seeds:
        rng = np.random.default_rng(s)
        x = 0.5 * rng.standard_normal((W, d))
        delta = np.stack((-0.5 * ((x[:, 0] - 0.1) / 0.2) ** 2, 1.5 * x[:, 1]))
        delta[:, [5, W // 2 + 9]] = 2.5        # the maximum, once in either half: both shards take the same c
        delta[0, [7, W // 2 + 1]] = [-np.inf, np.nan]
        out.append((x, delta))
    return out


def _run_rules(states, sl, gs, cov, shift, on):
    rule, hr = Rule(states[0][0].shape[1], sl.stop - sl.start, gs, cov), HistRule(on, MG)
    parts = []
    for i, (x, dl) in enumerate(states):
        rule.accumulate(x[sl], dl[:, sl], shift)
        hr.accumulate(x[sl], dl[:, sl], rule.c)
        if i == 0 or i == len(states) - 1:
            n_acc = rule.n_acc
            parts.append(dict(rule.request(i == 0), hist=hr.request(i == 0, n_acc)))
    return parts


def test_two_shards_merge_to_the_whole_and_combine_through_the_all_reduce():
    spec = ProblemSpec.from_info(QUICK)
    d, W, gs, cov, shift, on = 2, 256, 64, [True, False], np.array([0.05, -0.02]), [True, True]
    states = _states(W, d, (1, 2, 3))
    whole = _run_rules(states, slice(0, W), gs, cov, shift, on)
    halves = [_run_rules(states, slice(0, W // 2), gs, cov, shift, on), _run_rules(states, slice(W // 2, W), gs, cov, shift, on)]
    assert whole[0]["c"].tolist() == [2.5, 2.5]
    # interval 0: equal c, so the 128-bit words of the shards add up to the whole's exactly
    for h in range(2):
        tot = [(int(b) << 64) + int(a) for k in range(2) for a, b in zip(halves[k][0]["hist"]["lo"][h], halves[k][0]["hist"]["hi"][h])]
        nc = len(tot) // 2
        lo, hi = words([tot[i] + tot[nc + i] for i in range(nc)])
        assert np.array_equal(lo, whole[0]["hist"]["lo"][h]) and np.array_equal(hi, whole[0]["hist"]["hi"][h])
    cfg = parse_option({"g": {"function": "lambda a: a", "marginals": True},
                        "l": {"function": "lambda b: b", "cov": False, "marginals": True}}, spec.sampled)
    marg = SimpleNamespace(cfg={"params": ["a", "b"], "pairs": [("b", "a")], "bins": 8, "bins2d": 4,
                                "resolved": {"a": (-1.0, 1.0), "b": (-1.0, 1.0)}, "n_counters": slab_size(2, 8, 1, 4)})

    def product(parts, host):
        a = ImportanceAccumulator(cfg, spec, host)
        a.ivs, a.open, a.shift, a.G, a.marg = [parts[0]], parts[1], shift, len(parts[0]["n"][0]), marg
        return a, a.product([], combined=host.size > 1)

    ref = product(whole, _host(W))[1]
    assert ref.n_acc == 3 and ref.marginals("g").n_samples == 3 * W and ref.marginals("l").weights("a").sum() > 0
    pa, pb = (product(h, _host(W // 2))[1] for h in halves)
    both = pa.merge(pb)
    for name in ("g", "l"):
        a, b = both.marginals(name), ref.marginals(name)
        assert a.log_scale == b.log_scale and a.saturated == b.saturated and a.n_samples == b.n_samples
        # ("g" has the same c in every shard and interval, and its sums stay below 2^53: exact; "l" meets to rounding)
        assert np.array_equal(a.slab, b.slab) if name == "g" else np.allclose(a.slab, b.slab, rtol=1e-13, atol=0)
        assert a == pa.marginals(name).merge(pb.marginals(name)) and pa.marginals(name) != b
    assert both.sums[0].tobytes() == ref.sums[0].tobytes()
    with pytest.raises(ImportanceError, match="importance: only shards of one run"):
        pa.merge(Importance.from_parts(["g", "l"], pb.params, pb.shift, cov, W // 2, halves[1]))     # (no histograms)
    # ... and over two processes: process 0 only sends (recorded), process 1 reduces against the recorded rows
    a0, a1 = (product(h, _host(W // 2, 1, rank))[0] for rank, h in enumerate(halves))

    class _Sent(Exception):
        pass

    a0.host = _host(W // 2, 2, 0, None)
    sent0 = []

    def record(buf):
        sent0.append(buf.copy())
        if len(sent0) == 1:      # the head: answer with what process 1 will send (the same C, n_acc, G)
            buf[...] = buf + np.concatenate((np.zeros(len(buf) // 2), buf[:len(buf) // 2]))
        else:
            raise _Sent
    a0.host.all_reduce_sum = record
    with pytest.raises(_Sent):
        a0.product([], combined=True)
    row = sent0[1].reshape(2, -1)
    assert not row[1].any() and row.shape[1] == sum(s.size for s in pa.sums) + 2 * 2 + 3 * 2 + 2 * slab_size(2, 8, 1, 4) + 2
    k = [0]

    def reduce1(buf):
        buf[...] = buf + sent0[k[0]]
        k[0] += 1
    a1.host = _host(W // 2, 2, 1, reduce1)
    got = a1.product([], combined=True)
    assert got == both and got.marginals("g") == ref.marginals("g")
    assert a1.product([], combined=False).marginals("g") == pb.marginals("g")


# ------------------------------------------------------------------------------- the window
def _replayed(s):
    """The rule applied to exactly the accumulations of the window: per alternative with the key (weights at
    the scale C, saturated, C) and the closing read-outs."""
    eng, a = s.engine, acc(s)
    ivs = [iv[0] for iv in s._intervals] + [s._snaps_in_interval]
    seen = eng.seen[len(eng.seen) - sum(ivs):]
    hr, parts, at = HistRule(a.want, eng._mg), [], 0
    for n in ivs:
        c = np.array([rule_c(dl) for dl in seen[at][1]]) if n else np.zeros(len(a.want))
        for x, dl in seen[at:at + n]:
            hr.accumulate(x, dl, c)
        parts.append((c, hr.request(True, n)))
        at += n
    parts = [p for p in parts if p[1]["n_acc"]]
    C = np.max([p[0] for p in parts], axis=0)
    out = {}
    for h, k in enumerate(hr.alts):
        w = np.zeros(hr.n_counters)
        for c, p in parts:
            w = w + math.exp(c[k] - C[k]) * hist_value(p["lo"][h], p["hi"][h])
        out[a.names[k]] = (w, sum(int(p["saturated"][h]) for _, p in parts), C[k])
    return out, parts


def test_a_run_on_the_double_follows_the_window_and_writes_the_file(tmp_path):
    p = str(tmp_path / "a")
    s = make(p, max_samples=60000)
    s.run()
    a = acc(s)
    assert len(s.progress) >= 5 and s._dropped_snapshots > 0 and len(a.ivs) == len(s._intervals)
    assert s.engine.hist_log == [("configure", [True, False, True])] and a.want == [True, False, True]
    assert all(iv["hist"]["n_acc"] == iv["n_acc"] == w[0] for iv, w in zip(a.ivs, s._intervals))
    iw = s.products()["importance"]
    mg = s.products()["marginals"]
    want, parts = _replayed(s)
    assert sorted(want) == ["bao", "tilt"]
    for name, (w, sat, C) in want.items():
        wm = iw.marginals(name)
        assert isinstance(wm, WeightedMarginals) and np.array_equal(wm.slab, w) and wm.slab.any()
        assert (wm.saturated, wm.log_scale) == (sat, C) == (iw.saturated(name), iw.C[iw.names.index(name)])
        # names, pairs, bins and ranges are the run's marginals': both overlay bin for bin
        assert (wm.params, wm.pairs, wm.bins, wm.bins2d, wm.ranges) == (mg.params, mg.pairs, mg.bins, mg.bins2d, mg.ranges)
        assert wm.n_accumulations == iw.n_acc == mg.n_accumulations and wm.n_samples == mg.n_samples
        assert np.array_equal(wm.edges("a"), mg.edges("a")) and wm.weights2d("b", "a").shape == (4, 4)
    with pytest.raises(ImportanceError, match="importance: alternative 'tight' keeps no reweighted marginals"):
        iw.marginals("tight")
    # the posterior of a, N(0.2, 0.1), times a Gaussian of mean 0.31 and sd 0.2: the weighted histogram moved
    prec = 1 / 0.1 + 1 / 0.04
    assert abs(iw.marginals("bao").mean("a") - (0.2 / 0.1 + 0.31 / 0.04) / prec) < 0.12      # (bins 0.22 wide)
    assert abs(iw.marginals("bao").mean("a") - iw.mean("bao")[0]) < 0.12 < abs(mg.mean("a") - 2.0)
    # a second call moves nothing; the file loads equal; the product outlives the engine
    assert s.products(combined=True)["importance"] == iw
    assert Importance.load(p + ".importance.npz") == iw
    s.close()
    assert a.engine is None and a.product(s._intervals) == iw


def test_the_weights_of_an_entry_are_consistent_with_the_sums(tmp_path):
    """Per interval and alternative, over a 1-D entry of a sampled parameter every used walker adds its q
    exactly once (under, over or a bin), and q 2^-32 lies in (e - 2^-32, e]; so the entry's exact total T obeys
    S1' - n_used 2^-32 < T 2^-32 <= S1' with S1' the exact sum of e.  The float chain S1 of the sums differs
    from S1' by at most (n - 1) u S1' per chain, u = 2^-53, to first order; the chains of the groups and
    accumulations are then added, which a slack of 2 n_used 2^-53 S1 covers.  Nothing saturated."""
    s = make(max_samples=20000)
    s.run()
    a = acc(s)
    a.product(s._intervals)
    checked = 0
    for part in a.ivs + [a.open]:
        if not part["n_acc"]:
            continue
        for h, k in enumerate(i for i, v in enumerate(a.want) if v):
            assert int(part["hist"]["saturated"][h]) == 0
            S1 = float(np.asarray(part["sums"][:2 * 7] if k == 0 else part["sums"][2 * 7 + 2 * 6:]).reshape(2, -1)[:, 0].sum())
            n_used = int(part["n"][k].sum())
            slack = Fraction(2 * n_used, 1 << 53) * Fraction(S1)
            for e in range(2):      # the entries of a and of b: 16 bins + 2
                lo, hi = part["hist"]["lo"][h][18 * e:18 * e + 18], part["hist"]["hi"][h][18 * e:18 * e + 18]
                T = Fraction(sum((int(b) << 64) + int(v) for v, b in zip(lo, hi)), 1 << 32)
                assert Fraction(S1) - slack - Fraction(n_used, 1 << 32) < T <= Fraction(S1) + slack, (k, e, float(T), S1)
                checked += 1
    assert checked >= 8


def test_a_resume_in_mid_interval_ends_bit_identical_and_both_resume_refusals(tmp_path):
    one = make(str(tmp_path / "a"), 40000)
    one.run()
    p = str(tmp_path / "b")
    b1 = make(p, 20000)
    b1.run()
    z = np.load(p + ".1.state.npz", allow_pickle=False)
    n_iv, nc = len(z["iv_n"]), slab_size(2, 16, 1, 4)
    new = {"iw_hist_on": (np.int64, (3,)), "iw_iv_hlo": (np.uint64, (n_iv, 2, nc)), "iw_iv_hhi": (np.uint64, (n_iv, 2, nc)),
           "iw_iv_hsat": (np.uint64, (n_iv, 2)), "iw_open_hlo": (np.uint64, (1, 2, nc)),
           "iw_open_hhi": (np.uint64, (1, 2, nc)), "iw_open_hsat": (np.uint64, (1, 2))}
    for k, (dtype, shape) in new.items():
        assert z[k].shape == shape and z[k].dtype == np.dtype(dtype), (k, z[k].dtype, z[k].shape)
    assert z["iw_hist_on"].tolist() == [1, 0, 1] and int(z["iw_open_nacc"][0]) > 0 and z["iw_open_hlo"].any()
    b2 = make(p, 40000, resume=True)
    assert b2.engine.hist_log == [("configure", [True, False, True]), ("set", 2 * nc)]
    back = b2.engine._hr.request(False, 0)
    assert np.array_equal(back["lo"], z["iw_open_hlo"][0]) and np.array_equal(back["hi"], z["iw_open_hhi"][0])
    b2.run()
    got, ref = b2.products()["importance"], one.products()["importance"]
    assert got == ref and all(got.marginals(n).slab.tobytes() == ref.marginals(n).slab.tobytes() for n in ("bao", "tilt"))
    assert got.n_samples > Importance.load(p + ".importance.npz").n_samples or Importance.load(p + ".importance.npz") == got
    # other flags than the file's are refused by name ...
    flipped = {k: dict(v, marginals=(k == "tight")) for k, v in OPT.items()}
    none = {k: {q: w for q, w in v.items() if q != "marginals"} for k, v in OPT.items()}
    for opt, now in ((flipped, r"\[False, True, False\]"), (none, r"\[False, False, False\]")):
        with pytest.raises(LoggedError, match=r"importance: cannot resume -- the run was written with marginals: "
                                              r"\[True, False, True\] per alternative, and now has " + now):
            make(p, 50000, resume=True, importance=opt)
    # ... and so is the key on a run that was written without it
    q = str(tmp_path / "c")
    make(q, 5000, importance=none).run()
    zq = np.load(q + ".1.state.npz", allow_pickle=False)
    assert not [k for k in zq.files if "_h" in k and k.startswith("iw_")] and "iw_names" in zq.files
    with pytest.raises(LoggedError, match=r"importance: cannot resume -- the run was written with marginals: "
                                          r"\[False, False, False\] per alternative, and now has \[True, False, True\]"):
        make(q, 9000, resume=True)
    make(q, 9000, resume=True, importance=none).run()         # (as it was written: served as before)


# ------------------------------------------------------------------------------- off
class Untouchable(HistOracleEngine):
    """Every one of the four new methods raises: a run without the key must call none of them."""


for _name in ("configure_importance_hist", "importance_hist_layout", "fetch_importance_hist", "importance_hist_set"):
    def _raises(self, *a, _n=_name, **k):
        raise AssertionError(f"{_n} was called without the key")
    setattr(Untouchable, _name, _raises)


def test_a_run_without_the_key_never_touches_the_new_methods(tmp_path):
    class Off(MCMCHip):
        _engine_factory = staticmethod(Untouchable)
    none = {k: {q: w for q, w in v.items() if q != "marginals"} for k, v in OPT.items()}
    p = str(tmp_path / "d")
    o = {"seed": 21, "n_walkers": 128, "group_size": 64, "steps_per_launch": 40, "max_samples": 8000, "Rminus1_stop": 0.0,
         "learn_every": "20d", "snapshot_every": 40, "importance": none, "marginals": MARG}
    s = Off(o, ProblemSpec.from_info(QUICK), output=p)
    s.run()
    iw = s.products()["importance"]
    assert iw.marg is None and iw.saturated("bao") == 0 and "marginals" in s.products()
    z = np.load(p + ".1.state.npz", allow_pickle=False)
    assert "iw_hist_on" not in z.files and not [k for k in z.files if k.startswith("iw_") and "_h" in k]
    assert not [k for k in np.load(p + ".importance.npz").files if k.startswith("hist_") or k.startswith("marg_")]
    s.close()
    Off(dict(o, max_samples=12000), ProblemSpec.from_info(QUICK), output=p, resume=True).run()
    # the double of before this feature (no such methods at all) still serves a run without the key ...

    class OldDouble(ImOracleEngine, MargOracleEngine):
        pass

    class Old(MCMCHip):
        _engine_factory = staticmethod(OldDouble)
    assert "importance" in Old(dict(o, max_samples=4000), ProblemSpec.from_info(QUICK)).products()
    # ... and refuses the key by name
    with pytest.raises(LoggedError, match=r"its library predates mcmc_hip_importance_hist_\*"):
        Old(dict(o, importance=OPT), ProblemSpec.from_info(QUICK))


def test_the_rule_of_the_quantised_weight():
    e = np.array([0.0, 1.0, 2.0 ** -32, 2.0 ** -32 * (1 - 2.0 ** -52), 65536.0, 65536.0 * (1 + 2.0 ** -52), 1e300, 0.3, 7.0])
    used = np.array([True, True, True, True, True, True, True, True, False])
    q, sat = rule_q(e, used)
    assert q.tolist() == [0, 1 << 32, 1, 0, 1 << 48, 1 << 48, 1 << 48, int(math.floor(0.3 * 2 ** 32)), 0]
    assert sat.tolist() == [False] * 5 + [True, True, False, False]
    # one walker each: under, on lo, an interior edge (the upper bin), on hi (the last bin), over, NaN (nowhere)
    x = np.array([[-1e-300], [0.0], [0.5], [1.0], [np.nextafter(1.0, 2.0)], [np.nan]])
    add = rule_add(x, np.arange(1, 7, dtype=np.uint64), [0], 2, [], 1, [0.0], [1.0])
    assert add.tolist() == [1, 5, 2, 3 + 4]
    lo, hi = words([(1 << 64) + 5, 3])
    assert lo.tolist() == [5, 3] and hi.tolist() == [1, 0]
    assert rule_e([0.0], 0.0)[0][0] == 1.0
