"""Importance reweighting, host side (no GPU): the parsing of the sampler option `importance` and its
refusals by name, the arithmetic of the product on crafted sums, the merge of shards, files, and the
window bookkeeping of the sampler on an oracle-backed engine double that serves the importance methods
in numpy (tests/importance_ref.py: THE REFERENCE, the rule of DESIGN.md section 2 "Importance")."""
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest

from cobaya_amd.importance import (Importance, ImportanceAccumulator, ImportanceError, n_chains, parse_option)
from cobaya_amd.model import ProblemSpec
from cobaya_amd.sampler import HIP_DEFAULTS, LoggedError, MCMCHip
from tests.importance_ref import ImOracleEngine, Rule
from tests.oracle_engine import OracleEngine
from tests.test_host_logic import QUICK

BAO = "lambda a: -0.5 * ((a - 0.31) / 0.2) ** 2"


def module_level_log_ratio(a, b):
    return -0.5 * (b / 0.5) ** 2 + 0.0 * a


OPT = {"bao": {"function": BAO}, "tight": {"function": "tests.test_importance_host:module_level_log_ratio",
                                           "cov": False}}


class OnDouble(MCMCHip):
    _engine_factory = staticmethod(ImOracleEngine)


def acc(s):
    """The sampler's `ImportanceAccumulator` (None: the option is off)."""
    return next((p for p in s._products if p.name == "importance"), None)


def make(prefix=None, max_samples=30000, resume=False, **opts):
    o = {"seed": 21, "n_walkers": 128, "group_size": 64, "steps_per_launch": 40,
         "max_samples": max_samples, "Rminus1_stop": 0.0, "learn_every": "20d",
         "snapshot_every": 40, "importance": OPT}
    o.update(opts)
    return OnDouble(o, ProblemSpec.from_info(QUICK), output=prefix, resume=resume)


# ------------------------------------------------------------------------------- the option
def test_the_option_parses_to_named_alternatives():
    import torch
    assert HIP_DEFAULTS["importance"] is None
    assert parse_option(None, ["a", "b"]) is None and parse_option(False, ["a", "b"]) is None
    cfg = parse_option({**OPT, "call": {"function": lambda b, a: a - b, "cov": True}}, ["a", "b"])
    assert [c["name"] for c in cfg] == ["bao", "tight", "call"] and [c["cov"] for c in cfg] == [True, False, True]
    assert [c["function"].args for c in cfg] == [["a"], ["a", "b"], ["b", "a"]]       # bound BY NAME
    a = torch.tensor([0.31, 0.51], dtype=torch.float64)
    assert cfg[0]["function"].function(a).tolist() == [0.0, -0.5]
    assert cfg[2]["function"].function(a, 2 * a).tolist() == [0.31, 0.51]
    # cov defaults to d <= 128
    many = ["p%d" % i for i in range(129)]
    assert parse_option({"x": {"function": "lambda p0: p0"}}, many)[0]["cov"] is False
    assert parse_option({"x": {"function": "lambda p0: p0"}}, many[:128])[0]["cov"] is True
    assert parse_option({"x": {"function": "lambda p0: p0", "cov": False}}, many[:3])[0]["cov"] is False


class NeverBuilt(ImOracleEngine):
    def __init__(self, *a, **k):
        raise AssertionError("the option must be refused before the engine is created")


class Refusing(MCMCHip):
    _engine_factory = staticmethod(NeverBuilt)


@pytest.mark.parametrize("opt, match", [
    ({}, "importance: expected None or a dict of 1..8 named alternatives"),
    (True, "importance: expected None or a dict"),
    ({"k%d" % i: {"function": BAO} for i in range(9)}, "importance: at most 8 alternatives are served, not 9"),
    ({"bao": BAO}, "importance: alternative 'bao': expected a dict with the key 'function'"),
    ({"bao": {"cov": True}}, "importance: alternative 'bao': no 'function'"),
    ({"bao": {"function": BAO, "every": 2}}, r"importance: alternative 'bao': unknown key\(s\) \['every'\]"),
    ({"bao": {"function": BAO, "cov": 1}}, "importance: alternative 'bao': cov must be True, False or None"),
    ({"bao": {"function": "lambda q: q"}}, "importance: alternative 'bao': argument 'q' is not a sampled parameter"),
    ({"bao": {"function": "lambda: 1.0"}}, "importance: alternative 'bao': its function takes no arguments"),
    ({"bao": {"function": "lambda *a: a[0]"}}, "importance: parameter 'bao': the derived function takes \\*a"),
    ({"bao": {"function": "lambda a: ("}}, "importance: parameter 'bao': the derived function .* could not be evaluated"),
    ({"bao": {"function": "no.such.module:f"}}, "importance: parameter 'bao': the derived function .* could not be resolved"),
    ({"bao": {"function": 3.5}}, "importance: parameter 'bao': `derived` must be a callable"),
])
def test_refusals_by_name_before_the_engine_is_created(opt, match):
    with pytest.raises(ImportanceError, match=match):
        parse_option(opt, ["a", "b"])
    with pytest.raises(LoggedError, match=match):
        Refusing({"n_walkers": 128, "group_size": 64, "importance": opt}, ProblemSpec.from_info(QUICK))


def test_refusal_of_a_derived_argument_of_cov_above_128_of_a_temperature_and_of_old_engines():
    info = {"likelihood": {"one": None},
            "params": {"a": {"prior": {"min": 0, "max": 1}}, "b": {"prior": {"min": 0, "max": 1}},
                       "s": {"derived": "lambda a, b: a + b"}}}
    from cobaya_amd.derived import ENGINE_METHODS as DERIVED_METHODS

    class WithDerivedRows(MCMCHip):     # (an engine the derived rows themselves are not refused on)
        _engine_factory = staticmethod(type("E", (NeverBuilt,), {m: None for m in DERIVED_METHODS}))
    with pytest.raises(LoggedError, match="importance: alternative 'x': argument 's' is a function-derived "
                                          "parameter, which is out of scope"):
        WithDerivedRows({"n_walkers": 128, "group_size": 64, "importance": {"x": {"function": "lambda s: s"}}},
                 ProblemSpec.from_info(info))
    many = ["p%d" % i for i in range(129)]
    with pytest.raises(ImportanceError, match="importance: alternative 'x': cov: True needs d <= 128, not d = 129"):
        parse_option({"x": {"function": "lambda p0: p0", "cov": True}}, many)
    with pytest.raises(LoggedError, match="importance: the sums weigh the walkers as they are, which at temperature 2"):
        Refusing({"n_walkers": 128, "group_size": 64, "importance": OPT, "temperature": 2}, ProblemSpec.from_info(QUICK))

    class Old(MCMCHip):
        _engine_factory = staticmethod(OracleEngine)    # (no importance entry points)
    with pytest.raises(LoggedError, match="importance: this engine keeps no importance sums"):
        Old({"n_walkers": 128, "group_size": 64, "importance": OPT}, ProblemSpec.from_info(QUICK))
    s = Old({"n_walkers": 128, "group_size": 64}, ProblemSpec.from_info(QUICK))   # off: served as before
    assert "importance" not in s.products()


# ------------------------------------------------------------------------------- the product
def _part(d, cov, G, c, rows, n, counters=(0, 0, 0), n_acc=1):
    """A read-out of ONE alternative: rows [G][n_chains]."""
    return {"sums": np.array(rows, dtype=np.float64).reshape(G * n_chains(d, cov)), "n": np.array([n], np.uint64),
            "counters": np.array([counters], np.uint64), "c": np.array([c]), "n_acc": n_acc}


def test_the_arithmetic_of_the_product_on_crafted_sums():
    """d = 2 with the covariance, two groups, two intervals; by hand.  Chains: S1 S2 M0 M1 V0 V1 Q10."""
    d, G, W = 2, 2, 128
    shift = np.array([1.0, -2.0])
    r0 = [[4.0, 6.0, 2.0, -1.0, 3.0, 2.0, 0.5], [6.0, 9.0, 1.0, 1.0, 2.0, 4.0, -0.5]]
    r1 = [[1.0, 1.0, 0.5, 0.25, 1.0, 1.0, 0.25], [3.0, 2.0, 1.5, -0.75, 2.0, 3.0, 0.75]]
    parts = [_part(d, True, G, 0.5, r0, [60, 64], (4, 3, 0), 1), _part(d, True, G, 0.5 + math.log(2.0), r1, [64, 64], (0, 1, 2), 1)]
    iw = Importance.from_parts(["bao"], ["a", "b"], shift, [True], W, parts)
    C = 0.5 + math.log(2.0)
    tot = 0.5 * np.array(r0) + np.array(r1)                   # interval 0 scaled by exp(c0 - C) = 1 / 2
    tot[:, 1] = 0.25 * np.array(r0)[:, 1] + np.array(r1)[:, 1]    # ... and S2, a sum of squares, by its square
    assert iw.C[0] == C and np.allclose(iw.sums[0], tot, rtol=1e-15)
    S = tot.sum(0)
    n = 60 + 64 + 64 + 64
    assert iw.n_samples == 2 * W and iw.n_used("bao") == n and iw.n_groups == 2
    assert (iw.zero("bao"), iw.nonfinite("bao"), iw.clamped("bao")) == (4, 4, 2)
    assert math.isclose(iw.log_ratio("bao"), C + math.log(S[0] / n), rel_tol=1e-15)
    assert math.isclose(iw.ess("bao"), S[0] ** 2 / S[1], rel_tol=1e-15)
    assert math.isclose(iw.ess_fraction("bao"), S[0] ** 2 / S[1] / n, rel_tol=1e-15)
    m = S[2:4] / S[0]
    assert np.allclose(iw.mean("bao"), shift + m, rtol=1e-15)
    assert np.allclose(iw.var("bao"), S[4:6] / S[0] - m * m, rtol=1e-14)
    assert np.allclose(iw.std("bao"), np.sqrt(S[4:6] / S[0] - m * m), rtol=1e-14)
    want = np.array([[S[4], S[6]], [S[6], S[5]]]) / S[0] - np.outer(m, m)
    assert np.allclose(iw.cov("bao"), want, rtol=1e-14) and np.array_equal(iw.cov("bao"), iw.cov("bao").T)
    # the jackknives: delete one group
    ng = np.array([124.0, 128.0])
    loo = np.log((S[0] - tot[:, 0]) / (n - ng))
    assert math.isclose(iw.log_ratio_stderr("bao"), math.sqrt(0.5 * ((loo - loo.mean()) ** 2).sum()), rel_tol=1e-13)
    lm = (S[2:4] - tot[:, 2:4]) / (S[0] - tot[:, 0])[:, None]
    assert np.allclose(iw.mean_stderr("bao"), np.sqrt(0.5 * ((lm - lm.mean(0)) ** 2).sum(0)), rtol=1e-13)
    lines = iw.summary().splitlines()
    assert len(lines) == 1 and "Importance bao" in lines[0] and "clamped" in lines[0] and "WARNING" in lines[0]
    with pytest.raises(KeyError, match="no alternative 'tight'"):
        iw.mean("tight")
    # an interval without an accumulation is skipped, c included
    assert Importance.from_parts(["bao"], ["a", "b"], shift, [True], W,
                                 parts + [_part(d, True, G, 99.0, np.zeros((G, 7)), [0, 0], n_acc=0)]) == iw
    with pytest.raises(ImportanceError, match="importance: the arrays of 1 alternatives and 2 parameters"):
        Importance(["bao"], ["a", "b"], shift, [True], W, 1, [0.0], [np.zeros((2, 6))], [[1, 1]], [0], [0], [0])


def test_centring_constants_1400_apart_underflow_the_smaller_interval_to_zero_and_stay_finite():
    d, G, W = 1, 2, 128
    small = [[5.0, 7.0, 1.0, 2.0], [6.0, 8.0, -1.0, 3.0]]      # S1 S2 M0 V0
    big = [[2.0, 1.5, 0.5, 0.25], [3.0, 2.5, -0.25, 0.5]]
    iw = Importance.from_parts(["x"], ["a"], [0.0], [False], W,
                               [_part(d, False, G, -700.0, small, [64, 64]), _part(d, False, G, 700.0, big, [64, 64])])
    assert iw.C[0] == 700.0 and np.array_equal(iw.sums[0], np.array(big))       # exp(-1400) = 0.0 exactly
    vals = [iw.log_ratio("x"), iw.log_ratio_stderr("x"), iw.ess("x"), *iw.mean("x"), *iw.std("x"), *iw.mean_stderr("x")]
    assert np.all(np.isfinite(vals))
    assert math.isclose(iw.log_ratio("x"), 700.0 + math.log(5.0 / 256), rel_tol=1e-15)    # n counts both intervals
    assert math.isclose(iw.ess("x"), 25.0 / 4.0) and math.isclose(iw.mean("x")[0], 0.05)
    with pytest.raises(ImportanceError, match="importance: alternative 'x' keeps no covariance"):
        iw.cov("x")
    # the order of the intervals does not matter to which one survives
    back = Importance.from_parts(["x"], ["a"], [0.0], [False], W,
                                 [_part(d, False, G, 700.0, big, [64, 64]), _part(d, False, G, -700.0, small, [64, 64])])
    assert back == iw


def test_an_alternative_whose_every_weight_is_zero():
    d, G, W = 2, 2, 128
    parts = [{"sums": np.concatenate((np.zeros(G * 7), np.array([[2.0, 2.0, 1.0, 0.0, 1.0, 1.0],
                                                                  [2.0, 2.0, 0.0, 1.0, 1.0, 1.0]]).reshape(-1))),
              "n": np.array([[64, 64], [64, 64]], np.uint64), "counters": np.array([[128, 0, 0], [0, 0, 0]], np.uint64),
              "c": np.array([0.0, 0.25]), "n_acc": 1}]
    with np.errstate(all="raise"):       # (no warning, no exception on the way)
        iw = Importance.from_parts(["none", "some"], ["a", "b"], [0.0, 0.0], [True, False], W, parts)
        assert iw.log_ratio("none") == -math.inf and math.isnan(iw.log_ratio_stderr("none"))
        assert iw.ess("none") == 0.0 and iw.ess_fraction("none") == 0.0 and iw.zero("none") == 128
        assert np.all(np.isnan(iw.mean("none"))) and np.all(np.isnan(iw.std("none")))
        assert np.all(np.isnan(iw.cov("none"))) and np.all(np.isnan(iw.mean_stderr("none")))
        assert math.isclose(iw.log_ratio("some"), 0.25 + math.log(4.0 / 128)) and iw.ess("some") == 4.0
        lines = iw.summary().splitlines()
    assert len(lines) == 2 and "none" in lines[0] and "WARNING" in lines[0] and "WARNING" in lines[1]
    # nothing used at all
    empty = Importance.from_parts(["x"], ["a"], [0.0], [False], W, [], n_groups=2)
    assert math.isnan(empty.log_ratio("x")) and empty.n_used("x") == 0 and "no walker" in empty.summary()


# ------------------------------------------------------------------------------- shards, files
def _host(W, size=1, rank=0, reduce=None):
    return SimpleNamespace(fail=None, n_walkers=W, size=size, rank=rank, temperature=1.0, snapshot_steps=40,
                           all_reduce_sum=reduce)


def _states(W, d, seeds):
    out = []
    for s in seeds:
        rng = np.random.default_rng(s)
        x = 0.3 * rng.standard_normal((W, d))
        delta = np.stack((-0.5 * ((x[:, 0] - 0.1) / 0.2) ** 2, 1.5 * x[:, 1]))
        delta[:, [5, W // 2 + 9]] = 2.5        # the maximum, once in either half: both shards take the same c
        delta[0, [7, W // 2 + 1]] = [-np.inf, np.nan]
        out.append((x, delta))
    return out


def _run_rule(states, sl, gs, cov, shift):
    rule = Rule(states[0][0].shape[1], sl.stop - sl.start, gs, cov)
    rule.accumulate(states[0][0][sl], states[0][1][:, sl], shift)
    parts = [rule.request(True)]
    for x, dl in states[1:]:
        rule.accumulate(x[sl], dl[:, sl], shift)
    parts.append(rule.request(False))
    return parts


def test_two_shards_merge_to_the_whole_and_combine_through_the_all_reduce():
    spec = ProblemSpec.from_info(QUICK)
    d, W, gs, cov, shift = 2, 256, 64, [True, False], np.array([0.05, -0.02])
    states = _states(W, d, (1, 2, 3))
    whole = _run_rule(states, slice(0, W), gs, cov, shift)
    halves = [_run_rule(states, slice(0, W // 2), gs, cov, shift), _run_rule(states, slice(W // 2, W), gs, cov, shift)]
    assert whole[0]["c"].tolist() == [2.5, 2.5] and np.array_equal(halves[1][1]["c"], whole[1]["c"])
    cfg = parse_option({"g": {"function": "lambda a: a"}, "l": {"function": "lambda b: b", "cov": False}}, spec.sampled)

    def product(parts, host):
        a = ImportanceAccumulator(cfg, spec, host)
        a.ivs, a.open, a.shift, a.G = [parts[0]], parts[1], shift, len(parts[0]["n"][0])
        return a, a.product([], combined=host.size > 1)

    ref = product(whole, _host(W))[1]
    assert ref.n_acc == 3 and ref.n_groups == 4 and ref.n_samples == 3 * W
    assert ref.zero("g") == 3 and ref.nonfinite("g") == 3 and ref.nonfinite("l") == 0
    pa, pb = (product(h, _host(W // 2))[1] for h in halves)
    both = pa.merge(pb)
    assert both == ref and pa != ref and pa.n_groups == 2
    for name in ("g", "l"):      # a shard's groups are bit for bit the same groups of the whole ensemble
        assert both.log_ratio(name) == ref.log_ratio(name) and both.log_ratio_stderr(name) == ref.log_ratio_stderr(name)
        assert both.ess(name) == ref.ess(name) and np.array_equal(both.mean(name), ref.mean(name))
    assert np.array_equal(both.cov("g"), ref.cov("g"))
    # shards with DIFFERENT centring constants meet at the larger one
    lower = Importance(pb.names, pb.params, pb.shift, pb.cov_kept, pb.n_walkers, pb.n_acc, pb.C - 1.0,
                       [s * np.where(np.arange(s.shape[1]) == 1, math.e ** 2, math.e) for s in pb.sums], pb.n, pb.n_zero, pb.n_nonfinite, pb.n_clamped)
    mixed = pa.merge(lower)
    assert np.array_equal(mixed.C, ref.C) and math.isclose(mixed.log_ratio("g"), ref.log_ratio("g"), rel_tol=1e-14)
    assert np.allclose(mixed.mean("l"), ref.mean("l"), rtol=1e-13)
    with pytest.raises(ImportanceError, match="importance: only shards of one run"):
        pa.merge(Importance(["g"], pa.params, pa.shift, [True], 128, pa.n_acc, pa.C[:1], pa.sums[:1], pa.n[:1],
                            [0], [0], [0]))
    # ... and the same over two processes: the common C first, then each fills its own row
    accs = [product(h, _host(W // 2, 1, rank))[0] for rank, h in enumerate(halves)]

    class _Sent(Exception):
        pass

    # process 0 only sends (recorded); process 1 then reduces against the recorded rows, call by call
    a0, a1 = accs
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
    assert len(sent0) == 2 and not sent0[1].reshape(2, -1)[1].any()
    k = [0]

    def reduce1(buf):
        buf[...] = buf + sent0[k[0]]
        k[0] += 1
    a1.host = _host(W // 2, 2, 1, reduce1)
    assert a1.product([], combined=True) == ref
    assert a1.product([], combined=False).n_groups == 2


def test_save_and_load_of_the_product(tmp_path):
    d, G, W = 2, 2, 128
    rng = np.random.default_rng(3)
    parts = [{"sums": np.abs(rng.standard_normal(G * 7 + G * 6)) + 1.0, "n": np.array([[60, 64], [64, 63]], np.uint64),
              "counters": np.array([[1, 4, 0], [0, 1, 2]], np.uint64), "c": np.array([0.5, -3.0]), "n_acc": 2}]
    iw = Importance.from_parts(["bao", "tight"], ["a", "b"], [0.25, -1.0], [True, False], W, parts)
    p = str(tmp_path / "i.npz")
    iw.save(p)
    back = Importance.load(p)
    assert back == iw and back.log_ratio("tight") == iw.log_ratio("tight") and back.clamped("tight") == 2
    assert np.array_equal(back.cov("bao"), iw.cov("bao")) and back.n_samples == 2 * W
    z = np.load(p)
    assert float(z["log_ratio"][0]) == iw.log_ratio("bao") and np.array_equal(z["mean"][1], iw.mean("tight"))
    other = Importance.from_parts(["bao", "tight"], ["a", "b"], [0.25, -1.0], [True, False], W,
                                  [dict(parts[0], c=np.array([0.5, -2.0]))])
    assert other != iw and iw != "importance"


# ------------------------------------------------------------------------------- the window
def test_a_run_on_the_double_follows_the_window_and_writes_the_file(tmp_path):
    p = str(tmp_path / "a")
    s = make(p, max_samples=60000)
    s.run()
    a, log = acc(s), s.engine.im_log
    assert len(s.progress) >= 5 and s._dropped_snapshots > 0          # intervals were dropped
    assert len(a.ivs) == len(s._intervals)
    assert all(iv["n_acc"] == w[0] for iv, w in zip(a.ivs, s._intervals))
    steps = [e[1] for e in log if e[0] == "acc"]
    n_snap = s._dropped_snapshots + sum(iv[0] for iv in s._intervals) + s._snaps_in_interval
    assert steps == [40 * k for k in range(1, n_snap + 1)]            # beside every moment snapshot
    cs = np.array([iv["c"] for iv in a.ivs])
    assert np.all(np.isfinite(cs)) and np.all(cs <= 0.0) and len(np.unique(cs[:, 0])) > 1    # a new c per interval
    iw = s.products()["importance"]
    n_open = s.engine._imr.n_acc
    assert iw.n_acc == sum(iv[0] for iv in s._intervals) + n_open and iw.n_samples == iw.n_acc * 128
    assert iw.names == ["bao", "tight"] and iw.params == ["a", "b"] and iw.cov_kept == [True, False]
    assert np.array_equal(iw.shift, s._shift)
    # the posterior N((0.2, 0), [[0.1, 0.05], [0.05, 0.2]]) in a wide box times a Gaussian in a of mean 0.31, sd
    # 0.2: a has precision 1 / 0.1 + 1 / 0.04 and mean (0.2 / 0.1 + 0.31 / 0.04) / that
    prec = 1 / 0.1 + 1 / 0.04
    assert abs(iw.mean("bao")[0] - (0.2 / 0.1 + 0.31 / 0.04) / prec) < 0.05
    assert abs(iw.std("bao")[0] - prec ** -0.5) < 0.04
    assert 0.2 < iw.ess_fraction("bao") < 0.9 and iw.clamped("bao") == 0 and iw.nonfinite("bao") == 0
    assert np.isfinite(iw.log_ratio("tight")) and iw.log_ratio_stderr("tight") > 0
    # a second call moves nothing (the open interval is only peeked at)
    assert s.products(combined=True)["importance"] == iw
    assert Importance.load(p + ".importance.npz") == iw
    s.close()
    assert a.engine is None and a.product(s._intervals) == iw         # the product outlives the engine
    # a new run with the prefix and `force` cleans the file
    OnDouble({"n_walkers": 128, "group_size": 64, "seed": 1}, ProblemSpec.from_info(QUICK), output=p, force=True)
    assert not os.path.exists(p + ".importance.npz")


def test_a_resume_in_mid_interval_ends_bit_identical_and_both_resume_refusals(tmp_path):
    one = make(str(tmp_path / "a"), 40000)
    one.run()
    p = str(tmp_path / "b")
    b1 = make(p, 20000)
    b1.run()
    z = np.load(p + ".1.state.npz", allow_pickle=False)
    n_iv, G, n_sums = len(z["iv_n"]), 2, 2 * (7 + 6)
    owned = {"iw_names": (None, (2,)), "iw_cov": (np.int64, (2,)), "iw_shift": (np.float64, (2,)),
             "iw_iv_sums": (np.float64, (n_iv, n_sums)), "iw_iv_n": (np.uint64, (n_iv, 2, G)),
             "iw_iv_counters": (np.uint64, (n_iv, 2, 3)), "iw_iv_c": (np.float64, (n_iv, 2)),
             "iw_iv_nacc": (np.int64, (n_iv,)), "iw_open_sums": (np.float64, (1, n_sums)),
             "iw_open_n": (np.uint64, (1, 2, G)), "iw_open_counters": (np.uint64, (1, 2, 3)),
             "iw_open_c": (np.float64, (1, 2)), "iw_open_nacc": (np.int64, (1,))}
    assert {k for k in z.files if k.startswith("iw_")} == set(owned)
    for k, (dtype, shape) in owned.items():
        assert z[k].shape == shape and (dtype is None or z[k].dtype == np.dtype(dtype)), (k, z[k].dtype, z[k].shape)
    assert int(z["iw_open_nacc"][0]) > 0 and z["iw_open_sums"].any()     # stopped in mid-interval
    first = Importance.load(p + ".importance.npz")
    assert first == b1.products()["importance"]
    b2 = make(p, 40000, resume=True)
    r = b2.engine._imr
    assert r.n_acc == int(z["iw_open_nacc"][0]) and np.array_equal(r.sums[0].reshape(-1), z["iw_open_sums"][0][:2 * 7])
    assert np.array_equal(r.c, z["iw_open_c"][0])                     # c included: no new maximum is taken
    b2.run()
    got, ref = b2.products()["importance"], one.products()["importance"]
    assert got == ref and all(a.tobytes() == b.tobytes() for a, b in zip(got.sums, ref.sums))
    assert got.log_ratio("bao") == ref.log_ratio("bao") and got.n_samples > first.n_samples
    assert Importance.load(p + ".importance.npz") == got
    other = {"bao": OPT["bao"], "loose": OPT["tight"]}
    flipped = {"bao": {"function": BAO, "cov": False}, "tight": OPT["tight"]}
    for opt in (other, flipped, {"bao": OPT["bao"]}):
        with pytest.raises(LoggedError, match="importance: cannot resume -- the run was written with the alternatives"):
            make(p, 50000, resume=True, importance=opt)
    # ... and a run that was written without the option
    q = str(tmp_path / "c")
    make(q, 5000, importance=None).run()
    zq = np.load(q + ".1.state.npz", allow_pickle=False)
    assert not [k for k in zq.files if k.startswith("iw_")] and not os.path.exists(q + ".importance.npz")
    with pytest.raises(LoggedError, match="importance: cannot resume -- the run was written without importance"):
        make(q, 9000, resume=True)


class Untouchable(ImOracleEngine):
    """Every importance method raises: a run without the option must call none of them."""


for _name in ("configure_importance", "importance_layout", "importance_row_views", "accumulate_importance",
              "request_importance", "fetch_importance", "importance_set"):
    def _raises(self, *a, _n=_name, **k):
        raise AssertionError(f"{_n} was called without the option")
    setattr(Untouchable, _name, _raises)


def test_a_run_without_the_option_never_touches_the_importance_methods(tmp_path):
    class Off(MCMCHip):
        _engine_factory = staticmethod(Untouchable)
    p = str(tmp_path / "d")
    s = Off({"seed": 21, "n_walkers": 128, "group_size": 64, "steps_per_launch": 40, "max_samples": 8000,
             "Rminus1_stop": 0.0, "learn_every": "20d", "snapshot_every": 40}, ProblemSpec.from_info(QUICK), output=p)
    s.run()
    assert acc(s) is None and "importance" not in s.products()
    s.close()
    Off({"seed": 21, "n_walkers": 128, "group_size": 64, "steps_per_launch": 40, "max_samples": 12000,
         "Rminus1_stop": 0.0, "learn_every": "20d", "snapshot_every": 40}, ProblemSpec.from_info(QUICK), output=p,
        resume=True).run()


def test_a_function_that_misbehaves_is_named():
    import torch
    for fn, match in ((lambda a: a.sum(), "importance: alternative 'x': its function must return shape"),
                      (lambda a: a.float(), "importance: alternative 'x': its function must return dtype"),
                      (lambda a: a.numpy(), "importance: alternative 'x': its function must return a torch.Tensor"),
                      (lambda a: a / torch.zeros(3), "importance: alternative 'x': its function raised RuntimeError")):
        s = make(importance={"x": {"function": fn}})
        with pytest.raises(Exception, match=match):
            s.run()
