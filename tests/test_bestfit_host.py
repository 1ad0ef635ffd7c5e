"""Best fit, MAP and profile likelihoods, host side (no GPU): the ordering key, the merge rule, the
`BestFit` product, the parsing of the sampler option `bestfit`, the merge over processes, and the
window bookkeeping of the sampler on an oracle-backed engine double that serves the best-fit
methods in numpy (tests/bestfit_ref.py: THE REFERENCE, the rule of DESIGN.md section 2 "Best fit
and profiles").  Every comparison is on keys and integers, bit for bit."""
import os
from types import SimpleNamespace

import numpy as np
import pytest

from cobaya_amd.bestfit import (BestFit, BestFitAccumulator, BestFitError, empty_records, key_of,
                                merge_records, parse_option, value_of)
from cobaya_amd.model import ProblemSpec
from cobaya_amd.sampler import LoggedError, MCMCHip
from tests.bestfit_ref import BfOracleEngine, rule_key, rule_merge_records, rule_over
from tests.oracle_engine import OracleEngine
from tests.test_host_logic import QUICK


class OnDouble(MCMCHip):
    _engine_factory = staticmethod(BfOracleEngine)


def acc(s):
    """The sampler's `BestFitAccumulator` (None: the option is off)."""
    return next((p for p in s._products if p.name == "bestfit"), None)


def make(prefix=None, max_samples=30000, resume=False, **opts):
    o = {"seed": 21, "n_walkers": 128, "group_size": 64, "steps_per_launch": 40,
         "max_samples": max_samples, "Rminus1_stop": 0.0, "learn_every": "20d",
         "snapshot_every": 40, "bestfit": {"params": "all", "bins": 16}}
    o.update(opts)
    return OnDouble(o, ProblemSpec.from_info(QUICK), output=prefix, resume=resume)


# ------------------------------------------------------------------------------- the key
SPECIALS = [-np.inf, -1e300, -1.0, -2.2250738585072014e-308, -5e-324, -0.0, 0.0, 5e-324,
            2.2250738585072014e-308, 1.0, 1e300, np.inf]     # ascending; denormals on either side of +-0


def test_the_key_orders_like_the_doubles_and_skips_nan():
    keys = key_of(SPECIALS)
    assert keys.dtype == np.uint64 and np.array_equal(keys, rule_key(SPECIALS))
    assert np.all(keys[1:] > keys[:-1])                    # strictly: -0.0 < +0.0 as well
    assert int(keys[0]) == 0x000FFFFFFFFFFFFF and int(keys[0]) > 0     # -inf: the smallest non-empty key
    assert int(key_of([-0.0])[0]) == 0x7FFFFFFFFFFFFFFF and int(key_of([0.0])[0]) == 0x8000000000000000
    nans = np.array([np.nan, -np.nan, np.float64(np.nan)])
    nans = np.concatenate((nans, np.array([0xFFFFFFFFFFFFFFFF, 0x7FF0000000000001], np.uint64).view(np.float64)))
    assert not key_of(nans).any() and not rule_key(nans).any()
    back = value_of(keys)
    assert np.array_equal(back.view(np.uint64), np.array(SPECIALS).view(np.uint64))      # bit for bit, the sign of zero too
    assert np.isnan(value_of(np.zeros(1, np.uint64))[0])
    rng = np.random.default_rng(3)
    v = rng.standard_normal(4000) * 10.0 ** rng.integers(-300, 300, 4000)
    k = key_of(v)
    assert np.array_equal(np.argsort(k, kind="stable"), np.argsort(v, kind="stable"))
    assert np.array_equal(k, rule_key(v)) and np.array_equal(value_of(k), v)


def _rec(d, map_=None, best=None):
    """Records with (value, walker, step) per row; x = walker + 0.5 in every coordinate."""
    out = empty_records(d)
    for r, t in enumerate((map_, best)):
        if t is None:
            continue
        v, w, step = t
        out[r, 0] = key_of([v])[0]
        out[r, 1], out[r, 2] = w, step
        out[r, 3:6] = np.array([v, -1.0, v + 1.0]).view(np.uint64)
        out[r, 6:] = np.full(d, w + 0.5).view(np.uint64)
    return out


def test_the_merge_rule_with_ties():
    d = 3
    a = _rec(d, (1.0, 7, 100), (2.0, 9, 40))
    for b, rows in [
        (_rec(d, (1.5, 8, 200), (1.0, 1, 1)), ("b", "a")),          # the greater key wins, whatever the step
        (_rec(d, (1.0, 3, 100), (2.0, 9, 41)), ("b", "a")),         # a tie: lower step, then lower walker
        (_rec(d, (1.0, 7, 99), (2.0, 10, 40)), ("b", "a")),
        (_rec(d, (1.0, 2, 101), (2.0, 8, 40)), ("a", "b")),
        (_rec(d, None, (-np.inf, 0, 0)), ("a", "a")),               # empty loses; -inf loses to 2.0
        (_rec(d, (-0.0, 1, 1), None), ("a", "a")),
    ]:
        want = np.array([(a if rows[r] == "a" else b)[r] for r in range(2)])
        assert np.array_equal(merge_records(a, b), want)
        assert np.array_equal(merge_records(b, a), want)            # symmetric
        assert np.array_equal(rule_merge_records(a, b), want)
    e = empty_records(d)
    assert np.array_equal(merge_records(e, a), a) and np.array_equal(merge_records(e, e), e)
    z = _rec(d, (-0.0, 5, 5), (-np.inf, 5, 5))
    assert np.array_equal(merge_records(z, _rec(d, (0.0, 6, 6), None))[0], _rec(d, (0.0, 6, 6))[0])   # -0.0 < +0.0
    assert np.array_equal(merge_records(e, z), z)                   # -inf is not empty


# ------------------------------------------------------------------------------- BestFit
def _filled(quantity="loglike", seed=5, n=3000, walker_offset=0, step=17):
    rng = np.random.default_rng(seed)
    x = np.column_stack((rng.normal(0.3, 0.2, n), rng.uniform(-1, 1, n)))
    ll = -0.5 * ((x[:, 0] - 0.3) / 0.2) ** 2 - 0.5 * (x[:, 1] / 0.4) ** 2
    lpr = -0.1 * x[:, 1] ** 2
    st = {"x": x, "logpost": ll + lpr, "logprior": lpr, "loglike": ll, "step": step}
    lo, hi = [-0.2, -0.5], [1.0, 0.5]
    slab, rec, _ = rule_over([st], 2, [0, 1], 24, lo, hi, quantity, walker_offset)
    b = BestFit(["a", "b"], ["a", "b"], 24, {"a": (lo[0], hi[0]), "b": (lo[1], hi[1])}, quantity, slab, rec, 1, n)
    return b, st, lo, hi


def test_records_profiles_and_intervals_of_a_known_population():
    b, st, lo, hi = _filled()
    w = int(np.argmax(st["loglike"]))
    r = b.bestfit
    assert (r.walker, r.step) == (w, 17) and r.loglike == st["loglike"][w] and r.chi2 == -2.0 * r.loglike
    assert r.logprior == st["logprior"][w] and r.logpost == st["logpost"][w]
    assert np.array_equal(r.x, st["x"][w]) and r.point == {"a": st["x"][w, 0], "b": st["x"][w, 1]}
    m = b.map
    assert m.walker == int(np.argmax(st["logpost"])) and m.logpost == st["logpost"].max()
    for i, name in enumerate(("a", "b")):
        p = b.profile(name)
        assert p.shape == (24,) and p.dtype == np.float64
        assert np.array_equal(b.edges(name), np.linspace(lo[i], hi[i], 25))
        e = b.edges(name)
        for k in range(24):     # the definition, by hand: edges are exact enough away from ties here
            inb = (st["x"][:, i] >= lo[i]) & (st["x"][:, i] <= hi[i]) & \
                  (np.minimum(np.floor((st["x"][:, i] - lo[i]) * (24 / (hi[i] - lo[i]))), 23) == k)
            assert (np.isnan(p[k]) and not inb.any()) or p[k] == st["loglike"][inb].max()
        dc = b.delta_chi2(name)
        assert np.nanmin(dc) == 0.0 and np.all(dc[~np.isnan(dc)] >= 0)
        a_, b_ = b.interval(name)
        inside = np.flatnonzero(dc <= 1.0)
        assert (a_, b_) == (e[inside[0]], e[inside[-1] + 1])
        wide = b.interval(name, delta=4.0)
        assert wide[0] <= a_ and wide[1] >= b_
    # one sigma of a: 0.2 around 0.3 -- the interval is that, to the bins (0.05 wide) and the sampling
    a_, b_ = b.interval("a")
    assert 0.05 <= a_ <= 0.15 and 0.45 <= b_ <= 0.55
    assert "best fit chi2" in b.summary() and "MAP" in b.summary() and "\n" not in b.summary()
    with pytest.raises(KeyError, match="no profile"):
        b.profile("c")
    empty = BestFit(["a", "b"], ["a"], 4, {"a": (0, 1)})
    assert empty.map is None and empty.bestfit is None and np.all(np.isnan(empty.profile("a")))
    assert "nothing" in empty.summary()
    with pytest.raises(BestFitError, match="bestfit: no sample"):
        empty.delta_chi2("a")
    only = BestFit(["a", "b"], [], 64, {})
    assert only.slab.shape == (0, 0) and only.records.shape == (2, 8)


def test_merge_refuses_other_layouts_and_files_round_trip(tmp_path):
    b, st, lo, hi = _filled()
    c, st2, *_ = _filled(seed=6, walker_offset=3000, step=18)
    both = b.merge(c)
    assert np.array_equal(both.slab, np.maximum(b.slab, c.slab)) and both.n_samples == 6000
    assert both.n_accumulations == 2
    assert both.bestfit.loglike == max(st["loglike"].max(), st2["loglike"].max())
    assert both.merge(b) .slab.tobytes() == both.slab.tobytes()
    assert b.merge(b).records.tobytes() == b.records.tobytes()
    rng_other = BestFit(["a", "b"], ["a", "b"], 24, {"a": (lo[0], hi[0] + 1e-9), "b": (lo[1], hi[1])})
    for other in (rng_other, BestFit(["a", "b"], ["a", "b"], 12, b.ranges),
                  BestFit(["a", "b"], ["b", "a"], 24, b.ranges),
                  BestFit(["a", "b"], ["a", "b"], 24, b.ranges, "logpost")):
        with pytest.raises(BestFitError, match="same layout"):
            b.merge(other)
    path = str(tmp_path / "m.bestfit.npz")
    b.save(path)
    back = BestFit.load(path)
    assert back == b and back.slab.dtype == np.uint64 and back.records.dtype == np.uint64
    assert back.ranges == b.ranges and back.quantity == "loglike" and back != both
    only = BestFit(["a", "b"], [], 64, {}, "logpost", records=b.records)
    only.save(path)
    assert BestFit.load(path) == only and BestFit.load(path).map.walker == b.map.walker
    assert not os.path.exists(path + ".npz")


# ------------------------------------------------------------------------------- the option
def test_every_shorthand_of_the_option():
    names = ["a", "b", "c"]
    assert parse_option(None, names) is None and parse_option(False, names) is None
    t = parse_option(True, names)
    assert t == {"params": names, "bins": 64, "ranges": "prior", "quantity": "loglike"}
    assert parse_option({}, names) == t and parse_option({"params": "all"}, names) == t
    rec = parse_option({"params": None, "quantity": "logpost"}, names)
    assert rec["params"] == [] and rec["quantity"] == "logpost"
    one = parse_option({"params": ["c"], "bins": 1024, "ranges": {"c": [0, 2]}}, names)
    assert one["params"] == ["c"] and one["bins"] == 1024 and one["ranges"] == {"c": (0.0, 2.0)}
    cfg = acc(make(bestfit=True)).cfg
    assert cfg["params"] == ["a", "b"] and cfg["bins"] == 64 and cfg["quantity"] == "loglike"
    assert cfg["resolved"] == {"a": (-0.5, 3.0), "b": (-5.0, 5.0)}       # "prior": bounds; loc +- 5 scale
    s = make(bestfit=None)
    assert acc(s) is None and s.engine._bfr is None and "bestfit" not in s.products()
    s = make(bestfit={"params": None})
    assert s.engine.bestfit_layout() == {"on": 1, "n": 0, "bins": 0, "quantity": "loglike", "n_slab": 0,
                                         "n_records": 16}
    s = make(bestfit={"params": ["b"], "ranges": "covmat", "quantity": "logpost"})
    centre, sig = s._shift, np.sqrt(np.diag(s._initial_covmat))
    assert acc(s).cfg["resolved"] == {"b": (centre[1] - 5 * sig[1], centre[1] + 5 * sig[1])}
    assert s.engine._bf_cfg["dims"] == [1] and s.engine._bf_cfg["quantity"] == "logpost"
    make(bestfit=True, temperature=2)          # served at any temperature


class NeverBuilt(BfOracleEngine):
    def __init__(self, *a, **k):
        raise AssertionError("the option must be refused before the engine is created")


class Refusing(MCMCHip):
    _engine_factory = staticmethod(NeverBuilt)


@pytest.mark.parametrize("opt, match", [
    ({"params": ["a", "nope"]}, r"bestfit: unknown parameter name\(s\) \['nope'\]"),
    ({"params": ["a", "a"]}, "bestfit: params lists a parameter twice"),
    ({"params": "some"}, "bestfit: params must be"),
    ({"bins": 1025}, "bestfit: bins must be an integer in 1..1024"),
    ({"bins": 0}, "bestfit: bins must be"),
    ({"bins": 2.5}, "bestfit: bins must be"),
    ({"ranges": {"a": [1, 1]}}, r"bestfit: ranges\['a'\] must be a finite \[lo, hi\]"),
    ({"ranges": {"q": [0, 1]}}, "bestfit: ranges names unknown"),
    ({"ranges": "posterior"}, "bestfit: ranges must be"),
    ({"quantity": "chi2"}, "bestfit: quantity must be one of"),
    ({"binz": 3}, r"bestfit: unknown key\(s\) \['binz'\]"),
    ("all", "bestfit: expected True, None or a dict"),
])
def test_refusals_by_name_before_the_engine_is_created(opt, match):
    with pytest.raises(LoggedError, match=match):
        Refusing({"n_walkers": 128, "group_size": 64, "bestfit": opt}, ProblemSpec.from_info(QUICK))


def test_refusal_of_engines_without_the_methods():
    class Old(MCMCHip):
        _engine_factory = staticmethod(OracleEngine)    # (no best-fit entry points)
    with pytest.raises(LoggedError, match="bestfit: this engine keeps no best fit"):
        Old({"n_walkers": 128, "group_size": 64, "bestfit": True}, ProblemSpec.from_info(QUICK))
    Old({"n_walkers": 128, "group_size": 64}, ProblemSpec.from_info(QUICK))   # off: served as before


# ------------------------------------------------------------------------------- several processes
def test_two_ranks_combine_through_one_all_reduce_sum():
    spec = ProblemSpec.from_info(QUICK)
    parts = [_filled(seed=11, walker_offset=0, step=40), _filled(seed=12, walker_offset=3000, step=40)]
    # ... with a tie on the bestfit key across the ranks: the lower walker id (rank 0's) must win
    parts[1][0].records[1] = parts[0][0].records[1]
    parts[1][0].records[1, 1] = 3000 + 5
    sent, accs = [], []
    for rank, (b, *_x) in enumerate(parts):
        host = SimpleNamespace(fail=None, n_walkers=3000, size=2, rank=rank, temperature=1.0, snapshot_steps=40,
                               all_reduce_sum=lambda buf: sent.append(buf.copy()))
        a = BestFitAccumulator(parse_option({"params": "all", "bins": 24}, spec.sampled), spec, host)
        a.cfg["resolved"] = dict(b.ranges)
        a.open = (b.slab.copy(), b.records.copy(), 1)
        a.product([], combined=True)          # (records what this rank sends)
        accs.append(a)
    assert len(sent) == 2 and sent[0].dtype == np.float64 and sent[0].shape == sent[1].shape
    n_words = 2 * 24 + 2 * 8
    assert sent[0].size == 2 * (2 * n_words + 1)
    m0, m1 = sent[0].reshape(2, -1), sent[1].reshape(2, -1)
    assert not m0[1].any() and not m1[0].any()                       # each fills its own row of a zero matrix
    assert np.all(m0 < 2.0 ** 32) and np.all(m0 == np.floor(m0))    # 32-bit halves: exact in float64
    total = sent[0] + sent[1]

    def summed(buf):
        buf[...] = total
    want = parts[0][0].merge(parts[1][0])
    for a in accs:
        a.host.all_reduce_sum = summed
        got = a.product([], combined=True)
        assert np.array_equal(got.slab, want.slab) and np.array_equal(got.records, want.records)
        assert got.n_samples == 6000 and got.n_accumulations == 1
        assert got.bestfit.walker == int(parts[0][0].records[1, 1])
        alone = a.product([], combined=False)
        assert alone.n_samples == 3000 and not np.array_equal(alone.slab, want.slab)


# ------------------------------------------------------------------------------- the window
def _expected(s):
    """The rule applied to exactly the states the moment window holds (everything after the
    dropped snapshots) plus the unfinished interval."""
    eng = s.engine
    states = eng.bf_states[s._dropped_snapshots:]
    return rule_over(states, eng.d, walker_offset=eng.walker_offset, **eng._bf_cfg)


def test_product_holds_the_window_of_the_moments_and_nothing_older():
    s = make(max_samples=60000)
    s.run()
    assert len(s.progress) >= 5 and s._dropped_snapshots > 0 and s._iv0 > 0   # intervals were dropped
    assert len(acc(s).ivs) == len(s._intervals)
    b = s.products()["bestfit"]
    slab, rec, n = _expected(s)
    assert n == sum(iv[0] for iv in s._intervals) + s._snaps_in_interval < len(s.engine.bf_states)
    assert np.array_equal(b.slab, slab) and np.array_equal(b.records, rec) and b.slab.dtype == np.uint64
    assert b.n_accumulations == n and b.n_samples == n * 128
    # the record is a walker of a recorded state, whole
    r = b.bestfit
    st = next(t for t in s.engine.bf_states if t["step"] == r.step)
    assert np.array_equal(st["x"][r.walker], r.x) and st["loglike"][r.walker] == r.loglike
    assert r.step > s.engine.bf_states[s._dropped_snapshots - 1]["step"]        # ... of the window
    assert r.loglike == max(t["loglike"].max() for t in s.engine.bf_states[s._dropped_snapshots:])
    # a second call moves nothing (the unfinished interval is held on the host by then)
    assert s.products(combined=True)["bestfit"] == b
    a = acc(s)
    s.close()
    assert a.engine is None and a.product(s._intervals) == b      # the product outlives the engine


def test_a_resume_in_mid_interval_ends_bit_identical(tmp_path):
    one = make(str(tmp_path / "a"), 40000)
    one.run()
    p = str(tmp_path / "b")
    b1 = make(p, 20000)
    b1.run()
    z = np.load(p + ".1.state.npz", allow_pickle=False)
    n_iv = len(z["iv_n"])
    U = np.dtype("<U1")
    owned = {"bf_params": (U, (2,)), "bf_bins": (np.int64, (2,)), "bf_ranges": (np.float64, (2, 2)),
             "bf_iv_slab": (np.uint64, (n_iv, 2, 16)), "bf_iv_rec": (np.uint64, (n_iv, 2, 8)),
             "bf_open_slab": (np.uint64, (2, 16)), "bf_open_rec": (np.uint64, (2, 8)), "bf_open_n": (np.int64, ())}
    assert {k for k in z.files if k.startswith("bf_")} == set(owned)
    for k, (dtype, shape) in owned.items():
        assert (z[k].dtype, z[k].shape) == (np.dtype(dtype), shape), (k, z[k].dtype, z[k].shape)
    assert z["bf_params"].tolist() == ["a", "b"] and z["bf_bins"].tolist() == [16, 0]
    assert int(z["bf_open_n"]) > 0 and z["bf_open_slab"].any() and z["bf_open_rec"][:, 0].all()   # stopped in mid-interval
    first = BestFit.load(p + ".bestfit.npz")
    assert first == b1.products()["bestfit"]
    b2 = make(p, 40000, resume=True)
    assert b2.engine._bfr.n == int(z["bf_open_n"])      # the unfinished interval is back on the device
    assert np.array_equal(b2.engine._bfr.records, z["bf_open_rec"])
    b2.run()
    got, ref = b2.products()["bestfit"], one.products()["bestfit"]
    assert got == ref and got.slab.tobytes() == ref.slab.tobytes() and got.records.tobytes() == ref.records.tobytes()
    assert got.n_accumulations > first.n_accumulations
    assert BestFit.load(p + ".bestfit.npz") == got
    slab, rec, n = _expected(one)
    assert np.array_equal(ref.slab, slab) and np.array_equal(ref.records, rec) and ref.n_accumulations == n
    # the layout is part of the resume geometry
    for other in ({"params": "all", "bins": 16, "ranges": {"a": [0, 1]}}, {"params": "all", "bins": 32},
                  {"params": "all", "bins": 16, "quantity": "logpost"}, {"params": ["a"], "bins": 16}):
        with pytest.raises(LoggedError, match="bestfit: cannot resume"):
            make(p, 50000, resume=True, bestfit=other)


def test_off_writes_no_key_and_the_output_file_is_cleaned(tmp_path):
    p = str(tmp_path / "c")
    make(p, 5000, bestfit=None).run()
    z = np.load(p + ".1.state.npz", allow_pickle=False)
    assert not [k for k in z.files if k.startswith("bf_")] and not os.path.exists(p + ".bestfit.npz")
    with pytest.raises(LoggedError, match="bestfit: cannot resume -- the run was written without"):
        make(p, 9000, resume=True)
    p = str(tmp_path / "d")
    make(p, 5000).run()
    assert os.path.exists(p + ".bestfit.npz")
    OnDouble({"n_walkers": 128, "group_size": 64, "seed": 1}, ProblemSpec.from_info(QUICK), output=p, force=True)
    assert not os.path.exists(p + ".bestfit.npz")
