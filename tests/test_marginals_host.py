"""Streaming marginal histograms, host side (no GPU): the `Marginals` product, the parsing of the
sampler option `marginals`, and the window bookkeeping of the sampler on an oracle-backed engine
double that serves the five marginal methods in numpy.

THE REFERENCE of every count in this file and in tests/test_gpu_marginals.py is `rule_slab`: the
rule of DESIGN.md section 2 ("Marginals") written in numpy with the operations of the kernel --
`np.floor((x - lo) * s)`, `np.minimum`, and masks.  It is deliberately NOT `np.histogram`, which
treats values within an ulp of an edge differently (it compares with the edges it formed by
`linspace`; the rule multiplies by s = B / (hi - lo))."""
import os

import numpy as np
import pytest

from cobaya_amd.marginals import Marginals, MarginalsError, parse_option, slab_size
from cobaya_amd.model import ProblemSpec
from cobaya_amd.sampler import LoggedError, MCMCHip
from tests.oracle_engine import OracleEngine
from tests.test_host_logic import QUICK


# ------------------------------------------------------------------------------- the rule
def rule_bins(x, lo, hi, B):
    """(in-range mask, bin of every value; the bin of an out-of-range value is meaningless)."""
    x = np.asarray(x, dtype=np.float64)
    s = np.float64(B) / (np.float64(hi) - np.float64(lo))
    inside = (x >= lo) & (x <= hi)
    with np.errstate(invalid="ignore", over="ignore"):
        k = np.minimum(np.floor((x - np.float64(lo)) * s), B - 1)
    return inside, np.where(inside, k, 0).astype(np.int64)


def rule_slab(x, dims1, bins1, pairs, bins2, lo, hi):
    """The uint64 slab one accumulation of the states x[W, d] adds, in the engine's layout:
    per 1-D entry [under, over, c_0 .. c_{B-1}], then per pair [outside, c_00 ..] row-major with the
    pair's first parameter as the row."""
    x = np.asarray(x, dtype=np.float64)
    out = []
    for i in dims1:
        inside, k = rule_bins(x[:, i], lo[i], hi[i], bins1)
        e = np.zeros(bins1 + 2, np.uint64)
        e[0] = np.count_nonzero(x[:, i] < lo[i])
        e[1] = np.count_nonzero(x[:, i] > hi[i])
        e[2:] = np.bincount(k[inside], minlength=bins1)
        out.append(e)
    for i, j in pairs:
        in_i, ki = rule_bins(x[:, i], lo[i], hi[i], bins2)
        in_j, kj = rule_bins(x[:, j], lo[j], hi[j], bins2)
        inside = in_i & in_j
        e = np.zeros(bins2 * bins2 + 1, np.uint64)
        e[0] = np.count_nonzero(~inside)
        e[1:] = np.bincount(ki[inside] * bins2 + kj[inside], minlength=bins2 * bins2)
        out.append(e)
    return np.concatenate(out) if out else np.zeros(0, np.uint64)


# ------------------------------------------------------------------------------- the double
class MargOracleEngine(OracleEngine):
    """The oracle-backed engine double with the five marginal methods (configure, accumulate,
    request, fetch, set) in numpy; it keeps every accumulated snapshot for the tests."""

    def configure_marginals(self, dims1=(), bins1=128, pairs=(), bins2=32, lo=None, hi=None):
        self._mg = dict(dims1=[int(i) for i in dims1], bins1=int(bins1),
                        pairs=[(int(a), int(b)) for a, b in pairs], bins2=int(bins2),
                        lo=np.array(lo, float), hi=np.array(hi, float))
        n = slab_size(len(self._mg["dims1"]), bins1, len(self._mg["pairs"]), bins2)
        self._mg_slab, self._mg_n, self._mg_req = np.zeros(n, np.uint64), 0, None
        self.snapshots = []

    def accumulate_marginals(self):
        x = self._state.x.copy()
        self.snapshots.append(x)
        self._mg_slab += rule_slab(x, **self._mg)
        self._mg_n += 1

    def request_marginals(self):
        assert self._mg_req is None, "a marginals request is already pending"
        self._mg_req = (self._mg_slab.copy(), self._mg_n)
        self._mg_slab[...] = 0
        self._mg_n = 0

    def fetch_marginals(self):
        out, self._mg_req = self._mg_req, None
        assert out is not None, "no marginals request is pending"
        return out

    def marginals_set(self, counts, n_accumulations):
        self._mg_slab[...] = counts
        self._mg_n = int(n_accumulations)


class OnDouble(MCMCHip):
    _engine_factory = staticmethod(MargOracleEngine)


def acc(s):
    """The sampler's `MarginalsAccumulator` (None: the option is off)."""
    return next((p for p in s._products if p.name == "marginals"), None)


def make(prefix=None, max_samples=30000, resume=False, **opts):
    o = {"seed": 21, "n_walkers": 128, "group_size": 64, "steps_per_launch": 40,
         "max_samples": max_samples, "Rminus1_stop": 0.0, "learn_every": "20d",
         "snapshot_every": 40, "marginals": {"params": "all", "pairs": [["b", "a"]], "bins": 16,
                                             "bins2d": 4}}
    o.update(opts)
    return OnDouble(o, ProblemSpec.from_info(QUICK), output=prefix, resume=resume)


# ------------------------------------------------------------------------------- Marginals
def _filled():
    rng = np.random.default_rng(5)
    x = np.column_stack((rng.normal(0.3, 0.2, 4000), rng.uniform(-1, 1, 4000)))
    lo, hi = [-0.2, -0.5], [1.0, 0.5]
    slab = rule_slab(x, [0, 1], 24, [(1, 0)], 6, lo, hi)
    m = Marginals(["a", "b"], [("b", "a")], 24, 6, {"a": (lo[0], hi[0]), "b": (lo[1], hi[1])},
                  slab, n_accumulations=1, n_samples=4000)
    return m, x, lo, hi


def test_densities_integrate_to_one_and_counts_keep_their_roles():
    m, x, lo, hi = _filled()
    for name, i in (("a", 0), ("b", 1)):
        width = (hi[i] - lo[i]) / 24
        assert np.isclose(m.density(name).sum() * width, 1.0, rtol=1e-14)
        under, over = m.outside(name)
        assert under == np.count_nonzero(x[:, i] < lo[i]) and over == np.count_nonzero(x[:, i] > hi[i])
        assert int(m.counts(name).sum()) + under + over == 4000
        assert np.array_equal(m.edges(name), np.linspace(lo[i], hi[i], 25))
    area = ((hi[0] - lo[0]) / 6) * ((hi[1] - lo[1]) / 6)
    assert np.isclose(m.density2d("b", "a").sum() * area, 1.0, rtol=1e-14)
    c2 = m.counts2d("b", "a")                  # rows follow b, columns a
    inside = (x[:, 0] >= lo[0]) & (x[:, 0] <= hi[0]) & (x[:, 1] >= lo[1]) & (x[:, 1] <= hi[1])
    assert int(c2.sum()) == np.count_nonzero(inside) and m.outside("b", "a") == 4000 - int(c2.sum())
    kb = rule_bins(x[inside, 1], lo[1], hi[1], 6)[1]
    assert np.array_equal(c2.sum(axis=1), np.bincount(kb, minlength=6))
    with pytest.raises(KeyError, match="order"):
        m.counts2d("a", "b")


def test_quantile_inverts_a_known_histogram():
    m = Marginals(["t"], [], 4, 1, {"t": (0.0, 4.0)},
                  np.array([0, 0, 10, 0, 30, 60], np.uint64), 1, 100)
    assert m.quantile("t", 0.05) == pytest.approx(0.5)      # half of the first bin's 10
    assert m.quantile("t", 0.10) == pytest.approx(1.0)
    assert m.quantile("t", 0.25) == pytest.approx(2.5)      # the empty bin is crossed at once
    assert m.quantile("t", 0.70) == pytest.approx(3.5)
    assert m.quantile("t", 1.0) == pytest.approx(4.0)
    np.testing.assert_allclose(m.quantile("t", [0.4, 0.1]), [3.0, 1.0])
    assert m.mean("t") == pytest.approx((10 * 0.5 + 30 * 2.5 + 60 * 3.5) / 100)
    with pytest.raises(MarginalsError, match="quantile"):
        m.quantile("t", 1.5)


def test_sum_refuses_other_layouts_and_files_round_trip(tmp_path):
    m, _, lo, hi = _filled()
    two = m + m
    assert np.array_equal(two.slab, 2 * m.slab) and two.n_samples == 8000 and two.n_accumulations == 2
    other = Marginals(["a", "b"], [("b", "a")], 24, 6, {"a": (lo[0], hi[0] + 1e-9), "b": (lo[1], hi[1])})
    with pytest.raises(MarginalsError, match="same layout"):
        m + other
    with pytest.raises(MarginalsError, match="same layout"):
        m + Marginals(["a", "b"], [("a", "b")], 24, 6, m.ranges)
    with pytest.raises(MarginalsError, match="same layout"):
        m + Marginals(["a", "b"], [("b", "a")], 12, 6, m.ranges)
    path = str(tmp_path / "m.marginals.npz")
    m.save(path)
    back = Marginals.load(path)
    assert back == m and back.slab.dtype == np.uint64 and back.ranges == m.ranges
    assert back.pairs == [("b", "a")]
    only1d = Marginals(["a"], [], 8, 32, {"a": (0.0, 1.0)})
    only1d.save(path)
    assert Marginals.load(path) == only1d


# ------------------------------------------------------------------------------- the option
def test_every_shorthand_of_the_option():
    names = ["a", "b", "c"]
    assert parse_option(None, names) is None and parse_option(False, names) is None
    t = parse_option(True, names)
    assert t == {"params": names, "pairs": [], "bins": 128, "bins2d": 32, "ranges": "prior"}
    assert parse_option({}, names) == t and parse_option({"params": "all", "pairs": None}, names) == t
    allp = parse_option({"params": [], "pairs": "all", "bins2d": 8}, names)
    assert allp["params"] == [] and allp["pairs"] == [("a", "b"), ("a", "c"), ("b", "c")]
    one = parse_option({"params": ["c"], "pairs": [["c", "a"]], "bins": 1024, "bins2d": 64,
                        "ranges": {"c": [0, 2]}}, names)
    assert one["params"] == ["c"] and one["pairs"] == [("c", "a")] and one["ranges"] == {"c": (0.0, 2.0)}
    cfg = acc(make(marginals=True)).cfg
    assert cfg["params"] == ["a", "b"] and cfg["pairs"] == [] and cfg["bins"] == 128
    assert acc(make(marginals=None)) is None and not hasattr(make(marginals=None).engine, "_mg")


def test_the_three_range_modes():
    s = make()       # "prior": the uniform prior's bounds, loc +- 5 scale of the normal one
    assert acc(s).cfg["resolved"] == {"a": (-0.5, 3.0), "b": (-5.0, 5.0)}
    mg = s.engine._mg
    assert mg["dims1"] == [0, 1] and mg["pairs"] == [(1, 0)] and (mg["bins1"], mg["bins2"]) == (16, 4)
    assert np.array_equal(mg["lo"], [-0.5, -5.0]) and np.array_equal(mg["hi"], [3.0, 5.0])
    s = make(marginals={"params": ["a", "b"], "ranges": {"b": [-1, 1.5]}})   # an explicit entry wins
    assert acc(s).cfg["resolved"] == {"a": (-0.5, 3.0), "b": (-1.0, 1.5)}
    s = make(marginals={"params": ["a", "b"], "ranges": "covmat"})
    centre, sig = s._shift, np.sqrt(np.diag(s._initial_covmat))
    want_a = (max(centre[0] - 5 * sig[0], -0.5), min(centre[0] + 5 * sig[0], 3.0))   # clipped to the support
    assert acc(s).cfg["resolved"]["a"] == want_a
    assert acc(s).cfg["resolved"]["b"] == (centre[1] - 5 * sig[1], centre[1] + 5 * sig[1])
    assert sig[1] == 0.5 and want_a[0] == -0.5      # (`proposal: 0.5`; the lower clip acts)


class NeverBuilt(MargOracleEngine):
    def __init__(self, *a, **k):
        raise AssertionError("the option must be refused before the engine is created")


class Refusing(MCMCHip):
    _engine_factory = staticmethod(NeverBuilt)


@pytest.mark.parametrize("opt, match", [
    ({"params": ["a", "nope"]}, r"marginals: unknown parameter name\(s\) \['nope'\]"),
    ({"pairs": [["a", "zz"]]}, r"marginals: unknown parameter name\(s\) \['zz'\]"),
    ({"pairs": [["a", "a"]]}, "marginals: the pair .* two different parameters"),
    ({"bins": 1025}, "marginals: bins must be an integer in 1..1024"),
    ({"bins2d": 65, "pairs": "all"}, "marginals: bins2d must be an integer in 1..64"),
    ({"bins": 0}, "marginals: bins must be"),
    ({"ranges": {"a": [1, 1]}}, r"marginals: ranges\['a'\] must be a finite \[lo, hi\]"),
    ({"ranges": {"q": [0, 1]}}, "marginals: ranges names unknown"),
    ({"ranges": "posterior"}, "marginals: ranges must be"),
    ({"binz": 3}, r"marginals: unknown key\(s\) \['binz'\]"),
    ("all", "marginals: expected True, None or a dict"),
])
def test_refusals_by_name_before_the_engine_is_created(opt, match):
    with pytest.raises(LoggedError, match=match):
        Refusing({"n_walkers": 128, "group_size": 64, "marginals": opt}, ProblemSpec.from_info(QUICK))


def test_refusals_of_slab_size_temperature_and_old_engines():
    d = 70      # "pairs": "all" at 64 x 64 bins: 2415 x 4097 counters = 79 MB > 64 MiB
    info = {"likelihood": {"one": None},
            "params": {f"p{i}": {"prior": {"min": 0, "max": 1}} for i in range(d)}}
    with pytest.raises(LoggedError, match="marginals: .*pairs.* above the 67108864 allowed"):
        Refusing({"n_walkers": 128, "group_size": 64, "marginals": {"pairs": "all", "bins2d": 64}},
                 ProblemSpec.from_info(info))
    assert 8 * slab_size(d, 128, 2415, 64) > 64 << 20 >= 8 * slab_size(60, 128, 1770, 64)
    with pytest.raises(LoggedError, match="marginals: .*temperature 2"):
        Refusing({"n_walkers": 128, "group_size": 64, "marginals": True, "temperature": 2},
                 ProblemSpec.from_info(QUICK))

    class Old(MCMCHip):
        _engine_factory = staticmethod(OracleEngine)    # (no marginal entry points)
    with pytest.raises(LoggedError, match="marginals: this engine has no marginal histograms"):
        Old({"n_walkers": 128, "group_size": 64, "marginals": True}, ProblemSpec.from_info(QUICK))
    Old({"n_walkers": 128, "group_size": 64}, ProblemSpec.from_info(QUICK))   # off: served as before


# ------------------------------------------------------------------------------- the window
def _expected(s):
    """The rule applied to exactly the snapshots the moment window holds (the intervals of
    `_intervals`, i.e. everything after the dropped snapshots) plus the unfinished interval."""
    eng = s.engine
    snaps = eng.snapshots[s._dropped_snapshots:]
    slab = np.zeros_like(eng._mg_slab)
    for x in snaps:
        slab += rule_slab(x, **eng._mg)
    return slab, len(snaps)


def test_products_hold_the_window_of_the_moments_and_nothing_older():
    s = make(max_samples=60000)
    s.run()
    assert len(s.progress) >= 5 and s._dropped_snapshots > 0 and s._iv0 > 0   # intervals were dropped
    assert len(acc(s).ivs) == len(s._intervals)
    m = s.products()["marginals"]
    slab, n = _expected(s)
    assert n == sum(iv[0] for iv in s._intervals) + s._snaps_in_interval < len(s.engine.snapshots)
    assert np.array_equal(m.slab, slab) and m.slab.dtype == np.uint64
    assert m.n_accumulations == n and m.n_samples == n * 128
    # the dropped intervals are gone: the same count over ALL snapshots is larger
    assert int(m.counts("a").sum()) + sum(m.outside("a")) == n * 128
    # a second call moves nothing (the unfinished interval is held on the host by then)
    again = s.products(combined=True)["marginals"]
    assert again == m
    assert m.params == ["a", "b"] and m.pairs == [("b", "a")] and m.counts2d("b", "a").shape == (4, 4)


def test_a_resume_in_mid_interval_ends_with_identical_counts(tmp_path):
    one = make(str(tmp_path / "a"), 40000)
    one.run()
    p = str(tmp_path / "b")
    b1 = make(p, 20000)
    b1.run()
    z = np.load(p + ".1.state.npz")
    assert int(z["marg_open_n"]) > 0 and z["marg_open"].sum() > 0       # stopped in mid-interval
    assert z["marg_iv"].shape == (len(z["iv_n"]), slab_size(2, 16, 1, 4))
    first = Marginals.load(p + ".marginals.npz")
    assert first == b1.products()["marginals"]
    b2 = make(p, 40000, resume=True)
    assert b2.engine._mg_n == int(z["marg_open_n"])     # the unfinished interval is back on the device
    b2.run()
    got, ref = b2.products()["marginals"], one.products()["marginals"]
    assert np.array_equal(got.slab, ref.slab) and got == ref
    assert got.n_accumulations > first.n_accumulations
    assert Marginals.load(p + ".marginals.npz") == got
    slab, n = _expected(one)
    assert np.array_equal(ref.slab, slab) and ref.n_accumulations == n
    # the ranges are part of the resume geometry
    with pytest.raises(LoggedError, match="marginals: cannot resume"):
        make(p, 50000, resume=True, marginals={"params": "all", "pairs": [["b", "a"]], "bins": 16,
                                               "bins2d": 4, "ranges": {"a": [0, 1]}})
    with pytest.raises(LoggedError, match="marginals: cannot resume"):
        make(p, 50000, resume=True, marginals={"params": "all", "pairs": [["b", "a"]], "bins": 32,
                                               "bins2d": 4})
    assert not os.path.exists(p + ".marginals.npz.npz")


def test_the_output_file_is_cleaned_with_the_other_files(tmp_path):
    p = str(tmp_path / "c")
    make(p, 5000).run()
    assert os.path.exists(p + ".marginals.npz")
    OnDouble({"n_walkers": 128, "group_size": 64, "seed": 1}, ProblemSpec.from_info(QUICK), output=p,
             force=True)
    assert not os.path.exists(p + ".marginals.npz")
