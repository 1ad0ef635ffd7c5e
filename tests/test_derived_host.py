"""Derived parameters given as functions, host side (no GPU): the three forms of a function in
`params`, every refusal by its message, the marginals option over derived names, the arithmetic of
the `Derived` product on crafted sums, and the numpy rule (tests/derived_ref.py) against a
long-double restatement.  Every test fails without the feature."""
from types import SimpleNamespace

import numpy as np
import pytest

from cobaya_amd import derived as D
from cobaya_amd import marginals as M
from cobaya_amd.model import DerivedFunction, ProblemSpec, UnsupportedModel
from cobaya_amd.sampler import HIP_DEFAULTS, EnsembleMCMC
from tests.derived_ref import Rule, group_sums


def module_level_ratio(a, b):
    return a / b


def _info(extra, like=None):
    return {"likelihood": like or {"one": None},
            "params": {"a": {"prior": {"min": 0, "max": 1}}, "b": {"prior": {"min": 0, "max": 1}}, **extra}}


# ------------------------------------------------------------------------------ the model
def test_the_three_forms_of_a_function():
    import torch
    spec = ProblemSpec.from_info(_info({
        "s": {"derived": "lambda a, b: a + torch.sqrt(b) * math.pi", "latex": "s"},
        "r": {"derived": "tests.test_derived_host:module_level_ratio"},
        "q": {"derived": lambda s, a: s * a}}))
    assert spec.sampled == ["a", "b"] and spec.derived == [] and spec.derived_names == ["s", "r", "q"]
    fs = spec.derived_functions
    assert all(isinstance(f, DerivedFunction) for f in fs)
    assert [f.args for f in fs] == [["a", "b"], ["a", "b"], ["s", "a"]]      # q takes an EARLIER derived
    a, b = torch.tensor([0.25, 1.0], dtype=torch.float64), torch.tensor([4.0, 9.0], dtype=torch.float64)
    s = fs[0].function(a, b)
    assert s.dtype == torch.float64 and np.allclose(s.numpy(), [0.25 + 2 * np.pi, 1.0 + 3 * np.pi])
    assert fs[1].function.__name__ == "module_level_ratio" and fs[1].function(6.0, 3.0) == 2.0
    assert np.allclose(fs[2].function(s, a).numpy(), s.numpy() * a.numpy())
    assert spec.labels == {"s": "s"}
    # with a likelihood of the user's own
    spec = ProblemSpec.from_info(_info({"c": {"derived": "lambda a, b: a * b"}},
                                       {"f": {"class": "device_function", "function": lambda p: p.sum(1)}}))
    assert spec.like_kind == "device_function" and spec.derived_names == ["c"]
    # a model without them is what it was
    assert ProblemSpec.from_info(_info({})).derived_functions == []


@pytest.mark.parametrize("extra, match", [
    ({"s": {"derived": "lambda a, c: a + c"}}, r"parameter 's': the derived function takes \['c'\]"),
    ({"s": {"derived": "lambda a, t: a"}, "t": {"derived": "lambda a: a"}}, r"parameter 's'.*takes \['t'\].*earlier"),
    ({"s": {"derived": "lambda *a: a[0]"}}, r"parameter 's'.*\*a"),
    ({"s": {"derived": "lambda a: ("}}, "parameter 's'.*could not be evaluated"),
    ({"s": {"derived": "no_such_module_xyz:f"}}, "parameter 's'.*could not be resolved"),
    ({"s": {"derived": "just some words"}}, "parameter 's'.*'lambda ...: ...' or 'package.module:name'"),
    ({"s": {"derived": 3.5}}, "parameter 's': derived functions are not supported"),
    ({f"s{k}": {"derived": "lambda a: a"} for k in range(33)}, "33 derived parameters are given as functions.*at most 32"),
])
def test_a_bad_function_is_refused_by_name(extra, match):
    with pytest.raises(UnsupportedModel, match=match):
        ProblemSpec.from_info(_info(extra))


def test_refusals_beside_other_derived_parameters_and_what_stays_as_it_was():
    mix = {"gaussian_mixture": {"means": [[0.5, 0.5]], "covs": [np.eye(2) * 0.01], "derived": True}}
    plain = {"x0": None, "x1": None}
    ProblemSpec.from_info(_info(plain, mix))                       # (the standardised coordinates alone: served)
    with pytest.raises(UnsupportedModel, match=r"derived functions \['s'\] cannot stand beside.*derived: True"):
        ProblemSpec.from_info(_info({**plain, "s": {"derived": "lambda a: a"}}, mix))
    # a derived name WITHOUT a function keeps today's messages
    with pytest.raises(UnsupportedModel, match="derived parameters need a gaussian_mixture"):
        ProblemSpec.from_info(_info({"u": None}))
    with pytest.raises(UnsupportedModel, match="no derived parameters"):
        ProblemSpec.from_info(_info({"u": None}, {"f": {"class": "device_function", "function": lambda p: p.sum(1)}}))
    # the hosted path (a live cobaya Model owns its derived parameters): its present behaviour
    with pytest.raises(UnsupportedModel, match="parameter 's': derived functions are not supported"):
        ProblemSpec._from_params(_info({"s": {"derived": "lambda a: a"}})["params"], functions=False)
    # 32 are served
    spec = ProblemSpec.from_info(_info({f"s{k}": {"derived": "lambda a: a"} for k in range(32)}))
    assert len(spec.derived_functions) == 32


# ------------------------------------------------------------------------------ the sampler's options
class _Refused(Exception):
    pass


def _host(**kw):
    def fail(msg, *args, cause=None):
        raise _Refused(msg % args if args else msg)
    return SimpleNamespace(**{"fail": fail, "n_walkers": 128, "size": 1, "rank": 0, "all_reduce_sum": lambda b: b,
                              "temperature": 1.0, "snapshot_steps": 40, "emit": "snapshots", **kw})


class _Factory:
    """An engine factory with every method the accumulator asks for."""
    for _m in D.ENGINE_METHODS:
        locals()[_m] = None


def test_the_option_and_the_accumulators_refusals():
    spec = ProblemSpec.from_info(_info({"s": {"derived": "lambda a, b: a + b"}}))
    assert HIP_DEFAULTS["derived_stats"] is None and EnsembleMCMC.derived_stats is None
    assert EnsembleMCMC.PRODUCT_CLASSES[0] is D.DerivedAccumulator       # before the marginals
    assert D.parse_option(None, ["a", "b"]) == {"cross": ["a", "b"]}
    assert D.parse_option({"cross": "all"}, ["a", "b"]) == {"cross": ["a", "b"]}
    assert D.parse_option({"cross": ["b"]}, ["a", "b"]) == {"cross": ["b"]}
    assert D.parse_option({"cross": None}, ["a", "b"]) == {"cross": []}
    assert D.parse_option(False, ["a", "b"]) is False
    for opt, match in (({"cross": ["c"]}, r"derived_stats: cross names unknown parameter\(s\) \['c'\]"),
                       ({"cros": 1}, "derived_stats: unknown key"), (3, "derived_stats: expected"),
                       ({"cross": "some"}, "derived_stats: cross must be"), ({"cross": ["a", "a"]}, "twice")):
        with pytest.raises(D.DerivedError, match=match):
            D.parse_option(opt, ["a", "b"])
    acc = D.DerivedAccumulator.from_option(None, spec, _Factory, _host())
    assert acc.names == ["s"] and acc.cross == ["a", "b"] and acc.stats and acc.name == "derived"
    off = D.DerivedAccumulator.from_option(False, spec, _Factory, _host())
    assert off is not None and not off.stats                             # (rows and marginals still get values)
    assert D.DerivedAccumulator.from_option(None, ProblemSpec.from_info(_info({})), _Factory, _host()) is None
    with pytest.raises(_Refused, match="emit: chains is not served \\(use emit: snapshots\\)"):
        D.DerivedAccumulator.from_option(None, spec, _Factory, _host(emit="chains"))
    with pytest.raises(_Refused, match="derived_stats: .*temperature 2"):
        D.DerivedAccumulator.from_option(None, spec, _Factory, _host(temperature=2.0))
    with pytest.raises(_Refused, match="derived_stats: cross names unknown"):
        D.DerivedAccumulator.from_option({"cross": ["zz"]}, spec, _Factory, _host())
    with pytest.raises(_Refused, match="this engine keeps no derived rows"):
        D.DerivedAccumulator.from_option(None, spec, object, _host())


def test_marginals_over_derived_names():
    sampled, derived = ["a", "b"], ["s", "p"]
    cfg = M.parse_option({"params": ["a", "s"], "pairs": [["b", "p"]], "ranges": {"s": [-1, 3], "p": [0, 1]}},
                         sampled, derived)
    assert cfg["params"] == ["a", "s"] and cfg["pairs"] == [("b", "p")] and cfg["ranges"]["s"] == (-1.0, 3.0)
    assert M.parse_option(True, sampled, derived)["params"] == sampled              # "all": the sampled ones
    assert M.parse_option({"params": ["a"]}, sampled) == M.parse_option({"params": ["a"]}, sampled, derived)
    for opt in ({"params": ["s"]}, {"params": ["s"], "ranges": "covmat"}, {"params": ["s"], "ranges": {"a": [0, 1]}},
                {"pairs": [["a", "p"]], "ranges": {"s": [0, 1]}}):
        with pytest.raises(M.MarginalsError, match=r"marginals: derived parameter\(s\) \['[sp]'\] need an explicit ranges"):
            M.parse_option(opt, sampled, derived)
    with pytest.raises(M.MarginalsError, match=r"unknown parameter name\(s\) \['s'\]"):
        M.parse_option({"params": ["s"], "ranges": {"s": [0, 1]}}, sampled)          # (existing calls: as before)
    spec = ProblemSpec.from_info(_info({"s": {"derived": "lambda a, b: a + b"}}))
    got = M.resolve_ranges(M.parse_option({"params": ["a", "s"], "ranges": {"s": [0, 2]}}, sampled, ["s"]), spec)
    assert got == {"a": (0.0, 1.0), "s": (0.0, 2.0)}
    with pytest.raises(M.MarginalsError, match="derived parameter 's' needs an explicit ranges entry"):
        M.resolve_ranges({"params": ["s"], "pairs": [], "ranges": "prior"}, spec)


# ------------------------------------------------------------------------------ the product
def _sums(z, x, shift, xshift):
    a, b = z - shift, x - xshift
    tj, tk = np.tril_indices(z.shape[1])
    return dict(n_samples=len(z), n_used=len(z), A=a.sum(0), B=(a[:, tj] * a[:, tk]).sum(0), C=a.T @ b, X=b.sum(0),
                V=(b * b).sum(0), bad=np.zeros(z.shape[1], np.uint64), vmin=z.min(0), vmax=z.max(0))


def test_the_arithmetic_of_the_product_on_crafted_sums(tmp_path):
    rng = np.random.default_rng(2)
    n, shift, xshift = 1000, np.array([10.0, -3.0, 0.5]), np.array([0.1, 0.2])
    x = rng.standard_normal((n, 2)) * [0.5, 2.0] + [0.1, 0.3]
    z = np.column_stack((10.0 + x[:, 0] + x[:, 1], -3.0 + x[:, 0] * x[:, 1], rng.standard_normal(n)))
    names, cross = ["s", "p", "w"], ["a", "b"]
    dv = D.Derived(names, cross, shift, xshift, **_sums(z, x, shift, xshift))
    np.testing.assert_allclose([dv.mean(k) for k in names], np.mean(z, axis=0), rtol=1e-12)
    np.testing.assert_allclose(dv.cov(), np.cov(z.T, ddof=0), rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose([dv.std(k) for k in names], np.std(z, axis=0), rtol=1e-12)
    full = np.cov(np.column_stack((z, x)).T, ddof=0)
    for j, k in enumerate(names):
        for c, s in enumerate(cross):
            np.testing.assert_allclose(dv.cross_cov(k, s), full[j, 3 + c], rtol=1e-10, atol=1e-15)
    corr = np.corrcoef(np.column_stack((z, x)).T)
    np.testing.assert_allclose(dv.corr("s", "p"), corr[0, 1], rtol=1e-10)
    np.testing.assert_allclose(dv.corr("s", "b"), corr[0, 4], rtol=1e-10)
    np.testing.assert_allclose([dv.sampled_mean("a"), dv.sampled_mean("b")], x.mean(0), rtol=1e-12)
    assert (dv.min("p"), dv.max("w")) == (z[:, 1].min(), z[:, 2].max()) and dv.nonfinite("s") == 0
    assert "s = " in dv.summary() and "1000 of 1000" in dv.summary()
    with pytest.raises(KeyError, match="no derived parameter 'a'"):
        dv.mean("a")
    with pytest.raises(KeyError, match="no cross-moments with 'w'"):
        dv.cross_cov("s", "w")
    # merge: two shards of one run are the whole
    h = n // 3
    one = D.Derived(names, cross, shift, xshift, **_sums(z[:h], x[:h], shift, xshift))
    two = D.Derived(names, cross, shift, xshift, **_sums(z[h:], x[h:], shift, xshift))
    both = one.merge(two)
    assert (both.n_samples, both.n_used) == (n, n) and (both.min("s"), both.max("s")) == (dv.min("s"), dv.max("s"))
    np.testing.assert_allclose(both.cov(), dv.cov(), rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose([both.mean(k) for k in names], [dv.mean(k) for k in names], rtol=1e-14)
    with pytest.raises(D.DerivedError, match="only shards of one run"):
        one.merge(D.Derived(names, cross, shift + 1.0, xshift, **_sums(z, x, shift + 1.0, xshift)))
    # files
    path = str(tmp_path / "x.derived.npz")
    dv.save(path)
    back = D.Derived.load(path)
    assert back == dv and back.A.tobytes() == dv.A.tobytes() and back.B.tobytes() == dv.B.tobytes()
    assert np.allclose(np.load(path)["cov"], dv.cov())
    # nothing used: said, not divided by
    empty = D.Derived(["s"], [], [0.0], [], 10, 0, [0.0], [0.0], np.zeros((1, 0)), [], [], [10], [np.nan], [np.nan])
    assert empty.nonfinite("s") == 10 and np.isnan(empty.min("s")) and "no walker" in empty.summary()
    with pytest.raises(D.DerivedError, match="no walker with finite derived values"):
        empty.mean("s")


# ------------------------------------------------------------------------------ the rule
def test_the_numpy_rule_against_a_long_double_restatement():
    """Chains of gs terms of float64: every partial sum is rounded once, so a chain differs from the
    same chain in long double (64-bit mantissa: its own error is 2^-11 of this) by at most
    gs * 2^-53 * sum |terms|; the pooling of G group values adds G * 2^-53 * sum |group values|."""
    rng = np.random.default_rng(4)
    W, gs, m, d = 384, 128, 3, 4
    shift, xshift = np.array([0.3, -0.2, 1.0]), np.array([0.1, 0.0, -0.4, 0.2])
    cross = [2, 0, 3]
    x, z = rng.uniform(-2, 2, (W, d)), rng.standard_normal((W, m)) * 3.0
    z[5, 1], z[130, 0], z[200, 2] = np.nan, np.inf, -np.inf
    rule = Rule(W, gs, m, cross, shift, xshift)
    rule.accumulate(x, z)
    got = rule.request()
    used = np.isfinite(z).all(1)
    assert got["N"] == W - 3 and got["bad"].tolist() == [1, 1, 1] and got["n"] == 1
    assert np.array_equal(got["min"], np.where(np.isfinite(z), z, np.inf).min(0))
    assert np.array_equal(got["max"], np.where(np.isfinite(z), z, -np.inf).max(0))
    a = np.asarray(z - shift, np.longdouble)
    b = np.asarray(x[:, cross] - xshift[cross], np.longdouble)
    want = [np.zeros(s, np.longdouble) for s in ((m,), (m * (m + 1) // 2,), (m, len(cross)), (len(cross),), (len(cross),))]
    mag = [np.zeros(w.shape) for w in want]
    for g in range(W // gs):
        sl = slice(g * gs, (g + 1) * gs)
        parts = group_sums(a[sl], b[sl], used[sl], dtype=np.longdouble)[1:]
        absp = group_sums(np.abs(a[sl]), np.abs(b[sl]), used[sl], dtype=np.longdouble)[1:]
        for k in range(5):
            want[k] = want[k] + parts[k]
            mag[k] = mag[k] + np.asarray(absp[k], np.float64)
    for k, key in enumerate(("A", "B", "C", "X", "V")):
        err = np.abs(np.asarray(got[key], np.longdouble) - want[k]).astype(np.float64)
        bound = (gs + W // gs) * 2.0 ** -53 * mag[k]
        assert (err <= bound).all(), (key, err.max(), bound.min())
        assert (err > 0).any() or key == "X"           # (float64 really rounded: the bound is not vacuous)
