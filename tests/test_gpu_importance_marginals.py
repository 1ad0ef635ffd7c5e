"""Reweighted marginal histograms on the MI355X (importance_hist_kernels.hip, mcmc_hip_importance_hist_*): the
128-bit words, `saturated` and the accumulations equal the rule of DESIGN.md section 2 ("Importance marginals")
-- tests/importance_hist_ref.py, numpy plus the oracle's dexp -- bit for bit on crafted states at the smallest
shapes at which the kernels can still go wrong; the words do not depend on steps_per_launch, add up over
walker-offset shards and survive a resume; every step path hands the product the state its stored snapshots
show; and a run recovers the quantiles of the exact reweighted Gaussian within six standard deviations of the
statistic on exact draws.  Every test fails without the feature: the entry points and the key do not exist."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402,F401  (before the first Engine: one HIP runtime for both)

from cobaya_amd import run  # noqa: E402
from cobaya_amd.engine import ERR_ARG, ERR_STATE, Engine, EngineError  # noqa: E402,F401
from cobaya_amd.importance import Importance  # noqa: E402
from cobaya_amd.marginals import WeightedMarginals, slab_size  # noqa: E402
from tests.importance_hist_ref import HistRule, same_hist, words  # noqa: E402
from tests.importance_ref import Rule, rule_c, same  # noqa: E402
from tests.test_gpu_importance import _engine, _gaussian, _state  # noqa: E402

LN_Q1 = 32 * math.log(2.0)          # 22.18...: e = 2^-32, q = 1, lies this far below c


def _crafted_x(W, n_cols, rng, lo, hi, bins):
    """Ordinary values, and in every column values exactly on lo, on hi, on interior edges and one ulp outside
    either end."""
    x = rng.uniform(lo - 0.5, hi + 0.5, (W, n_cols))
    edges = [lo + (hi - lo) * k / b for b in bins for k in range(1, b)][:8]
    special = [lo, hi, np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf), np.nextafter(lo, np.inf),
               np.nextafter(hi, -np.inf)] + edges
    for j in range(n_cols):
        x[rng.permutation(W)[:len(special)], j] = special
    return x


def _crafted_delta(n_alt, W, rng, c, above=False, none_finite=False):
    """Log-weights whose finite maximum is c (twice per row), either side of q = 1, 800 below c, -inf, +inf, NaN
    and -0.0; `above`: up to 11 above c (unsaturated) and 12, 701 and 1 500 above it (saturated: three per row)."""
    if none_finite:
        return rng.choice([np.nan, np.inf, -np.inf], size=(n_alt, W))
    dl = c - rng.uniform(0.0, 30.0, (n_alt, W))
    for k in range(n_alt):
        at = rng.permutation(W)[:18]
        dl[k, at[:2]] = c
        dl[k, at[2:11]] = [-np.inf, np.inf, np.nan, -0.0, c - 800.0, c - LN_Q1 + 1e-9, c - LN_Q1 - 1e-9,
                           np.nextafter(c - LN_Q1, np.inf), -np.inf]
        if above:
            dl[k, at[11:18]] = [c + 0.5, c + 5.25, c + 11.0, c + 11.09, c + 12.0, c + 701.0, c + 1500.0]
    return dl


def _accumulate(eng, rule, hr, x, delta, shift, step, d):
    """The crafted state (its columns from d on are the derived rows) and log-weights through the engine and,
    where given, through the rules."""
    eng.set_full_state(_state(x[:, :d], step))
    if x.shape[1] > d:
        eng.derived_set_values(np.ascontiguousarray(x[:, d:]))
    _, dev, stream = eng.importance_row_views()
    with torch.cuda.stream(stream):
        dev.copy_(torch.from_numpy(np.ascontiguousarray(delta)))
    eng.accumulate_importance(dev)
    if rule is not None:
        rule.accumulate(x[:, :d], delta, shift)
        hr.accumulate(x, delta, rule.c)


def _request(eng, rule, hr, close):
    """One request: both read-outs of the engine against both rules'."""
    eng.request_importance(close)
    got, n_acc = eng.fetch_importance(), rule.n_acc
    goth = eng.fetch_importance_hist()
    same(got, rule.request(close))
    same_hist(goth, hr.request(close, n_acc))
    return got, goth


CASES = {  # d, m derived rows, W, group size, 1-D entries, bins, pairs, bins2d, flags
    "one-bin": (1, 0, 64, 64, [0], 1, [], 1, [True]),
    "seven-bins-and-a-1x1-pair": (2, 0, 128, 64, [0, 1], 7, [(1, 0)], 1, [True, False, True]),
    "slices-the-last-partial": (3, 0, 4160, 64, [0, 1, 2], 5, [(0, 2)], 3, [False, True]),
    "largest-lds": (30, 0, 256, 64, list(range(30)), 1024, [(0, 1), (29, 3), (7, 8)], 64, [True] * 8),
    "d-above-128": (200, 0, 128, 64, [0, 129, 199], 9, [(199, 0)], 4, [True, True]),
    "derived-row-with-nan": (2, 1, 128, 64, [0, 2], 6, [(2, 1), (0, 1)], 3, [True, False]),
}


@pytest.mark.parametrize("case", list(CASES))
def test_words_saturated_and_accumulations_equal_the_rule_bit_for_bit(case):
    d, m, W, gs, dims1, bins1, pairs, bins2, on = CASES[case]
    rng = np.random.default_rng(sum(map(ord, case)))
    n_alt, cov, lo_v, hi_v = len(on), [False] * len(on), -2.0, 2.0
    lo, hi = np.full(d + m, lo_v), np.full(d + m, hi_v)
    mg = dict(dims1=dims1, bins1=bins1, pairs=pairs, bins2=bins2, lo=lo, hi=hi)
    nc = slab_size(len(dims1), bins1, len(pairs), bins2)
    shift = 0.1 * rng.standard_normal(d)

    def crafted_x():
        x = _crafted_x(W, d + m, rng, lo_v, hi_v, (bins1, bins2))
        if m:
            x[rng.permutation(W)[:5], d:] = np.nan         # only a derived row can be NaN
        return x

    def engine(with_hist):
        eng = _engine(d, W, gs)
        if m:
            eng.configure_derived(m)
        eng.set_moment_shift(shift)
        eng.configure_importance(cov)
        if with_hist:
            with pytest.raises(EngineError) as e:          # the marginals come first
                eng.configure_importance_hist(on)
            assert e.value.code == ERR_STATE
        eng.configure_marginals(dims1, bins1, pairs, bins2, lo, hi)
        assert eng.importance_hist_layout() == {"n_hist": 0, "on": [False] * n_alt, "n_counters": 0, "n_words": 0}
        if with_hist:
            eng.configure_importance_hist(on)
            assert eng.importance_hist_layout() == {"n_hist": sum(on), "on": on, "n_counters": nc,
                                                    "n_words": sum(on) * (2 * nc + 1)}
        return eng

    eng, off = engine(True), engine(False)
    rule, hr = Rule(d, W, gs, cov), HistRule(on, mg)

    def both(x, delta, step):
        _accumulate(eng, rule, hr, x, delta, shift, step, d)
        _accumulate(off, None, None, x, delta, shift, step, d)

    def request(close):
        got, goth = _request(eng, rule, hr, close)
        off.request_importance(close)
        same(off.fetch_importance(), got)      # the sums with the key on are the sums with it off, bit for bit
        return got, goth

    # interval 1: c = 3.5 from its first accumulation; the second lies up to 1 500 above it
    both(crafted_x(), _crafted_delta(n_alt, W, rng, 3.5), 5)
    _, h1 = request(False)                                             # a peek disturbs nothing
    assert not h1["saturated"].any() and not h1["hi"].any() and h1["lo"].any()
    both(crafted_x(), _crafted_delta(n_alt, W, rng, 3.5, above=True), 9)
    got, goth = request(True)
    assert got["c"].tolist() == [3.5] * n_alt and got["n_acc"] == goth["n_acc"] == 2       # the c the words were formed under
    assert goth["saturated"].tolist() == [3] * sum(on)                 # c + 12, c + 701, c + 1 500
    # interval 2: no finite log-weight in its first accumulation gives c = 0; then 1 480 above it saturates
    both(crafted_x(), _crafted_delta(n_alt, W, rng, 0.0, none_finite=True), 13)
    both(crafted_x(), _crafted_delta(n_alt, W, rng, -20.0, above=True), 17)
    got, goth = request(True)
    assert got["c"].tolist() == [0.0] * n_alt and goth["saturated"].tolist() == [2] * sum(on)   # -20 + 701, -20 + 1 500
    _, empty = request(False)                                          # closed: all zero
    assert not empty["lo"].any() and not empty["hi"].any() and not empty["saturated"].any() and empty["n_acc"] == 0
    # a set-back that is then added to, with the carry: the chosen low words are 2^64 - 1
    x = crafted_x()
    both(x, _crafted_delta(n_alt, W, rng, 1.0), 21)
    part, parth = request(False)
    full = dict(parth, lo=np.where(parth["lo"] != 0, np.uint64(2 ** 64 - 1), parth["lo"]))
    for e in (eng, off):
        e.configure_importance(cov)                                    # (everything is dropped, the histograms too)
        assert e.importance_hist_layout()["n_words"] == 0
        e.importance_set(part)
    eng.configure_importance_hist(on)
    eng.importance_set(part)
    eng.importance_hist_set(full)
    hr.set(full)
    both(x, _crafted_delta(n_alt, W, rng, 300.0), 25)                  # the same x: the same counters are added to
    got, goth = request(True)
    assert got["c"].tolist() == [1.0] * n_alt and got["n_acc"] == 2
    rose = (full["lo"] == np.uint64(2 ** 64 - 1)) & (goth["hi"] == full["hi"] + np.uint64(1))
    assert rose.any() and np.array_equal(goth["hi"][rose], full["hi"][rose] + np.uint64(1))
    with pytest.raises(EngineError) as e:
        eng.importance_hist_set(dict(parth, lo=parth["lo"][:, :-1], hi=parth["hi"][:, :-1]))
    assert e.value.code == ERR_ARG
    # all flags off, and new marginals, release the histograms
    eng.configure_importance_hist([False] * n_alt)
    assert eng.importance_hist_layout()["n_words"] == 0
    eng.configure_importance_hist(on)
    eng.configure_marginals(dims1[:1], bins1, [], bins2, lo, hi)
    assert eng.importance_hist_layout()["n_words"] == 0
    eng.close()
    off.close()


def test_with_the_key_off_the_layout_reports_zero_words():
    eng = _engine(2, 128, 64)
    assert eng.importance_hist_layout()["n_words"] == 0
    with pytest.raises(EngineError) as e:
        eng.configure_importance_hist([])
    assert e.value.code == ERR_STATE                                   # before importance_configure
    eng.configure_importance([True, False])
    eng.configure_marginals([0, 1], 8, [], 4, np.full(2, -1.0), np.full(2, 1.0))
    eng.configure_importance_hist([False, False])
    lay = eng.importance_hist_layout()
    assert lay == {"n_hist": 0, "on": [False, False], "n_counters": 0, "n_words": 0}
    eng.set_full_state(_state(np.zeros((128, 2))))
    _, delta, _ = eng.importance_row_views()
    eng.accumulate_importance(delta)
    eng.request_importance(True)
    eng.fetch_importance()
    with pytest.raises(EngineError) as e:
        eng.fetch_importance_hist()
    assert e.value.code == ERR_STATE
    eng.close()


# ------------------------------------------------------------------------------ the same words under other conditions
MEAN3, COV3 = np.array([0.3, -0.2, 0.1]), np.array([[0.5, 0.2, 0.0], [0.2, 0.4, 0.1], [0.0, 0.1, 0.3]])


def _capped(a, b):
    """A log-weight whose maximum, -0.125, many walkers of every shard attain: the shards take the same c."""
    return torch.clamp(-0.5 * ((a - 0.3) / 0.2) ** 2 + 0.25 * b, max=-0.125)


def _stepped(W, offset, x0, launches):
    """Two intervals of two accumulations, `launches` = the step counts between them."""
    eng = _engine(3, W, 64, walker_offset=offset, gaussian=(MEAN3, COV3))
    eng.set_state(x0)
    eng.set_moment_shift(MEAN3)
    eng.configure_importance([False])
    eng.configure_marginals([0, 1, 2], 12, [(0, 1)], 5, np.full(3, -2.0), np.full(3, 2.0))
    eng.configure_importance_hist([True])
    xrows, delta, stream = eng.importance_row_views()
    parts = []
    for k, spl in enumerate(launches):
        for n in spl:
            eng.step(n)
        with torch.cuda.stream(stream):
            delta[0].copy_(_capped(xrows[0], xrows[1]))
        eng.accumulate_importance(delta)
        if k % 2:
            eng.request_importance(True)
            parts.append((eng.fetch_importance(), eng.fetch_importance_hist()))
    eng.close()
    return parts


def test_the_words_do_not_depend_on_steps_per_launch_and_add_up_over_shards():
    W = 256
    x0 = MEAN3 + np.random.default_rng(4).standard_normal((W, 3)) @ np.linalg.cholesky(COV3).T
    whole = _stepped(W, 0, x0, [[40], [40], [40], [40]])
    other = _stepped(W, 0, x0, [[20, 20], [8, 32], [40], [13, 27]])
    for (a, ah), (b, bh) in zip(whole, other):
        same(a, b)
        same_hist(ah, bh)
    assert whole[0][0]["c"][0] == -0.125 and whole[0][1]["n_acc"] == 2 and len(whole) == 2 and whole[0][1]["lo"].any()
    halves = [_stepped(W // 2, off, x0[off:off + W // 2], [[40], [40], [40], [40]]) for off in (0, W // 2)]
    for k in range(2):     # equal c: the 128-bit words of the shards add up to the whole's, exactly
        assert halves[0][k][0]["c"][0] == halves[1][k][0]["c"][0] == -0.125
        tot = [sum((int(h[k][1]["hi"][0][i]) << 64) + int(h[k][1]["lo"][0][i]) for h in halves)
               for i in range(whole[k][1]["lo"].shape[1])]
        lo, hi = words(tot)
        assert np.array_equal(lo, whole[k][1]["lo"][0]) and np.array_equal(hi, whole[k][1]["hi"][0])
        assert int(whole[k][1]["saturated"][0]) == sum(int(h[k][1]["saturated"][0]) for h in halves)


# ------------------------------------------------------------------------------ through `run`
MEAN, COV = [0.3, -0.2], [[0.5, 0.2], [0.2, 0.4]]
FUNCTIONS = {"bao": lambda a: -0.5 * (((a - 0.31) * 2.5) * ((a - 0.31) * 2.5)), "tilt": lambda a, b: 0.5 * a - 0.25 * (b * b)}
OPTION = {"bao": {"function": "lambda a: -0.5 * (((a - 0.31) * 2.5) * ((a - 0.31) * 2.5))", "marginals": True},
          "tilt": {"function": "lambda a, b: 0.5 * a - 0.25 * (b * b)", "cov": False, "marginals": True},
          "flat": {"function": "lambda b: 0.0 * b", "cov": False}}
MARG = {"params": ["a", "b", "s"], "pairs": [["b", "a"], ["s", "a"]], "bins": 24, "bins2d": 6, "ranges": {"s": [-3.0, 3.0]}}


def _info(like=None, **opts):
    o = {"n_walkers": 512, "group_size": 64, "seed": 7, "Rminus1_stop": 0.0, "max_samples": 200000,
         "steps_per_launch": 40, "moments_every": 1, "snapshot_every": 40, "max_rows": 1 << 22, "learn_every": "20d",
         "importance": OPTION, "marginals": MARG}
    o.update(opts)
    return {"likelihood": like or {"gaussian": {"mean": MEAN, "cov": COV}},
            "params": {"a": {"prior": {"min": -6, "max": 6}, "ref": {"dist": "norm", "loc": 0.3, "scale": 0.5}},
                       "b": {"prior": {"min": -6, "max": 6}, "ref": {"dist": "norm", "loc": -0.2, "scale": 0.5}},
                       "s": {"derived": "lambda a, b: a + b"}},
            "sampler": {"mcmc_hip": o}}


def _banana(pts):
    return -0.5 * (pts[:, 0] ** 2 + ((pts[:, 1] - 0.5 * pts[:, 0] ** 2) / 0.5) ** 2)


def _acc(smp):
    return next(p for p in smp._products if p.name == "importance")


@pytest.mark.parametrize("path", ["incremental", "full", "device_function"])
def test_every_step_path_gives_the_product_bit_for_bit_by_replay(path, tmp_path):
    """The window's snapshots are the stored rows: replayed through the numpy rule, interval by interval, they
    give the words of every interval and the product bit for bit (the log-weights and the derived name use
    exactly rounded operations only)."""
    from tests.products_together import snapshots_of
    W = 512
    if path == "device_function":
        info = _info({"banana": {"class": "device_function", "function": _banana}}, max_tries="2000d")
    else:
        info = _info(**({"evaluation": "full"} if path == "full" else {}))
    info["output"] = str(tmp_path / "iw")
    _, smp = run(info)
    kernel = smp.engine.last_step_kernel()
    print(path, kernel)
    assert ("fn_walker" in kernel) == (path == "device_function") and bool(smp.incremental) == (path == "incremental")
    iw = smp.products()["importance"]
    a = _acc(smp)
    counts = [iv[0] for iv in smp._intervals] + [smp._snaps_in_interval]
    snaps = snapshots_of(smp)
    snaps = snaps[len(snaps) - sum(counts):]
    assert iw.n_acc == sum(counts) > 4 and len(smp._intervals) >= 2
    mcfg = next(p for p in smp._products if p.name == "marginals").cfg
    names = ["a", "b", "s"]
    lo, hi = (np.array([mcfg["resolved"][n][k] for n in names]) for k in (0, 1))
    mg = dict(dims1=[0, 1, 2], bins1=24, pairs=[(1, 0), (2, 0)], bins2=6, lo=lo, hi=hi)
    hr, parts, at = HistRule([True, True, False], mg), [], 0
    for n, held in zip(counts, list(a.ivs) + [a.open]):
        span = snaps[at:at + n]
        deltas = [np.stack((FUNCTIONS["bao"](s["x"][:, 0]), FUNCTIONS["tilt"](s["x"][:, 0], s["x"][:, 1]), 0.0 * s["x"][:, 1]))
                  for s in span]
        c = np.array([rule_c(dl) for dl in deltas[0]]) if n else np.zeros(3)
        for s, dl in zip(span, deltas):
            assert np.array_equal(s["z"][:, 0], s["x"][:, 0] + s["x"][:, 1])
            hr.accumulate(np.column_stack((s["x"], s["z"])), dl, c)
        want = hr.request(True, n)
        same_hist(held["hist"], want)
        if n:
            assert np.array_equal(held["c"], c)
        parts.append(dict(held, hist=want))
        at += n
    want = Importance.from_parts(iw.names, iw.params, smp._shift, [True, False, False], W, parts,
                                 marg=dict(mcfg, ranges=mcfg["resolved"], on=[True, True, False]))
    assert iw == want and all(iw.marginals(n).slab.tobytes() == want.marginals(n).slab.tobytes() for n in ("bao", "tilt"))
    wm, um = iw.marginals("bao"), smp.products()["marginals"]
    assert isinstance(wm, WeightedMarginals) and (wm.params, wm.pairs, wm.ranges) == (um.params, um.pairs, um.ranges)
    assert wm.saturated == 0 and wm.n_samples == um.n_samples == iw.n_samples and wm.weights("s").sum() > 0
    if path != "device_function":      # (the Gaussian: "tilt" moves the marginal of a upwards)
        assert iw.marginals("tilt").mean("a") > um.mean("a")
    assert Importance.load(str(tmp_path / "iw.importance.npz")) == iw
    smp.close()
    assert smp.products()["importance"] == iw        # the product outlives the engine


def test_a_resume_in_mid_interval_is_bit_identical(tmp_path):
    from cobaya_amd.model import ProblemSpec
    from cobaya_amd.sampler import MCMCHip

    def make(prefix, resume, max_samples):
        info = _info()
        opts = dict(info["sampler"]["mcmc_hip"], seed=21, max_samples=max_samples)
        return MCMCHip(opts, ProblemSpec.from_info(info), output=prefix, resume=resume)

    a = make(str(tmp_path / "a"), False, 150000)
    a.run()
    pa = a.products()["importance"]
    a.close()
    b1 = make(str(tmp_path / "b"), False, 30000)
    b1.run()
    assert b1.n_steps_raw < a.n_steps_raw
    z = np.load(str(tmp_path / "b.1.state.npz"), allow_pickle=False)
    b1.close()
    b2 = make(str(tmp_path / "b"), True, 150000)
    assert b2.engine.importance_layout()["n_accumulations"] == int(z["iw_open_nacc"][0]) > 0
    b2.engine.request_importance(False)
    b2.engine.fetch_importance()
    back = b2.engine.fetch_importance_hist()             # the open histograms are on the device again
    assert np.array_equal(back["lo"], z["iw_open_hlo"][0]) and np.array_equal(back["hi"], z["iw_open_hhi"][0])
    assert back["lo"].any() and back["n_acc"] == int(z["iw_open_nacc"][0])
    b2.run()
    pb = b2.products()["importance"]
    assert b2.n_steps_raw == a.n_steps_raw and pb == pa
    assert all(pa.marginals(n).slab.tobytes() == pb.marginals(n).slab.tobytes() for n in ("bao", "tilt"))
    b2.close()


# ------------------------------------------------------------------------------ statistics
# sd of the 0.16, 0.5 and 0.84 quantiles of the weighted marginal over 200 repetitions of N0 exact draws of
# N(mu, Sigma) through the quantised rule (q = floor(min(e, 2^16) 2^32), 128 bins over mu +- 6 sigma), measured
# on the CPU with numpy BEFORE any device run: per quantile the largest sd over the parameters in units of
# sigma_i, times sqrt(N0)
N0 = 65536
CALIBRATED = {2: (1.2705, 1.2311, 1.4082), 30: (2.1025, 1.9574, 2.2599)}
QS = [0.16, 0.5, 0.84]


def _normal_cdf(t):
    return 0.5 * (1.0 + np.vectorize(math.erf)(t / math.sqrt(2.0)))


@pytest.mark.parametrize("d", [2, 30])
def test_a_run_recovers_the_quantiles_of_the_exact_reweighted_gaussian(d):
    """The construction of test_a_run_recovers_the_exact_reweighted_gaussian: the target N(mu, Sigma) in a box 12
    sigma wide, reweighted to N(0.8 mu + 0.2 m, 0.8 Sigma) with m = mu + 0.5 sqrt(diag Sigma).  The 0.16, 0.5 and
    0.84 quantiles of the weighted marginal of each parameter are compared with those the EXACT bin masses of
    that Gaussian give through the same `quantile` rule, which removes any binning bias.

    The bar, measured on the CPU before any device run: 200 repetitions of N0 = 65 536 exact numpy draws through
    the quantised rule gave, per parameter, sd of the three quantiles between 0.00418 and 0.00550 sigma_i at d = 2
    (largest per quantile: 0.00496, 0.00481, 0.00550) and between 0.00622 and 0.00883 sigma_i at d = 30 (0.00821,
    0.00765, 0.00883).  As in that test the sd is carried to the run's N = n_samples as sd0 sqrt(N0 / N), and the
    device result lies within 6 of those.

    Measured on an MI355X, the largest deviation over the parameters of the 0.16 / 0.5 / 0.84 quantiles in those
    sd: d = 2 (N = 565 248, 138 accumulations) 0.37 / 2.20 / 1.91; d = 30 (N = 1 089 536, 266 accumulations)
    1.76 / 2.36 / 1.76; nothing saturated; ESS fractions 0.935 and 0.386."""
    W = 4096
    mu, S = _gaussian(d)
    sig = np.sqrt(np.diag(S))
    m = mu + 0.5 * sig
    names = ["p%d" % i for i in range(d)]
    dev = torch.device("cuda", 0)
    P, mt = torch.tensor(np.linalg.inv(4 * S), device=dev), torch.tensor(m, device=dev)

    def quad(*rows):
        dx = torch.stack(rows) - mt[:, None]
        return -0.5 * (dx * (P @ dx)).sum(0)
    fn = eval("lambda %s: quad(%s)" % (", ".join(names), ", ".join(names)), {"quad": quad})
    info = {"likelihood": {"gaussian": {"mean": mu.tolist(), "cov": S.tolist()}},
            "params": {n: {"prior": {"min": mu[i] - 6 * sig[i], "max": mu[i] + 6 * sig[i]},
                           "ref": {"dist": "norm", "loc": mu[i], "scale": sig[i]}} for i, n in enumerate(names)},
            "sampler": {"mcmc_hip": {"n_walkers": W, "seed": 11, "marginals": True,
                                     "importance": {"wide": {"function": fn, "marginals": True}}}}}
    _, smp = run(info)
    iw = smp.products()["importance"]
    wm = iw.marginals("wide")
    N = iw.n_samples
    exact_mean, exact_sd = 0.8 * mu + 0.2 * m, np.sqrt(0.8) * sig
    worst = np.zeros(3)
    for i, n in enumerate(names):
        masses = np.diff(_normal_cdf((wm.edges(n) - exact_mean[i]) / exact_sd[i]))
        exact = WeightedMarginals([n], [], wm.bins, 1, {n: wm.ranges[n]}, np.concatenate(([0.0, 0.0], masses)))
        dev_sd = (wm.quantile(n, QS) - exact.quantile(n, QS)) / (np.array(CALIBRATED[d]) * math.sqrt(1.0 / N) * sig[i])
        worst = np.maximum(worst, np.abs(dev_sd))
    print("d", d, "N", N, "n_acc", iw.n_acc, "saturated", wm.saturated, "ESS fraction", iw.ess_fraction("wide"),
          "largest deviation of the 0.16 / 0.5 / 0.84 quantiles in sd:", worst.round(3).tolist())
    assert wm.saturated == 0 and wm.n_samples == N and (wm.bins, len(wm.params)) == (128, d)
    assert np.all(worst <= 6)
    smp.close()
