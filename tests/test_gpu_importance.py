"""Importance sums on the MI355X (importance_kernels.hip, mcmc_hip_importance_*): sums, counts, the
counters and c equal the rule of DESIGN.md section 2 ("Importance") -- tests/importance_ref.py, numpy plus
the oracle's dexp -- bit for bit on crafted states at the smallest shapes at which the kernels can still
go wrong; the bits do not depend on steps_per_launch, on how the walkers are sharded or on a resume;
every step path hands the product the state its stored snapshots show; and a run recovers the exact
reweighted Gaussian within six standard deviations of the estimator on exact draws.  No second rank is
started here: the merge of two walker-offset shards stands in for it (the all-reduce of several processes
is tested on the host, tests/test_importance_host.py).  Every test fails without the feature: the entry
points and the option do not exist."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402,F401  (before the first Engine: one HIP runtime for both)

from cobaya_amd import run  # noqa: E402
from cobaya_amd.engine import ERR_ARG, ERR_STATE, Engine, EngineError  # noqa: E402
from cobaya_amd.importance import Importance, n_chains  # noqa: E402
from tests.importance_ref import Rule, same  # noqa: E402


def _engine(d, W, gs, walker_offset=0, gaussian=None):
    """An engine that serves d (d > 128: the huge path, which wants incremental evaluation of a
    Gaussian)."""
    big = d > 128
    eng = Engine(d, W, group_size=gs, device=0, seed=3, incremental=big, walker_offset=walker_offset)
    eng.set_prior([0] * d, [-50.0] * d, [50.0] * d)
    if gaussian is not None:
        eng.set_target_gaussian_mixture([gaussian[0]], [gaussian[1]])
    elif big:
        eng.set_target_gaussian_mixture([np.zeros(d)], [np.eye(d)])
    else:
        eng.set_target_one()
    eng.set_proposal_cov(0.01 * np.eye(d) if gaussian is None else gaussian[1])
    return eng


def _state(x, step=1):
    W = len(x)
    z = np.zeros(W, np.int32)
    return {"x": np.ascontiguousarray(x, dtype=np.float64), "logpost": np.zeros(W), "logprior": np.zeros(W),
            "loglike": np.zeros(W), "weight": z + 1, "prior_rej": z, "burn_left": z,
            "n_accept": np.zeros(W, np.int64), "step": np.uint64(step)}


def _configure(eng, cov, gs):
    """The alternatives; groups wider than the engine serves (64, 128, 256) are the sums' own."""
    eng.configure_importance(cov)
    if gs != eng.group_size:
        eng.importance_set_group_size(gs)


def _accumulate(eng, rule, x, delta, shift, step):
    """The crafted state and log-weights through the engine and through the rule."""
    eng.set_full_state(_state(x, step))
    _, dev, stream = eng.importance_row_views()
    with torch.cuda.stream(stream):
        dev.copy_(torch.from_numpy(np.ascontiguousarray(delta)))
    eng.accumulate_importance(dev)
    rule.accumulate(x, delta, shift)


def _crafted_x(W, d, rng):
    """Ordinary values with denormals and, in the LAST dimension, values at 1e150 whose products overflow."""
    x = rng.standard_normal((W, d))
    x[rng.integers(0, W, 6), rng.integers(0, d, 6)] = [5e-324, -5e-324, 1e-310, -3e-309, 2.2250738585072014e-308, 0.0]
    x[[2, W - 3], d - 1] = [1e150, -1e150]
    return x


def _crafted_delta(n_alt, W, rng, c, specials=True, above=False, none_finite=False):
    """Log-weights whose finite maximum is c (twice per row), with -inf, +inf, NaN, -0.0 and values 800
    below c; `above`: also 701 and 1 500 above c; `none_finite`: NaN and infinities alone."""
    if none_finite:
        return rng.choice([np.nan, np.inf, -np.inf], size=(n_alt, W))
    dl = c - rng.uniform(0.0, 40.0, (n_alt, W))
    for k in range(n_alt):
        at = rng.permutation(W)[:12]
        dl[k, at[:2]] = c
        if specials:
            dl[k, at[2:8]] = [-np.inf, np.inf, np.nan, -0.0, c - 800.0, -np.inf]
        if above:
            dl[k, at[8:10]] = [c + 701.0, c + 1500.0]
    return dl


CASES = [  # (d, W, group_size, cov per alternative)
    (1, 64, 64, [True] * 8),                       # one group, one column
    (2, 128, 64, [True, False, True]),             # the smallest multi-group shape
    (31, 256, 128, [True, False, True]),           # either side of a 32-column block
    (33, 256, 64, [True, False, True, True, False, True, False, True]),
    (64, 8192, 8192, [True]),                      # one long chain (the engine's own groups: 256 walkers)
    (128, 128, 64, [True, False, True]),           # the largest covariance
    (200, 128, 64, [False] * 8),                   # d above 128
]


@pytest.mark.parametrize("d, W, gs, cov", CASES, ids=["d%d-W%d-gs%d-alt%d" % (c[0], c[1], c[2], len(c[3])) for c in CASES])
def test_sums_counts_counters_and_c_equal_the_rule_bit_for_bit(d, W, gs, cov):
    rng = np.random.default_rng(1000 * d + W)
    n_alt, G = len(cov), W // gs
    eng = _engine(d, W, min(gs, 256))
    assert eng.importance_layout()["n_alt"] == 0
    with pytest.raises(EngineError) as e:
        eng.request_importance(True)
    assert e.value.code == ERR_STATE
    _configure(eng, cov, gs)
    lay = eng.importance_layout()
    assert (lay["n_alt"], lay["n_groups"], lay["cov"]) == (n_alt, G, [int(c) for c in cov])
    assert lay["n_sums"] == sum(G * n_chains(d, c) for c in cov) and lay["n_accumulations"] == 0
    shift = 0.1 * rng.standard_normal(d)
    eng.set_moment_shift(shift)
    rule = Rule(d, W, gs, cov)
    # interval 1: c = 3.5 from its first accumulation; the second lies 701 and 1 500 above it
    _accumulate(eng, rule, _crafted_x(W, d, rng), _crafted_delta(n_alt, W, rng, 3.5), shift, 5)
    eng.request_importance(False)                                   # a peek disturbs nothing
    same(eng.fetch_importance(), rule.request(False))
    _accumulate(eng, rule, _crafted_x(W, d, rng), _crafted_delta(n_alt, W, rng, 3.5, above=True), shift, 9)
    eng.request_importance(True)
    got, want = eng.fetch_importance(), rule.request(True)
    same(got, want)
    assert got["c"].tolist() == [3.5] * n_alt and got["n_acc"] == 2
    assert np.all(got["counters"][:, 2] == 2) and np.all(got["counters"][:, 1] == 4) and np.all(got["counters"][:, 0] == 4)
    assert int(got["n"].sum()) == n_alt * (2 * W - 4)
    # interval 2: no finite log-weight in its first accumulation gives c = 0; then everything above 700 is clamped
    _accumulate(eng, rule, _crafted_x(W, d, rng), _crafted_delta(n_alt, W, rng, 0.0, none_finite=True), shift, 13)
    _accumulate(eng, rule, _crafted_x(W, d, rng), _crafted_delta(n_alt, W, rng, -20.0, above=True), shift, 17)
    eng.request_importance(True)
    got, want = eng.fetch_importance(), rule.request(True)
    same(got, want)
    assert got["c"].tolist() == [0.0] * n_alt and np.all(got["counters"][:, 2] == 1)     # -20 + 1 500 alone
    # interval 3: ordinary weights, every chain finite and alive
    x = rng.standard_normal((W, d))
    _accumulate(eng, rule, x, _crafted_delta(n_alt, W, rng, -7.25, specials=False), shift, 21)
    eng.request_importance(True)
    got, want = eng.fetch_importance(), rule.request(True)
    same(got, want)
    assert np.all(np.isfinite(got["sums"])) and np.count_nonzero(got["sums"]) == got["sums"].size
    eng.request_importance(False)                                   # closed: all zero
    empty = eng.fetch_importance()
    assert not empty["sums"].any() and not empty["n"].any() and empty["n_acc"] == 0
    # set: an unfinished interval goes back, c included, and is added to
    _accumulate(eng, rule, x, _crafted_delta(n_alt, W, rng, 1.0, specials=False), shift, 25)
    eng.request_importance(False)
    part = eng.fetch_importance()
    _configure(eng, cov, gs)                                        # (everything is dropped)
    eng.importance_set(part)
    _accumulate(eng, rule, x, _crafted_delta(n_alt, W, rng, 300.0), shift, 29)
    eng.request_importance(True)
    got = eng.fetch_importance()
    same(got, rule.request(True))
    assert got["c"].tolist() == [1.0] * n_alt and got["n_acc"] == 2
    with pytest.raises(EngineError) as e:
        eng.importance_set(dict(part, sums=part["sums"][:-1]))
    assert e.value.code == ERR_ARG
    eng.close()


def test_cov_above_128_and_wrong_tensors_are_refused_by_the_engine():
    eng = _engine(200, 128, 64)
    with pytest.raises(EngineError, match="the covariance is kept for d <= 128") as e:
        eng.configure_importance([False, True])
    assert e.value.code == ERR_ARG
    with pytest.raises(EngineError, match="n_alt = 9"):
        eng.configure_importance([False] * 9)
    eng.configure_importance([False])
    eng.set_full_state(_state(np.zeros((128, 200))))
    with pytest.raises(EngineError, match="accumulate_importance: delta must be"):
        eng.accumulate_importance(torch.zeros((1, 64), dtype=torch.float64, device="cuda"))
    with pytest.raises(EngineError, match="accumulate_importance: delta must be"):
        eng.accumulate_importance(torch.zeros((1, 128), dtype=torch.float64))
    eng.configure_importance([])
    assert eng.importance_layout()["n_alt"] == 0
    eng.close()


# ------------------------------------------------------------------------------ the same bits under other conditions
MEAN3, COV3 = np.array([0.3, -0.2, 0.1]), np.array([[0.5, 0.2, 0.0], [0.2, 0.4, 0.1], [0.0, 0.1, 0.3]])


def _capped(a, b):
    """A log-weight whose maximum, -0.125, many walkers of every shard attain: the shards take the same c."""
    return torch.clamp(-0.5 * ((a - 0.3) / 0.2) ** 2 + 0.25 * b, max=-0.125)


def _stepped(W, offset, x0, launches, cov=(True, False)):
    """Two intervals of two accumulations, `launches` = the step counts between them."""
    eng = _engine(3, W, 64, walker_offset=offset, gaussian=(MEAN3, COV3))
    eng.set_state(x0)
    eng.set_moment_shift(MEAN3)
    eng.configure_importance(cov)
    xrows, delta, stream = eng.importance_row_views()
    parts = []
    for k, spl in enumerate(launches):
        for n in spl:
            eng.step(n)
        with torch.cuda.stream(stream):
            delta[0].copy_(_capped(xrows[0], xrows[1]))
            delta[1].copy_(-0.5 * xrows[2] * xrows[2])
        eng.accumulate_importance(delta)
        if k % 2:
            eng.request_importance(True)
            parts.append(eng.fetch_importance())
    eng.close()
    return parts


def test_the_bits_do_not_depend_on_steps_per_launch_or_on_how_the_walkers_are_sharded():
    W = 256
    x0 = MEAN3 + np.random.default_rng(4).standard_normal((W, 3)) @ np.linalg.cholesky(COV3).T
    whole = _stepped(W, 0, x0, [[40], [40], [40], [40]])
    other = _stepped(W, 0, x0, [[20, 20], [8, 32], [40], [13, 27]])
    for a, b in zip(whole, other):
        same(a, b)
    assert whole[0]["c"][0] == -0.125 and whole[0]["n_acc"] == 2 and len(whole) == 2
    halves = [_stepped(W // 2, off, x0[off:off + W // 2], [[40], [40], [40], [40]]) for off in (0, W // 2)]
    for k in range(2):     # a shard's groups are bit for bit the same groups of the whole ensemble
        assert halves[0][k]["c"][0] == halves[1][k]["c"][0] == -0.125
    names, params = ["capped", "square"], ["a", "b", "c"]
    ref = Importance.from_parts(names, params, MEAN3, [True, False], W, whole)
    pa, pb = (Importance.from_parts(names, params, MEAN3, [True, False], W // 2, h) for h in halves)
    both = pa.merge(pb)
    # (the second alternative's c is each shard's own maximum: its sums meet at the larger one, to rounding)
    assert both.sums[0].tobytes() == ref.sums[0].tobytes() and np.array_equal(both.n, ref.n)
    assert both.log_ratio("capped") == ref.log_ratio("capped") and both.ess("capped") == ref.ess("capped")
    assert np.array_equal(both.cov("capped"), ref.cov("capped"))
    assert math.isclose(both.log_ratio("square"), ref.log_ratio("square"), rel_tol=1e-13)
    np.testing.assert_allclose(both.mean("square"), ref.mean("square"), rtol=1e-12)


# ------------------------------------------------------------------------------ through `run`
MEAN, COV = [0.3, -0.2], [[0.5, 0.2], [0.2, 0.4]]


def np_bao(a):
    return -0.5 * ((a - 0.31) * 2.5) ** 2        # (no division: torch multiplies by a scalar's reciprocal)


def np_tilt(a, b):
    return 0.5 * a - 0.25 * b * b


OPTION = {"bao": {"function": "lambda a: -0.5 * ((a - 0.31) * 2.5) ** 2"},
          "tilt": {"function": lambda a, b: 0.5 * a - 0.25 * b * b, "cov": False}}


def _info(like=None, **opts):
    o = {"n_walkers": 512, "group_size": 64, "seed": 7, "Rminus1_stop": 0.0, "max_samples": 200000,
         "steps_per_launch": 40, "moments_every": 1, "snapshot_every": 40, "max_rows": 1 << 22, "learn_every": "20d",
         "importance": OPTION}
    o.update(opts)
    return {"likelihood": like or {"gaussian": {"mean": MEAN, "cov": COV}},
            "params": {"a": {"prior": {"min": -6, "max": 6}, "ref": {"dist": "norm", "loc": 0.3, "scale": 0.5}},
                       "b": {"prior": {"min": -6, "max": 6}, "ref": {"dist": "norm", "loc": -0.2, "scale": 0.5}}},
            "sampler": {"mcmc_hip": o}}


def _banana(pts):
    return -0.5 * (pts[:, 0] ** 2 + ((pts[:, 1] - 0.5 * pts[:, 0] ** 2) / 0.5) ** 2)


@pytest.mark.parametrize("path", ["incremental", "full", "device_function"])
def test_every_step_path_hands_the_product_the_state_of_its_stored_snapshots(path, tmp_path):
    """The window's snapshots are the last stored rows: replayed through the numpy rule, interval by
    interval, they give the product bit for bit (the log-weights use exactly rounded operations only)."""
    W, gs = 512, 64
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
    ivs = [iv[0] for iv in smp._intervals] + [smp._snaps_in_interval]
    assert iw.n_acc == sum(ivs) > 4 and len(smp._intervals) >= 2 and iw.n_samples == iw.n_acc * W
    data = smp.products()["sample"].data
    x = data[["a", "b"]].to_numpy()[-iw.n_samples:].reshape(iw.n_acc, W, 2)
    rule, parts, at = Rule(2, W, gs, [True, False]), [], 0
    for n in ivs:
        for snap in x[at:at + n]:
            rule.accumulate(snap, np.stack((np_bao(snap[:, 0]), np_tilt(snap[:, 0], snap[:, 1]))), smp._shift)
        parts.append(rule.request(True))
        at += n
    want = Importance.from_parts(["bao", "tilt"], ["a", "b"], smp._shift, [True, False], W, parts)
    print("C", iw.C, want.C, "n equal", np.array_equal(iw.n, want.n), "largest relative difference of the sums",
          [float(np.abs(a / b - 1).max()) for a, b in zip(iw.sums, want.sums)])
    assert iw == want and all(a.tobytes() == b.tobytes() for a, b in zip(iw.sums, want.sums))
    assert iw.nonfinite("bao") == iw.clamped("bao") == iw.zero("tilt") == 0 and iw.n_used("tilt") == iw.n_samples
    assert 0.3 < iw.ess_fraction("bao") <= 1.0 and np.isfinite(iw.log_ratio_stderr("tilt"))
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

    # (a run ends at the first checkpoint that sees max_samples: 30000 ends the first leg at an early
    # checkpoint, 150000 ends both runs at the same later one)
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
    assert b2.engine.importance_layout()["n_accumulations"] == int(z["iw_open_nacc"][0])
    b2.engine.request_importance(False)
    back = b2.engine.fetch_importance()               # the open interval is on the device again, c included
    assert back["sums"].tobytes() == z["iw_open_sums"][0].tobytes() and np.array_equal(back["c"], z["iw_open_c"][0])
    b2.run()
    pb = b2.products()["importance"]
    assert b2.n_steps_raw == a.n_steps_raw
    assert pb == pa and pa.n_used("bao") > 0 and all(s.tobytes() == t.tobytes() for s, t in zip(pa.sums, pb.sums))
    b2.close()


# ------------------------------------------------------------------------------ statistics
def _gaussian(d):
    rng = np.random.default_rng(100 + d)
    A = rng.standard_normal((d, d)) / np.sqrt(d)
    return rng.standard_normal(d), 0.3 * (A @ A.T) + 0.2 * np.eye(d)


# sd of the estimators over 200 repetitions of N0 exact draws of N(mu, Sigma), measured on the CPU with numpy
# BEFORE any device run: (sd of log_ratio, the largest sd of a mean in units of sigma_i), both times sqrt(N0)
N0 = 65536
CALIBRATED = {2: (0.2700, 0.7976), 30: (1.3189, 1.4489)}


@pytest.mark.parametrize("d", [2, 30])
def test_a_run_recovers_the_exact_reweighted_gaussian(d):
    """The target is N(mu, Sigma) in a box 12 sigma wide, reweighted by delta(x) = -(x - m)^T (4 Sigma)^-1
    (x - m) / 2 with m = mu + 0.5 sqrt(diag Sigma): the new posterior is N(0.8 mu + 0.2 m, 0.8 Sigma) and
    log_ratio = (d / 2) ln 0.8 - (mu - m)^T Sigma^-1 (mu - m) / 10.

    The bar, measured on the CPU before any device run: 200 repetitions of N0 = 65 536 exact numpy draws
    gave sd(log_ratio) = 0.001055 at d = 2 and 0.005152 at d = 30, sd(mean_i) between 0.00300 and 0.00312
    sigma_i at d = 2 and between 0.00474 and 0.00566 sigma_i at d = 30, and ESS fractions of 0.935 and
    0.388 (smallest 0.934 and 0.379).  The number of snapshots of a run's window is only known once it has
    stopped, so the sd is carried to the run's count N = n_samples as sd0 sqrt(N0 / N) (the estimators
    are means of N terms).  The device result lies within 6 of those, the product's own jackknife errors
    within a factor 2 of them, and the ESS fraction stays above 0.25.

    Measured on an MI355X: d = 2 (N = 565 248): log_ratio -1.04 sd from the truth, the means within 2.09,
    jackknife / sd 0.96 and 1.05 ... 1.19, ESS fraction 0.935; d = 30 (N = 1 089 536): +2.04, 1.94, 0.89 and
    0.80 ... 1.00, 0.386."""
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
            "sampler": {"mcmc_hip": {"n_walkers": W, "seed": 11, "importance": {"wide": {"function": fn}}}}}
    _, smp = run(info)
    iw = smp.products()["importance"]
    N = iw.n_samples
    sd_lr, sd_mean = (v * math.sqrt(1.0 / N) for v in CALIBRATED[d])
    exact_lr = 0.5 * d * math.log(0.8) - (mu - m) @ np.linalg.solve(S, mu - m) / 10
    exact_mean, exact_cov = 0.8 * mu + 0.2 * m, 0.8 * S
    dev_lr = (iw.log_ratio("wide") - exact_lr) / sd_lr
    dev_mean = (iw.mean("wide") - exact_mean) / (sd_mean * sig)
    jk_lr, jk_mean = iw.log_ratio_stderr("wide") / sd_lr, iw.mean_stderr("wide") / (sd_mean * sig)
    print("d", d, "N", N, "n_acc", iw.n_acc, "ESS fraction", iw.ess_fraction("wide"))
    print(" log_ratio", iw.log_ratio("wide"), "exact", exact_lr, "in sd", dev_lr, "jackknife / sd", jk_lr)
    print(" means in sd: max", np.abs(dev_mean).max(), "jackknife / sd: min", jk_mean.min(), "max", jk_mean.max())
    print(" cov rel err max", np.abs(iw.cov("wide") / exact_cov - 1).max() if d == 2 else
          np.abs(np.diag(iw.cov("wide")) / np.diag(exact_cov) - 1).max(),
          "host seconds per snapshot in the function", next(p for p in smp._products if p.name == "importance").eval_seconds / iw.n_acc)
    assert iw.ess_fraction("wide") > 0.25 and iw.nonfinite("wide") == iw.clamped("wide") == 0
    assert abs(dev_lr) <= 6 and np.all(np.abs(dev_mean) <= 6)
    assert 0.5 <= jk_lr <= 2 and np.all((jk_mean >= 0.5) & (jk_mean <= 2))
    smp.close()
