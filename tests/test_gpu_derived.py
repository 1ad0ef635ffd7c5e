"""Derived parameters on the MI355X (derived_kernels.hip, mcmc_hip_derived_*, cobaya_amd/derived.py):
the sums equal the rule of DESIGN.md section 2 ("Derived") -- tests/derived_ref.py, numpy -- bit for
bit on crafted values at the smallest shapes at which the kernel can still go wrong (one chunk of 64
walkers per group and several; a group that is no multiple of the chunk; one group of 8192 walkers,
far larger than the LDS tile; 1, 3 and 32 derived rows, i.e. one pass of eight rows and five; no
cross column, a few, and 200 of them, i.e. one block of 32 columns and seven); the marginals read
the derived rows; and `run` carries the functions through rows, products, files and a resume.
Every test fails without the feature: the entry points and the option do not exist.

The engine is created with group_size 64, 128 or 256 only; the groups of 96 and 8192 walkers are
those of the derived sums alone (`derived_set_group_size`)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402,F401  (before the first Engine: one HIP runtime for both)

from cobaya_amd import run  # noqa: E402
from cobaya_amd.derived import Derived  # noqa: E402
from cobaya_amd.engine import ERR_ARG, ERR_CALLBACK, ERR_STATE, Engine, EngineError  # noqa: E402
from cobaya_amd.sampler import LoggedError  # noqa: E402
from tests.derived_ref import Rule, same, zero  # noqa: E402
from tests.test_marginals_host import rule_slab  # noqa: E402


def _engine(d, W, gs):
    """An engine that serves d (d > 128: the huge path, which wants incremental evaluation of a
    Gaussian); its state is crafted, nothing is stepped."""
    big = d > 128
    eng = Engine(d, W, group_size=gs, device=0, seed=3, incremental=big)
    eng.set_prior([0] * d, [-50.0] * d, [50.0] * d)
    if big:
        eng.set_target_gaussian_mixture([np.zeros(d)], [np.eye(d)])
    else:
        eng.set_target_one()
    eng.set_proposal_cov(0.01 * np.eye(d))
    return eng


def _state(x, step=1):
    W = len(x)
    z = np.zeros(W, np.int32)
    return {"x": np.ascontiguousarray(x, dtype=np.float64), "logpost": np.zeros(W), "logprior": np.zeros(W),
            "loglike": np.zeros(W), "weight": z + 1, "prior_rej": z, "burn_left": z,
            "n_accept": np.zeros(W, np.int64), "step": np.uint64(step)}


def _crafted(W, d, m, gs, rng, k):
    """(x[W, d], z[W, m]): values of order one with NaN, +-inf, -0.0, denormals and +-1e300 (finite,
    with overflowing products) among them, and one group without a used walker."""
    x = rng.uniform(-3.0, 3.0, (W, d))
    z = rng.standard_normal((W, m)) * rng.uniform(0.5, 4.0, m) + rng.uniform(-2.0, 2.0, m)
    j = lambda q: q % m   # noqa: E731
    z[3 + k, j(0)] = np.nan
    z[7, j(1)] = np.inf
    z[11, j(2)] = -np.inf
    z[12, j(0)], z[12, j(1)] = np.nan, np.inf          # two non-finite values of one walker
    z[17, j(1)] = -0.0
    z[18, j(2)] = 5e-324
    z[19, j(0)] = -2.2250738585072014e-308 / 4
    z[23, j(k)] = 1e300
    z[29, j(k + 1)] = -1e300
    z[W - 1, j(2)] = 1e300                             # the last walker of the last group
    if W // gs > 1 and k == 0:
        z[gs:2 * gs, j(1)] = np.nan                    # group 1: no used walker
    return x, z


SHAPES = [(512, gs, gs, 3, m, nc) for gs in (64, 256) for m in (1, 3, 32) for nc in (0, 3)]
SHAPES += [(192, 64, 96, 3, 3, 3),          # a group of one chunk and a half
           (8192, 64, 8192, 3, 3, 3),       # ONE group: 128 chunks, the chains carried in registers
           (256, 64, 64, 200, 3, 200)]      # seven blocks of columns; cross indices up to 199


@pytest.mark.parametrize("W, gs_engine, gs, d, m, n_cross", SHAPES)
def test_the_sums_equal_the_rule_bit_for_bit(W, gs_engine, gs, d, m, n_cross):
    rng = np.random.default_rng(10000 * m + 100 * n_cross + W + gs)
    eng = _engine(d, W, gs_engine)
    assert eng.derived_layout() == {"m": 0, "n_cross": 0, "group_size": 0, "n_accumulations": 0}
    cross = list(range(d))[::-1][:n_cross]              # (not in ascending order)
    shift, xshift = rng.uniform(-1.0, 1.0, m), rng.uniform(-1.0, 1.0, d)
    eng.configure_derived(m, cross, shift)
    if gs != gs_engine:
        eng.derived_set_group_size(gs)
    assert eng.derived_layout() == {"m": m, "n_cross": n_cross, "group_size": gs, "n_accumulations": 0}
    rule = Rule(W, gs, m, cross, shift, xshift)
    data = [_crafted(W, d, m, gs, rng, k) for k in range(3)]
    for k, (x, z) in enumerate(data[:2]):
        eng.set_full_state(_state(x, k + 1))
        if k == 0:
            eng.set_moment_shift(xshift)
        eng.derived_set_values(z)
        assert eng.derived_get_values().tobytes() == z.tobytes()
        eng.accumulate_derived()
        rule.accumulate(x, z)
    eng.request_derived()
    got = eng.fetch_derived()
    want = rule.request()
    same(got, want)
    assert got["n"] == 2 and 0 < got["N"] < 2 * W and got["bad"].sum() >= 8
    print("W", W, "gs", gs, "d", d, "m", m, "n_cross", n_cross, "N", got["N"], "bad", got["bad"].tolist(),
          "non-finite sums", int((~np.isfinite(got["B"])).sum()), "of", got["B"].size)
    assert not np.isfinite(got["B"]).all()              # (1e300 squared overflowed, as the rule's did)
    # the read-out zeroed the accumulators
    eng.request_derived()
    same(eng.fetch_derived(), zero(m, n_cross))
    # set, then one more accumulation = three uninterrupted accumulations
    eng.derived_set(got)
    rule.set(want)
    x, z = data[2]
    eng.set_full_state(_state(x, 3))
    eng.derived_set_values(z)
    eng.accumulate_derived()
    rule.accumulate(x, z)
    eng.request_derived()
    got3 = eng.fetch_derived()
    same(got3, rule.request())
    whole = Rule(W, gs, m, cross, shift, xshift)
    for x, z in data:
        whole.accumulate(x, z)
    same(got3, whole.request())
    assert got3["n"] == 3
    eng.close()


def test_benign_values_give_finite_moments_and_bad_calls_name_their_argument():
    d, W, gs, m = 3, 256, 128, 2
    rng = np.random.default_rng(5)
    eng = _engine(d, W, gs)
    for call in (eng.accumulate_derived, eng.request_derived, eng.derived_buffers):
        with pytest.raises(EngineError) as ei:
            call()
        assert ei.value.code == ERR_STATE and "derived_configure" in str(ei.value)
    for kw, word in ((dict(m=33, shift=np.zeros(33)), "m ="), (dict(cross_dims=[3]), "cross_dims"), (dict(cross_dims=[1, 1]), "duplicate"),
                     (dict(shift=[0.0, np.inf]), "shift")):
        with pytest.raises(EngineError) as ei:
            eng.configure_derived(**{"m": m, "cross_dims": [0], "shift": [0.0, 0.0], **kw})
        assert ei.value.code == ERR_ARG and word in str(ei.value), str(ei.value)
    eng.configure_derived(m, [0, 2], [0.5, -0.5])
    with pytest.raises(EngineError) as ei:
        eng.derived_set_group_size(100)
    assert ei.value.code == ERR_ARG and "group_size" in str(ei.value)
    x, z = rng.uniform(-1, 1, (W, d)), rng.standard_normal((W, m))
    eng.set_full_state(_state(x))
    eng.derived_set_values(z)
    eng.accumulate_derived()
    eng.request_derived()
    with pytest.raises(EngineError) as ei:
        eng.request_derived()
    assert ei.value.code == ERR_STATE and "pending" in str(ei.value)
    got = eng.fetch_derived()
    rule = Rule(W, gs, m, [0, 2], [0.5, -0.5], np.zeros(d))
    rule.accumulate(x, z)
    same(got, rule.request())
    prod = Derived(["u", "v"], ["a", "c"], [0.5, -0.5], [0.0, 0.0], W, got["N"], got["A"], got["B"], got["C"],
                   got["X"], got["V"], got["bad"], got["min"], got["max"])
    np.testing.assert_allclose([prod.mean("u"), prod.mean("v")], z.mean(0), rtol=1e-12)
    np.testing.assert_allclose(prod.cov(), np.cov(z.T, ddof=0), rtol=1e-10)
    full = np.cov(np.column_stack((z, x[:, [0, 2]])).T, ddof=0)
    np.testing.assert_allclose([prod.cross_cov("u", "a"), prod.cross_cov("v", "c")], [full[0, 2], full[1, 3]],
                               rtol=1e-9, atol=1e-15)
    np.testing.assert_allclose(prod.corr("u", "c"), np.corrcoef(z[:, 0], x[:, 2])[0, 1], rtol=1e-9, atol=1e-15)
    assert (prod.min("u"), prod.max("v")) == (z[:, 0].min(), z[:, 1].max()) and prod.nonfinite("u") == 0
    eng.configure_derived(0)
    assert eng.derived_layout()["m"] == 0
    eng.close()


# ------------------------------------------------------------------------------ marginals over derived rows
def test_marginals_read_the_derived_rows_and_nan_behaves_as_documented():
    d, W, gs, m = 3, 512, 64, 2
    rng = np.random.default_rng(8)
    x = rng.uniform(-1.0, 1.0, (W, d))
    z = np.column_stack((x[:, 0] + x[:, 1], x[:, 0] * x[:, 2]))
    z[5, 0], z[9, 1], z[300, 0] = np.nan, np.nan, np.inf
    z[6, 0], z[7, 0], z[8, 0] = -1.5, 1.5, 0.0          # the walls and an interior edge
    lo = np.array([-1.0, -1.0, -1.0, -1.5, -0.8])
    hi = np.array([1.0, 1.0, 1.0, 1.5, 0.8])
    cfg = ([0, 3, 4], 16, [(1, 3), (4, 2), (3, 4)], 6, lo, hi)

    eng = _engine(d, W, gs)
    with pytest.raises(EngineError) as ei:               # no derived rows yet: 3 is no index
        eng.configure_marginals([3], 16, [], 6, lo[:3], hi[:3])
    assert ei.value.code == ERR_ARG
    eng.configure_derived(m, [], [0.0, 0.0])
    eng.configure_marginals(*cfg)
    with pytest.raises(EngineError) as ei:               # (the entries read z: it cannot go away)
        eng.configure_derived(0)
    assert ei.value.code == ERR_STATE and "marginals" in str(ei.value)
    eng.set_full_state(_state(x))
    eng.derived_set_values(z)
    eng.accumulate_marginals()
    eng.request_marginals()
    got, n = eng.fetch_marginals()
    want = rule_slab(np.column_stack((x, z)), *cfg)
    assert n == 1 and np.array_equal(got, want)
    e = got[18:36]                                       # the 1-D entry of derived row 0
    assert int(e.sum()) == W - 1 and e[1] >= 1           # the NaN is counted nowhere, +inf is `over`
    pair = got[3 * 18:3 * 18 + 37]                       # (sampled 1, derived 0): its NaN and inf are `outside`
    assert int(pair.sum()) == W and pair[0] >= 2
    # a sampled-only layout counts what it counts on an engine without derived rows
    only = ([0, 2], 16, [(1, 2)], 6, lo, hi)
    eng.configure_marginals(*only)
    eng.accumulate_marginals()
    eng.request_marginals()
    with_rows = eng.fetch_marginals()[0]
    eng.close()
    eng = _engine(d, W, gs)
    eng.configure_marginals(*only[:4], lo[:3], hi[:3])
    eng.set_full_state(_state(x))
    eng.accumulate_marginals()
    eng.request_marginals()
    today = eng.fetch_marginals()[0]
    assert np.array_equal(with_rows, today) and np.array_equal(today, rule_slab(x, *only[:4], lo[:3], hi[:3]))
    eng.close()


# ------------------------------------------------------------------------------ end to end
MEAN, COV = [0.3, -0.2], [[0.5, 0.2], [0.2, 0.4]]


def _info(**opts):
    o = {"n_walkers": 4096, "seed": 7, "Rminus1_stop": 0.0, "max_samples": 1.5e6, "steps_per_launch": 40,
         "moments_every": 1, "snapshot_every": 40, "max_rows": 1 << 22}
    o.update(opts)
    return {"likelihood": {"gaussian": {"mean": MEAN, "cov": COV}},
            "params": {"a": {"prior": {"min": -6, "max": 6}, "ref": {"dist": "norm", "loc": 0.3, "scale": 0.5}},
                       "b": {"prior": {"min": -6, "max": 6}, "ref": {"dist": "norm", "loc": -0.2, "scale": 0.5}},
                       "s": {"derived": "lambda a, b: a + b"},
                       "p": {"derived": lambda a, b: a * b}},
            "sampler": {"mcmc_hip": o}}


def test_run_carries_the_functions_through_rows_moments_and_marginals(tmp_path):
    W = 4096
    info = _info(marginals={"params": ["s", "a"], "ranges": {"s": [-8.0, 8.0]}, "bins": 128})
    info["output"] = str(tmp_path / "dv")
    _, smp = run(info)
    prod = smp.products()
    dv, mg, data = prod["derived"], prod["marginals"], prod["sample"].data
    assert list(prod["sample"].columns[:6]) == ["weight", "minuslogpost", "a", "b", "s", "p"]
    a, b, s, p = (data[k].to_numpy() for k in "absp")
    # every stored row: the derived columns from its own columns, bit for bit
    assert len(a) >= 4 * W and (a + b).tobytes() == s.tobytes() and (a * b).tobytes() == p.tobytes()
    n_acc = sum(iv[0] for iv in smp._intervals) + smp._snaps_in_interval
    assert dv.names == ["s", "p"] and dv.cross == ["a", "b"] and dv.n_samples == dv.n_used == n_acc * W > 0
    assert dv.nonfinite("s") == dv.nonfinite("p") == 0
    # mean(s) = the window's pooled means of a and b; the moments' own sums give them
    gsum = sum(iv[1].sum(0) for iv in smp._intervals)
    acc_n, acc_gs, _ = smp.engine.read_moments(reset=False)
    assert acc_n == smp._snaps_in_interval
    mean_ab = smp._shift + (gsum + acc_gs.sum(0)) / (n_acc * W)
    print("mean s", dv.mean("s"), "pooled a + b", mean_ab.sum(), "rel", dv.mean("s") / mean_ab.sum() - 1)
    np.testing.assert_allclose(dv.mean("s"), mean_ab.sum(), rtol=1e-9)
    np.testing.assert_allclose([dv.sampled_mean("a"), dv.sampled_mean("b")], mean_ab, rtol=1e-9)
    css, split = dv.cov()[0, 0], dv.cross_cov("s", "a") + dv.cross_cov("s", "b")
    print("cov ss", css, "cross a + cross b", split, "rel", css / split - 1)
    np.testing.assert_allclose(css, split, rtol=1e-9)
    # the window's snapshots are the last stored rows: the product is their moments
    ws = s[-dv.n_samples:]
    np.testing.assert_allclose([dv.mean("s"), dv.std("s")], [ws.mean(), ws.std()], rtol=1e-9)
    assert (dv.min("s"), dv.max("s")) == (ws.min(), ws.max())
    np.testing.assert_allclose(dv.corr("s", "p"), np.corrcoef(ws, p[-dv.n_samples:])[0, 1], rtol=1e-8)
    # mean(p) = mu_a mu_b + Sigma_ab within 6 standard errors, one snapshot as the independent sample
    true_p = MEAN[0] * MEAN[1] + COV[0][1]
    err = dv.std("p") / np.sqrt(W)
    print("mean p", dv.mean("p"), "true", true_p, "in standard errors", (dv.mean("p") - true_p) / err)
    assert abs(dv.mean("p") - true_p) <= 6 * err
    # marginals of s: nothing outside, so the histogram mean lies within half a bin of the mean
    assert mg.outside("s") == (0, 0) and int(mg.counts("s").sum()) == dv.n_samples
    half = 0.5 * 16.0 / 128
    print("histogram mean s", mg.mean("s"), "half bin", half)
    assert abs(mg.mean("s") - dv.mean("s")) <= half
    assert Derived.load(str(tmp_path / "dv.derived.npz")) == dv
    header = open(tmp_path / "dv.1.txt").readline().split()
    assert header[1:7] == ["weight", "minuslogpost", "a", "b", "s", "p"]
    smp.close()
    assert smp.products()["derived"] == dv        # the product outlives the engine


def test_a_resume_in_mid_run_is_bit_identical(tmp_path):
    from cobaya_amd.model import ProblemSpec
    from cobaya_amd.sampler import MCMCHip

    def make(prefix, resume, max_samples):
        info = _info()
        opts = {"seed": 21, "n_walkers": 512, "group_size": 64, "steps_per_launch": 40, "max_samples": max_samples,
                "Rminus1_stop": 0.0, "learn_every": "20d", "snapshot_every": 40,
                "marginals": {"params": ["p"], "ranges": {"p": [-4.0, 4.0]}}}
        return MCMCHip(opts, ProblemSpec.from_info(info), output=prefix, resume=resume)

    # (a run ends at the first checkpoint that sees max_samples: 30000 ends the first leg at an early
    # checkpoint, 150000 ends both runs at the same later one)
    a = make(str(tmp_path / "a"), False, 150000)
    a.run()
    pa = a.products()
    a.close()
    b1 = make(str(tmp_path / "b"), False, 30000)
    b1.run()
    assert b1.n_steps_raw < a.n_steps_raw
    b1.close()
    b2 = make(str(tmp_path / "b"), True, 150000)
    assert b2.n_steps_raw == b1.n_steps_raw
    b2.run()
    pb = b2.products()
    assert b2.n_steps_raw == a.n_steps_raw
    assert pb["derived"] == pa["derived"] and pa["derived"].n_used > 0
    assert pb["marginals"] == pa["marginals"]
    # the rows the resumed process stored itself, against the same rows of the uninterrupted run
    da, db = pa["sample"].data[["a", "b", "s", "p"]].to_numpy(), pb["sample"].data[["a", "b", "s", "p"]].to_numpy()
    assert len(da) == len(db) > 0
    n_own = sum(len(r) for r in b2._rows)
    assert n_own > 0 and da[-n_own:].tobytes() == db[-n_own:].tobytes()
    np.testing.assert_allclose(db[:-n_own], da[:-n_own], rtol=1e-7)      # (through the chain file: %.8g)
    b2.close()


def test_with_a_device_function_likelihood():
    def banana(pts):                    # the banana of the README
        return -0.5 * (pts[:, 0] ** 2 + ((pts[:, 1] - 0.5 * pts[:, 0] ** 2) / 0.5) ** 2)

    info = {"likelihood": {"banana": {"class": "device_function", "function": banana}},
            "params": {"a": {"prior": {"min": -8, "max": 8}, "ref": 0, "proposal": 1},
                       "b": {"prior": {"min": -6, "max": 30}, "ref": 0.5, "proposal": 1},
                       "c": {"derived": "lambda a, b: a * b"}},
            "sampler": {"mcmc_hip": {"n_walkers": 2048, "seed": 3, "group_size": 64, "max_tries": "2000d",
                                     "max_samples": 2048 * 300, "Rminus1_stop": 0.0}}}
    _, smp = run(info)
    assert smp.engine.last_step_kernel().startswith("mcmc::fn_walker_kernel")
    prod = smp.products()
    data, dv = prod["sample"].data, prod["derived"]
    a, b, c = (data[k].to_numpy() for k in "abc")
    assert len(c) > 0 and (a * b).tobytes() == c.tobytes()
    assert dv.names == ["c"] and dv.n_used == dv.n_samples > 0 and np.isfinite(dv.mean("c")) and dv.std("c") > 0
    assert dv.min("c") <= dv.mean("c") <= dv.max("c")
    smp.close()


# ------------------------------------------------------------------------------ errors
@pytest.mark.parametrize("bad, match", [
    (lambda a, b: (a + b)[:-1], r"'s'.*shape \(256,\), got shape \(255,\)"),
    (lambda a, b: (a + b).float(), "'s'.*dtype torch.float64, got dtype torch.float32"),
    (lambda a, b: (a + b).cpu(), "'s'.*device cuda:0, got device cpu"),
    (lambda a, b: [0.0] * len(a), "'s'.*must return a torch.Tensor, got list"),
])
def test_a_wrong_result_names_the_parameter(bad, match):
    info = _info(n_walkers=256, group_size=64)
    info["params"]["s"] = {"derived": bad}
    with pytest.raises(LoggedError, match=match):
        run(info)


def test_a_raising_function_surfaces_as_the_cause_and_the_next_run_works():
    state = {"calls": 0}

    def s(a, b):
        state["calls"] += 1
        if state["calls"] == 4:
            raise ValueError("boom at the user's side")
        return a + b

    info = _info(n_walkers=256, group_size=64, max_samples=1e9)
    info["params"]["s"] = {"derived": s}
    with pytest.raises(EngineError) as ei:
        run(info)
    assert ei.value.code == ERR_CALLBACK and "'s'" in str(ei.value)
    assert isinstance(ei.value.__cause__, ValueError) and "boom" in str(ei.value.__cause__)
    _, smp = run(_info(n_walkers=256, group_size=64, max_samples=2e5))     # a fresh sampler: works
    assert smp.products()["derived"].n_used > 0
    smp.close()


def test_derived_stats_false_sums_nothing_but_fills_the_rows():
    _, smp = run(_info(n_walkers=256, group_size=64, max_samples=2e5, derived_stats=False))
    data = smp.products()["sample"].data
    a, b, s = (data[k].to_numpy() for k in "abs")
    assert len(s) > 0 and (a + b).tobytes() == s.tobytes()
    assert smp.engine.derived_layout()["n_accumulations"] == 0 and smp.products()["derived"].n_used == 0
    smp.close()
