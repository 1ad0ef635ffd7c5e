"""Streaming marginal histograms on the MI355X (marginal_kernels.hip, mcmc_hip_marginals_*): the
counts equal the rule of DESIGN.md section 2 ("Marginals") -- `rule_slab` of
tests/test_marginals_host.py: numpy with the kernel's own operations, NOT np.histogram, which
treats values within an ulp of an edge differently -- with INTEGER equality, at the smallest shapes
at which the kernel can still go wrong; the read-out is stream-ordered; the sampler's product counts
exactly the snapshots of its window."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402,F401  (before the first Engine: one HIP runtime for both)

from cobaya_amd import run  # noqa: E402
from cobaya_amd.engine import ERR_ARG, ERR_STATE, Engine, EngineError  # noqa: E402
from tests.test_marginals_host import rule_slab  # noqa: E402


def _gauss_engine(d, W, gs, seed=11, incremental=False, walker_offset=0, x0=None, target="gaussian"):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((d, d)) / np.sqrt(d)
    cov = 0.004 * (0.5 * A @ A.T + 0.5 * np.eye(d))
    mean = 0.5 + 0.02 * rng.standard_normal(d)
    eng = Engine(d, W, group_size=gs, device=0, seed=seed, incremental=incremental,
                 walker_offset=walker_offset)
    eng.set_prior([0] * d, [0.0] * d, [1.0] * d)
    if target == "one":
        eng.set_target_one()
    else:
        eng.set_target_gaussian_mixture([mean], [cov])
    eng.set_proposal_cov(cov)
    if x0 is None:
        x0 = np.clip(mean + rng.standard_normal((W, d)) * np.sqrt(np.diag(cov)), 0.01, 0.99)
    eng.set_state(x0)
    return eng, mean, cov, x0


def _ranges(mean, cov):
    """Asymmetric and narrower than where the walkers go: under, over and outside all occur."""
    sd = np.sqrt(np.diag(cov))
    return mean - 1.1 * sd, mean + 1.7 * sd


SHAPES = [   # (d, W, group, incremental, pairs)
    (2, 128, 64, False, [(0, 1), (1, 0)]),
    (5, 192, 64, False, [(3, 1), (1, 3), (0, 4)]),      # W is no multiple of 256; row / column roles
    (33, 256, 64, False, [(32, 0), (5, 31)]),           # the d > 32 state path
    (130, 256, 64, True, [(129, 0), (64, 128)]),        # d > 128: huge_kernels.hip keeps x as [d][W] too
]


@pytest.mark.parametrize("d, W, gs, inc, pairs", SHAPES, ids=lambda v: str(v) if isinstance(v, int) else None)
def test_counts_equal_the_rule(d, W, gs, inc, pairs):
    """Fails without the feature: the entry points do not exist."""
    eng, mean, cov, _ = _gauss_engine(d, W, gs, incremental=inc)
    lo, hi = _ranges(mean, cov)
    dims1 = sorted({0, d - 1, d // 2})
    for bins1, bins2 in ((1, 1), (7, 3), (1024, 64)):
        eng.configure_marginals(dims1, bins1, pairs, bins2, lo, hi)
        lay = eng.marginals_layout()
        assert lay["n_counters"] == len(dims1) * (bins1 + 2) + len(pairs) * (bins2 * bins2 + 1)
        assert lay["offset_pairs"] == len(dims1) * (bins1 + 2) and (lay["n1"], lay["n2"]) == (len(dims1), len(pairs))
        want = np.zeros(lay["n_counters"], np.uint64)
        for _ in range(3):
            eng.step(3)
            eng.accumulate_marginals()
            want += rule_slab(eng.get_state()["x"], dims1, bins1, pairs, bins2, lo, hi)
        eng.request_marginals()
        got, n = eng.fetch_marginals()
        assert n == 3 and got.dtype == np.uint64
        assert np.array_equal(got, want)
        assert int(got[:bins1 + 2].sum()) == 3 * W                      # every walker is counted once
        assert 0 < int(got[0]) and 0 < int(got[1])                      # under and over both occur
        assert 0 < int(got[lay["offset_pairs"]]) < 3 * W                # ... and a pair's outside
    eng.close()


def test_crafted_states_on_the_edges():
    """[0, 1] with 8 bins inside a prior on [-1, 2]: walkers exactly at 0, at 1, at every interior
    edge k / 8 and one ulp on either side of an edge; a value on an edge lands in the UPPER bin, 1.0
    in the last; what lies outside is counted as under / over / outside, exactly."""
    d, W = 2, 128
    eng = Engine(d, W, group_size=64, device=0, seed=3)
    eng.set_prior([0, 0], [-1.0, -1.0], [2.0, 2.0])
    eng.set_target_one()
    eng.set_proposal_cov(0.01 * np.eye(d))
    edges = [k / 8 for k in range(1, 8)]
    col = ([0.0, 1.0] + edges + [np.nextafter(e, -1.0) for e in edges] + [np.nextafter(e, 2.0) for e in edges]
           + [np.nextafter(0.0, -1.0), -0.5, -0.75, np.nextafter(1.0, 2.0), 1.5])
    x = np.full((W, d), 0.5)
    x[:len(col), 0] = col
    x[:, 1] = 0.3
    x[100, 1], x[101, 1], x[102, 1] = -0.25, 1.25, np.nextafter(1.0, 2.0)   # only the SECOND coordinate is out
    x[0, 1] = 1.0                                                    # (0, 1): in range, last column
    eng.set_state(x)
    lo, hi = np.zeros(d), np.ones(d)
    eng.configure_marginals([0, 1], 8, [(0, 1), (1, 0)], 8, lo, hi)
    eng.accumulate_marginals()
    eng.request_marginals()
    got, n = eng.fetch_marginals()
    assert n == 1 and np.array_equal(got, rule_slab(x, [0, 1], 8, [(0, 1), (1, 0)], 8, lo, hi))
    # ... and stated by hand for the first parameter: 0 -> bin 0; k/8 and its upper neighbour -> bin
    # k; its lower neighbour -> bin k - 1; 1.0 -> bin 7; the filler 0.5 -> bin 4
    hand = np.zeros(8, np.int64)
    hand[0] += 1
    hand[7] += 1
    for k in range(1, 8):
        hand[k] += 2
        hand[k - 1] += 1
    hand[4] += W - len(col)
    assert np.array_equal(got[2:10].astype(np.int64), hand)
    assert (int(got[0]), int(got[1])) == (3, 2)                      # under: three below 0; over: two above 1
    under2, over2 = int(got[10]), int(got[11])
    assert (under2, over2) == (1, 2)
    off = 20
    assert int(got[off]) == 5 + 3 and int(got[off + 65]) == 5 + 3    # outside: either coordinate out (disjoint walkers)
    c01 = got[off + 1:off + 65].reshape(8, 8)
    assert int(c01[0, 7]) == 1                                        # walker 0: (0.0, 1.0) -> row 0, LAST column
    c10 = got[off + 66:].reshape(8, 8)
    assert np.array_equal(c10, c01.T)
    eng.close()


def test_all_walkers_in_one_bin_twice():
    """The serialised-atomics case: 256 walkers on one point, two accumulations -> exactly 512."""
    d, W = 2, 256
    x = np.full((W, d), 0.5)
    eng, *_ = _gauss_engine(d, W, 64, x0=x)
    eng.configure_marginals([0, 1], 7, [(0, 1)], 3, np.zeros(d), np.ones(d))
    eng.accumulate_marginals()
    eng.accumulate_marginals()
    eng.request_marginals()
    got, n = eng.fetch_marginals()
    assert n == 2
    want = np.zeros_like(got)
    want[2 + 3] = want[9 + 2 + 3] = 512           # floor(0.5 * 7) = 3
    want[18 + 1 + 1 * 3 + 1] = 512                # floor(0.5 * 3) = 1 on both axes
    assert np.array_equal(got, want)
    eng.close()


def test_two_shards_add_up_to_the_whole_ensemble():
    d, W = 5, 256
    whole, mean, cov, x0 = _gauss_engine(d, W, 64, seed=19)
    lo, hi = _ranges(mean, cov)
    cfg = ([0, 2, 4], 16, [(1, 3), (4, 0)], 5, lo, hi)
    parts = [_gauss_engine(d, W // 2, 64, seed=19, walker_offset=k * (W // 2),
                           x0=x0[k * (W // 2):(k + 1) * (W // 2)])[0] for k in range(2)]
    out = []
    for eng in [whole] + parts:
        eng.configure_marginals(*cfg)
        for _ in range(2):
            eng.step(4)
            eng.accumulate_marginals()
        eng.request_marginals()
        out.append(eng.fetch_marginals()[0])
    assert np.array_equal(np.vstack([p.get_state()["x"] for p in parts]), whole.get_state()["x"])
    assert np.array_equal(out[1] + out[2], out[0]) and int(out[0][:18].sum()) == 2 * W
    for eng in [whole] + parts:
        eng.close()


def test_request_resets_in_stream_order_and_set_continues_the_count():
    d, W = 3, 128
    eng, mean, cov, _ = _gauss_engine(d, W, 64, seed=23)
    lo, hi = _ranges(mean, cov)
    cfg = ([0, 1, 2], 12, [(2, 0)], 4)
    with pytest.raises(EngineError) as ei:        # no slab yet
        eng.accumulate_marginals()
    assert ei.value.code == ERR_STATE
    eng.configure_marginals(*cfg, lo, hi)
    with pytest.raises(EngineError) as ei:
        eng.fetch_marginals()
    assert ei.value.code == ERR_STATE
    eng.step(2)
    eng.accumulate_marginals()
    first = rule_slab(eng.get_state()["x"], *cfg, lo, hi)
    eng.request_marginals()
    eng.step(2)
    eng.accumulate_marginals()                    # queued AFTER the request: the next fetch's
    second = rule_slab(eng.get_state()["x"], *cfg, lo, hi)
    got, n = eng.fetch_marginals()
    assert n == 1 and np.array_equal(got, first)
    eng.request_marginals()
    got, n = eng.fetch_marginals()
    assert n == 1 and np.array_equal(got, second) and not np.array_equal(first, second)
    eng.request_marginals()
    got, n = eng.fetch_marginals()
    assert n == 0 and not got.any()
    # resume: the counts of an unfinished interval go back, the next accumulation adds to them
    eng.marginals_set(first, 3)
    eng.step(1)
    eng.accumulate_marginals()
    third = rule_slab(eng.get_state()["x"], *cfg, lo, hi)
    eng.request_marginals()
    got, n = eng.fetch_marginals()
    assert n == 4 and np.array_equal(got, first + third)
    with pytest.raises(EngineError) as ei:
        eng.marginals_set(first[:-1], 1)
    assert ei.value.code == ERR_ARG and "counts" in str(ei.value)
    # a bad configuration names its argument and leaves the old slab alone
    for kw, word in ((dict(dims1=[3]), "dims1"), (dict(pairs=[(1, 1)]), "pairs"), (dict(bins1=1025), "bins1"),
                     (dict(bins2=65), "bins2"), (dict(pairs=[(0, 7)]), "pairs"),
                     (dict(hi=np.array([np.inf, 1, 1])), "hi"), (dict(lo=hi), "lo")):
        a = dict(dims1=[0, 1, 2], bins1=12, pairs=[(2, 0)], bins2=4, lo=lo, hi=hi)
        a.update(kw)
        with pytest.raises(EngineError) as ei:
            eng.configure_marginals(**a)
        assert ei.value.code == ERR_ARG and word in str(ei.value), (word, str(ei.value))
    assert eng.marginals_layout()["n_counters"] == 3 * 14 + 17
    eng.configure_marginals()                     # n1 = n2 = 0: off, the slab is freed
    assert eng.marginals_layout()["n_counters"] == 0
    with pytest.raises(EngineError):
        eng.accumulate_marginals()
    eng.close()


def test_around_the_one_likelihood_and_a_device_function():
    eng, mean, cov, _ = _gauss_engine(4, 128, 64, seed=29, target="one")
    lo, hi = np.full(4, 0.25), np.full(4, 0.8)
    cfg = ([0, 3], 9, [(1, 2)], 6, lo, hi)
    eng.configure_marginals(*cfg)
    eng.step(5)
    eng.accumulate_marginals()
    want = rule_slab(eng.get_state()["x"], *cfg)
    eng.request_marginals()
    assert np.array_equal(eng.fetch_marginals()[0], want)
    eng.close()

    def banana(p):                      # the banana of tests/test_gpu_function_target.py
        return -0.5 * (p[:, 0] ** 2 + ((p[:, 1] - 0.5 * p[:, 0] ** 2) / 0.5) ** 2)

    eng = Engine(2, 128, group_size=64, device=0, seed=31)
    eng.set_prior([0, 0], [-8.0, -6.0], [8.0, 30.0])
    eng.set_target_function(banana)
    eng.set_proposal_cov(np.eye(2))
    rng = np.random.default_rng(31)
    eng.set_state(np.column_stack((rng.normal(0, 1, 128), rng.normal(0.5, 0.5, 128))))
    lo, hi = np.array([-1.5, -0.5]), np.array([1.5, 2.0])
    cfg = ([0, 1], 32, [(0, 1)], 8, lo, hi)
    eng.configure_marginals(*cfg)
    eng.step(8)
    assert eng.last_step_kernel().startswith("mcmc::fn_walker_kernel")
    eng.accumulate_marginals()
    want = rule_slab(eng.get_state()["x"], *cfg)
    eng.request_marginals()
    got, n = eng.fetch_marginals()
    assert n == 1 and np.array_equal(got, want) and int(got[:34].sum()) == 128
    eng.close()


# ------------------------------------------------------------------------------ end to end
def _quickstart(**opts):
    o = {"n_walkers": 4096, "seed": 7, "Rminus1_stop": 0.0, "max_samples": 3.0e6,
         "steps_per_launch": 40, "moments_every": 1, "snapshot_every": 40, "max_rows": 1 << 22}
    o.update(opts)
    return {"likelihood": {"gaussian_mixture": {"means": [0.2, 0], "covs": [[0.1, 0.05], [0.05, 0.2]]}},
            "params": {"a": {"prior": {"min": -0.5, "max": 3}},
                       "b": {"prior": {"dist": "norm", "loc": 0, "scale": 1}, "ref": 0, "proposal": 0.5}},
            "sampler": {"mcmc_hip": o}}


def test_run_counts_the_window_exactly_as_the_rule_on_the_stored_rows():
    """README quickstart with `marginals: True`: every accumulated snapshot is also stored
    (moments_every 1, snapshot_every = one launch, max_rows large enough), so the product must equal
    the rule applied to the stored rows of the window's snapshots -- exactly."""
    W = 4096
    _, s = run(_quickstart(marginals=True))
    prod = s.products()
    m = prod["marginals"]
    assert m.n_accumulations == sum(iv[0] for iv in s._intervals) + s._snaps_in_interval
    assert m.n_samples == m.n_accumulations * W and 0 < s._dropped_snapshots
    x = prod["sample"].data[["a", "b"]].to_numpy()
    assert len(x) == (s._dropped_snapshots + m.n_accumulations) * W      # nothing was thinned away
    xs = x[-m.n_samples:]                                                # the window's snapshots
    lo, hi = np.array([-0.5, -5.0]), np.array([3.0, 5.0])                # ranges: "prior"
    assert m.ranges == {"a": (-0.5, 3.0), "b": (-5.0, 5.0)} and m.bins == 128 and m.pairs == []
    want = rule_slab(xs, [0, 1], 128, [], 32, lo, hi)
    assert np.array_equal(m.slab, want)
    for i, name in enumerate(("a", "b")):
        assert m.outside(name) == (0, 0)
        # the binning bound: with nothing outside, the histogram mean lies within half a bin width
        # of the mean of the same samples
        half = 0.5 * (hi[i] - lo[i]) / 128
        print(name, "histogram mean", m.mean(name), "sample mean", xs[:, i].mean(), "half bin", half)
        assert abs(m.mean(name) - xs[:, i].mean()) <= half
        assert int(m.counts(name).sum()) == m.n_samples
    s.close()
    assert s.products()["marginals"] == m        # the product outlives the engine


def test_without_the_option_no_slab_exists_and_no_marginal_kernel_can_run():
    _, s = run(_quickstart(max_samples=4.0e5))
    assert "marginals" not in s.products()
    assert s.engine.marginals_layout()["n_counters"] == 0
    with pytest.raises(EngineError) as ei:       # (the launch needs the slab the option allocates)
        s.engine.accumulate_marginals()
    assert ei.value.code == ERR_STATE
    s.close()
