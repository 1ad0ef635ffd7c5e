"""Evidence of the run, host side (no GPU): the parsing of the sampler option `evidence` and its
refusals by name, the estimate and its jackknife on canned sums, the `clipped` rule at a wall, the
merge of shards, and the window bookkeeping of the sampler on an oracle-backed engine double that
serves the evidence methods in numpy (tests/evidence_ref.py: THE REFERENCE, the rule of DESIGN.md
section 2 "Evidence")."""
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest

from cobaya_amd.evidence import (DEFAULT_RADII, Evidence, EvidenceAccumulator, EvidenceError, clipped_radii,
                                 log_ball, log_volume, parse_option)
from cobaya_amd.model import ProblemSpec
from cobaya_amd.sampler import LoggedError, MCMCHip
from tests.evidence_ref import EvOracleEngine, Rule, ell_flat, rule_c, rule_linv, rule_s
from tests.oracle_engine import OracleEngine
from tests.test_host_logic import QUICK


class OnDouble(MCMCHip):
    _engine_factory = staticmethod(EvOracleEngine)


def acc(s):
    """The sampler's `EvidenceAccumulator` (None: the option is off)."""
    return next((p for p in s._products if p.name == "evidence"), None)


def make(prefix=None, max_samples=30000, resume=False, **opts):
    o = {"seed": 21, "n_walkers": 128, "group_size": 64, "steps_per_launch": 40,
         "max_samples": max_samples, "Rminus1_stop": 0.0, "learn_every": "20d",
         "snapshot_every": 40, "evidence": True}
    o.update(opts)
    return OnDouble(o, ProblemSpec.from_info(QUICK), output=prefix, resume=resume)


# ------------------------------------------------------------------------------- the option
def test_the_option_parses_to_radii_and_every():
    assert parse_option(None) is None and parse_option(False) is None
    assert parse_option(True) == {"radii": list(DEFAULT_RADII), "every": 1}
    assert DEFAULT_RADII == (0.5, 0.75, 1.0, 1.5, 2.0)
    assert parse_option({"radii": [1, 2.5], "every": 3}) == {"radii": [1.0, 2.5], "every": 3}
    assert parse_option({"radii": np.linspace(0.25, 2.0, 8)})["radii"] == list(np.linspace(0.25, 2.0, 8))
    assert parse_option({"every": 2.0})["every"] == 2


class NeverBuilt(EvOracleEngine):
    def __init__(self, *a, **k):
        raise AssertionError("the option must be refused before the engine is created")


class Refusing(MCMCHip):
    _engine_factory = staticmethod(NeverBuilt)


@pytest.mark.parametrize("opt, match", [
    ({"radii": []}, "evidence: radii must be 1..8 ascending positive numbers"),
    ({"radii": [0.5] * 2}, "evidence: radii must be"),
    ({"radii": [1.0, 0.5]}, "evidence: radii must be"),
    ({"radii": [0.0, 1.0]}, "evidence: radii must be"),
    ({"radii": [-1.0]}, "evidence: radii must be"),
    ({"radii": [1.0, float("inf")]}, "evidence: radii must be"),
    ({"radii": list(range(1, 10))}, "evidence: radii must be"),
    ({"radii": "wide"}, "evidence: radii must be"),
    ({"radii": 1.0}, "evidence: radii must be"),
    ({"radii": [True]}, "evidence: radii must be"),
    ({"every": 0}, "evidence: every must be an integer >= 1"),
    ({"every": 1.5}, "evidence: every must be"),
    ({"every": True}, "evidence: every must be"),
    ({"radius": [1.0]}, r"evidence: unknown key\(s\) \['radius'\]"),
    ("all", "evidence: expected True, None or a dict"),
])
def test_refusals_by_name_before_the_engine_is_created(opt, match):
    with pytest.raises(EvidenceError, match=match):
        parse_option(opt)
    with pytest.raises(LoggedError, match=match):
        Refusing({"n_walkers": 128, "group_size": 64, "evidence": opt}, ProblemSpec.from_info(QUICK))


def test_refusal_of_a_temperature_and_of_engines_without_the_methods():
    with pytest.raises(LoggedError, match="evidence: the sums weigh the walkers as they are, which at temperature 2"):
        Refusing({"n_walkers": 128, "group_size": 64, "evidence": True, "temperature": 2}, ProblemSpec.from_info(QUICK))

    class Old(MCMCHip):
        _engine_factory = staticmethod(OracleEngine)    # (no evidence entry points)
    with pytest.raises(LoggedError, match="evidence: this engine keeps no evidence sums"):
        Old({"n_walkers": 128, "group_size": 64, "evidence": True}, ProblemSpec.from_info(QUICK))
    s = Old({"n_walkers": 128, "group_size": 64}, ProblemSpec.from_info(QUICK))   # off: served as before
    assert "evidence" not in s.products()


# ------------------------------------------------------------------------------- the estimate
def test_the_estimate_and_the_jackknife_on_canned_sums():
    """Two intervals with different c, volume and n_acc; four groups of 64 walkers; by hand."""
    d, W, G = 3, 256, 4
    sums = np.array([[[3.0], [5.0], [4.0], [6.0]], [[30.0], [10.0], [20.0], [25.0]]])
    counts = np.array([[[7], [9], [8], [10]], [[70], [30], [50], [60]]], np.uint64)
    c, n_acc, lnvol = np.array([1.5, -2.0]), np.array([2, 10]), np.array([[0.3], [0.7]])
    ev = Evidence(d, [1.0], W, sums, counts, np.repeat(c[:, None], G, 1), n_acc, lnvol, np.zeros((2, 1), bool), 3)
    scale = np.exp(-c - lnvol[:, 0])                      # exp(-c) / volume per interval
    t = (sums[:, :, 0] * scale[:, None]).sum(0)           # per group, over the window
    N = n_acc.sum()
    # the n_acc-weighted mean of the intervals' Y = sum_g acc / (n_acc W) exp(-c) / vol
    Y_iv = sums[:, :, 0].sum(1) / (n_acc * W) * scale
    Y = (n_acc * Y_iv).sum() / N
    assert math.isclose(t.sum() / (W * N), Y, rel_tol=1e-15)
    assert math.isclose(ev.lnZ, -math.log(Y), rel_tol=1e-14, abs_tol=1e-14)
    loo = np.array([-math.log((t.sum() - t[g]) / ((W - 64) * N)) for g in range(G)])
    err = math.sqrt((G - 1) / G * ((loo - loo.mean()) ** 2).sum())
    assert math.isclose(ev.stderr, err, rel_tol=1e-12)
    assert ev.radius == 1.0 and ev.n_samples == 12 * W and ev.clamped == 3 and ev.n_groups == 4
    assert np.allclose(ev.inside_fraction(), counts.sum() / (12 * W), rtol=1e-15)
    assert "ln Z" in ev.summary() and "\n" not in ev.summary() and "clamped" in ev.summary()
    # equal groups: the jackknife sees no spread
    flat = Evidence(d, [1.0], W, np.full((1, G, 1), 2.0), np.ones((1, G, 1), np.uint64), np.zeros((1, G)), [1],
                    [[0.0]], [[False]])
    assert flat.stderr < 1e-15 and math.isclose(flat.lnZ, -math.log(8.0 / W), rel_tol=1e-15)
    # c far outside the range of exp: the logs carry it
    far = Evidence(d, [1.0], W, sums[:1], counts[:1], np.full((1, G), -5000.0), [2], [[0.3]], [[False]])
    assert math.isclose(far.lnZ, -(math.log(18.0) - math.log(2 * W) + 5000.0 - 0.3), rel_tol=1e-15)
    # nothing inside, or one group only
    none = Evidence(d, [1.0], W, np.zeros((1, G, 1)), np.zeros((1, G, 1), np.uint64), np.zeros((1, G)), [1],
                    [[0.0]], [[False]])
    assert math.isnan(none.lnZ) and none.radius is None and "no unclipped radius" in none.summary()
    one = Evidence(d, [1.0], 64, [[[2.0]]], [[[1]]], [[0.0]], [1], [[0.0]], [[False]])
    assert math.isclose(one.lnZ, -math.log(2.0 / 64)) and math.isnan(one.stderr)
    with pytest.raises(EvidenceError, match="evidence: the arrays"):
        Evidence(d, [1.0], W, sums, counts[:1], np.zeros((2, G)), n_acc, lnvol, np.zeros((2, 1), bool))


def test_the_headline_is_the_unclipped_radius_of_smallest_error():
    G = 4
    sums = np.zeros((1, G, 3))
    sums[0, :, 0] = [1.0, 3.0, 1.0, 3.0]          # wide spread
    sums[0, :, 1] = [2.0, 2.1, 2.0, 2.1]          # narrow
    sums[0, :, 2] = 2.0                           # none at all -- but clipped
    clip = np.array([[False, False, True]])
    ev = Evidence(2, [0.5, 1.0, 2.0], 256, sums, np.ones((1, G, 3), np.uint64), np.zeros((1, G)), [1],
                  np.zeros((1, 3)), clip)
    err = ev.stderr_by_radius()
    assert err[2] < err[1] < err[0] and ev.clipped().tolist() == [False, False, True]
    assert ev.radius == 1.0 and ev.lnZ == ev.lnZ_by_radius()[1] and ev.stderr == err[1]
    # a clip in an interval that accumulated nothing does not count
    ev2 = Evidence(2, [1.0], 256, np.ones((2, G, 1)), np.ones((2, G, 1), np.uint64), np.zeros((2, G)), [1, 0],
                   np.zeros((2, 1)), [[False], [True]])
    assert ev2.clipped().tolist() == [False]


def test_exact_gaussian_draws_give_ln_z_within_the_jackknife_error():
    """The reference rule over exact draws of a normalised Gaussian (Z = 1): d = 3, 2048 walkers."""
    d, W, gs = 3, 2048, 64
    rng = np.random.default_rng(5)
    A = rng.standard_normal((d, d))
    C = A @ A.T / d + 0.5 * np.eye(d)
    mu = rng.standard_normal(d)
    Lc = np.linalg.cholesky(C)

    def draws(n):
        x = mu + rng.standard_normal((n, d)) @ Lc.T
        q = np.sum(np.linalg.solve(Lc, (x - mu).T) ** 2, axis=0)
        return x, -0.5 * q - 0.5 * d * math.log(2 * math.pi) - np.log(np.diag(Lc)).sum()

    x0, _ = draws(W)                                 # the ellipsoid comes from an independent draw
    r2 = np.array(DEFAULT_RADII) * d
    rule = Rule(d, W, gs, r2)
    x, lp = draws(W)
    rule.set_ellipsoid(x0.mean(0), np.cov(x0.T), lp)
    rule.accumulate(x, lp)
    part = rule.request(True)
    lnvol = log_volume(part["active"], d, r2)
    ev = Evidence(d, DEFAULT_RADII, W, [part["sums"]], [part["counts"]], np.full((1, W // gs), part["active"][-1]),
                  [1], [lnvol], np.zeros((1, 5), bool), part["clamped"])
    # (the sd of ln Z over replications is about 0.025 at d = 2 with 4 096 draws, so about 0.035 with
    # 2 048; the jackknife of ONE replication over 32 groups, at the radius it likes best, is within
    # a factor of five below and three above that)
    assert ev.clamped == 0 and 0.007 < ev.stderr < 0.1
    assert abs(ev.lnZ) < 5 * ev.stderr
    assert np.all(np.abs(ev.lnZ_by_radius()) < 5 * ev.stderr_by_radius())
    frac = ev.inside_fraction()
    assert np.all(np.diff(frac) > 0) and 0.35 < frac[2] < 0.8       # chi2_3 <= 3: 0.61
    assert math.isclose(log_ball(3), math.log(4 * math.pi / 3), rel_tol=1e-14)


def test_a_radius_is_clipped_when_its_bounding_box_leaves_the_prior_box():
    d = 2
    C = np.array([[0.04, 0.01], [0.01, 0.09]])
    m = np.array([0.5, -1.0])
    ell = ell_flat(m, rule_linv(C))
    r2 = np.array([0.5, 1.0, 2.0]) * d
    sig = np.sqrt(np.diag(C))
    inf = np.inf
    assert clipped_radii(ell, d, r2, [-inf, -inf], [inf, inf]).tolist() == [False] * 3
    # the wall between the second and the third radius, in either dimension and on either side
    for i in range(d):
        for side in (-1, 1):
            lo, hi = np.full(d, -inf), np.full(d, inf)
            wall = m[i] + side * 1.7 * sig[i]                     # sqrt(2) < 1.7 < 2
            (hi if side > 0 else lo)[i] = wall
            assert clipped_radii(ell, d, r2, lo, hi).tolist() == [False, False, True]
    # on the wall is inside; one step of the wall towards the centre is not.  (sigma comes back from
    # Linv: the wall is put where the product's own arithmetic has it)
    L = np.linalg.inv(rule_linv(C))
    edge = m[0] + math.sqrt(r2[1]) * np.sqrt(np.sum(np.tril(L) ** 2, axis=1))[0]
    assert clipped_radii(ell, d, r2, [-inf, -inf], [edge, inf]).tolist() == [False, False, True]
    assert clipped_radii(ell, d, r2, [-inf, -inf], [np.nextafter(edge, -inf), inf]).tolist() == [False, True, True]
    assert math.isclose(log_volume(ell, d, r2)[1],
                        math.log(math.pi * r2[1] * math.sqrt(np.linalg.det(C))), rel_tol=1e-13)


# ------------------------------------------------------------------------------- shards
def _host(W, size=1, rank=0, reduce=None):
    return SimpleNamespace(fail=None, n_walkers=W, size=size, rank=rank, temperature=1.0, snapshot_steps=40,
                           all_reduce_sum=reduce)


def _population(W, d, seed):
    rng = np.random.default_rng(seed)
    x = 0.3 * rng.standard_normal((W, d))
    lp = -0.5 * np.sum((x / 0.3) ** 2, axis=1)
    lp[[5, W // 2 + 9]] = 1.0          # the maximum, once in either half: both shards take the same c
    return x, lp


def test_two_shards_merge_to_the_whole_and_combine_through_one_all_reduce():
    spec = ProblemSpec.from_info(QUICK)
    d, W, gs = 2, 256, 64
    r2 = np.array(DEFAULT_RADII) * d
    C = 0.09 * np.eye(d)
    states = [_population(W, d, s) for s in (1, 2, 3)]

    def run(sl):
        rule = Rule(d, sl.stop - sl.start, gs, r2)
        rule.set_ellipsoid(np.zeros(d), C, states[0][1][sl])
        rule.accumulate(states[0][0][sl], states[0][1][sl])
        rule.set_ellipsoid(0.01 * np.ones(d), 1.1 * C)
        parts = [rule.request(True, states[1][1][sl])]
        for x, lp in states[1:]:
            rule.accumulate(x[sl], lp[sl])
        parts.append(rule.request(True, states[2][1][sl]))
        return parts

    whole, halves = run(slice(0, W)), [run(slice(0, W // 2)), run(slice(W // 2, W))]
    assert whole[0]["active"][-1] == 1.0 and np.array_equal(halves[1][1]["active"], whole[1]["active"])
    for k in range(2):     # a shard's groups are bit for bit the same groups of the whole ensemble
        assert np.array_equal(np.vstack([h[k]["sums"] for h in halves]), whole[k]["sums"])
        assert np.array_equal(np.vstack([h[k]["counts"] for h in halves]), whole[k]["counts"])

    def product(parts, host):
        a = EvidenceAccumulator(parse_option(True), spec, host)
        a.ivs, a.open = [parts[0]], parts[1]
        return a, a.product([], combined=host.size > 1)

    ref = product(whole, _host(W))[1]
    assert ref.n_acc.tolist() == [1, 2] and ref.n_groups == 4 and ref.n_samples == 3 * W
    pa, pb = (product(h, _host(W // 2))[1] for h in halves)
    assert pa.merge(pb) == ref and pa.merge(pb).lnZ == ref.lnZ and pa.merge(pb).stderr == ref.stderr
    assert pa != ref and pa.n_groups == 2
    with pytest.raises(EvidenceError, match="evidence: only shards of one run"):
        pa.merge(Evidence(d, [1.0], 128, pa.sums[:, :, :1], pa.counts[:, :, :1], pa.c, pa.n_acc, pa.lnvol[:, :1],
                          pa.clip[:, :1]))
    # ... and the same over two processes: each fills its own row of a zero matrix
    sent, accs = [], []

    class Sent(Exception):
        pass

    def record(buf):           # (what this rank sends; the reduction itself follows below)
        sent.append(buf.copy())
        raise Sent
    for rank, h in enumerate(halves):
        a = EvidenceAccumulator(parse_option(True), spec, _host(W // 2, 2, rank, record))
        a.ivs, a.open = [h[0]], h[1]
        with pytest.raises(Sent):
            a.product([], combined=True)
        accs.append(a)
    assert len(sent) == 2 and sent[0].shape == sent[1].shape
    m0, m1 = sent[0].reshape(2, -1), sent[1].reshape(2, -1)
    assert not m0[1].any() and not m1[0].any()
    total = sent[0] + sent[1]

    def summed(buf):
        buf[...] = total
    for a in accs:
        a.host.all_reduce_sum = summed
        assert a.product([], combined=True) == ref
        assert a.product([], combined=False).n_groups == 2


def test_save_and_load_of_the_product(tmp_path):
    G = 2
    ev = Evidence(2, [0.5, 1.0], 128, np.arange(8.0).reshape(2, G, 2) + 1, np.arange(8).reshape(2, G, 2),
                  np.array([[1.0, 1.0], [2.0, 2.5]]), [3, 4], [[0.1, 0.2], [0.3, 0.4]], [[False, True], [False, False]], 7)
    p = str(tmp_path / "e.npz")
    ev.save(p)
    back = Evidence.load(p)
    assert back == ev and back.lnZ == ev.lnZ and back.clamped == 7 and back.clipped().tolist() == [False, True]
    z = np.load(p)
    assert float(z["lnZ"]) == ev.lnZ and np.array_equal(z["lnZ_by_radius"], ev.lnZ_by_radius())
    assert ev.radius == 0.5                           # (radius 1.0 is clipped)


# ------------------------------------------------------------------------------- the window
def test_learned_ellipsoids_switch_at_interval_boundaries_and_the_window_follows_the_moments():
    s = make(max_samples=60000)
    s.run()
    a, log = acc(s), s.engine.ev_log
    assert len(s.progress) >= 5 and s._dropped_snapshots > 0          # intervals were dropped
    assert len(a.ivs) == len(s._intervals)
    assert log[0] == ("ellipsoid", False)                             # attach: active at once
    staged = [k for k, e in enumerate(log) if e == ("ellipsoid", True)]
    assert len(staged) >= 3
    # every filed interval was taken under ONE ellipsoid, and a staged one shows in the interval
    # AFTER the closing request that followed it
    ells = [p["active"] for p in a.ivs]
    assert all(p["n"] == iv[0] for p, iv in zip(a.ivs, s._intervals))
    assert any(not np.array_equal(e0, e1) for e0, e1 in zip(ells, ells[1:]))
    closes = [k for k, e in enumerate(log) if e == ("request", True)]
    k0 = staged[0]
    nxt = next(k for k in closes if k > k0)
    assert any(e[0] == "acc" for e in log[k0:nxt])                    # accumulations between: still the old one
    d = 2
    for p in a.ivs:
        m, Linv, c = p["active"][:d], p["active"][d:d + d * d].reshape(d, d), p["active"][-1]
        assert np.isfinite(c) and Linv[0, 1] == 0.0 and np.all(np.diag(Linv) > 0)
    ev = s.products()["evidence"]
    n_open = s.engine._evr.n
    assert ev.n_acc.tolist() == [iv[0] for iv in s._intervals] + ([n_open] if n_open else [])
    assert ev.n_samples == (sum(iv[0] for iv in s._intervals) + s._snaps_in_interval) * 128
    assert np.isfinite(ev.lnZ_by_radius()).all() and ev.clamped == 0
    # the centre follows the window's pooled mean: the posterior's, not the initial points'
    assert np.allclose(a.centre, [0.2, 0.0], atol=0.15) and not np.array_equal(ells[-1][:d], a.ivs[0]["active"][:d])
    # a second call moves nothing (the open interval is only peeked at)
    assert s.products(combined=True)["evidence"] == ev
    s.close()
    assert a.engine is None and a.product(s._intervals) == ev         # the product outlives the engine


def test_every_third_snapshot_is_accumulated():
    s = make(max_samples=20000, evidence={"every": 3})
    s.run()
    steps = [e[1] for e in s.engine.ev_log if e[0] == "acc"]
    n_snap = s._dropped_snapshots + sum(iv[0] for iv in s._intervals) + s._snaps_in_interval
    assert steps == [40 * k for k in range(3, n_snap + 1, 3)] and len(steps) >= 3
    assert acc(s).phase == n_snap


def test_a_resume_in_mid_interval_ends_bit_identical(tmp_path):
    one = make(str(tmp_path / "a"), 40000)
    one.run()
    p = str(tmp_path / "b")
    b1 = make(p, 20000)
    b1.run()
    z = np.load(p + ".1.state.npz", allow_pickle=False)
    n_iv, G, n_r, n_ell = len(z["iv_n"]), 2, 5, 7
    owned = {"ev_radii": (np.float64, (n_r,)), "ev_book": (np.int64, (2,)), "ev_centre": (np.float64, (2,)),
             "ev_iv_sums": (np.float64, (n_iv, G, n_r)), "ev_iv_counts": (np.uint64, (n_iv, G, n_r)),
             "ev_iv_n": (np.int64, (n_iv, 2)), "ev_iv_ell": (np.float64, (n_iv, n_ell)),
             "ev_open_sums": (np.float64, (G, n_r)), "ev_open_counts": (np.uint64, (G, n_r)),
             "ev_open_n": (np.int64, (2,)), "ev_active": (np.float64, (n_ell,))}
    assert {k for k in z.files if k.startswith("ev_")} == set(owned) | {"ev_staged"}
    for k, (dtype, shape) in owned.items():
        assert (z[k].dtype, z[k].shape) == (np.dtype(dtype), shape), (k, z[k].dtype, z[k].shape)
    assert z["ev_staged"].shape in ((0,), (n_ell,))
    assert int(z["ev_open_n"][0]) > 0 and z["ev_open_sums"].any()     # stopped in mid-interval
    first = Evidence.load(p + ".evidence.npz")
    assert first == b1.products()["evidence"]
    b2 = make(p, 40000, resume=True)
    r = b2.engine._evr
    assert r.n == int(z["ev_open_n"][0]) and np.array_equal(r.acc, z["ev_open_sums"])
    assert np.array_equal(r.active, z["ev_active"])                   # c included: no new maximum is taken
    assert (r.staged is None) == (z["ev_staged"].size == 0)
    b2.run()
    got, ref = b2.products()["evidence"], one.products()["evidence"]
    assert got == ref and got.sums.tobytes() == ref.sums.tobytes() and got.c.tobytes() == ref.c.tobytes()
    assert got.lnZ == ref.lnZ and got.n_samples > first.n_samples
    assert Evidence.load(p + ".evidence.npz") == got
    for other in ({"radii": [1.0]}, {"every": 2}):
        with pytest.raises(LoggedError, match="evidence: cannot resume"):
            make(p, 50000, resume=True, evidence=other)


def test_off_writes_no_key_and_the_output_file_is_cleaned(tmp_path):
    p = str(tmp_path / "c")
    s = make(p, 5000, evidence=None)
    s.run()
    assert s.engine.evidence_layout()["on"] == 0 and "evidence" not in s.products()
    z = np.load(p + ".1.state.npz", allow_pickle=False)
    assert not [k for k in z.files if k.startswith("ev_")] and not os.path.exists(p + ".evidence.npz")
    with pytest.raises(LoggedError, match="evidence: cannot resume -- the run was written without"):
        make(p, 9000, resume=True)
    p = str(tmp_path / "d")
    make(p, 5000).run()
    assert os.path.exists(p + ".evidence.npz")
    OnDouble({"n_walkers": 128, "group_size": 64, "seed": 1}, ProblemSpec.from_info(QUICK), output=p, force=True)
    assert not os.path.exists(p + ".evidence.npz")


def test_the_reference_s_is_the_squared_whitened_distance():
    rng = np.random.default_rng(2)
    d = 7
    A = rng.standard_normal((d, d))
    C = A @ A.T + np.eye(d)
    x, m = rng.standard_normal((50, d)), rng.standard_normal(d)
    want = np.einsum("wi,ij,wj->w", x - m, np.linalg.inv(C), x - m)
    assert np.allclose(rule_s(x, m, rule_linv(C)), want, rtol=1e-11)
    assert rule_c([np.nan, -3.0, -0.5, np.nan]) == -0.5 and rule_c([np.nan]) == 0.0
