"""Evidence sums on the MI355X (evidence_kernels.hip, mcmc_hip_evidence_*): sums, counts and c equal
the rule of DESIGN.md section 2 ("Evidence") -- tests/evidence_ref.py, numpy plus the oracle's dexp
-- bit for bit on crafted states at the smallest shapes at which the kernels can still go wrong
(d below, at and above a block of four rows, a multiple of four and not, one and several rounds of
the four waves, d = 200 with 100 KiB of LDS; one and two 64-walker workgroups per group); the
ellipsoid switches in stream order; shards reproduce the whole; and a run recovers ln Z of a
Gaussian in a box within six standard deviations of the reference rule on exact draws.  Every test
fails without the feature: the entry points and the option do not exist."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402,F401  (before the first Engine: one HIP runtime for both)

from cobaya_amd import run  # noqa: E402
from cobaya_amd.engine import ERR_ARG, ERR_STATE, Engine, EngineError  # noqa: E402
from cobaya_amd.evidence import DEFAULT_RADII, Evidence, log_volume  # noqa: E402
from tests.evidence_ref import Rule, rule_c, rule_linv  # noqa: E402


def _same(got, want):
    """A read-out of the engine against the rule's, bit for bit."""
    assert got["sums"].dtype == np.float64 and got["counts"].dtype == np.uint64
    assert got["sums"].shape == want["sums"].shape
    assert got["sums"].tobytes() == want["sums"].tobytes(), (got["sums"], want["sums"])
    assert np.array_equal(got["counts"], want["counts"])
    assert (got["clamped"], got["n"]) == (want["clamped"], want["n"])
    for k in ("active", "staged"):
        assert (got[k] is None) == (want[k] is None)
    if got["active"] is not None:
        assert got["active"][-1].tobytes() == want["active"][-1].tobytes()       # c


def _engine(d, W, gs, walker_offset=0):
    """An engine that serves d (d > 128: the huge path, which wants incremental evaluation of a
    Gaussian); its state is crafted, nothing is stepped."""
    big = d > 128
    eng = Engine(d, W, group_size=gs, device=0, seed=3, incremental=big, walker_offset=walker_offset)
    eng.set_prior([0] * d, [-50.0] * d, [50.0] * d)
    if big:
        eng.set_target_gaussian_mixture([np.zeros(d)], [np.eye(d)])
    else:
        eng.set_target_one()
    eng.set_proposal_cov(0.01 * np.eye(d))
    return eng


def _state(x, logpost, step=1):
    W = len(logpost)
    z = np.zeros(W, np.int32)
    return {"x": np.ascontiguousarray(x, dtype=np.float64), "logpost": np.asarray(logpost, np.float64),
            "logprior": np.zeros(W), "loglike": np.asarray(logpost, np.float64), "weight": z + 1, "prior_rej": z,
            "burn_left": z, "n_accept": np.zeros(W, np.int64), "step": np.uint64(step)}


def _spd(d, rng):
    A = rng.standard_normal((d, d)) / np.sqrt(d)
    return 0.3 * (A @ A.T) + 0.2 * np.eye(d)


def _crafted(W, d, m, C, rng, step, spread=1.0):
    """Walkers around m with |Linv (x - m)|^2 about spread^2 d: the ladder 0.5 d .. 2 d cuts through
    them; logpost over fifty units."""
    x = m + spread * rng.standard_normal((W, d)) @ np.linalg.cholesky(C).T
    return _state(x, rng.uniform(-60.0, -10.0, W), step)


# ------------------------------------------------------------------------------ bit for bit
@pytest.mark.parametrize("W, gs", [(128, 64), (256, 128)])
@pytest.mark.parametrize("d", [1, 3, 32, 33, 100, 200])
def test_sums_counts_and_c_equal_the_rule_bit_for_bit(W, gs, d):
    rng = np.random.default_rng(1000 * d + W)
    C, m = _spd(d, rng), rng.standard_normal(d)
    r2 = np.array(DEFAULT_RADII) * d
    eng = _engine(d, W, gs)
    assert eng.evidence_layout() == {"on": 0, "n_radii": 0, "n_groups": 0, "n_ell": 0, "active": 0, "staged": 0,
                                     "n_accumulations": 0}
    eng.configure_evidence(r2)
    A, B = _crafted(W, d, m, C, rng, 5), _crafted(W, d, m, C, rng, 9, spread=1.2)
    A["logpost"][[7, W - 1]] = -3.0                   # the maximum, twice
    B["logpost"][0] = 20.0                            # above c in a later accumulation: c - logpost < 0
    eng.set_full_state(A)
    eng.evidence_set_ellipsoid(m, C)
    assert eng.evidence_layout() == {"on": 1, "n_radii": 5, "n_groups": W // gs, "n_ell": d * (d + 1) + 1,
                                     "active": 1, "staged": 0, "n_accumulations": 0}
    eng.accumulate_evidence()
    eng.set_full_state(B)
    eng.accumulate_evidence()
    eng.request_evidence(True)
    got = eng.fetch_evidence()
    Linv = got["active"][d:d + d * d].reshape(d, d)
    assert np.array_equal(got["active"][:d], m) and not np.triu(Linv, 1).any()
    assert np.allclose(Linv, rule_linv(C), rtol=1e-9, atol=1e-12)
    rule = Rule(d, W, gs, r2)
    rule.set_ellipsoid(m, logpost=A["logpost"], Linv=Linv)
    assert rule.active[-1] == -3.0
    rule.accumulate(A["x"], A["logpost"])
    rule.accumulate(B["x"], B["logpost"])
    want = rule.request(True)
    _same(got, want)
    inside = got["counts"].sum(0) / (2.0 * W)
    print("d", d, "inside", inside, "c", got["active"][-1])
    assert got["n"] == 2 and np.all(np.diff(inside) >= 0) and inside[-1] > 0.5 and (d < 3 or inside[0] < 0.5)
    assert np.all(got["sums"][:, -1] > 0)
    eng.close()


# ------------------------------------------------------------------------------ edge cases
def test_the_boundary_is_inside_a_far_walker_is_clamped_and_outside_adds_nothing():
    d, W, gs = 3, 128, 64
    eng = _engine(d, W, gs)
    eng.configure_evidence([25.0])
    x = np.full((W, d), 40.0)                         # everyone else: far outside
    lp = np.full(W, -5.0)
    x[0] = [3.0, 4.0, 0.0]                            # s == 25 exactly: inside
    x[1] = [3.0, np.nextafter(4.0, 5.0), 0.0]         # one ulp further: outside
    x[64] = [0.0, 0.0, 5.0]                           # (the second group) s == 25
    x[65] = [1.0, 1.0, 1.0]
    lp[0], lp[64] = -1.0, -2.5
    lp[65] = -1.0 - 701.0                             # c - logpost = 701 > 700: clamped, and counted
    lp[66] = -1.0 - 700.0                             # == 700: not clamped (and outside)
    lp[2] = -1.0 - 900.0                              # clamped and outside: counted all the same
    st = _state(x, lp)
    eng.set_full_state(st)
    eng.evidence_set_ellipsoid(np.zeros(d), np.eye(d))
    eng.accumulate_evidence()
    eng.request_evidence(True)
    got = eng.fetch_evidence()
    assert np.array_equal(got["active"][d:-1].reshape(d, d), np.eye(d)) and got["active"][-1] == -1.0
    rule = Rule(d, W, gs, [25.0])
    rule.set_ellipsoid(np.zeros(d), logpost=lp, Linv=np.eye(d))
    rule.accumulate(x, lp)
    _same(got, rule.request(True))
    assert got["counts"].tolist() == [[1], [2]] and got["clamped"] == 2
    from oracle import cbind
    assert got["sums"][0, 0] == 1.0                                   # dexp(0)
    assert got["sums"][1, 0] == cbind.dexp(1.5) + cbind.dexp(700.0)   # ascending: walker 64, then 65
    assert math.isclose(cbind.dexp(700.0), math.exp(700.0), rel_tol=1e-15) and got["sums"][1, 0] < np.inf
    # all walkers outside every radius: zeros (and the read-out above emptied the device)
    eng.set_full_state(_state(np.full((W, d), 40.0), lp))
    eng.accumulate_evidence()
    eng.request_evidence(True)
    got = eng.fetch_evidence()
    assert got["n"] == 1 and not got["sums"].any() and not got["counts"].any()
    assert got["clamped"] == 2                        # (this interval's two: the counter was emptied too)
    assert np.array_equal(got["sums"].view(np.uint64), np.zeros((2, 1), np.uint64))      # +0.0
    eng.close()


# ------------------------------------------------------------------------------ the engine
def test_a_staged_ellipsoid_takes_over_inside_the_closing_request_with_a_fresh_c():
    d, W, gs = 5, 128, 64
    rng = np.random.default_rng(8)
    C1, C2, m1, m2 = _spd(d, rng), _spd(d, rng), rng.standard_normal(d), rng.standard_normal(d)
    r2 = np.array([0.5, 1.0, 2.0]) * d
    eng = _engine(d, W, gs)
    for call in (eng.accumulate_evidence, eng.request_evidence, lambda: eng.evidence_set_ellipsoid(m1, C1),
                 lambda: eng.evidence_set(np.zeros((2, 3)), np.zeros((2, 3), np.uint64), 0, 0)):
        with pytest.raises(EngineError) as ei:        # before configure: nothing is allocated or launched
            call()
        assert ei.value.code == ERR_STATE and "evidence_configure must precede" in str(ei.value)
    eng.configure_evidence(r2)
    with pytest.raises(EngineError) as ei:
        eng.accumulate_evidence()
    assert ei.value.code == ERR_STATE and "no ellipsoid is active" in str(ei.value)
    with pytest.raises(EngineError) as ei:
        eng.fetch_evidence()
    assert ei.value.code == ERR_STATE
    S = [_crafted(W, d, m1, C1, rng, 3), _crafted(W, d, m1, C1, rng, 6), _crafted(W, d, m2, C2, rng, 9),
         _crafted(W, d, m2, C2, rng, 12)]
    eng.set_full_state(S[0])
    eng.evidence_set_ellipsoid(m1, C1)
    eng.accumulate_evidence()
    eng.evidence_set_ellipsoid(m2, C2)                # staged: the open interval does not see it
    assert eng.evidence_layout()["staged"] == 1
    eng.set_full_state(S[1])
    eng.accumulate_evidence()
    peek = (eng.request_evidence(False), eng.fetch_evidence())[1]      # disturbs nothing
    assert peek["n"] == 2 and peek["staged"] is not None and np.array_equal(peek["staged"][:d], m2)
    with pytest.raises(EngineError) as ei:
        (eng.request_evidence(True), eng.request_evidence(True))
    assert ei.value.code == ERR_STATE and "pending" in str(ei.value)
    eng.set_full_state(S[2])                          # queued AFTER the closing request: c came from S[1]
    eng.accumulate_evidence()
    first = eng.fetch_evidence()
    assert first["n"] == 2 and first["sums"].tobytes() == peek["sums"].tobytes()
    assert np.array_equal(first["active"], peek["active"]) and np.array_equal(first["active"][:d], m1)
    eng.set_full_state(S[3])
    eng.accumulate_evidence()
    eng.request_evidence(True)
    second = eng.fetch_evidence()
    assert second["staged"] is None and np.array_equal(second["active"][:d], m2)
    assert second["active"][-1] == rule_c(S[1]["logpost"]) != first["active"][-1]
    L1 = first["active"][d:-1].reshape(d, d)
    L2 = second["active"][d:-1].reshape(d, d)
    rule = Rule(d, W, gs, r2)
    rule.set_ellipsoid(m1, logpost=S[0]["logpost"], Linv=L1)
    rule.accumulate(S[0]["x"], S[0]["logpost"])
    rule.set_ellipsoid(m2, Linv=L2)
    rule.accumulate(S[1]["x"], S[1]["logpost"])
    _same(first, rule.request(True, S[1]["logpost"]))
    rule.accumulate(S[2]["x"], S[2]["logpost"])       # from zero, under the new m, Linv and c
    rule.accumulate(S[3]["x"], S[3]["logpost"])
    _same(second, rule.request(True, S[3]["logpost"]))
    eng.request_evidence(True)
    empty = eng.fetch_evidence()
    assert empty["n"] == 0 and not empty["sums"].any() and not empty["counts"].any() and empty["clamped"] == 0
    # a bad argument names itself and leaves everything alone
    with pytest.raises(EngineError, match="positive-definite"):
        eng.evidence_set_ellipsoid(m1, -C1)
    with pytest.raises(EngineError) as ei:
        eng.evidence_set(np.zeros((2, 2)), np.zeros((2, 2), np.uint64), 0, 0, second["active"])
    assert ei.value.code == ERR_ARG and "sums and counts" in str(ei.value)
    for bad in ([], [1.0, 1.0], [-1.0], [2.0, 1.0], list(range(1, 10))):
        if len(bad):
            with pytest.raises(EngineError) as ei:
                eng.configure_evidence(bad)
            assert ei.value.code == ERR_ARG
    assert eng.evidence_layout()["n_radii"] == 3 and eng.evidence_layout()["staged"] == 0
    eng.configure_evidence([])                        # off again: everything is freed
    assert eng.evidence_layout()["on"] == 0
    eng.close()


def test_walker_offset_shards_reproduce_the_groups_of_the_whole():
    d, W, gs = 6, 256, 64
    rng = np.random.default_rng(4)
    C, m = _spd(d, rng), rng.standard_normal(d)
    r2 = np.array(DEFAULT_RADII) * d
    states = [_crafted(W, d, m, C, rng, 2), _crafted(W, d, m, C, rng, 4)]
    states[0]["logpost"][[3, W // 2 + 70]] = -2.0     # the maximum, once in either half: one c
    out = []
    for off, n in ((0, W), (0, W // 2), (W // 2, W // 2)):
        eng = _engine(d, n, gs, walker_offset=off)
        eng.configure_evidence(r2)
        for k, st in enumerate(states):
            part = {key: (v[off:off + n] if key != "step" else v) for key, v in st.items()}
            eng.set_full_state(part)
            if k == 0:
                eng.evidence_set_ellipsoid(m, C)
            eng.accumulate_evidence()
        eng.request_evidence(True)
        out.append(eng.fetch_evidence())
        eng.close()
    whole, a, b = out
    assert whole["active"][-1] == a["active"][-1] == b["active"][-1] == -2.0
    assert np.vstack((a["sums"], b["sums"])).tobytes() == whole["sums"].tobytes() and whole["sums"].all()
    assert np.array_equal(np.vstack((a["counts"], b["counts"])), whole["counts"])


def test_a_resume_in_mid_interval_is_bit_identical():
    d, W, gs = 4, 128, 64
    rng = np.random.default_rng(6)
    C, C2, m = _spd(d, rng), _spd(d, rng), rng.standard_normal(d)
    r2 = np.array([1.0, 2.0]) * d
    S = [_crafted(W, d, m, C, rng, k) for k in (1, 2, 3, 4)]

    def tail(eng):
        """What both runs do after the resume point."""
        eng.set_full_state(S[2])
        eng.accumulate_evidence()
        eng.request_evidence(True)                    # the staged ellipsoid takes over here
        one = eng.fetch_evidence()
        eng.set_full_state(S[3])
        eng.accumulate_evidence()
        eng.request_evidence(True)
        return one, eng.fetch_evidence()

    eng = _engine(d, W, gs)
    eng.configure_evidence(r2)
    eng.set_full_state(S[0])
    eng.evidence_set_ellipsoid(m, C)
    eng.accumulate_evidence()
    eng.set_full_state(S[1])
    eng.accumulate_evidence()
    eng.evidence_set_ellipsoid(m + 0.1, C2)
    eng.request_evidence(False)
    saved = eng.fetch_evidence()
    ref = tail(eng)
    eng.close()
    eng = _engine(d, W, gs)
    eng.configure_evidence(r2)
    eng.evidence_set(saved["sums"], saved["counts"], saved["clamped"], saved["n"], saved["active"], saved["staged"])
    assert eng.evidence_layout() == {"on": 1, "n_radii": 2, "n_groups": 2, "n_ell": d * (d + 1) + 1, "active": 1,
                                     "staged": 1, "n_accumulations": 2}
    got = tail(eng)
    eng.close()
    for g, r in zip(got, ref):
        _same(g, r)
        assert np.array_equal(g["active"], r["active"])
    assert got[0]["n"] == 3 and got[1]["n"] == 1 and not np.array_equal(got[0]["active"], got[1]["active"])


# ------------------------------------------------------------------------------ end to end
def _box_info(d, W, seed, **opts):
    """One Gaussian mode in the box [0, 2]^d, its walls at least eight sigma away."""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((d, d)) / np.sqrt(d)
    cov = 0.004 * (0.5 * A @ A.T + 0.5 * np.eye(d))
    mean = 1.0 + 0.05 * rng.standard_normal(d)
    sig = np.sqrt(np.diag(cov))
    assert np.all(mean - 8 * sig > 0.0) and np.all(mean + 8 * sig < 2.0)
    names = [f"a__{i}" for i in range(d)]
    info = {"likelihood": {"gaussian_mixture": {"means": [mean], "covs": [cov], "input_params_prefix": "a_"}},
            "params": {n: {"prior": {"min": 0.0, "max": 2.0},
                           "ref": {"dist": "norm", "loc": float(mean[i]), "scale": float(sig[i])},
                           "proposal": float(sig[i])} for i, n in enumerate(names)},
            "sampler": {"mcmc_hip": {"seed": seed, "n_walkers": W, "evidence": True, **opts}}}
    return info, mean, cov


def _sigma_ref(d, W, cov, reps=32, seed=99):
    """The standard deviation of the REFERENCE RULE's ln Z over `reps` replications of ONE snapshot of
    W exact Gaussian draws, the ellipsoid of each taken from an independent draw."""
    rng = np.random.default_rng(seed)
    Lc = np.linalg.cholesky(cov)
    logdet = np.log(np.diag(Lc)).sum()
    r2 = np.array(DEFAULT_RADII) * d
    out = []
    for _ in range(reps):
        z0, z = rng.standard_normal((W, d)), rng.standard_normal((W, d))
        x0, x = z0 @ Lc.T, z @ Lc.T
        lp = -0.5 * np.sum(z * z, axis=1) - 0.5 * d * math.log(2 * math.pi) - logdet
        rule = Rule(d, W, 64, r2)
        rule.set_ellipsoid(x0.mean(0), np.cov(x0.T), lp)
        rule.accumulate(x, lp)
        p = rule.request(True)
        ev = Evidence(d, DEFAULT_RADII, W, [p["sums"]], [p["counts"]], np.full((1, W // 64), p["active"][-1]), [1],
                      [log_volume(p["active"], d, r2)], np.zeros((1, len(r2)), bool))
        out.append(ev.lnZ)                            # (the truth is 0: the density is normalised)
    return float(np.std(out, ddof=1)), float(np.mean(out))


@pytest.mark.parametrize("d", [2, 30])
def test_ln_z_of_a_gaussian_in_a_box_against_the_true_value(d, tmp_path):
    """Run to the default stop; |lnZ - ln Z_true| <= 6 sigma_ref with ln Z_true = -ln V_box, sigma_ref
    from the reference rule on exact draws (an upper bound for a run with many snapshots)."""
    W = 4096
    prefix = str(tmp_path / "e")
    info, mean, cov = _box_info(d, W, 17 + d)
    info["output"] = prefix
    _, s = run(info)
    assert s.converged
    ev = s.products()["evidence"]
    sigma_ref, mean_ref = _sigma_ref(d, W, cov)
    true = -d * math.log(2.0)
    print("d", d, "lnZ", ev.lnZ, "true", true, "diff", ev.lnZ - true, "stderr", ev.stderr, "sigma_ref", sigma_ref,
          "mean_ref", mean_ref, "by radius", ev.lnZ_by_radius() - true, "stderr by radius", ev.stderr_by_radius(),
          "inside", ev.inside_fraction(), "n_acc", ev.n_acc.tolist(), "radius", ev.radius)
    assert abs(ev.lnZ - true) <= 6 * sigma_ref
    assert sigma_ref / 20 <= ev.stderr <= 3 * sigma_ref
    assert not ev.clipped().any() and ev.clamped == 0 and ev.radii == list(DEFAULT_RADII)
    assert ev.n_samples == (sum(iv[0] for iv in s._intervals) + s._snaps_in_interval) * W > 0
    assert Evidence.load(prefix + ".evidence.npz") == ev
    s.close()


def test_every_third_snapshot_and_the_option_off():
    info, _, _ = _box_info(2, 256, 5, Rminus1_stop=0.0, max_samples=256 * 200, steps_per_launch=20,
                           moments_every=1)
    info["sampler"]["mcmc_hip"]["evidence"] = {"every": 3}
    _, s = run(info)
    n_snap = s._dropped_snapshots + sum(iv[0] for iv in s._intervals) + s._snaps_in_interval
    a = next(p for p in s._products if p.name == "evidence")
    total = sum(p["n"] for p in a.ivs) + s.engine.evidence_layout()["n_accumulations"]
    kept = sum(iv[0] for iv in s._intervals) + s._snaps_in_interval
    assert a.phase == n_snap >= 9 and kept // 3 - 1 <= total <= kept // 3 + 1
    ev = s.products()["evidence"]
    assert ev.n_acc.sum() == total and np.isfinite(ev.lnZ)
    s.close()
    info["sampler"]["mcmc_hip"]["evidence"] = None
    _, s = run(info)
    assert "evidence" not in s.products()
    assert s.engine.evidence_layout() == {"on": 0, "n_radii": 0, "n_groups": 0, "n_ell": 0, "active": 0,
                                          "staged": 0, "n_accumulations": 0}
    s.close()


def test_the_banana_as_a_device_function():
    """A function target emits no rows; its normalisation is its own, so only: finite, nothing clamped."""
    def banana(p):
        return -0.5 * (p[:, 0] ** 2 + ((p[:, 1] - 0.5 * p[:, 0] ** 2) / 0.5) ** 2)

    info = {"likelihood": {"banana": {"class": "device_function", "function": banana}},
            "params": {"a": {"prior": {"min": -8, "max": 8}, "ref": 0, "proposal": 1},
                       "b": {"prior": {"min": -6, "max": 30}, "ref": 0.5, "proposal": 1}},
            "sampler": {"mcmc_hip": {"n_walkers": 2048, "seed": 3, "group_size": 64, "max_tries": "2000d",
                                     "max_samples": 2048 * 300, "Rminus1_stop": 0.0, "evidence": True}}}
    _, s = run(info)
    assert s.engine.last_step_kernel().startswith("mcmc::fn_walker_kernel")
    ev = s.products()["evidence"]
    print("banana lnZ", ev.lnZ, "+-", ev.stderr, "by radius", ev.lnZ_by_radius(), "clipped", ev.clipped())
    assert np.isfinite(ev.lnZ) and ev.clamped == 0 and ev.n_samples > 0
    s.close()
