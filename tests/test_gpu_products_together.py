"""The six device products switched on TOGETHER, on the MI355X: all six slabs on one engine, fed by the step
kernels' states, every read-out against its own numpy rule over the states read back -- whatever the order in
which the slabs were configured and accumulated, with one of them configured off and on again beside the
others, and on two walker-offset shards; then `run` with everything on along four step paths, every interval
of every product replayed from the stored rows through the rules, the chain that of the run without products
and each product that of the run with its option alone; and a resume with everything on.  No CPU double
appears here: the references are the rules of DESIGN.md section 2 (tests/*_ref.py, `rule_slab`), fed with
what the device holds.  Every comparison is of bits but the two documented ones of (b)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402,F401  (before the first Engine: one HIP runtime for both)

from cobaya_amd import run  # noqa: E402
from cobaya_amd.bestfit import merge_records  # noqa: E402
from cobaya_amd.engine import Engine  # noqa: E402
from cobaya_amd.model import ProblemSpec  # noqa: E402
from cobaya_amd.sampler import MCMCHip  # noqa: E402
from tests import autocorr_ref, bestfit_ref, derived_ref, evidence_ref, importance_ref  # noqa: E402
from tests.products_together import (DERIVED_FUNCTIONS, IMPORTANCE_FUNCTIONS, PRODUCTS, all_options,  # noqa: E402
                                     derived_params, fn, only, same_as_replayed, same_bits, same_product)
from tests.test_marginals_host import rule_slab  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F_S, F_T = fn(DERIVED_FUNCTIONS["s"]), fn(DERIVED_FUNCTIONS["t"])                # (numpy and torch alike)
F_BAO, F_TILT = fn(IMPORTANCE_FUNCTIONS["bao"]), fn(IMPORTANCE_FUNCTIONS["tilt"])


# =============================================================================== (a) all six slabs on one engine
STEPS = (7, 5, 11, 3, 9)            # steps before each of the five accumulations
CLOSE_AFTER = 2                     # ... all six are closed behind the third
STAGE_AFTER = 1                     # ... a second ellipsoid is staged behind the second
DV_SHIFT = np.array([0.125, -0.25])
CONFIGURE_B = ("importance", "evidence", "bestfit", "autocorr", "derived", "marginals")
REVERSED = ("derived",) + PRODUCTS[:0:-1]       # (`derived` stays first: `marginals` reads its rows)


def _target(d):
    rng = np.random.default_rng(100 + d)
    A = rng.standard_normal((d, d)) / np.sqrt(d)
    return 0.1 * rng.standard_normal(d), 0.3 * (A @ A.T) + 0.2 * np.eye(d)


def _x0(d, W):
    mean, cov = _target(d)
    return mean + np.random.default_rng(7 * d + W).standard_normal((W, d)) @ np.linalg.cholesky(cov).T


class _Six:
    """One engine with the six slabs; `cov`: the importance alternatives; `leave_out`: products that stay off."""

    def __init__(self, d, W, gs, incremental, x0, offset=0, cov=(True, False), configure=PRODUCTS, leave_out=()):
        self.d, self.W, self.gs, self.cov = d, W, gs, list(cov)
        self.on = [p for p in PRODUCTS if p not in leave_out]
        mean, c = _target(d)
        self.ell = [(mean, c), (mean + 0.05, 1.5 * c)]
        self.shift = mean + 0.01
        eng = self.eng = Engine(d, W, group_size=gs, device=0, seed=5, incremental=incremental, walker_offset=offset)
        eng.set_prior([0] * d, [-50.0] * d, [50.0] * d)
        eng.set_target_gaussian_mixture([mean], [c])
        eng.set_proposal_cov(c)
        eng.set_state(x0)
        eng.set_moment_shift(self.shift)
        self.lo = np.array([-1.5] * d + [-2.5, -2.5])
        self.hi = np.array([1.5] * d + [2.5, 2.5])
        for name in configure:
            if name in self.on:
                self.configure(name)

    # -- one product
    def configure(self, name):
        eng, d = self.eng, self.d
        if name == "derived":
            eng.configure_derived(2, [1, 0], DV_SHIFT)
        elif name == "marginals":
            eng.configure_marginals(self.dims1(), 16, [(1, 0)], 8, self.lo, self.hi)
        elif name == "autocorr":
            eng.configure_autocorr([1, 0], 3)
        elif name == "bestfit":
            eng.configure_bestfit(list(range(d)), 16, self.lo[:d], self.hi[:d])
        elif name == "evidence":
            eng.configure_evidence([1.0 * d, 2.0 * d])
            eng.evidence_set_ellipsoid(*self.ell[0])
        elif name == "importance":
            eng.configure_importance(self.cov)

    def dims1(self):
        return [0, self.d - 1, self.d]           # (index d: the first derived row)

    def off(self, name):
        getattr(self.eng, "configure_" + name)()

    def fill(self, name):
        """The derived rows / the log-weights from the state as it lies on the device, on the engine's stream,
        as the accumulators do."""
        eng = self.eng
        if name == "derived":
            x, z, stream = eng.derived_row_views()
            with torch.cuda.stream(stream):
                z[0].copy_(F_S(x[0], x[1]))
                z[1].copy_(F_T(x[0], z[0]))
        elif name == "importance":
            x, delta, stream = eng.importance_row_views()
            with torch.cuda.stream(stream):
                delta[0].copy_(F_BAO(x[0]))
                delta[1].copy_(F_TILT(x[0], x[1]))
            return delta

    def accumulate(self, name):
        delta = self.fill(name)
        if name == "importance":
            self.eng.accumulate_importance(delta)
        else:
            getattr(self.eng, "accumulate_" + name)()

    def request(self, name, close=True):
        f = getattr(self.eng, "request_" + name)
        f(close) if name in ("evidence", "importance") else f()

    def fetch(self, name):
        return getattr(self.eng, "fetch_" + name)()

    # -- the sequence of the issue
    def drive(self, order=PRODUCTS, toggle=None):
        """step, sync, read the state back, accumulate all six -- five times; all six closed behind the third
        accumulation, back to back, and fetched in the reverse order; at the end the open interval.  `toggle`:
        that product is configured off and on again between the fourth and the fifth accumulation."""
        eng, on = self.eng, self.on
        out = {"states": [eng.get_full_state()], "closed": {}, "open": {}}
        if "evidence" in on:
            self.request("evidence", False)
            out["ellipsoid"] = self.fetch("evidence")
        for k, n in enumerate(STEPS):
            eng.step(n)
            eng.sync()
            out["states"].append(eng.get_full_state())
            for name in order:
                if name in on:
                    self.accumulate(name)
            if k == STAGE_AFTER and "evidence" in on:
                eng.evidence_set_ellipsoid(*self.ell[1])
            if k == CLOSE_AFTER:
                for name in order:
                    if name in on:
                        self.request(name)
                for name in reversed(order):
                    if name in on:
                        out["closed"][name] = self.fetch(name)
            if k == CLOSE_AFTER + 1 and toggle:
                self.off(toggle)
                self.configure(toggle)
        for name in on:
            self.request(name, False)
            out["open"][name] = self.fetch(name)
        out["kernel"] = eng.last_step_kernel()
        eng.close()
        return out

    # -- the rules over the states read back
    def rules(self, out, offset=0):
        """{"closed", "open"}: what the six rules give for the states of `out` (evidence: with the inverse
        Cholesky factors the engine reports, which differ from numpy's in the last bits)."""
        d, W, gs, on = self.d, self.W, self.gs, self.on
        st0, states = out["states"][0], out["states"][1:]
        z = [np.column_stack((F_S(s["x"][:, 0], s["x"][:, 1]), F_T(s["x"][:, 0], F_S(s["x"][:, 0], s["x"][:, 1]))))
             for s in states]
        first, second = range(CLOSE_AFTER + 1), range(CLOSE_AFTER + 1, len(STEPS))
        want = {"closed": {}, "open": {}}
        if "derived" in on:
            r = derived_ref.Rule(W, gs, 2, [1, 0], DV_SHIFT, self.shift)
            for part, span in (("closed", first), ("open", second)):
                for k in span:
                    r.accumulate(states[k]["x"], z[k])
                want[part]["derived"] = r.request()
        if "marginals" in on:
            for part, span in (("closed", first), ("open", second)):
                slab = sum(rule_slab(np.column_stack((states[k]["x"], z[k])), self.dims1(), 16, [(1, 0)], 8,
                                     self.lo, self.hi) for k in span)
                want[part]["marginals"] = (slab, len(span))
        if "autocorr" in on:
            r = autocorr_ref.Rule([1, 0], 3, gs, self.shift)
            for part, span in (("closed", first), ("open", second)):
                for k in span:
                    r.accumulate(states[k]["x"])
                want[part]["autocorr"] = r.read_and_zero()
        if "bestfit" in on:
            r = bestfit_ref.Rule(d, list(range(d)), 16, self.lo[:d], self.hi[:d], "loglike", walker_offset=offset)
            for part, span in (("closed", first), ("open", second)):
                for k in span:
                    r.accumulate(states[k])
                want[part]["bestfit"] = r.read_and_empty()
        if "evidence" in on:
            keys = ("sums", "counts", "clamped", "n", "active")
            e0, staged = out["ellipsoid"], out["closed"]["evidence"]["staged"]
            r = evidence_ref.Rule(d, W, gs, [1.0 * d, 2.0 * d])
            r.set_ellipsoid(self.ell[0][0], logpost=st0["logpost"], Linv=e0["active"][d:-1].reshape(d, d))
            same_bits(e0["active"], r.active, ("evidence", "the first ellipsoid and its c"))
            assert staged is not None and np.array_equal(staged[:d], self.ell[1][0])
            for k in first:
                r.accumulate(states[k]["x"], states[k]["logpost"])
                if k == STAGE_AFTER:
                    r.set_ellipsoid(self.ell[1][0], Linv=staged[d:-1].reshape(d, d))
            w = r.request(True, states[CLOSE_AFTER]["logpost"])      # (activates the staged one, with a new c)
            want["closed"]["evidence"] = {k: w[k] for k in keys}
            for k in second:
                r.accumulate(states[k]["x"], states[k]["logpost"])
            w = r.request(False)
            want["open"]["evidence"] = {k: w[k] for k in keys}
            assert w["staged"] is None and out["open"]["evidence"]["staged"] is None
        if "importance" in on:
            r = importance_ref.Rule(d, W, gs, self.cov)
            for part, span in (("closed", first), ("open", second)):
                for k in span:
                    x = states[k]["x"]
                    r.accumulate(x, np.stack((F_BAO(x[:, 0]), F_TILT(x[:, 0], x[:, 1]))), self.shift)
                want[part]["importance"] = r.request(True)
        return want


def _same_readouts(got, want, names):
    for part in ("closed", "open"):
        for name in names:
            same_bits(got[part][name], want[part][name], (part, name))


SHAPES = {  # d, W, group_size, incremental evaluation, the kernel's name holds
    "d2-scratch": (2, 128, 64, False, "::step_kernel<"),
    "d30-incremental": (30, 512, 128, True, "step_inc_kernel"),
    "d33-scratch": (33, 256, 64, False, "step_pair_kernel"),
    "d130-huge": (130, 128, 64, True, "huge_step_kernel"),
}


@pytest.mark.parametrize("shape", list(SHAPES))
def test_six_slabs_on_one_engine_each_equal_their_rule_over_the_states_read_back(shape):
    d, W, gs, inc, family = SHAPES[shape]
    cov = (True, False) if d <= 128 else (False, False)
    six = _Six(d, W, gs, inc, _x0(d, W), cov=cov)
    got = six.drive()
    print(shape, got["kernel"])
    assert family in got["kernel"] and ("inc" in got["kernel"] or "huge" in got["kernel"]) == inc, got["kernel"]
    assert six.on == list(PRODUCTS)         # (nothing is refused at d = 130: every product serves d <= 256)
    want = six.rules(got)
    _same_readouts(got, want, PRODUCTS)
    # ... of states that moved, sums that are alive and an ellipsoid that changed at the closing request
    assert not np.array_equal(got["states"][1]["x"], got["states"][2]["x"])
    assert got["closed"]["importance"]["n_acc"] == 3 and got["open"]["importance"]["n_acc"] == 2
    assert got["closed"]["derived"]["N"] == 3 * W and got["open"]["marginals"][1] == 2
    assert got["closed"]["bestfit"][1][:, 0].all() and got["closed"]["autocorr"][1].tolist() == [3, 2, 1, 0]
    assert got["open"]["autocorr"][1].tolist() == [2, 2, 2, 2]         # (the ring outlives the closing request)
    ev = got["closed"]["evidence"], got["open"]["evidence"]
    assert ev[0]["counts"].sum() > 0 and ev[1]["counts"].sum() > 0 and ev[0]["n"] == 3
    assert not np.array_equal(ev[0]["active"], ev[1]["active"]) and np.array_equal(ev[1]["active"][:d], six.ell[1][0])


@pytest.mark.parametrize("shape", ["d2-scratch", "d30-incremental"])
def test_the_bits_depend_neither_on_the_order_of_configuration_nor_on_that_of_accumulation(shape):
    d, W, gs, inc, _ = SHAPES[shape]
    x0 = _x0(d, W)
    base = _Six(d, W, gs, inc, x0).drive()
    for configure, order in ((PRODUCTS, REVERSED), (CONFIGURE_B, PRODUCTS), (CONFIGURE_B, REVERSED)):
        other = _Six(d, W, gs, inc, x0, configure=configure).drive(order)
        same_bits(other["states"], base["states"], ("states",))
        _same_readouts(other, base, PRODUCTS)


@pytest.mark.parametrize("shape", ["d2-scratch", "d30-incremental"])
def test_a_product_configured_off_and_on_again_leaves_the_others_open_intervals_untouched(shape):
    d, W, gs, inc, _ = SHAPES[shape]
    x0 = _x0(d, W)
    base = _Six(d, W, gs, inc, x0).drive()
    for toggled in PRODUCTS[1:]:            # (`derived` cannot go while `marginals` reads its rows)
        other = _Six(d, W, gs, inc, x0).drive(toggle=toggled)
        _same_readouts(other, base, [p for p in PRODUCTS if p != toggled])
        # ... and its own new slab holds the one accumulation that followed, and nothing older
        mine = other["open"][toggled]
        assert _n_open(mine, toggled) == 1 and _n_open(base["open"][toggled], toggled) == 2, toggled
        if toggled == "autocorr":           # (its ring began anew as well: lag 0 alone)
            assert mine[1].tolist() == [1, 0, 0, 0]


def _n_open(part, name):
    return {"marginals": lambda p: p[1], "autocorr": lambda p: int(p[1][0]), "bestfit": lambda p: p[2],
            "evidence": lambda p: p["n"], "importance": lambda p: p["n_acc"]}[name](part)


# =============================================================================== (b) two walker-offset shards
@pytest.mark.parametrize("shape", ["d2-scratch", "d30-incremental"])
def test_two_walker_offset_shards_with_everything_on(shape):
    """Each shard's six read-outs equal the rules over ITS walkers (global walker ids in the records); its
    states are the whole ensemble's.  Merged: counts, keys and records are those of the whole exactly.  The
    float sums of a shard are the same groups only where the centring constant is the same (evidence and
    importance take c from the shard's own walkers: tests/test_gpu_evidence.py, tests/test_gpu_importance.py);
    `autocorr` pools its groups in another order, within the bound of tests/test_gpu_autocorr.py."""
    d, W, gs, inc, _ = SHAPES[shape]
    x0, h = _x0(d, W), W // 2
    whole_six = _Six(d, W, gs, inc, x0)
    whole = whole_six.drive()
    halves = []
    for off in (0, h):
        six = _Six(d, h, gs, inc, x0[off:off + h], offset=off)
        got = six.drive()
        _same_readouts(got, six.rules(got, offset=off), PRODUCTS)
        halves.append(got)
    a, b = halves
    for k in range(len(STEPS) + 1):
        for key in ("x", "logpost", "loglike"):
            assert np.array_equal(np.concatenate((a["states"][k][key], b["states"][k][key])), whole["states"][k][key])
    G = W // gs
    for part in ("closed", "open"):
        w, p, q = whole[part], a[part], b[part]
        assert np.array_equal(p["marginals"][0] + q["marginals"][0], w["marginals"][0])
        assert np.array_equal(np.maximum(p["bestfit"][0], q["bestfit"][0]), w["bestfit"][0])
        assert np.array_equal(merge_records(p["bestfit"][1], q["bestfit"][1]), w["bestfit"][1])
        assert np.array_equal(merge_records(q["bestfit"][1], p["bestfit"][1]), w["bestfit"][1])
        assert np.array_equal(np.concatenate((p["evidence"]["counts"], q["evidence"]["counts"])), w["evidence"]["counts"])
        assert np.array_equal(np.concatenate((p["importance"]["n"], q["importance"]["n"]), axis=1), w["importance"]["n"])
        assert p["derived"]["N"] + q["derived"]["N"] == w["derived"]["N"]
        assert np.array_equal(np.fmin(p["derived"]["min"], q["derived"]["min"]), w["derived"]["min"])
        assert np.array_equal(np.fmax(p["derived"]["max"], q["derived"]["max"]), w["derived"]["max"])
        assert np.array_equal(p["autocorr"][1], w["autocorr"][1]) and np.array_equal(q["autocorr"][1], w["autocorr"][1])
    # autocorr: two orders of one sum of G terms per accumulation differ by at most G 2^-52 sum |term|
    r = autocorr_ref.Rule([1, 0], 3, gs, whole_six.shift)
    for k in range(CLOSE_AFTER + 1):
        r.accumulate(whole["states"][k + 1]["x"])
    err = np.abs(a["closed"]["autocorr"][0] + b["closed"]["autocorr"][0] - whole["closed"]["autocorr"][0])
    bound = G * 2.0 ** -52 * r.abs_sums
    print(shape, "autocorr: largest error / bound", np.max(err[bound > 0] / bound[bound > 0]))
    assert np.all(err <= bound)
    # where a shard's c IS the whole's, its groups are the whole's groups bit for bit
    for part in ("closed", "open"):
        for k, sh in enumerate((a, b)):
            ev, wv = sh[part]["evidence"], whole[part]["evidence"]
            if ev["active"][-1] == wv["active"][-1]:
                same_bits(ev["sums"], wv["sums"][k * (G // 2):(k + 1) * (G // 2)], (part, "evidence", k))
    assert any(sh["closed"]["evidence"]["active"][-1] == whole["closed"]["evidence"]["active"][-1] for sh in (a, b))


# =============================================================================== (c) `run` with everything on
def _banana(pts):
    return -0.5 * (pts[:, 0] ** 2 + ((pts[:, 1] - 0.5 * pts[:, 0] ** 2) / 0.5) ** 2)


def _model(path):
    """(likelihood, params without the derived ones, sampler options of the path, max_samples)."""
    if path == "mixture-d30":
        g = np.load(os.path.join(GOLDEN, "targets.npz"))
        mean, cov = g["mean_d30"], g["cov_d30"]
        sig = np.sqrt(np.diag(cov))
        like = {"gaussian_mixture": {"means": [mean.tolist(), (mean + 0.5 * sig).tolist()],
                                     "covs": [cov.tolist(), cov.tolist()]}}
        params = {"p%d" % i: {"prior": {"min": 0.0, "max": 1.0}, "ref": {"dist": "norm", "loc": float(mean[i]), "scale": float(sig[i])}}
                  for i in range(30)}
        return like, params, {}, 1300000
    params = {"a": {"prior": {"min": -6, "max": 6}, "ref": {"dist": "norm", "loc": 0.3, "scale": 0.5}},
              "b": {"prior": {"min": -6, "max": 6}, "ref": {"dist": "norm", "loc": -0.2, "scale": 0.5}}}
    if path == "device_function":
        return {"banana": {"class": "device_function", "function": _banana}}, params, {"max_tries": "2000d"}, 200000
    like = {"gaussian": {"mean": [0.3, -0.2], "cov": [[0.5, 0.2], [0.2, 0.4]]}}
    return like, params, ({"evaluation": "full"} if path == "full" else {}), 200000


def _info(path, which="all", **opts):
    """`which`: "all", "none" or one product's name (`derived`: the functions in `params` alone)."""
    like, params, extra, max_samples = _model(path)
    names = list(params)
    o = {"n_walkers": 512, "group_size": 64, "seed": 7, "Rminus1_stop": 0.0, "max_samples": max_samples,
         "steps_per_launch": 40, "moments_every": 1, "snapshot_every": 40, "max_rows": 1 << 22, "learn_every": "20d"}
    o.update(extra)
    every = all_options(names)
    if which not in ("all", "none", "derived"):
        every = only(every, which)
    if which in ("all", "derived", "marginals"):        # (the histogram of `s` needs its rows)
        params = dict(params, **derived_params(names))
    if which == "marginals":
        o["derived_stats"] = False
    if which in ("none", "derived"):
        every = {k: None for k in every}
    o.update(every)
    o.update(opts)
    return {"likelihood": like, "params": params, "sampler": {"mcmc_hip": o}}


FAMILY = {"incremental": ("step_inc_kernel", True), "full": ("::step_kernel<", False),
          "mixture-d30": ("mix_kernel", True), "device_function": ("fn_walker_kernel", False)}


def _chain(smp, d):
    """What of a run does not depend on its products, as bytes: the stored rows without the derived columns,
    the final state, the proposal covariance, the progress columns and the step kernel."""
    st = smp.engine.get_state()
    rows = np.vstack(smp._rows)[:, :5 + d]
    return {"rows": np.ascontiguousarray(rows).tobytes(), "x": st["x"].tobytes(), "logpost": st["logpost"].tobytes(),
            "proposal": smp.engine.get_proposal_cov().tobytes(), "steps": smp.n_steps_raw,
            "progress": smp.progress[["N", "acceptance_rate", "Rminus1"]].to_numpy(dtype=np.float64).tobytes(),
            "kernel": smp.engine.last_step_kernel()}


@pytest.mark.parametrize("path", list(FAMILY))
def test_a_run_with_everything_on_replays_through_the_rules_and_leaves_the_chain_alone(path):
    _, smp = run(_info(path))
    d, kernel = smp.spec.d, smp.engine.last_step_kernel()
    print(path, kernel, "launches", smp._launches, "intervals", smp._iv0 + len(smp._intervals), "in the window",
          len(smp._intervals), "open", smp._snaps_in_interval)
    assert FAMILY[path][0] in kernel and bool(smp.incremental) == FAMILY[path][1], kernel
    assert [p.name for p in smp._products] == list(PRODUCTS)
    assert len(smp._intervals) >= 2 and smp._iv0 + len(smp._intervals) >= 3 and smp._dropped_snapshots > 0
    # every interval of every product: the rules over the stored rows
    assert same_as_replayed(smp) == {name: len(smp._intervals) + 1 for name in PRODUCTS}
    prod = smp.products()
    n = sum(iv[0] for iv in smp._intervals) + smp._snaps_in_interval
    assert prod["derived"].n_used == prod["derived"].n_samples == n * 512 == prod["importance"].n_samples
    assert prod["marginals"].n_accumulations == n and int(prod["marginals"].counts("s").sum()) > 0
    # the chain is that of the run without any product
    want = _chain(smp, d)
    _, bare = run(_info(path, "none"))
    assert not bare._products
    have = _chain(bare, d)
    assert have == want, [k for k in want if have[k] != want[k]]
    bare.close()
    if path == "incremental":               # ... and each product that of the run with its option alone
        for name in PRODUCTS:
            _, alone = run(_info(path, name))
            assert [p.name for p in alone._products if p.live] == [name], name
            same_product(name, alone.products()[name], prod[name])
            assert _chain(alone, d) == want, name
            alone.close()
    smp.close()
    after = smp.products()
    for name in PRODUCTS:
        same_product(name, after[name], prod[name])


# =============================================================================== (d) resume with everything on
def test_a_resume_in_mid_interval_with_everything_on_is_bit_identical(tmp_path):
    """Two legs against one run, ending at the same checkpoint (a run ends at the first checkpoint that sees
    max_samples).  `autocorr` does not restore its ring: its reference is the two-leg run with `autocorr`
    alone (tests/test_gpu_autocorr.py pins what the missing pairs are)."""
    def make(prefix, resume, max_samples, which="all"):
        info = _info("incremental", which, seed=21, max_samples=max_samples)
        return MCMCHip(info["sampler"]["mcmc_hip"], ProblemSpec.from_info(info), output=prefix, resume=resume)

    a = make(str(tmp_path / "a"), False, 150000)
    a.run()
    pa = a.products()
    a.close()
    b1 = make(str(tmp_path / "b"), False, 30000)
    b1.run()
    assert b1.n_steps_raw < a.n_steps_raw
    z = np.load(str(tmp_path / "b.1.state.npz"), allow_pickle=False)
    b1.close()
    b2 = make(str(tmp_path / "b"), True, 150000)
    # the open interval of every product is on the device again, with the bytes of the state file
    assert int(z["marg_open_n"]) > 0 and int(z["iw_open_nacc"][0]) > 0 and z["iw_open_sums"].any()
    eng = b2.engine
    eng.request_importance(False)
    back = eng.fetch_importance()
    assert back["sums"].tobytes() == z["iw_open_sums"][0].tobytes() and np.array_equal(back["c"], z["iw_open_c"][0])
    assert back["n_acc"] == int(z["iw_open_nacc"][0])
    eng.request_evidence(False)
    back = eng.fetch_evidence()
    assert back["sums"].tobytes() == z["ev_open_sums"].tobytes() and np.array_equal(back["counts"], z["ev_open_counts"])
    assert back["active"].tobytes() == z["ev_active"].tobytes() and back["n"] == int(z["ev_open_n"][0])
    accs = {p.name: p for p in b2._products}
    s_, n_ = accs["autocorr"]._peek(False)
    assert s_.tobytes() == z["ac_open"].tobytes() and np.array_equal(n_, z["ac_open_pairs"])
    dv = accs["derived"]._peek(False)
    for k in ("A", "B", "C", "X", "V", "bad"):
        assert np.asarray(dv[k]).tobytes() == z["dv_open_" + k][0].tobytes(), k
    assert [dv["N"], dv["n"]] == z["dv_open_N"][0].tolist() and dv["n"] > 0
    # (the exact ones are split: what the device holds of them is read out and set back)
    eng.request_marginals()
    counts, n_mg = eng.fetch_marginals()
    assert np.array_equal(counts, z["marg_open"]) and n_mg == int(z["marg_open_n"])
    eng.marginals_set(counts, n_mg)
    eng.request_bestfit()
    slab, rec, n_bf = eng.fetch_bestfit()
    assert np.array_equal(slab, z["bf_open_slab"]) and np.array_equal(rec, z["bf_open_rec"]) and n_bf == int(z["bf_open_n"])
    eng.bestfit_set(slab, rec, n_bf)
    b2.run()
    assert b2.n_steps_raw == a.n_steps_raw
    pb = b2.products()
    for name in PRODUCTS:
        if name != "autocorr":
            same_product(name, pb[name], pa[name])
    c1 = make(str(tmp_path / "c"), False, 30000, "autocorr")
    c1.run()
    c1.close()
    c2 = make(str(tmp_path / "c"), True, 150000, "autocorr")
    c2.run()
    same_product("autocorr", pb["autocorr"], c2.products()["autocorr"])
    # (the pairs that bridge the resume point are missing where it lies in the window at the end)
    bridged = b1._launches > a._dropped_snapshots
    print("resumed after", b1._launches, "snapshots; the window begins after", a._dropped_snapshots)
    assert (pa["autocorr"].n_pairs - pb["autocorr"].n_pairs).tolist() == ([0, 1, 2, 3] if bridged else [0, 0, 0, 0])
    b2.close()
    c2.close()
