"""The device products switched on TOGETHER, host side (no GPU): the sampler on the five CPU doubles
composed into one engine (tests/products_together.py; `derived` stays out: it has no double).  Each product
of the run with everything on equals, to the byte, the product of the run with that option alone, and the
chain equals the chain without any product; at a checkpoint every product's request / fetch state machine
runs once, undisturbed by its neighbours'; a resume in mid-interval restores all of them; no two products
share a key of the state file.  Every comparison is of bits."""
import functools

import numpy as np
import pytest

from cobaya_amd.model import ProblemSpec
from cobaya_amd.sampler import MCMCHip
from tests.products_together import ALL, ON_HOST, AllOracleEngine, on_host, only, same_as_replayed, same_product
from tests.test_host_logic import QUICK

HOST = on_host(ALL)
NONE = {k: None for k in HOST}
SPLIT = ("marginals", "bestfit")            # their unfinished interval is drained to the host
CLOSES = ("evidence", "importance")         # their request takes a flag; a peek is a request that does not close


class OnAll(MCMCHip):
    _engine_factory = staticmethod(AllOracleEngine)


def make(W=128, prefix=None, max_samples=None, resume=False, options=HOST, **opts):
    """The QUICK two-parameter model on the composed double.  `max_samples` defaults to what closes ten
    intervals, six of them in the window at the end, in 45 launches (at 128 walkers and at 512)."""
    o = {"seed": 21, "n_walkers": W, "group_size": 64, "steps_per_launch": 40, "moments_every": 1,
         "max_samples": 470 * W if max_samples is None else max_samples, "Rminus1_stop": 0.0,
         "learn_every": "20d", "snapshot_every": 40}
    o.update(options)
    o.update(opts)
    return OnAll(o, ProblemSpec.from_info(QUICK), output=prefix, resume=resume)


@functools.lru_cache(maxsize=None)
def finished(W, which, moments_every=1, every=1):
    """A finished run (not closed) with `which` on: "all", "none" or one product's name."""
    options = HOST if which == "all" else NONE if which == "none" else only(HOST, which)
    if every != 1 and options["evidence"]:
        options = dict(options, evidence=dict(options["evidence"], every=every))
    s = make(W, options=options, moments_every=moments_every)
    s.run()
    return s


def _chain(s):
    """What of a run does not depend on its products: the stored rows, the final state, the proposal
    covariance and the progress columns (the timestamp apart), as bytes."""
    st = s.engine.get_state()
    return {"rows": s.products()["sample"].data.to_numpy(dtype=np.float64).tobytes(),
            "x": np.asarray(st["x"]).tobytes(), "logpost": np.asarray(st["logpost"]).tobytes(),
            "proposal": s.engine.get_proposal_cov().tobytes(), "steps": s.n_steps_raw,
            "progress": s.progress[["N", "acceptance_rate", "Rminus1"]].to_numpy(dtype=np.float64).tobytes()}


# ------------------------------------------------------------------------------- together = alone = rule
@pytest.mark.parametrize("W", [128, 512])
def test_every_product_of_the_run_with_all_of_them_equals_its_run_alone(W):
    s = finished(W, "all")
    assert s._iv0 + len(s._intervals) >= 4 and len(s._intervals) >= 3 and s._dropped_snapshots > 0
    assert [p.name for p in s._products] == list(ON_HOST)
    got = s.products()
    for name in ON_HOST:
        alone = finished(W, name)
        assert [p.name for p in alone._products] == [name]
        same_product(name, got[name], alone.products()[name])
    want = _chain(finished(W, "none"))
    assert not finished(W, "none")._products
    for which in ("all",) + ON_HOST:
        have = _chain(finished(W, which))
        assert have == want, (which, [k for k in want if have[k] != want[k]])
    # ... and all of them counted the same snapshots: those of the moment window plus the unfinished interval
    n = sum(iv[0] for iv in s._intervals) + s._snaps_in_interval
    assert got["marginals"].n_accumulations == got["bestfit"].n_accumulations == got["importance"].n_acc == n
    assert int(got["evidence"].n_acc.sum()) == n == int(got["autocorr"].n_pairs[0])
    assert n * W == got["marginals"].n_samples == got["evidence"].n_samples == got["importance"].n_samples


@pytest.mark.parametrize("W", [128, 512])
def test_every_interval_of_every_product_equals_its_rule_over_the_stored_rows(W):
    """... = rule: the stored rows replayed through the numpy rules, interval by interval."""
    s = finished(W, "all")
    assert same_as_replayed(s) == {name: len(s._intervals) + 1 for name in ON_HOST}


def test_the_products_outlive_the_engine_unchanged():
    s = make()
    s.run()
    before = s.products()
    assert s.products(combined=True).keys() == before.keys()
    s.close()
    assert s.engine is None and all(p.engine is None for p in s._products)
    after = s.products()
    assert after["sample"].data.equals(before["sample"].data) and len(after["sample"].data) > 0
    for name in ON_HOST:
        same_product(name, after[name], before[name])
        same_product(name, after[name], finished(128, "all").products()[name])


# ------------------------------------------------------------------------------- one checkpoint, six state machines
def _check_log(log, lag):
    """What the composed double was asked, in stream order.  Returns the number of checkpoints."""
    live, k = list(ON_HOST), len(ON_HOST)
    pending, n_ckpt, steps_since, waits = {}, 0, None, []
    i = 0
    while i < len(log):
        verb, what, flag = log[i]
        if verb == "step":
            if steps_since is not None:
                steps_since += 1
        elif (verb, what) == ("request", "moments"):
            # a checkpoint: exactly one closing request of every live product, back to back, in the sampler's order
            assert not pending, (i, pending)
            assert log[i + 1:i + 1 + k] == [("request", p, True) for p in live], (i, log[i:i + 1 + k])
            pending = {p: "checkpoint" for p in live}
            n_ckpt, steps_since = n_ckpt + 1, 0
            i += k
        elif (verb, what) == ("fetch", "moments"):
            # ... each fetched `lag` launches later (fewer only where the run ends), before anything else
            assert log[i + 1:i + 1 + k] == [("fetch", p, None) for p in live], (i, log[i:i + 1 + k])
            assert set(pending) == set(live) and set(pending.values()) == {"checkpoint"}
            waits.append(steps_since)
            pending, steps_since = {}, None
            i += k
        elif verb == "request":
            # beside the checkpoints: a read of the unfinished interval, fetched at once
            assert what not in pending, (i, what, "a second request before the fetch")
            assert log[i + 1] == ("fetch", what, None), (i, log[i:i + 2])
            if what in CLOSES:
                assert flag is False, (i, what, "a peek that closes")
            elif what not in SPLIT:        # read out and set back to the same values
                assert log[i + 2] == ("set", what, None), (i, log[i:i + 3])
                i += 1
            i += 1
        elif verb == "fetch":
            raise AssertionError((i, what, "a fetch without its request"))
        elif verb == "set":
            assert what not in pending, (i, what, "a set between a request and its fetch")
        i += 1
    assert not pending
    assert all(w == lag for w in waits[:-1]) and 0 <= waits[-1] <= lag, (lag, waits)
    return n_ckpt


@pytest.mark.parametrize("lag", [1, 2])
def test_at_a_checkpoint_every_product_is_requested_once_and_fetched_before_its_next_request(lag, tmp_path):
    """With a state file written at every checkpoint, so that peeks, drains and sets fall between them."""
    s = make(prefix=str(tmp_path / "m"), checkpoint_lag=lag, output_every=0)
    s.run()
    log = s.engine.log
    n_ckpt = _check_log(log, lag)
    assert n_ckpt == len(s.progress) >= 4
    for p in ON_HOST:
        n_acc = sum(1 for e in log if e[:2] == ("accumulate", p))
        assert n_acc == s._launches == sum(1 for e in log if e[0] == "step")
        assert sum(1 for e in log if e[:2] == ("set", p)) == (0 if p in SPLIT + CLOSES else
                                                              sum(1 for e in log if e == ("request", p, True)) - n_ckpt)
    assert sum(1 for e in log if e[:2] == ("request", "importance") and e[2] is False) >= n_ckpt    # the saves' peeks
    # the saves moved nothing: the products are those of the run that wrote no file
    if lag == 2:
        for name in ON_HOST:
            same_product(name, s.products()[name], finished(128, "all").products()[name])


# ------------------------------------------------------------------------------- resume, the state file
def test_a_resume_in_mid_interval_with_everything_on_is_bit_identical(tmp_path):
    """Two legs against one uninterrupted run, ending at the same checkpoint.  `autocorr` does not restore
    its ring (the pairs that bridge the resume point are missing, tests/test_autocorr_host.py): its reference
    is the two-leg run with `autocorr` alone."""
    one = make(prefix=str(tmp_path / "a"), max_samples=40000)
    one.run()
    p = str(tmp_path / "b")
    b1 = make(prefix=p, max_samples=20000)
    b1.run()
    z = np.load(p + ".1.state.npz", allow_pickle=False)
    assert int(z["marg_open_n"]) > 0 and int(z["bf_open_n"]) > 0 and int(z["ev_open_n"][0]) > 0
    assert int(z["iw_open_nacc"][0]) > 0 and int(z["ac_open_pairs"][0]) > 0          # stopped in mid-interval
    b2 = make(prefix=p, max_samples=40000, resume=True)
    eng = b2.engine
    assert eng._mg_n == int(z["marg_open_n"]) and eng._bfr.n == int(z["bf_open_n"])  # back on the "device"
    assert eng._evr.n == int(z["ev_open_n"][0]) and eng._imr.n_acc == int(z["iw_open_nacc"][0])
    assert np.array_equal(eng._acr.sums, z["ac_open"]) and eng._acr.held == 0
    b2.run()
    assert b2.n_steps_raw == one.n_steps_raw > b1.n_steps_raw
    got, ref = b2.products(), one.products()
    for name in ON_HOST:
        if name != "autocorr":
            same_product(name, got[name], ref[name])
    q = str(tmp_path / "c")
    make(prefix=q, max_samples=20000, options=only(HOST, "autocorr")).run()
    c2 = make(prefix=q, max_samples=40000, resume=True, options=only(HOST, "autocorr"))
    c2.run()
    same_product("autocorr", got["autocorr"], c2.products()["autocorr"])
    assert (ref["autocorr"].n_pairs - got["autocorr"].n_pairs).tolist() == [0, 1, 2, 3]
    assert _chain(b2)["x"] == _chain(one)["x"] and _chain(b2)["proposal"] == _chain(one)["proposal"]


def test_no_two_products_share_a_key_of_the_state_file(tmp_path):
    """By set arithmetic over every accumulator's `save()`: a seventh product is covered as it is."""
    p = str(tmp_path / "k")
    s = make(prefix=p, max_samples=20000)
    s.run()
    make(prefix=str(tmp_path / "n"), max_samples=2000, options=NONE).run()
    own = set(np.load(str(tmp_path / "n") + ".1.state.npz", allow_pickle=False).files)
    keys = {q.name: set(q.save(False)) for q in s._products}
    assert len(keys) == len(s._products) == len(ON_HOST) and all(keys.values())
    names = list(keys)
    for i, a in enumerate(names):
        assert not keys[a] & own, (a, sorted(keys[a] & own))
        for b in names[i + 1:]:
            assert not keys[a] & keys[b], (a, b, sorted(keys[a] & keys[b]))
    written = set(np.load(p + ".1.state.npz", allow_pickle=False).files)
    assert written == own.union(*keys.values()), sorted(written ^ own.union(*keys.values()))


# ------------------------------------------------------------------------------- cadence
def test_moments_every_2_and_evidence_every_2_count_every_second_and_every_fourth_launch():
    s = finished(128, "all", 2, 2)
    log = s.engine.log
    n_launch = sum(1 for e in log if e[0] == "step")
    count = {p: sum(1 for e in log if e[:2] == ("accumulate", p)) for p in ON_HOST}
    assert n_launch == s._launches and all(count[p] == n_launch // 2 for p in ON_HOST if p != "evidence")
    assert count["evidence"] == n_launch // 4 > 4
    # every product but evidence beside every moment snapshot (every second launch), evidence beside every second
    at, snaps, ev = 0, [], []
    for verb, what, flag in log:
        at += flag if verb == "step" else 0
        if (verb, what) == ("accumulate", "marginals"):
            snaps.append(at)
        if (verb, what) == ("accumulate", "evidence"):
            ev.append(at)
    assert snaps == [80 * k for k in range(1, len(snaps) + 1)] and ev == [160 * k for k in range(1, len(ev) + 1)]
    got = s.products()
    n = sum(iv[0] for iv in s._intervals) + s._snaps_in_interval
    assert got["marginals"].n_accumulations == got["importance"].n_acc == n
    assert abs(2 * int(got["evidence"].n_acc.sum()) - n) <= 1 and got["autocorr"].interval_steps == 80
    for name in ON_HOST:
        same_product(name, got[name], finished(128, name, 2, 2).products()[name])
    assert _chain(s) == _chain(finished(128, "none", 2, 2))
