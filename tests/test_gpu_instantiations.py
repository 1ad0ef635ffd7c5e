"""Every reachable instantiation of the incremental step kernels ONCE, device against oracle,
bit for bit: the cases of tests/instantiations.py (their conditions, on the oracle alone:
tests/test_instantiations_host.py).  Per case a launch of 5 steps from step 0, a teleport to
40 L - 70 (tests/far_steps.py) and one launch of 133 steps: every kernel's column chunk is at
most 64 columns, so the long launch crosses two chunk boundaries and reuses a double buffer,
crosses the refresh of y at 40 L and a cycle boundary.  After each launch x, the log-posterior
parts, weights, accept counts, the carried y and mode log-densities and the emitted rows are the
oracle's, and last_step_kernel() is the predicted name.  The kernels that evaluate every trial
from scratch (walker_kernels.hip at every compiled D, walker_kernels_big.hip at the smallest and
the largest d of every DP) need no teleport: 5 steps, then d + 7.

A device error (anything but a failed comparison) ends the module: no engine is created after it."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import instantiations as I  # noqa: E402
from tests.far_steps import teleport  # noqa: E402
from tests.test_gpu_parity import assert_bit_equal, compare_state, make_pair  # noqa: E402


def _items():
    """(family, dq, MODE or KM) -> names: one pytest item runs at most about a dozen engines."""
    items = {}
    for n in I.swept():      # (every reachable name but I.HELD_BACK)
        third = n.km if n.km else n.mode if n.mode is not None else 0
        items.setdefault((n.family, n.dq, third), []).append(n)
    return items


ITEMS = _items()
SITEMS = {}
for _n in I.enumerate_scratch():
    if not _n.why:
        SITEMS.setdefault((_n.family, _n.D), []).append(_n)
DEVICE_ERROR = []      # the first exception that was no failed comparison


def run_all(cases, run):
    """Every case of an item; failed comparisons are collected, anything else is a device error."""
    if DEVICE_ERROR:
        pytest.fail(f"not run: the device reported an error earlier in this module: {DEVICE_ERROR[0]}")
    failed = []
    for c in cases:
        try:
            run(c)
        except AssertionError as e:
            failed.append(str(e))
        except BaseException as e:
            DEVICE_ERROR.append(f"{c.name} at d = {c.d}: {type(e).__name__}: {e}")
            raise
    assert not failed, "\n".join(failed)


def run_case(c):
    args, kw = I.pair_arguments(c)
    eng, prob, st = make_pair(*args, **kw)
    try:
        what = f"{c.name} at d = {c.d} (seed {c.seed}): "
        L = eng.cycle_length()
        assert L == I.cycle_length(c), what
        compare_state(eng, st)
        for launch, n in enumerate((I.FIRST, I.LONG)):
            if launch == 1:
                teleport(eng, st, I.teleport_target(L))
            eng.step(n)
            eng.sync()
            st.run(n, n_threads=8)
            where = what + f"launch {launch}, after step {st.step}: "
            try:
                compare_state(eng, st)
            except AssertionError as e:
                raise AssertionError(where + str(e)) from None
            full = eng.get_full_state()
            assert_bit_equal(full["y"], st.y, where + "carried whitened residuals")
            assert np.array_equal(full["n_accept"], st.n_accept), where + "n_accept"
            assert np.array_equal(full["prior_rej"], st.prior_rej), where + "prior_rej"
            if c.emit:
                rows, ref = eng.drain_samples(), st.drain()
                assert rows.shape == ref.shape, where + f"{rows.shape} rows against {ref.shape}"
                assert_bit_equal(rows, ref, where + "emitted rows")
            # (the engine appends the dimension it ran at to the launcher's name)
            assert eng.last_step_kernel() == f"{c.name} (d={c.d})", where + eng.last_step_kernel()
        counters = eng.counters()
        assert counters["accepted"] == int(st.n_accept.sum()) and counters["dropped_rows"] == 0, what
    finally:
        eng.close()


@pytest.mark.parametrize("family,dq,third", list(ITEMS), ids=[f"{f}-dq{q}-{t}" for f, q, t in ITEMS])
def test_every_instantiation_bit_exact(family, dq, third, monkeypatch):
    if family in (I.DUO_MIX, I.DUO_ONE):
        monkeypatch.setenv("MCMC_HIP_DUO", "1")      # (mcmc_hip_create reads it)
    run_all([c for n in ITEMS[(family, dq, third)] for c in I.cases_of(n)], run_case)


def run_scratch_case(c):
    args, kw = I.scratch_pair_arguments(c)
    eng, prob, st = make_pair(*args, **kw)
    try:
        what = f"{c.name} at d = {c.d}, D = {c.D}: "
        compare_state(eng, st)
        for launch, n in enumerate(I.scratch_steps(c)):
            eng.step(n)
            eng.sync()
            st.run(n, n_threads=8)
            where = what + f"launch {launch}, after step {st.step}: "
            try:
                compare_state(eng, st)
            except AssertionError as e:
                raise AssertionError(where + str(e)) from None
            full = eng.get_full_state()
            assert np.array_equal(full["n_accept"], st.n_accept), where + "n_accept"
            assert np.array_equal(full["prior_rej"], st.prior_rej), where + "prior_rej"
            assert eng.last_step_kernel() == f"{c.name} (d={c.d})", where + eng.last_step_kernel()
        assert eng.counters()["accepted"] == int(st.n_accept.sum()), what
    finally:
        eng.close()


@pytest.mark.parametrize("family,D", list(SITEMS), ids=[f"{f}-D{q}" for f, q in SITEMS])
def test_every_from_scratch_instantiation_bit_exact(family, D):
    run_all([c for n in SITEMS[(family, D)] for c in I.scratch_cases_of(n)], run_scratch_case)
