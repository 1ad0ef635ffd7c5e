"""A call of mcmc_hip_step that ENDS A SPAN of direction cycles inside it.  The steppers that form
their directions call by call (from scratch, blocked, dragging, one function, several functions,
the binned target) cut a call where the direction buffer's byte budget ends
(cobaya_amd/csrc/step_span.h); at a test's size that is hundreds of thousands of cycles away, in
production about every 270 steps at d = 30 with 65 536 walkers.  MCMC_HIP_DIR_BUDGET_KIB=1 makes every
span ONE cycle: a call of 2 steps (so that the next begins inside a cycle), then one of 3 L + 2 steps
across four span ends, the whole state compared after each -- with the oracle (or the stepper's
reference) bit for bit, and with an engine of the same seed that ran without the switch.  That the
switch is in force is seen where a span is a launch (the Gaussian targets: `step_launches`); the
function and binned steppers launch per step and read the same budget (ctx.h: max_span_cycles)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402,F401  (before the first Engine: function targets need ONE HIP runtime)

from cobaya_amd import pliklite as P  # noqa: E402
from oracle import cbind as O  # noqa: E402
from tests import far_steps as F  # noqa: E402
from tests import test_gpu_function_blocks as FBT  # noqa: E402
from tests import test_gpu_function_target as FT  # noqa: E402
from tests.pliklite_common import small_dataset  # noqa: E402
from tests.test_gpu_far_steps import make_far_pair  # noqa: E402
from tests.test_gpu_parity import bits  # noqa: E402
from tests.test_gpu_pliklite import make as make_binned  # noqa: E402
from tests.test_gpu_support_walls import compare_everything  # noqa: E402
from tests.test_step_span_host import spans_restated  # noqa: E402

SWITCH = "MCMC_HIP_DIR_BUDGET_KIB"


def calls(L):
    return (2, 3 * L + 2)


def assert_same_engines(eng, plain, what, keys=()):
    a, b = eng.get_full_state(), plain.get_full_state()
    for k in ("x", "logpost", "logprior", "loglike") + tuple(keys):
        assert np.array_equal(bits(a[k]), bits(b[k])), f"{what}{k} differs from the engine without {SWITCH}"
    for k in ("weight", "prior_rej", "burn_left", "n_accept", "step"):
        assert np.array_equal(a[k], b[k]), f"{what}{k} differs from the engine without {SWITCH}"


def both(monkeypatch, make):
    """make() twice: without the switch, then with it (mcmc_hip_create reads it)."""
    monkeypatch.delenv(SWITCH, raising=False)
    plain = make()
    monkeypatch.setenv(SWITCH, "1")
    return make(), plain


# ------------------------------------------------------------------ Gaussian targets, from scratch
@pytest.mark.parametrize("c", [F._c("scratch-d3", 3, path=["::step_kernel<"]), F.BY_NAME["scratch-d8-blocked"],
                               F.BY_NAME["scratch-d6-drag"]], ids=F.case_id)
def test_from_scratch_steppers_across_span_ends_bit_exact(c, monkeypatch):
    (eng, prob, st), (plain, _, _) = both(monkeypatch, lambda: make_far_pair(c))
    L = eng.cycle_length()
    assert L == F.cycle_lengths(c)[0] == {"scratch-d3": 3, "scratch-d8-blocked": 13}.get(c.name, L)
    assert c.W // c.gs > 1
    compare_everything(eng, st, "start: ")
    _, n_drag, Lf = F.cycle_lengths(c)
    for n in calls(L):
        # these steppers launch one step kernel per span: that the switch is in force shows in their
        # number (1 KiB holds no cycle: one per span, and of the fast directions the least, two)
        spans = spans_restated(st.step, n, L, 1, n_drag, Lf, 2)
        assert len(spans) == 1 if n == 2 else len(spans) >= 4
        for e, launches in ((eng, len(spans)), (plain, 1)):
            e.kernel_times(reset=True)
            e.step(n)
            e.sync()
            assert e.kernel_times()["step_launches"] == launches
        st.run(n, n_threads=8)
        compare_everything(eng, st, f"after {st.step} steps: ")
        assert_same_engines(eng, plain, f"after {st.step} steps: ")
    for word in c.path:
        assert word in eng.last_step_kernel(), eng.last_step_kernel()
    assert 0 < st.n_accept.sum() < c.W * st.step and eng.counters()["steps"] == st.step == 3 * L + 4
    eng.close()
    plain.close()


# ------------------------------------------------------------------ one function
def test_function_stepper_across_span_ends_bit_exact(monkeypatch):
    d, W, gs = 3, 128, 64
    rec, rec_plain = FT.Recorder(), FT.Recorder()
    monkeypatch.delenv(SWITCH, raising=False)
    plain, _ = FT._pair(d, W, gs, rec_plain)
    monkeypatch.setenv(SWITCH, "1")
    eng, ref = FT._pair(d, W, gs, rec)
    FT._assert_states_equal(eng, ref)
    rec.on = True
    for n in calls(d):
        rec.calls.clear()
        for e in (eng, plain):
            e.step(n)
            e.sync()
        assert len(rec.calls) == n
        for pts, ll in rec.calls:
            t = ref.propose()
            assert np.array_equal(FT._bits(pts), FT._bits(t)), f"trial of step {ref.step}"
            ref.accept(ll)
        FT._assert_states_equal(eng, ref)
        assert_same_engines(eng, plain, f"after {ref.step} steps: ")
    assert eng.last_step_kernel().startswith(FT.KERNEL)
    assert 0 < ref.n_accept.sum() < W * ref.step and ref.step == 3 * d + 4
    eng.close()
    plain.close()


# ------------------------------------------------------------------ two functions over two blocks
def test_functions_stepper_across_span_ends_bit_exact(monkeypatch):
    # d = 4 in blocks 2 + 2 with factors 1 and 2 (L = 6), two groups; function 0 reads the slow block
    # alone and is spared on the fast slots
    monkeypatch.setitem(FBT.LAYOUTS, "d4", (4, 128, 64, [[1, 3], [0, 2]], [1, 2], [[1, 3], [3, 0, 2]], 1.0, ()))
    monkeypatch.delenv(SWITCH, raising=False)
    plain, _, _ = FBT._pair("d4")
    monkeypatch.setenv(SWITCH, "1")
    eng, ref, fns = FBT._pair("d4")
    L = ref.p.cycle_length()
    assert L == eng.cycle_length() == 6 and ref.W // 64 > 1
    FBT._assert_states_equal(eng, ref)
    for n in calls(L):
        plain.step(n)
        plain.sync()
        FBT._replay(eng, ref, fns, n)
        FBT._assert_states_equal(eng, ref)
        assert_same_engines(eng, plain, f"after {ref.step} steps: ", keys=("ll_c",))
    assert eng.last_step_kernel().startswith(FBT.KERNEL)
    assert min(ref.calls) < max(ref.calls) == ref.step == 3 * L + 4
    assert 0 < ref.n_accept.sum() < ref.W * ref.step
    eng.close()
    plain.close()


# ------------------------------------------------------------------ the binned target
def test_binned_stepper_across_span_ends_bit_exact(monkeypatch):
    # the smallest case of test_binned_steps_bit_exact: 88 bins, d = 6, 256 walkers in groups of 64
    ds = small_dataset()
    target = P.BinnedGaussian.from_dataset(ds)
    emu = P.synthetic_emulator(5, ds.lmax)
    W, gs, T, d = 256, 64, 1.0, emu.n + 1
    (eng, prob, B, C), (plain, _, _, _) = both(monkeypatch, lambda: make_binned(target, emu, W=W, gs=gs, T=T))
    rng = np.random.default_rng(77)
    x0 = np.concatenate((emu.theta0, [1.0])) + rng.standard_normal((W, d)) @ np.linalg.cholesky(C).T
    eng.set_state(x0)
    plain.set_state(x0)
    st = O.State(prob, x0)
    compare_everything(eng, st, "start: ")
    for n in calls(d):
        for e in (eng, plain):
            e.step(n)
            e.sync()
        st.run(n, n_threads=4)
        compare_everything(eng, st, f"after {st.step} steps: ")
        assert_same_engines(eng, plain, f"after {st.step} steps: ")
    assert "pl_fused_kernel" in eng.last_step_kernel()
    assert 0 < st.n_accept.sum() < W * st.step and eng.counters()["steps"] == st.step == 3 * d + 4
    eng.close()
    plain.close()
