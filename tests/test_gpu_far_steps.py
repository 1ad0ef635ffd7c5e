"""Every step kernel FAR OUT: device against oracle, bit for bit, across the step indices where an
index of the kernels or their launchers carries into a high word -- 2^31 and 2^32 (the Philox
counter words of a step), 2^33 (the index of the paired stream, step div 2), L 2^31 and L 2^32
(the cycle index of a cycle of L steps, which the specification keeps modulo 2^32), and for
dragging 2^32 / n_drag (the fast sub-step counter).  A run at 10^6 steps per walker and second is
there within the hour; the tests get there by tests/far_steps.py: `teleport`, which rewrites the
step counter of a full state.  The cases and their boundaries: tests/far_steps.py; that the oracle's
result at each of them differs from what a narrowed index would give: tests/test_far_steps_host.py.

Per boundary B one launch of 24 steps that begins on B, then launches of 8, 30 and 17 steps from
B - 21 (before B, across it, beyond it), the whole state compared after every launch.  First of all
the same launches at step 4099: a failure THERE blames the teleport, not a far step."""
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402,F401  (before the first Engine: function targets need ONE HIP runtime)

from cobaya_amd import engine as E  # noqa: E402
from cobaya_amd import pliklite as P  # noqa: E402
from oracle import cbind as O  # noqa: E402
from tests import far_steps as F  # noqa: E402
from tests import huge_ref  # noqa: E402
from tests.pliklite_common import sampling_problem, small_dataset  # noqa: E402
from tests.test_gpu_parity import bits  # noqa: E402
from tests.test_gpu_support_walls import compare_everything  # noqa: E402

SEED = 3
CONTROL_B = F.CONTROL + F.BEFORE


def make_far_pair(c, cap=0, burn_in=0, thin=1):
    """Engine and oracle of a case on ONE set of constants (the engine's)."""
    kinds, a, b, periodic, blocking, means, covs, x0 = F.case_problem(c)
    own = c.variant == "own"
    eng = E.Engine(c.d, c.W, group_size=c.gs, seed=SEED, incremental=c.inc, emit_capacity=cap,
                   burn_in=burn_in, shared_basis=not own, basis_group_size=c.bgs if c.inc else None)
    eng.set_prior(kinds.tolist(), a.tolist(), b.tolist(),
                  None if periodic is None else periodic.tolist())
    eng.set_target_gaussian_mixture(means, covs, None)
    kw = {}
    if blocking is not None:
        blocks, over, last_slow, n_drag = blocking
        eng.set_blocking(blocks, over, last_slow, n_drag)
        kw = dict(blocks=blocks, oversampling=over, drag_last_slow=last_slow, drag_steps=n_drag)
    eng.set_proposal_cov(covs[0])
    if thin > 1:
        eng.set_emit_thin(thin)
    prob = O.Problem(c.d, kinds.tolist(), a.tolist(), b.tolist(), periodic=periodic, means=means,
                     covs=covs, T=eng.get_proposal_transform(), group_size=1 if own else c.bgs,
                     seed=SEED, derived=eng.derived_constants(), incremental=c.inc,
                     carry_modes=eng.carries_modes(), carry_periodic=eng.carries_periodic(), **kw)
    eng.set_state(x0)
    st = O.State(prob, x0, burn_in=burn_in, row_cap=cap, thin=thin)
    return eng, prob, st


def where(B, S0, launch, step):
    p = max(B.bit_length() - 1, 0)
    name = f"2^{p}" if B == 1 << p else f"{B / F.P32:.6g} x 2^32"
    return f"B = {B} ({name}), teleported to {S0}, launch {launch}, after step {step}: "


def compare(eng, st, B, S0, launch):
    """compare_everything, naming the boundary, the launch and the first walker and dimension
    that differ."""
    what = where(B, S0, launch, st.step)
    try:
        return compare_everything(eng, st, what)
    except AssertionError as e:
        x = eng.get_full_state()["x"]
        bad = np.argwhere(bits(x) != bits(st.x))
        first = (f"first differing walker {bad[0][0]}, dimension {bad[0][1]} of {len(bad)}"
                 if len(bad) else "x is equal")
        raise AssertionError(f"{what}{first}; {e}") from None


def cross(eng, st, B, after=None, n_accept_base=None):
    """The two passes of boundary B (tests/far_steps.py: passes), a fresh teleport for each."""
    for S0, launches in F.passes(B):
        F.teleport(eng, st, S0, n_accept_base)
        for i, n in enumerate(launches):
            eng.step(n)
            eng.sync()
            st.run(n, n_threads=8)
            compare(eng, st, B, S0, i)
            if after is not None:
                after(B, S0, i)
        assert int(eng.get_full_state()["step"]) == st.step == S0 + sum(launches)


def assert_kernel(c, kernel):
    assert c.path
    for word in c.path:
        assert word in kernel, (c.name, kernel)
    assert ("_inc_" in kernel or "_duo_" in kernel) == c.inc, kernel    # (from scratch: neither)
    assert ("two lanes" in kernel or "duo" in kernel) == c.duo, kernel
    if c.mode is not None or c.dq is not None:
        m = re.search(r"step_inc_kernel<(\d+), (\d),", kernel)
        assert m, kernel
        if c.dq is not None:
            assert int(m.group(1)) == c.dq, kernel
        if c.mode is not None:
            assert int(m.group(2)) == c.mode, kernel


@pytest.mark.parametrize("c", F.CASES, ids=F.case_id)
def test_steps_across_far_boundaries_bit_exact(c, monkeypatch):
    if c.duo:
        monkeypatch.setenv("MCMC_HIP_DUO", "1")
    eng, prob, st = make_far_pair(c)
    assert eng.cycle_length() == F.cycle_lengths(c)[0]
    compare_everything(eng, st, "start: ")
    eng.step(5)      # (so that every carried value exists before the first teleport)
    eng.sync()
    st.run(5, n_threads=8)
    compare_everything(eng, st, "after 5 steps from 0: ")
    cross(eng, st, CONTROL_B)                 # the control first: the teleport itself
    assert_kernel(c, eng.last_step_kernel())
    for B in F.boundaries(c):
        cross(eng, st, B)
    kernel = eng.last_step_kernel()
    print(f"{c.name}: {kernel}; boundaries {F.boundaries(c)}")
    assert_kernel(c, kernel)
    counters = eng.counters()
    assert counters["steps"] == st.step and counters["accepted"] == int(st.n_accept.sum())
    eng.close()


# ------------------------------------------------------------------ d > 128
class HugeState:
    """tests/huge_ref.py (the restatement of the oracle's step beyond its d = 128) behind the
    interface `teleport` and the comparison need."""

    def __init__(self, prob, x0):
        self.p, self.s, self.step, self.anchor = prob, huge_ref.fresh_state(prob, x0), 0, True

    @property
    def n_accept(self):
        return self.s["n_accept"]

    def run(self, n):
        huge_ref.run(self.p, self.s, n, step0=self.step, anchor=self.anchor)
        self.anchor = False    # (y is formed by the first launch, like the engine's)
        self.step += n


@pytest.mark.parametrize("d", F.HUGE_DIMS)
def test_huge_steps_across_far_boundaries_bit_exact(d):
    """huge_kernels.hip: a launch stays inside one cycle, y is refreshed from x at the multiples
    of 40 d -- at d = 205 step 2^33 + 8 is one, inside the launch across 2^33."""
    from tests.test_gpu_huge_dim import _engine
    W, gs, K = 256, 64, 1
    eng, kinds, a, b, means, covs, rng = _engine(d, K, W, gs, 100 + d)
    x0 = np.clip(means[0] + 0.5 * rng.standard_normal((W, d)) * np.sqrt(np.diag(covs[0])), 0.001, 0.999)
    eng.set_state(x0)
    prob = O.Problem(d, kinds, a, b, means=means, covs=covs, T=eng.get_proposal_transform(),
                     group_size=gs, seed=100 + d, incremental=True, max_tries=40 * d,
                     derived=eng.derived_constants())
    assert prob.refresh_every == 40 * d
    ref = HugeState(prob, x0)

    def same(what):
        s = eng.get_full_state()
        for k in ("x", "logpost", "logprior", "loglike"):
            bad = np.argwhere(bits(s[k]) != bits(ref.s[k]))
            assert not len(bad), f"{what}{k}: first differing index {bad[0]} of {len(bad)}"
        assert np.array_equal(bits(s["y"]), bits(ref.s["y"].reshape(W, K * d))), what + "y"
        for k in ("weight", "prior_rej", "n_accept"):
            assert np.array_equal(s[k], ref.s[k]), what + k

    eng.step(5)
    eng.sync()
    ref.run(5)
    same("after 5 steps from 0: ")
    refreshed = []
    for B in (CONTROL_B, F.P31, F.P32, F.P33, d * F.P31, d * F.P32):
        for S0, launches in F.passes(B):
            F.teleport(eng, ref, S0)
            for i, n in enumerate(launches):
                if any((ref.step + k) % (40 * d) == 0 for k in range(n)):
                    refreshed.append((B, S0, i))
                eng.step(n)
                eng.sync()
                ref.run(n)
                same(where(B, S0, i, ref.step))
    assert eng.last_step_kernel().startswith("mcmc::huge_step_kernel")
    assert ((F.P33, F.P33 - F.BEFORE, 1) in refreshed) == (d == 205), refreshed
    assert 0 < ref.n_accept.sum() < W * ref.step
    assert eng.counters()["steps"] == ref.step and eng.counters()["accepted"] == int(ref.n_accept.sum())
    eng.close()


# ------------------------------------------------------------------ function targets
def test_function_target_steps_across_far_boundaries_bit_exact():
    """fn_walker_kernel (d = 3: the cycle index is step div 3), by record and replay as in
    tests/test_gpu_function_target.py: the reference is stepped with the values the function
    returned on the device; the trial points it was given are the reference's, bit for bit."""
    from tests.test_gpu_function_target import KERNEL, Recorder, _assert_states_equal, _bits, _pair
    d, W, gs = 3, 128, 64
    rec = Recorder()
    eng, ref = _pair(d, W, gs, rec)
    _assert_states_equal(eng, ref)
    rec.on = True

    def launch(n, what):
        rec.calls.clear()
        eng.step(n)
        eng.sync()
        assert len(rec.calls) == n
        for pts, ll in rec.calls:
            t = ref.propose()
            bad = np.argwhere(_bits(pts) != _bits(t))
            assert not len(bad), f"{what}trial of step {ref.step}: first differing walker {bad[0][0]}, dimension {bad[0][1]}"
            ref.accept(ll)
        _assert_states_equal(eng, ref)

    launch(5, "from 0: ")
    for B in (CONTROL_B, F.P31, F.P32, d * F.P31, d * F.P32):
        for S0, launches in F.passes(B):
            F.teleport(eng, ref, S0)
            ref._cycle = None      # (its cache of the cycle's bases)
            for i, n in enumerate(launches):
                launch(n, where(B, S0, i, ref.step))
    assert eng.last_step_kernel().startswith(KERNEL)
    assert 0 < ref.n_accept.sum() < W * 400
    assert eng.counters()["steps"] == ref.step == d * F.P32 - F.BEFORE + sum(F.LAUNCHES)
    eng.close()


# ------------------------------------------------------------------ plik-lite
def test_binned_likelihood_steps_across_far_boundaries_bit_exact():
    """pl_fused_kernel: three launches per Metropolis step, the proposal of step s + 1 in the
    launch that accepts step s."""
    ds = small_dataset()
    target = P.BinnedGaussian.from_dataset(ds)
    emu = P.synthetic_emulator(5, ds.lmax)
    d, W, gs = emu.n + 1, 256, 64
    kinds, a, b, C = sampling_problem(target, emu)
    eng = E.Engine(d, W, group_size=gs, seed=SEED)
    eng.set_prior(kinds, a, b)
    eng.set_target_binned_gaussian(target, emu, calib_index=emu.n)
    eng.set_proposal_cov(C)
    k = eng.binned_constants()
    Bn = O.Binned(target.bin_table(), target.weights, target.X_data, Linv=k["Linv"],
                  theta0=emu.theta0, D0=emu.D0, J=emu.J, calib=emu.n)
    prob = O.Problem(d, kinds, a, b, T=eng.get_proposal_transform(), group_size=gs, seed=SEED,
                     derived=eng.derived_constants(), binned=Bn)
    rng = np.random.default_rng(77)
    x0 = np.concatenate((emu.theta0, [1.0])) + rng.standard_normal((W, d)) @ np.linalg.cholesky(C).T
    eng.set_state(x0)
    st = O.State(prob, x0)
    compare_everything(eng, st, "start: ")
    for B in (CONTROL_B, F.P31, F.P32, d * F.P31, d * F.P32):
        cross(eng, st, B)
    assert "pl_fused_kernel" in eng.last_step_kernel()
    assert 0 < st.n_accept.sum() < W * 400
    assert eng.counters()["accepted"] == int(st.n_accept.sum())
    eng.close()


# ------------------------------------------------------------------ emitted rows
@pytest.mark.parametrize("name", ["from scratch, burn-in 2", "incremental, thinned by 3"])
def test_emitted_rows_across_2_32_bit_exact(name):
    """Rows (and, thinned on the device, the walkers' remainders) across B = 2^32.  The rows a
    launch stored are drained before the next teleport: set_full_state empties the row store."""
    inc = name.startswith("incremental")
    c = (F._c("emit-d9-thin3", 9, inc=True, path=["step_inc_kernel", "emit"], dq=3, mode=0) if inc
         else F._c("emit-d3", 3, path=["::step_kernel<false, true>"]))
    thin = 3 if inc else 1
    eng, prob, st = make_far_pair(c, cap=64, burn_in=0 if inc else 2, thin=thin)
    n_rows = [0]

    def rows_equal(B, S0, i):
        rows, ref = eng.drain_samples(), st.drain()
        what = where(B, S0, i, st.step)
        assert rows.shape == ref.shape, what + f"{rows.shape} rows against {ref.shape}"
        bad = np.argwhere(bits(rows) != bits(ref))
        assert not len(bad), what + f"emitted rows: first differing row {bad[0][0]}, column {bad[0][1]}"
        if thin > 1:
            assert np.array_equal(eng.get_thin_carry(), st.thin_acc), what + "thin remainders"
        n_rows[0] += len(rows)

    eng.step(5)
    eng.sync()
    st.run(5, n_threads=8)
    rows_equal(0, 0, 0)
    for B in (CONTROL_B, F.P32):
        cross(eng, st, B, after=rows_equal)
        if thin > 1:
            assert st.thin_acc.max() > 0      # remainders were carried over the teleports
    assert_kernel(c, eng.last_step_kernel())
    assert n_rows[0] > c.W and eng.counters()["dropped_rows"] == 0
    eng.close()


# ------------------------------------------------------------------ the scheduler's switches
@pytest.mark.parametrize("switch", ["MCMC_HIP_NO_PREFETCH", "MCMC_HIP_LOOKAHEAD", "MCMC_HIP_EAGER_DIRECTIONS"])
def test_scheduler_switches_across_2_32_bit_exact(switch, monkeypatch):
    """tests/test_gpu_schedule_invariance.py at far steps: a direction set prepared ahead is
    recognised by its first step (DirSet::step0 == span.step0), 64 bits on both sides."""
    monkeypatch.setenv(switch, "1")      # (mcmc_hip_create reads them)
    c = F.BY_NAME["inc-d30-mode0"]
    eng, prob, st = make_far_pair(c)
    eng.step(5)
    eng.sync()
    st.run(5, n_threads=8)
    for B in (CONTROL_B, F.P32):
        cross(eng, st, B)
    assert_kernel(c, eng.last_step_kernel())
    eng.close()


# ------------------------------------------------------------------ counters
@pytest.mark.parametrize("base", [F.P31 - 3, F.P32 - 3], ids=["2^31-3", "2^32-3"])
@pytest.mark.parametrize("name", ["scratch-d13", "inc-d30-mode0", "duo-d30"])
def test_accept_counters_beyond_32_bits(name, base, monkeypatch):
    """Every walker's n_accept starts three accepts below 2^31 / 2^32; the ensemble total
    (acc_total, fed by the kernels' 32-bit per-launch counter) is then 2^38 or 2^39."""
    c = F.BY_NAME[name]
    if c.duo:
        monkeypatch.setenv("MCMC_HIP_DUO", "1")
    eng, prob, st = make_far_pair(c)
    S0 = F.P32 - F.BEFORE
    F.teleport(eng, st, S0, n_accept_base=base)
    assert eng.counters()["accepted"] == c.W * base
    for i, n in enumerate(F.LAUNCHES):
        eng.step(n)
        eng.sync()
        st.run(n, n_threads=8)
        compare(eng, st, F.P32, S0, i)
    s = eng.get_full_state()
    assert s["n_accept"].dtype == np.int64 and np.array_equal(s["n_accept"], st.n_accept)
    assert np.sum(st.n_accept > base + 3) > c.W // 2       # most walkers passed the power of two
    counters = eng.counters()
    total = int(st.n_accept.sum())
    assert total > c.W * base > 1 << 37 and counters["accepted"] == total
    assert counters["steps"] == S0 + sum(F.LAUNCHES) == st.step
    assert isinstance(counters["steps"], int) and isinstance(counters["accepted"], int)
    assert_kernel(c, eng.last_step_kernel())
    eng.close()
