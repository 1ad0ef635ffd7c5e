"""The scheduler's developer switches give the oracle's bits.

Between two step kernels of an incremental run the engine forms direction sets on a second stream,
ahead of the launch that needs them or at the call that begins with it, refreshes y = L^-1 (x - mu)
in a kernel of its own or inside the step kernel, and keeps a set over several calls
(capi_incremental.hip: acquire_direction_set, launch_segment, prepare_next_set).  Three switches,
read by mcmc_hip_create, move that work around -- MCMC_HIP_NO_PREFETCH (everything in line on the
main stream), MCMC_HIP_LOOKAHEAD=1 (a set per call), MCMC_HIP_EAGER_DIRECTIONS=1 (the next call's
set formed at the end of this one) -- and docs/KERNELS.md promises the same bits for all of them.
Here every kernel family runs under each: 256 walkers, R-1 groups of 64, a Haar basis per 128,
d = 6, so y is refreshed every R = 40 d = 240 steps; calls of 150, 170, 1 and 400 steps cross the
refresh at 240, 480 and 720, and the last call holds two refreshes (where a set spans calls, the
second is the step kernel's own).  The proposal is refreshed after the second call, which makes
every set formed ahead stale.  After every call the whole state -- x, the carried y and mode
log-densities, log-posterior parts, weights, counters -- is the C oracle's, bit for bit.

Launches cut by the direction buffers (IncPlan::max_cyc, max_steps_vu) cannot be reached at this
size; they stay covered at d = 100 by test_gpu_bench_geometry.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from test_gpu_parity import assert_bit_equal, compare_state, make_pair  # noqa: E402

D, W, GS, BGS = 6, 256, 64, 128
CALLS = (150, 170, 1, 400)

SHAPES = {
    "one-box": (dict(), None, "step_inc_kernel<2, "),
    "one-box-two-lanes": (dict(), {"MCMC_HIP_DUO": "1"}, "two lanes>"),
    "two-normal-priors": (dict(kinds=[0, 1, 0, 0, 1, 0], a=[0.0, 0.5, 0.0, 0.0, 0.5, 0.0],
                               b=[1.0, 0.25, 1.0, 1.0, 0.25, 1.0]), None, "step_inc_kernel<2, "),
    "one-periodic": (dict(periodic=[0, 0, 1, 0, 0, 0]), None, "periodic>"),
    "two-modes": (dict(K=2), None, "step_inc_mix_kernel"),
    "two-modes-one-periodic": (dict(K=2, periodic=[0, 0, 1, 0, 0, 0]), None, "mcmc::step_inc_"),
    "dragging": (dict(blocks=[[0, 1], [2, 3, 4, 5]], over=[1, 1], drag_last_slow=0, drag_steps=3),
                 None, "drag_inc_kernel"),
}
SWITCHES = {"default": {}, "no-prefetch": {"MCMC_HIP_NO_PREFETCH": "1"},
            "lookahead-1": {"MCMC_HIP_LOOKAHEAD": "1"}, "eager": {"MCMC_HIP_EAGER_DIRECTIONS": "1"}}


@pytest.mark.parametrize("switch", list(SWITCHES))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_scheduler_switches_give_the_oracles_bits(shape, switch, monkeypatch):
    kw, env, kernel = SHAPES[shape]
    for k, v in {**(env or {}), **SWITCHES[switch]}.items():   # (mcmc_hip_create reads them)
        monkeypatch.setenv(k, v)
    eng, prob, st = make_pair(D, W, GS, incremental=True, basis_group_size=BGS, max_tries=1e9, **kw)
    # (dragging: a cycle is the two slow parameters, so y is refreshed every 80 steps)
    assert prob.refresh_every == (80 if shape == "dragging" else 240)
    for call, n in enumerate(CALLS):
        eng.step(n)
        eng.sync()
        st.run(n, n_threads=8)
        compare_state(eng, st)
        s = eng.get_full_state()
        assert_bit_equal(s["y"], st.y, f"{shape} / {switch}, call {call}: carried whitened residual")
        assert np.array_equal(s["prior_rej"], st.prior_rej) and np.array_equal(s["n_accept"], st.n_accept)
        assert int(s["step"]) == st.step
        name = eng.last_step_kernel()
        assert kernel in name and ("two lanes" in name) == (shape == "one-box-two-lanes"), name
        if call == 1:   # what a learn checkpoint does: sets formed ahead are stale from here on
            eng.set_proposal_cov(np.cov(st.x.T))
            prob.set_T(eng.get_proposal_transform())
    assert st.step == sum(CALLS) == 721
    assert eng.counters()["accepted"] == int(st.n_accept.sum()) > 0
    eng.close()
