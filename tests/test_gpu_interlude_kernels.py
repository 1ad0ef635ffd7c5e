"""The kernels that run between two step kernels, at the edges of their layouts, bit for bit against
the oracle:

- group_moments_kernel (2 x 2 tiles of the lower triangle, a column pair per ds_read_b128; ragged
  tiles at odd d, diagonal tiles, tiles that wrap round the workgroup at gs = 64, the group sums on
  the last wave) and pool_moments_kernel (batches of 64 and 16 groups and a remainder, round 127,
  128, 255, 256 groups);
- whiten_state_kernel (rows_times_column: batches of eight and four columns and the triangle on the
  diagonal, ragged last row block, row blocks dealt to the waves in pairs; a workgroup whose walkers
  are partly absent) and, through short launches, whiten_directions_kernel, which shares the helper;
- the checkpoint read-out (request_moments / fetch_moments) of what those kernels accumulated."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from cobaya_amd import engine as E  # noqa: E402
from oracle import cbind as O  # noqa: E402
from tests.test_gpu_moments import _bits, _check, _states  # noqa: E402
from tests.test_gpu_parity import assert_bit_equal, compare_state, make_pair  # noqa: E402


# ------------------------------------------------------------------------------ moments
@pytest.mark.parametrize("d,gs,G", [(d, gs, G) for d in (1, 2, 3, 4, 5, 29, 30, 31, 32)
                                    for gs in (64, 128, 256) for G in (1, 2, 3)])
def test_moments_tile_edges(d, gs, G):
    """Odd d (a tile with a row and a column beyond d), d = 1 and 2 (one tile, diagonal), d = 29 ... 32
    at gs = 64 (120 / 136 tiles on 64 threads) and at gs = 256 (the sums beside the tiles); both
    sides of NPAIR + D <= 2 gs, where the layout before this one changed regime."""
    _check(d, gs, G)


@pytest.mark.parametrize("G", [127, 128, 129, 255, 256, 257])
def test_moments_pool_edges(G):
    """pool_moments_kernel: short of, at and past two and four batches of 64 groups, with the
    batches of 16 and the remainder behind them."""
    _check(6, 64, G)


# ------------------------------------------------------------------------------ whitening
def _whiten_case(d, K, W):
    eng, prob, st = make_pair(d, W, 64, K=K, incremental=True, rng=np.random.default_rng(31 * d + K))
    y = eng.get_full_state()["y"]          # (set_state left y to be formed: whiten_state_kernel)
    x = eng.get_state()["x"]
    eng.close()
    assert y.shape == (W, K * d)
    assert_bit_equal(y, prob.whiten(x), f"y = L^-1 (x - mu), d = {d}, K = {K}, W = {W}")
    assert_bit_equal(y, st.y, "the oracle's own start")


@pytest.mark.parametrize("W", [64, 192, 320])
@pytest.mark.parametrize("d", [2, 3, 4, 5, 7, 8, 9, 29, 30, 31, 32, 33, 100, 128])
def test_whiten_state_one_mode(d, W):
    """Row blocks 1 ... 32, ragged last blocks of 1, 2 and 3 rows, an odd and an even number of
    blocks (the middle block of the pairing), chains with and without the batch of four."""
    _whiten_case(d, 1, W)


@pytest.mark.parametrize("W", [64, 192, 320])
@pytest.mark.parametrize("K", [2, 3])
@pytest.mark.parametrize("d", [2, 3, 4, 5, 7, 8, 9, 29, 30, 31, 32])
def test_whiten_state_mixtures(d, K, W):
    """y is [K][d][W]: every mode with its own mean and its own L^-1."""
    _whiten_case(d, K, W)


def test_one_parameter_has_no_incremental_mode():
    """d = 1 never reaches whiten_state_kernel: the engine refuses incremental evaluation there."""
    with pytest.raises(E.EngineError, match="incremental evaluation needs d >= 2"):
        E.Engine(1, 64, group_size=64, device=0, seed=1, incremental=True)


# ------------------------------------------------------------------------------ directions
def _launches(d, W, gs, launches, **kw):
    eng, prob, st = make_pair(d, W, gs, incremental=True, **kw)
    for n in launches:
        eng.step(n)
        eng.sync()
        st.run(n, n_threads=8)
        compare_state(eng, st)
        assert_bit_equal(eng.get_full_state()["y"], st.y, "carried whitened residual")
    assert eng.counters()["accepted"] == int(st.n_accept.sum())
    eng.close()


@pytest.mark.parametrize("d", [2, 5, 30, 31])
def test_directions_short_launches(d):
    """Launches of 3 steps (one partly filled workgroup of whiten_directions_kernel) at d that is
    no multiple of 4, then 67 steps: a full workgroup of columns and a second one with three."""
    _launches(d, 256, 64, (3, 3, 67))


def test_directions_dragging_slots():
    _launches(9, 256, 64, (3, 3), blocks=[[0, 1, 2], [3, 4], [5, 6, 7, 8]], over=[1, 1, 2],
              drag_last_slow=1, drag_steps=3)


def test_directions_one_parameter_block():
    _launches(7, 256, 64, (3, 3), blocks=[[0, 1, 2], [3], [4, 5, 6]], over=[1, 2, 3])


def test_directions_normal_priors():
    _launches(27, 256, 64, (3, 3), kinds=[0] * 6 + [1] * 21, a=[0.0] * 6 + [0.5] * 21,
              b=[1.0] * 6 + [0.25] * 21)


# ------------------------------------------------------------------------------ read-out
def _moment_engine(d, gs, G, max_tries=None):
    eng = E.Engine(d, G * gs, group_size=gs, device=0, seed=3, max_tries=max_tries)
    eng.set_prior([0] * d, [-50.0] * d, [50.0] * d)
    eng.set_target_one()
    eng.set_proposal_cov(np.eye(d))
    return eng


@pytest.mark.parametrize("d,gs,G", [(5, 64, 3), (30, 256, 2)])
def test_read_out_equals_a_synchronous_read(d, gs, G):
    x1, x2, shift = _states(d, G * gs, 77 + d)
    engs = [_moment_engine(d, gs, G) for _ in range(2)]
    for eng in engs:
        eng.set_state(x1)
        eng.set_moment_shift(shift)
        eng.accumulate_moments()
        eng.set_state(x2)
        eng.accumulate_moments()
    n0, gsum0, S0 = engs[0].read_moments()
    engs[1].request_moments()
    n1, gsum1, S1, c = engs[1].fetch_moments()
    assert n0 == n1 == 2
    assert np.array_equal(_bits(gsum0), _bits(gsum1)) and np.array_equal(_bits(S0), _bits(S1))
    ref = engs[0].counters()
    assert c["steps"] == ref["steps"] == 0 and c["accepted"] == ref["accepted"] == 0
    gsum_o, S_o = O.moments(x1, gs, shift=shift)
    gsum_o, S_o = O.moments(x2, gs, shift=shift, group_sum=gsum_o, pooled=S_o)
    assert np.array_equal(_bits(gsum1), _bits(gsum_o)) and np.array_equal(_bits(S1), _bits(S_o))
    # the request reset the accumulators
    n, gsum, S = engs[1].read_moments()
    assert n == 0 and not gsum.any() and not S.any()
    for eng in engs:
        eng.close()


def test_read_out_reports_a_stuck_walker():
    """A walker that tripped max_tries is seen through the fetch (the run loop never synchronises)."""
    d, gs, G = 4, 64, 2
    eng = E.Engine(d, G * gs, group_size=gs, device=0, seed=5, max_tries=2.0)
    eng.set_prior([0] * d, [0.0] * d, [1.0] * d)
    eng.set_target_gaussian_mixture([np.full(d, 0.5)], [np.eye(d) * 1e-8])
    # (every trial stays inside the box and lands ~10^4 sigma off the peak: rejected by the
    # likelihood -- rejections by the prior do not count towards max_tries)
    eng.set_proposal_cov(np.eye(d) * 1e-4)
    eng.set_state(np.full((G * gs, d), 0.5))
    eng.step(40)
    eng.accumulate_moments()
    eng.request_moments()
    with pytest.raises(E.EngineError, match="stuck"):
        eng.fetch_moments()
    eng.close()


def test_read_out_reports_a_function_targets_error_flag():
    """A device-function target that returns NaN inside the support for one walker: the flag rides
    in the other half of the word behind the accept counter and the fetch raises the target's
    error, without any synchronisation before it.  Before the walker is flagged the same engine
    fetches clean, and so does a twin with a built-in target (no flag word of a function: that
    half is written as zero)."""
    state = {"nan": False}

    def f(p):
        ll = -((p - 0.5) ** 2).sum(1) * 50.0
        if state["nan"]:
            ll[70] = float("nan")
        return ll

    d, W = 2, 128
    x0 = np.random.default_rng(0).uniform(0.3, 0.7, (W, d))
    eng = E.Engine(d, W, group_size=64, device=0, seed=2)
    eng.set_prior(np.zeros(d, np.int32), np.zeros(d), np.ones(d))
    eng.set_target_function(f)
    eng.set_proposal_cov(1e-6 * np.eye(d))      # narrow: every trial stays inside the support
    eng.set_state(x0)
    twin = E.Engine(d, W, group_size=64, device=0, seed=2)
    twin.set_prior(np.zeros(d, np.int32), np.zeros(d), np.ones(d))
    twin.set_target_gaussian_mixture([np.full(d, 0.5)], [np.eye(d) * 0.01])
    twin.set_proposal_cov(1e-6 * np.eye(d))
    twin.set_state(x0)
    for e in (eng, twin):                        # nothing flagged: both fetch clean
        e.step(2)
        e.accumulate_moments()
        e.request_moments()
        n, gsum, S, c = e.fetch_moments()
        assert n == 1 and c["steps"] == 2 and np.all(np.isfinite(gsum)) and np.all(np.isfinite(S))
    state["nan"] = True
    eng.step(2)
    eng.accumulate_moments()
    eng.request_moments()
    with pytest.raises(E.TargetError, match=r"walker 70\b") as ei:
        eng.fetch_moments()
    assert ei.value.code == E.ERR_TARGET
    twin.step(2)
    twin.accumulate_moments()
    twin.request_moments()
    n, _, _, c = twin.fetch_moments()
    assert n == 1 and c["steps"] == 4
    eng.close()
    twin.close()
