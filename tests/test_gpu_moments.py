"""The moment kernels (group_moments_kernel / pool_moments_kernel of walker_kernels.hip, the
`_big` pair of walker_kernels_big.hip, the pair of huge_kernels.hip) against the oracle's
`orc_moments`, bit for bit and without stepping: states are set, accumulated twice (the `+=` of
the group sums and the carried pooled sums) and read back.  The shapes are the ones at which the
kernels change path: every compiled d <= 32, both sides of NPAIR + D <= 2 gs, the 64- and 16-deep
batches of the pool kernels with their remainders, the slice boundary of the big kernel (d = 79 /
80 at gs = 256) and the d > 128 pair."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from cobaya_amd import engine as E  # noqa: E402
from oracle import cbind as O  # noqa: E402


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _states(d, W, seed):
    """Two states in the +-50 box: columns at mixed scales (1e-3 ... 50), some entries exactly
    zero, some walkers repeated."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(2):
        scale = np.minimum(50.0, 10.0 ** rng.uniform(-3, 1.7, d))
        x = np.clip(rng.standard_normal((W, d)) * scale * 0.4, -49.0, 49.0)   # (inside the box)
        x[rng.random((W, d)) < 0.05] = 0.0
        rep = rng.integers(0, W, W // 8)
        x[rep] = x[rng.integers(0, W, W // 8)]
        out.append(x)
    shift = 0.3 * np.minimum(50.0, 10.0 ** rng.uniform(-3, 1.7, d)) * rng.standard_normal(d)
    shift[::5] = 0.0
    return out[0], out[1], shift


def _check(d, gs, G):
    W = G * gs
    eng = E.Engine(d, W, group_size=gs, device=0, seed=3, incremental=d > 128)
    eng.set_prior([0] * d, [-50.0] * d, [50.0] * d)
    eng.set_target_one()
    eng.set_proposal_cov(np.eye(d))
    x1, x2, shift = _states(d, W, 1000 * d + gs + G)
    eng.set_state(x1)
    eng.set_moment_shift(shift)
    eng.accumulate_moments()
    eng.set_state(x2)
    eng.accumulate_moments()
    n, g_gs, g_S = eng.read_moments()
    eng.close()
    gsum, S = O.moments(x1, gs, shift=shift)
    gsum, S = O.moments(x2, gs, shift=shift, group_sum=gsum, pooled=S)
    assert n == 2 and g_gs.shape == (G, d) and g_S.shape == (d, d)
    bad = np.argwhere(_bits(g_gs) != _bits(gsum))
    assert len(bad) == 0, f"group sums differ at {bad[:5].tolist()} ({len(bad)} of {gsum.size})"
    bad = np.argwhere(_bits(g_S) != _bits(S))
    assert len(bad) == 0, f"pooled second moments differ at {bad[:5].tolist()} ({len(bad)} of {S.size})"


EDGES_32 = (1, 2, 13, 14, 15, 20, 21, 22, 30, 31, 32)


@pytest.mark.parametrize("d,gs,G",
                         [(d, 64, 3) for d in range(1, 33)]
                         + [(d, gs, 3) for gs in (128, 256) for d in EDGES_32]
                         + [(6, 64, G) for G in (1, 15, 16, 17, 63, 64, 65, 81)])
def test_moments_lane_per_walker_kernels(d, gs, G):
    """d <= 32: group_moments_kernel is compiled per d, finds (i, j) of a pair from a float
    sqrtf and lays the sums out in two regimes (NPAIR + D <= 2 gs or not); pool_moments_kernel
    adds the groups in batches of 64 and 16 and a remainder."""
    _check(d, gs, G)


@pytest.mark.parametrize("d,gs,G",
                         [(d, gs, 2) for d in (33, 34, 63, 64, 65, 79, 80, 81, 127, 128)
                          for gs in (64, 128, 256)]
                         + [(40, 64, G) for G in (15, 16, 17, 33)])
def test_moments_column_sweep_kernels(d, gs, G):
    """33 <= d <= 128: group_moments_big_kernel slices the pairs where they do not fit (gs = 256:
    no slicing at d = 79, two slices at d = 80)."""
    _check(d, gs, G)


@pytest.mark.parametrize("d,gs,G", [(d, gs, 17) for d in (129, 255, 256) for gs in (64, 256)])
def test_moments_above_128_parameters(d, gs, G):
    _check(d, gs, G)
