"""The column chunks of the incremental step kernels arrive by LDS-DMA, issued where the compiler does not
count it (incremental_common.h: stage16_dma), so that the LDS reads of a step are waited for by their
count; the DMA is retired by hand in front of the barrier that publishes a chunk.  A chunk read before it
has landed, or a pair consumed before its read has returned, is a wrong operand -- a failed comparison
here, not a fault.  Launches of one chunk - 1, one chunk, one chunk + 1 and two chunks + 1 steps, each
starting inside an octet of steps, and a call across the refresh of y at 40 d steps (its second launch
refreshes y in the kernel before its first chunk is staged): x, y, logpost, loglike, weight, prior_rej and
n_accept bit for bit the oracle's."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from cobaya_amd import engine as E  # noqa: E402
from oracle import cbind as O  # noqa: E402
from tests.test_gpu_parity import assert_bit_equal, compare_state, make_pair  # noqa: E402


def duo1_chunk(dq):   # incremental_duo.hip: duo1_chunk
    return min(((80 * 1024 - 16896 - 2048) // (2 * 64 * dq)) & ~3, 64)


def duo_chunk_mix(dq, km):   # incremental_duo.hip: duo_chunk_mix (x in registers: two modes up to d = 32)
    c = (((80 * 1024 - 16896 - 2560 - 2048) // 16) // ((1 + km) * 4 * dq)) & ~3
    return max(4, min(c, 64))


def inc_chunk(dq):   # incremental_common.h: inc_chunk (no periodic parameter, no carried log-prior)
    c = ((2048 if dq >= 14 else 896) // (4 * dq)) & ~3
    return max(4, min(c, 64))


def test_the_chunk_lengths_are_the_kernels():
    """The formulas above restate constexpr functions of the kernels: their text is looked up in the sources, so that
    a changed chunk length fails here instead of moving the launches below off the chunk boundaries unnoticed."""
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cobaya_amd", "csrc")
    with open(os.path.join(csrc, "incremental_duo.hip")) as f:
        duo = f.read()
    with open(os.path.join(csrc, "incremental_common.h")) as f:
        common = f.read()
    assert "int c = ((80 * 1024 - 16896 - 2048) / (2 * 64 * dq)) & ~3;\n    return c > 64 ? 64 : c;" in duo
    assert ("const int avail = 80 * 1024 - 16896 - 2560 - 2048 - (duo_x_in_lds(km, dq) ? dq * 4096 : 0);\n"
            "    int c = ((avail / 16) / ((1 + km) * 4 * dq)) & ~3;\n    return c < 4 ? 4 : (c > 64 ? 64 : c);") in duo
    assert ("int c = ((dq >= 14 ? 2048 : 896) / (4 * dq)) & ~3;\n    return c < 4 ? 4 : (c > 64 ? 64 : c);") in common
    assert duo1_chunk(8) == 60 and all(duo1_chunk(dq) == 64 for dq in range(1, 8))
    assert inc_chunk(8) == 28 and inc_chunk(25) == 20
    assert duo_chunk_mix(2, 2) == 64 and duo_chunk_mix(8, 2) == 36


def _check(eng, st):
    compare_state(eng, st)   # x, logpost, logprior, loglike, weight (and the carried mode log-densities)
    s = eng.get_full_state()
    assert_bit_equal(s["y"], st.y, "carried whitened residual")
    assert np.array_equal(s["prior_rej"], st.prior_rej)
    assert np.array_equal(s["n_accept"], st.n_accept)


def _chunk_launches(eng, st, d, C, kernel, not_kernel=None):
    def call(n):
        eng.step(n)
        eng.sync()
        st.run(n, n_threads=8)
        _check(eng, st)
        name = eng.last_step_kernel()
        assert kernel in name and (not_kernel is None or not_kernel not in name), name

    _check(eng, st)
    call(3)
    for n in (C - 1, C, C + 1, 2 * C + 1):
        if st.step % 8 == 0:
            call(1)
        assert st.step % 8 != 0
        call(n)
    # across the next refresh of y: the launch behind it runs one chunk + 1 steps
    R = 40 * d
    if st.step % 8 == 0:
        call(1)
    before = st.step // R
    call(R - st.step % R + C + 1)
    assert st.step // R == before + 1
    c = eng.counters()
    assert c["steps"] == st.step and c["accepted"] == int(st.n_accept.sum())


@pytest.mark.parametrize("d", [2, 5, 30, 32])
def test_two_lanes_one_mode_chunk_boundaries(d, monkeypatch):
    monkeypatch.setenv("MCMC_HIP_DUO", "1")
    monkeypatch.delenv("MCMC_HIP_ACCEPT_SLACK", raising=False)
    eng, prob, st = make_pair(d, 256, 128, incremental=True, rng=np.random.default_rng(9500 + d))
    _chunk_launches(eng, st, d, duo1_chunk((d + 3) // 4), "two lanes")
    eng.close()


def test_two_lanes_one_mode_always_exact_accept(monkeypatch):
    """MCMC_HIP_ACCEPT_SLACK=inf: the logarithm's table is read from LDS on every step, between the DMA in
    flight and the step's counted waits."""
    monkeypatch.setenv("MCMC_HIP_DUO", "1")
    monkeypatch.setenv("MCMC_HIP_ACCEPT_SLACK", "inf")
    d = 30
    eng, prob, st = make_pair(d, 256, 128, incremental=True, rng=np.random.default_rng(9530))
    _chunk_launches(eng, st, d, duo1_chunk(8), "two lanes")
    eng.close()


def test_two_lanes_one_mode_walkers_at_the_wall(monkeypatch):
    """Most trials of the walkers at the walls leave the box: the exact box test uses the step's pairs again."""
    monkeypatch.setenv("MCMC_HIP_DUO", "1")
    monkeypatch.delenv("MCMC_HIP_ACCEPT_SLACK", raising=False)
    d, W, gs = 30, 256, 128
    eng = E.Engine(d, W, group_size=gs, seed=3, incremental=True)
    eng.set_prior([0] * d, [0.0] * d, [1.0] * d)
    rng = np.random.default_rng(77 + d)
    mean = np.where(np.arange(d) % 2 == 0, 0.015, 0.985)
    A = rng.normal(size=(d, d))
    cov = (A @ A.T / d + np.eye(d)) * 0.02 ** 2
    eng.set_target_gaussian_mixture([mean], [cov])
    eng.set_proposal_cov(cov)
    prob = O.Problem(d, [0] * d, [0.0] * d, [1.0] * d, means=mean, covs=cov,
                     T=eng.get_proposal_transform(), group_size=gs, seed=3,
                     derived=eng.derived_constants(), incremental=True)
    x0 = np.clip(mean + rng.normal(size=(W, d)) * 0.01, 1e-4, 1 - 1e-4)
    eng.set_state(x0)
    st = O.State(prob, x0)
    _chunk_launches(eng, st, d, duo1_chunk(8), "two lanes")
    assert int(st.prior_rej.sum()) > 0
    eng.close()


@pytest.mark.parametrize("d", [30, 100])
def test_four_lanes_one_mode_chunk_boundaries(d):
    eng, prob, st = make_pair(d, 256, 128, incremental=True, rng=np.random.default_rng(9600 + d))
    _chunk_launches(eng, st, d, inc_chunk((d + 3) // 4), "step_inc_kernel", not_kernel="two lanes")
    eng.close()


@pytest.mark.parametrize("d", [5, 30])
def test_two_lanes_mixture_chunk_boundaries(d, monkeypatch):
    monkeypatch.setenv("MCMC_HIP_DUO", "1")
    K = 2
    w = np.random.default_rng(d).uniform(0.5, 1.5, K)
    eng, prob, st = make_pair(d, 256, 128, K=K, incremental=True, weights=(w / w.sum()).tolist(),
                              rng=np.random.default_rng(9700 + d))
    _chunk_launches(eng, st, d, duo_chunk_mix((d + 3) // 4, K), "step_duo_mix_kernel")
    eng.close()
