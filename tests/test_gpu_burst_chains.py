"""The variate burst of the one-mode two-lane step kernel (incremental_duo.hip `step_inc_duo_kernel`, det_math.h
`OctetRng`): a lane half draws the four (r, accept estimate) variates of its two Philox blocks as one straight-line
burst of interleaved chains, per octet of the global step index.  Only the order across the variates differs from
`PairRng::draw<true>`, so every state stays the oracle's bit for bit: for every dq from 1 to 8 with and without a padded
row, for launches that begin at every step offset of an octet, for launches of 1, 7, 8, 9 and 17 steps, of one LDS chunk
less and plus a step and of two chunks plus one (an octet then straddles a chunk boundary), at a temperature other
than one, through a burn-in that ends inside an octet, and across the one path whose code moved: a radial uniform in
its lowest bin (kr == 0), which the burst leaves to a redraw behind its stores, as the first and as the last variate
of a lane half, and an accept uniform in its lowest bin (ka == 0), whose estimate stays a NaN."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from cobaya_amd import engine as E  # noqa: E402
from oracle import cbind as O  # noqa: E402
from tests.test_gpu_parity import assert_bit_equal, compare_state, make_pair, random_target  # noqa: E402

# every dq = ceil(d / 4) from 1 to 8, with a padded row (d % 4 != 0) and without
DIMS = [2, 3, 4, 5, 8, 11, 12, 15, 16, 17, 20, 23, 24, 27, 28, 29, 30, 31, 32]


def test_the_dimensions_cover_every_dq_with_and_without_a_padded_row():
    for dq in range(1, 9):
        mine = [d for d in DIMS if (d + 3) // 4 == dq]
        assert any(d % 4 == 0 for d in mine) and any(d % 4 != 0 for d in mine), (dq, mine)


def duo1_chunk(dq):
    """columns of one LDS chunk of step_inc_duo_kernel (incremental_duo.hip: duo1_chunk)"""
    return min(64, ((80 * 1024 - 16896 - 2048) // (2 * 64 * dq)) & ~3)


def launches(dq):
    """The launch lengths of a case, and the step offsets inside an octet their launches begin at"""
    c = duo1_chunk(dq)
    lengths = [1, 7, 8, 9, 17, c - 1, c + 1, 2 * c + 1] + [9] * 7
    starts = np.cumsum([0] + lengths[:-1])
    return lengths, sorted({int(s) % 8 for s in starts})


def test_the_launches_begin_at_every_offset_of_an_octet():
    for dq in range(1, 9):
        lengths, offsets = launches(dq)
        assert offsets == list(range(8)), (dq, offsets)
        c = duo1_chunk(dq)
        assert {1, 7, 8, 9, 17, c - 1, c + 1, 2 * c + 1} <= set(lengths)
    assert [duo1_chunk(dq) for dq in range(1, 9)] == [64] * 7 + [60]


def _compare(eng, st):
    compare_state(eng, st)   # x, logpost, logprior, loglike, weight
    s = eng.get_full_state()
    assert_bit_equal(s["y"], st.y, "carried whitened residual")
    assert np.array_equal(s["prior_rej"], st.prior_rej)
    assert np.array_equal(s["n_accept"], st.n_accept)
    assert np.array_equal(s["burn_left"], st.burn_left)


def _run(eng, st, lengths, walker0=0):
    _compare(eng, st)
    for n in lengths:
        eng.step(n)
        eng.sync()
        st.run(n, walker0=walker0, n_threads=8)
        _compare(eng, st)
        assert "two lanes" in eng.last_step_kernel(), eng.last_step_kernel()
    c = eng.counters()
    assert c["steps"] == st.step and c["accepted"] == int(st.n_accept.sum())


@pytest.mark.parametrize("d", DIMS)
def test_every_dq_every_octet_offset_and_chunk_boundary_bit_exact(d, monkeypatch):
    monkeypatch.setenv("MCMC_HIP_DUO", "1")
    eng, prob, st = make_pair(d, 256, 128, incremental=True, rng=np.random.default_rng(2500 + d))
    _run(eng, st, launches((d + 3) // 4)[0])
    eng.close()


def test_a_temperature_other_than_one_bit_exact(monkeypatch):
    monkeypatch.setenv("MCMC_HIP_DUO", "1")
    eng, prob, st = make_pair(30, 256, 128, incremental=True, T=1.7, rng=np.random.default_rng(2541))
    _run(eng, st, launches(8)[0][:7])
    eng.close()


def test_a_burn_in_that_ends_inside_an_octet_bit_exact(monkeypatch):
    """burn_in = 5 accepted steps: at an acceptance near 0.3 the chains leave their burn-in around step 17, each at
    a step of its own -- the first launches end while chains are still burning"""
    monkeypatch.setenv("MCMC_HIP_DUO", "1")
    eng, prob, st = make_pair(30, 256, 128, incremental=True, burn_in=5, rng=np.random.default_rng(2542))
    lengths = launches(8)[0][:7]
    burning = []
    _compare(eng, st)
    for n in lengths:
        eng.step(n)
        eng.sync()
        st.run(n, n_threads=8)
        _compare(eng, st)
        burning.append(int((st.burn_left > 0).sum()))
    # chains left their burn-in inside the launches, at steps that are no multiple of eight among them
    assert burning[0] == 256 and burning[-1] < 256 and len(set(burning)) > 2, burning
    eng.close()


# ---------------------------------------------------------------- the lowest bins
# The one path whose code moved.  A radial uniform in its lowest bin (kr == 0, 2^-24 per variate) is left by the burst
# with the r of the bin's upper edge, E = neg_log_short(1, 25) = 25 ln 2, and redrawn behind the stores with the tail
# (pair_tail: E > 24 ln 2 from a Philox block of its own).  A kernel that never redraws differs from the oracle in r at
# that step alone -- by 2 % or so --, which a REJECTED move does not show: the cases therefore take (walker, step) hits
# at which the oracle ACCEPTS, so that x, y and the carried log-likelihood of that walker hold r itself.  The proposal is
# a tenth of the target's width, where a move of |r| = 6 is accepted about every other time.
SEED = 7
LOW_D, LOW_W = 30, 128


def _low_hits(residue):
    """(walker, step) of seed 7 with kr == 0 and step % 4 == residue (the variate's place among the four of its lane
    half), in the oracle's order over windows of 2^13 walkers x 2^10 steps (about one hit in two windows)"""
    for g0 in range(0, 1 << 20, 1 << 13):
        s0 = 0
        while s0 < 1024:
            hit = O.find_short_tail(SEED, g0, 1 << 13, s0, 1024 - s0, 0)
            if hit is None:
                break
            if hit[1] % 4 == residue and hit[1] >= 8:
                yield hit
            s0 = hit[1] + 1


def _low_pair(off):
    """engine and oracle problem of 128 walkers from walker id `off` on, d = 30, proposal = 0.01 x the target's covariance"""
    d = LOW_D
    rng = np.random.default_rng(2550)
    means, covs = random_target(d, 1, rng)
    eng = E.Engine(d, LOW_W, group_size=LOW_W, seed=SEED, walker_offset=off, incremental=True)
    eng.set_prior([0] * d, [0.0] * d, [1.0] * d)
    eng.set_target_gaussian_mixture(means, covs)
    eng.set_proposal_cov(covs[0] * 0.01)
    prob = O.Problem(d, [0] * d, [0.0] * d, [1.0] * d, means=means, covs=covs, T=eng.get_proposal_transform(),
                     group_size=LOW_W, seed=SEED, derived=eng.derived_constants(), incremental=True)
    x0 = np.clip(means[0] + rng.normal(size=(LOW_W, d)) * np.sqrt(np.diag(covs[0])), 1e-3, 1 - 1e-3)
    eng.set_state(x0)
    return eng, prob, x0


@pytest.mark.parametrize("residue", [0, 3], ids=["kr-first-variate", "kr-last-variate"])
def test_a_radial_uniform_in_its_lowest_bin_is_redrawn_behind_the_burst(residue, monkeypatch):
    """The first hit at which the oracle accepts the move (the first and the third candidate, found on the oracle
    alone): the walker's x after that step is x + r v with the redrawn r, bit for bit, on the device too."""
    monkeypatch.setenv("MCMC_HIP_DUO", "1")
    found = None
    for n, (gid, step) in enumerate(_low_hits(residue)):
        assert n < 8, "no accepted lowest-bin step among eight candidates"
        off, w = gid - gid % LOW_W, gid % LOW_W
        eng, prob, x0 = _low_pair(off)
        probe = O.State(prob, x0)
        probe.run(step, walker0=off, n_threads=8)
        before, x_before = int(probe.n_accept[w]), probe.x[w].copy()
        probe.run(1, walker0=off, n_threads=8)
        if int(probe.n_accept[w]) == before + 1:
            assert np.any(probe.x[w] != x_before)
            found = (gid, step, off, w, eng, prob, x0, x_before, probe.x[w].copy())
            break
        eng.close()
    gid, step, off, w, eng, prob, x0, x_before, x_after = found
    print(f"kr == 0 at walker {gid}, step {step} (candidate {n + 1}): accepted by the oracle")
    assert step % 4 == residue and step > 3
    r, _ = O.pair_variates(SEED, gid, step)
    e_edge = 25 * np.log(2.0)                          # the bin's upper edge: what the burst itself leaves
    expo = abs(r) > 24 * np.log(2.0)                   # |r| = E on the exponential branch, sqrt(2 E) on the other
    assert (abs(r) if expo else r * r / 2.0) > 24 * np.log(2.0)          # the redrawn tail
    # the accepted move is r times the column, so the un-redrawn r would land the walker elsewhere, far above an ulp
    r_edge = e_edge if expo else np.sqrt(2.0 * e_edge)
    assert np.abs(x_after - x_before).max() * abs(abs(r) - r_edge) / abs(r) > 1e-6
    st = O.State(prob, x0)
    _run(eng, st, (step - 3, 8), walker0=off)          # the second launch begins three steps before the step and crosses it
    eng.close()


def test_an_accept_uniform_in_its_lowest_bin_keeps_its_nan_estimate(monkeypatch):
    """ka == 0: the burst stages a NaN estimate and the step's exact branch draws the tail, as before (the hit of
    tests/test_gpu_lazy_accept.py, from start points of its own)"""
    monkeypatch.setenv("MCMC_HIP_DUO", "1")
    hit = O.find_short_tail(SEED, 0, 1 << 17, 0, 4096, 1)
    assert hit is not None
    gid, step = hit
    assert step > 3
    assert O.pair_variates(SEED, gid, step)[1] > 28 * np.log(2.0)
    off = gid - gid % 128
    eng, prob, st = make_pair(4, 128, 128, seed=SEED, incremental=True, walker_offset=off,
                              rng=np.random.default_rng(2551))
    _run(eng, st, (step - 3, 8), walker0=off)
    eng.close()
