"""The specification FAR OUT, on the oracle alone (CPU): what tests/test_gpu_far_steps.py compares
the kernels with at step indices around 2^31, 2^32 and 2^33.

* the variates at far steps against a restatement on the Philox block: the counter words are
  (step mod 2^32, step div 2^32), on the paired stream (P mod 2^32, P div 2^32) with P = step div 2;
* the case table has power: at every boundary of every case the oracle's end state differs from
  what a kernel with a narrowed index would reach (tests/far_steps.py: `narrowed`), or the bit
  comparison could not see that kernel;
* acceptance stays sane out there;
* the cycle rule: the cycle index is kept modulo 2^32, so a run from step L 2^32 draws the bases of
  cycle 0 again (with other variates: the step counter has 64 bits);
* a sampler state file whose `step` lies above 2^32 resumes like a teleported engine."""
import shutil

import numpy as np
import pytest

from oracle import cbind as O
from tests import far_steps as F

SEED = 3
FAR_STEPS = (F.P32 - 1, F.P32, F.P33 - 2, F.P33 - 1, F.P33, F.P33 + 1)
ACCEPTANCE = (0.05, 0.9)


# ------------------------------------------------------------------ the variates
@pytest.mark.parametrize("seed", [SEED, (0x9E3779B9 << 32) | 7])
def test_paired_variates_at_far_steps_use_both_counter_words(seed):
    checked = 0
    for S in FAR_STEPS + (F.CONTROL, 30 * F.P32 + 5):
        for gid in (0, 1, 77, 65535, 4_000_000_000):
            want = F.paired_variates(O, seed, gid, S)
            if want is None:       # (a lowest bin: one in 2^24, redrawn from a block of its own)
                continue
            assert O.pair_variates(seed, gid, S) == want, (S, gid)
            checked += 1
    assert checked >= 38
    # a dropped high word is another variate (so the comparisons can tell)
    for S in (F.P33, F.P33 + 1):
        assert O.pair_variates(seed, 5, S) != O.pair_variates(seed, 5, S - F.P33)


def _flat_problem(group_size=64):
    """d = 1, the `one` likelihood, T = 1 and a wide box: every trial is accepted and, from x = 0,
    lands on fma(r, +-1, 0) = +-r exactly."""
    return O.Problem(1, [0], [-1000.0], [1000.0], T=np.ones((1, 1)), group_size=group_size, seed=SEED)


def test_unpaired_variates_at_far_steps_use_both_counter_words():
    """The un-paired stream has no export of its own: the radial variate is read off a flat
    one-parameter run, |x'| = |r| (one parameter: the variates of a one-parameter block)."""
    W = 128
    prob = _flat_problem()
    for S in FAR_STEPS + (F.CONTROL,):
        st = O.State(prob, np.zeros((W, 1)))
        st.step = S
        st.run(1, n_threads=2)
        assert np.all(st.n_accept == 1)
        want = np.array([abs(F.unpaired_variates(O, SEED, gid, S, oned=True)[0]) for gid in range(W)])
        assert np.array_equal(np.abs(st.x[:, 0]), want), S
        if S >= F.P32:    # ... and not the variate of the low word alone
            low = np.array([abs(F.unpaired_variates(O, SEED, gid, S & F.M32, oned=True)[0]) for gid in range(W)])
            assert not np.any(low == want)


# ------------------------------------------------------------------ the cases
def oracle_alone(c):
    """Problem and start of a case with the oracle's OWN constants (numpy recipe)."""
    kinds, a, b, periodic, blocking, means, covs, x0 = F.case_problem(c)
    kw = {}
    if blocking is not None:
        blocks, over, last_slow, n_drag = blocking
        kw = dict(blocks=blocks, oversampling=over, drag_last_slow=last_slow, drag_steps=n_drag)
        T = O.blocked_transform(covs[0], blocks, 2.4)
    else:
        T = O.proposal_transform(covs[0], 2.4)
    own = c.variant == "own"
    prob = O.Problem(c.d, kinds.tolist(), a.tolist(), b.tolist(), periodic=periodic, means=means,
                     covs=covs, T=T, group_size=1 if own else c.bgs, seed=SEED, incremental=c.inc,
                     carry_modes=True, carry_periodic=True, **kw)   # (where they apply: Problem)
    return prob, x0


def _run(prob, x0, S0, n, model=None):
    st = O.State(prob, x0)
    if prob.c.carry_modes:     # (formed at step 0 or a refresh otherwise: tests/far_steps.py, teleport)
        st.anchor_modes()
    if model is None:
        st.step = S0
        st.run(n, n_threads=4)
    else:
        F.run_narrowed(st, S0, n, model)
    return st


def test_the_table_names_every_family_once_and_boundaries_follow_the_rule():
    assert len({c.name for c in F.CASES}) == len(F.CASES) >= 27
    for c in F.CASES:
        L, nd, Lf = F.cycle_lengths(c)
        B = F.boundaries(c)
        assert F.P31 in B and F.P32 in B and (F.P33 in B) == (c.inc or L == 2 or L == 4)
        assert L * F.P31 in B and L * F.P32 in B
        assert 128 <= c.W <= 256 and c.gs == 64
        if nd:
            assert -(-F.P32 // nd) in B and any(b * nd >= Lf * F.P32 > (b - 1) * nd for b in B)
    c = F.BY_NAME["scratch-d8-blocked"]
    assert F.cycle_lengths(c) == (13, 0, 0)             # a cycle that is not d steps long
    assert F.cycle_lengths(F.BY_NAME["scratch-d40-blocked"])[0] == 60
    assert F.cycle_lengths(F.BY_NAME["scratch-d6-drag"]) == (2, 3, 4)
    # d = 205: y is refreshed at step 2^33 + 8, inside the launch [2^33 - 13, 2^33 + 17)
    assert (F.P33 + 8) % (40 * F.HUGE_DIMS[1]) == 0 and F.LAUNCHES[0] - F.BEFORE <= 8 < sum(F.LAUNCHES[:2]) - F.BEFORE


@pytest.mark.parametrize("c", F.CASES, ids=F.case_id)
def test_the_case_has_power_and_moves_at_every_boundary(c):
    """At every boundary: the chain moves (acceptance over the 55 steps in [0.05, 0.9]), and the
    end state differs from that of every narrowed index the window tells apart.  A boundary of
    dragging's fast counter alone (step * n_drag crosses 2^32 while step is below 2^31) moves no
    step index: there the fast CYCLE a 32-bit counter would name must be another one."""
    prob, x0 = oracle_alone(c)
    L, nd, Lf = F.cycle_lengths(c)
    n = sum(F.LAUNCHES)
    ends = {}
    for B in (F.CONTROL + F.BEFORE,) + tuple(F.boundaries(c)):
        S0 = B - F.BEFORE
        st = _run(prob, x0, S0, n)
        acc = st.n_accept.sum() / (c.W * n)
        assert ACCEPTANCE[0] <= acc <= ACCEPTANCE[1], (B, acc)
        assert np.isfinite(st.logpost).all()
        ends[B] = st.x.copy()
        if B < F.P31:
            if B != F.CONTROL + F.BEFORE:
                f = np.arange(S0 * nd, (S0 + n) * nd)
                assert nd and f.max() >= F.P32
                beyond = f[f >= F.P32]
                assert np.all((beyond & F.M32) // Lf != (beyond // Lf) & F.M32)
            continue
        told = 0
        for model in F.MODELS:
            for S in (S0, B):      # both passes: from B - 21, and from B itself
                m = n if S == S0 else F.ON_BOUNDARY
                if all(F.narrowed(S + k, model) == S + k for k in range(m)):
                    continue
                ref = ends[B] if S == S0 else _run(prob, x0, S, m).x
                bad = _run(prob, x0, S, m, model)
                assert not np.array_equal(bad.x, ref), (B, S, model)
                assert np.mean(np.any(bad.x != ref, axis=1)) > 0.5, (B, S, model)
                told += 1
        assert told >= 2, B
        if c.inc and B == F.P33:
            assert all(F.narrowed(B + 3, m) != B + 3 for m in ("low word", "pair low word"))
    # one start, different steps: all ends distinct (the step index is in every variate)
    keys = sorted(ends)
    for i, p in enumerate(keys):
        for q in keys[i + 1:]:
            assert not np.array_equal(ends[p], ends[q]), (p, q)


# ------------------------------------------------------------------ the cycle rule
def test_a_run_from_L_2_32_draws_the_bases_of_cycle_0():
    """the basis of (group, cycle) is keyed on cycle mod 2^32 -- after
    L 2^32 steps the sequence of bases repeats while the variates (64-bit step) do not.  d = 2,
    the `one` likelihood in a wide box: every trial is accepted, so x' - x = r v with the column v
    of the step; v must be column (step mod 2) of `basis_blocked(group, cycle mod 2^32)`."""
    d, W, gs = 2, 128, 64
    T = np.array([[1.0, 0.0], [0.25, 0.5]])
    prob = O.Problem(d, [0, 0], [-1000.0] * 2, [1000.0] * 2, T=T, group_size=gs, seed=SEED)
    for S0, cycles in ((2 * F.P32, (0, 1)), (2 * F.P32 - 2, (F.M32, 0)), (F.P32, (F.P31, F.P31 + 1))):
        st = O.State(prob, np.zeros((W, d)))
        st.step = S0
        for k in range(4):
            before = st.x.copy()
            S = st.step
            st.run(1, n_threads=2)
            assert (S // d) & F.M32 == cycles[k // 2]
            for g in range(W // gs):
                V, _ = prob.basis_blocked(g, cycles[k // 2])
                other, _ = prob.basis_blocked(g, cycles[k // 2] ^ 1)
                for w in range(g * gs, (g + 1) * gs):
                    r = F.unpaired_variates(O, SEED, w, S)[0]
                    v = (st.x[w] - before[w]) / r
                    np.testing.assert_allclose(v, V[k % d], rtol=1e-9, atol=1e-12)
                    assert not np.allclose(v, other[k % d], rtol=1e-3, atol=1e-6)
    # ... and the variates differ: the two runs are not the same run
    a = O.State(prob, np.zeros((W, d)))
    b = O.State(prob, np.zeros((W, d)))
    b.step = 2 * F.P32
    a.run(4)
    b.run(4)
    assert not np.array_equal(a.x, b.x)


# ------------------------------------------------------------------ the sampler's state file
def test_a_state_file_above_2_32_resumes_like_a_teleported_engine(tmp_path):
    """`step` travels through np.savez, np.load and int(): a float, an int32 or a signed 64-bit
    cast on that way would continue somewhere else."""
    from tests.test_sampler_on_oracle import make
    far = F.P33 + F.P32 + 12345          # beyond 2^33; its low word is not the step it was written at
    p, q, r = (str(tmp_path / n) for n in "pqr")
    first = make(p, 20000)
    first.run()
    state = p + ".1.state.npz"
    written = int(np.load(state)["step"])
    assert 0 < written < F.P31
    for other in (q, r):
        for ext in (".checkpoint", ".covmat", ".progress", ".1.state.npz", ".1.txt"):
            shutil.copy(p + ext, other + ext)
    z = dict(np.load(state, allow_pickle=False))
    assert z["step"].dtype == np.uint64
    z["step"] = np.uint64(far)
    np.savez(state, **z)

    moved = make(p, 40000, resume=True)              # the file says `far`
    assert int(moved.engine.get_full_state()["step"]) == far
    ported = make(q, 40000, resume=True)             # the file says `written`: teleported by hand
    fs = ported.engine.get_full_state()
    assert int(fs["step"]) == written
    fs["step"] = far
    ported.engine.set_full_state(fs)
    stayed = make(r, 40000, resume=True)
    for s in (moved, ported, stayed):
        s.run()
    a, b, c = (s.engine.get_full_state() for s in (moved, ported, stayed))
    n = int(a["step"]) - far
    assert 0 < n < 100000 and int(b["step"]) == far + n and int(c["step"]) > written
    assert a["step"].dtype == np.uint64
    for k in ("x", "logpost", "logprior", "loglike", "weight", "n_accept", "prior_rej", "y"):
        assert np.array_equal(a[k], b[k]), k
    assert not np.array_equal(a["x"], c["x"])        # ... and not like the run that stayed
    assert moved.engine.counters()["steps"] == far + n
    # the state written at the end holds the far step, exactly
    assert int(np.load(state)["step"]) == far + n
