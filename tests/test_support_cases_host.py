"""The conditions on the cases of tests/support_cases.py, on the ORACLE ALONE (CPU): a case is of
use to tests/test_gpu_support_walls.py only if its chain meets the walls all the time and still
moves.  And loglike_ref, the long-double reference of the evaluator comparison, pinned to a
50-digit restatement."""
import numpy as np
import pytest

from oracle import cbind as O
from tests import support_cases as S

SHARE_BAND = (0.15, 0.8)     # trials that left the support, of all trials
MIN_ACCEPTANCE = 0.1


def _host_cases():
    """One oracle run per distinct problem: the GPU cases that differ only in the ensemble's
    layout on the device share theirs."""
    seen, out = set(), []
    for c in S.CASES:
        key = (c.d, c.scale, c.K, c.variant if c.variant != "duo" else None, c.W)
        if key not in seen:
            seen.add(key)
            out.append(c)
    return out


def oracle_alone(c, dragging=True):
    """Problem and state of a case with the oracle's OWN constants (numpy recipe, derived=None)."""
    kinds, a, b, periodic, blocking, means, covs, x0 = S.case_problem(c)
    if blocking is not None and not dragging:
        blocking = (blocking[0], blocking[1], -1, 0)
    scratch = "scratch" in (c.variant or "")
    kw = {}
    if blocking is not None:
        blocks, over, last_slow, n_drag = blocking
        kw = dict(blocks=blocks, oversampling=over, drag_last_slow=last_slow, drag_steps=n_drag)
        T = O.blocked_transform(covs[0], blocks, 2.4)
    else:
        T = O.proposal_transform(covs[0], 2.4)
    prob = O.Problem(c.d, kinds.tolist(), a.tolist(), b.tolist(), periodic=periodic, means=means,
                     covs=covs, T=T, group_size=c.gs, seed=3, derived=None,
                     incremental=not scratch, **kw)
    return prob, O.State(prob, x0), kinds, a, b


@pytest.mark.parametrize("c", _host_cases(), ids=S.case_id)
def test_the_case_meets_the_walls_and_still_moves(c):
    # (a dragging step whose slow trial leaves the support is not counted in prior_rej,
    # mcmc.py:590-592: the share is taken with Metropolis steps on the same blocks, and the
    # dragging chain itself must move and stay inside, see below)
    drag = c.variant in ("drag", "scratch drag")
    prob, st, kinds, a, b = oracle_alone(c, dragging=False)
    L = prob.refresh_every // 40
    st.run(40 * L + 17, n_threads=8)     # across one refresh
    out = 0
    steps = 200
    for _ in range(steps):
        before = st.prior_rej.copy()
        st.run(1, n_threads=8)
        out += int(np.sum(st.prior_rej > before))
    share = out / (steps * c.W)
    acceptance = st.n_accept.sum() / (c.W * st.step)
    print(f"{S.case_id(c)}: share {share:.3f} acceptance {acceptance:.3f}")
    assert SHARE_BAND[0] <= share <= SHARE_BAND[1], share
    assert acceptance >= MIN_ACCEPTANCE, acceptance
    assert S.inside(st.x, a, b, kinds)
    assert np.isfinite(st.logpost).all()
    if drag:
        prob, st, kinds, a, b = oracle_alone(c)
        st.run(prob.refresh_every + 17, n_threads=8)
        assert st.n_accept.sum() / (c.W * st.step) >= MIN_ACCEPTANCE
        assert S.inside(st.x, a, b, kinds)
        # walkers within 0.01 of the width (a third of a sigma) of a wall
        near = S.near_wall(st.x, a, b, kinds)
        print(f"{S.case_id(c)}: dragging acceptance {st.n_accept.sum() / (c.W * st.step):.3f}, "
              f"near a wall {near.mean():.3f}")
        assert near.mean() > 0.15


def test_wall_list_covers_every_lane_class_and_the_last_row():
    for c in S.CASES:
        kinds, a, b, periodic, blocking = S.case_setup(c)
        walls = S.wall_list(c.d, kinds, periodic)
        assert len(walls) >= min(4, c.d), (S.case_id(c), walls)
        assert c.d - 1 in walls
        if c.d >= 5:
            assert {i % 4 for i in walls} == {0, 1, 2, 3}


def test_scales_are_what_they_are_named_for():
    f32 = np.float32
    a, b = S.box("offset", 4)
    with np.errstate(over="ignore"):
        lo = np.nextafter(a.astype(f32), f32(np.inf))    # rounded inward: the copies cross
        hi = np.nextafter(b.astype(f32), f32(-np.inf))
        assert np.all(lo > hi)
        a, b = S.box("beyond float", 4)
        assert np.all(np.isinf(a.astype(f32))) and np.all(np.isinf(b.astype(f32)))
        a, b = S.box("below float", 4)
        assert np.all(a.astype(f32) == 0) and np.all(b.astype(f32) == 0)
    a, b = S.box("negative", 12)
    assert np.all(b < 0) and len(set(zip(a, b))) == 6
    a, b = S.box("mixed", 10)
    assert len(set(zip(a[:5], b[:5]))) == 5 and (a[5], b[5]) == (a[0], b[0])
    for name in S.ONE_BOX:
        a, b = S.box(name, 3)
        assert np.all(a == 0) and len(set(b)) == 1


# ------------------------------------------------------------------ the long-double reference
@pytest.mark.parametrize("scale", S.EVAL_SCALES)
@pytest.mark.parametrize("d,K", [(5, 1), (5, 3), (30, 1)])
def test_loglike_ref_against_50_digits(d, K, scale):
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 50
    a, b, means, covs, pts = S.eval_problem(d, K, scale)
    pts = np.concatenate([pts[:6], pts[-2:]])
    ref = S.loglike_ref(pts, means, covs)
    want = []
    for x in pts:
        terms = []
        for k in range(K):
            # (mp.cholesky tests its pivots against an ABSOLUTE epsilon: no use at 1e-100)
            C = [[mp.mpf(float(v)) for v in row] for row in covs[k]]
            L = mp.zeros(d)
            for j in range(d):
                L[j, j] = mp.sqrt(C[j][j] - sum(L[j, q] ** 2 for q in range(j)))
                for i in range(j + 1, d):
                    L[i, j] = (C[i][j] - sum(L[i, q] * L[j, q] for q in range(j))) / L[j, j]
            y = []
            for i in range(d):
                r = mp.mpf(float(x[i])) - mp.mpf(float(means[k][i]))
                y.append((r - sum(L[i, q] * y[q] for q in range(i))) / L[i, i])
            chi2 = sum(v * v for v in y)
            logdet = 2 * sum(mp.log(L[i, i]) for i in range(d))
            terms.append(-mp.log(K) - (chi2 + d * mp.log(2 * mp.pi) + logdet) / 2)
        top = max(terms)
        want.append(top + mp.log(sum(mp.exp(t - top) for t in terms)))
    # the reference has to be MORE precise than the float64 it judges: an extended long double
    # (where np.longdouble is float64 this fails rather than pin a double to itself)
    eps = float(np.finfo(np.longdouble).eps)
    assert eps < 2e-19
    worst = 0.0
    for got, w in zip(ref, want):
        err = abs(mp.mpf(float(got)) + mp.mpf(float(got - np.longdouble(float(got)))) - w)
        worst = max(worst, float(err / (eps * max(1.0, abs(float(w))))))
        # a backward-stable solve in long double: cond(L) (about 3 here) d eps relative to chi2;
        # at d = 30 that is 1.3e-17, a ninth of float64's eps
        assert err <= 4 * d * eps * max(1.0, abs(float(w)))
    print(f"d={d} K={K} {scale}: worst error {worst:.2f} eps_longdouble max(1, |loglike|)")


@pytest.mark.parametrize("scale", S.EVAL_SCALES)
@pytest.mark.parametrize("d,K", S.EVAL_SHAPES)
def test_the_numpy_recipe_is_close_to_the_reference(d, K, scale):
    """The tolerance of the device comparison is 4 x this error: it has to be a rounding error."""
    a, b, means, covs, pts = S.eval_problem(d, K, scale)
    ref = S.loglike_ref(pts, means, covs)
    got = S.loglike_numpy(pts, means, covs)
    rel = np.max(S.relative_error(got, ref))
    print(f"d={d} K={K} {scale}: numpy recipe {rel:.3g} relative")
    # a backward-stable Cholesky and solve (cond(L) is about 3 here): a few d eps.  Eight times the
    # summation-order floor of the device comparison: 1.2e-14 at d = 5, 9.6e-14 at d = 100
    assert rel <= 8 * (d + 8) * 2.0 ** -53


def test_the_librarys_rule_sends_every_incremental_case_to_its_kernel_family():
    """mcmc_hip_incremental_choice (a pure function of the library, no device) on the shape of
    every incremental case: the family the GPU file then finds in last_step_kernel()."""
    from cobaya_amd import engine as E
    want = {"step_inc_mix_kernel": E.INC_MIX, "step_duo_mix_kernel": E.INC_DUO_MIX,
            "drag_inc_kernel": E.INC_DRAG, "step_inc_regs_kernel": E.INC_ANY,
            "step_inc_any_kernel": E.INC_ANY}
    for c in S.CASES:
        v = c.variant or ""
        if "scratch" in v:
            continue
        kinds, a, b, per, blocking = S.case_setup(c)
        one_box = bool(np.all(kinds == 0) and len(set(a)) == 1 and len(set(b)) == 1)
        ch = E.incremental_choice(
            c.d, c.K, n_periodic=0 if per is None else int(per.sum()),
            n_drag=blocking[3] if blocking and blocking[2] >= 0 else 0, n_walkers=c.W,
            basis_group_size=c.gs, any_normal=bool(kinds.any()), one_box=one_box,
            box_lo_is_zero=bool(one_box and a[0] == 0),
            has_1d_block=bool(blocking and min(len(x) for x in blocking[0]) == 1),
            emit=v == "emit", duo=1 if v == "duo" else -1)
        if "two lanes" in c.path:
            family = E.INC_DUO_ONE
        elif "emit" in c.path:
            family = E.INC_STEP_EMIT
        else:
            family = next((f for word, f in want.items() if c.path[0].startswith(word)), E.INC_STEP)
        assert ch["family"] == family, (S.case_id(c), ch)
        assert ch["carry_periodic"] == int(v == "periodic"), S.case_id(c)
        assert (c.scale in S.ONE_BOX) == (one_box and a[0] == 0), S.case_id(c)
