"""Targets pressed against the walls of the prior support, on boxes of every scale -- the inputs of
tests/test_support_cases_host.py (the conditions on the cases, on the oracle alone) and of
tests/test_gpu_support_walls.py (device against oracle, bit for bit) -- and a long-double
restatement of the Gaussian-mixture log-likelihood for the constants and the evaluator.  No GPU
needed.

`wall_problem` places everything relative to the box by an affine map, so that one builder serves
every scale: the mean of a uniform parameter sits at a + m (b - a) with m = 0.5 except on the wall
parameters {0, 1, 2, 3, d - 1} (all four lane classes of the four-lane kernels, and the last,
partly padded, row), where m alternates 0.015 / 0.985; sigma is about 0.02 (b - a), so a wall is
three quarters of a sigma away."""
from collections import namedtuple

import numpy as np

WALL_LOW, WALL_HIGH = 0.015, 0.985
PERIODIC_BOX = (0.42, 0.58)      # a periodic parameter: a few sigma wide around its mode
NORMAL_PRIOR = (0.5, 0.3)        # a normal-prior parameter: (loc, scale)


def _same(lo, hi):
    return lambda d: (np.full(d, float(lo)), np.full(d, float(hi)))


def _negative(d):
    i = np.arange(d)
    return -3.0 - (i % 3), -1.0 + 0.25 * (i % 2)


def _from_zero(d):
    return np.zeros(d), 1.0 + 0.25 * (np.arange(d) % 2)


_CLASSES = ((2450000.0, 2450000.1), None, (-1e39, 1e39), (1e-50, 3e-50), (0.0, 1.0))


def _mixed(d):
    na, nb = _negative(d)
    a, b = np.empty(d), np.empty(d)
    for i in range(d):
        box = _CLASSES[i % 5]
        a[i], b[i] = (na[i], nb[i]) if box is None else box
    return a, b


# one box starting at 0 ("unit", "tiny", "large": MODE 0 of step_inc_kernel) or bounds of their own
SCALES = {
    "unit": _same(0.0, 1.0),
    "offset": _same(2450000.0, 2450000.1),    # narrower than two single-precision ulps
    "tiny": _same(0.0, 5e-9),
    "large": _same(0.0, 3e6),
    "negative": _negative,
    "beyond float": _same(-1e39, 1e39),       # beyond FLT_MAX
    "below float": _same(1e-50, 3e-50),       # below the single-precision subnormals
    "mixed": _mixed,                          # every degenerate single-precision copy beside ordinary ones
    "from zero": _from_zero,                  # bounds of their own with the lower one at 0
}
ONE_BOX = ("unit", "tiny", "large")


def box(scale, d):
    a, b = SCALES[scale](d)
    return np.asarray(a, dtype=np.float64).copy(), np.asarray(b, dtype=np.float64).copy()


def wall_list(d, kinds=None, periodic=None):
    """The wall parameters: {0, 1, 2, 3, d - 1}, those that exist, are uniform and not periodic."""
    out = []
    for i in sorted({0, 1, 2, 3, d - 1} & set(range(d))):
        if kinds is not None and kinds[i]:
            continue
        if periodic is not None and periodic[i]:
            continue
        out.append(i)
    return out


def wall_problem(d, a, b, K=1, kinds=None, periodic=None, rng=None, W=128):
    """means (K, d), covs (K, d, d), x0 (W, d) of a mixture against the walls of [a, b].  For a
    normal-prior parameter (kinds[i] = 1) a[i], b[i] are the prior's location and scale: the mode
    sits at the location.  A periodic parameter keeps its mode at the middle of an interval a few
    sigma wide, so that the wraps of the seam fall into the same steps as the wall of the others."""
    rng = rng or np.random.default_rng(d)
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    kinds = np.zeros(d, int) if kinds is None else np.asarray(kinds)
    periodic = np.zeros(d, int) if periodic is None else np.asarray(periodic)
    normal, per = kinds == 1, periodic != 0
    w = np.where(normal, b, b - a)
    m = np.full(d, 0.5)
    for j, i in enumerate(wall_list(d, kinds, periodic)):
        m[i] = WALL_LOW if j % 2 == 0 else WALL_HIGH
    centre = np.where(normal, a, a + m * w)
    s = np.where(per, 0.3125, 0.02) * w
    means, covs = [], []
    for k in range(K):
        A = rng.normal(size=(d, d))
        covs.append((A @ A.T / d + np.eye(d)) * np.outer(s, s))
        means.append(centre + np.where(per, 0.0, 0.01 * k) * w)
    means, covs = np.array(means), np.array(covs)
    x0 = means[0] + rng.normal(size=(W, d)) * 0.01 * w
    uni = ~normal & ~per
    x0[:, uni] = np.minimum(np.maximum(x0[:, uni], (a + 1e-4 * w)[uni]), (b - 1e-4 * w)[uni])
    x0[:, per] = a[per] + (x0[:, per] - a[per]) % w[per]
    return means, covs, x0


def inside(x, a, b, kinds=None):
    """Every coordinate of a uniform parameter within its bounds."""
    uni = np.ones(len(a), bool) if kinds is None else np.asarray(kinds) == 0
    return bool(np.all((x[:, uni] >= np.asarray(a)[uni]) & (x[:, uni] <= np.asarray(b)[uni])))


def near_wall(x, a, b, kinds=None, periodic=None):
    """Walkers with a wall parameter within 0.01 of the box's width (a third of a sigma) of its
    wall."""
    near = np.zeros(len(x), bool)
    for j, i in enumerate(wall_list(len(a), kinds, periodic)):
        w = b[i] - a[i]
        near |= (x[:, i] - a[i] < 0.01 * w) if j % 2 == 0 else (b[i] - x[:, i] < 0.01 * w)
    return near


# ------------------------------------------------------------------ the cases of the GPU file
# family: what the case is about; path: the words last_step_kernel() must contain; dq, mode: the
# template arguments of step_inc_kernel it must report (None: not reported by that family)
Case = namedtuple("Case", "family d scale K W gs variant path dq mode")


def _c(family, d, scale, K=1, W=128, gs=64, variant=None, path=(), dq=None, mode=None):
    return Case(family, d, scale, K, W, gs, variant, tuple(path), dq, mode)


def _dq(d):
    return (d + 3) // 4


def _cases():
    out = []
    inc = "step_inc_kernel"
    for d in (5, 30, 48, 52, 124):                           # MODE 0: the high-word test
        for sc in ONE_BOX:
            out.append(_c("box", d, sc, path=[inc], dq=_dq(d), mode=0))
    for d in (6, 48, 52, 56, 88, 92, 100, 124):              # MODE 1
        for sc in ("negative",) + (("mixed", "offset") if d in (6, 52, 56, 88, 92) else ()):
            out.append(_c("bounds", d, sc, path=[inc], dq=_dq(d), mode=1))
    # the vector verdict where the copies do NOT cross ("mixed" and "offset" send every step to the
    # exact comparisons): a bound at 0 (-0 and the subnormals against the smallest float) and
    # infinite copies
    for d in (56, 88):
        for sc in ("from zero", "beyond float"):
            out.append(_c("bounds", d, sc, path=[inc], dq=_dq(d), mode=1))
    for d in (27, 52, 72, 76, 100, 116):                     # MODE 2: half the parameters normal
        for sc in ("negative", "mixed"):
            out.append(_c("normal", d, sc, variant="normal", path=[inc], dq=_dq(d), mode=2))
    for d in (6, 30, 40, 52, 64, 100):                       # periodic parameters
        for sc in ("negative", "mixed"):
            out.append(_c("periodic", d, sc, variant="periodic", path=[inc, "periodic"],
                          dq=_dq(d), mode=1))
    out.append(_c("emit", 30, "mixed", variant="emit", path=[inc, "emit"], dq=8, mode=1))
    out.append(_c("1-D block", 7, "mixed", variant="oned", path=[inc, "1-D blocks"], dq=2, mode=1))
    for d, K in ((30, 2), (52, 3), (44, 4)):                 # mixtures, four lanes
        for sc in ("unit", "large", "negative", "mixed"):
            out.append(_c("mixture", d, sc, K=K, path=["step_inc_mix_kernel"]))
    for d, K in ((30, 2), (44, 2), (26, 3)):                 # mixtures, two lanes
        for sc in ("unit", "mixed"):
            out.append(_c("duo mixture", d, sc, K=K, W=256, gs=128, variant="duo",
                          path=["step_duo_mix_kernel"]))
    for d in (5, 30):                                        # one mode, two lanes
        for sc in ("tiny", "large"):
            out.append(_c("duo", d, sc, W=256, gs=128, variant="duo", path=[inc, "two lanes"],
                          dq=_dq(d), mode=0))
    # (the general kernels report <dq, register planes> and <dq>)
    out.append(_c("general", 30, "mixed", K=8, path=["step_inc_regs_kernel<8, 8>"]))
    out.append(_c("general", 6, "mixed", K=24, path=["step_inc_any_kernel<2>"]))
    out.append(_c("general", 30, "mixed", K=3, variant="periodic7",
                  path=["step_inc_regs_kernel<8, 4, periodic>"]))
    for d in (9, 40):                                        # dragging, incremental
        for sc in ("unit", "mixed"):
            out.append(_c("dragging", d, sc, variant="drag", path=["drag_inc_kernel"]))
    for sc in ("unit", "mixed"):                             # from scratch: one kernel per case
        for d in (5, 30):
            out.append(_c("scratch", d, sc, variant="scratch", path=["::step_kernel<false, false>"]))
        # two waves per 64 walkers: whole workgroups of 256 walkers
        out.append(_c("scratch", 40, sc, W=256, gs=128, variant="scratch", path=["step_pair_kernel"]))
        out.append(_c("scratch", 40, sc, variant="scratch", path=["step_big_reg_kernel"]))
        # matrix cores: whole workgroups of 256 walkers; the column sweep serves the others
        out.append(_c("scratch", 100, sc, W=256, gs=64, variant="scratch", path=["step_mfma_kernel<false>"]))
        out.append(_c("scratch", 100, sc, variant="scratch", path=["step_big_reg_kernel"]))
        out.append(_c("scratch", 40, sc, K=2, variant="scratch", path=["step_general_kernel"]))
        out.append(_c("scratch", 40, sc, variant="scratch blocked", path=["step_general_kernel"]))
        out.append(_c("scratch", 40, sc, variant="scratch drag", path=["drag_general_kernel"]))
    return out


CASES = _cases()


def case_id(c):
    return "-".join(str(v) for v in (c.family, f"d{c.d}", c.scale.replace(" ", "_"), f"K{c.K}",
                                     c.variant or "plain", f"W{c.W}")).replace(" ", "_")


def case_setup(c):
    """kinds, a, b, periodic, blocking of a case; blocking = None or the arguments of set_blocking
    (blocks, oversampling, drag_last_slow, drag_steps)."""
    d, v = c.d, c.variant or ""
    a, b = box(c.scale, d)
    kinds = np.zeros(d, int)
    periodic = None
    blocking = None
    if v == "normal":
        # about half the parameters with normal priors; the wall parameters stay uniform
        rng = np.random.default_rng(7000 + d)
        kinds = (rng.random(d) < 0.55).astype(int)
        kinds[[0, 1, 2, 3, d - 1]] = 0
        a[kinds == 1], b[kinds == 1] = NORMAL_PRIOR
    elif v in ("periodic", "periodic7"):
        per = [7] if v == "periodic7" else ([4] if d == 6 else [5, d - 3])
        periodic = np.zeros(d, int)
        periodic[per] = 1
        a[per], b[per] = PERIODIC_BOX
    elif v == "oned":
        blocking = ([[3], [0], [1, 2, 4, 5, 6]], [1, 1, 3], -1, 0)
    elif v == "drag":
        blocks = ([[0, 1, 2], [3, 4], [5, 6, 7, 8]] if d == 9
                  else [list(range(12)), list(range(12, 40))])
        last_slow = 1 if d == 9 else 0
        blocking = (blocks, [1] * (last_slow + 1) + [2] * (len(blocks) - last_slow - 1), last_slow,
                    4 if d == 9 else 3)
    elif v == "scratch blocked":
        blocking = ([list(range(20)), list(range(20, 40))], [1, 2], -1, 0)
    elif v == "scratch drag":
        blocking = ([list(range(12)), list(range(12, 40))], [1, 2], 0, 3)
    return kinds, a, b, periodic, blocking


def case_problem(c):
    """Everything of a case but engine and oracle: kinds, a, b, periodic, blocking, means, covs, x0."""
    kinds, a, b, periodic, blocking = case_setup(c)
    means, covs, x0 = wall_problem(c.d, a, b, K=c.K, kinds=kinds, periodic=periodic,
                                   rng=np.random.default_rng(c.d), W=c.W)
    return kinds, a, b, periodic, blocking, means, covs, x0


def case_launches(c, L):
    """Launches that cross the refresh at 40 L steps (from scratch there is none: a cycle and a half)."""
    if "scratch" in (c.variant or ""):
        return (1, 6, L + 3, 9, L + 1)
    return (1, 6, L + 3, 40 * L - (L + 10) - 2, 9, L + 1)


# ------------------------------------------------------------------ long-double reference
def cholesky_ld(cov):
    c = np.asarray(cov, dtype=np.longdouble)
    d = len(c)
    L = np.zeros((d, d), dtype=np.longdouble)
    for j in range(d):
        s = c[j, j] - np.dot(L[j, :j], L[j, :j])
        assert s > 0
        L[j, j] = np.sqrt(s)
        for i in range(j + 1, d):
            L[i, j] = (c[i, j] - np.dot(L[i, :j], L[j, :j])) / L[j, j]
    return L


def solve_lower_ld(L, r):
    """y with L y = r, r (n, d) row-wise."""
    r = np.asarray(r, dtype=np.longdouble)
    y = np.zeros_like(r)
    for i in range(L.shape[0]):
        y[:, i] = (r[:, i] - y[:, :i] @ L[i, :i]) / L[i, i]
    return y


def inverse_lower_ld(L):
    d = len(L)
    return solve_lower_ld(L, np.eye(d, dtype=np.longdouble)).T


def cnorm_ld(L):
    """d log(2 pi) + log det(cov), what the engine reports as `cnorm`."""
    d = len(L)
    pi = 4 * np.arctan(np.longdouble(1))     # (np.pi is pi to float64 only)
    return d * np.log(2 * pi) + 2 * np.sum(np.log(np.diag(L)))


def loglike_ref(x, means, covs, weights=None):
    """log sum_k w_k N(x; mean_k, cov_k) in np.longdouble: Cholesky, triangular solve,
    log-determinant, log-sum-exp."""
    x = np.atleast_2d(np.asarray(x, dtype=np.longdouble))
    means = np.atleast_2d(np.asarray(means, dtype=np.longdouble))
    covs = np.asarray(covs, dtype=np.float64)
    covs = covs if covs.ndim == 3 else covs[None]
    K = len(means)
    wts = (np.full(K, np.longdouble(1) / K) if weights is None
           else np.asarray(weights, dtype=np.longdouble))
    terms = np.empty((K, len(x)), dtype=np.longdouble)
    for k in range(K):
        L = cholesky_ld(covs[k])
        y = solve_lower_ld(L, x - means[k])
        terms[k] = np.log(wts[k]) - (np.sum(y * y, axis=1) + cnorm_ld(L)) / 2
    top = terms.max(axis=0)
    return top + np.log(np.sum(np.exp(terms - top), axis=0))


def loglike_numpy(x, means, covs, weights=None):
    """The plain float64 recipe (np.linalg.cholesky, solve_triangular, scipy's logsumexp form):
    the reference's own arithmetic, whose error against loglike_ref sets the tolerance."""
    from scipy.linalg import solve_triangular
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    means = np.atleast_2d(means)
    covs = np.asarray(covs, dtype=np.float64)
    covs = covs if covs.ndim == 3 else covs[None]
    K, d = means.shape
    wts = np.full(K, 1.0 / K) if weights is None else np.asarray(weights, dtype=np.float64)
    terms = np.empty((K, len(x)))
    for k in range(K):
        L = np.linalg.cholesky(covs[k])
        y = solve_triangular(L, (x - means[k]).T, lower=True)
        cn = d * np.log(2 * np.pi) + 2 * np.sum(np.log(np.diag(L)))
        terms[k] = np.log(wts[k]) - (np.sum(y * y, axis=0) + cn) / 2
    top = terms.max(axis=0)
    return top + np.log(np.sum(np.exp(terms - top), axis=0))


EVAL_SCALES = ("offset", "negative", "mixed", "tiny")
EVAL_SHAPES = [(d, K) for d in (5, 30, 100) for K in (1, 3)]


def eval_problem(d, K, scale):
    """Target and evaluation points of the evaluator comparison: 64 points drawn from the target and
    8 points 30 sigma out (along the first principal axes of the first mode)."""
    a, b = box(scale, d)
    rng = np.random.default_rng(500 + d + K)
    means, covs, _ = wall_problem(d, a, b, K=K, rng=rng, W=1)
    pts = []
    for n in range(64):
        k = n % K
        pts.append(means[k] + np.linalg.cholesky(covs[k]) @ rng.normal(size=d))
    L0 = np.linalg.cholesky(covs[0])
    for n in range(8):
        z = np.zeros(d)
        z[n % d] = 30.0 if n % 2 == 0 else -30.0
        pts.append(means[0] + L0 @ z)
    return a, b, means, covs, np.array(pts)


def relative_error(got, ref):
    """|got - ref| / max(1, |ref|) per point, against long-double values."""
    ref = np.asarray(ref, dtype=np.longdouble)
    return (np.abs(np.asarray(got) - ref) / np.maximum(1, np.abs(ref))).astype(np.float64)


def eval_bound(err_numpy, d, ref):
    """What the device may be off by, per point: 4 x the numpy recipe's own error `err_numpy` (its
    worst relative_error over the points of the problem), and no less than the summation-order
    floor (d + 8) 2^-53, both relative to max(1, |loglike|)."""
    size = np.maximum(1.0, np.abs(np.asarray(ref, dtype=np.float64)))
    return max(4.0 * float(err_numpy), (d + 8) * 2.0 ** -53) * size
