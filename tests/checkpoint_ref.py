"""A plain reference of the learn / convergence checkpoint (checkpoint_kernels.hip), for the
tests only: no GPU, no library of the product.

 * `window_sums`: the float64 sums over a window of intervals and the chain means -- a BIT
   specification (additions in ascending order from +0 and one division; nothing a compiler can
   contract);
 * `payload`, `rminus1`, `proposal_transform`: the statistics the all-reduce carries, R-1 of the
   means (cobaya/samplers/mcmc/mcmc.py:856-889) and the proposal transform
   (cobaya/samplers/mcmc/proposal.py:226-260) in `np.longdouble` (x87 extended, 64-bit
   significand).  Written as loops over rows / columns of element-wise long-double operations:
   numpy has no BLAS for long double, so no library routine decides an operation order here;
 * `crafted_payloads`: the fixed-seed family of all-reduced payloads the CPU test measures the
   host routine on and the GPU test runs the solve kernel on.
"""
import numpy as np

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)

# The device's bound on R-1:  |R_dev - R_ref| <= C_DEVICE eps (cond2(nW) + d) R_ref.
# test_checkpoint_ref.py measures the host routine's worst rel_err / (eps (cond2(nW) + d)) over
# the kept cases of crafted_payloads(): C_HOST_MEASURED (docs/MEASUREMENTS.md, "checkpoint
# kernels").  The device gets 8 x that, rounded up to a power of two: only its eigenvalue route
# differs (bisection on Sturm counts with a hardware reciprocal and a Newton step; the host runs
# QL), everything before the eigenproblem follows the host's operation order.  The CPU test
# asserts C_host <= C_DEVICE / 8, so the literal cannot drift from its measurement.
# (The worst case, d = 1 with two chains, is the cancellation in B = sum_mm - sum_mean^2 / n of
# two nearby means, which cond2(nW) does not see; from d = 2 on the measurement is below 1.6.)
C_HOST_MEASURED = 9.2333
C_DEVICE = 128.0

# a case whose within-chain matrix is so ill-conditioned that R-1 carries fewer than ~6 digits
# in double precision is no test of a kernel
DROP_ABOVE = 1e-6       # eps * cond2(nW)

DIMS = (1, 2, 3, 26, 27, 52, 53, 100, 128)


# ------------------------------------------------------------------ window sums (float64, bits)
def window_sums(intervals, n_per_chain):
    """`intervals`: the window's (group_sum[G][d], pooled_S[d][d]) pairs, oldest first.
    -> (g_sum, S_sum, means): each element the float64 sum of the intervals' in ascending order
    from +0 (the host's `sum(iv[1] for iv in intervals)`), means = g_sum / n_per_chain."""
    g_sum = np.zeros_like(np.asarray(intervals[0][0], dtype=np.float64))
    S_sum = np.zeros_like(np.asarray(intervals[0][1], dtype=np.float64))
    for g, S in intervals:            # (element-wise IEEE additions, one per interval)
        g_sum = g_sum + np.asarray(g, dtype=np.float64)
        S_sum = S_sum + np.asarray(S, dtype=np.float64)
    means = g_sum / np.float64(n_per_chain)
    return g_sum, S_sum, means


def sequential_sum(means):
    """sum over the chains (rows) one by one from +0, in float64: a bit specification of
    `sum_mean` given the chain means."""
    s = np.zeros(means.shape[1])
    for g in range(means.shape[0]):
        s = s + means[g]
    return s


# ------------------------------------------------------------------ the payload (long double)
def payload(means, S_window, Nc):
    """-> (sum_mean[d], sum_mm[d][d], sum_Ncov[d][d], abs_mm[d][d]) in long double from the
    float64 chain means [G][d], the window's pooled second moments S and the samples per chain
    Nc: sum_mm = sum_g m_g m_g^T, sum_Ncov = S - Nc sum_mm.  abs_mm = sum_g |m_gi m_gj|, the
    scale of the rounding error of a float64 evaluation of sum_mm."""
    m = np.asarray(means, dtype=np.float64).astype(LD)
    G, d = m.shape
    sum_mean = np.zeros(d, LD)
    sum_mm = np.zeros((d, d), LD)
    abs_mm = np.zeros((d, d), LD)
    for g in range(G):
        sum_mean = sum_mean + m[g]
        outer = m[g][:, None] * m[g][None, :]
        sum_mm = sum_mm + outer
        abs_mm = abs_mm + np.abs(outer)
    sum_Ncov = np.asarray(S_window, dtype=np.float64).astype(LD) - LD(Nc) * sum_mm
    return sum_mean, sum_mm, sum_Ncov, abs_mm


# ------------------------------------------------------------------ dense pieces (long double)
def _cholesky(A):
    """Lower Cholesky factor in long double, or None where it does not exist."""
    n = len(A)
    L = np.zeros((n, n), LD)
    for j in range(n):
        s = A[j, j] - (L[j, :j] * L[j, :j]).sum()
        if not (s > 0) or not np.isfinite(s):
            return None
        L[j, j] = np.sqrt(s)
        for i in range(j + 1, n):
            L[i, j] = (A[i, j] - (L[i, :j] * L[j, :j]).sum()) / L[j, j]
    return L


def _tri_inverse(L):
    n = len(L)
    Li = np.zeros((n, n), LD)
    for j in range(n):
        Li[j, j] = LD(1) / L[j, j]
        for i in range(j + 1, n):
            Li[i, j] = -(L[i, j:i] * Li[j:i, j]).sum() / L[i, i]
    return Li


def _matmul(A, B):
    n, m = A.shape[0], B.shape[1]
    C = np.zeros((n, m), LD)
    for i in range(n):
        for k in range(A.shape[1]):
            C[i] = C[i] + A[i, k] * B[k]
    return C


def rminus1(n_chains, sum_N, sum_Ncov, sum_mean, sum_mm):
    """mcmc.py:856-889 from the reduced sufficient statistics, in long double:
    W = sum N cov / sum N, B = cov of the chain means (ddof 1), both normalised by sqrt(diag B),
    L = chol(nW), M = L^-1 cB L^-T symmetrised, R-1 = max |eigvalsh(M)| (eigenvalues of the
    float64 cast: an error of a few eps of the largest, which is the statistic).
    -> (R-1, cond2(nW), mean_of_covs as long double), or None where a step of the reference
    raises LinAlgError (B not positive on the diagonal, nW not positive definite)."""
    sum_Ncov, sum_mean, sum_mm = (np.asarray(a).astype(LD) for a in (sum_Ncov, sum_mean, sum_mm))
    n, N = LD(n_chains), LD(sum_N)
    d = len(sum_mean)
    W = sum_Ncov / N
    with np.errstate(divide="ignore", invalid="ignore"):       # (one chain: n - 1 = 0, refused below)
        B = (sum_mm - sum_mean[:, None] * sum_mean[None, :] / n) / (n - LD(1))
    diag = np.array([B[i, i] for i in range(d)])
    if not np.all(diag > 0) or not np.all(np.isfinite(B)) or not np.all(np.isfinite(W)):
        return None
    sd = np.sqrt(diag)
    cB = B / sd[:, None] / sd[None, :]
    nW = W / sd[:, None] / sd[None, :]
    L = _cholesky(nW)
    if L is None:
        return None
    Li = _tri_inverse(L)
    M = _matmul(_matmul(Li, cB), Li.T.copy())
    M = LD(0.5) * (M + M.T)
    ev = np.linalg.eigvalsh(M.astype(np.float64))
    r = float(np.max(np.abs(ev)))
    if not np.isfinite(r):
        return None
    evW = np.linalg.eigvalsh(nW.astype(np.float64))
    cond = float(evW[-1] / evW[0]) if evW[0] > 0 else np.inf
    return r, cond, W


def proposal_transform(cov, i_of_j=None, scale=2.4):
    """BlockedProposer.set_covariance (proposal.py:226-260) in long double: the covariance
    reordered by i_of_j, std, the correlation matrix with a unit diagonal, its Cholesky factor,
    T = scale diag(std) L.  -> (T, cond2(corr)), or None where the factor does not exist."""
    cov = np.asarray(cov).astype(LD)
    d = len(cov)
    if i_of_j is not None:
        idx = np.asarray(i_of_j, dtype=int)
        cov = cov[idx][:, idx]
    diag = np.array([cov[i, i] for i in range(d)])
    if not np.all(diag > 0) or not np.all(np.isfinite(diag)):
        return None
    sd = np.sqrt(diag)
    corr = cov / sd[:, None] / sd[None, :]
    for i in range(d):
        corr[i, i] = LD(1)
    L = _cholesky(corr)
    if L is None:
        return None
    ev = np.linalg.eigvalsh(corr.astype(np.float64))
    cond = float(ev[-1] / ev[0]) if ev[0] > 0 else np.inf
    return LD(scale) * sd[:, None] * L, cond


# ------------------------------------------------------------------ the crafted family
def pack(n_chains, sum_N, sum_Ncov, sum_mean, sum_mm, d_accepted=0.0, d_steps=0.0, accepted=0.0):
    """The buffer of the all-reduce: [chains, sum N, accepted since, steps x walkers since,
    accepted | sum N cov | sum of chain means | sum of m m^T]."""
    return np.concatenate(([n_chains, sum_N, d_accepted, d_steps, accepted],
                           np.ravel(sum_Ncov), np.ravel(sum_mean), np.ravel(sum_mm))).astype(np.float64)


def unpack(P, d):
    P = np.asarray(P)
    return (P[0], P[1], P[5:5 + d * d].reshape(d, d), P[5 + d * d:5 + d * d + d],
            P[5 + d * d + d:5 + 2 * d * d + d].reshape(d, d))


def _within(rng, d, c, block_W):
    """W = Q diag(c^(-i/(d-1))) Q^T rescaled by per-parameter scales 10^U(-3, 3); `block_W`:
    2 x 2 and 1 x 1 diagonal blocks only (exact zeros elsewhere)."""
    lam = np.array([c ** (-i / max(d - 1, 1)) for i in range(d)])
    if block_W:
        W = np.zeros((d, d))
        i = 0
        while i < d:
            if i + 1 < d and (i // 2) % 2 == 0:
                t = rng.uniform(0.2, 1.2)
                Q = np.array([[np.cos(t), -np.sin(t)], [np.sin(t), np.cos(t)]])
                W[i:i + 2, i:i + 2] = (Q * lam[i:i + 2]) @ Q.T
                i += 2
            else:
                W[i, i] = lam[i]
                i += 1
    else:
        Q, _ = np.linalg.qr(rng.standard_normal((d, d)))
        W = (Q * lam) @ Q.T
    s = 10.0 ** rng.uniform(-3, 3, d)
    W = W * s[:, None] * s[None, :]
    return 0.5 * (W + W.T)


def case(rng, d, c, n_chains, spread=1.0, diag_B=False, block_W=False):
    """One payload of the family (`block_W` comes with `diag_B`)."""
    N = 6400.0                                 # samples per chain (100 snapshots of 64 walkers)
    W = _within(rng, d, c, block_W)
    sum_N = N * n_chains
    sum_Ncov = sum_N * W
    if not diag_B:
        # chain means ~ N(mu, W / N) (times `spread`); mu is of the size of that spread, as the
        # moment shift leaves it in a run (the statistic is formed from shifted sums)
        Lw = np.linalg.cholesky(W / N)
        sig = np.sqrt(np.diag(W) / N)
        mu = 0.5 * spread * sig * rng.standard_normal(d)
        means = mu + spread * (rng.standard_normal((n_chains, d)) @ Lw.T)
        sum_mean = sequential_sum(means)
        sum_mm = np.zeros((d, d))
        for g in range(n_chains):
            sum_mm = sum_mm + np.outer(means[g], means[g])
    else:
        # B exactly diagonal: chain means that sum to zero exactly and have no cross moments
        sum_mean = np.zeros(d)
        sum_mm = np.diag(np.diag(W) / N * (n_chains - 1) * rng.uniform(0.5, 2.0, d))
    sum_mm = 0.5 * (sum_mm + sum_mm.T)
    return pack(float(n_chains), sum_N, sum_Ncov, sum_mean, sum_mm,
                d_accepted=float(rng.integers(1, 10 ** 6)), d_steps=float(rng.integers(10 ** 6, 10 ** 9)),
                accepted=float(rng.integers(10 ** 6, 10 ** 12)))


_family = None


def crafted_payloads():
    """-> list of dicts {name, d, P (the float64 payload), ref (rminus1's result or None),
    kept}.  Seed 0; built once per process.
      d in DIMS x c in {1, 1e4, 1e8} x n_chains in {2, 8, 300}: chain means ~ N(mu, W / N);
      per d, `converged`: the spread of the means 1e-6 of that (R-1 of a converged run);
      per d, `diagB`: B exactly diagonal under a dense W, and `blocks`: B diagonal and W of
      2 x 2 and 1 x 1 blocks, so that M has exact zeros below its subdiagonal (the "column
      already tridiagonal" branch of wg_lambda_max).
    kept = the reference exists and eps cond2(nW) <= DROP_ABOVE."""
    global _family
    if _family is not None:
        return _family
    rng = np.random.default_rng(0)
    cases = []
    for d in DIMS:
        for c in (1.0, 1e4, 1e8):
            for n_chains in (2, 8, 300):
                cases.append((f"d{d}-c{c:g}-n{n_chains}", d, case(rng, d, c, n_chains)))
        cases.append((f"d{d}-converged", d, case(rng, d, 1e4, 8, spread=1e-6)))
        cases.append((f"d{d}-diagB", d, case(rng, d, 1e4, 8, diag_B=True)))
        cases.append((f"d{d}-blocks", d, case(rng, d, 1e4, 8, diag_B=True, block_W=True)))
    out = []
    for name, d, P in cases:
        ref = rminus1(*unpack(P, d))
        kept = ref is not None and EPS * ref[1] <= DROP_ABOVE
        out.append({"name": name, "d": d, "P": P, "ref": ref, "kept": kept})
    _family = out
    return out


def g7_payload(g):
    """The payload of golden `g7_multichain` (six chains of unequal length)."""
    Ns, means, covs = g["Ns"].astype(np.float64), g["means"], g["covs"]
    d = means.shape[1]
    sum_Ncov = np.zeros((d, d))
    sum_mm = np.zeros((d, d))
    for c in range(len(Ns)):
        sum_Ncov = sum_Ncov + Ns[c] * covs[c]
        sum_mm = sum_mm + np.outer(means[c], means[c])
    return pack(float(len(Ns)), float(Ns.sum()), 0.5 * (sum_Ncov + sum_Ncov.T), sequential_sum(means),
                0.5 * (sum_mm + sum_mm.T))
