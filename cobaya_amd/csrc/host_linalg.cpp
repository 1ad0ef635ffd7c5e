// libmcmc_hip.so: host-side small dense linear algebra and the arithmetic of mcmc_hip_gelman_rubin.
#include "host_linalg.h"

#include "../../include/mcmc_hip.h"

#include <algorithm>
#include <cmath>
#include <limits>
#include <vector>

// ------------------------------------------------------------------ small dense LA (host)
// lower Cholesky, row-major; false if not positive definite (np.linalg.cholesky semantics)
bool cholesky_lower(int n, const double* A, double* L)
{
    std::fill(L, L + (size_t)n * n, 0.0);
    for (int j = 0; j < n; ++j) {
        double s = A[j * n + j];
        for (int k = 0; k < j; ++k) s -= L[j * n + k] * L[j * n + k];
        if (!(s > 0.0) || !std::isfinite(s)) return false;
        const double ljj = std::sqrt(s);
        L[j * n + j] = ljj;
        for (int i = j + 1; i < n; ++i) {
            double t = A[i * n + j];
            for (int k = 0; k < j; ++k) t -= L[i * n + k] * L[j * n + k];
            L[i * n + j] = t / ljj;
        }
    }
    return true;
}

// inverse of a lower-triangular matrix (LAPACK dtrtri semantics, functions.py:81-89)
void tri_inverse_lower(int n, const double* L, double* Li)
{
    std::fill(Li, Li + (size_t)n * n, 0.0);
    for (int j = 0; j < n; ++j) {
        Li[j * n + j] = 1.0 / L[j * n + j];
        for (int i = j + 1; i < n; ++i) {
            double s = 0.0;
            for (int k = j; k < i; ++k) s += L[i * n + k] * Li[k * n + j];
            Li[i * n + j] = -s / L[i * n + i];
        }
    }
}

// eigenvalues of a symmetric matrix (np.linalg.eigvalsh, mcmc.py:881): Householder reduction
// to tridiagonal form followed by the implicit-shift QL iteration (the classic EISPACK
// tred1 / tql1 pair, eigenvalues only).  A is destroyed; returns false if QL fails to converge.
bool symmetric_eigenvalues(int n, double* A, double* ev)
{
    std::vector<double> e(n, 0.0);
    double* d = ev;
    for (int i = n - 1; i > 0; --i) {
        const int l = i - 1;
        double h = 0.0, scale = 0.0;
        if (l > 0) {
            for (int k = 0; k <= l; ++k) scale += std::fabs(A[i * n + k]);
            if (scale == 0.0) {
                e[i] = A[i * n + l];
            } else {
                for (int k = 0; k <= l; ++k) {
                    A[i * n + k] /= scale;
                    h += A[i * n + k] * A[i * n + k];
                }
                double f = A[i * n + l];
                const double g = (f >= 0.0) ? -std::sqrt(h) : std::sqrt(h);
                e[i] = scale * g;
                h -= f * g;
                A[i * n + l] = f - g;
                f = 0.0;
                for (int j = 0; j <= l; ++j) {
                    double gg = 0.0;
                    for (int k = 0; k <= j; ++k) gg += A[j * n + k] * A[i * n + k];
                    for (int k = j + 1; k <= l; ++k) gg += A[k * n + j] * A[i * n + k];
                    e[j] = gg / h;
                    f += e[j] * A[i * n + j];
                }
                const double hh = f / (h + h);
                for (int j = 0; j <= l; ++j) {
                    f = A[i * n + j];
                    const double gg = e[j] - hh * f;
                    e[j] = gg;
                    for (int k = 0; k <= j; ++k) A[j * n + k] -= f * e[k] + gg * A[i * n + k];
                }
            }
        } else {
            e[i] = A[i * n + l];
        }
        d[i] = h;
    }
    for (int i = 0; i < n; ++i) d[i] = A[i * n + i];
    // QL with implicit shifts on (d, e)
    for (int i = 1; i < n; ++i) e[i - 1] = e[i];
    e[n - 1] = 0.0;
    for (int l = 0; l < n; ++l) {
        int iter = 0, m;
        do {
            for (m = l; m < n - 1; ++m) {
                const double dd = std::fabs(d[m]) + std::fabs(d[m + 1]);
                if (std::fabs(e[m]) <= std::numeric_limits<double>::epsilon() * dd) break;
            }
            if (m != l) {
                if (++iter > 60) return false;
                double g = (d[l + 1] - d[l]) / (2.0 * e[l]);
                double r = std::hypot(g, 1.0);
                g = d[m] - d[l] + e[l] / (g + (g >= 0.0 ? std::fabs(r) : -std::fabs(r)));
                double s = 1.0, c = 1.0, p = 0.0;
                int i;
                for (i = m - 1; i >= l; --i) {
                    double f = s * e[i];
                    const double b = c * e[i];
                    r = std::hypot(f, g);
                    e[i + 1] = r;
                    if (r == 0.0) {
                        d[i + 1] -= p;
                        e[m] = 0.0;
                        break;
                    }
                    s = f / r;
                    c = g / r;
                    g = d[i + 1] - p;
                    r = (d[i] - g) * s + 2.0 * c * b;
                    p = s * r;
                    d[i + 1] = g + p;
                    g = c * r - b;
                }
                if (r == 0.0 && i >= l) continue;
                d[l] -= p;
                e[l] = g;
                e[m] = 0.0;
            }
        } while (m != l);
    }
    return true;
}

// np.allclose(A.T, A) (rtol 1e-5, atol 1e-8), proposal.py:243
bool is_symmetric(int n, const double* A)
{
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
            const double a = A[j * n + i], b = A[i * n + j];
            if (!(std::fabs(a - b) <= 1e-8 + 1e-5 * std::fabs(b))) return false;
        }
    return true;
}

extern "C" int mcmc_hip_gelman_rubin(int32_t d, double n_chains, double sum_N, const double* sum_Ncov,
                          const double* sum_mean, const double* sum_mm, double* Rminus1,
                          double* mean_of_covs)
{
    if (d < 1 || !sum_Ncov || !sum_mean || !sum_mm || !Rminus1 || !mean_of_covs)
        return MCMC_HIP_ERR_ARG;
    if (!(n_chains >= 2) || !(sum_N > 0)) return MCMC_HIP_ERR_ARG;
    const size_t n = d;
    std::vector<double> W(n * n), B(n * n), sd(n), nW(n * n), cB(n * n), L(n * n), Li(n * n),
        M(n * n), tmp(n * n), ev(n);
    for (size_t i = 0; i < n * n; ++i) W[i] = mean_of_covs[i] = sum_Ncov[i] / sum_N;  // mcmc.py:856
    // np.cov(means.T): (sum m m^T - n mbar mbar^T) / (n - 1)                        mcmc.py:860
    for (size_t i = 0; i < n; ++i)
        for (size_t j = 0; j < n; ++j)
            B[i * n + j] = (sum_mm[i * n + j] - sum_mean[i] * sum_mean[j] / n_chains) /
                           (n_chains - 1.0);
    for (size_t i = 0; i < n; ++i) {
        if (!(B[i * n + i] > 0.0)) return MCMC_HIP_ERR_NOT_PD;
        sd[i] = std::sqrt(B[i * n + i]);
    }
    for (size_t i = 0; i < n; ++i)
        for (size_t j = 0; j < n; ++j) {
            cB[i * n + j] = B[i * n + j] / sd[i] / sd[j];   // mcmc.py:865
            nW[i * n + j] = W[i * n + j] / sd[i] / sd[j];   // mcmc.py:866
        }
    if (!cholesky_lower(d, nW.data(), L.data())) return MCMC_HIP_ERR_NOT_PD;  // mcmc.py:871
    tri_inverse_lower(d, L.data(), Li.data());
    for (size_t i = 0; i < n; ++i)
        for (size_t j = 0; j < n; ++j) {
            double s = 0.0;
            for (size_t k = 0; k < n; ++k) s += Li[i * n + k] * cB[k * n + j];
            tmp[i * n + j] = s;
        }
    for (size_t i = 0; i < n; ++i)
        for (size_t j = 0; j < n; ++j) {
            double s = 0.0;
            for (size_t k = 0; k < n; ++k) s += tmp[i * n + k] * Li[j * n + k];
            M[i * n + j] = s;
        }
    for (size_t i = 0; i < n; ++i)
        for (size_t j = 0; j < i; ++j) M[i * n + j] = M[j * n + i] = 0.5 * (M[i * n + j] + M[j * n + i]);
    if (!symmetric_eigenvalues(d, M.data(), ev.data())) return MCMC_HIP_ERR_NOT_PD;  // mcmc.py:881-887
    double r = 0.0;
    for (size_t i = 0; i < n; ++i) r = std::max(r, std::fabs(ev[i]));
    if (!std::isfinite(r)) return MCMC_HIP_ERR_NOT_PD;
    *Rminus1 = r;  // mcmc.py:889
    return MCMC_HIP_OK;
}
