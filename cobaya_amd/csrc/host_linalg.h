// Small dense linear algebra on the host (row-major, n x n): what the targets, the proposal and
// mcmc_hip_gelman_rubin need.  Its results are uploaded and compared bit for bit with the oracle:
// compiled without contraction like everything else.
#pragma once

// lower Cholesky, row-major; false if not positive definite (np.linalg.cholesky semantics)
bool cholesky_lower(int n, const double* A, double* L);
// inverse of a lower-triangular matrix (LAPACK dtrtri semantics, functions.py:81-89)
void tri_inverse_lower(int n, const double* L, double* Li);
// eigenvalues of a symmetric matrix (np.linalg.eigvalsh); A is destroyed; false if QL fails to converge
bool symmetric_eigenvalues(int n, double* A, double* ev);
// np.allclose(A.T, A) (rtol 1e-5, atol 1e-8), proposal.py:243
bool is_symmetric(int n, const double* A);
