// Arguments of the d > 128 kernels (huge_kernels.hip): run-time d up to kMaxDimHuge, one parameter
// block, incremental evaluation of up to kHugeMaxModes Gaussian modes.
#pragma once
#include <stdint.h>

#include "kernels.h"   // MomentArgs, hipStream_t

namespace mcmc {

constexpr int kMaxDimHuge = 256;
constexpr int kHugeMaxModes = 4;
constexpr int kHugeRows = 64;   // huge_rows_kernel: rows of H per workgroup (LDS: 64 d doubles)

// doubles per (group, step) column of the direction set: v, u_1 .. u_K, w (the carried log-prior's
// stream), then |u|^2, v.w, loc.w
__host__ __device__ constexpr int huge_col_stride(int d, int K) { return (2 + K) * d + 4; }
// doubles of basis scratch per (group, cycle): the normals / reflectors, the signs, R = D H
__host__ __device__ constexpr long long huge_basis_scratch(int d)
{
    return (((long long)(d + 2) * (d - 1) / 2 + 2 + d + 1) & ~1ll) + (long long)d * d;
}

struct HugeBasisArgs {
    const double* T;   // [d][d] row-major lower-triangular proposal transform
    double* V;         // [n_groups][ncyc][d][d]: column c of cycle at V[c d + i]
    double* scratch;   // [n_slabs][huge_basis_scratch(d)]
    int d, ncyc;
    uint32_t group0, cycle0, key0, key1;
    int slab0;         // the first (group, cycle) slab of this batch: slab = g ncyc + cycle
    int n_slabs;
};

struct HugeDirArgs {
    const double* V;       // [BG][ncyc][d][d] (HugeBasisArgs)
    const double* Lrow;    // [K][d][d] row-major L^-1
    const double* prior;   // [5][dpad]: lo, hi, loc, 1/scale (0: not normal), mls
    double* out;           // [BG][n_steps][huge_col_stride(d, K)]
    unsigned long long step0, cycle0;
    int n_steps, ncyc, d, dpad, K;
    int carry_prior;
};

struct HugeStepArgs {
    double* x;            // [d][W]
    double* y;            // [K][d][W]
    double* logpost; double* logprior; double* loglike;
    int* weight; int* prior_rej; int* burn_left;
    long long* n_accept;
    unsigned long long* accept_total;
    int* stuck;
    const double* cols;   // [BG][n_steps][huge_col_stride(d, K)]
    const double* prior;  // [5][dpad]
    const double* Lrow;   // [K][d][d]
    const double* mean;   // [K][d]
    const double* scale;  // [d] (K = 0: the normal terms of the log-prior as eval_point forms them)
    const double* cnorm;  // [K]
    const double* mweight;   // [K]
    int d, dpad, K, W, bgs;
    uint32_t walker0, key0, key1;
    unsigned long long step0, refresh;   // y is refreshed from x at the steps that are multiples of refresh
    int n_steps;
    int anchor;           // refresh y (and re-anchor) before the first step whatever its number
    int carry_prior;
    double uniform_logp, temperature, max_tries;
};

struct HugeEvalArgs {
    const double* x;      // [n][d] point-major
    double* logprior; double* loglike;
    double* derived;      // [n][K d] or null
    const double* prior;  // [5][dpad]: a dimension has a normal prior iff 1/scale != 0
    const double* scale;  // [d]
    const double* Lrow; const double* mean; const double* cnorm; const double* mweight;
    int n, d, dpad, K;
    double uniform_logp;
};

}  // namespace mcmc

// the launchers of huge_kernels.hip (128 < d <= 256, run-time d; incremental evaluation, one block,
// up to four modes): declared here alone, for the kernels' translation unit and the host side
extern "C" hipError_t mcmc_hip_launch_huge_basis(const mcmc::HugeBasisArgs*, int, int, hipStream_t);
extern "C" hipError_t mcmc_hip_launch_huge_dirs(const mcmc::HugeDirArgs*, int, hipStream_t);
extern "C" hipError_t mcmc_hip_launch_huge_step(const mcmc::HugeStepArgs*, hipStream_t);
extern "C" hipError_t mcmc_hip_launch_huge_evaluate(const mcmc::HugeEvalArgs*, hipStream_t);
extern "C" hipError_t mcmc_hip_launch_huge_moments(const mcmc::MomentArgs*, int, int, hipStream_t);
