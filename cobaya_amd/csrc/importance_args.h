// Kernel arguments of importance_kernels.hip (shared with capi_importance.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mcmc {

constexpr int kImMaxAlt = 8;         // alternatives of one run
constexpr int kImMaxDim = 256;       // means and variances; with the covariance: kImMaxCovDim
constexpr int kImMaxCovDim = 128;    // the row tile of a covariance block holds d x 65 doubles of LDS
constexpr int kImThreads = 256;      // importance_group_kernel: four waves
constexpr int kImChunk = 64;         // walkers staged at a time: one lane each
constexpr int kImCols = 32;          // columns j of a workgroup: one lane each
constexpr int kImLd = 65;            // odd row stride of the tiles: 32 rows hit 32 different bank pairs
constexpr int kImRowsPerPass = 8;    // kImThreads / kImCols: rows i a pass of the threads covers
constexpr int kImMaxPasses = 16;     // kImMaxCovDim / kImRowsPerPass
constexpr double kImClamp = 700.0;   // the largest argument of dexp ("Importance")

constexpr int kImMaxPerThread = 8;   // importance_max_kernel: walkers a thread looks at

// The ordering key of a double (bestfit_kernels.hip's): an unsigned 64-bit integer ordered like the
// doubles, 0 = none.  c lives on the device as the key of the maximum of the finite log-weights.
__host__ __device__ inline unsigned long long im_key(double v)
{
    unsigned long long b;
    __builtin_memcpy(&b, &v, sizeof b);
    return b ^ ((b >> 63) ? ~0ull : (1ull << 63));
}
__host__ __device__ inline double im_value(unsigned long long key)   // (0 -> 0.0)
{
    const unsigned long long b = (key >> 63) ? (key ^ (1ull << 63)) : ~key;
    double v;
    __builtin_memcpy(&v, &b, sizeof v);
    return key == 0ull ? 0.0 : v;
}

// chains of one (alternative, group): S1 | S2 | M[d] | V[d] | with the covariance Q[d (d - 1) / 2],
// (i, j < i) at i (i - 1) / 2 + j
__host__ __device__ inline size_t im_n_chains(int d, int cov)
{
    return 2 + 2 * (size_t)d + (cov ? (size_t)d * (d - 1) / 2 : 0);
}

// the 64-bit words of the slab: sums (alternative k at off[k]: [G][n_chains] doubles) | n[n_alt][G]
// uint64 | counters[n_alt][3] uint64 (zero, nonfinite, clamped) | the keys of c [n_alt]
struct ImArgs {
    const double* x;               // the ensemble's state, dimension-major [d][W]
    const double* shift;           // [d] the moment shift
    const double* delta;           // [n_alt][W] the log-weights
    double* sums;
    unsigned long long* n;         // [n_alt][G] the used walkers
    unsigned long long* counters;  // [n_alt][3]
    unsigned long long* ckey;      // [n_alt]
    unsigned long long off[kImMaxAlt];   // where the chains of alternative k begin in `sums`
    int cov[kImMaxAlt];
    int W, d, gs, G, n_alt;
};

}  // namespace mcmc

// the launchers of importance_kernels.hip.  `importance`: the groups' ordered chains are added to
// `sums`, the counts to n and the counters; `importance_max`: the keys of c = the exact maximum of the
// finite delta[k][W] (the words are zeroed, then every workgroup adds its maximum with a 64-bit atomic
// max: exact, whatever the launch)
extern "C" hipError_t mcmc_hip_launch_importance(const mcmc::ImArgs* a, hipStream_t st);
extern "C" hipError_t mcmc_hip_launch_importance_max(const mcmc::ImArgs* a, hipStream_t st);
