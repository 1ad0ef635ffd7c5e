// Kernel arguments of autocorr_kernels.hip (shared with capi_autocorr.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mcmc {

constexpr int kAcMaxLags = 64;      // 1 <= lags <= 64: the ring holds lags + 1 snapshots
constexpr int kAcThreads = 256;
constexpr size_t kAcLdsMax = 64 * 1024;   // what a workgroup stages: the tile and the product rows

// One accumulation ("Autocorrelation").  `held` counts the snapshots the ring
// holds INCLUDING the current one (1 <= held <= lags + 1); the current snapshot goes into slot
// `head`, the snapshot k back lies in slot (head - k) mod (lags + 1).
struct AcArgs {
    const double* x;        // the ensemble's state, dimension-major [d][W]
    const double* shift;    // the moment shift [d]
    const int* dims;        // sampler indices of the configured dimensions [n]
    double* ring;           // [lags + 1][n][W]: the snapshots, as they were read (unshifted)
    double* ringS;          // [lags + 1][G][n]: the group sums S of every slot
    double* Pg;             // [G][lags + 1][n]: this accumulation's chains P[g, k, i]
    double* acc;            // [3][lags + 1][n]: accP, accA, accB
    int W, G, gs, n, lags, held, head;
    int rows_per_pass;      // product rows a workgroup keeps in LDS at a time
};

}  // namespace mcmc

// the launchers of autocorr_kernels.hip: the group chains, then (a launch boundary later) the pooling
extern "C" hipError_t mcmc_hip_launch_autocorr(const mcmc::AcArgs* a, hipStream_t st);
// product rows (of group_size + 1 doubles, beside the tile) that fit a workgroup's LDS
extern "C" int mcmc_hip_autocorr_rows_per_pass(int group_size, int lags);
