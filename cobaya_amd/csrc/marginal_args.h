// Kernel arguments of marginal_kernels.hip (shared with capi_marginals.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mcmc {

constexpr int kMargMaxBins1 = 1024;   // bins of a 1-D marginal
constexpr int kMargMaxBins2 = 64;     // bins per axis of a 2-D marginal: 64 x 64 x 4 B = 16 KiB of LDS
constexpr int kMargThreads = 256;

// One histogram of the slab ("Marginals").  1-D: counters
// [under, over, c_0 .. c_{B-1}] of parameter i; pair: [outside, c_{0,0} .. c_{B-1,B-1}], row-major
// with parameter i as the row and j as the column.  s = B / (hi - lo), formed on the host in double.
struct MargEntry {
    double lo_i, hi_i, s_i;
    double lo_j, hi_j, s_j;
    long long offset;      // of the entry's first counter in the slab
    int i, j;              // sampler indices -- d + r: row r of the derived rows z; j < 0: a 1-D entry
    int B;                 // bins (per axis)
    int pad_;
};

struct MargArgs {
    const double* x;               // the ensemble's state, dimension-major [d][W]
    const double* z;               // the derived rows [m][W] (derived_kernels.hip); null: none
    const MargEntry* entries;      // [n_entries]
    unsigned long long* slab;      // the counters of every entry
    int W;
    int d;                         // an entry's index i >= d reads row i - d of z
    int n_entries;
    int slice;                     // walkers one workgroup bins (a multiple of kMargThreads)
    int n_slices;                  // ceil(W / slice)
};

}  // namespace mcmc

// the launcher of marginal_kernels.hip: ONE launch bins every entry; lds_words = the counters of the
// largest entry (the uint32 histogram a workgroup keeps in LDS)
extern "C" hipError_t mcmc_hip_launch_marginals(const mcmc::MargArgs* a, int lds_words, hipStream_t st);
