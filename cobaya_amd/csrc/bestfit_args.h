// Kernel arguments of bestfit_kernels.hip (shared with capi_bestfit.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mcmc {

constexpr int kBfMaxBins = 1024;     // bins of a profile: 1024 x 8 B = 8 KiB of LDS
constexpr int kBfThreads = 256;
constexpr int kBfRecords = 2;        // 0: map (maximum of logpost), 1: bestfit (maximum of loglike)
// 64-bit words of a record in front of x[d] ("Best fit and profiles"):
// key, global walker id, step counter, bits of logpost, logprior, loglike
constexpr int kBfRecordHead = 6;

// One profile of the slab: best[B] of parameter i, bin k = the marginals' rule over [lo, hi] with
// s = B / (hi - lo) formed on the host in double.
struct BfEntry {
    double lo, hi, s;
    int i;                 // sampler index
    int pad_;
};

struct BfArgs {
    const double* x;               // the ensemble's state, dimension-major [d][W]
    const double* logpost;         // [W]
    const double* logprior;        // [W]
    const double* loglike;         // [W]
    const double* value;           // the profiled quantity: loglike or logpost
    const BfEntry* entries;        // [n_entries]
    unsigned long long* slab;      // [n_entries][B] keys, 0 = empty
    unsigned long long* cand;      // [n_slices][kBfRecords][2]: key, local walker id
    unsigned long long* records;   // [kBfRecords][kBfRecordHead + d]
    unsigned long long step;       // the step counter at the accumulation
    unsigned int walker0;          // global id of local walker 0
    int W, d;
    int n_entries, B;
    int slice;                     // walkers one workgroup reads (a multiple of kBfThreads)
    int n_slices;                  // ceil(W / slice)
};

}  // namespace mcmc

// the launchers of bestfit_kernels.hip: ONE launch takes every profile and the slices' candidates
// of both records, the second (one workgroup, queued behind it) commits the records
extern "C" hipError_t mcmc_hip_launch_bestfit(const mcmc::BfArgs* a, hipStream_t st);
extern "C" hipError_t mcmc_hip_launch_bestfit_commit(const mcmc::BfArgs* a, hipStream_t st);
