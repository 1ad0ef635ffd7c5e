// Kernel arguments of importance_hist_kernels.hip (shared with capi_importance.hip).
#pragma once
#include "importance_args.h"
#include "marginal_args.h"

namespace mcmc {

constexpr int kImHistThreads = 256;
constexpr int kImHistMaxSlice = 4096;        // walkers of one workgroup: its LDS sums stay below 2^60
constexpr int kImHistFracBits = 32;          // q = floor(min(e, 2^16) * 2^32) <= 2^48
constexpr double kImHistScale = 4294967296.0;   // 2^32
constexpr double kImHistCap = 65536.0;          // 2^16: a used walker with e above it is `saturated`

// The fixed-point weight of a walker ("Importance marginals"); e >= 0 is finite.
// The product by a power of two is exact, the conversion truncates: the floor of a value >= 0.
__host__ __device__ inline unsigned long long im_hist_q(double e)
{
    return (unsigned long long)((e < kImHistCap ? e : kImHistCap) * kImHistScale);
}

// the slab: per alternative WITH histograms (h = 0 .. n_hist - 1, ascending alternative)
// lo[n_counters] | hi[n_counters], the low and high words of the 128-bit counters in the layout of the
// marginals slab; behind all of them saturated[n_hist]
struct ImHistArgs {
    const double* x;               // the ensemble's state, dimension-major [d][W]
    const double* z;               // the derived rows [m][W]; null: none
    const MargEntry* entries;      // [n_entries] the table of the marginals
    const double* delta;           // [n_alt][W] the log-weights
    const unsigned long long* ckey;   // [n_alt] the keys of c (the importance slab's)
    unsigned long long* q;         // [n_hist][W] the quantised weights of this accumulation
    unsigned long long* slab;
    unsigned long long* saturated; // [n_hist]
    unsigned long long n_counters; // of one histogram set (the marginals slab's)
    int alt[kImMaxAlt];            // the alternative of histogram set h
    int W, d, n_entries, n_hist;
    int slice;                     // walkers one workgroup bins (a multiple of kImHistThreads, <= 4096)
    int n_slices;                  // ceil(W / slice)
};

}  // namespace mcmc

// the launchers of importance_hist_kernels.hip.  `weights`: q[h][W] of this accumulation and the
// saturated counts; `hist`: every used walker adds q where marginals_kernel adds 1; lds_words = the
// counters of the largest entry (the uint64 histogram a workgroup keeps in LDS)
extern "C" hipError_t mcmc_hip_launch_importance_hist_weights(const mcmc::ImHistArgs* a, hipStream_t st);
extern "C" hipError_t mcmc_hip_launch_importance_hist(const mcmc::ImHistArgs* a, int lds_words, hipStream_t st);
