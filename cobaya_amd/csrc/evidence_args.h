// Kernel arguments of evidence_kernels.hip (shared with capi_evidence.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mcmc {

constexpr int kEvMaxRadii = 8;       // radii of the ladder: one chain thread each
constexpr int kEvMaxDim = 256;       // d x 64 doubles of LDS per workgroup: 128 KiB at d = 256
constexpr int kEvThreads = 256;      // evidence_kernel: four waves share the 64 walkers of a workgroup
constexpr int kEvLanes = 64;         // walkers of a workgroup: one lane each
constexpr int kEvRows = 4;           // rows of Linv a wave carries side by side (one chain each)
constexpr double kEvClamp = 700.0;   // the largest argument of dexp ("Evidence")

constexpr int kEvMaxPerThread = 8;   // evidence_max_kernel: walkers a thread looks at

// The ordering key of a double (bestfit_kernels.hip's): an unsigned 64-bit integer ordered like the
// doubles, 0 = none.  c lives on the device as the key of the maximum of logpost.
__host__ __device__ inline unsigned long long ev_key(double v)
{
    unsigned long long b;
    __builtin_memcpy(&b, &v, sizeof b);
    return b ^ ((b >> 63) ? ~0ull : (1ull << 63));
}
__host__ __device__ inline double ev_value(unsigned long long key)   // (0 -> 0.0)
{
    const unsigned long long b = (key >> 63) ? (key ^ (1ull << 63)) : ~key;
    double v;
    __builtin_memcpy(&v, &b, sizeof v);
    return key == 0ull ? 0.0 : v;
}

// the 64-bit words of the slab: acc[G][n_r] doubles | cnt[G][n_r] uint64 | clamped uint64 | key of c
struct EvArgs {
    const double* x;               // the ensemble's state, dimension-major [d][W]
    const double* logpost;         // [W]
    const double* m;               // [d] the centre of the active ellipsoid
    const double* Linv;            // [d][d] row-major, lower triangular: chol(C)^-1
    double* s;                     // [W] scratch: |Linv (x - m)|^2 of every walker
    double* acc;                   // [G][n_r]
    unsigned long long* cnt;       // [G][n_r]
    unsigned long long* clamped;   // [1]
    unsigned long long* ckey;      // [1] the centring constant of the active ellipsoid, as its key
    double r2[kEvMaxRadii];        // R^2 of every radius, ascending
    int W, d, gs, G, n_r;
    int fused;                     // group_size == 64: a workgroup of evidence_kernel IS a group and
                                   // carries its chains itself (set by the launcher)
};

}  // namespace mcmc

// the launchers of evidence_kernels.hip.  `evidence`: s[W] of the active ellipsoid, then the
// groups' ordered chains into acc / cnt / clamped (two launches, the stream orders them; ONE where
// group_size is 64);
// `evidence_max`: the key of c = the exact maximum of logpost[W] (the word is zeroed, then every
// workgroup adds its maximum with a 64-bit atomic max: exact, whatever the launch)
extern "C" hipError_t mcmc_hip_launch_evidence(const mcmc::EvArgs* a, hipStream_t st);
extern "C" hipError_t mcmc_hip_launch_evidence_max(const mcmc::EvArgs* a, hipStream_t st);
