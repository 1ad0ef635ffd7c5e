// Kernel arguments of derived_kernels.hip (shared with capi_derived.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mcmc {

constexpr int kDvMaxNames = 32;     // derived rows z[m][W], m <= 32
constexpr int kDvMaxCross = 256;    // sampler indices whose cross-moments are kept (<= d <= 256)
constexpr int kDvThreads = 256;     // derived_group_kernel: 32 columns x 8 rows of a, up to five passes of rows
constexpr int kDvCols = 32;         // columns a workgroup carries (a lane each)
constexpr int kDvChunk = 64;        // walkers staged in LDS at a time
constexpr int kDvLd = kDvChunk + 1; // row stride of the tiles: odd, so that 32 columns hit 32 banks
constexpr int kDvRowsPerPass = kDvThreads / kDvCols;   // 8
constexpr int kDvMaxPasses = 5;     // passes of eight rows that hold m + 2 <= 34 rows

// The ordering key of a double (bestfit_kernels.hip's): an unsigned 64-bit integer ordered like the
// doubles, 0 = none.  max[j] lives on the device as the largest key, min[j] as the largest ~key.
__host__ __device__ inline unsigned long long dv_key(double v)
{
    unsigned long long b;
    __builtin_memcpy(&b, &v, sizeof b);
    return b ^ ((b >> 63) ? ~0ull : (1ull << 63));
}
__host__ __device__ inline double dv_value(unsigned long long key)   // (key != 0)
{
    const unsigned long long b = (key >> 63) ? (key ^ (1ull << 63)) : ~key;
    double v;
    __builtin_memcpy(&v, &b, sizeof v);
    return v;
}

// The columns every a_j is multiplied with, n_col = 1 + m + n_cross of them: column 0 is the
// constant 1 of a used walker (a_j * 1.0 is exact: the chain is A[j]), columns 1 .. m are a_k (B[j][k],
// kept for k <= j), the rest are b_c (C[j][c]).  Row m of a is the constant 1 of a used walker: its
// chains over the columns b_c are X[c] = sum b_c; row m + 1 is the column itself: V[c] = sum b_c b_c.
//
// The 64-bit words of the accumulator slab:
//   N uint64 | S[m + 2][n_col] doubles | bad[m] uint64 | kmax[m] keys | kmin[m] inverted keys
struct DvArgs {
    const double* x;          // the ensemble's state, dimension-major [d][W]
    const double* z;          // the derived rows, dimension-major [m][W]
    const double* shift;      // [m] the conditioning vector of the derived rows
    const double* xshift;     // [d] the moment shift
    const int* cross;         // [n_cross] sampler indices
    double* Sg;               // [G][m + 2][n_col] this accumulation's chains
    unsigned long long* Ng;   // [G] ... and used walkers
    unsigned long long* N;    // the slab, by part
    double* S;
    unsigned long long* bad;
    unsigned long long* kmax;
    unsigned long long* kmin;
    int W, gs, G, m, n_cross, n_col;
};

}  // namespace mcmc

// the launcher of derived_kernels.hip: the group chains, then (a launch boundary later) the pooling
extern "C" hipError_t mcmc_hip_launch_derived(const mcmc::DvArgs* a, hipStream_t st);
