// Streaming 1-D and 2-D marginal histograms of the ensemble (gfx950): what a moment snapshot keeps
// of the state x[d][W] besides its first and second moments.  The rule (DESIGN.md section 2,
// "Marginals"): a value is in range iff x >= lo && x <= hi; its bin is
// k = min((int)floor((x - lo) * s), B - 1) with s = B / (hi - lo) formed on the host -- the
// subtraction and the product are separate roundings (-ffp-contract=off).  Counters are uint64 in
// global memory, so the statistic does not depend on the order of the atomics or on the launch.
// An entry whose index is d + r reads row r of the derived rows z[m][W] instead of x.  A NaN compares
// false with everything: in a 1-D entry it is counted nowhere, in a pair it is counted `outside`.
//
//   marginals_kernel   one workgroup per (entry, slice of walkers): the slice's row(s) of x are read
//                      coalesced, binned into a uint32 histogram in LDS with LDS integer atomics,
//                      and the non-zero bins are added to the slab with 64-bit global atomics.
//
// All entries of an accumulation are ONE launch.  A slice holds at most 4096 walkers, so an LDS
// counter cannot overflow.
#include "marginal_args.h"

namespace mcmc {
namespace {

constexpr int kUnroll = 4;

// bin of an in-range value (the rule above); max(.., 0) never acts on a finite in-range value --
// it keeps the LDS index in bounds whatever the host handed down
__device__ __forceinline__ int marg_bin(double x, double lo, double s, int B)
{
    const double t = (x - lo) * s;
    const int k = (int)floor(t);
    return max(min(k, B - 1), 0);
}

__global__ void __launch_bounds__(kMargThreads) marginals_kernel(const MargArgs a)
{
    extern __shared__ unsigned int hist[];
    const int e = blockIdx.x / a.n_slices;
    const int sl = blockIdx.x - e * a.n_slices;
    if (e >= a.n_entries) return;
    const MargEntry E = a.entries[e];
    const bool pair = E.j >= 0;
    const int B = E.B;
    // LDS layout = the entry's slab layout: 1-D [under, over, bins], pair [outside, bins]
    const int head = pair ? 1 : 2;
    const int n_cnt = head + (pair ? B * B : B);
    for (int k = threadIdx.x; k < n_cnt; k += kMargThreads) hist[k] = 0u;
    __syncthreads();

    const int w0 = sl * a.slice;
    const int w1 = min(w0 + a.slice, a.W);
    // (an index from d up is a derived row; below d the entry reads x as it always did)
    const int ej = pair ? E.j : E.i;
    const double* __restrict__ xi = E.i < a.d ? a.x + (size_t)E.i * a.W : a.z + (size_t)(E.i - a.d) * a.W;
    const double* __restrict__ xj = ej < a.d ? a.x + (size_t)ej * a.W : a.z + (size_t)(ej - a.d) * a.W;
    for (int wb = w0 + (int)threadIdx.x; wb < w1; wb += kMargThreads * kUnroll) {
        double vi[kUnroll], vj[kUnroll];
#pragma unroll
        for (int r = 0; r < kUnroll; ++r) {
            const int w = wb + r * kMargThreads;
            const bool on = w < w1;
            vi[r] = on ? xi[w] : 0.0;
            vj[r] = (on && pair) ? xj[w] : 0.0;
        }
#pragma unroll
        for (int r = 0; r < kUnroll; ++r) {
            if (wb + r * kMargThreads >= w1) continue;
            const double v = vi[r];
            if (!pair) {
                if (v >= E.lo_i && v <= E.hi_i) atomicAdd(&hist[2 + marg_bin(v, E.lo_i, E.s_i, B)], 1u);
                else if (v < E.lo_i) atomicAdd(&hist[0], 1u);
                else if (v > E.hi_i) atomicAdd(&hist[1], 1u);
            } else {
                const double u = vj[r];
                const bool in = v >= E.lo_i && v <= E.hi_i && u >= E.lo_j && u <= E.hi_j;
                if (in) {
                    const int ki = marg_bin(v, E.lo_i, E.s_i, B), kj = marg_bin(u, E.lo_j, E.s_j, B);
                    atomicAdd(&hist[1 + ki * B + kj], 1u);
                } else {
                    atomicAdd(&hist[0], 1u);
                }
            }
        }
    }
    __syncthreads();

    unsigned long long* __restrict__ out = a.slab + E.offset;
    for (int k = threadIdx.x; k < n_cnt; k += kMargThreads) {
        const unsigned int c = hist[k];
        if (c != 0u) atomicAdd(&out[k], (unsigned long long)c);
    }
}

}  // namespace
}  // namespace mcmc

extern "C" hipError_t mcmc_hip_launch_marginals(const mcmc::MargArgs* a, int lds_words, hipStream_t st)
{
    if (a->n_entries <= 0 || a->n_slices <= 0) return hipSuccess;
    const size_t lds = sizeof(unsigned int) * (size_t)lds_words;
    hipLaunchKernelGGL(mcmc::marginals_kernel, dim3((unsigned)(a->n_entries * a->n_slices)),
                       dim3(mcmc::kMargThreads), lds, st, *a);
    return hipGetLastError();
}
