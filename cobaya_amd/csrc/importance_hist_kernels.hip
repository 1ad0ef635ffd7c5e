// Reweighted marginal histograms of the ensemble (gfx950): what a moment snapshot adds, per alternative
// that asks for them, to a weighted copy of the histograms of marginal_kernels.hip.  The rule (DESIGN.md
// section 2, "Importance marginals"): with c the centring constant of the importance interval, per walker
//     NaN or +inf: not used;   -inf: used, e = 0;   otherwise e = dexp(min(delta - c, 700))
// (the bits of e are importance_group_kernel's), and the weight is the FIXED-POINT integer
//     q = 0 (not used),   q = (uint64) floor(min(e, 2^16) * 2^32) <= 2^48,   saturated counts e > 2^16.
// A used walker adds q exactly where marginals_kernel adds 1 (same in-range test, same bin: separate
// roundings, -ffp-contract=off).  Integers: the sums depend neither on the order of the atomics nor on
// the slices nor on the launch.  Every counter of the slab is a 128-bit unsigned integer kept as the
// words (lo, hi); a workgroup adds its sum s with  old = atomicAdd(&lo, s); if (old + s < old)
// atomicAdd(&hi, 1):  whatever the order, (hi, lo) ends as the exact total.
//
//   importance_hist_weights_kernel   a thread per (walker, histogram set): q[h][W] once per accumulation,
//                                    so that dexp is not paid per entry; saturated[h] by one atomic per
//                                    wave that saw any.
//   importance_hist_kernel           one workgroup per (histogram set, entry, slice of walkers): the
//                                    slice's row(s) of x or z and of q are read coalesced, added into a
//                                    uint64 histogram in LDS (at most 1 + 64 x 64 words = 32 KiB) with
//                                    64-bit LDS atomics; the non-zero sums are flushed as above.
//
// A slice holds at most 4 096 walkers of at most 2^48 each: an LDS sum stays below 2^60.  Vector stores
// only; the stream orders the launches.
#include "importance_hist_args.h"
#include "det_math.h"

#pragma clang fp contract(off)

namespace mcmc {
namespace {

constexpr int kUnroll = 4;

__device__ __forceinline__ bool imh_finite(double v)
{
    return (((unsigned long long)__double_as_longlong(v) >> 52) & 0x7ffull) != 0x7ffull;
}

// bin of an in-range value: marginal_kernels.hip's, operation for operation
__device__ __forceinline__ int imh_bin(double x, double lo, double s, int B)
{
    const double t = (x - lo) * s;
    const int k = (int)floor(t);
    return max(min(k, B - 1), 0);
}

__global__ void __launch_bounds__(kImHistThreads) importance_hist_weights_kernel(const ImHistArgs a)
{
    const int h = blockIdx.y, k = a.alt[h];
    const int w = (int)blockIdx.x * kImHistThreads + (int)threadIdx.x;
    const bool on = w < a.W;
    const double cc = im_value(a.ckey[k]);
    const double dl = a.delta[(size_t)k * a.W + (on ? w : 0)];
    // e of the walker: importance_group_kernel's operations
    const bool fin = imh_finite(dl);
    const double arg = dl - cc;
    const bool cl = on && fin && arg > kImClamp;
    const double er = dexp(cl ? kImClamp : arg);
    const double e = (on && fin) ? er : 0.0;                  // (-inf: used with e = 0, which adds nothing)
    const bool sat = on && fin && e > kImHistCap;
    if (on) a.q[(size_t)h * a.W + w] = im_hist_q(e);
    const unsigned long long m = lanes(sat);
    if (m != 0ull && (threadIdx.x & 63) == 0) atomicAdd(&a.saturated[h], (unsigned long long)__popcll(m));
}

__global__ void __launch_bounds__(kImHistThreads) importance_hist_kernel(const ImHistArgs a)
{
    extern __shared__ unsigned long long hist64[];
    const int e = blockIdx.x / a.n_slices;
    const int sl = blockIdx.x - e * a.n_slices;
    const int h = blockIdx.y;
    if (e >= a.n_entries) return;
    const MargEntry E = a.entries[e];
    const bool pair = E.j >= 0;
    const int B = E.B;
    // LDS layout = the entry's slab layout: 1-D [under, over, bins], pair [outside, bins]
    const int head = pair ? 1 : 2;
    const int n_cnt = head + (pair ? B * B : B);
    for (int k = threadIdx.x; k < n_cnt; k += kImHistThreads) hist64[k] = 0ull;
    __syncthreads();

    const int w0 = sl * a.slice;
    const int w1 = min(w0 + a.slice, a.W);
    const int ej = pair ? E.j : E.i;
    const double* __restrict__ xi = E.i < a.d ? a.x + (size_t)E.i * a.W : a.z + (size_t)(E.i - a.d) * a.W;
    const double* __restrict__ xj = ej < a.d ? a.x + (size_t)ej * a.W : a.z + (size_t)(ej - a.d) * a.W;
    const unsigned long long* __restrict__ qh = a.q + (size_t)h * a.W;
    for (int wb = w0 + (int)threadIdx.x; wb < w1; wb += kImHistThreads * kUnroll) {
        double vi[kUnroll], vj[kUnroll];
        unsigned long long qv[kUnroll];
#pragma unroll
        for (int r = 0; r < kUnroll; ++r) {
            const int w = wb + r * kImHistThreads;
            const bool on = w < w1;
            vi[r] = on ? xi[w] : 0.0;
            vj[r] = (on && pair) ? xj[w] : 0.0;
            qv[r] = on ? qh[w] : 0ull;
        }
#pragma unroll
        for (int r = 0; r < kUnroll; ++r) {
            const unsigned long long q = qv[r];
            if (q == 0ull) continue;                              // (not used, weight zero, or past the slice)
            const double v = vi[r];
            if (!pair) {
                if (v >= E.lo_i && v <= E.hi_i) atomicAdd(&hist64[2 + imh_bin(v, E.lo_i, E.s_i, B)], q);
                else if (v < E.lo_i) atomicAdd(&hist64[0], q);
                else if (v > E.hi_i) atomicAdd(&hist64[1], q);
            } else {
                const double u = vj[r];
                const bool in = v >= E.lo_i && v <= E.hi_i && u >= E.lo_j && u <= E.hi_j;
                if (in) {
                    const int ki = imh_bin(v, E.lo_i, E.s_i, B), kj = imh_bin(u, E.lo_j, E.s_j, B);
                    atomicAdd(&hist64[1 + ki * B + kj], q);
                } else {
                    atomicAdd(&hist64[0], q);
                }
            }
        }
    }
    __syncthreads();

    unsigned long long* __restrict__ lo = a.slab + (size_t)h * 2 * a.n_counters + E.offset;
    unsigned long long* __restrict__ hi = lo + a.n_counters;
    for (int k = threadIdx.x; k < n_cnt; k += kImHistThreads) {
        const unsigned long long s = hist64[k];
        if (s != 0ull) {
            const unsigned long long old = atomicAdd(&lo[k], s);
            if (old + s < old) atomicAdd(&hi[k], 1ull);           // the carry of the 128-bit counter
        }
    }
}

}  // namespace
}  // namespace mcmc

extern "C" hipError_t mcmc_hip_launch_importance_hist_weights(const mcmc::ImHistArgs* a, hipStream_t st)
{
    if (a->W <= 0 || a->n_hist <= 0) return hipSuccess;
    if (a->n_hist > mcmc::kImMaxAlt) return hipErrorInvalidValue;
    hipLaunchKernelGGL(mcmc::importance_hist_weights_kernel,
                       dim3((unsigned)((a->W + mcmc::kImHistThreads - 1) / mcmc::kImHistThreads), (unsigned)a->n_hist),
                       dim3(mcmc::kImHistThreads), 0, st, *a);
    return hipGetLastError();
}

extern "C" hipError_t mcmc_hip_launch_importance_hist(const mcmc::ImHistArgs* a, int lds_words, hipStream_t st)
{
    if (a->W <= 0 || a->n_hist <= 0 || a->n_entries <= 0 || a->n_slices <= 0) return hipSuccess;
    if (a->n_hist > mcmc::kImMaxAlt || a->slice < 1 || a->slice > mcmc::kImHistMaxSlice ||
        (long long)a->slice * a->n_slices < a->W || lds_words < 2 ||
        lds_words > 1 + mcmc::kMargMaxBins2 * mcmc::kMargMaxBins2)
        return hipErrorInvalidValue;
    const size_t lds = sizeof(unsigned long long) * (size_t)lds_words;
    hipLaunchKernelGGL(mcmc::importance_hist_kernel, dim3((unsigned)(a->n_entries * a->n_slices), (unsigned)a->n_hist),
                       dim3(mcmc::kImHistThreads), lds, st, *a);
    return hipGetLastError();
}
